"""
The phase-guided Griffin-Lim start on the device (include/rfx.h: rfx_guided_call_options; csrc/rfx_guide.hip stages the guide, the
first launch of the call analyses it): every row starts from angles0 = G / |G|, G the STFT of its guide cut or zero-padded to the
output length, instead of random phases.

Parity is against the oracle's griffinlim(S, p, angles0=G / (G.abs() + 1e-16), n_iter).  No SNR floor is fixed in advance: where
|G| is near rounding noise the direction of G is ill conditioned in the oracle's float32 as much as on the device.  Each case
computes the oracle in float64 and in float32 in the same run and requires the device's SNR against the float64 result to be no
more than 6 dB (a factor of two in amplitude) below the float32 oracle's.  Figures of one run: profiles/guided_decode.txt.
Targets are |STFT| of helpers.synthetic_wave, guides a synthetic_wave of another seed: broadband, no digital silence.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from engines import B, CLIP2, ENGINES_BY_FORM as ENGINES, T, bits as _bits, plan_for as _plan, stft64 as _stft64
from helpers import oracle, snr_db, synthetic_tiles_u8, synthetic_wave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    return oracle()


_CASES = {}


def _case(O, name):
    """(params, plan, op, target magnitudes, their slots on the device, guide): computed once per engine, never modified"""
    if name not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        L = p.hop_length * (T - 1) + (p.n_fft & 1)
        mag = O.stft_complex(synthetic_wave(B, L, seed=101), op).abs()
        guide = synthetic_wave(B, L, seed=202)
        assert mag.shape == (B, op.n_stft, T)
        _CASES[name] = (p, plan, op, mag, plan.pack_magnitudes(mag.cuda()), guide)
    return _CASES[name]


# ---- parity with the oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [0, 1, 4])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_guided_start_matches_the_oracle(O, name, n_iter):
    p, plan, op, mag, S, guide = _case(O, name)
    G32, G64 = O.stft_complex(guide, op), _stft64(guide, op, O)
    want32 = O.griffinlim(mag, op, angles0=G32 / (G32.abs() + 1e-16), n_iter=n_iter)
    want64 = O.griffinlim(mag, op, angles0=G64 / (G64.abs() + 1e-16), n_iter=n_iter, dtype=torch.float64)
    got = plan.griffinlim(S, B, T, n_iter, 0.99, guide=guide.cuda()).cpu()
    assert got.shape == want32.shape and bool(torch.isfinite(got).all())
    dev, o32, both = snr_db(want64, got), snr_db(want64, want32), snr_db(want32, got)
    print(f"guided griffinlim {name} n_iter={n_iter}: device vs float64 oracle {dev:.1f} dB, float32 oracle vs float64 oracle {o32:.1f} dB, "
          f"device vs float32 oracle {both:.1f} dB")
    assert dev >= o32 - 6.0


# ---- bytes -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["specialised-runs", "specialised-frames", "row-family-48k", "generic-11025"])
def test_a_guided_row_depends_on_nothing_but_its_magnitudes_and_its_guide(O, name):
    p, plan, op, mag, S, guide = _case(O, name)
    L = guide.shape[1]
    g = guide.cuda()
    n_iter = 2
    base = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, seed=1)
    assert float(base.abs().max()) > 0 and bool(torch.isfinite(base).all())
    unguided = plan.griffinlim(S, B, T, n_iter, 0.99, seed=1)
    assert _bits(unguided) != _bits(base)
    # repeated, another seed, another row_base
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, seed=1)) == _bits(base)
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, seed=99)) == _bits(base)
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, seed=1, row_base=7)) == _bits(base)
    # row 1 alone
    S1 = plan.pack_magnitudes(mag[1:2].cuda())
    assert _bits(plan.griffinlim(S1, 1, T, n_iter, 0.99, guide=g[1:2])) == _bits(base[1])
    # scale of the guide
    for n in (5, -7):
        assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=torch.ldexp(g, torch.tensor(n, device="cuda")))) == _bits(base), n
    # rows of a strided guide tensor (a view of wider rows) and a guide off 16-byte alignment
    wide = torch.zeros(B, L + 7, device="cuda")
    wide[:, 3:3 + L] = g
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=wide[:, 3:3 + L])) == _bits(base)
    # fit: a short guide is the zero-padded one, a long guide the truncated one
    short = g[:, :L - 100].contiguous()
    padded = torch.cat([short, torch.zeros(B, 100, device="cuda")], dim=1)
    fit_short = plan.griffinlim(S, B, T, n_iter, 0.99, guide=short)
    assert _bits(fit_short) == _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=padded)) != _bits(base)
    long_ = torch.cat([g, torch.full((B, 100), 1e9, device="cuda")], dim=1)
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=long_)) == _bits(base)
    # digital silence: a silent row gives a silent row, its neighbours are untouched
    quiet = g.clone()
    quiet[1] = 0
    out = plan.griffinlim(S, B, T, n_iter, 0.99, guide=quiet)
    assert not bool(out[1].any()) and _bits(out[0]) == _bits(base[0]) and _bits(out[2]) == _bits(base[2])


@pytest.mark.parametrize("name", ["specialised-runs", "specialised-frames", "generic-11025"])
def test_a_null_guide_in_the_grown_struct_is_the_unguided_call(O, name):
    from riffusion import _hip

    p, plan, op, mag, S, guide = _case(O, name)
    lib, L = plan.lib, guide.shape[1]
    need = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = _hip.current_stream(torch.device("cuda"))
    plain, grown = torch.empty(B, L, device="cuda"), torch.empty(B, L, device="cuda")
    assert lib.rfx_griffinlim(plan.handle, S.data_ptr(), None, 5, B, T, 2, 0.99, plain.data_ptr(), ws.data_ptr(), need, stream) == 0
    opt = _hip.RfxGuidedCallOptions(ctypes.sizeof(_hip.RfxGuidedCallOptions), 0, 0, 0.0, 0.0, None, 0, 0, 0)
    assert lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 2, 0.99, grown.data_ptr(), ws.data_ptr(), need, stream, ctypes.byref(opt), None) == 0
    assert _bits(plain) == _bits(grown) and float(plain.abs().max()) > 0
    # the per-launch times of a guided call: n_iter + 1 entries, as before
    ms = (ctypes.c_float * 4)(-1, -1, -1, -7)
    plan.griffinlim(S, B, T, 2, 0.99, guide=guide.cuda(), launch_ms=ms)
    assert all(ms[i] > 0 for i in range(3)) and ms[3] == -7


def test_guided_rows_past_65535(O):
    """the staging kernels take the row on grid y, 65 535 rows per launch: 65 543 rows in one call equal the boundary rows alone
    (chirp-z geometry 1009: the smallest frames; T = 7 is the fewest frames whose L = 601 exceeds the reflect padding of 504)"""
    p, plan = _plan("chirp-z-1009")
    rows, Tn = 65543, 7
    L = p.hop_length * (Tn - 1) + 1
    gen = torch.Generator(device="cuda").manual_seed(17)
    S = torch.rand((rows * Tn, plan.frame_stride), device="cuda", generator=gen) * 1000.0
    guide = torch.randn((rows, L), device="cuda", generator=gen) * 8000.0
    whole = plan.griffinlim(S, rows, Tn, 1, 0.99, guide=guide)
    assert whole.shape == (rows, L) and bool(torch.isfinite(whole).all())
    for r in (0, 65534, 65535, 65536, rows - 1):
        alone = plan.griffinlim(S[r * Tn:(r + 1) * Tn], 1, Tn, 1, 0.99, guide=guide[r:r + 1])
        assert float(alone.abs().max()) > 0 and _bits(alone) == _bits(whole[r:r + 1]), r


# ---- fused equals staged -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lstsq", [False, True], ids=["sgd", "lstsq"])
def test_fused_guided_call_equals_its_parts(golden_dir, lstsq):
    from PIL import Image

    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    p = SpectrogramParams(stereo=True)
    plan = _hip.get_plan(p, "cuda")
    tile = np.array(Image.open(os.path.join(golden_dir, CLIP2 + "_stereo.png")).convert("RGB"))
    N, C, W, n_iter, seed = 2, 2, 33, 3, 40
    tiles = torch.from_numpy(np.stack([tile[:, 0:W], tile[:, 200:200 + W]])).cuda()
    L = p.hop_length * (W - 1)
    guide = synthetic_wave(N * C, L + 50, seed=303).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, True, lut)
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, C, seed=seed)
    wave = plan.griffinlim(lin, N * C, W, n_iter, 0.99, seed=seed + 1, guide=guide)
    pcm3, peak3 = plan.pcm16(wave, channels=C, normalize=True)
    assert _bits(plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide)) == _bits(wave)
    pcm1, peak1 = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide)
    assert pcm1.shape == (N, L, C) and _bits(pcm1) == _bits(pcm3) and _bits(peak1) == _bits(peak3)
    unguided, _ = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq)
    assert _bits(unguided) != _bits(pcm1) and int(pcm1.abs().max()) > 30000


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(O):
    """every refusal is RFX_ERR_INVALID and leaves the output buffer as it was"""
    from riffusion import _hip

    p, plan, op, mag, S, guide = _case(O, "specialised-frames")
    lib, L = plan.lib, guide.shape[1]
    g = guide.cuda()
    need = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = _hip.current_stream(torch.device("cuda"))
    out = torch.full((B, L), 123.0, device="cuda")
    angles = torch.zeros(B * T * plan.frame_stride, dtype=torch.complex64, device="cuda")
    size = ctypes.sizeof(_hip.RfxGuidedCallOptions)

    def call(opt, Tc=T, n_iter=2, angles0=None):
        rc = lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), angles0, 5, B, Tc, n_iter, 0.99, out.data_ptr(), ws.data_ptr(), need, stream,
                                   ctypes.byref(opt), None)
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        return rc, lib.rfx_last_error()

    ok = dict(d_guide=g.data_ptr(), stride=L, samples=L)

    def opt(d_guide, stride, samples, reserved=0.0):
        return _hip.RfxGuidedCallOptions(size, 0, 0, 0.0, reserved, d_guide, stride, samples, 0)

    rc, why = call(opt(**ok), angles0=angles.data_ptr())
    assert rc == -1 and b"two starts" in why
    rc, why = call(opt(g.data_ptr(), L, 0))
    assert rc == -1 and b"guide_samples" in why
    rc, why = call(opt(g.data_ptr(), L - 1, L))
    assert rc == -1 and b"guide_stride" in why
    rc, why = call(opt(**ok), Tc=21, n_iter=0)
    assert rc == -1 and b"Padding size should be less than" in why
    rc, why = call(opt(**ok, reserved=1.0))
    assert rc == -1 and b"reserved" in why
    # rfx_inverse_mel_ex takes no guide
    mel = torch.ones(1, plan.n_mels, T, device="cuda")
    slots = torch.full((T * plan.frame_stride,), 123.0, device="cuda")
    need_i = lib.rfx_inverse_mel_workspace_bytes(plan.handle, 1, T)
    ws_i = torch.empty(need_i, dtype=torch.uint8, device="cuda")
    o = opt(**ok)
    assert lib.rfx_inverse_mel_ex(plan.handle, mel.data_ptr(), 1, T, 1, None, 0, slots.data_ptr(), ws_i.data_ptr(), need_i, stream, ctypes.byref(o)) == -1
    assert b"takes no guide" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((slots == 123.0).all())
    # the fused calls refuse a short tile before the SGD runs
    with pytest.raises(_hip.RfxError, match="Padding size"):
        plan.waveform_from_mel(torch.ones(1, plan.n_mels, 21, device="cuda"), 1, 0, guide=g[:1])


# ---- the product entry points -------------------------------------------------------------------------------------------------------------

def _conv(stereo, iters=32):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, num_griffin_lim_iters=iters), device="cuda")


def test_product_guided_decode_depends_on_neither_chunking_nor_seed():
    conv = _conv(True)
    N, W = 5, 40
    L = conv.p.hop_length * (W - 1)
    tiles = synthetic_tiles_u8(N, 512, W, seed=8)
    guides = synthetic_wave(N * 2, L + 30, seed=9).reshape(N, 2, L + 30)

    def decode(g, **kw):
        kw.setdefault("seed", 3)
        return conv.audio_from_spectrogram_images(tiles, guide_waveforms=g, griffin_lim_iters=2, inverse_mel="lstsq", **kw)

    # (the closed-form InverseMelScale: with the SGD its random start still follows the seed, Griffin-Lim's does not)
    whole = decode(guides, tiles_per_call=64)
    assert whole.shape == (N, L, 2) and whole.dtype == np.int16 and np.abs(whole.astype(np.int32)).max() > 30000
    assert np.array_equal(decode(guides, tiles_per_call=2), whole)
    assert np.array_equal(decode(guides, tiles_per_call=64, seed=4), whole)
    assert not np.array_equal(decode(None, tiles_per_call=64), whole)
    # with the SGD: chunking-free as well, same seed
    sgd = conv.audio_from_spectrogram_images(tiles, guide_waveforms=guides, griffin_lim_iters=2, seed=3, tiles_per_call=64)
    assert np.array_equal(conv.audio_from_spectrogram_images(tiles, guide_waveforms=guides, griffin_lim_iters=2, seed=3, tiles_per_call=2), sgd)
    # a mono guide serves both channels; int16 guides are their float values; arrays and device tensors are taken alike
    mono = guides[:, :1]
    assert np.array_equal(decode(mono), decode(mono.repeat(1, 2, 1)))
    as_int = guides.to(torch.int16)
    assert np.array_equal(decode(as_int.numpy()), decode(as_int.float().cuda()))
    # float waveforms, the filters and the error report take the guide too
    wave = decode(guides, return_waveform=True)
    assert wave.shape == (N, 2, L) and np.isfinite(wave).all()
    pcm, err = decode(guides, return_error=True)
    assert np.array_equal(pcm, whole) and err.shape == (N,)
    filtered = decode(guides, apply_filters=True)
    assert filtered.shape == whole.shape and not np.array_equal(filtered, whole)
    for bad in (guides[:4], guides.double(), guides[:, :, 0]):
        with pytest.raises(ValueError):
            decode(bad)


def test_griffin_lim_iters_overrides_the_params():
    tiles = synthetic_tiles_u8(2, 512, 30, seed=10)
    got = _conv(False).audio_from_spectrogram_images(tiles, seed=6, griffin_lim_iters=3)
    want = _conv(False, iters=3).audio_from_spectrogram_images(tiles, seed=6)
    assert np.array_equal(got, want) and not np.array_equal(got, _conv(False).audio_from_spectrogram_images(tiles, seed=6))
    with pytest.raises(ValueError):
        _conv(False).audio_from_spectrogram_images(tiles, seed=6, griffin_lim_iters=-1)


def test_torch_seam_takes_a_guide_and_refuses_two_starts():
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(num_griffin_lim_iters=2), device="cuda")
    plan = conv._plan()
    Tn = 30
    mel = torch.rand(2, plan.n_mels, Tn, generator=torch.Generator().manual_seed(2)) * 1e6
    guide = synthetic_wave(2, conv.p.hop_length * (Tn - 1), seed=12)
    got = conv.waveform_from_mel_amplitudes(mel, seed=8, guide=guide)  # host tensors: the converter moves them
    want = plan.waveform_from_mel(mel.cuda(), 2, 2, 0.99, seed=8, guide=guide.cuda())
    assert _bits(got) == _bits(want) != _bits(conv.waveform_from_mel_amplitudes(mel, seed=8))
    with pytest.raises(ValueError, match="two starts"):
        conv.waveform_from_mel_amplitudes(mel, guide=guide, angles0=torch.ones(2, plan.n_stft, Tn, dtype=torch.complex64))


def _golden_clip2(golden_dir):
    from PIL import Image

    from riffusion.util import audio_util

    image = Image.open(os.path.join(golden_dir, CLIP2 + "_stereo.png"))
    segment = audio_util.PcmSegment.from_wav(os.path.join(golden_dir, CLIP2 + ".wav"))
    return image, segment


def test_the_source_clip_as_guide_halves_the_error_at_four_iterations(golden_dir):
    """the golden stereo tile of clip 2, its recording as the guide: on the oracle the guided start at 4 iterations measures a
    seventh of the random start's spectral convergence (tests/test_guided_start_cpu.py); the condition is half"""
    from riffusion.util import image_util

    image, segment = _golden_clip2(golden_dir)
    conv = _conv(True)
    tile = np.asarray(image_util.rgb_array_from_image(image))[None]
    guide = np.asarray(segment.get_array_of_samples(), dtype=np.int16).reshape(-1, 2).T[None]
    _, guided = conv.audio_from_spectrogram_images(tile, seed=1, guide_waveforms=np.ascontiguousarray(guide), griffin_lim_iters=4, return_error=True)
    _, random = conv.audio_from_spectrogram_images(tile, seed=1, griffin_lim_iters=4, return_error=True)
    print(f"golden stereo tile of clip 2, 4 iterations: guided spectral convergence {guided[0]:.4f}, random start {random[0]:.4f}")
    assert guided[0] < 0.5 * random[0]


def test_single_tile_api_and_cli_take_a_guide(golden_dir, tmp_path):
    from riffusion import cli
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.util import audio_util

    image, _ = _golden_clip2(golden_dir)
    wav = os.path.join(golden_dir, CLIP2 + ".wav")
    out = str(tmp_path / "guided.wav")
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", os.path.join(golden_dir, CLIP2 + "_stereo.png"), "--audio", out, "--guide-audio", wav,
              "--griffin-lim-iters", "2"])
    written = audio_util.PcmSegment.from_wav(out)
    conv = SpectrogramImageConverter(cli._params_from_image(image), device="cuda")
    torch.manual_seed(5)
    want = conv.audio_from_spectrogram_image(image, guide_segment=cli._load_segment(wav), griffin_lim_iters=2)
    assert written.channels == 2 and written.frame_rate == 44100
    assert np.array_equal(np.asarray(written.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    torch.manual_seed(5)
    plain = conv.audio_from_spectrogram_image(image, griffin_lim_iters=2)
    assert not np.array_equal(np.asarray(plain.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    # a guide at another rate is refused; a mono guide serves the stereo tile
    with pytest.raises(ValueError, match="Hz"):
        conv.audio_from_spectrogram_image(image, guide_segment=audio_util.PcmSegment(np.zeros((1000, 2), np.int16), 22050))
    mono = conv.audio_from_spectrogram_image(image, guide_segment=cli._load_segment(wav).set_channels(1), griffin_lim_iters=0)
    assert mono.channels == 2
