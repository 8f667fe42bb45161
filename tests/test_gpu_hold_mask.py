"""
Masked calls on the device (include/rfx.h: rfx_masked_call_options): a guided Griffin-Lim call keeps chosen BINS of chosen frames at
the guide's phase through every iteration.  The device applies the hold through its linearity (csrc/rfx_holdmask_core.h): the
iterations run on magnitudes that are zero in the held bins and a constant audio buffer c = ISTFT(S_held a0) is added to every
generation as it is folded.

Parity is against tests/mask_oracle.py.  The device's SNR against the float64 `where` oracle must be at least the smaller of the two
float32 oracles' SNRs (`where` form and split form: in float32 they round differently) minus the project's 6 dB margin of
tests/test_gpu_held_frames.py.  The four exact consequences of the definition are checked per engine:
  n_iter == 0              the guided call's bytes, whatever the mask
  an all-zero mask row     equals the guided call's row at the same n_iter, on the same form (==: the + c turns -0.0 into +0.0)
  an all-ones mask row     equals the guided call's row at n_iter == 0, whatever n_iter is (==)
  a row depends on its magnitudes, its guide row and its mask row alone: bit for bit
Shapes, engines, targets and guides are those of tests/test_gpu_held_frames.py: B = 3 rows of T = 33 frames.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import mask_oracle
from engines import B, CLIP2, ENGINES_BY_FORM as ENGINES, T, bits as _bits, plan_for as _plan, stft64 as _stft64
from helpers import oracle, snr_db, synthetic_tiles_u8, synthetic_wave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    return oracle()


def _held(n_stft, frames=T):
    """(3, n_stft, frames) bool: row 0 nothing; row 1 the bins [0, n_stft / 3 + 5) of every frame, every 8th frame entirely and bin
    n_stft - 1; row 2 everything"""
    held = np.zeros((3, n_stft, frames), dtype=bool)
    held[1, :n_stft // 3 + 5, :] = True
    held[1, :, ::8] = True
    held[1, n_stft - 1, :] = True
    held[2] = True
    return held


def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words)).cuda()


def _same(a, b):
    """equal as values (== : -0.0 and +0.0 are the same sample), finite"""
    return a.shape == b.shape and bool(torch.isfinite(a).all()) and bool((a == b).all())


_CASES = {}


def _case(O, name):
    """(params, plan, op, target magnitudes, their slots, guide, guide on the device, the guided call's results at n_iter 0 and 4 on
    the form a masked call takes, held (B, n_stft, T) bool, its bit mask on the device): computed once per engine, never modified"""
    if name not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        L = p.hop_length * (T - 1) + (p.n_fft & 1)
        mag = O.stft_complex(synthetic_wave(B, L, seed=101), op).abs()
        guide = synthetic_wave(B, L, seed=202)
        S, g = plan.pack_magnitudes(mag.cuda()), guide.cuda()
        guided = {n: plan.griffinlim(S, B, T, n, 0.99, guide=g) for n in (0, 4)}
        held = _held(op.n_stft)
        _CASES[name] = (p, plan, op, mag, S, guide, g, guided, held, _dev(mask_oracle.pack_bits(held)))
    return _CASES[name]


# ---- parity with the masked oracle ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [1, 4])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_masked_call_matches_the_oracle(O, name, n_iter):
    p, plan, op, mag, S, guide, g, _, held, bits = _case(O, name)
    G32, G64 = O.stft_complex(guide, op), _stft64(guide, op, O)
    a32, a64 = G32 / (G32.abs() + 1e-16), G64 / (G64.abs() + 1e-16)
    want64 = mask_oracle.masked_griffinlim(O, mag, op, a64, held, n_iter, dtype=torch.float64)
    where32 = mask_oracle.masked_griffinlim(O, mag, op, a32, held, n_iter)
    split32 = mask_oracle.masked_griffinlim(O, mag, op, a32, held, n_iter, split=True)
    got = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold_bins=bits).cpu()
    assert got.shape == want64.shape and bool(torch.isfinite(got).all())
    dev, w32, s32 = snr_db(want64, got), snr_db(want64, where32), snr_db(want64, split32)
    print(f"masked griffinlim {name} n_iter={n_iter}: device vs float64 oracle {dev:.1f} dB, float32 where-form oracle {w32:.1f} dB, "
          f"float32 split-form oracle {s32:.1f} dB")
    assert dev >= min(w32, s32) - 6.0


# ---- the four exact consequences --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENGINES))
def test_exact_consequences_of_the_mask(O, name):
    from riffusion import _hip

    p, plan, op, mag, S, guide, g, guided, held, bits = _case(O, name)
    assert float(guided[4].abs().max()) > 0 and _bits(guided[4]) != _bits(guided[0])
    # n_iter == 0: the guided call's bytes, whatever the mask
    assert _bits(plan.griffinlim(S, B, T, 0, 0.99, guide=g, hold_bins=bits)) == _bits(guided[0])
    out = plan.griffinlim(S, B, T, 4, 0.99, guide=g, hold_bins=bits)
    # an all-zero row: the guided call's row at the same n_iter on the same form (the masked call takes the per-frame form; on the
    # specialised engine both forms give a clip the same bits)
    assert _same(out[0], guided[4][0])
    # an all-ones row: the guided call's row at n_iter == 0
    assert _same(out[2], guided[0][2])
    assert not _same(out[1], guided[4][1]) and not _same(out[1], guided[0][1])
    # garbage in the unused bits of the last word changes nothing
    valid = op.n_stft - 32 * (plan.hold_mask_words - 1)
    assert 0 < valid < 32
    dirty = bits.clone()
    dirty[:, :, -1] |= torch.tensor(np.uint32((0xFFFFFFFF << valid) & 0xFFFFFFFF).astype(np.int32).item(), dtype=torch.int32, device="cuda")
    assert _bits(dirty) != _bits(bits)
    assert _bits(plan.griffinlim(S, B, T, 4, 0.99, guide=g, hold_bins=dirty)) == _bits(out)
    # a NULL d_hold_bins in the grown struct is the guided call, within the guided call's workspace
    lib, L = plan.lib, g.shape[1]
    need = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    raw = torch.empty(B, L, device="cuda")
    opt = _hip.RfxMaskedCallOptions(ctypes.sizeof(_hip.RfxMaskedCallOptions), 0, 0, 0.0, 0.0, g.data_ptr(), L, L, 0, None, 0, None, 0, 0)
    assert lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 4, 0.99, raw.data_ptr(), ws.data_ptr(), need,
                                 _hip.current_stream(torch.device("cuda")), ctypes.byref(opt), None) == 0
    assert _bits(raw) == _bits(guided[4])


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_a_masked_row_depends_on_nothing_but_its_magnitudes_its_guide_and_its_mask(O, name):
    p, plan, op, mag, S, guide, g, _, held, bits = _case(O, name)
    n_iter = 3
    base = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold_bins=bits, seed=1)
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold_bins=bits, seed=1)) == _bits(base)
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold_bins=bits, seed=99, row_base=7)) == _bits(base)
    # the other rows' masks
    other = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold_bins=bits[[2, 1, 0]].contiguous())
    assert _bits(other[1]) == _bits(base[1]) and _bits(other[0]) != _bits(base[0])
    # row 1 alone, and the batch reversed
    alone = plan.griffinlim(S.reshape(B, -1)[1:2].reshape(-1).contiguous(), 1, T, n_iter, 0.99, guide=g[1:2], hold_bins=bits[1:2].contiguous())
    assert _bits(alone) == _bits(base[1:2])
    rev = plan.griffinlim(plan.pack_magnitudes(mag.flip(0).cuda()), B, T, n_iter, 0.99, guide=g.flip(0).contiguous(), hold_bins=bits.flip(0).contiguous())
    assert _bits(rev.flip(0)) == _bits(base)


# ---- band to bin ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["specialised-frames", "generic-11025"])
def test_band_mask_expands_as_the_cpu_statement(O, name):
    from riffusion import _hip

    p, plan = _plan(name)
    lo, hi = mask_oracle.bin_bands(plan.melfb.numpy())
    dlo, dhi = _hip.bin_bands(plan._cparams, plan.melfb)
    assert np.array_equal(lo, dlo) and np.array_equal(hi, dhi)
    rng = np.random.default_rng(5)
    bands = rng.random((B, plan.n_mels, T)) < 0.8
    bands[1] = True   # one row all held
    bands[2] = False  # one row none held
    want = mask_oracle.bins_from_bands(bands, lo, hi)
    assert want[1][lo >= 0].all() and not want[1][lo < 0].any() and not want[2].any() and 0 < want[0].sum() < want[1].sum()
    for given in (torch.from_numpy(bands).cuda(), torch.from_numpy(bands.astype(np.uint8) * 7).cuda()):
        got = plan.hold_bins_from_bands(given)
        assert got.shape == (B, T, plan.hold_mask_words) and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), mask_oracle.pack_bits(want))  # every bit, the unused tail bits 0


# ---- large batches -----------------------------------------------------------------------------------------------------------------------------

def test_masked_rows_past_65535():
    """65 543 rows in one call equal the boundary rows alone: the split's and the staging's 65 535 rows per launch (chirp-z geometry
    1009: the smallest frames; T = 7 is the fewest frames whose L = 601 exceeds the reflect padding of 504)"""
    p, plan = _plan("chirp-z-1009")
    rows, Tn = 65543, 7
    L = p.hop_length * (Tn - 1) + 1
    gen = torch.Generator(device="cuda").manual_seed(17)
    S = torch.rand((rows * Tn, plan.frame_stride), device="cuda", generator=gen) * 1000.0
    guide = torch.randn((rows, L), device="cuda", generator=gen) * 8000.0
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, Tn, plan.hold_mask_words), device="cuda", generator=gen, dtype=torch.int64).to(torch.int32)
    bits[100] = 0
    bits[65535] = -1
    whole = plan.griffinlim(S, rows, Tn, 2, 0.99, guide=guide, hold_bins=bits)
    assert whole.shape == (rows, L) and bool(torch.isfinite(whole).all())
    for r in (0, 100, 65534, 65535, 65536, rows - 1):
        alone = plan.griffinlim(S[r * Tn:(r + 1) * Tn], 1, Tn, 2, 0.99, guide=guide[r:r + 1], hold_bins=bits[r:r + 1].contiguous())
        assert float(alone.abs().max()) > 0 and _bits(alone) == _bits(whole[r:r + 1]), r


# ---- workspace, timings, refusals ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENGINES))
def test_masked_workspace_queries_and_launch_times(O, name):
    p, plan, op, mag, S, guide, g, _, held, bits = _case(O, name)
    lib = plan.lib
    plain, masked = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T), helpers.need(lib, "griffinlim", plan.handle, B, T, **helpers.MASKED)
    L = g.shape[1]
    assert masked >= plain + 4 * (B * T * op.n_stft + B * L)  # X and c
    if name == "specialised-runs":  # the frame buffer of the per-frame form on top
        assert masked == helpers.need(lib, "griffinlim", _plan("specialised-frames")[1].handle, B, T, **helpers.MASKED) > plain + B * T * 4410 * 4
    assert helpers.need(lib, "waveform_from_mel", plan.handle, B, T, **helpers.MASKED) >= lib.rfx_waveform_from_mel_workspace_bytes(plan.handle, B, T)
    assert helpers.need(lib, "audio_from_image", plan.handle, B, 0, T, **helpers.MASKED) >= lib.rfx_audio_from_image_workspace_bytes(plan.handle, B, 0, T)
    assert lib.rfx_hold_mask_words(plan.handle) == (op.n_stft + 31) // 32 == plan.hold_mask_words
    ms = (ctypes.c_float * 4)(-1, -1, -1, -7)
    plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold_bins=bits, launch_ms=ms)
    assert all(ms[i] > 0 for i in range(3)) and ms[3] == -7


@pytest.mark.parametrize("name", ["specialised-runs", "specialised-frames", "generic-11025"])
def test_refusals_launch_nothing(O, name):
    """every refusal comes before any launch and leaves the output buffer as it was"""
    from riffusion import _hip

    p, plan, op, mag, S, guide, g, _, held, bits = _case(O, name)
    lib, L = plan.lib, g.shape[1]
    plain, masked = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T), helpers.need(lib, "griffinlim", plan.handle, B, T, **helpers.MASKED)
    ws = torch.empty(masked + 16, dtype=torch.uint8, device="cuda")
    stream = _hip.current_stream(torch.device("cuda"))
    out = torch.full((B, L), 123.0, device="cuda")
    pairs = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    words = plan.hold_mask_words
    size = ctypes.sizeof(_hip.RfxMaskedCallOptions)

    def call(d_guide, d_bins, hold_words=words, reserved4=0, d_pairs=None, ws_bytes=masked, angles0=None):
        opt = _hip.RfxMaskedCallOptions(size, 0, 0, 0.0, 0.0, d_guide, L, L, 0, d_pairs, 0, d_bins, hold_words, reserved4)
        rc = lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), angles0, 5, B, T, 2, 0.99, out.data_ptr(), ws.data_ptr(), ws_bytes, stream,
                                   ctypes.byref(opt), None)
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        return rc, lib.rfx_last_error()

    rc, why = call(None, bits.data_ptr())
    assert rc == -1 and b"needs a guide" in why
    rc, why = call(g.data_ptr(), bits.data_ptr() + 2)
    assert rc == -1 and b"aligned" in why
    rc, why = call(g.data_ptr(), bits.data_ptr(), reserved4=1)
    assert rc == -1 and b"reserved4" in why
    rc, why = call(g.data_ptr(), bits.data_ptr(), hold_words=words - 1)
    assert rc == -1 and b"hold_words" in why
    rc, why = call(g.data_ptr(), bits.data_ptr(), d_pairs=pairs.data_ptr())
    assert rc == -1 and b"d_hold_frames" in why
    angles0 = torch.zeros((B * T, plan.frame_stride), dtype=torch.complex64, device="cuda")
    rc, why = call(g.data_ptr(), bits.data_ptr(), angles0=angles0.data_ptr())
    assert rc == -1 and b"two starts" in why
    rc, why = call(g.data_ptr(), bits.data_ptr(), ws_bytes=plain)
    assert rc == -3 and b"workspace too small" in why
    rc, why = call(g.data_ptr(), bits.data_ptr(), ws_bytes=masked - 1)
    assert rc == -3
    # the fused entries check the masked query too
    mel = torch.ones(B, plan.n_mels, T, device="cuda")
    need = helpers.need(lib, "waveform_from_mel", plan.handle, B, T, **helpers.MASKED)
    ws2 = torch.empty(need, dtype=torch.uint8, device="cuda")
    opt = _hip.RfxMaskedCallOptions(size, 0, 0, 0.0, 0.0, g.data_ptr(), L, L, 0, None, 0, bits.data_ptr(), words, 0)
    assert lib.rfx_waveform_from_mel_ex(plan.handle, mel.data_ptr(), B, T, 1, 0, 2, 0.99, out.data_ptr(), ws2.data_ptr(), need - 1, stream, ctypes.byref(opt)) == -3
    # rfx_inverse_mel_ex holds no bins
    slots = torch.full((T * plan.frame_stride,), 123.0, device="cuda")
    need_i = lib.rfx_inverse_mel_workspace_bytes(plan.handle, 1, T)
    ws_i = torch.empty(need_i, dtype=torch.uint8, device="cuda")
    opt = _hip.RfxMaskedCallOptions(size, 0, 0, 0.0, 0.0, None, 0, 0, 0, None, 0, bits.data_ptr(), words, 0)
    assert lib.rfx_inverse_mel_ex(plan.handle, mel.data_ptr(), 1, T, 1, None, 0, slots.data_ptr(), ws_i.data_ptr(), need_i, stream, ctypes.byref(opt)) == -1
    assert b"holds no bins" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and bool((slots == 123.0).all())
    # the Python layer: no guide, held frames as well, a wrong shape, type or device
    with pytest.raises(ValueError, match="needs a guide"):
        plan.griffinlim(S, B, T, 2, 0.99, hold_bins=bits)
    with pytest.raises(ValueError, match="together with hold"):
        plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold=pairs, hold_bins=bits)
    for bad in (bits[:2], bits[:, :, :-1], bits.long(), bits.cpu()):
        with pytest.raises(ValueError):
            plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold_bins=bad)


# ---- fused equals staged ---------------------------------------------------------------------------------------------------------------------

def _tile_bands(n_mels, W):
    """a (n_mels, W) bool band mask in spectrogram orientation: the low two thirds of the bands, and every 8th frame entirely"""
    bands = np.zeros((n_mels, W), dtype=bool)
    bands[:2 * n_mels // 3] = True
    bands[:, ::8] = True
    return bands


@pytest.mark.parametrize("lstsq", [False, True], ids=["sgd", "lstsq"])
def test_fused_masked_call_equals_its_parts(golden_dir, lstsq):
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
    bands = np.stack([_tile_bands(plan.n_mels, W)] * (N * C))
    bands[2:] = bands[2:, ::-1]  # the second clip keeps the high bands
    bits = plan.hold_bins_from_bands(torch.from_numpy(np.ascontiguousarray(bands)).cuda())
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, True, lut)
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, C, seed=seed)
    wave = plan.griffinlim(lin, N * C, W, n_iter, 0.99, seed=seed + 1, guide=guide, hold_bins=bits)
    pcm3, peak3 = plan.pcm16(wave, channels=C, normalize=True)
    assert _bits(plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide, hold_bins=bits)) == _bits(wave)
    pcm1, peak1 = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide, hold_bins=bits)
    assert pcm1.shape == (N, L, C) and _bits(pcm1) == _bits(pcm3) and _bits(peak1) == _bits(peak3)
    start_only, _ = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide)
    assert _bits(start_only) != _bits(pcm1) and int(pcm1.abs().max()) > 30000


@pytest.mark.parametrize("lstsq", [False, True], ids=["sgd", "lstsq"])
def test_fused_masked_call_on_a_row_family_equals_its_parts(lstsq):
    """at 48 kHz the SGD stage of the fused call writes the magnitudes in the family's slot order: the split acts on that order"""
    p, plan = _plan("row-family-48k")
    n_iter, seed = 3, 11
    mel = torch.rand(B, plan.n_mels, T, generator=torch.Generator().manual_seed(4)).cuda() * 1e6
    g = synthetic_wave(B, p.hop_length * (T - 1), seed=202).cuda()
    bits = _dev(mask_oracle.pack_bits(_held(plan.n_stft)))
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, 1, seed=seed)
    wave = plan.griffinlim(lin, B, T, n_iter, 0.99, seed=seed + 1, guide=g, hold_bins=bits)
    assert _bits(plan.waveform_from_mel(mel, 1, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=g, hold_bins=bits)) == _bits(wave)


# ---- the product entry points ---------------------------------------------------------------------------------------------------------------

def _conv(stereo, iters=32):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, num_griffin_lim_iters=iters), device="cuda")


def test_product_masked_decode_depends_on_neither_chunking_nor_the_form_of_the_mask():
    from PIL import Image

    conv = _conv(True)
    N, W = 5, 40
    L = conv.p.hop_length * (W - 1)
    tiles = synthetic_tiles_u8(N, 512, W, seed=8)
    guides = synthetic_wave(N * 2, L + 30, seed=9).reshape(N, 2, L + 30)
    one = _tile_bands(512, W)
    per_clip = np.stack([one, np.zeros_like(one), np.ones_like(one), one[::-1], one])

    def decode(mask, **kw):
        return conv.audio_from_spectrogram_images(tiles, guide_waveforms=guides, griffin_lim_iters=3, inverse_mel="lstsq", seed=3, hold_mask=mask, **kw)

    whole = decode(per_clip, tiles_per_call=64)
    assert whole.shape == (N, L, 2) and whole.dtype == np.int16
    assert np.array_equal(decode(per_clip, tiles_per_call=1), whole)
    assert np.array_equal(decode(torch.from_numpy(per_clip).cuda(), tiles_per_call=2), whole)
    start_only, start = decode(None), conv.audio_from_spectrogram_images(tiles, guide_waveforms=guides, griffin_lim_iters=0, inverse_mel="lstsq", seed=3)
    assert np.array_equal(whole[1], start_only[1]) and np.array_equal(whole[2], start[2])  # nothing held, everything held
    assert not np.array_equal(whole[0], start_only[0]) and not np.array_equal(whole[0], start[0])
    # one mask for all clips: as an (n_mels, W) array, and as a PIL image (black is kept; image rows run from the top)
    assert np.array_equal(decode(one)[0], whole[0]) and np.array_equal(decode(one)[4], whole[4])
    image = Image.fromarray(np.where(one[::-1], 0, 255).astype(np.uint8), mode="L")
    assert np.array_equal(decode(image), decode(one))
    # a stereo tile holds both channel rows: the float waveform of clip 2 (everything held) is its start, on both channels
    wave, wave0 = decode(per_clip, return_waveform=True), conv.audio_from_spectrogram_images(
        tiles, guide_waveforms=guides, griffin_lim_iters=0, inverse_mel="lstsq", seed=3, return_waveform=True)
    assert wave.shape == (N, 2, L) and np.array_equal(wave[2], wave0[2]) and not np.array_equal(wave[0, 0], wave0[0, 0]) \
        and not np.array_equal(wave[0, 1], wave0[0, 1])
    with pytest.raises(ValueError, match="guide"):
        conv.audio_from_spectrogram_images(tiles, griffin_lim_iters=3, hold_mask=one)
    with pytest.raises(ValueError, match="hold_frames"):
        decode(one, hold_frames=(3, 3))
    for bad in (per_clip[:4], one[:, :-1], one[:-1]):
        with pytest.raises(ValueError):
            decode(bad)


def test_torch_seam_takes_a_hold_mask():
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(num_griffin_lim_iters=2), device="cuda")
    plan = conv._plan()
    Tn = 30
    mel = torch.rand(2, plan.n_mels, Tn, generator=torch.Generator().manual_seed(2)) * 1e6
    guide = synthetic_wave(2, conv.p.hop_length * (Tn - 1), seed=12)
    bands = np.stack([_tile_bands(plan.n_mels, Tn)] * 2)
    got = conv.waveform_from_mel_amplitudes(mel, seed=8, guide=guide, hold_mask=bands)
    want = plan.waveform_from_mel(mel.cuda(), 2, 2, 0.99, seed=8, guide=guide.cuda(), hold_bins=plan.hold_bins_from_bands(torch.from_numpy(bands).cuda()))
    assert _bits(got) == _bits(want) != _bits(conv.waveform_from_mel_amplitudes(mel, seed=8, guide=guide))
    with pytest.raises(ValueError, match="guide"):
        conv.waveform_from_mel_amplitudes(mel, seed=8, hold_mask=bands)
    with pytest.raises(ValueError):
        conv.waveform_from_mel_amplitudes(mel, seed=8, guide=guide, hold_mask=bands[:, :, :-1])


def test_cli_hold_mask_decodes_the_golden_tile(golden_dir, tmp_path):
    from PIL import Image

    from riffusion import cli
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.util import audio_util, image_util

    png, wav = os.path.join(golden_dir, CLIP2 + "_stereo.png"), os.path.join(golden_dir, CLIP2 + ".wav")
    image = Image.open(png)
    mask = Image.open(os.path.join(golden_dir, "mask_gradient_dark.png")).resize((image.width, image.height), Image.NEAREST)
    mask_png, out = str(tmp_path / "mask.png"), str(tmp_path / "masked.wav")
    mask.save(mask_png)
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", png, "--audio", out, "--guide-audio", wav, "--griffin-lim-iters", "2", "--hold-mask", mask_png])
    written = audio_util.PcmSegment.from_wav(out)
    conv = SpectrogramImageConverter(cli._params_from_image(image), device="cuda")
    assert written.channels == 2 and written.frame_rate == 44100
    torch.manual_seed(5)
    want = conv.audio_from_spectrogram_image(image, guide_segment=cli._load_segment(wav), griffin_lim_iters=2, hold_mask=mask)
    assert np.array_equal(np.asarray(written.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    torch.manual_seed(5)
    start_only = conv.audio_from_spectrogram_image(image, guide_segment=cli._load_segment(wav), griffin_lim_iters=2)
    assert not np.array_equal(np.asarray(start_only.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    held = image_util.hold_mask_from_image(mask)
    assert held.shape == (image.height, image.width) and 0 < held.mean() < 1
    # another threshold holds other bands: other bytes
    out2 = str(tmp_path / "masked2.wav")
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", png, "--audio", out2, "--guide-audio", wav, "--griffin-lim-iters", "2", "--hold-mask", mask_png,
              "--hold-keep-threshold", "0.2"])
    assert open(out2, "rb").read() != open(out, "rb").read()
    with pytest.raises(SystemExit):
        cli.main(["image-to-audio", "--image", png, "--audio", out, "--hold-mask", mask_png])
