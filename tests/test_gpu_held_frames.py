"""
Held frames on the device (include/rfx.h: rfx_held_call_options): a guided Griffin-Lim call keeps the first `head` and the last
`tail` frames of a row at the guide's phase through every iteration.  Launch 0 is the guided call's; launches 1 .. n_iter walk the
list of the free frames (csrc/rfx_guide.hip compacts it) and leave the held frames' synthesis frames as launch 0 wrote them.

Parity is against tests/held_oracle.py - the oracle's Griffin-Lim loop with `angles[..., held] = a0[..., held]` after the projection -
by the rule of tests/test_gpu_guided_start.py, unchanged: each case computes the oracle in float64 and in float32 in the same run and
requires the device's SNR against the float64 result to be no more than 6 dB below the float32 oracle's.  The three exact
consequences of the definition are checked on bytes, on every engine:
  (0, 0) for a row        the bytes of the guided call
  head + tail >= T        the bytes of the guided call with n_iter = 0, whatever n_iter is
  held-only samples       (every frame whose window reaches them is held) the bytes they have at n_iter = 0
Shapes, engines, targets and guides are those of tests/test_gpu_guided_start.py: B = 3 rows of T = 33 frames.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import held_oracle
import helpers
from engines import B, CLIP2, ENGINES_BY_FORM as ENGINES, T, bits as _bits, plan_for as _plan, stft64 as _stft64
from helpers import oracle, snr_db, synthetic_tiles_u8, synthetic_wave

pytestmark = pytest.mark.gpu

HOLDS = [(0, 0), (7, 3), (33, 0)]      # nothing held, both ends held, everything held
SPANS = [(12, 11), (7, 3), (0, 9)]     # rows with held-only samples at both ends, at the head, at the tail
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def O():
    return oracle()


def _hold(pairs):
    return torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)


_CASES = {}


def _case(O, name):
    """(params, plan, op, target magnitudes, their slots on the device, guide on the device, the guided call's results at n_iter 0
    and 4): computed once per engine, never modified"""
    if name not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        L = p.hop_length * (T - 1) + (p.n_fft & 1)
        mag = O.stft_complex(synthetic_wave(B, L, seed=101), op).abs()
        guide = synthetic_wave(B, L, seed=202)
        assert mag.shape == (B, op.n_stft, T)
        S, g = plan.pack_magnitudes(mag.cuda()), guide.cuda()
        guided = {n: plan.griffinlim(S, B, T, n, 0.99, guide=g) for n in (0, 4)}
        _CASES[name] = (p, plan, op, mag, S, guide, g, guided)
    return _CASES[name]


# ---- parity with the held oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [1, 4])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_held_frames_match_the_oracle(O, name, n_iter):
    p, plan, op, mag, S, guide, g, _ = _case(O, name)
    G32, G64 = O.stft_complex(guide, op), _stft64(guide, op, O)
    want32 = held_oracle.held_griffinlim(O, mag, op, G32 / (G32.abs() + 1e-16), HOLDS, n_iter)
    want64 = held_oracle.held_griffinlim(O, mag, op, G64 / (G64.abs() + 1e-16), HOLDS, n_iter, dtype=torch.float64)
    got = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold=_hold(HOLDS)).cpu()
    assert got.shape == want32.shape and bool(torch.isfinite(got).all())
    dev, o32, both = snr_db(want64, got), snr_db(want64, want32), snr_db(want32, got)
    print(f"held griffinlim {name} n_iter={n_iter}: device vs float64 oracle {dev:.1f} dB, float32 oracle vs float64 oracle {o32:.1f} dB, "
          f"device vs float32 oracle {both:.1f} dB")
    assert dev >= o32 - 6.0


# ---- bytes: the three exact consequences --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENGINES))
def test_nothing_held_is_the_guided_call(O, name):
    """(0, 0) in every row, as a zero array and as a NULL d_hold_frames in the grown struct: the guided call's bytes.  On the
    specialised engine the guided call of the runs plan takes runs and the held one frames: same bytes."""
    from riffusion import _hip

    p, plan, op, mag, S, guide, g, guided = _case(O, name)
    assert float(guided[4].abs().max()) > 0 and _bits(guided[4]) != _bits(guided[0])
    assert _bits(plan.griffinlim(S, B, T, 4, 0.99, guide=g, hold=_hold([(0, 0)] * B))) == _bits(guided[4])
    assert _bits(plan.griffinlim(S, B, T, 0, 0.99, guide=g, hold=_hold(HOLDS))) == _bits(guided[0])
    lib, L = plan.lib, g.shape[1]
    need = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)  # a NULL d_hold_frames asks for no more than the guided call
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, L, device="cuda")
    opt = _hip.RfxHeldCallOptions(ctypes.sizeof(_hip.RfxHeldCallOptions), 0, 0, 0.0, 0.0, g.data_ptr(), L, L, 0, None, 0)
    assert lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 4, 0.99, out.data_ptr(), ws.data_ptr(), need,
                                 _hip.current_stream(torch.device("cuda")), ctypes.byref(opt), None) == 0
    assert _bits(out) == _bits(guided[4])


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_a_fully_held_row_keeps_its_start_while_its_neighbours_iterate(O, name):
    p, plan, op, mag, S, guide, g, guided = _case(O, name)
    out = plan.griffinlim(S, B, T, 4, 0.99, guide=g, hold=_hold(HOLDS))
    assert _bits(out[0]) == _bits(guided[4][0])            # (0, 0)
    assert _bits(out[2]) == _bits(guided[0][2])            # (33, 0)
    assert _bits(out[1]) not in (_bits(guided[4][1]), _bits(guided[0][1]))
    for full in ((0, T), (20, 13), (T, T)):
        out = plan.griffinlim(S, B, T, 4, 0.99, guide=g, hold=_hold([(0, 0), full, (0, 0)]))
        assert _bits(out[1]) == _bits(guided[0][1]) and _bits(out[0]) == _bits(guided[4][0]) and _bits(out[2]) == _bits(guided[4][2]), full


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_held_only_samples_keep_their_start(O, name):
    p, plan, op, mag, S, guide, g, guided = _case(O, name)
    only = held_oracle.held_only_samples(SPANS, T, op).cuda()
    per_row = only.sum(dim=1).tolist()
    hop, half = op.hop_length, op.win_length // 2  # frame t's window: [hop t - half, hop t - half + win)
    end = op.win_length - half
    assert per_row == [12 * hop - half + (g.shape[1] - (21 * hop + end)), 7 * hop - half, g.shape[1] - (23 * hop + end)]
    out = plan.griffinlim(S, B, T, 4, 0.99, guide=g, hold=_hold(SPANS))
    assert _bits(out[only]) == _bits(guided[0][only])
    assert _bits(guided[4][only]) != _bits(guided[0][only])  # the start-only decode moves them
    for r in range(B):
        assert _bits(out[r][~only[r]]) != _bits(guided[0][r][~only[r]]), r


# ---- a row depends on its magnitudes, its guide and its pair ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENGINES))
def test_a_held_row_depends_on_nothing_but_its_magnitudes_its_guide_and_its_pair(O, name):
    p, plan, op, mag, S, guide, g, _ = _case(O, name)
    n_iter = 3
    base = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold=_hold(SPANS), seed=1)
    # repeated, another seed, another row_base
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold=_hold(SPANS), seed=1)) == _bits(base)
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold=_hold(SPANS), seed=99, row_base=7)) == _bits(base)
    # the other rows' pairs
    other = plan.griffinlim(S, B, T, n_iter, 0.99, guide=g, hold=_hold([(33, 0), SPANS[1], (0, 0)]))
    assert _bits(other[1]) == _bits(base[1]) and _bits(other[0]) != _bits(base[0])
    # its position in the batch: every row alone, and the rows in reverse order
    for r in range(B):
        alone = plan.griffinlim(S.reshape(B, -1)[r:r + 1].reshape(-1).contiguous(), 1, T, n_iter, 0.99, guide=g[r:r + 1], hold=_hold([SPANS[r]]))
        assert _bits(alone) == _bits(base[r:r + 1]), r
    rev = plan.griffinlim(plan.pack_magnitudes(mag.flip(0).cuda()), B, T, n_iter, 0.99, guide=g.flip(0).contiguous(), hold=_hold(SPANS[::-1]))
    assert _bits(rev.flip(0)) == _bits(base)


@pytest.mark.parametrize("name", ["specialised-frames", "generic-11025"])
def test_pairs_are_clamped_not_validated(O, name):
    p, plan, op, mag, S, guide, g, _ = _case(O, name)

    def run(pairs):
        return plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold=_hold(pairs))

    assert _bits(run([(40, 1), (-5, 4), (20, 20)])) == _bits(run([(33, 0), (0, 4), (20, 13)]))
    assert _bits(run([(INT_MAX, INT_MAX), (INT_MIN, INT_MIN), (INT_MIN, INT_MAX)])) == _bits(run([(33, 0), (0, 0), (0, 33)]))
    assert _bits(run([(-1, -1), (INT_MAX, INT_MIN), (5, INT_MIN)])) == _bits(run([(0, 0), (33, 0), (5, 0)]))


def test_held_rows_past_65535_and_across_chunks(O):
    """66 000 rows in one call equal the boundary rows alone: the compaction's chunks of 1024 rows, the staging's 65 535 rows per
    launch (chirp-z geometry 1009: the smallest frames; T = 7 is the fewest frames whose L = 601 exceeds the reflect padding of 504)"""
    p, plan = _plan("chirp-z-1009")
    rows, Tn = 66000, 7
    L = p.hop_length * (Tn - 1) + 1
    gen = torch.Generator(device="cuda").manual_seed(17)
    S = torch.rand((rows * Tn, plan.frame_stride), device="cuda", generator=gen) * 1000.0
    guide = torch.randn((rows, L), device="cuda", generator=gen) * 8000.0
    hold = torch.randint(-1, 5, (rows, 2), device="cuda", generator=gen, dtype=torch.int32)
    hold[2048:3072] = 7  # a chunk with nothing free
    whole = plan.griffinlim(S, rows, Tn, 2, 0.99, guide=guide, hold=hold)
    assert whole.shape == (rows, L) and bool(torch.isfinite(whole).all())
    for r in (0, 1023, 1024, 2047, 2048, 3071, 3072, 65535, 65536, rows - 1):
        alone = plan.griffinlim(S[r * Tn:(r + 1) * Tn], 1, Tn, 2, 0.99, guide=guide[r:r + 1], hold=hold[r:r + 1].contiguous())
        assert float(alone.abs().max()) > 0 and _bits(alone) == _bits(whole[r:r + 1]), r


# ---- workspace, timings, refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENGINES))
def test_held_workspace_queries_and_launch_times(O, name):
    p, plan, op, mag, S, guide, g, _ = _case(O, name)
    lib = plan.lib
    unheld, held = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T), helpers.need(lib, "griffinlim", plan.handle, B, T, **helpers.HELD)
    assert held >= unheld + 4 * (B * T + 1)
    if name == "specialised-runs":  # the frame buffer of the per-frame form on top
        frames_plan = _plan("specialised-frames")[1]
        assert held == helpers.need(lib, "griffinlim", frames_plan.handle, B, T, **helpers.HELD) > unheld + B * T * 4410 * 4
    assert helpers.need(lib, "waveform_from_mel", plan.handle, B, T, **helpers.HELD) >= lib.rfx_waveform_from_mel_workspace_bytes(plan.handle, B, T)
    assert helpers.need(lib, "audio_from_image", plan.handle, B, 0, T, **helpers.HELD) >= lib.rfx_audio_from_image_workspace_bytes(plan.handle, B, 0, T)
    ms = (ctypes.c_float * 4)(-1, -1, -1, -7)
    plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold=_hold(HOLDS), launch_ms=ms)
    assert all(ms[i] > 0 for i in range(3)) and ms[3] == -7


@pytest.mark.parametrize("name", ["specialised-runs", "specialised-frames", "generic-11025"])
def test_refusals_launch_nothing(O, name):
    """every refusal comes before any launch and leaves the output buffer as it was"""
    from riffusion import _hip

    p, plan, op, mag, S, guide, g, _ = _case(O, name)
    lib, L = plan.lib, g.shape[1]
    unheld, held = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T), helpers.need(lib, "griffinlim", plan.handle, B, T, **helpers.HELD)
    ws = torch.empty(held + 16, dtype=torch.uint8, device="cuda")
    stream = _hip.current_stream(torch.device("cuda"))
    out = torch.full((B, L), 123.0, device="cuda")
    hold = _hold(HOLDS)
    size = ctypes.sizeof(_hip.RfxHeldCallOptions)

    def call(d_guide, d_hold, reserved3=0, ws_bytes=held):
        opt = _hip.RfxHeldCallOptions(size, 0, 0, 0.0, 0.0, d_guide, L, L, 0, d_hold, reserved3)
        rc = lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 2, 0.99, out.data_ptr(), ws.data_ptr(), ws_bytes, stream,
                                   ctypes.byref(opt), None)
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        return rc, lib.rfx_last_error()

    rc, why = call(None, hold.data_ptr())
    assert rc == -1 and b"needs a guide" in why
    rc, why = call(g.data_ptr(), hold.data_ptr() + 2)
    assert rc == -1 and b"aligned" in why
    rc, why = call(g.data_ptr(), hold.data_ptr(), reserved3=1)
    assert rc == -1 and b"reserved3" in why
    rc, why = call(g.data_ptr(), hold.data_ptr(), ws_bytes=unheld)  # (on the runs plan: no frame buffer in it)
    assert rc == -3 and b"workspace too small" in why
    rc, why = call(g.data_ptr(), hold.data_ptr(), ws_bytes=held - 1)
    assert rc == -3
    # the fused entries check the held query too
    mel = torch.ones(B, plan.n_mels, T, device="cuda")
    need = helpers.need(lib, "waveform_from_mel", plan.handle, B, T, **helpers.HELD)
    ws2 = torch.empty(need, dtype=torch.uint8, device="cuda")
    opt = _hip.RfxHeldCallOptions(size, 0, 0, 0.0, 0.0, g.data_ptr(), L, L, 0, hold.data_ptr(), 0)
    assert lib.rfx_waveform_from_mel_ex(plan.handle, mel.data_ptr(), B, T, 1, 0, 2, 0.99, out.data_ptr(), ws2.data_ptr(), need - 1, stream, ctypes.byref(opt)) == -3
    # rfx_inverse_mel_ex holds no frames
    slots = torch.full((T * plan.frame_stride,), 123.0, device="cuda")
    need_i = lib.rfx_inverse_mel_workspace_bytes(plan.handle, 1, T)
    ws_i = torch.empty(need_i, dtype=torch.uint8, device="cuda")
    opt = _hip.RfxHeldCallOptions(size, 0, 0, 0.0, 0.0, None, 0, 0, 0, hold.data_ptr(), 0)
    assert lib.rfx_inverse_mel_ex(plan.handle, mel.data_ptr(), 1, T, 1, None, 0, slots.data_ptr(), ws_i.data_ptr(), need_i, stream, ctypes.byref(opt)) == -1
    assert b"holds no frames" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and bool((slots == 123.0).all())
    # the Python layer: hold without a guide, a wrong shape, a wrong type
    with pytest.raises(ValueError, match="needs a guide"):
        plan.griffinlim(S, B, T, 2, 0.99, hold=hold)
    for bad in (hold[:2], hold.long(), hold.cpu()):
        with pytest.raises(ValueError):
            plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold=bad)


# ---- fused equals staged -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lstsq", [False, True], ids=["sgd", "lstsq"])
def test_fused_held_call_equals_its_parts(golden_dir, lstsq):
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
    hold = _hold([(12, 0), (12, 0), (7, 9), (7, 9)])  # the two rows of a stereo clip share its pair
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, True, lut)
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, C, seed=seed)
    wave = plan.griffinlim(lin, N * C, W, n_iter, 0.99, seed=seed + 1, guide=guide, hold=hold)
    pcm3, peak3 = plan.pcm16(wave, channels=C, normalize=True)
    assert _bits(plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide, hold=hold)) == _bits(wave)
    pcm1, peak1 = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide, hold=hold)
    assert pcm1.shape == (N, L, C) and _bits(pcm1) == _bits(pcm3) and _bits(peak1) == _bits(peak3)
    start_only, _ = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq, guide=guide)
    assert _bits(start_only) != _bits(pcm1) and int(pcm1.abs().max()) > 30000


# ---- the product entry points -------------------------------------------------------------------------------------------------------------

def _conv(stereo, iters=32):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, num_griffin_lim_iters=iters), device="cuda")


def test_product_held_decode_depends_on_neither_chunking_nor_the_form_of_the_pairs():
    conv = _conv(True)
    N, W = 5, 40
    L = conv.p.hop_length * (W - 1)
    tiles = synthetic_tiles_u8(N, 512, W, seed=8)
    guides = synthetic_wave(N * 2, L + 30, seed=9).reshape(N, 2, L + 30)
    pairs = np.array([(0, 0), (12, 0), (0, 12), (10, 10), (40, 0)])

    def decode(hold, **kw):
        return conv.audio_from_spectrogram_images(tiles, guide_waveforms=guides, griffin_lim_iters=3, inverse_mel="lstsq", seed=3, hold_frames=hold, **kw)

    whole = decode(pairs, tiles_per_call=64)
    assert whole.shape == (N, L, 2) and whole.dtype == np.int16
    assert np.array_equal(decode(pairs, tiles_per_call=1), whole)
    assert np.array_equal(decode(torch.from_numpy(pairs).cuda(), tiles_per_call=2), whole)
    start_only, start = decode(None), conv.audio_from_spectrogram_images(tiles, guide_waveforms=guides, griffin_lim_iters=0, inverse_mel="lstsq", seed=3)
    assert np.array_equal(whole[0], start_only[0]) and np.array_equal(whole[4], start[4])  # (0, 0) and a full hold
    assert not np.array_equal(whole[1], start_only[1]) and not np.array_equal(whole[1], start[1])
    # one pair for all clips; values past the frame count are clamped
    assert np.array_equal(decode((10, 10))[3], whole[3]) and np.array_equal(decode((99, 5))[4], whole[4])
    # the float waveform and the error report take it too
    wave = decode(pairs, return_waveform=True)
    assert wave.shape == (N, 2, L) and np.isfinite(wave).all()
    pcm, err = decode(pairs, return_error=True)
    assert np.array_equal(pcm, whole) and err.shape == (N,)
    with pytest.raises(ValueError, match="guide"):
        conv.audio_from_spectrogram_images(tiles, griffin_lim_iters=3, hold_frames=(10, 10))
    for bad in (pairs[:4], (1, 2, 3), (0.5, 1.0)):
        with pytest.raises(ValueError):
            decode(bad)


def test_torch_seam_takes_hold_frames():
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(num_griffin_lim_iters=2), device="cuda")
    plan = conv._plan()
    Tn = 30
    mel = torch.rand(2, plan.n_mels, Tn, generator=torch.Generator().manual_seed(2)) * 1e6
    guide = synthetic_wave(2, conv.p.hop_length * (Tn - 1), seed=12)
    got = conv.waveform_from_mel_amplitudes(mel, seed=8, guide=guide, hold_frames=[(12, 0), (0, 40)])
    want = plan.waveform_from_mel(mel.cuda(), 2, 2, 0.99, seed=8, guide=guide.cuda(), hold=_hold([(12, 0), (0, 30)]))
    assert _bits(got) == _bits(want) != _bits(conv.waveform_from_mel_amplitudes(mel, seed=8, guide=guide))
    assert conv.hold_frames_for(0.1, 0.05) == conv.p.hold_frames_for(0.1, 0.05) == (6, 1)
    with pytest.raises(ValueError, match="guide"):
        conv.waveform_from_mel_amplitudes(mel, seed=8, hold_frames=(3, 3))


def _golden_clip2(golden_dir):
    from PIL import Image

    from riffusion.util import audio_util

    image = Image.open(os.path.join(golden_dir, CLIP2 + "_stereo.png"))
    segment = audio_util.PcmSegment.from_wav(os.path.join(golden_dir, CLIP2 + ".wav"))
    return image, segment


def test_cli_hold_flags_decode_the_golden_tile(golden_dir, tmp_path):
    from riffusion import cli
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.util import audio_util

    image, _ = _golden_clip2(golden_dir)
    png, wav = os.path.join(golden_dir, CLIP2 + "_stereo.png"), os.path.join(golden_dir, CLIP2 + ".wav")
    out = str(tmp_path / "held.wav")
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", png, "--audio", out, "--guide-audio", wav, "--griffin-lim-iters", "2", "--hold-head-ms", "1000",
              "--hold-tail-ms", "500"])
    written = audio_util.PcmSegment.from_wav(out)
    conv = SpectrogramImageConverter(cli._params_from_image(image), device="cuda")
    assert written.channels == 2 and written.frame_rate == 44100
    assert len(np.asarray(written.get_array_of_samples())) == 2 * conv.p.hop_length * (image.width - 1)
    torch.manual_seed(5)
    want = conv.audio_from_spectrogram_image(image, guide_segment=cli._load_segment(wav), griffin_lim_iters=2, hold_frames=conv.hold_frames_for(1.0, 0.5))
    assert conv.hold_frames_for(1.0, 0.5) == (96, 46)
    assert np.array_equal(np.asarray(written.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    torch.manual_seed(5)
    start_only = conv.audio_from_spectrogram_image(image, guide_segment=cli._load_segment(wav), griffin_lim_iters=2)
    assert not np.array_equal(np.asarray(start_only.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    with pytest.raises(ValueError, match="guide"):
        conv.audio_from_spectrogram_image(image, hold_frames=(3, 3))
    with pytest.raises(SystemExit):
        cli.main(["image-to-audio", "--image", png, "--audio", out, "--hold-head-ms", "1000"])


def test_full_width_decode_of_clip_2_holds_the_kept_audio(golden_dir):
    """the golden stereo tile of clip 2 at its full width, its recording with samples [88200, 132300) zeroed as the guide, the frames
    wholly inside the kept audio held: the kept samples (those only held frames reach) keep their n_iter = 0 values bit for bit,
    while the start-only decode the project shipped moves them.  The drift and both spectral convergences are printed: figures,
    the condition is the equality."""
    from riffusion.util import image_util

    image, segment = _golden_clip2(golden_dir)
    tile = np.asarray(image_util.rgb_array_from_image(image))[None]
    Tn = tile.shape[2]
    clip = np.asarray(segment.get_array_of_samples(), dtype=np.int16).reshape(-1, 2).T[None].astype(np.float32)
    lo, hi = 88200, 132300
    guide = clip.copy()
    guide[:, :, lo:hi] = 0
    import riffusion_oracle as O_

    for n_iter in (4, 32):
        conv = _conv(True)
        L = conv.p.hop_length * (Tn - 1)
        pair = conv.hold_frames_for(lo / 44100.0, (L - hi) / 44100.0)
        only = held_oracle.held_only_samples([pair], Tn, O_.params_from(conv.p))[0].numpy()
        assert only[:lo - 4851].all() and only[hi + 4851:L].all() and not only[lo:hi].any()

        def decode(n, hold):
            return conv.audio_from_spectrogram_images(tile, seed=1, guide_waveforms=guide, griffin_lim_iters=n, hold_frames=hold,
                                                      return_waveform=True, return_error=True)

        (start, _), (free, sc_free), (held, sc_held) = decode(0, None), decode(n_iter, None), decode(n_iter, pair)
        start, free, held = torch.from_numpy(start[0]), torch.from_numpy(free[0]), torch.from_numpy(held[0])
        m = torch.from_numpy(only)
        print(f"golden clip 2, full width ({Tn} frames, hold {pair}), n_iter = {n_iter}: kept samples vs. their n_iter = 0 values: start-only "
              f"{held_oracle.db(start[:, m], free[:, m]):.1f} dB, held {'equal' if torch.equal(held[:, m], start[:, m]) else 'NOT equal'}; "
              f"spectral convergence start-only {float(sc_free[0]):.4f}, held {float(sc_held[0]):.4f}")
        assert _bits(held[:, m]) == _bits(start[:, m])
        assert _bits(free[:, m]) != _bits(start[:, m])
