"""
Loop calls on the device (include/rfx.h: rfx_loop_call_options): a row's T columns are the STFT of a signal with period hop T;
launches 1 .. n_iter read their input modulo the period (compile-time variants of the frame kernels), every fold is circular.

Parity is against tests/loop_oracle.py's loop_griffinlim with the same injected start.  By the rule of
tests/test_gpu_held_frames.py no SNR floor is fixed in advance: each case computes the oracle in float64 and in float32 in the same
run and requires the device's SNR against the float64 result to be no more than 6 dB below the float32 oracle's; the circular
spectral convergence of the device result, computed on the CPU in float64, lies within 1 % (relative) of the float32 oracle's.
The exact properties compare bits.  B = 3 rows of T = 41 frames: the smallest T valid on all three engines, one past a whole period
on the specialised engine, no multiple of 16; on the specialised engine T = 40 as well (period == n_fft: every frame wraps).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import loop_oracle
from engines import CLIP2, LOOPING, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave

pytestmark = pytest.mark.gpu

B, T = 3, 41
SHAPES = [(name, T) for name in LOOPING] + [("specialised", 40)]
SHAPE_IDS = [f"{name}-T{t}" for name, t in SHAPES]


@pytest.fixture(scope="module")
def O():
    return oracle()


_CASES = {}


def _case(O, name, frames=T):
    """(params, plan, op, target magnitudes (B, n_stft, frames), injected start, their slots on the device): computed once per engine
    and frame count, never modified"""
    if (name, frames) not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        P = p.hop_length * frames
        mag = loop_oracle.loop_stft(O, synthetic_wave(B, P, seed=101), op).abs()
        assert mag.shape == (B, op.n_stft, frames) and frames >= loop_oracle.min_frames(op)
        a0 = torch.rand(mag.shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(7))
        _CASES[(name, frames)] = (p, plan, op, mag, a0, plan.pack_magnitudes(mag.cuda()), plan.pack_complex(a0.cuda()))
    return _CASES[(name, frames)]


# ---- parity with the oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [0, 1, 4])
@pytest.mark.parametrize("name,frames", SHAPES, ids=SHAPE_IDS)
def test_loop_call_matches_the_oracle(O, name, frames, n_iter):
    p, plan, op, mag, a0, S, A = _case(O, name, frames)
    want32 = loop_oracle.loop_griffinlim(O, mag, op, a0, n_iter, torch.float32)
    want64 = loop_oracle.loop_griffinlim(O, mag, op, a0, n_iter, torch.float64)
    got = plan.griffinlim(S, B, frames, n_iter, 0.99, angles0_slots=A, loop=True).cpu()
    assert got.shape == want32.shape == (B, p.hop_length * frames) and bool(torch.isfinite(got).all())
    dev, o32, both = snr_db(want64, got), snr_db(want64, want32), snr_db(want32, got)
    sc_dev, sc_o32 = loop_oracle.loop_spectral_convergence(O, got, mag, op), loop_oracle.loop_spectral_convergence(O, want32, mag, op)
    print(f"loop griffinlim {name} T={frames} n_iter={n_iter}: device vs float64 oracle {dev:.1f} dB, float32 oracle vs float64 oracle {o32:.1f} dB, "
          f"device vs float32 oracle {both:.1f} dB; circular spectral convergence device {sc_dev:.6f}, float32 oracle {sc_o32:.6f}")
    assert dev >= o32 - 6.0
    assert abs(sc_dev - sc_o32) <= 0.01 * sc_o32


# ---- exact properties ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,frames", SHAPES, ids=SHAPE_IDS)
def test_rolled_columns_give_rolled_audio(O, name, frames):
    p, plan, op, mag, a0, S, A = _case(O, name, frames)
    n_iter = 2
    base = plan.griffinlim(S, B, frames, n_iter, 0.99, angles0_slots=A, loop=True)
    assert float(base.abs().max()) > 0
    for k in (1, 16, frames - 1):
        Sk = plan.pack_magnitudes(torch.roll(mag, k, dims=-1).cuda())
        Ak = plan.pack_complex(torch.roll(a0, k, dims=-1).cuda())
        rolled = plan.griffinlim(Sk, B, frames, n_iter, 0.99, angles0_slots=Ak, loop=True)
        assert _bits(rolled) == _bits(torch.roll(base, k * p.hop_length, dims=-1)), k
    # ... which the unlooped call of the same columns does not do
    plain = plan.griffinlim(S, B, frames, n_iter, 0.99, angles0_slots=A)
    assert plain.shape[1] == op.hop_length * (frames - 1) + (op.n_fft & 1) and _bits(plain) != _bits(base[:, :plain.shape[1]])


@pytest.mark.parametrize("name", LOOPING)
def test_a_loop_row_depends_on_its_magnitudes_and_its_start_alone(O, name):
    p, plan, op, mag, a0, S, A = _case(O, name)
    n_iter = 2
    base = plan.griffinlim(S, B, T, n_iter, 0.99, angles0_slots=A, loop=True, seed=1)
    for r in range(B):  # a row alone
        Sr, Ar = plan.pack_magnitudes(mag[r:r + 1].cuda()), plan.pack_complex(a0[r:r + 1].cuda())
        assert _bits(plan.griffinlim(Sr, 1, T, n_iter, 0.99, angles0_slots=Ar, loop=True, seed=5, row_base=9)) == _bits(base[r]), r
    rev = plan.griffinlim(plan.pack_magnitudes(mag.flip(0).cuda()), B, T, n_iter, 0.99, angles0_slots=plan.pack_complex(a0.flip(0).cuda()), loop=True)
    assert _bits(rev.flip(0)) == _bits(base)
    # the random start: seed and row_base matter through it alone - row r of a call with row_base = b is row r + b of the larger call
    drawn = plan.griffinlim(S, B, T, n_iter, 0.99, loop=True, seed=3)
    assert _bits(drawn) != _bits(base) and _bits(drawn) != _bits(plan.griffinlim(S, B, T, n_iter, 0.99, loop=True, seed=4))
    tail = plan.griffinlim(plan.pack_magnitudes(mag[1:].cuda()), B - 1, T, n_iter, 0.99, loop=True, seed=3, row_base=1)
    assert _bits(tail) == _bits(drawn[1:])
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, loop=True, seed=3)) == _bits(drawn)
    # a guided loop call has no randomness left
    guide = synthetic_wave(B, p.hop_length * T - 100, seed=202).cuda()
    guided = plan.griffinlim(S, B, T, n_iter, 0.99, guide=guide, loop=True, seed=1)
    assert guided.shape == base.shape and bool(torch.isfinite(guided).all()) and float(guided.abs().max()) > 0
    assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, guide=guide, loop=True, seed=99, row_base=4)) == _bits(guided) != _bits(drawn)
    # silent magnitudes give silence
    silent = plan.griffinlim(torch.zeros_like(S), B, T, n_iter, 0.99, loop=True, seed=3)
    assert silent.shape == base.shape and not bool(silent.any())


@pytest.mark.parametrize("name", ["specialised", "generic-11025"])
def test_guided_loop_start_is_the_phase_of_the_circular_stft(O, name):
    """n_iter = 0: the device analyses the fitted guide with the circular STFT, projects, and synthesises - against the oracle by the parity rule"""
    p, plan, op, mag, a0, S, A = _case(O, name)
    P = p.hop_length * T
    guide = synthetic_wave(B, P, seed=202)
    G32, G64 = loop_oracle.loop_stft(O, guide, op), loop_oracle.loop_stft(O, guide, op, torch.float64)
    want32 = loop_oracle.loop_griffinlim(O, mag, op, G32 / (G32.abs() + 1e-16), 1, torch.float32)
    want64 = loop_oracle.loop_griffinlim(O, mag, op, G64 / (G64.abs() + 1e-16), 1, torch.float64)
    got = plan.griffinlim(S, B, T, 1, 0.99, guide=guide.cuda(), loop=True).cpu()
    dev, o32 = snr_db(want64, got), snr_db(want64, want32)
    print(f"guided loop griffinlim {name} n_iter=1: device vs float64 oracle {dev:.1f} dB, float32 oracle vs float64 oracle {o32:.1f} dB")
    assert dev >= o32 - 6.0


# ---- unchanged behaviour ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["specialised", "generic-11025"])
def test_loop_zero_in_the_grown_struct_is_the_masked_size_call(O, name):
    from riffusion import _hip

    p, plan, op, mag, a0, S, A = _case(O, name)
    lib, n_iter = plan.lib, 2
    L = lib.rfx_griffinlim_output_samples(plan.handle, T)
    g = synthetic_wave(B, L, seed=202).cuda()
    pairs = torch.tensor([[3, 2]] * B, dtype=torch.int32, device="cuda")
    bits = torch.zeros((B, T, plan.hold_mask_words), dtype=torch.int32, device="cuda")
    bits[:, :, :40] = -1
    ws = torch.empty(helpers.need(lib, "griffinlim", plan.handle, B, T, **helpers.MASKED), dtype=torch.uint8, device="cuda")
    stream = _hip.current_stream(torch.device("cuda"))
    cases = {"plain": dict(), "guided": dict(guide=g), "held": dict(guide=g, hold=pairs), "masked": dict(guide=g, hold_bins=bits)}
    for what, kw in cases.items():
        want = plan.griffinlim(S, B, T, n_iter, 0.99, seed=6, **kw)
        o = _hip.call_options(rows=B, **kw)
        grown = _hip.RfxLoopCallOptions(ctypes.sizeof(_hip.RfxLoopCallOptions), o.flags, o.row_base, o.magnitude_hint, 0.0,
                                        getattr(o, "d_guide", None), getattr(o, "guide_stride", 0), getattr(o, "guide_samples", 0), 0,
                                        getattr(o, "d_hold_frames", None), 0, getattr(o, "d_hold_bins", None), getattr(o, "hold_words", 0), 0, 0, 0)
        out = torch.full((B, L), 123.0, device="cuda")
        assert lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 6, B, T, n_iter, 0.99, out.data_ptr(), ws.data_ptr(), ws.numel(), stream,
                                     ctypes.byref(grown), None) == 0, lib.rfx_last_error()
        assert _bits(out) == _bits(want), what


# ---- workspace, launch times, refusals ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LOOPING)
def test_loop_workspace_queries_and_launch_times(O, name):
    p, plan, op, mag, a0, S, A = _case(O, name)
    lib = plan.lib
    need = helpers.need(lib, "griffinlim", plan.handle, B, T, loop=1)
    assert need > 0 and lib.rfx_griffinlim_loop_output_samples(plan.handle, T) == p.hop_length * T == plan.output_samples(T, True)
    assert need >= 4 * B * T * op.win_length  # the synthesis frames
    assert helpers.need(lib, "griffinlim", plan.handle, B, loop_oracle.min_frames(op) - 1, loop=1) == 0
    assert helpers.need(lib, "waveform_from_mel", plan.handle, B, T, loop=1) > need
    assert helpers.need(lib, "audio_from_image", plan.handle, B, 0, T, loop=1) > helpers.need(lib, "waveform_from_mel", plan.handle, B, T, loop=1)
    ms = (ctypes.c_float * 4)(-1, -1, -1, -7)
    plan.griffinlim(S, B, T, 2, 0.99, angles0_slots=A, loop=True, launch_ms=ms)
    assert all(ms[i] > 0 for i in range(3)) and ms[3] == -7


@pytest.mark.parametrize("name", ["specialised", "generic-11025"])
def test_refusals_launch_nothing(O, name):
    """every refusal comes before any launch and leaves the output buffer as it was"""
    from riffusion import _hip

    p, plan, op, mag, a0, S, A = _case(O, name)
    lib, P = plan.lib, p.hop_length * T
    need = helpers.need(lib, "griffinlim", plan.handle, B, T, loop=1)
    ws = torch.empty(need + helpers.need(lib, "griffinlim", plan.handle, B, T, **helpers.MASKED), dtype=torch.uint8, device="cuda")
    stream = _hip.current_stream(torch.device("cuda"))
    out = torch.full((B, P), 123.0, device="cuda")
    g = synthetic_wave(B, P, seed=202).cuda()
    pairs = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    bits = torch.zeros((B, T, plan.hold_mask_words), dtype=torch.int32, device="cuda")
    size = ctypes.sizeof(_hip.RfxLoopCallOptions)

    def call(loop=1, reserved5=0, d_guide=None, d_pairs=None, d_bins=None, frames=T, ws_bytes=None):
        opt = _hip.RfxLoopCallOptions(size, 0, 0, 0.0, 0.0, d_guide, P if d_guide else 0, P if d_guide else 0, 0, d_pairs, 0, d_bins,
                                      plan.hold_mask_words if d_bins else 0, 0, loop, reserved5)
        rc = lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, frames, 2, 0.99, out.data_ptr(), ws.data_ptr(),
                                   ws.numel() if ws_bytes is None else ws_bytes, stream, ctypes.byref(opt), None)
        torch.cuda.synchronize()
        assert bool((out == 123.0).all())
        return rc, lib.rfx_last_error()

    low = loop_oracle.min_frames(op)
    rc, why = call(frames=low - 1)
    assert rc == -1 and f"at least {low} frames, got {low - 1}".encode() in why
    rc, why = call(d_guide=g.data_ptr(), d_pairs=pairs.data_ptr())
    assert rc == -1 and b"loop together with" in why
    rc, why = call(d_guide=g.data_ptr(), d_bins=bits.data_ptr())
    assert rc == -1 and b"loop together with" in why
    rc, why = call(loop=2)
    assert rc == -1 and b"loop must be 0 or 1" in why
    rc, why = call(reserved5=1)
    assert rc == -1 and b"reserved5" in why
    rc, why = call(ws_bytes=need - 1)
    assert rc == -3 and b"workspace too small" in why
    # rfx_inverse_mel_ex decodes no loop
    mel = torch.ones(1, plan.n_mels, T, device="cuda")
    slots = torch.full((T * plan.frame_stride,), 123.0, device="cuda")
    need_i = lib.rfx_inverse_mel_workspace_bytes(plan.handle, 1, T)
    ws_i = torch.empty(need_i, dtype=torch.uint8, device="cuda")
    opt = _hip.RfxLoopCallOptions(size, 0, 0, 0.0, 0.0, None, 0, 0, 0, None, 0, None, 0, 0, 1, 0)
    assert lib.rfx_inverse_mel_ex(plan.handle, mel.data_ptr(), 1, T, 1, None, 0, slots.data_ptr(), ws_i.data_ptr(), need_i, stream, ctypes.byref(opt)) == -1
    assert b"decodes no loop" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((slots == 123.0).all())
    # the Python layer
    with pytest.raises(ValueError, match=f"at least {low} frames, got {low - 1}"):
        plan.griffinlim(S, B, low - 1, 2, 0.99, loop=True)
    with pytest.raises(ValueError, match="loop together with"):
        plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold=pairs, loop=True)
    with pytest.raises(ValueError, match="loop together with"):
        plan.griffinlim(S, B, T, 2, 0.99, guide=g, hold_bins=bits, loop=True)


def test_the_chirp_z_engine_refuses_a_loop_call():
    from riffusion import _hip

    p, plan = _plan("chirp-z-1009")
    lib = plan.lib
    assert p.hop_length * T >= p.n_fft  # the frame count is not what is refused
    assert helpers.need(lib, "griffinlim", plan.handle, B, T, loop=1) == 0 == helpers.need(lib, "waveform_from_mel", plan.handle, B, T, loop=1)
    S = torch.ones(B * T * plan.frame_stride, device="cuda")
    P = p.hop_length * T
    out = torch.full((B, P), 123.0, device="cuda")
    ws = torch.empty(lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T + 1), dtype=torch.uint8, device="cuda")
    opt = _hip.RfxLoopCallOptions(ctypes.sizeof(_hip.RfxLoopCallOptions), 0, 0, 0.0, 0.0, None, 0, 0, 0, None, 0, None, 0, 0, 1, 0)
    rc = lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 2, 0.99, out.data_ptr(), ws.data_ptr(), ws.numel(),
                               _hip.current_stream(torch.device("cuda")), ctypes.byref(opt), None)
    torch.cuda.synchronize()
    assert rc == -4 and b"chirp-z" in lib.rfx_last_error() and bool((out == 123.0).all())
    opt.loop = 0  # the same call unlooped runs
    assert lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 2, 0.99, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _hip.current_stream(torch.device("cuda")), ctypes.byref(opt), None) == 0
    with pytest.raises(ValueError, match="chirp-z"):
        plan.griffinlim(S, B, T, 2, 0.99, loop=True)


# ---- fused equals staged ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lstsq", [False, True], ids=["sgd", "lstsq"])
def test_fused_loop_call_equals_its_parts(golden_dir, lstsq):
    from PIL import Image

    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    p = SpectrogramParams(stereo=True)
    plan = _hip.get_plan(p, "cuda")
    lib = plan.lib
    tile = np.array(Image.open(os.path.join(golden_dir, CLIP2 + "_stereo.png")).convert("RGB"))
    N, C, W, n_iter, seed = 2, 2, 41, 3, 40
    tiles = torch.from_numpy(np.stack([tile[:, 0:W], tile[:, 200:200 + W]])).cuda()
    P = p.hop_length * W
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, True, lut)
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, C, seed=seed)
    wave = plan.griffinlim(lin, N * C, W, n_iter, 0.99, seed=seed + 1, loop=True)
    assert wave.shape == (N * C, P)
    pcm3, peak3 = plan.pcm16(wave, channels=C, normalize=True)
    assert _bits(plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, lstsq=lstsq, loop=True)) == _bits(wave)
    pcm1, peak1 = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq, loop=True)
    assert pcm1.shape == (N, P, C) and _bits(pcm1) == _bits(pcm3) and _bits(peak1) == _bits(peak3)
    unlooped, _ = plan.audio_from_image(tiles, True, lut, n_iter, 0.99, seed=seed, lstsq=lstsq)
    assert unlooped.shape == (N, P - p.hop_length, C) and int(pcm1.abs().max()) > 30000
    # a workspace one byte below the loop query
    stream = _hip.current_stream(torch.device("cuda"))
    opt = _hip.call_options(rows=N * C, lstsq=lstsq, loop=True)
    need = helpers.need(lib, "waveform_from_mel", plan.handle, N * C, W, loop=1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((N * C, P), 123.0, device="cuda")
    assert lib.rfx_waveform_from_mel_ex(plan.handle, mel.data_ptr(), N * C, W, C, seed, n_iter, 0.99, out.data_ptr(), ws.data_ptr(), need - 1, stream,
                                        ctypes.byref(opt)) == -3
    need = helpers.need(lib, "audio_from_image", plan.handle, N, 1, W, loop=1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    pcm = torch.full((N, P, C), 77, dtype=torch.int16, device="cuda")
    peak = torch.zeros(N, device="cuda")
    assert lib.rfx_audio_from_image_u8_ex(plan.handle, tiles.data_ptr(), N, W, 1, lut.data_ptr(), seed, n_iter, 0.99, 1, peak.data_ptr(), pcm.data_ptr(),
                                          ws.data_ptr(), need - 1, stream, ctypes.byref(opt)) == -3
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and bool((pcm == 77).all())
    assert lib.rfx_audio_from_image_u8_ex(plan.handle, tiles.data_ptr(), N, W, 1, lut.data_ptr(), seed, n_iter, 0.99, 1, peak.data_ptr(), pcm.data_ptr(),
                                          ws.data_ptr(), need, stream, ctypes.byref(opt)) == 0
    assert _bits(pcm) == _bits(pcm1)


@pytest.mark.parametrize("lstsq", [False, True], ids=["sgd", "lstsq"])
def test_fused_loop_call_on_a_row_family_equals_its_parts(lstsq):
    """at 48 kHz the SGD stage of the fused call writes the magnitudes in the family's slot order"""
    p, plan = _plan("row-family-48k")
    n_iter, seed = 3, 11
    mel = torch.rand(B, plan.n_mels, T, generator=torch.Generator().manual_seed(4)).cuda() * 1e6
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, 1, seed=seed)
    wave = plan.griffinlim(lin, B, T, n_iter, 0.99, seed=seed + 1, loop=True)
    assert _bits(plan.waveform_from_mel(mel, 1, n_iter, 0.99, seed=seed, lstsq=lstsq, loop=True)) == _bits(wave)


# ---- the product entry points ---------------------------------------------------------------------------------------------------------------

def _conv(stereo, iters=32):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, num_griffin_lim_iters=iters), device="cuda")


def test_product_loop_decode(golden_dir):
    from PIL import Image

    from riffusion.util import image_util

    conv = _conv(True, iters=4)
    W, seed = 64, 21
    tiles = np.stack([np.array(Image.open(os.path.join(golden_dir, name)).convert("RGB"))[:, 100:100 + W] for name in ("og_beat.png", "vibes.png")])
    N, P = len(tiles), conv.p.hop_length * W
    whole = conv.audio_from_spectrogram_images(tiles, loop=True, seed=seed, tiles_per_call=2)
    assert whole.shape == (N, P, 2) and whole.dtype == np.int16 and int(np.abs(whole).max()) > 30000
    assert np.array_equal(conv.audio_from_spectrogram_images(tiles, loop=True, seed=seed, tiles_per_call=1), whole)
    # ... the C ABI route
    plan = conv.converter._plan()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    pcm, _ = plan.audio_from_image(torch.from_numpy(tiles).cuda(), True, lut, 4, 0.99, seed=seed, magnitude_hint=30e6, loop=True)
    assert np.array_equal(pcm.cpu().numpy(), whole)
    # the float waveforms, the filters and a guide go with it
    wave = conv.audio_from_spectrogram_images(tiles, loop=True, seed=seed, return_waveform=True)
    assert wave.shape == (N, 2, P)
    print("seam figure of the product's loop decode, per clip and channel:", np.round(loop_oracle.seam_figure(torch.from_numpy(wave)), 2).tolist())
    filtered = conv.audio_from_spectrogram_images(tiles, loop=True, seed=seed, apply_filters=True)
    assert filtered.shape == whole.shape and not np.array_equal(filtered, whole)
    guides = synthetic_wave(N * 2, P, seed=9).reshape(N, 2, P)
    # (with the closed-form InverseMelScale a guided decode has no randomness left: the seed changes nothing)
    guided = conv.audio_from_spectrogram_images(tiles, loop=True, seed=seed, guide_waveforms=guides, inverse_mel="lstsq")
    assert guided.shape == whole.shape
    assert np.array_equal(guided, conv.audio_from_spectrogram_images(tiles, loop=True, seed=seed + 1, guide_waveforms=guides, inverse_mel="lstsq"))
    unlooped = conv.audio_from_spectrogram_images(tiles, seed=seed)
    assert unlooped.shape == (N, P - conv.p.hop_length, 2)
    # what does not go with a loop
    with pytest.raises(ValueError, match="loop together with"):
        conv.audio_from_spectrogram_images(tiles, loop=True, guide_waveforms=guides, hold_frames=(3, 3))
    with pytest.raises(ValueError, match="loop together with"):
        conv.audio_from_spectrogram_images(tiles, loop=True, guide_waveforms=guides, hold_mask=np.ones((512, W), dtype=bool))
    with pytest.raises(ValueError, match="return_error"):
        conv.audio_from_spectrogram_images(tiles, loop=True, return_error=True)
    with pytest.raises(ValueError, match="sequence"):
        conv.audio_from_spectrogram_image_sequence(tiles, loop=True)
    with pytest.raises(ValueError, match="at least 40 frames, got 39"):
        conv.audio_from_spectrogram_images(tiles[:, :, :39], loop=True)


def test_torch_seam_and_the_spectrogram_entry_take_loop():
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(num_griffin_lim_iters=2), device="cuda")
    plan = conv._plan()
    mel = torch.rand(2, plan.n_mels, T, generator=torch.Generator().manual_seed(2)) * 1e6
    got = conv.waveform_from_mel_amplitudes(mel, seed=8, loop=True)
    assert got.shape == (2, conv.p.hop_length * T)
    assert _bits(got) == _bits(plan.waveform_from_mel(mel.cuda(), 2, 2, 0.99, seed=8, loop=True)) != _bits(conv.waveform_from_mel_amplitudes(mel, seed=8))
    a0 = torch.rand(2, plan.n_fft // 2 + 1, T, dtype=torch.complex64, generator=torch.Generator().manual_seed(3))
    staged = conv.waveform_from_mel_amplitudes(mel, seed=8, angles0=a0, loop=True)
    assert staged.shape == got.shape and _bits(staged) != _bits(got)
    with pytest.raises(ValueError, match="loop together with"):
        conv.waveform_from_mel_amplitudes(mel, seed=8, guide=torch.zeros(2, 100), hold_frames=(1, 1), loop=True)
    with pytest.raises(ValueError, match="at least 40 frames"):
        conv.waveform_from_mel_amplitudes(mel[:, :, :30], seed=8, loop=True)
    torch.manual_seed(4)
    seg = conv.audio_from_spectrogram(mel.numpy(), apply_filters=False, loop=True)
    assert int(seg.frame_count()) == conv.p.hop_length * T and seg.channels == 2


def test_cli_loop_writes_the_period(golden_dir, tmp_path):
    from PIL import Image

    from riffusion import cli
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.util import audio_util

    image = Image.open(os.path.join(golden_dir, "og_beat_64.png"))
    W = image.width
    assert W >= 40
    png, out = os.path.join(golden_dir, "og_beat_64.png"), str(tmp_path / "loop.wav")
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", png, "--audio", out, "--loop", "--griffin-lim-iters", "4"])
    written = audio_util.PcmSegment.from_wav(out)
    params = cli._params_from_image(image)
    assert int(written.frame_count()) == params.hop_length * W and written.frame_rate == params.sample_rate
    conv = SpectrogramImageConverter(params, device="cuda")
    torch.manual_seed(5)
    want = conv.audio_from_spectrogram_image(image, griffin_lim_iters=4, loop=True)
    assert np.array_equal(np.asarray(written.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    # the batch command takes the flag as well
    src, dst = tmp_path / "tiles", tmp_path / "clips"
    src.mkdir()
    image.save(str(src / "a.png"), exif=image.getexif(), format="PNG")
    cli.main(["images-to-audio-batch", "--image-dir", str(src), "--output-dir", str(dst), "--loop"])
    assert int(audio_util.PcmSegment.from_wav(str(dst / "a.wav")).frame_count()) == params.hop_length * W
