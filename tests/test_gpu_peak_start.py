"""
The spectral-peak start on the device (include/rfx.h: rfx_peak_start, rfx_start_call_options): Griffin-Lim's initial angles built
from the magnitudes alone, standalone and as the start of the three inverse entries.

* Standalone against the float64 restatement tests/peak_start_oracle.py: every component within 1e-5 (the decisions are exact, the
  double chain agrees to 1e-11 turns, the rest is the float32 fraction and float32 sincos: tests/test_peak_start_cpu.py), and the raw
  slots are bit-equal to pack_complex(unpack_complex(slots)): conjugate slots conjugated, both copies of a bin written, padding 0.
  On the specialised engine B = 3, T = 37 with the crafted frames and tile columns of the CPU test, at 48 kHz (row family) B = 2,
  T = 22, at 8 kHz / 64 filters (a generic plan) B = 2, T = 21, and at 11.025 kHz (the generic frame engine) B = 2, T = 21.
* A call with start = 1 is bit-equal to the staged route - inverse mel, rfx_peak_start, the call with the angles injected - for each of
  the three entries, at 0 and 3 iterations, mono and stereo, as a loop call, on the per-frame and on the run form, and at 48 kHz where
  the fused call's magnitudes are in the row family's slot order.
* A row depends on its magnitudes alone; start = 0 in the new struct changes nothing; a workspace one byte short is refused; the
  product path decodes with a lower spectral error than the random start at 2 iterations on every seed tile.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import peak_start_inputs as inputs
import peak_start_oracle
from engines import CLIP2, bits as _bits
from helpers import oracle

pytestmark = pytest.mark.gpu

TILES = ["og_beat", "vibes", "agile", "marim", "motorway"]

ENGINES = {  # name: (rfx_plan_griffinlim_engine's answer, SpectrogramParams keywords, B, T)
    "specialised": ("specialised", dict(), 3, 37),
    "row-family-48k": ("row-family", dict(sample_rate=48000), 2, 22),
    # a generic plan (rfx_plan: everything but the default geometry); n_fft = 3200 = 40 * 80 runs on the row family's frame kernels
    "8k-64-filters": ("row-family", dict(sample_rate=8000, max_frequency=4000, num_frequencies=64), 2, 21),
    "generic-11025": ("generic", dict(sample_rate=11025, max_frequency=5512), 2, 21),  # ... and the generic frame kernels themselves
}


@pytest.fixture(scope="module")
def O():
    return oracle()


def _plan(name):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    engine, kw, B, T = ENGINES[name]
    p = SpectrogramParams(**kw)
    plan = _hip.get_plan(p, "cuda")
    assert plan.griffinlim_engine == engine and (name == "specialised") != bool(plan.generic)
    return p, plan, B, T


_CASES = {}


def _case(O, golden_dir, name):
    """(params, plan, B, T, magnitudes (B, F, T) float32 numpy, the crafted row's case table): computed once per engine"""
    if name not in _CASES:
        p, plan, B, T = _plan(name)
        F = plan.n_stft
        crafted, at = inputs.crafted_row(F, T)
        rows = [crafted]
        if name == "specialised":
            rows.append(inputs.tile_magnitudes(O, O.params_from(p), golden_dir, "og_beat", 100, 137)[0].numpy())
        while len(rows) < B:
            rows.append(inputs.crafted_row(F, T, seed=10 + len(rows))[0])
        _CASES[name] = (p, plan, B, T, np.ascontiguousarray(np.stack(rows).astype(np.float32)), at)
    return _CASES[name]


# ---- standalone, against the restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ENGINES))
def test_peak_start_matches_the_restatement(O, golden_dir, name):
    p, plan, B, T, mag, at = _case(O, golden_dir, name)
    want, peaks = peak_start_oracle.peak_start(mag, p.hop_length, p.n_fft, details=True)
    inputs.assert_crafted_cases(peaks[0], at, plan.n_stft)
    S = plan.pack_magnitudes(torch.from_numpy(mag).cuda())
    slots = plan.peak_start(S, B, T)
    assert slots.shape == (B * T, plan.frame_stride) and slots.dtype == torch.complex64
    got = plan.unpack_complex(slots, B, T).cpu().numpy()
    assert got.shape == want.shape and not np.isnan(got.real).any() and not np.isnan(got.imag).any()
    err = max(float(np.abs(got.real - want.real).max()), float(np.abs(got.imag - want.imag).max()))
    print(f"{name}: largest component error against the restatement {err:.2e}")
    assert err <= 1e-5
    # the raw slots are what rfx_pack_complex makes of them: conjugate slots, both copies, zero padding
    assert _bits(slots) == _bits(plan.pack_complex(plan.unpack_complex(slots, B, T)))
    # a frame without a peak: phase 0 everywhere, (-1)^k
    t = at["zero"]
    assert np.array_equal(got[0, :, t], np.where(np.arange(plan.n_stft) % 2 == 1, -1.0, 1.0).astype(np.complex64))


def test_a_row_depends_on_its_magnitudes_alone(O, golden_dir):
    p, plan, B, T, mag, at = _case(O, golden_dir, "specialised")
    S = plan.pack_magnitudes(torch.from_numpy(np.nan_to_num(mag)).cuda())  # (a NaN magnitude makes a NaN row: nothing to compare)
    n_iter = 2
    base = plan.griffinlim(S, B, T, n_iter, 0.99, peak_start=True, seed=1)
    assert bool(torch.isfinite(base).all()) and min(float(base[r].abs().max()) for r in range(B)) > 0
    per_row = T * plan.frame_stride
    for r in range(B):  # a row alone, with another seed and another row_base
        Sr = S.reshape(-1)[r * per_row:(r + 1) * per_row].clone()
        alone = plan.griffinlim(Sr, 1, T, n_iter, 0.99, peak_start=True, seed=99, row_base=7)
        assert _bits(alone) == _bits(base[r:r + 1]), r
    # the same row as row 2 of 3
    order = [2, 0, 1]
    Sp = S.reshape(B, per_row)[order].contiguous()
    moved = plan.griffinlim(Sp, B, T, n_iter, 0.99, peak_start=True, seed=5, row_base=3)
    assert _bits(moved[2]) == _bits(base[1]) and _bits(moved[0]) == _bits(base[2])
    # the start itself
    a = plan.peak_start(S, B, T).reshape(B, -1)
    assert _bits(plan.peak_start(Sp, B, T).reshape(B, -1)[2]) == _bits(a[1])
    assert plan.peak_start(S, 0, T).shape == (0, plan.frame_stride)  # B == 0 is a no-op


# ---- a call with start = 1 equals the staged route ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [0, 3])
@pytest.mark.parametrize("stereo", [False, True], ids=["mono-2", "stereo-1"])
def test_fused_entries_equal_the_staged_route(golden_dir, stereo, n_iter):
    from PIL import Image

    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    p = SpectrogramParams(stereo=stereo)
    plan = _hip.get_plan(p, "cuda")
    W, seed = 37, 40
    C = 2 if stereo else 1
    if stereo:
        tile = np.array(Image.open(os.path.join(golden_dir, CLIP2 + "_stereo.png")).convert("RGB"))
        tiles = torch.from_numpy(np.ascontiguousarray(tile[None, :, 200:200 + W])).cuda()
    else:
        tiles = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(golden_dir, n + ".png")).convert("RGB"))[:, 100:100 + W]
                                           for n in ("vibes", "marim")])).cuda()
    N = tiles.shape[0]
    B = N * C
    assert B == 2
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, stereo, lut)
    lin = plan.inverse_mel(mel, C, seed=seed)
    angles = plan.peak_start(lin, B, W)
    staged = plan.griffinlim(lin, B, W, n_iter, 0.99, angles0_slots=angles, seed=seed + 1)
    assert float(staged.abs().max()) > 0
    assert plan.lib.rfx_griffinlim_form(plan.handle, B, W) == _hip.GL_FORMS["frames"]  # the per-frame form
    assert _bits(plan.griffinlim(lin, B, W, n_iter, 0.99, peak_start=True, seed=seed + 1)) == _bits(staged)
    assert _bits(plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, peak_start=True)) == _bits(staged)
    pcm3, peak3 = plan.pcm16(staged, channels=C, normalize=True)
    pcm1, peak1 = plan.audio_from_image(tiles, stereo, lut, n_iter, 0.99, seed=seed, peak_start=True)
    assert _bits(pcm1) == _bits(pcm3) and _bits(peak1) == _bits(peak3)
    # ... and differs from the random start
    assert _bits(plan.griffinlim(lin, B, W, n_iter, 0.99, seed=seed + 1)) != _bits(staged)


def test_fused_loop_call_equals_the_staged_route(golden_dir):
    from PIL import Image

    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    plan = _hip.get_plan(SpectrogramParams(), "cuda")
    W, seed, n_iter = 41, 12, 3
    tiles = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(golden_dir, n + ".png")).convert("RGB"))[:, 100:100 + W]
                                       for n in ("agile", "motorway")])).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, False, lut)
    lin = plan.inverse_mel(mel, 1, seed=seed)
    staged = plan.griffinlim(lin, 2, W, n_iter, 0.99, angles0_slots=plan.peak_start(lin, 2, W), seed=seed + 1, loop=True)
    assert staged.shape == (2, plan.hop_length * W)
    assert _bits(plan.griffinlim(lin, 2, W, n_iter, 0.99, peak_start=True, loop=True)) == _bits(staged)
    assert _bits(plan.waveform_from_mel(mel, 1, n_iter, 0.99, seed=seed, peak_start=True, loop=True)) == _bits(staged)
    pcm3, _ = plan.pcm16(staged, channels=1, normalize=True)
    assert _bits(plan.audio_from_image(tiles, False, lut, n_iter, 0.99, seed=seed, peak_start=True, loop=True)[0]) == _bits(pcm3)


def test_run_form_equals_the_staged_route():
    """the smallest batch of T = 37 frames the specialised engine decodes on the run form"""
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    plan = _hip.get_plan(SpectrogramParams(), "cuda")
    T = 37
    B = next(b for b in range(1, 4096) if plan.lib.rfx_griffinlim_form(plan.handle, b, T) == _hip.GL_FORMS["runs"])
    assert plan.lib.rfx_griffinlim_form(plan.handle, B - 1, T) == _hip.GL_FORMS["frames"]
    print(f"run form from B = {B} rows of {T} frames on")
    row = torch.from_numpy(np.nan_to_num(inputs.crafted_row(plan.n_stft, T, seed=4)[0]))
    g = torch.Generator().manual_seed(6)
    mag = row[None] * (0.5 + torch.rand(B, plan.n_stft, 1, generator=g))  # every row its own spectrum, smooth over time
    S = plan.pack_magnitudes(mag.cuda())
    del mag
    for n_iter in (0, 3):
        staged = plan.griffinlim(S, B, T, n_iter, 0.99, angles0_slots=plan.peak_start(S, B, T))
        assert _bits(plan.griffinlim(S, B, T, n_iter, 0.99, peak_start=True, seed=3, row_base=11)) == _bits(staged)
    plan.release_workspaces()


@pytest.mark.parametrize("name,lstsq", [("row-family-48k", False), ("row-family-48k", True), ("8k-64-filters", False), ("generic-11025", False)],
                         ids=["row-family-48k-sgd", "row-family-48k-lstsq", "8k-64-filters-sgd", "generic-11025-sgd"])
def test_fused_call_on_the_generic_engines_equals_the_staged_route(name, lstsq):
    """at 48 kHz the SGD stage of the fused call leaves the magnitudes in the row family's slot order: the start reads them through the
    position table; the closed form leaves plain frames, and so does the SGD stage wherever it cannot write that order"""
    p, plan, B, _ = _plan(name)
    T, n_iter, seed = 24, 3, 11  # (an iteration reflect-pads by n_fft / 2: hop (T - 1) must exceed it, 22 frames at 8 kHz)
    mel = torch.rand(B, plan.n_mels, T, generator=torch.Generator().manual_seed(4)).cuda() * 1e6
    lin = plan.inverse_mel_lstsq(mel) if lstsq else plan.inverse_mel(mel, 1, seed=seed)
    staged = plan.griffinlim(lin, B, T, n_iter, 0.99, angles0_slots=plan.peak_start(lin, B, T))
    assert float(staged.abs().max()) > 0
    assert _bits(plan.griffinlim(lin, B, T, n_iter, 0.99, peak_start=True)) == _bits(staged)
    assert _bits(plan.waveform_from_mel(mel, 1, n_iter, 0.99, seed=seed, lstsq=lstsq, peak_start=True)) == _bits(staged)


# ---- the struct: start = 0, the workspace, the refusals on a live plan -------------------------------------------------------------------

def test_start_zero_changes_nothing_and_short_workspaces_are_refused(O, golden_dir):
    from riffusion import _hip
    from riffusion.util import image_util

    p, plan, B, T, mag, at = _case(O, golden_dir, "specialised")
    lib = plan.lib
    S = plan.pack_magnitudes(torch.from_numpy(np.nan_to_num(mag)).cuda())
    L = plan.output_samples(T)
    stream = _hip.current_stream(torch.device("cuda"))
    need = helpers.need(lib, "griffinlim", plan.handle, B, T, start=1)
    base = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)
    angles_bytes = -(-B * T * plan.frame_stride * 8 // 256) * 256
    assert need == base + angles_bytes + lib.rfx_peak_start_workspace_bytes(plan.handle, B, T)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(opt, ws_bytes, angles0=None):
        out = torch.full((B, L), 123.0, device="cuda")
        rc = lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), angles0, 5, B, T, 2, 0.99, out.data_ptr(), ws.data_ptr(), ws_bytes, stream, ctypes.byref(opt), None)
        torch.cuda.synchronize()
        return rc, out

    def start_opt(start, **kw):
        f = dict(d_guide=None, d_pairs=None, d_bins=None, reserved6=0)
        f.update(kw)
        return _hip.RfxStartCallOptions(ctypes.sizeof(_hip.RfxStartCallOptions), 0, 2, 0.0, 0.0, f["d_guide"], L if f["d_guide"] else 0, L if f["d_guide"] else 0, 0,
                                        f["d_pairs"], 0, f["d_bins"], plan.hold_mask_words if f["d_bins"] else 0, 0, 0, 0, start, f["reserved6"])

    loop_sized = _hip.RfxLoopCallOptions(ctypes.sizeof(_hip.RfxLoopCallOptions), 0, 2, 0.0, 0.0, None, 0, 0, 0, None, 0, None, 0, 0, 0, 0)
    rc0, want = call(loop_sized, base)
    rc1, got = call(start_opt(0), base)  # start = 0 takes the unflagged workspace and gives the unflagged bytes
    assert rc0 == 0 == rc1 and _bits(got) == _bits(want) and not bool((got == 123.0).all())
    rc, out = call(start_opt(1), need - 1)
    assert rc == -3 and b"workspace too small" in lib.rfx_last_error() and bool((out == 123.0).all())
    rc, peaks_out = call(start_opt(1), need)
    assert rc == 0 and _bits(peaks_out) == _bits(plan.griffinlim(S, B, T, 2, 0.99, peak_start=True)) != _bits(want)
    # the refusals on a live plan: nothing is launched, the output stays
    g = torch.zeros(B, L, device="cuda")
    pairs = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    bits = torch.zeros((B, T, plan.hold_mask_words), dtype=torch.int32, device="cuda")
    A = torch.zeros(B * T * plan.frame_stride, dtype=torch.complex64, device="cuda")
    for opt, angles0, word in ((start_opt(2), None, b"start must be 0 or 1"), (start_opt(1, reserved6=1), None, b"reserved6"),
                               (start_opt(1, d_guide=g.data_ptr()), None, b"d_guide"), (start_opt(1), A.data_ptr(), b"d_angles0_slots"),
                               (start_opt(1, d_guide=g.data_ptr(), d_pairs=pairs.data_ptr()), None, b"d_hold_frames"),
                               (start_opt(1, d_guide=g.data_ptr(), d_bins=bits.data_ptr()), None, b"d_hold_bins")):
        rc, out = call(opt, need, angles0)
        assert rc == -1 and word in lib.rfx_last_error() and bool((out == 123.0).all()), word
    # the fused entries' queries
    mel = torch.rand(B, plan.n_mels, T, generator=torch.Generator().manual_seed(1)).cuda() * 1e6
    opt = start_opt(1)
    opt.row_base = 0
    need_w = helpers.need(lib, "waveform_from_mel", plan.handle, B, T, start=1)
    assert need_w == lib.rfx_waveform_from_mel_workspace_bytes(plan.handle, B, T) + need - base
    ws_w = torch.empty(need_w, dtype=torch.uint8, device="cuda")
    out = torch.full((B, L), 123.0, device="cuda")
    args = (plan.handle, mel.data_ptr(), B, T, 1, 3, 2, 0.99, out.data_ptr(), ws_w.data_ptr())
    assert lib.rfx_waveform_from_mel_ex(*args, need_w - 1, stream, ctypes.byref(opt)) == -3
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())
    assert lib.rfx_waveform_from_mel_ex(*args, need_w, stream, ctypes.byref(opt)) == 0
    assert _bits(out) == _bits(plan.waveform_from_mel(mel, 1, 2, 0.99, seed=3, peak_start=True))
    need_a = helpers.need(lib, "audio_from_image", plan.handle, B, 0, T, start=1)
    assert need_a == lib.rfx_audio_from_image_workspace_bytes(plan.handle, B, 0, T) + need - base
    ws_a = torch.empty(need_a, dtype=torch.uint8, device="cuda")
    tiles = torch.randint(0, 256, (B, plan.n_mels, T, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    pcm = torch.full((B, L, 1), 77, dtype=torch.int16, device="cuda")
    peak = torch.zeros(B, device="cuda")
    args = (plan.handle, tiles.data_ptr(), B, T, 0, lut.data_ptr(), 3, 2, 0.99, 1, peak.data_ptr(), pcm.data_ptr(), ws_a.data_ptr())
    assert lib.rfx_audio_from_image_u8_ex(*args, need_a - 1, stream, ctypes.byref(opt)) == -3
    torch.cuda.synchronize()
    assert bool((pcm == 77).all())
    assert lib.rfx_audio_from_image_u8_ex(*args, need_a, stream, ctypes.byref(opt)) == 0
    assert _bits(pcm) == _bits(plan.audio_from_image(tiles, False, lut, 2, 0.99, seed=3, peak_start=True)[0])
    # the timed form keeps n_iter + 1 entries
    ms = (ctypes.c_float * 4)(-1, -1, -1, -7)
    plan.griffinlim(S, B, T, 2, 0.99, peak_start=True, launch_ms=ms)
    assert all(ms[i] > 0 for i in range(3)) and ms[3] == -7


# ---- the product path ----------------------------------------------------------------------------------------------------------------------

def _tiles(golden_dir, W=64):
    from PIL import Image

    return np.stack([np.array(Image.open(os.path.join(golden_dir, n + ".png")).convert("RGB"))[:, 100:100 + W] for n in TILES])


def test_product_decode_has_a_lower_error_than_the_random_start_at_two_iterations(golden_dir):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramImageConverter(SpectrogramParams(), device="cuda")
    tiles = _tiles(golden_dir)
    pcm_p, err_p = conv.audio_from_spectrogram_images(tiles, phase_start="peaks", griffin_lim_iters=2, return_error=True, seed=3)
    pcm_r, err_r = conv.audio_from_spectrogram_images(tiles, phase_start="random", griffin_lim_iters=2, return_error=True, seed=3)
    for name, a, b in zip(TILES, err_p, err_r):
        print(f"{name}: spectral convergence at 2 iterations, peaks {a:.4f} random {b:.4f}")
    assert pcm_p.shape == pcm_r.shape == (5, conv.p.hop_length * 63, 1)
    assert (err_p < err_r).all()
    # the default is the random start, unchanged
    assert np.array_equal(conv.audio_from_spectrogram_images(tiles, griffin_lim_iters=2, seed=3), pcm_r)
    # return_error's staged route gives the fused route's bytes
    assert np.array_equal(conv.audio_from_spectrogram_images(tiles, phase_start="peaks", griffin_lim_iters=2, seed=3), pcm_p)


def test_chunks_give_the_same_pcm_and_the_other_entries_take_the_start(golden_dir):
    from PIL import Image

    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramImageConverter(SpectrogramParams(num_griffin_lim_iters=2), device="cuda")
    tiles = _tiles(golden_dir, 40)[:3]
    whole = conv.audio_from_spectrogram_images(tiles, phase_start="peaks", seed=8, tiles_per_call=3)
    assert np.array_equal(conv.audio_from_spectrogram_images(tiles, phase_start="peaks", seed=8, tiles_per_call=1), whole)
    assert not np.array_equal(conv.audio_from_spectrogram_images(tiles, seed=8, tiles_per_call=3), whole)
    # with the closed-form InverseMelScale nothing random is left: the seed changes nothing
    a = conv.audio_from_spectrogram_images(tiles, phase_start="peaks", seed=1, inverse_mel="lstsq")
    assert np.array_equal(conv.audio_from_spectrogram_images(tiles, phase_start="peaks", seed=2, inverse_mel="lstsq", tiles_per_call=2), a)
    # the single-image entry, the sequence and the torch-level seam
    image = Image.fromarray(tiles[0])
    torch.manual_seed(5)
    seg = conv.audio_from_spectrogram_image(image, apply_filters=False, phase_start="peaks", inverse_mel="lstsq")
    assert np.array_equal(np.asarray(seg.get_array_of_samples()).reshape(-1, 1), a[0])
    joined = conv.audio_from_spectrogram_image_sequence(tiles, crossfade_s=0.0, apply_filters=False, phase_start="peaks", inverse_mel="lstsq")
    assert int(joined.frame_count()) == 3 * a.shape[1]
    sc = conv.converter
    plan = sc._plan()
    mel = torch.rand(2, plan.n_mels, 40, generator=torch.Generator().manual_seed(2)) * 1e6
    got = sc.waveform_from_mel_amplitudes(mel, seed=8, phase_start="peaks")
    assert _bits(got) == _bits(plan.waveform_from_mel(mel.cuda(), 2, 2, 0.99, seed=8, peak_start=True)) != _bits(sc.waveform_from_mel_amplitudes(mel, seed=8))
    torch.manual_seed(4)
    assert int(sc.audio_from_spectrogram(mel.numpy(), apply_filters=False, phase_start="peaks").frame_count()) == sc.p.hop_length * 39
    with pytest.raises(ValueError, match='phase_start="peaks" does not go with'):
        conv.audio_from_spectrogram_images(tiles, phase_start="peaks", guide_waveforms=np.zeros((3, 1, 100), np.float32))
    with pytest.raises(ValueError, match="peak_start does not go with"):
        plan.griffinlim(plan.pack_magnitudes(torch.rand(1, plan.n_stft, 40).cuda()), 1, 40, 2, 0.99, peak_start=True, guide=torch.zeros(1, 100, device="cuda"))


def test_cli_phase_start_writes_the_peak_decode(golden_dir, tmp_path):
    from PIL import Image

    from riffusion import cli
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.util import audio_util

    png, out = os.path.join(golden_dir, "og_beat_64.png"), str(tmp_path / "peaks.wav")
    image = Image.open(png)
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", png, "--audio", out, "--phase-start", "peaks", "--griffin-lim-iters", "2"])
    written = audio_util.PcmSegment.from_wav(out)
    conv = SpectrogramImageConverter(cli._params_from_image(image), device="cuda")
    torch.manual_seed(5)
    want = conv.audio_from_spectrogram_image(image, griffin_lim_iters=2, phase_start="peaks")
    assert np.array_equal(np.asarray(written.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    src, dst = tmp_path / "tiles", tmp_path / "clips"
    src.mkdir()
    image.save(str(src / "a.png"), exif=image.getexif(), format="PNG")
    torch.manual_seed(5)
    cli.main(["images-to-audio-batch", "--image-dir", str(src), "--output-dir", str(dst), "--phase-start", "peaks", "--griffin-lim-iters", "2"])
    batch = audio_util.PcmSegment.from_wav(str(dst / "a.wav"))
    assert np.array_equal(np.asarray(batch.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
