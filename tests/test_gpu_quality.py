"""
rfx_spectral_error on the device (csrc/rfx_quality.hip) and what is built on it: Plan.spectral_error,
SpectrogramConverter.spectral_convergence and `return_error` of the batch decode.

Shapes: per geometry the smallest T whose waveform is longer than the forward transform's reflect padding (n_fft / 2), and T = 33
(no multiple of the 16-frame Griffin-Lim group nor of the reduction's 4-frame chunk); the default 44.1 kHz plan (specialised
engine, slot layout), 48 kHz and 8 kHz (row family; 8 kHz is the smallest n_fft of tests/test_gpu_generic_geometry.py) and the
odd n_fft = 3465 of that file (generic FFT engine, the smallest it serves there).

Bounds.  Exact known answers and batch invariance are bit equality.  Against numpy float64: relative n * 2^-52, n = n_stft * T
elements, the worst case of any summation order of non-negative terms (tests/test_quality_cpu.py).  Against the CPU oracle's
float32 figure: ORACLE_MULTIPLE below.
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import oracle

pytestmark = pytest.mark.gpu

GIB = 1 << 30
GROUP_BYTES = 128 << 20  # include/rfx.h: rows are walked in groups of at most this many bytes of magnitudes
TILES = ["og_beat", "agile", "marim", "motorway", "vibes"]
# Against the oracle the bound is not a constant: the oracle's own float32-vs-float64 distance for this figure (torch.stft and
# both norms in float32, against the same formula in float64) depends on the input and on the host's torch build and thread
# count - 1.3e-6 .. 8.8e-6 relative on 4-iteration Griffin-Lim results of ten 64-column ranges of the golden tiles on one host,
# 6.0e-5 for og_beat [100:164] on another.  The test measures it on its own five inputs, on the host it runs on, and allows
# ORACLE_MULTIPLE times the largest of the five: the device figure and the oracle's float32 figure each lie within that distance
# of the float64 figure (the device's far closer - its transform is float32 too, but its sums are double), hence within twice
# of it of each other.
ORACLE_MULTIPLE = 2.0

GEOMETRIES = {
    "44k": {},
    "48k": dict(sample_rate=48000),
    "8k": dict(sample_rate=8000, max_frequency=4000),
    "odd3465": dict(sample_rate=34650, padded_duration_ms=100, window_duration_ms=100, max_frequency=8000),
}
ENGINE_OF = {"44k": "specialised", "48k": "row-family", "8k": "row-family", "odd3465": "generic"}


@pytest.fixture(scope="module")
def O():
    return oracle()


def _params(**kw):
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramParams(**kw)


def _plan(**kw):
    from riffusion import _hip

    return _hip.get_plan(_params(**kw), "cuda:0")


def _samples(plan, T):
    return plan.lib.rfx_griffinlim_output_samples(plan.handle, T)


def _smallest_T(plan):
    T = 2
    while _samples(plan, T) <= plan.n_fft // 2:
        T += 1
    return T


def _bits(t: torch.Tensor) -> bytes:
    return t.detach().cpu().contiguous().numpy().tobytes()


_cases = {}


def _case(geom: str, which: str):
    """(plan, B, T, wave (B, L), a = the plan's magnitudes of wave, m = a random target, sums) computed once per shape"""
    key = (geom, which)
    if key not in _cases:
        plan = _plan(**GEOMETRIES[geom])
        assert plan.griffinlim_engine == ENGINE_OF[geom]
        T = _smallest_T(plan) if which == "min" else 33
        B, L = 3, _samples(plan, T)
        assert L > plan.n_fft // 2 and plan.lib.rfx_stft_frames(plan.handle, L) == T
        g = torch.Generator(device="cuda").manual_seed(len(geom) * 100 + T)
        wave = torch.randn((B, L), device="cuda", generator=g) * 8000.0
        a, _, Tn = plan.stft(wave, True, False)
        assert Tn == T
        m = plan.pack_magnitudes(torch.rand((B, plan.n_stft, T), device="cuda", generator=g) * float(a.max()))
        sums = plan.spectral_error(wave, m, B, T)
        torch.cuda.synchronize()
        _cases[key] = (plan, B, T, wave, a, m, sums)
    return _cases[key]


SHAPES = [(g, w) for g in GEOMETRIES for w in ("min", "33")]


@pytest.mark.parametrize("geom,which", SHAPES)
def test_exact_known_answers(geom, which):
    plan, B, T, wave, a, m, sums = _case(geom, which)
    assert sums.shape == (B, 2) and sums.dtype == torch.float64 and bool((sums > 0).all())
    # the target is the waveform's own magnitudes: every difference is zero
    same = plan.spectral_error(wave, a, B, T)
    assert bool((same[:, 0] == 0.0).all()) and bool((same[:, 1] > 0).all())
    # a silent waveform: (0 - m)^2 = m^2 term by term, in the same order
    silent = plan.spectral_error(torch.zeros_like(wave), m, B, T)
    assert _bits(silent[:, 0]) == _bits(silent[:, 1]) == _bits(sums[:, 1])
    # powers of two: every float32 step of the transform and every double product and sum scales exactly
    for k in (-20, 12):
        scaled = plan.spectral_error(wave * 2.0 ** k, m * 2.0 ** k, B, T)
        assert _bits(scaled) == _bits(sums * 4.0 ** k), k


@pytest.mark.parametrize("geom,which", SHAPES)
def test_sums_against_numpy_float64(geom, which):
    plan, B, T, wave, a, m, sums = _case(geom, which)
    a64 = plan.unpack_magnitudes(a, B, T).cpu().numpy().astype(np.float64)
    m64 = plan.unpack_magnitudes(m, B, T).cpu().numpy().astype(np.float64)
    want = np.stack([((a64 - m64) ** 2).sum(axis=(1, 2)), (m64 ** 2).sum(axis=(1, 2))], axis=1)
    n = plan.n_stft * T
    rel = np.abs(sums.cpu().numpy() - want) / want
    print(f"{geom} T {T}: relative distance to numpy float64 {rel.max():.2e}, bound {n * 2.0 ** -52:.2e}")
    assert (rel <= n * 2.0 ** -52).all()


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_a_rows_bytes_do_not_depend_on_the_batch(geom):
    plan, B, T, wave, a, m, sums = _case(geom, "min")
    w0, m0 = wave[1:2], m[T:2 * T]
    alone = plan.spectral_error(w0, m0, 1, T)
    assert _bits(alone[0]) == _bits(sums[1])
    g = torch.Generator(device="cuda").manual_seed(5)
    for rows, places in ((5, (0, 4)), (64, (37,))):
        for place in places:
            wb = torch.randn((rows, wave.shape[1]), device="cuda", generator=g) * 3000.0
            mb = torch.rand((rows * T, plan.frame_stride), device="cuda", generator=g) * 1e5
            wb[place], mb[place * T:(place + 1) * T] = w0[0], m0
            got = plan.spectral_error(wb, mb, rows, T)
            assert _bits(got[place]) == _bits(alone[0]), (rows, place)


def test_rows_on_both_sides_of_a_group_boundary():
    """More rows than one group of the entry's walk holds (128 MiB of magnitudes: 162 rows of 22 frames): the rows around the
    boundary and the last one equal the same rows alone."""
    plan, _, T, wave, _, m, sums = _case("44k", "min")
    per_group = GROUP_BYTES // (T * plan.frame_stride * 4)
    B = per_group + 9
    assert plan.lib.rfx_spectral_error_workspace_bytes(plan.handle, B, T) == plan.lib.rfx_spectral_error_workspace_bytes(plan.handle, 10 * B, T)
    g = torch.Generator(device="cuda").manual_seed(6)
    wb = torch.randn((B, wave.shape[1]), device="cuda", generator=g) * 8000.0
    mb = torch.rand((B * T, plan.frame_stride), device="cuda", generator=g) * 3e5
    got = plan.spectral_error(wb, mb, B, T)
    for r in (0, per_group - 1, per_group, per_group + 1, B - 1):
        assert _bits(got[r]) == _bits(plan.spectral_error(wb[r:r + 1], mb[r * T:(r + 1) * T], 1, T)[0]), r


def _require(gib: float) -> None:
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs {gib:.0f} GiB of free device memory, {free / GIB:.1f} GiB free")


def _release(plan):
    plan.release_workspaces()
    torch.cuda.empty_cache()


def test_past_65535_rows():
    """65 543 rows of the smallest geometry in one call (the target filled in slot layout directly, padding included: it is
    not counted): the rows around 65535 equal the same rows alone."""
    _require(14)
    plan, _, T, wave, _, _, _ = _case("8k", "min")
    B, L = 65536 + 7, wave.shape[1]
    g = torch.Generator(device="cuda").manual_seed(7)
    wb = torch.randn((B, L), device="cuda", generator=g) * 8000.0
    mb = torch.rand((B * T, plan.frame_stride), device="cuda", generator=g) * 1e5
    got = plan.spectral_error(wb, mb, B, T)
    assert bool(torch.isfinite(got).all()) and bool((got > 0).all())
    for r in (0, 1, 65534, 65535, 65536, B - 1):
        assert _bits(got[r]) == _bits(plan.spectral_error(wb[r:r + 1], mb[r * T:(r + 1) * T], 1, T)[0]), r
    del wb, mb
    _release(plan)


def test_past_2_31_slot_elements():
    """448 rows of 512 frames of the default geometry: the target's float slots pass 4 GiB of byte offset at row 223 and 2^31
    elements at row 446.  The rows on both sides equal the same rows alone."""
    _require(14)
    plan = _plan()
    B, T = 448, 512
    L = _samples(plan, T)
    g = torch.Generator(device="cuda").manual_seed(8)
    wb = torch.randn((B, L), device="cuda", generator=g) * 8000.0
    mb = torch.rand((B * T, plan.frame_stride), device="cuda", generator=g) * 3e5
    got = plan.spectral_error(wb, mb, B, T)
    for r in (0, 222, 223, 224, 445, 446, 447):
        assert _bits(got[r]) == _bits(plan.spectral_error(wb[r:r + 1], mb[r * T:(r + 1) * T], 1, T)[0]), r
    del wb, mb
    _release(plan)


# ---- against the oracle ----------------------------------------------------------------------------------------------------------
def _golden_rgb(golden_dir, name):
    from riffusion.util import image_util

    with Image.open(os.path.join(golden_dir, f"{name}.png")) as im:
        return np.ascontiguousarray(np.asarray(image_util.rgb_array_from_image(im)))


def test_spectral_convergence_against_the_oracle(O, golden_dir):
    """converter.spectral_convergence against O.spectral_convergence on the same waveform and magnitudes: a 4-iteration
    Griffin-Lim result of columns [100:164] of every golden tile."""
    from riffusion.spectrogram_converter import SpectrogramConverter

    params = _params(num_griffin_lim_iters=4)
    op = O.params_from(params)
    conv = SpectrogramConverter(params, device="cuda")
    plan = conv._plan()
    n, T = len(TILES), 64
    mel = torch.from_numpy(np.concatenate([O.spectrogram_from_image_u8(_golden_rgb(golden_dir, t)[:, 100:100 + T], 0.25, False, 30e6) for t in TILES]))
    lin_slots = plan.inverse_mel(mel.cuda(), 1, seed=3)
    wave = plan.griffinlim(lin_slots, n, T, 4, 0.99, seed=4)
    lin = plan.unpack_magnitudes(lin_slots, n, T)
    got = conv.spectral_convergence(wave, lin)
    assert got.shape == (n,) and got.dtype == torch.float64
    assert _bits(got) == _bits(conv.convergence_from_sums(*plan.spectral_error(wave, lin_slots, n, T).unbind(1)))
    wave_h, lin_h = wave.cpu(), lin.cpu()
    win = O.hann_window(op).double()
    want, want64 = [], []
    for i in range(n):
        want.append(O.spectral_convergence(wave_h[i:i + 1], lin_h[i:i + 1], op))
        X = torch.stft(wave_h[i:i + 1].double(), n_fft=op.n_fft, hop_length=op.hop_length, win_length=op.win_length, window=win, center=True,
                       pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        want64.append(float(torch.linalg.norm(X.abs() - lin_h[i:i + 1].double()) / torch.linalg.norm(lin_h[i:i + 1].double())))
    oracle_distance = max(abs(a - b) / b for a, b in zip(want, want64))
    rel = [abs(float(got[i]) - want[i]) / want[i] for i in range(n)]
    for i, tile in enumerate(TILES):
        print(f"{tile}: device {float(got[i]):.9f}, oracle float32 {want[i]:.9f}, float64 {want64[i]:.9f}; device vs oracle {rel[i]:.2e}, "
              f"oracle float32 vs float64 {abs(want[i] - want64[i]) / want64[i]:.2e}, device vs float64 {abs(float(got[i]) - want64[i]) / want64[i]:.2e}")
    print(f"oracle's largest float32-vs-float64 distance on these inputs {oracle_distance:.2e}, bound {ORACLE_MULTIPLE:g} x that")
    assert oracle_distance > 0 and max(rel) <= ORACLE_MULTIPLE * oracle_distance


# ---- the product call ------------------------------------------------------------------------------------------------------------
def _tiles(golden_dir, names, width=32):
    return np.stack([_golden_rgb(golden_dir, t)[:, 100:100 + width] for t in names])


@pytest.mark.parametrize("stereo", [False, True])
def test_return_error_of_the_batch_decode(golden_dir, stereo):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    conv = SpectrogramImageConverter(_params(stereo=stereo, num_griffin_lim_iters=8), device="cuda")
    plan = conv.converter._plan()
    tiles = _tiles(golden_dir, TILES[:3])
    if stereo:  # (the golden tiles are grey: give the two channels different content)
        tiles[:, :, :, 2] = tiles[:, ::-1, :, 1]
    N, C, T, seed = 3, 2 if stereo else 1, 32, 5
    errors = []
    for per_call in (1, 2, 64):
        plain = conv.audio_from_spectrogram_images(tiles, seed=seed, tiles_per_call=per_call)
        pcm, err = conv.audio_from_spectrogram_images(tiles, seed=seed, tiles_per_call=per_call, return_error=True)
        assert isinstance(err, np.ndarray) and err.shape == (N,) and err.dtype == np.float64
        assert pcm.dtype == plain.dtype and pcm.shape == plain.shape and pcm.tobytes() == plain.tobytes(), per_call
        errors.append(err)
    assert errors[0].tobytes() == errors[1].tobytes() == errors[2].tobytes()
    assert (errors[0] > 0).all() and (errors[0] < 1).all()
    # recomputed from the float waveforms and InverseMelScale's magnitudes
    wave = conv.audio_from_spectrogram_images(tiles, seed=seed, return_waveform=True, return_device=True)
    wave_e, err_d = conv.audio_from_spectrogram_images(tiles, seed=seed, return_waveform=True, return_device=True, return_error=True)
    assert _bits(wave_e) == _bits(wave) and err_d.is_cuda and _bits(err_d) == errors[0].tobytes()
    from riffusion.util import image_util

    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(torch.from_numpy(tiles).cuda(), stereo, lut)
    lin_slots = plan.inverse_mel(mel, C, seed=seed, magnitude_hint=30e6)
    rows = wave.reshape(N * C, -1)
    sums = plan.spectral_error(rows, lin_slots, N * C, T).reshape(N, C, 2).sum(1)
    assert _bits(conv.converter.convergence_from_sums(sums[:, 0], sums[:, 1])) == errors[0].tobytes()
    per_row = conv.converter.spectral_convergence(rows, plan.unpack_magnitudes(lin_slots, N * C, T))
    if not stereo:
        assert _bits(per_row) == errors[0].tobytes()
    else:  # a clip's pooled figure lies between its channels'
        lo, hi = per_row.reshape(N, C).min(1).values.cpu().numpy(), per_row.reshape(N, C).max(1).values.cpu().numpy()
        assert (lo <= errors[0]).all() and (errors[0] <= hi).all()
    # filters, resize and the sequence call: the PCM is the PCM without the flag, the errors are those of the resized tiles
    kw = dict(seed=seed, tiles_per_call=2, apply_filters=True, size=(40, 512))
    plain = conv.audio_from_spectrogram_images(tiles, **kw)
    pcm, err = conv.audio_from_spectrogram_images(tiles, return_error=True, **kw)
    assert pcm.tobytes() == plain.tobytes() and err.shape == (N,) and (err > 0).all()
    seg = conv.audio_from_spectrogram_image_sequence(tiles, seed=seed, return_device=True, size=(40, 512))
    seg_e, err_s = conv.audio_from_spectrogram_image_sequence(tiles, seed=seed, return_device=True, size=(40, 512), return_error=True)
    assert torch.equal(seg, seg_e) and _bits(err_s) == err.tobytes()
    host_seg, host_err = conv.audio_from_spectrogram_image_sequence(tiles, seed=seed, return_error=True)
    assert isinstance(host_err, np.ndarray) and host_err.tobytes() == errors[0].tobytes() and host_seg.frame_count() > 0


def test_griffinlim_iterations_lower_the_error(golden_dir):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    tiles = _tiles(golden_dir, TILES)
    err = {}
    for iters in (0, 8):
        conv = SpectrogramImageConverter(_params(num_griffin_lim_iters=iters), device="cuda")
        err[iters] = conv.audio_from_spectrogram_images(tiles, seed=9, return_error=True)[1]
    print("spectral convergence after 0 / 8 Griffin-Lim iterations:", ", ".join(f"{t} {a:.4f} / {b:.4f}" for t, a, b in zip(TILES, err[0], err[8])))
    assert (err[8] < err[0]).all()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_return_error_refuses_a_group(golden_dir):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    conv = SpectrogramImageConverter(_params(), device="cuda")
    with pytest.raises(ValueError, match="group"):
        conv.audio_from_spectrogram_images(_tiles(golden_dir, TILES[:1]), seed=1, return_error=True, group=True)


def test_entry_refuses_before_any_launch():
    from riffusion import _hip

    plan, B, T, wave, a, m, sums = _case("44k", "min")
    lib = plan.lib
    need = lib.rfx_spectral_error_workspace_bytes(plan.handle, B, T)
    assert need > B * T * plan.frame_stride * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    stream = _hip.current_stream(plan.device)

    def call(Bc, Tc, nbytes, wave_ptr=wave.data_ptr()):
        return lib.rfx_spectral_error(plan.handle, wave_ptr, m.data_ptr(), Bc, Tc, out.data_ptr(), ws.data_ptr(), nbytes, stream)

    assert call(B, T, need - 1) == -3 and b"workspace too small" in lib.rfx_last_error()
    assert call(B, T, 0) == -3
    assert call(B, T - 1, need) == -1 and b"reflect padding" in lib.rfx_last_error()  # one frame fewer: not longer than n_fft / 2
    assert call(-1, T, need) == -1 and call(B, T, need, wave_ptr=None) == -1
    assert lib.rfx_spectral_error(plan.handle, wave.data_ptr(), m.data_ptr() + 4, B, T, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert b"aligned" in lib.rfx_last_error()
    assert lib.rfx_spectral_error(None, None, None, 0, T, None, None, 0, None) == 0  # no rows: nothing to do, nothing to check
    assert lib.rfx_spectral_error_workspace_bytes(plan.handle, 0, T) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote its output"
    assert call(B, T, need) == 0
    torch.cuda.synchronize()
    assert _bits(out) == _bits(sums)
    assert plan.spectral_error(wave[:0], m[:0], 0, T).shape == (0, 2)
    with pytest.raises(ValueError):
        plan.spectral_error(wave[:, :-1], m, B, T)
