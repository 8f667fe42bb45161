"""
CPU checks of the windowed-sinc resampler and of the pitch shift's host side (include/rfx.h "SINC RESAMPLE", "PITCH SHIFT";
csrc/rfx_resample_core.h).

* The oracles (tests/resample_oracle.py): the sparse float64 form equals the dense transcription of torchaudio's two functions to
  1e-15 relative (of the result's largest sample) on 2/1, 1/2, 55/49, 160/147 and 147/160, and every tap it drops is below 1e-30 in
  the dense float64 kernel.
* rfx_resample_sinc_frames and rfx_resample_sinc_table (host only) against the sparse oracle's, for those pairs plus 7787/7350 and
  33037/44100: K; `first` and ntaps exactly; every weight the float64 weight rounded to float32, to one unit in the last place (the
  library's sine and cosine are libm's, the oracle's numpy's); zero past a phase's run.  The emulator's table is the library's bit
  for bit.  The cap: every integer semitone shift within +-12 at 8 to 96 kHz gets a table; a pair past the cap is refused with -4.
* tests/emu/rfx_resample_emu.cpp runs the core's own sum on the host.  PARITY, as on the device (tests/test_gpu_resample.py): every
  figure is an SNR against the float64 oracle, all printed;
      emu >= f32         the all-float32 transcription, what functional.resample computes on a float32 waveform: outright
      emu >= k64 - 6 dB  the float64 kernel rounded to float32, what transforms.Resample computes: the project's rule
  L = 5 (shorter than the filter), 2000 and 3001; B = 3, the last row all zero.  33037/44100 has no dense kernel (11.7 GB): its two
  float32 figures are the sparse float32 forms of tests/resample_oracle.py - the same kernels on the kept taps, a float32 sum in
  ascending order.  For the pairs that have both, the sparse figures are printed next to the dense ones.
* THE WIDER CASES (WIDE_CASES, apart from PAIRS x LENGTHS): 4/1 and 12/1 (n = 1: one phase of 49 and 145 taps), 1/4 and 1/12 (o = 1),
  3/2, 44099/44100 and 44100/44099 (44100 and 44099 phases) at L = 1, 2, 255, 1000; (lowpass_filter_width, rolloff) = (1, 0.99),
  (16, 0.99), (64, 0.9476), (6, 1.0), (6, 0.5) at 55/49, 1/2 and 2/1, L = 1000 (3 to 271 taps); 160/147 at L = 277 .. 280, K = 255 .. 258
  around a workgroup's 256 outputs.  The table assertions above, and the emulator's two gates against the sparse float32 forms.
* Exact properties of the emulator: the zero row, a row alone, x * 2^+-40, the delay by o samples, a row read as zero past `valid`.
* Refusals of the entries without a device; include/rfx.h as C99; the Python layers' refusals (kaiser, requires_grad, steps).
* The emulator and a `main` of its own are also built as a stand-alone program with -fsanitize=address,undefined and run; nothing
  sanitized is loaded into Python.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import resample_oracle as RO
from engines import bits as _bits
from helpers import snr_db
from resample_cases import (DENSE, DENSE_PAIRS, EMU_SRC, LENGTHS, PAIRS, SEAM_LENGTHS, WIDE_CASES, WIDE_IDS, WIDE_TABLES, emulator, gates, run_emu,
                            sparse_figures, table64, wave, wide_gates)

EMU_MAIN = "rfx_resample_emu_main.cpp"


@pytest.fixture(scope="module")
def emu():
    return emulator()


# ---- the oracles ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", DENSE_PAIRS)
def test_sparse_oracle_is_the_dense_one(orig, new):
    for L in LENGTHS:
        x = wave(L)
        dense = RO.dense_resample(x, orig, new, torch.float64)
        sparse = RO.sparse_resample(x, orig, new, table=table64(orig, new))
        assert dense.shape == sparse.shape == (3, RO.frames(L, orig, new))
        err = float((dense - sparse).abs().max() / dense.abs().max())
        print(f"{orig}/{new} L{L}: sparse against dense {err:.2e}")
        assert err <= 1e-15


@pytest.mark.parametrize("orig,new", DENSE)
def test_every_dropped_tap_is_below_1e_30(orig, new):
    o, n, _, width = RO.geometry(orig, new)
    k64, w = RO.dense_kernel(orig, new, torch.float64)
    assert w == width and tuple(k64.shape) == (n, 1, 2 * width + o)
    k64 = k64[:, 0, :].numpy()
    first, count, wts = table64(orig, new)
    i = np.arange(2 * width + o)[None, :]
    kept = (i >= (first + width)[:, None]) & (i < (first + width + count)[:, None])
    dropped = np.abs(k64[~kept])
    print(f"{orig}/{new}: {kept.sum(1).min()}..{kept.sum(1).max()} of {2 * width + o} taps kept, largest dropped {dropped.max():.2e}")
    assert dropped.max() < 1e-30
    # ... and the kept ones are the dense kernel's values (to a few units of float64: torch's sine and cosine against numpy's)
    for p in range(0, n, max(1, n // 97)):
        assert np.allclose(k64[p, first[p] + width:first[p] + width + count[p]], wts[:count[p], p], rtol=1e-13, atol=1e-17)


# ---- the host entries ----------------------------------------------------------------------------------------------------------------------

def _frames_and_table(emu, orig, new, lpw=6, rolloff=0.99):
    from riffusion import _hip

    o, n, _, _ = RO.geometry(orig, new)
    for L in (1, 2, 5, 2000, 3001, 225351, 2 ** 24 + 1):
        assert _hip.resample_sinc_frames(L, orig, new) == RO.frames(L, orig, new) == emu.emu_rs_frames(L, orig, new), L
    first64, count, w64 = table64(orig, new, lpw, rolloff)
    first, taps = _hip.resample_sinc_table(orig, new, lpw, rolloff)
    assert first.dtype == np.int32 and taps.dtype == np.float32 and taps.shape == w64.shape == (int(count.max()), n)
    assert np.array_equal(first, first64)
    past = np.arange(taps.shape[0])[:, None] >= count[None, :]
    assert not taps[past].any()  # zero past a phase's run
    want = w64.astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(taps - want) <= ulp).all()  # the float64 weight, rounded once (sine and cosine from two libraries)
    assert (taps != want).mean() < 1e-3
    # the emulator's table is the library's
    n2, nt2 = ctypes.c_int32(0), ctypes.c_int32(0)
    f2, t2 = np.zeros_like(first), np.zeros_like(taps)
    assert emu.emu_rs_table(orig, new, lpw, rolloff, f2.ctypes.data, t2.ctypes.data, ctypes.byref(n2), ctypes.byref(nt2)) == 0
    assert (n2.value, nt2.value) == (n, taps.shape[0]) and f2.tobytes() == first.tobytes() and t2.tobytes() == taps.tobytes()
    return taps.shape[0]


@pytest.mark.parametrize("orig,new", PAIRS)
def test_frames_and_table_are_the_oracles(emu, orig, new):
    _frames_and_table(emu, orig, new)


@pytest.mark.parametrize("orig,new,lpw,rolloff", WIDE_TABLES, ids=[f"{o}/{n}-lpw{w}-rolloff{r:.4g}" for o, n, w, r in WIDE_TABLES])
def test_frames_and_table_of_the_wide_cases(emu, orig, new, lpw, rolloff):
    """one phase (n = 1), o = 1, 44100 phases, and the filters other than 6 / 0.99: the same assertions"""
    ntaps = _frames_and_table(emu, orig, new, lpw, rolloff)
    print(f"{orig}/{new} lpw {lpw} rolloff {rolloff:.4g}: {RO.geometry(orig, new)[1]} phases of {ntaps} taps")
    for L, K in SEAM_LENGTHS.items():
        assert RO.frames(L, 160, 147) == K


def test_every_semitone_shift_gets_a_table_below_the_cap():
    """orig = int(sr / 2^(-s / 12)) -> sr for s in -12 .. 12 at the usual rates from 8 to 96 kHz, sized without building the table"""
    from riffusion import _hip

    lib = _hip.load_library()
    most = 0
    for sr in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000):
        for s in range(-12, 13):
            orig = int(sr / 2.0 ** (-s / 12))
            n, nt = ctypes.c_int32(0), ctypes.c_int32(0)
            assert lib.rfx_resample_sinc_table(orig, sr, 6, 0.99, None, None, 0, ctypes.byref(n), ctypes.byref(nt)) == 0, (sr, s, lib.rfx_last_error())
            assert 13 <= nt.value <= 25, (sr, s, nt.value)
            most = max(most, 4 * n.value * nt.value)
    print(f"largest table {most / 2 ** 20:.2f} MiB")
    assert most <= 16 << 20


def test_refusals_without_a_device():
    from riffusion import _hip

    lib = _hip.load_library()
    k = ctypes.c_int(-7)
    for L, o, n, word in ((0, 2, 1, b"L must"), (5, 0, 1, b"frequencies"), (5, 2, -1, b"frequencies"), (2 ** 31 - 1, 1, 2, b"2^31")):
        assert lib.rfx_resample_sinc_frames(L, o, n, ctypes.byref(k)) == -1 and k.value == -7
        assert b"rfx_resample_sinc_frames: " in lib.rfx_last_error() and word in lib.rfx_last_error(), (L, o, n)
    assert lib.rfx_resample_sinc_frames(5, 2, 1, None) == -1
    assert lib.rfx_resample_sinc_frames(5, 2, 1, ctypes.byref(k)) == 0 and k.value == 3
    n, nt = ctypes.c_int32(-7), ctypes.c_int32(-7)
    f, t = np.full(64, 9, np.int32), np.full(64 * 32, 9, np.float32)
    table = lib.rfx_resample_sinc_table
    for args in ((0, 1, 6, 0.99), (1, 0, 6, 0.99), (2, 1, 0, 0.99), (2, 1, 6, 0.0), (2, 1, 6, 1.5), (2, 1, 6, float("nan"))):
        assert table(*args, f.ctypes.data, t.ctypes.data, t.size, ctypes.byref(n), ctypes.byref(nt)) == -1, args
    assert table(55, 49, 6, 0.99, f.ctypes.data, None, t.size, ctypes.byref(n), ctypes.byref(nt)) == -1 and b"go together" in lib.rfx_last_error()
    assert table(55, 49, 6, 0.99, f.ctypes.data, t.ctypes.data, 49 * 14 - 1, ctypes.byref(n), ctypes.byref(nt)) == -1 and b"capacity" in lib.rfx_last_error()
    assert table(55, 49, 6, 0.99, None, None, 0, None, ctypes.byref(nt)) == -1
    # past the cap: RFX_ERR_UNSUPPORTED with the cap in the message, before and after the walk over the phases
    assert table(1, 2 ** 23 + 1, 6, 0.99, None, None, 0, ctypes.byref(n), ctypes.byref(nt)) == -4 and b"16 MiB" in lib.rfx_last_error()
    assert table(999983, 1000003, 6, 0.99, None, None, 0, ctypes.byref(n), ctypes.byref(nt)) == -4 and b"16 MiB" in lib.rfx_last_error()
    assert (n.value, nt.value) == (-7, -7) and (f == 9).all() and (t == 9).all()  # the outputs untouched
    assert table(55, 49, 6, 0.99, None, None, 0, ctypes.byref(n), ctypes.byref(nt)) == 0 and (n.value, nt.value) == (49, 14)
    # the device entries: B == 0 is a no-op, B < 0 and a NULL pointer are refusals, under the entry's name
    assert lib.rfx_resample_sinc(None, 0, 5, 2, 1, None, None, 0, None, None) == 0
    assert lib.rfx_resample_sinc(None, 1, 5, 2, 1, None, None, 0, None, None) == -1 and b"rfx_resample_sinc: null" in lib.rfx_last_error()
    assert lib.rfx_resample_sinc(None, -1, 5, 2, 1, None, None, 0, None, None) == -1
    x = np.zeros(64, np.float32)
    bad = lib.rfx_resample_sinc
    assert bad(x.ctypes.data, 1, 5, 0, 1, f.ctypes.data, t.ctypes.data, 25, x.ctypes.data + 128, None) == -1 and b"frequencies" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 0, 2, 1, f.ctypes.data, t.ctypes.data, 25, x.ctypes.data + 128, None) == -1 and b"L must" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 2 ** 31 - 1, 1, 2, f.ctypes.data, t.ctypes.data, 13, x.ctypes.data + 128, None) == -1 and b"2^31" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 5, 2, 1, None, t.ctypes.data, 25, x.ctypes.data + 128, None) == -1 and b"null" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 5, 2, 1, f.ctypes.data, t.ctypes.data, 0, x.ctypes.data + 128, None) == -1 and b"ntaps" in lib.rfx_last_error()
    assert bad(x.ctypes.data + 2, 1, 5, 2, 1, f.ctypes.data, t.ctypes.data, 25, x.ctypes.data + 128, None) == -1 and b"aligned" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 5, 2, 1, f.ctypes.data + 2, t.ctypes.data, 25, x.ctypes.data + 128, None) == -1 and b"aligned" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 8, 2, 1, f.ctypes.data, t.ctypes.data, 25, x.ctypes.data + 16, None) == -1 and b"overlap" in lib.rfx_last_error()
    assert bad(x.ctypes.data, 1, 5, 1, 2 ** 23 + 1, f.ctypes.data, t.ctypes.data, 13, x.ctypes.data + 128, None) == -4 and b"16 MiB" in lib.rfx_last_error()
    assert not x.any()
    assert lib.rfx_pitch_shift(None, None, 0, 20000, 2.0, 12, None, None, 0, None, None, 0, None) == 0
    assert lib.rfx_pitch_shift(None, None, 1, 20000, 2.0, 12, None, None, 0, None, None, 0, None) == -1 and b"rfx_pitch_shift: null" in lib.rfx_last_error()
    assert lib.rfx_pitch_shift(None, None, -1, 20000, 2.0, 12, None, None, 0, None, None, 0, None) == -1
    assert lib.rfx_pitch_shift_workspace_bytes(None, 1, 20000, 2.0, 12) == 0 and lib.rfx_pitch_shift_resample_freq(None, 20000, 2.0, 12) == 0
    for bad_steps in (float("nan"), float("inf"), "2", True, torch.tensor(2.0), [2.0, 3.0]):
        with pytest.raises(ValueError, match="n_steps"):
            _hip.check_pitch_steps(bad_steps)
    for bad_bins in (0, -12, 12.0, True):
        with pytest.raises(ValueError, match="bins_per_octave"):
            _hip.check_pitch_steps(2, bad_bins)
    assert _hip.check_pitch_steps(2) == (2.0, 12) and _hip.check_pitch_steps(-0.5, 24) == (-0.5, 24)


def test_header_compiles_as_c99_with_the_entries(tmp_path):
    emu_build.header_compiles_as_c99(
        tmp_path,
        '#include "rfx.h"\n'
        "size_t q(const rfx_plan* p) { return rfx_pitch_shift_workspace_bytes(p, 1, 20000, 2.0, 12) + (size_t)rfx_pitch_shift_resample_freq(p, 20000, 2.0, 12)"
        " + RFX_RESAMPLE_MAX_TABLE_BYTES; }\n"
        "int r(int32_t* f, float* t, int32_t* n, int* k) {\n"
        "  return rfx_resample_sinc_frames(5, 2, 1, k) + rfx_resample_sinc_table(2, 1, 6, 0.99, f, t, 25, n, n) + rfx_resample_sinc(t, 1, 5, 2, 1, f, t, 25, t, 0); }\n"
        "int s(const rfx_plan* p, float* x, int32_t* f, void* ws) { return rfx_pitch_shift(p, x, 1, 20000, -5.0, 12, f, x, 13, x, ws, 0, 0); }\n")


# ---- the emulator --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("orig,new", PAIRS)
def test_parity_of_the_emulator(emu, orig, new, L):
    r64, f32, k64 = gates(orig, new, L)
    y = run_emu(emu, wave(L), orig, new)
    e = snr_db(r64[:-1], y[:-1])
    s32, s64 = sparse_figures(orig, new, L)
    print(f"{orig}/{new} L{L}: emu {e:.1f} dB, all-float32 {f32:.1f} dB, float32-rounded kernel {k64:.1f} dB (sparse float32 forms: {s32:.1f}, {s64:.1f} dB)")
    assert tuple(y.shape) == tuple(r64.shape) and torch.isfinite(y).all()
    assert not y[-1].any()  # the zero row leaves as zeros
    assert e >= f32, (orig, new, L, e, f32)
    assert e >= k64 - 6.0, (orig, new, L, e, k64)


@pytest.mark.parametrize("orig,new,L,lpw,rolloff", WIDE_CASES, ids=WIDE_IDS)
def test_parity_of_the_emulator_at_the_wide_cases(emu, orig, new, L, lpw, rolloff):
    """the two gates of test_parity_of_the_emulator against the sparse float32 forms; several L = 1 and L = 2 cases are equalities"""
    r64, f32, k64 = wide_gates(orig, new, L, lpw, rolloff)
    x = wave(L)
    y = run_emu(emu, x, orig, new, lpw=lpw, rolloff=rolloff)
    e = snr_db(r64[:-1], y[:-1])
    print(f"{orig}/{new} L{L} lpw {lpw} rolloff {rolloff:.4g}: K {y.shape[1]}, emu {e:.1f} dB, all-float32 {f32:.1f} dB, float32-rounded kernel {k64:.1f} dB")
    assert tuple(y.shape) == tuple(r64.shape) == (3, RO.frames(L, orig, new)) and torch.isfinite(y).all()
    assert not y[-1].any()  # the zero row leaves as zeros
    assert e >= f32, (orig, new, L, e, f32)
    assert e >= k64 - 6.0, (orig, new, L, e, k64)
    for r in (0, 2):
        assert _bits(run_emu(emu, x[r:r + 1], orig, new, lpw=lpw, rolloff=rolloff)) == _bits(y[r:r + 1]), r


@pytest.mark.parametrize("orig,new", PAIRS)
def test_exact_properties_of_the_emulator(emu, orig, new):
    o, n, _, _ = RO.geometry(orig, new)
    for L in (5, 2000):
        x = wave(L)
        y = run_emu(emu, x, orig, new)
        for r in (0, 2):
            assert _bits(run_emu(emu, x[r:r + 1], orig, new)) == _bits(y[r:r + 1]), (L, r)
        for e in (40, -40):
            assert _bits(run_emu(emu, x * 2.0 ** e, orig, new)) == _bits(y * 2.0 ** e), (L, e)
        xd = torch.nn.functional.pad(x, (o, 0))  # delayed by o samples: the output is delayed by n
        yd = run_emu(emu, xd, orig, new)
        assert yd.shape[1] == y.shape[1] + n and _bits(yd[:, n:]) == _bits(y)
        # a row read as zero past `valid` gives the bits of the row padded with zeros (the pitch shift's cut and pad)
        xz = x.clone()
        xz[:, L // 2:] = 0
        assert _bits(run_emu(emu, x, orig, new, valid=L // 2)) == _bits(run_emu(emu, xz, orig, new))


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------------

def test_python_refusals_before_any_device_work():
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    x = torch.zeros(2, 3000)
    with pytest.raises(ValueError, match="kaiser"):
        audio_util.resample_waveform(x, 48000, 44100, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError, match="positive integers"):
        audio_util.resample_waveform(x, 0, 44100)
    with pytest.raises(ValueError, match="positive integers"):
        audio_util.resample_waveform(x, 48000.5, 44100)
    with pytest.raises(RuntimeError, match="no backward"):
        audio_util.resample_waveform(x.clone().requires_grad_(), 48000, 44100)
    c = SpectrogramConverter(SpectrogramParams(), device="cpu")  # (no plan on the CPU: a call that reached for one would say so)
    w = torch.zeros(2, 20000, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        c.pitch_shift(w, 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):  # grad mode off: the rule does not apply, the call goes on to the plan
        c.pitch_shift(w, 2)
    for bad in (float("nan"), torch.tensor(2.0), "2"):
        with pytest.raises(ValueError, match="n_steps"):
            c.pitch_shift(w.detach(), bad)
    with pytest.raises(ValueError, match="bins_per_octave"):
        c.pitch_shift(w.detach(), 2, bins_per_octave=0)


def test_command_line_argument_checks(capsys):
    from riffusion import cli

    assert cli._semitones(semitones="-5") == -5.0 and cli._semitones(semitones=0.5) == 0.5
    for flags in (["--semitones", "nan"], ["--semitones", "inf"], ["--semitones", "two"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["pitch-shift", "--audio", "missing.wav", "--output", "out.wav"] + flags)
        assert e.value.code == 2, flags
        assert "--semitones" in capsys.readouterr().err, flags
    with pytest.raises(SystemExit):  # --semitones is required
        cli.main(["pitch-shift", "--audio", "missing.wav", "--output", "out.wav"])


# ---- the sanitized stand-alone program ---------------------------------------------------------------------------------------------------------

def test_sanitized_stand_alone_emulator():
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program; the sanitizers'
    runtimes are linked statically, so the program carries them itself"""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-ffp-contract=off", "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr
