"""
CPU checks of the time stretch (include/rfx.h, "TIME STRETCH"; csrc/rfx_vocoder_core.h, rfx_plan_core.h: vocoder_table).

* tests/emu/rfx_vocoder_emu.cpp runs the core's own walk on the host, in float32 as the kernel does (its final sine and cosine in
  double, rounded once: the host has no sincospif).  PARITY: every figure is an SNR against the float64 oracle (tests/vocoder_oracle.py, a
  transcription of torchaudio.functional.phase_vocoder): `emu` the emulator's, `o32` the float32 oracle's on the same input; both printed.
  X is seeded complex64 noise over the oracle STFT of helpers.synthetic_wave (tests/test_gpu_istft.py builds it so), the last row all
  zero; T = 2 takes the first two frames of the T = 41 spectrogram (two frames' worth of samples are too few for torch.stft's reflect
  padding).  Rates 1.25, 0.75, 1.1, 0.9; geometry: the four parameter sets of tests/engines.py.
    T = 41, T = 2            emu >= o32 - 6 dB    the project's rule (tests/test_gpu_held_frames.py)
    T = 512, defaults, B = 1 emu >= o32           no allowance: phases as wrapped turns are the point of the formulation
  THE WIDE RATES (RATES_WIDE; the oracle's step positions are the double products i * rate, tests/vocoder_oracle.py): bpm ratios whose
  products come within rounding of an integer (2/3, 4/3, 0.3, 1.2), rates >= 2 (every step takes two new frames: 2, 3, 2.5, 7.3),
  <= 0.5 (a pair stays for several steps: 0.5, 0.125) and >= T (one output frame: 40, 41, 50), at T = 41 on the four engines and at
  T = 3 and T = 1 on two; the same rule, and finite, the zero row, a row alone.  T_out >= 2 is 40 - 60 dB clear; T_out = 1 (frame 0
  through polar form and back) sits 3.7 - 5.0 dB below a float32 oracle that is at float32's rounding floor of 144 dB.
  A structured input (frames 10 .. 19 of a row exactly zero; a real bin with alternating sign; a negative real bin with -0.0 i; a purely
  imaginary bin) at 1.25, 2/3 and 3, the rule on the whole and on each of the four slices (emu 120 - 127 dB overall, >= 148 dB on the
  three bins); a step whose two frames are zero leaves as exact zeros.  A noise-free analysis (the STFT of a 440 Hz sine): emu 117 - 119
  against o32 87 - 93 dB.
* The steps: the oracle's pair and weight of every step, and the core's voc_step through the emulator, are Python's own
  floor(i * rate) and float32(i * rate - floor) at every rate of the vocoder and pitch-shift tests; torch.arange(0, T, rate) has the
  same floors at the rates the older figures were recorded at and other floors at 2/3, 4/3, 0.3 and 1.2 (with the oracle on arange
  steps the emulator sits at -1 to +4 dB there; a torch whose arange has the products' floors skips that half).
* Exact properties: the zero row leaves as zeros; rate = 1 returns the input's bits; a row alone gives the bits it gives in the batch;
  rfx_phase_vocoder_frames is len(torch.arange(0, T, rate, dtype=float64)).
* The position table, per engine, through rfx_debug_vocoder_table: one primary position per bin; every position points at the
  primary of its own bin; every advance is +-frac(hop k / D) to one float32 rounding, the sign the conjugate flag's.  And the slot walk
  of the emulator on that table: the result, read back bin by bin from the primary slots, equals the bin-order result, both
  slots of a doubled bin agree, padding is zero.
* Refusals of the entries without a device; include/rfx.h as C99; the requires_grad refusal; the command line's argument checks.
* The emulator and a `main` of its own are also built as a stand-alone program with -fsanitize=address,undefined and run; nothing
  sanitized is loaded into Python.
"""
import ctypes
import math
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import vocoder_oracle as VO
from engines import ENGINES, bits as _bits
from helpers import oracle, snr_db
from vocoder_cases import (ALL_RATES, ARANGE_DIFFERS, EMU_SRC, RATES, RATES_WIDE, SEMITONE_RATES, SINE_RATES, STRUCTURED_RATES, WIDE_IDS, WIDE_SHAPES,
                           _vr, emulator, oracle_figures, oracle_pair, run_emu, sine_analysis, spectrogram, structured)

EMU_MAIN = "rfx_vocoder_emu_main.cpp"


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def emu():
    return emulator()


# ---- the steps ---------------------------------------------------------------------------------------------------------------------------

def test_oracle_steps_are_the_double_products(emu):
    """The oracle's frame pair and weight of every step are Python's own floor(i * rate) and float32(i * rate - floor) - Python floats
    are IEEE doubles - and so are the core's (voc_step through the emulator).  torch.arange(0, T, rate) has the same floors at every
    rate the suite recorded figures at before the oracle stated its steps, and other floors at the bpm ratios."""
    for rate in ALL_RATES:
        for T in (41, 512):
            n = VO.frames(T, rate)
            prod = [i * rate for i in range(n)]
            i0, a32 = VO.pairs(T, rate, torch.float32)
            a64 = VO.pairs(T, rate, torch.float64)[1]
            assert i0.dtype == torch.int64 and i0.tolist() == [math.floor(x) for x in prod], (rate, T)
            assert a64.tolist() == [x - math.floor(x) for x in prod], (rate, T)
            assert a32.numpy().tobytes() == np.array([np.float32(x - math.floor(x)) for x in prod], np.float32).tobytes(), (rate, T)
        a = ctypes.c_float(-1.0)
        for i in range(4096):
            x = i * rate
            assert emu.emu_voc_step(i, rate, ctypes.byref(a)) == math.floor(x) and np.float32(a.value) == np.float32(x - math.floor(x)), (rate, i)
    # a product past 2^31: the pair is clamped to a frame that cannot exist, before the conversion to int
    a = ctypes.c_float(-1.0)
    assert emu.emu_voc_step(1000, 1e7, ctypes.byref(a)) == 2147483646 and a.value == 0.0
    assert emu.emu_voc_step(1000, 1e7, None) == 2147483646
    assert emu.emu_voc_step(214, 1e7, None) == 2140000000 and emu.emu_voc_step(215, 1e7, None) == 2147483646

    def floors_differ(rate, T):
        ar = torch.arange(0, T, rate, dtype=torch.float64)
        return [i for i, (x, y) in enumerate(zip(ar.tolist(), [i * rate for i in range(len(ar))])) if math.floor(x) != math.floor(y)]

    for rate in RATES + SEMITONE_RATES:  # no recorded figure of the older tests moves
        for T in (41, 512):
            assert floors_differ(rate, T) == [], (rate, T)
    same = []
    for rate in ARANGE_DIFFERS:
        at = {T: floors_differ(rate, T) for T in (41, 512)}
        print(f"rate {rate}: torch.arange(0, T, rate, float64) picks another pair at steps {at[41][:4]} of T = 41, {len(at[512])} steps of T = 512")
        if not (at[41] or at[512]):
            same.append(rate)
    if same:  # this half pins torch, not the project
        pytest.skip(f"torch {torch.__version__}: torch.arange(0, T, rate, dtype=float64) has the products' floors at {same}")


# ---- parity ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [41, 2])
@pytest.mark.parametrize("name", list(ENGINES))
def test_parity_within_6_db_of_float32_torch(O, emu, name, T):
    _, op, X = spectrogram(O, name, 3, T)
    for rate in RATES:
        r64, o32 = oracle_figures(O, name, 3, T, rate)
        Y = run_emu(emu, X, op.hop_length, rate)
        e = snr_db(_vr(r64), _vr(Y))
        print(f"{name} T{T} rate {rate}: emu {e:.1f} dB, o32 {o32:.1f} dB")
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all()
        assert e >= o32 - 6.0, (name, T, rate, e, o32)
        assert not _vr(Y[-1]).any()  # the zero row leaves as zeros


def test_parity_above_float32_torch_at_512_frames(O, emu):
    _, op, X = spectrogram(O, "specialised", 1, 512)
    for rate in RATES:
        r64, o32 = oracle_figures(O, "specialised", 1, 512, rate)
        e = snr_db(_vr(r64), _vr(run_emu(emu, X, op.hop_length, rate)))
        print(f"specialised T512 rate {rate}: emu {e:.1f} dB, o32 {o32:.1f} dB")
        assert e >= o32, (rate, e, o32)


@pytest.mark.parametrize("name,T", WIDE_SHAPES, ids=WIDE_IDS)
def test_parity_at_the_wide_rates(O, emu, name, T):
    """RATES_WIDE; T_out = 1 (rate >= T: frame 0 through polar form and back) sits about 5 dB below a float32 oracle that is at
    float32's rounding floor near 144 dB - inside the rule, and printed"""
    _, op, X = spectrogram(O, name, 3, T)
    for rate in RATES_WIDE:
        r64, o32 = oracle_figures(O, name, 3, T, rate)
        Y = run_emu(emu, X, op.hop_length, rate)
        e = snr_db(_vr(r64), _vr(Y))
        print(f"{name} T{T} rate {rate:.4g}: T_out {Y.shape[-1]}, emu {e:.1f} dB, o32 {o32:.1f} dB")
        assert tuple(Y.shape) == tuple(r64.shape) == (3, X.shape[1], math.ceil(T / rate)) and torch.isfinite(_vr(Y)).all()
        assert e >= o32 - 6.0, (name, T, rate, e, o32)
        assert not _vr(Y[-1]).any()  # the zero row leaves as zeros
        for r in (0, 2):  # a row alone gives the bits it gives in the batch
            assert _bits(run_emu(emu, X[r:r + 1], op.hop_length, rate)) == _bits(Y[r:r + 1]), (rate, r)


def test_parity_on_structured_input(O, emu):
    op, X, slices = structured(O)
    for rate in STRUCTURED_RATES:
        r64, r32 = oracle_pair(X, rate, op.hop_length)
        Y = run_emu(emu, X, op.hop_length, rate)
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all() and not _vr(Y[-1]).any()
        for what, at in [("whole", (slice(None), slice(None)))] + list(slices.items()):
            e, o32 = snr_db(_vr(r64[at]), _vr(Y[at])), snr_db(_vr(r64[at]), _vr(r32[at]))
            print(f"structured rate {rate:.4g}, {what}: emu {e:.1f} dB, o32 {o32:.1f} dB")
            assert e >= o32 - 6.0, (rate, what, e, o32)
        # a step whose two frames are both zero leaves with magnitude exactly 0
        i0 = VO.pairs(41, rate)[0]
        both = (i0 >= 10) & (i0 + 1 <= 19)
        assert bool(both.any()) and not _vr(Y[0][:, both]).any(), rate
        assert bool((Y[0][:, ~both].abs() > 0).any(1).all())
        for r in (0, 1):
            assert _bits(run_emu(emu, X[r:r + 1], op.hop_length, rate)) == _bits(Y[r:r + 1]), (rate, r)


def test_parity_on_a_noise_free_analysis(O, emu):
    op, X = sine_analysis(O)
    for rate in SINE_RATES:
        r64, r32 = oracle_pair(X, rate, op.hop_length)
        Y = run_emu(emu, X, op.hop_length, rate)
        e, o32 = snr_db(_vr(r64), _vr(Y)), snr_db(_vr(r64), _vr(r32))
        print(f"440 Hz sine rate {rate:.4g}: emu {e:.1f} dB, o32 {o32:.1f} dB")
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all()
        assert e >= o32 - 6.0, (rate, e, o32)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ENGINES))
def test_copy_at_rate_one_and_a_row_alone(O, emu, name):
    _, op, X = spectrogram(O, name, 3, 41)
    assert _bits(run_emu(emu, X, op.hop_length, 1.0)) == _bits(X)
    for rate in (1.25, 0.9):
        Y = run_emu(emu, X, op.hop_length, rate)
        for r in (0, 2):
            assert _bits(run_emu(emu, X[r:r + 1], op.hop_length, rate)) == _bits(Y[r:r + 1]), (rate, r)


def test_frame_count_is_torch_aranges():
    from riffusion import _hip

    for rate in RATES + [0.5, 2.0, 3.7]:
        for T in range(1, 601):
            assert _hip.phase_vocoder_frames(T, rate) == len(torch.arange(0, T, rate, dtype=torch.float64)), (T, rate)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def _table(name):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    _, kw, plan_kw = ENGINES[name]
    p = SpectrogramParams(**kw)
    cp = _hip.RfxParams(p.sample_rate, p.n_fft, p.win_length, p.hop_length, p.num_frequencies, p.max_mel_iters)
    return p, _hip.vocoder_table(cp, **plan_kw)


@pytest.mark.parametrize("name", list(ENGINES))
def test_table_primary_positions_and_advances(name):
    p, (bins, src, adv, conj) = _table(name)
    n_stft, D = p.n_fft // 2 + 1, 2 * (p.n_fft // 2)
    S = len(bins)
    assert S >= n_stft and len(src) == len(adv) == len(conj) == S
    pad = bins < 0
    assert (src[pad] == -1).all() and not adv[pad].any() and not conj[pad].any()  # the padding marker
    held = np.flatnonzero(~pad)
    assert ((src[held] >= 0) & (src[held] < S)).all()
    primary = held[src[held] == held]
    assert sorted(bins[primary].tolist()) == list(range(n_stft))  # every bin has exactly one primary position
    assert (bins[src[held]] == bins[held]).all() and (src[src[held]] == src[held]).all()  # ... and every position points at its own bin's
    k = bins[held].astype(np.int64)
    frac = ((p.hop_length * k) % D).astype(np.float64) / D
    want = np.where(conj[held] != 0, -frac, frac).astype(np.float32)  # one float32 rounding of the exact fraction
    assert np.array_equal(adv[held], want)
    assert (np.signbit(adv[held]) == (conj[held] != 0)).all()  # the sign is the flag's, a zero advance included
    # torchaudio's linspace step for even and odd n_fft alike: pi hop / (n_stft - 1) per bin is hop / D of a turn
    lin = torch.linspace(0, math.pi * p.hop_length, n_stft, dtype=torch.float64).numpy() / (2 * math.pi)
    assert np.abs((lin[k] - frac + 0.5) % 1.0 - 0.5).max() < 1e-9
    if name == "specialised":
        assert S == 9408 and len(held) == 9261 and len(primary) == 8821  # 440 bins a second time
        assert conj[primary].any()  # a primary position can hold the conjugate itself
    else:
        assert np.array_equal(held, np.arange(n_stft)) and np.array_equal(src[held], held) and not conj.any()  # plain frames


@pytest.mark.parametrize("name", list(ENGINES))
def test_slot_walk_on_the_table_is_the_bin_walk(O, emu, name):
    _, op, X = spectrogram(O, name, 3, 41)
    _, (bins, src, adv, conj) = _table(name)
    S, T = len(bins), X.shape[-1]
    held = bins >= 0
    Xn = X.numpy()
    slots = np.full((3, T, S), 7 + 7j, np.complex64)  # what rfx_pack_complex writes, the padding left as junk: it is never read
    slots[:, :, held] = np.transpose(Xn[:, bins[held], :], (0, 2, 1))
    slots[:, :, conj != 0] = np.conj(slots[:, :, conj != 0])
    for rate in (1.25, 0.75):
        want = run_emu(emu, X, op.hop_length, rate).numpy()
        Tout = want.shape[-1]
        out = np.full((3, Tout, S), 123, np.complex64)
        assert emu.emu_vocoder_slots(S, src.ctypes.data, adv.ctypes.data, conj.ctypes.data, 3, T, rate, slots.ctypes.data, out.ctypes.data) == Tout
        assert not out[:, :, ~held].any()  # padding is written zero
        primary = np.flatnonzero(held & (src == np.arange(S)))
        got = np.transpose(out[:, :, primary], (0, 2, 1)).copy()  # rfx_unpack_complex: each bin from its primary slot
        flip = conj[primary] != 0
        got[:, flip, :] = np.conj(got[:, flip, :])
        order = np.argsort(bins[primary])
        # a conjugate trajectory is the conjugate of the plain one: equal as numbers (x - x is +0 in both, so the sign of an exact zero can differ)
        assert np.array_equal(got[:, order, :], want)
        # pack(unpack(out)) == out: every slot is its bin's value, conjugated where its own flag says so
        again = np.empty_like(out)
        again[:, :, ~held] = 0
        byslot = np.transpose(got[:, order, :][:, bins[held], :], (0, 2, 1))
        again[:, :, held] = np.where(conj[held] != 0, np.conj(byslot), byslot)
        assert again.tobytes() == out.tobytes()


# ---- the entries without a device ------------------------------------------------------------------------------------------------------------

def test_refusals_without_a_device():
    from riffusion import _hip

    lib = _hip.load_library()
    n = ctypes.c_int(-7)
    for T, rate, word in ((41, 0.0, b"rate"), (41, -1.0, b"rate"), (41, float("nan"), b"rate"), (41, float("inf"), b"rate"), (0, 1.25, b"T must"),
                          (2 ** 31 - 1, 0.5, b"2^31")):
        assert lib.rfx_phase_vocoder_frames(T, rate, ctypes.byref(n)) == -1 and n.value == -7
        assert b"rfx_phase_vocoder_frames: " in lib.rfx_last_error() and word in lib.rfx_last_error(), (T, rate)
    assert lib.rfx_phase_vocoder_frames(41, 1.25, None) == -1
    assert lib.rfx_phase_vocoder_frames(41, 1.25, ctypes.byref(n)) == 0 and n.value == 33
    # B == 0 is a no-op, B < 0 and a NULL pointer are refusals, under the entry's name
    assert lib.rfx_phase_vocoder(None, None, 0, 41, 1.25, None, None) == 0
    assert lib.rfx_phase_vocoder(None, None, 1, 41, 1.25, None, None) == -1 and b"rfx_phase_vocoder: null" in lib.rfx_last_error()
    assert lib.rfx_phase_vocoder(None, None, -1, 41, 1.25, None, None) == -1
    assert lib.rfx_time_stretch(None, None, 0, 20000, 1.25, None, None, 0, None) == 0
    assert lib.rfx_time_stretch(None, None, 1, 20000, 1.25, None, None, 0, None) == -1 and b"rfx_time_stretch: null" in lib.rfx_last_error()
    assert lib.rfx_time_stretch(None, None, -1, 20000, 1.25, None, None, 0, None) == -1
    assert lib.rfx_time_stretch_workspace_bytes(None, 1, 20000, 1.25) == 0 and lib.rfx_time_stretch_samples(None, 20000, 1.25) == 0
    for bad in (0, -1.0, float("nan"), float("inf"), "1.25", True, torch.tensor(1.25), [1.25, 0.8]):
        with pytest.raises(ValueError, match="rate"):
            _hip.check_stretch_rate(bad)
    assert _hip.check_stretch_rate(2) == 2.0


def test_header_compiles_as_c99_with_the_entries(tmp_path):
    emu_build.header_compiles_as_c99(
        tmp_path,
        '#include "rfx.h"\n'
        "size_t q(const rfx_plan* p) { return rfx_time_stretch_workspace_bytes(p, 1, 20000, 1.25) + (size_t)rfx_time_stretch_samples(p, 20000, 1.25); }\n"
        "int r(const rfx_plan* p, void* x, float* y, void* ws, int* n) {\n"
        "  return rfx_phase_vocoder_frames(41, 1.25, n) + rfx_phase_vocoder(p, x, 1, 41, 1.25, ws, 0) + rfx_time_stretch(p, y, 1, 20000, 0.8, y, ws, 0, 0); }\n"
        "int t(const rfx_params* p, int32_t* a, float* f, uint8_t* c, int32_t* n) { return rfx_debug_vocoder_table(p, 0, a, a, f, c, 0, n); }\n")


def test_an_input_that_requires_grad_is_refused_before_the_plan():
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    c = SpectrogramConverter(SpectrogramParams(), device="cpu")  # (no plan on the CPU: a call that reached for one would say so)
    w = torch.zeros(2, 20000, requires_grad=True)
    X = torch.zeros(2, 8821, 9, dtype=torch.complex64, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        c.time_stretch(w, 1.25)
    with pytest.raises(RuntimeError, match="no backward"):
        c.time_stretch_spectrogram(X, 1.25)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):  # grad mode off: the rule does not apply, the call goes on to the plan
        c.time_stretch(w, 1.25)
    for bad in (0.0, float("nan"), torch.tensor(1.25)):
        with pytest.raises(ValueError, match="rate"):
            c.time_stretch(w.detach(), bad)
    with pytest.raises(ValueError, match="linear bins"):
        c.time_stretch_spectrogram(X.detach()[:, :-1], 1.25)
    with pytest.raises(ValueError, match="complex"):
        c.time_stretch_spectrogram(X.detach().abs(), 1.25)
    with pytest.raises(ValueError, match="length"):
        c.time_stretch(w.detach(), 1.25, length=-1)


def test_command_line_argument_checks(capsys):
    from riffusion import cli

    assert cli._stretch_rate(rate=1.25, bpm_from=0.0, bpm_to=0.0) == 1.25
    assert cli._stretch_rate(rate=0.0, bpm_from=120.0, bpm_to=100.0) == 100.0 / 120.0
    for flags in ([], ["--rate", "1.25", "--bpm-from", "120", "--bpm-to", "100"], ["--bpm-from", "120"], ["--bpm-to", "100"], ["--rate", "-2"],
                  ["--rate", "nan"], ["--rate", "inf"], ["--bpm-from", "120", "--bpm-to", "-1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["time-stretch", "--audio", "missing.wav", "--output", "out.wav"] + flags)
        assert e.value.code == 2, flags
        err = capsys.readouterr().err
        assert "--rate" in err or "--bpm" in err, flags
    with pytest.raises(SystemExit):  # --audio and --output are required
        cli.main(["time-stretch", "--rate", "1.25"])


# ---- the sanitized stand-alone program ---------------------------------------------------------------------------------------------------------

def test_sanitized_stand_alone_emulator():
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program; the sanitizers'
    runtimes are linked statically, so the program carries them itself"""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-ffp-contract=off", "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr
