"""
What the time stretch's tests share (TEST INFRASTRUCTURE ONLY; tests/test_vocoder_cpu.py and tests/test_gpu_vocoder.py): the rates,
the inputs - seeded spectrograms on the engines of tests/engines.py, the structured one, a sine's analysis - each made once and left
unchanged, the oracle's figures of them, and the host emulator (csrc/rfx_vocoder_core.h compiled for the host with
tests/emu/rfx_vocoder_emu.cpp), built once per process.
"""
import ctypes
import functools
import math

import torch

import emu_build
import istft_oracle as IO
import vocoder_oracle as VO
from engines import ENGINES
from helpers import snr_db, synthetic_wave

EMU_SRC = "rfx_vocoder_emu.cpp"
RATES = [1.25, 0.75, 1.1, 0.9]
# bpm ratios (near-integer products), rates >= 2 (every step takes two new frames), <= 0.5 (a pair stays for several steps), >= T (one output frame)
RATES_WIDE = [2 / 3, 4 / 3, 0.3, 1.2, 2.0, 3.0, 2.5, 7.3, 0.5, 0.125, 40.0, 41.0, 50.0]
SEMITONE_RATES = [2.0 ** (-n / 12) for n in (2, -5, 12, -12)]  # the pitch shift's, tests/test_gpu_pitch_shift.py
# every rate of the vocoder and pitch-shift tests: the frame-count test's, the command line's 100 / 120, the pitch shift's other steps
ALL_RATES = RATES + RATES_WIDE + SEMITONE_RATES + [3.7, 100.0 / 120.0] + [2.0 ** (-n / 12) for n in (24, -24, 0.5, 1e-9, -1e-9)]
ARANGE_DIFFERS = [2 / 3, 4 / 3, 0.3, 1.2]  # where the float64 CPU arange leaves the products (on the torch build this was written with)
SPECIAL_ENGINES = ["specialised", "chirp-z-1009"]
_CASES = {}


@functools.lru_cache(maxsize=1)
def emulator():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_voc_frames.argtypes, lib.emu_voc_frames.restype = [i, d], ctypes.c_longlong
    lib.emu_voc_advance.argtypes, lib.emu_voc_advance.restype = [i, i, i], ctypes.c_float
    lib.emu_voc_step.argtypes, lib.emu_voc_step.restype = [i, d, ctypes.POINTER(ctypes.c_float)], i
    lib.emu_vocoder.argtypes = [i, i, i, i, d, vp, vp]
    lib.emu_vocoder_slots.argtypes = [i, vp, vp, vp, i, i, d, vp, vp]
    return lib


def _vr(x):
    return torch.view_as_real(x.resolve_conj())


def spectrogram(O, name, B, T):
    """the input of a case (shared with tests/test_gpu_vocoder.py): (SpectrogramParams, oracle params, X (B, n_stft, T) complex64), made
    once and left unchanged.  B > 1: the last row is all zero.  T = 1, 2, 3: the first frames of the T = 41 spectrogram."""
    from riffusion.spectrogram_params import SpectrogramParams

    key = (name, B, T)
    if key not in _CASES:
        p = SpectrogramParams(**ENGINES[name][1])
        op = O.params_from(p)
        if T <= 3:
            X = spectrogram(O, name, B, 41)[2][..., :T].clone()
        else:
            gen = torch.Generator().manual_seed(77 + T + B)
            X = IO.stft(O, synthetic_wave(B, IO.samples(op, T), seed=303), op, torch.float64)
            assert X.shape[-1] == T, (X.shape[-1], T)
            rms = float(X.abs().pow(2).mean().sqrt())
            X = X + 0.7071 * rms * torch.complex(torch.randn(X.shape, generator=gen, dtype=torch.float64), torch.randn(X.shape, generator=gen, dtype=torch.float64))
            X = X.to(torch.complex64)
            if B > 1:
                X[-1] = 0
        _CASES[key] = (p, op, X)
    return _CASES[key]


def oracle_figures(O, name, B, T, rate):
    """(float64 result, SNR of the float32 oracle against it), made once per case and rate"""
    key = (name, B, T, rate)
    if key not in _CASES:
        _, op, X = spectrogram(O, name, B, T)
        r64 = VO.phase_vocoder(X, rate, op.hop_length, torch.float64)
        _CASES[key] = (r64, snr_db(_vr(r64), _vr(VO.phase_vocoder(X, rate, op.hop_length, torch.float32))))
    return _CASES[key]


def run_emu(emu, X, hop, rate):
    B, F, T = X.shape
    X = X.contiguous()
    Y = torch.full((B, F, VO.frames(T, rate)), 123.0, dtype=torch.complex64)
    frames = emu.emu_vocoder(F, hop, B, T, rate, X.data_ptr(), Y.data_ptr())
    assert frames == Y.shape[-1], (frames, Y.shape[-1])
    return Y


STRUCTURED_RATES = [1.25, 2 / 3, 3.0]
# The float64 oracle's own rounding floor, 2^-53 relative: 319.1 dB.  A figure above it says nothing about the result - the difference
# IS the oracle's error.  On the structured input's special bins at rate 3 every phase is an exact multiple of a quarter turn; there
# sincospif answers exact zeros, the oracle's polar(mag, pi) does not (sin(pi) is 1.2e-16 in double), and the emulator, whose sine is
# double's, repeats the oracle's error and scores 464 dB where the exact answer scores 319.5.  So a figure is capped here before
# another figure is held to it.
REF_FLOOR_DB = 20 * math.log10(2.0 ** 53)
SINE_RATES = [1.25, 2 / 3]


def structured(O):
    """(op, X, the four slices that are gated on their own) of the structured input (shared with tests/test_gpu_vocoder.py): the
    specialised T = 41 case with frames 10 .. 19 of row 0 exactly zero; row 1: bin 0 real with alternating sign, the last bin real
    negative with imaginary part -0.0, bin 5 purely imaginary.  Made once and left unchanged."""
    if "structured" not in _CASES:
        _, op, X = spectrogram(O, "specialised", 3, 41)
        X = X.clone()
        X[0, :, 10:20] = 0
        sign = torch.tensor([1.0, -1.0]).repeat(21)[:41]
        X[1, 0] = torch.complex(X[1, 0].abs() * sign, torch.zeros(41))
        X[1, -1] = torch.complex(-X[1, -1].abs(), torch.full((41,), -0.0))
        X[1, 5] = torch.complex(torch.zeros(41), X[1, 5].imag)
        assert bool(torch.signbit(X[1, -1].imag).all()) and bool((X[1, -1].real < 0).all()) and not X[1, 5].real.any() and bool((X[1, 0].real[1::2] < 0).all())
        slices = {"row 0 (ten zero frames)": (0, slice(None)), "row 1 bin 0 (real, alternating)": (1, 0), "row 1 last bin (negative, -0.0 i)": (1, -1),
                  "row 1 bin 5 (imaginary)": (1, 5)}
        _CASES["structured"] = (op, X, slices)
    return _CASES["structured"]


def sine_analysis(O):
    """(op, X (1, n_stft, 41) complex64): the float64 oracle STFT of an 8000-amplitude 440 Hz sine on the specialised engine, rounded
    once - an analysis without noise, whose bins away from the line are small and smooth (shared with tests/test_gpu_vocoder.py)"""
    if "sine" not in _CASES:
        from riffusion.spectrogram_params import SpectrogramParams

        p = SpectrogramParams()
        op = O.params_from(p)
        Lw = IO.samples(op, 41)
        w = 8000 * torch.sin(2 * math.pi * 440.0 * torch.arange(Lw, dtype=torch.float64) / p.sample_rate)
        X = IO.stft(O, w.reshape(1, Lw), op, torch.float64).to(torch.complex64)
        assert X.shape[-1] == 41, X.shape[-1]
        _CASES["sine"] = (op, X)
    return _CASES["sine"]


def oracle_pair(X, rate, hop):
    """(float64 result, float32 result) of the oracle on an input that is no `spectrogram` case"""
    return VO.phase_vocoder(X, rate, hop, torch.float64), VO.phase_vocoder(X, rate, hop, torch.float32)


WIDE_SHAPES = [(name, 41) for name in ENGINES] + [(name, T) for T in (3, 1) for name in SPECIAL_ENGINES]
WIDE_IDS = [f"{name}-T{t}" for name, t in WIDE_SHAPES]
