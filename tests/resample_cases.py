"""
What the windowed-sinc resampler's tests share (TEST INFRASTRUCTURE ONLY; tests/test_resample_cpu.py and tests/test_gpu_resample.py):
the rate pairs, lengths and filters, the seeded waves, the gates worked out from the oracle, and the host emulator
(csrc/rfx_resample_core.h compiled for the host with tests/emu/rfx_resample_emu.cpp), built once per process.
"""
import ctypes
import functools

import torch

import emu_build
import resample_oracle as RO
from helpers import snr_db

EMU_SRC = "rfx_resample_emu.cpp"
DENSE_PAIRS = [(2, 1), (1, 2), (55, 49), (160, 147), (147, 160)]
DENSE = DENSE_PAIRS + [(7787, 7350)]  # a dense kernel fits: 0.46 GB of float64 for the last
PAIRS = DENSE + [(33037, 44100)]
LENGTHS = [5, 2000, 3001]
# The wider cases, kept apart from PAIRS x LENGTHS: (orig, new, L, lowpass_filter_width, rolloff)
DEFAULT_FILTER = (6, 0.99)
WIDE_PAIRS = [(4, 1), (12, 1), (1, 4), (1, 12), (3, 2), (44099, 44100), (44100, 44099)]  # n = 1: one phase; o = 1; far more phases than outputs
WIDE_LENGTHS = [1, 2, 255, 1000]
FILTER_PAIRS = [(55, 49), (1, 2), (2, 1)]
FILTERS = [(1, 0.99), (16, 0.99), (64, 0.9475937167399596), (6, 1.0), (6, 0.5)]
SEAM_LENGTHS = {277: 255, 278: 256, 279: 257, 280: 258}  # 160/147: K on both sides of a workgroup's 256 outputs
WIDE_CASES = ([(o, n, L) + DEFAULT_FILTER for o, n in WIDE_PAIRS for L in WIDE_LENGTHS] + [(o, n, 1000) + f for o, n in FILTER_PAIRS for f in FILTERS]
              + [(160, 147, L) + DEFAULT_FILTER for L in SEAM_LENGTHS])
WIDE_IDS = [f"{o}/{n}-L{L}-lpw{lpw}-rolloff{ro:.4g}" for o, n, L, lpw, ro in WIDE_CASES]
WIDE_TABLES = sorted({(o, n, lpw, ro) for o, n, _, lpw, ro in WIDE_CASES})
_CACHE = {}


@functools.lru_cache(maxsize=1)
def emulator():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i, ll, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    lib.emu_rs_frames.argtypes, lib.emu_rs_frames.restype = [ll, i, i], ll
    lib.emu_rs_table.argtypes = [i, i, i, d, vp, vp, vp, vp]
    lib.emu_resample.argtypes, lib.emu_resample.restype = [vp, i, ll, ll, i, i, vp, vp, i, vp, ll, ll], None
    return lib


def wave(L, B=3, seed=0):
    """the input of a case (shared with tests/test_gpu_resample.py): seeded float32 noise of unit variance, the last row all zero; made
    once and left unchanged"""
    key = ("wave", L, B, seed)
    if key not in _CACHE:
        x = torch.randn(B, L, generator=torch.Generator().manual_seed(1234 + L + seed), dtype=torch.float32)
        if B > 1:
            x[-1] = 0
        _CACHE[key] = x
    return _CACHE[key]


def table64(orig, new, lpw=6, rolloff=0.99):
    key = ("table", orig, new, lpw, rolloff)
    if key not in _CACHE:
        _CACHE[key] = RO.sparse_table(orig, new, lpw, rolloff)
    return _CACHE[key]


def sparse_figures(orig, new, L, lpw=6, rolloff=0.99):
    """SNRs of the two sparse float32 forms against the float64 result"""
    key = ("sfig", orig, new, L, lpw, rolloff)
    if key not in _CACHE:
        x, tb = wave(L), table64(orig, new, lpw, rolloff)
        r64 = RO.sparse_resample(x, orig, new, lpw, rolloff, table=tb)
        _CACHE[key] = tuple(snr_db(r64[:-1], RO.sparse_resample_f32(x, orig, new, RO.sparse_weights(orig, new, dt, lpw, rolloff, table=tb), tb)[:-1])
                            for dt in (torch.float32, torch.float64))
    return _CACHE[key]


def wide_gates(orig, new, L, lpw, rolloff):
    """`gates` of a WIDE_CASES case: the float64 result and the two sparse float32 figures, as for 33037/44100 - these pairs either have
    no dense kernel of sensible size or gain nothing from one"""
    key = ("wfig", orig, new, L, lpw, rolloff)
    if key not in _CACHE:
        r64 = RO.sparse_resample(wave(L), orig, new, lpw, rolloff, table=table64(orig, new, lpw, rolloff))
        _CACHE[key] = (r64,) + sparse_figures(orig, new, L, lpw, rolloff)
    return _CACHE[key]


def gates(orig, new, L):
    """(float64 result, SNR of the all-float32 oracle: to reach outright, SNR of the float32-rounded-kernel oracle: to reach within
    6 dB) of a case, made once.  The dense transcriptions where their kernel fits, the sparse float32 forms for 33037/44100."""
    key = ("fig", orig, new, L)
    if key not in _CACHE:
        x = wave(L)
        r64 = RO.sparse_resample(x, orig, new, table=table64(orig, new))
        if (orig, new) in DENSE:
            _CACHE[key] = (r64, snr_db(r64[:-1], RO.resample_f32(x, orig, new)[:-1]), snr_db(r64[:-1], RO.resample_f32_kernel64(x, orig, new)[:-1]))
        else:
            _CACHE[key] = (r64,) + sparse_figures(orig, new, L)
    return _CACHE[key]


def run_emu(emu, x, orig, new, valid=None, lpw=6, rolloff=0.99):
    from riffusion import _hip

    if orig == new:
        return x.clone()
    first, taps = _hip.resample_sinc_table(orig, new, lpw, rolloff)
    o, n, _, _ = RO.geometry(orig, new)
    x = x.contiguous()
    B, L = x.shape
    K = RO.frames(L, orig, new)
    y = torch.full((B, K), 123.0)
    emu.emu_resample(x.data_ptr(), B, L, L if valid is None else valid, o, n, first.ctypes.data, taps.ctypes.data, taps.shape[0], y.data_ptr(), K, K)
    return y
