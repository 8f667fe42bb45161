"""
ctypes binding of librfx.so (include/rfx.h) and the per-`SpectrogramParams` plan cache.

This is the only place where Python touches the native library.  Tensors are handed over as raw
device pointers (`tensor.data_ptr()`) together with torch's current HIP stream; the library never
sees a torch type.  If the shared library is missing the import of the HIP path fails loudly -
there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import dataclasses
import functools
import math
import os
import threading
import typing as T

import numpy as np
import torch

from riffusion._decode import DecodeExtras

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("RFX_LIB_PATH") or os.path.join(os.path.dirname(_PKG_DIR), "librfx.so")

_lib: T.Optional[ctypes.CDLL] = None
_lib_lock = threading.Lock()

c_void_p, c_int, c_size_t, c_float, c_uint64 = (
    ctypes.c_void_p,
    ctypes.c_int,
    ctypes.c_size_t,
    ctypes.c_float,
    ctypes.c_uint64,
)


class RfxParams(ctypes.Structure):
    """rfx_params of include/rfx.h."""

    _fields_ = [
        ("sample_rate", ctypes.c_int32),
        ("n_fft", ctypes.c_int32),
        ("win_length", ctypes.c_int32),
        ("hop_length", ctypes.c_int32),
        ("n_mels", ctypes.c_int32),
        ("max_mel_iters", ctypes.c_int32),
    ]


class RfxPlanOptions(ctypes.Structure):
    """rfx_plan_options of include/rfx.h."""

    _fields_ = [("struct_size", ctypes.c_uint32), ("gl_form", ctypes.c_int32), ("gl_frames_per_slot", ctypes.c_int32),
                ("frame_engine", ctypes.c_int32), ("plan_layout", ctypes.c_int32), ("imel_form", ctypes.c_int32)]


class RfxPlanBankReport(ctypes.Structure):
    """rfx_plan_bank_report of include/rfx.h: what plan creation decides for a parameter set and a filterbank (tests, no GPU)."""

    _fields_ = ([("struct_size", ctypes.c_uint32)]
                + [(n, ctypes.c_int32) for n in ("engine", "frame_stride", "imel_ok", "imel_kernel", "fast_ok", "unit_form", "wave_ok",
                                                 "line_from", "f_lo", "f_hi", "nnz", "fwd_ok", "fwd_product", "fwd_packed")]
                + [("fwd_kb_mask", ctypes.c_uint32)]
                + [(n, ctypes.c_int32) for n in ("fwd_prod_arr", "band_rows", "Mpad", "n_kblocks")]
                + [("line_tolerance", ctypes.c_double), ("line_deviation", ctypes.c_double), ("imel_why", ctypes.c_char * 96)]
                + [(n, ctypes.c_int32) for n in ("fft_length", "pass_length", "czt_chirp_elems", "czt_h_elems")])


class RfxCompressOptions(ctypes.Structure):
    """rfx_compress_options of include/rfx.h: rfx_pcm16_apply_filters_compressed's tables, form and flag list."""

    _fields_ = [("struct_size", ctypes.c_uint32), ("form", ctypes.c_int32), ("look_frames", ctypes.c_int32),
                ("chunk_frames", ctypes.c_int32), ("d_gain10_by_rms", ctypes.c_void_p), ("d_gain12_by_rms", ctypes.c_void_p),
                ("d_boost_by_peak", ctypes.c_void_p), ("d_above", ctypes.c_void_p), ("d_max_att", ctypes.c_void_p),
                ("d_inc", ctypes.c_void_p), ("d_dec", ctypes.c_void_p), ("margin", ctypes.c_double), ("d_flags", ctypes.c_void_p),
                ("flag_capacity", ctypes.c_int64), ("d_rounds", ctypes.c_void_p), ("n_flagged", ctypes.c_int64)]


# rfx_compress_form: the recurrence of compress_dynamic_range; chunked is the measured faster form
COMPRESS_FORMS = {"sequential": 0, "chunked": 1}
# products x2 * 10^(-att/20) closer than this to an integer are recomputed with the host's pow (include/rfx.h)
COMPRESS_MARGIN = 2.0 ** -30
COMPRESS_FLAG_BYTES = 24


class RfxCallOptions(ctypes.Structure):
    """rfx_call_options of include/rfx.h (round 6): per-call options of the inverse entry points."""

    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("row_base", ctypes.c_uint64),
                ("magnitude_hint", ctypes.c_float), ("reserved", ctypes.c_float)]


CALL_INVERSE_MEL_LSTSQ = 1  # RFX_CALL_INVERSE_MEL_LSTSQ
INVERSE_MEL_FORMS = ("sgd", "lstsq")  # the `inverse_mel` keyword of the converters


class RfxGuidedCallOptions(ctypes.Structure):
    """rfx_guided_call_options of include/rfx.h: rfx_call_options grown at its tail by the guide of a phase-guided Griffin-Lim start."""

    _fields_ = RfxCallOptions._fields_ + [("d_guide", ctypes.c_void_p), ("guide_stride", ctypes.c_int64),
                                          ("guide_samples", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


class RfxHeldCallOptions(ctypes.Structure):
    """rfx_held_call_options of include/rfx.h: rfx_guided_call_options grown at its tail by the frames a guided call holds."""

    _fields_ = RfxGuidedCallOptions._fields_ + [("d_hold_frames", ctypes.c_void_p), ("reserved3", ctypes.c_uint64)]


class RfxMaskedCallOptions(ctypes.Structure):
    """rfx_masked_call_options of include/rfx.h: rfx_held_call_options grown at its tail by the bins a guided call holds."""

    _fields_ = RfxHeldCallOptions._fields_ + [("d_hold_bins", ctypes.c_void_p), ("hold_words", ctypes.c_int32), ("reserved4", ctypes.c_int32)]


class RfxLoopCallOptions(ctypes.Structure):
    """rfx_loop_call_options of include/rfx.h: rfx_masked_call_options grown at its tail by the loop switch."""

    _fields_ = RfxMaskedCallOptions._fields_ + [("loop", ctypes.c_uint32), ("reserved5", ctypes.c_uint32)]


class RfxStartCallOptions(ctypes.Structure):
    """rfx_start_call_options of include/rfx.h: rfx_loop_call_options grown at its tail by the choice of Griffin-Lim's start."""

    _fields_ = RfxLoopCallOptions._fields_ + [("start", ctypes.c_uint32), ("reserved6", ctypes.c_uint32)]


def check_call_rules(wording: T.Mapping[str, T.Any], *only: str, loop: bool = False, peak_start: bool = False, **extras: T.Any) -> None:
    """The combination rules of a Griffin-Lim call's extras, stated once for every Python layer (the library states them for the C
    ABI: rule_refusal of csrc/rfx_api_inverse.hip).  `extras`: the caller's other starts and holds under its own argument names,
    None when not given.  `wording`: the layer's message for each rule it checks (`{given}`: the names of the extras given);
    under "roles", what the layer's names mean where they are not the library's own `angles0`, `guide`, `hold`, `hold_bins`.
    `only`: the rules to check now, for a layer that has checks of its own between them (default: all of `wording`, in its order).
    ValueError with the first broken rule's message."""
    roles = wording.get("roles", {})
    given = [name for name, value in extras.items() if value is not None]
    if not given:  # (every rule is about an extra)
        return
    has = {roles.get(name, name) for name in given}
    broken = {
        "peak_start": peak_start,                                  # the peak start is a start of its own and holds nothing
        "peak_and_guide": peak_start and "guide" in has,           # (the layers that know no other extra a peak start could meet)
        "loop_holds": loop and bool(has & {"hold", "hold_bins"}),  # a loop holds nothing
        "two_starts": {"guide", "angles0"} <= has,                 # a guide and injected angles are two starts
        "hold_needs_guide": "hold" in has and "guide" not in has,  # frames and bins are held at a guide's phase
        "bins_need_guide": "hold_bins" in has and "guide" not in has,
        "bins_and_hold": {"hold", "hold_bins"} <= has,             # a mask and held frames exclude each other
    }
    for rule in only or [rule for rule in wording if rule != "roles"]:
        if broken[rule]:
            raise ValueError(wording[rule].format(given=", ".join(given)))


_HOLD_WORDING = {"hold_needs_guide": "hold needs a guide: the frames are held at the guide's phase",
                 "bins_need_guide": "hold_bins needs a guide: the bins are held at the guide's phase",
                 "bins_and_hold": "hold_bins together with hold is not served: set the held frames' bits in the mask"}
BUILDER_WORDING = {"peak_start": "peak_start together with guide, hold or hold_bins is not served: each is a start, or needs the guide's",
                   "loop_holds": "loop together with hold or hold_bins is not served", **_HOLD_WORDING}
PLAN_WORDING = {"roles": {"angles0_slots": "angles0"}, "loop_holds": BUILDER_WORDING["loop_holds"],
                "peak_start": "peak_start does not go with {given}: the peak start needs no guide and holds nothing",
                "two_starts": "a guide and angles0_slots are two starts: give one", **_HOLD_WORDING}

_MASK_DTYPES = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)  # a bit mask's words


def call_options(*, rows: int = 0, row_base: int = 0, magnitude_hint: float = 0.0, lstsq: bool = False, guide: T.Optional[torch.Tensor] = None,
                 hold: T.Optional[torch.Tensor] = None, hold_bins: T.Optional[torch.Tensor] = None, loop: bool = False, peak_start: bool = False):
    """The options of an inverse call, as the shortest of the structs above that holds what is given (the library reads a struct by
    its size): RfxCallOptions for none of the extras, RfxGuidedCallOptions for a guide alone, and so on.
    `lstsq`: the fused inverse calls run the closed-form InverseMelScale (rfx_inverse_mel_lstsq) in place of the SGD.
    `rows`: the call's Griffin-Lim rows, which the tensors are checked against.
    `guide`: a (rows, Lg) float32 device tensor whose samples are contiguous (rows may be strided).  `hold`: a contiguous (rows, 2)
    int32 tensor of {head, tail} on the guide's device.  `hold_bins`: a contiguous (rows, T, words) int32 (or uint32) tensor on the
    guide's device, bin b of a frame held iff bit b & 31 of word b >> 5 is set.  `loop`: the row's columns are one period (a clip's
    end runs into its start).  `peak_start`: Griffin-Lim starts from phases built from the call's magnitudes.  Which of them go
    together: `check_call_rules`.  The caller keeps the tensors alive until the call is issued."""
    rules = functools.partial(check_call_rules, BUILDER_WORDING, loop=loop, peak_start=peak_start, guide=guide, hold=hold, hold_bins=hold_bins)
    rules("peak_start", "loop_holds")
    if row_base < 0:
        raise ValueError("row_base must be >= 0")
    cls: T.Any = RfxCallOptions
    fields: T.Dict[str, T.Any] = dict(flags=CALL_INVERSE_MEL_LSTSQ if lstsq else 0, row_base=int(row_base), magnitude_hint=float(magnitude_hint))
    if guide is not None:
        if guide.dtype != torch.float32 or guide.dim() != 2 or guide.shape[0] != rows or guide.shape[1] < 1:
            raise ValueError(f"guide must be a ({rows}, Lg) float32 tensor with Lg >= 1, got {tuple(guide.shape)} {guide.dtype}")
        if guide.stride(1) != 1 or (rows > 1 and guide.stride(0) < guide.shape[1]):
            raise ValueError("guide rows must be contiguous runs of samples that do not overlap")
        cls = RfxGuidedCallOptions
        fields.update(d_guide=guide.data_ptr(), guide_stride=guide.stride(0) if rows > 1 else guide.shape[1], guide_samples=guide.shape[1])
    if hold is not None:
        rules("hold_needs_guide")
        if hold.dtype != torch.int32 or tuple(hold.shape) != (rows, 2) or not hold.is_contiguous():
            raise ValueError(f"hold must be a contiguous ({rows}, 2) int32 tensor of (head, tail) frames, got {tuple(hold.shape)} {hold.dtype}")
        if hold.device != guide.device:
            raise ValueError(f"hold on {hold.device}, guide on {guide.device}")
        cls = RfxHeldCallOptions
        fields.update(d_hold_frames=hold.data_ptr())
    if hold_bins is not None:
        rules("bins_need_guide", "bins_and_hold")
        if hold_bins.dtype not in _MASK_DTYPES or hold_bins.dim() != 3 or hold_bins.shape[0] != rows or not hold_bins.is_contiguous():
            raise ValueError(f"hold_bins must be a contiguous ({rows}, T, words) int32 tensor of bit masks, got {tuple(hold_bins.shape)} {hold_bins.dtype}")
        if hold_bins.device != guide.device:
            raise ValueError(f"hold_bins on {hold_bins.device}, guide on {guide.device}")
        cls = RfxMaskedCallOptions
        fields.update(d_hold_bins=hold_bins.data_ptr(), hold_words=int(hold_bins.shape[2]))
    if loop:
        cls = RfxLoopCallOptions
        fields.update(loop=1)
    if peak_start:
        cls = RfxStartCallOptions
        fields.update(start=1)
    return cls(struct_size=ctypes.sizeof(cls), **fields)


PHASE_STARTS = ("random", "peaks")
PEAKS_WORDING = 'phase_start="peaks" does not go with {given}: the peak start needs no guide and holds nothing'


def check_phase_start(phase_start: str, **others: T.Any) -> bool:
    """True for "peaks", False for "random"; ValueError for anything else, and for "peaks" together with another start or a hold
    (`others`: the caller's angles0 / guide / hold arguments by name, None when not given)"""
    if phase_start not in PHASE_STARTS:
        raise ValueError(f'phase_start must be one of {PHASE_STARTS}, got {phase_start!r}')
    check_call_rules({"peak_start": PEAKS_WORDING}, peak_start=phase_start == "peaks", **others)
    return phase_start == "peaks"


def loop_min_frames(hop_length: int, n_fft: int) -> int:
    """the smallest T a loop call takes: hop_length * T >= n_fft, so that a frame covers the period at most once"""
    return -(-int(n_fft) // int(hop_length))


def check_loop_frames(hop_length: int, n_fft: int, Tn: int) -> None:
    """ValueError for a loop call of Tn frames below `loop_min_frames` (the library's RFX_ERR_INVALID, raised before any device work)"""
    need = loop_min_frames(hop_length, n_fft)
    if Tn < need:
        raise ValueError(f"a loop decode needs hop_length * T >= n_fft ({hop_length} * T >= {n_fft}): at least {need} frames, got {Tn}")


def check_loop_samples(hop_length: int, n_fft: int, samples: int) -> None:
    """ValueError for rows of `samples` samples a loop forward call does not take - anything but a positive multiple of hop_length that
    is at least n_fft: the library's own refusal (rfx_debug_loop_samples: RFX_ERR_INVALID with the nearest legal lengths below and
    above), raised before any device work"""
    lib = load_library()
    samples = int(samples)
    if not -2 ** 31 <= samples < 2 ** 31:
        raise ValueError(f"a loop call's rows of {samples} samples do not fit the library's int")
    cp = RfxParams(0, int(n_fft), 0, int(hop_length), 0, 0)
    if lib.rfx_debug_loop_samples(ctypes.byref(cp), samples) != 0:
        msg = lib.rfx_last_error()
        raise ValueError(msg.decode() if msg else "rfx_debug_loop_samples refused the length")


def loop_nearest_samples(hop_length: int, n_fft: int, samples: int) -> T.Tuple[int, int]:
    """(below, above): the nearest row lengths a loop forward call takes, as the library states them (rfx_debug_loop_nearest_samples) -
    the largest legal length <= samples (0: there is none) and the smallest one >= samples"""
    cp = RfxParams(0, int(n_fft), 0, int(hop_length), 0, 0)
    below, above = ctypes.c_int64(0), ctypes.c_int64(0)
    if not -2 ** 31 <= int(samples) < 2 ** 31:
        raise ValueError(f"a loop call's rows of {samples} samples do not fit the library's int")
    check(load_library().rfx_debug_loop_nearest_samples(ctypes.byref(cp), int(samples), ctypes.byref(below), ctypes.byref(above)))
    return int(below.value), int(above.value)


def spectral_loss_floor(log_floor: T.Optional[float]) -> float:
    """the log floor as the library takes it: None or 0 -> 0.0 ("no log term"), else the float32 nearest to it; ValueError for what
    the library refuses - a negative or non-finite floor, or one below 1e-18 (1 / floor^2 must fit float32 in the backward)"""
    if log_floor is None:
        return 0.0
    f = float(np.float32(log_floor))
    if f == 0.0 and float(log_floor) == 0.0:
        return 0.0
    if not (np.isfinite(f) and f >= float(np.float32(1e-18))):
        raise ValueError(f"log_floor must be None, 0 or a finite value of at least 1e-18, got {log_floor!r}")
    return f


def check_inverse_mel(inverse_mel: str) -> bool:
    """True for "lstsq", False for "sgd"; anything else raises."""
    if inverse_mel not in INVERSE_MEL_FORMS:
        raise ValueError(f"inverse_mel must be one of {list(INVERSE_MEL_FORMS)}, got {inverse_mel!r}")
    return inverse_mel == "lstsq"


class RfxLstsqBankReport(ctypes.Structure):
    """rfx_lstsq_bank_report of include/rfx.h: whether the closed-form InverseMelScale serves a filterbank, and its factor tables."""

    _fields_ = [("struct_size", ctypes.c_uint32), ("ok", ctypes.c_int32), ("min_pivot_ratio", ctypes.c_double), ("min_pivot", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("h_neg_l", ctypes.c_void_p), ("h_inv_d", ctypes.c_void_p), ("why", ctypes.c_char * 160)]


def lstsq_bank_report(cp: RfxParams, melfb: torch.Tensor, tables: bool = False):
    """rfx_debug_lstsq_bank (host only, no GPU) for the (n_stft, n_mels) float32 filterbank `melfb`: the report and, with
    `tables`, the two float32 factor tables (None when the bank is refused)."""
    melfb = melfb.to(torch.float32).contiguous()
    report = RfxLstsqBankReport(struct_size=ctypes.sizeof(RfxLstsqBankReport))
    neg_l, inv_d = np.zeros(cp.n_mels, np.float32), np.zeros(cp.n_mels, np.float32)
    if tables:
        report.h_neg_l, report.h_inv_d = neg_l.ctypes.data, inv_d.ctypes.data
    check(load_library().rfx_debug_lstsq_bank(ctypes.byref(cp), melfb.data_ptr(), ctypes.byref(report)))
    return (report, (neg_l, inv_d) if report.ok else None) if tables else report


def lstsq_collect_lists(cp: RfxParams, melfb: torch.Tensor) -> T.Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """rfx_debug_lstsq_collect (host only, no GPU) for the (n_stft, n_mels) float32 filterbank `melfb`: (ptr, bin, pos, weight), the
    per-filter lists the backward of the closed-form InverseMelScale sums - CSR over filters, entries in summation order."""
    melfb = melfb.to(torch.float32).contiguous()
    lib, n = load_library(), ctypes.c_int32(0)
    ptr = np.zeros(cp.n_mels + 1, np.int32)
    check(lib.rfx_debug_lstsq_collect(ctypes.byref(cp), melfb.data_ptr(), ptr.ctypes.data, None, None, None, 0, ctypes.byref(n)))
    bins, pos, w = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.float32)
    check(lib.rfx_debug_lstsq_collect(ctypes.byref(cp), melfb.data_ptr(), None, bins.ctypes.data, pos.ctypes.data, w.ctypes.data, n.value,
                                      ctypes.byref(n)))
    return ptr, bins, pos, w


def bin_bands(cp: RfxParams, melfb: torch.Tensor) -> T.Tuple[np.ndarray, np.ndarray]:
    """rfx_debug_bin_bands (host only, no GPU) for the (n_stft, n_mels) float32 filterbank `melfb`: per linear bin the first and the
    last mel band with a nonzero weight, (n_stft,) int16 each, -1 / -1 for a bin no filter reaches - what `Plan.hold_bins_from_bands`
    expands a band mask by."""
    melfb = melfb.to(torch.float32).contiguous()
    lo, hi = np.zeros(melfb.shape[0], np.int16), np.zeros(melfb.shape[0], np.int16)
    check(load_library().rfx_debug_bin_bands(ctypes.byref(cp), melfb.data_ptr(), lo.ctypes.data, hi.ctypes.data))
    return lo, hi


GL_FORMS = {"auto": 0, "runs": 1, "frames": 2}  # rfx_gl_form
FRAME_ENGINES = {"auto": 0, "generic": 1}       # rfx_frame_engine
PLAN_LAYOUTS = {"auto": 0, "generic": 1}        # rfx_plan_layout
IMEL_FORMS = {"auto": 0, "groups": 1}           # rfx_imel_form
# opt-in engines beside them (rfx_frame_engine): "chirp-z" runs FFT lengths with a prime factor above 13, which "auto" refuses
OPT_IN_FRAME_ENGINES = {"chirp-z": 2}
GL_ENGINE_NAMES = {0: "specialised", 1: "generic", 2: "row-family", 3: "chirp-z"}  # rfx_plan_griffinlim_engine


def check_stretch_rate(rate: T.Any) -> float:
    """the rate of a time stretch as the library takes it: a finite positive number (one rate per call)"""
    import numbers

    if isinstance(rate, bool) or not isinstance(rate, numbers.Real):
        raise ValueError(f"rate must be one real number (one rate per call), got {type(rate).__name__}")
    rate = float(rate)
    if not (rate > 0.0) or rate == float("inf"):
        raise ValueError(f"rate must be finite and positive, got {rate}")
    return rate


def check_pitch_steps(n_steps: T.Any, bins_per_octave: T.Any = 12) -> T.Tuple[float, int]:
    """the shift of a pitch shift as the library takes it: one finite number of steps (one shift per call) of 1 / bins_per_octave
    octave, bins_per_octave a positive integer"""
    import numbers

    if isinstance(n_steps, bool) or not isinstance(n_steps, numbers.Real):
        raise ValueError(f"n_steps must be one real number (one shift per call), got {type(n_steps).__name__}")
    n_steps = float(n_steps)
    if n_steps != n_steps or n_steps in (float("inf"), float("-inf")):
        raise ValueError(f"n_steps must be finite, got {n_steps}")
    if isinstance(bins_per_octave, bool) or not isinstance(bins_per_octave, numbers.Integral) or int(bins_per_octave) < 1:
        raise ValueError(f"bins_per_octave must be a positive integer, got {bins_per_octave!r}")
    return n_steps, int(bins_per_octave)


def phase_vocoder_frames(Tn: int, rate: float) -> int:
    """rfx_phase_vocoder_frames (host only, no GPU): ceil(Tn / rate) in double, the length of torch.arange(0, Tn, rate)"""
    n = c_int(0)
    check(load_library().rfx_phase_vocoder_frames(int(Tn), float(rate), ctypes.byref(n)))
    return n.value


def vocoder_table(cp: RfxParams, frame_engine: str = "auto") -> T.Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """rfx_debug_vocoder_table (host only, no GPU): (bin, src, advance, conj) per position of a frame of complex slots - the bin it
    holds (-1: padding), the primary position of that bin (-1: padding), the bin's signed advance in turns, and whether the position
    holds the conjugate."""
    lib, n = load_library(), ctypes.c_int32(0)
    opt = RfxPlanOptions(ctypes.sizeof(RfxPlanOptions), 0, 0, {**FRAME_ENGINES, **OPT_IN_FRAME_ENGINES}[frame_engine], 0, 0)
    check(lib.rfx_debug_vocoder_table(ctypes.byref(cp), ctypes.byref(opt), None, None, None, None, 0, ctypes.byref(n)))
    bins, src = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    adv, conj = np.zeros(n.value, np.float32), np.zeros(n.value, np.uint8)
    check(lib.rfx_debug_vocoder_table(ctypes.byref(cp), ctypes.byref(opt), bins.ctypes.data, src.ctypes.data, adv.ctypes.data, conj.ctypes.data,
                                      n.value, ctypes.byref(n)))
    return bins, src, adv, conj


class RfxError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol declared in include/rfx.h
SIGNATURES: T.Dict[str, T.Tuple[T.Any, T.List[T.Any]]] = {
    "rfx_last_error": (ctypes.c_char_p, []),
    "rfx_version": (c_int, []),
    "rfx_frame_stride": (c_int, []),
    "rfx_num_bins": (c_int, []),
    "rfx_plan_frame_stride": (c_int, [c_void_p]),
    "rfx_plan_is_generic": (c_int, [c_void_p]),
    "rfx_plan_griffinlim_engine": (c_int, [c_void_p]),
    "rfx_mel_scale_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_plan_create": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_int, ctypes.POINTER(c_void_p)]),
    "rfx_plan_create_ex": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_int, c_void_p, ctypes.POINTER(c_void_p)]),
    "rfx_griffinlim_form": (c_int, [c_void_p, c_int, c_int]),
    "rfx_griffinlim_runs": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int]),
    "rfx_debug_run_start": (ctypes.c_int64, [ctypes.c_int64] * 6),
    "rfx_debug_gl_partition": (c_int, [c_int, c_int, c_int, c_void_p, c_int]),
    "rfx_debug_range_exponents": (c_int, [c_float, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "rfx_debug_plan_bank": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, ctypes.POINTER(RfxPlanBankReport)]),
    "rfx_debug_lstsq_bank": (c_int, [ctypes.POINTER(RfxParams), c_void_p, ctypes.POINTER(RfxLstsqBankReport)]),
    "rfx_plan_lstsq_ok": (c_int, [c_void_p]),
    "rfx_inverse_mel_lstsq_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_inverse_mel_lstsq": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_debug_lstsq_collect": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(ctypes.c_int32)]),
    "rfx_inverse_mel_lstsq_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_inverse_mel_lstsq_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # (plan, [mel,] guide, guide_samples, grad_wave, B, T, out, workspace, workspace_bytes, stream)
    "rfx_griffinlim_guided_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_griffinlim_guided_backward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_griffinlim_guided_backward_loop_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_griffinlim_guided_backward_loop": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_waveform_from_mel_guided_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_waveform_from_mel_guided_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_waveform_from_mel_guided_backward_loop_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_waveform_from_mel_guided_backward_loop": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_debug_guide_project_tables": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_int, ctypes.POINTER(ctypes.c_int32)]),
    "rfx_stft_frames": (c_int, [c_void_p, c_int]),
    "rfx_plan_imel_kernel": (c_int, [c_void_p]),
    "rfx_plan_imel_unit_form": (c_int, [c_void_p]),
    "rfx_plan_destroy": (c_int, [c_void_p]),
    "rfx_pack_magnitudes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rfx_pack_complex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rfx_unpack_complex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rfx_stft": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rfx_spectral_error_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_spectral_error": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # loop encode: the forward entries on the circular STFT (the loop twins of equal signature: LOOP_TWINS below)
    "rfx_stft_loop_frames": (c_int, [c_void_p, c_int]),
    "rfx_debug_loop_samples": (c_int, [c_void_p, c_int]),
    "rfx_debug_loop_nearest_samples": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "rfx_mel_loop_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_griffinlim_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_griffinlim_workspace_bytes_ex": (c_size_t, [c_void_p, c_int, c_int, c_void_p]),
    "rfx_peak_start_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_peak_start": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_griffinlim_loop_output_samples": (c_int, [c_void_p, c_int]),
    "rfx_debug_loop_frames": (c_int, [c_void_p, c_int]),
    "rfx_hold_mask_words": (c_int, [c_void_p]),
    "rfx_hold_bins_from_bands": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rfx_debug_bin_bands": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_void_p]),
    "rfx_griffinlim_output_samples": (c_int, [c_void_p, c_int]),
    "rfx_griffinlim": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "rfx_griffinlim_timed": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p],
    ),
    "rfx_griffinlim_ex": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p],
    ),
    "rfx_unpack_magnitudes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "rfx_mel_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_mel_from_waveform": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_mel_scale": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # backward of the forward path (riffusion/_autograd.py)
    "rfx_stft_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_stft_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_mel_scale_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_mel_scale_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_mel_from_waveform_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_mel_from_waveform_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_debug_mel_adjoint": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(ctypes.c_int32)]),
    # inverse spectrogram (riffusion/_autograd.py: IstftFunction)
    "rfx_istft_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_istft": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_istft_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_istft_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_debug_istft_backward_padded_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_debug_istft_backward_padded": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # time stretch: the phase vocoder between rfx_stft and rfx_istft
    "rfx_phase_vocoder_frames": (c_int, [c_int, ctypes.c_double, ctypes.POINTER(c_int)]),
    "rfx_phase_vocoder": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_void_p, c_void_p]),
    "rfx_time_stretch_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, ctypes.c_double]),
    "rfx_time_stretch_samples": (c_int, [c_void_p, c_int, ctypes.c_double]),
    "rfx_time_stretch": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_debug_vocoder_table": (c_int, [ctypes.POINTER(RfxParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                        ctypes.POINTER(ctypes.c_int32)]),
    # sinc resample and pitch shift: the time stretch, then the resampler back to the duration
    "rfx_resample_sinc_frames": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "rfx_resample_sinc_table": (c_int, [c_int, c_int, c_int, ctypes.c_double, c_void_p, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32)]),
    "rfx_resample_sinc": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "rfx_pitch_shift_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, ctypes.c_double, c_int]),
    "rfx_pitch_shift_resample_freq": (c_int, [c_void_p, c_int, ctypes.c_double, c_int]),
    "rfx_pitch_shift": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    # fused spectral losses (riffusion/_autograd.py: SpectralLossFunction)
    "rfx_spectral_loss_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_spectral_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_spectral_loss_backward_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_spectral_loss_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_void_p, c_void_p, c_size_t,
                                           c_void_p]),
    "rfx_inverse_mel_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_inverse_mel": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_uint64, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    "rfx_inverse_mel_ex": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_uint64, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p],
    ),
    "rfx_image_decode_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rfx_image_encode_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rfx_audio_from_image_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "rfx_audio_from_image_workspace_bytes_ex": (c_size_t, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "rfx_audio_from_image_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_uint64, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_audio_from_image_u8_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_uint64, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "rfx_waveform_from_mel_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "rfx_waveform_from_mel_workspace_bytes_ex": (c_size_t, [c_void_p, c_int, c_int, c_void_p]),
    "rfx_waveform_from_mel_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_uint64, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "rfx_waveform_from_mel": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_uint64, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_image_from_waveform_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "rfx_image_from_waveform": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_pcm16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rfx_pcm16_filters_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rfx_pcm16_apply_filters": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_pcm16_stitch": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, ctypes.c_int64, c_void_p, c_void_p]),
    "rfx_pcm16_compress_filters_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rfx_pcm16_apply_filters_compressed": (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(RfxCompressOptions), c_void_p, c_void_p,
                                                   c_size_t, c_void_p]),
    "rfx_image_resize_coefficients": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "rfx_image_resize_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "rfx_image_resize_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_pcm16_resample_frames": (c_int, [ctypes.c_int64, c_int, c_int, ctypes.POINTER(ctypes.c_int64)]),
    "rfx_pcm16_resample": (c_int, [c_void_p, ctypes.c_int64, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p]),
    "rfx_pcm16_clips_to_waveform": (c_int, [c_void_p, ctypes.c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rfx_image_from_pcm16_clips_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "rfx_image_from_pcm16_clips": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rfx_jpeg_quant_tables": (c_int, [c_int, c_void_p, c_void_p]),
    "rfx_jpeg_scan_capacity": (c_size_t, [c_int, c_int]),
    "rfx_jpeg_encode_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rfx_jpeg_encode_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rfx_jpeg_decode_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_size_t]),
    "rfx_jpeg_decode_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "rfx_png_decode_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_size_t]),
    "rfx_png_decode_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "rfx_png_stream_capacity": (c_size_t, [c_int, c_int, c_int]),
    "rfx_png_encode_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "rfx_png_encode_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}
# A loop twin takes what its plain form takes: rfx_<name>_loop, and rfx_<name>_loop_workspace_bytes where the plain form has a query
for _name in ("stft", "mel_from_waveform", "image_from_waveform", "image_from_pcm16_clips", "spectral_error", "istft", "istft_backward", "spectral_loss", "spectral_loss_backward"):
    SIGNATURES[f"rfx_{_name}_loop"] = SIGNATURES[f"rfx_{_name}"]
    if f"rfx_{_name}_workspace_bytes" in SIGNATURES:
        SIGNATURES[f"rfx_{_name}_loop_workspace_bytes"] = SIGNATURES[f"rfx_{_name}_workspace_bytes"]

# rfx_png_encode_u8's modes (RFX_PNG_RGB, RFX_PNG_GRAY, RFX_PNG_AUTO)
PNG_MODES = {"rgb": 0, "gray": 1, "auto": 2}

# PIL.Image.Resampling values of the filters rfx_image_resize_u8 implements (rfx_resize_filter)
RESIZE_FILTERS = {1: "LANCZOS", 2: "BILINEAR", 3: "BICUBIC"}


def resize_coefficients(in_size: int, out_size: int, resample: int) -> np.ndarray:
    """rfx_image_resize_coefficients (host only, no GPU): one axis's table as int32 [2 * out_size bounds | out_size * ksize
    fixed-point weights] - Pillow's Resample.c coefficients, bit for bit."""
    lib = load_library()
    ksize = lib.rfx_image_resize_coefficients(int(in_size), int(out_size), int(resample), None, None, 0)
    if ksize < 0:
        check(ksize)
    table = np.zeros(2 * out_size + out_size * ksize, dtype=np.int32)
    rc = lib.rfx_image_resize_coefficients(int(in_size), int(out_size), int(resample), table.ctypes.data,
                                           table.ctypes.data + 8 * out_size, out_size * ksize)
    if rc < 0:
        check(rc)
    return table


def jpeg_quant_tables(quality: int) -> np.ndarray:
    """rfx_jpeg_quant_tables (host only, no GPU): libjpeg's two quantisation tables of `quality` (1 .. 100, else RfxError) as
    (2, 64) uint16 in natural order, luma first - what Pillow's `Image.save(f, "JPEG", quality=quality)` uses."""
    tables = np.zeros((2, 64), dtype=np.uint16)
    check(load_library().rfx_jpeg_quant_tables(int(quality), tables.ctypes.data, tables.ctypes.data + 128))
    return tables


def check_tiles(img: torch.Tensor) -> torch.Tensor:
    """`img` if it is an (N, H, W, 3) uint8 batch, on any device; ValueError otherwise."""
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError("expected (N, H, W, 3) uint8 images")
    return img


def pack_streams(streams: T.Sequence[bytes], tables: T.Sequence[np.ndarray]) -> T.Tuple[np.ndarray, np.ndarray, T.List[int]]:
    """What a file decode uploads in one copy: [offsets | tables | pad | streams] as one uint8 array - the N + 1 cumulative int64
    offsets of the byte strings, each per-image table, the joined strings on a 16-byte boundary -> (array, offsets, every part's position)."""
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    parts = [offsets.view(np.uint8)] + [np.ascontiguousarray(t).reshape(-1).view(np.uint8) for t in tables]
    at = [0] + [int(v) for v in np.cumsum([p.size for p in parts])]
    pad = -at[-1] % 16
    at[-1] += pad
    return np.concatenate(parts + [np.zeros(pad, np.uint8), np.frombuffer(b"".join(streams), np.uint8)]), offsets, at


def split_packed(packed: bytes, sizes: T.Sequence[int]) -> T.List[bytes]:
    """N byte strings of `sizes` bytes from their concatenation."""
    ends = np.cumsum(sizes)
    return [packed[int(e) - size:int(e)] for e, size in zip(ends, sizes)]


CLIP_FRAMES_MAX = (1 << 31) - 1  # Lw of the clip entries is a C int


def resample_frames(in_frames: int, in_rate: int, out_rate: int) -> int:
    """rfx_pcm16_resample_frames (host only, no GPU): frames audioop.ratecv makes of `in_frames` frames; refuses rate pairs
    whose reduced rates reach 2^20."""
    out = ctypes.c_int64(0)
    check(load_library().rfx_pcm16_resample_frames(int(in_frames), int(in_rate), int(out_rate), ctypes.byref(out)))
    return int(out.value)


def library_path() -> str:
    return _LIB_PATH


def load_library() -> ctypes.CDLL:
    """Load librfx.so (built by `__graft_entry__.build()` / csrc/build.sh).  Raises if absent."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(_LIB_PATH):
                raise RfxError(
                    f"{_LIB_PATH} not found: build the HIP library first "
                    "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback"
                )
            lib = ctypes.CDLL(_LIB_PATH)
            for name, (restype, argtypes) in SIGNATURES.items():
                fn = getattr(lib, name)  # AttributeError if the .so does not export it
                fn.restype = restype
                fn.argtypes = argtypes
            _lib = lib
    return _lib


def check(status: int) -> None:
    if status != 0:
        msg = load_library().rfx_last_error()
        raise RfxError(f"librfx error {status}: {msg.decode() if msg else '?'}")


def current_stream(device: T.Optional[torch.device] = None) -> int:
    """torch's current stream ON `device` (not on the calling thread's current device)."""
    return torch.cuda.current_stream(device).cuda_stream


def resolve_device(device: T.Union[str, torch.device]) -> torch.device:
    """'cuda' -> the indexed device it means for the calling thread right now."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RfxError("the HIP path runs on the GPU only (device 'cuda'); there is no CPU implementation")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


# ---- sinc resample (include/rfx.h "SINC RESAMPLE"): torchaudio.functional.resample with the Hann window -------------------------------
RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF = 6, 0.99  # torchaudio's defaults
_resample_tables: "collections.OrderedDict[T.Any, T.Any]" = collections.OrderedDict()
_resample_lock = threading.Lock()


def check_resample_method(resampling_method: str) -> None:
    """only torchaudio's default window is stated"""
    if resampling_method != "sinc_interp_hann":
        raise ValueError(f"resampling_method {resampling_method!r} is not served: only 'sinc_interp_hann' (torchaudio's default) is; "
                         "there is no kaiser window on the device")


def resample_sinc_frames(L: int, orig_freq: int, new_freq: int) -> int:
    """rfx_resample_sinc_frames (host only, no GPU): ceil(new L / orig) on the reduced pair, the samples L samples give"""
    k = c_int(0)
    check(load_library().rfx_resample_sinc_frames(int(L), int(orig_freq), int(new_freq), ctypes.byref(k)))
    return k.value


def resample_sinc_table(orig_freq: int, new_freq: int, lowpass_filter_width: int = RESAMPLE_LOWPASS_FILTER_WIDTH,
                        rolloff: float = RESAMPLE_ROLLOFF, device: T.Optional[T.Union[str, torch.device]] = None) -> T.Tuple[T.Any, T.Any]:
    """rfx_resample_sinc_table: (first (n,) int32, taps (ntaps, n) float32 - tap-major) of the reduced pair.  Without `device` the
    host table as numpy arrays (no GPU); with one, the uploaded tensors, kept per (orig, new, lowpass_filter_width, rolloff, device)
    - the 32 most recently used pairs."""
    key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), None if device is None else resolve_device(device))
    with _resample_lock:
        hit = _resample_tables.get(key)
        if hit is not None:
            _resample_tables.move_to_end(key)
            return hit
    lib, n, ntaps = load_library(), ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib.rfx_resample_sinc_table(key[0], key[1], key[2], key[3], None, None, 0, ctypes.byref(n), ctypes.byref(ntaps)))
    first, taps = np.zeros(n.value, np.int32), np.zeros((ntaps.value, n.value), np.float32)
    check(lib.rfx_resample_sinc_table(key[0], key[1], key[2], key[3], first.ctypes.data, taps.ctypes.data, taps.size, ctypes.byref(n), ctypes.byref(ntaps)))
    if device is None:
        return first, taps
    table = (torch.from_numpy(first).to(key[4]), torch.from_numpy(taps).to(key[4]))
    with _resample_lock:
        _resample_tables[key] = table
        while len(_resample_tables) > 32:
            _resample_tables.popitem(last=False)
    return table


def resample_sinc(wave: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = RESAMPLE_LOWPASS_FILTER_WIDTH,
                  rolloff: float = RESAMPLE_ROLLOFF) -> torch.Tensor:
    """rfx_resample_sinc: (B, L) float32 on a GPU -> (B, ceil(new L / orig)) float32 there: torchaudio.functional.resample with the
    Hann window.  orig == new gives a copy."""
    if wave.device.type != "cuda" or wave.dtype != torch.float32 or wave.dim() != 2:
        raise ValueError(f"expected a (B, L) float32 waveform on the GPU, got {tuple(wave.shape)} {wave.dtype} on {wave.device}")
    wave = wave.contiguous()
    B, L = wave.shape
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    K = resample_sinc_frames(L, orig_freq, new_freq)
    first, taps = (None, None) if orig_freq == new_freq else resample_sinc_table(orig_freq, new_freq, lowpass_filter_width, rolloff, wave.device)
    out = torch.empty((B, K), dtype=torch.float32, device=wave.device)
    if B:
        check(load_library().rfx_resample_sinc(wave.data_ptr(), B, L, orig_freq, new_freq, None if first is None else first.data_ptr(),
                                               None if taps is None else taps.data_ptr(), 0 if taps is None else int(taps.shape[0]),
                                               out.data_ptr(), current_stream(wave.device)))
    return out


# ------------------------------------------------------------------------------------------------
# Host-side constants, built with the same torch ops torchaudio uses so that they are bit-identical
# to the buffers of the reference's modules (spectrogram_converter.py:47-99)
# ------------------------------------------------------------------------------------------------


def hann_window(win_length: int) -> torch.Tensor:
    return torch.hann_window(win_length, periodic=True, dtype=torch.float32)


def _hz_to_mel(freq: float, mel_scale: str) -> float:
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + freq / 700.0)
    # slaney
    f_sp = 200.0 / 3
    if freq >= 1000.0:
        return 1000.0 / f_sp + math.log(freq / 1000.0) / (math.log(6.4) / 27.0)
    return freq / f_sp


def _mel_to_hz(mels: torch.Tensor, mel_scale: str) -> torch.Tensor:
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    f_sp = 200.0 / 3
    freqs = f_sp * mels
    min_log_mel = 1000.0 / f_sp
    logstep = math.log(6.4) / 27.0
    is_log = mels >= min_log_mel
    freqs[is_log] = 1000.0 * torch.exp(logstep * (mels[is_log] - min_log_mel))
    return freqs


def mel_filterbank(
    n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int, norm: T.Optional[str], mel_scale: str
) -> torch.Tensor:
    """Triangular mel filterbank (n_freqs, n_mels), the buffer of torchaudio's MelScale/InverseMelScale."""
    if norm is not None and norm != "slaney":
        raise ValueError('norm must be one of None or "slaney"')
    if mel_scale not in ("htk", "slaney"):
        raise ValueError('mel_scale should be one of "htk" or "slaney".')
    grid = torch.linspace(0, sample_rate // 2, n_freqs)
    mel_pts = torch.linspace(_hz_to_mel(f_min, mel_scale), _hz_to_mel(f_max, mel_scale), n_mels + 2)
    hz_pts = _mel_to_hz(mel_pts, mel_scale)
    widths = hz_pts[1:] - hz_pts[:-1]
    dist = hz_pts.unsqueeze(0) - grid.unsqueeze(1)
    falling = (-1.0 * dist[:, :-2]) / widths[:-1]
    rising = dist[:, 2:] / widths[1:]
    fb = torch.max(torch.zeros(1), torch.min(falling, rising))
    if norm == "slaney":
        fb = fb * (2.0 / (hz_pts[2 : n_mels + 2] - hz_pts[:n_mels])).unsqueeze(0)
    return fb.to(torch.float32).contiguous()


class WorkspaceArena:
    """
    Reusable device workspaces of ONE plan (round 6).  Every C entry point takes a caller-provided scratch buffer (1.7 GB for
    64 mono tiles); until round 5 each Python call asked torch's caching allocator for a fresh one, and the allocator - which
    splits a freed 1.7 GB block as soon as a smaller request comes by - answered one call in twenty with a 20 ms hipMalloc.
    The arena keeps the buffers instead:

    * `take(nbytes, stream)` CHECKS OUT an idle buffer of at least `nbytes` that was last used on the same HIP stream (kernels
      of consecutive calls on one stream are ordered, so the hand-over needs no event), or allocates one - grow-only: a buffer
      that is too small is dropped in favour of the bigger one, sizes are rounded up to 32 MiB;
    * `give(buf, stream)` returns it when the call has QUEUED its kernels.
    A buffer that is checked out belongs to one host call: two threads of a pool that share a converter - and torch's default
    stream - (reference cli.py:172-204) get two buffers.  The lock guards the free lists only (microseconds); allocation happens
    outside it.  At most `max_idle` idle buffers are kept per plan (least recently used dropped first); `clear()` / the plan's
    `close()` release them.  The buffers are torch tensors, so `torch.cuda.memory_stats()` sees them.
    """

    GRANULE = 32 << 20

    def __init__(self, device: torch.device, max_idle: int = 4):
        self.device, self.max_idle = device, max_idle
        self._lock = threading.Lock()
        self._idle: "collections.OrderedDict[int, T.Tuple[int, torch.Tensor]]" = collections.OrderedDict()  # id -> (stream, buffer), LRU first
        self.allocations = 0  # buffers ever allocated (tests: steady state allocates nothing)

    def take(self, nbytes: int, stream: int) -> torch.Tensor:
        dropped = None
        with self._lock:
            best = None
            for key, (st, buf) in self._idle.items():
                if st == stream and buf.numel() >= nbytes and (best is None or buf.numel() < self._idle[best][1].numel()):
                    best = key
            if best is not None:
                return self._idle.pop(best)[1]
            for key, (st, buf) in self._idle.items():  # grow: the too-small buffer of this stream makes room for its successor
                if st == stream:
                    dropped = self._idle.pop(key)[1]
                    break
            self.allocations += 1
        del dropped  # back to torch's allocator (it was allocated and used on `stream` only: stream-ordered reuse is safe)
        size = max(self.GRANULE, -(-int(nbytes) // self.GRANULE) * self.GRANULE)
        return torch.empty(size, dtype=torch.uint8, device=self.device)

    def give(self, buf: torch.Tensor, stream: int) -> None:
        with self._lock:
            self._idle[id(buf)] = (stream, buf)
            while len(self._idle) > self.max_idle:
                self._idle.popitem(last=False)

    def clear(self) -> None:
        with self._lock:
            self._idle.clear()

    def idle_bytes(self) -> int:
        with self._lock:
            return sum(buf.numel() for _, buf in self._idle.values())


class _Borrowed:
    """`with plan._workspace(n) as ws:` - a checked-out arena buffer, returned when the call's kernels have been queued."""

    __slots__ = ("arena", "stream", "buf")

    def __init__(self, arena: WorkspaceArena, nbytes: int, stream: int):
        self.arena, self.stream = arena, stream
        self.buf = arena.take(nbytes, stream)

    def __enter__(self) -> torch.Tensor:
        return self.buf

    def __exit__(self, *exc: T.Any) -> bool:
        self.arena.give(self.buf, self.stream)
        return False


class Plan:
    """Owns one rfx_plan (device constants for one parameter set on one device)."""

    def __init__(self, params: T.Any, device: torch.device, gl_form: str = "auto", frame_engine: str = "auto",
                 plan_layout: str = "auto", imel_form: str = "auto"):
        self.lib = load_library()
        if gl_form not in GL_FORMS:
            raise ValueError(f"gl_form must be one of {sorted(GL_FORMS)}, got {gl_form!r}")
        engines = {**FRAME_ENGINES, **OPT_IN_FRAME_ENGINES}
        if frame_engine not in engines:
            raise ValueError(f"frame_engine must be one of {sorted(engines)}, got {frame_engine!r}")
        if plan_layout not in PLAN_LAYOUTS:
            raise ValueError(f"plan_layout must be one of {sorted(PLAN_LAYOUTS)}, got {plan_layout!r}")
        if imel_form not in IMEL_FORMS:
            raise ValueError(f"imel_form must be one of {sorted(IMEL_FORMS)}, got {imel_form!r}")
        self.gl_form = gl_form
        self.device = device
        self.sample_rate = int(params.sample_rate)
        self.n_fft, self.win_length, self.hop_length = params.n_fft, params.win_length, params.hop_length
        self.n_stft = self.n_fft // 2 + 1
        self.n_mels = params.num_frequencies
        self.window = hann_window(self.win_length)
        self.melfb = mel_filterbank(
            self.n_stft,
            float(params.min_frequency),
            float(params.max_frequency),
            self.n_mels,
            params.sample_rate,
            params.mel_scale_norm,
            params.mel_scale_type,
        )
        cp = RfxParams(params.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels, params.max_mel_iters)
        handle = c_void_p()
        self.device = device = resolve_device(device)
        opt = RfxPlanOptions(ctypes.sizeof(RfxPlanOptions), GL_FORMS[gl_form], 0, engines[frame_engine], PLAN_LAYOUTS[plan_layout],
                             IMEL_FORMS[imel_form])
        check(
            self.lib.rfx_plan_create_ex(
                ctypes.byref(cp), self.window.data_ptr(), self.melfb.data_ptr(), device.index, ctypes.byref(opt), ctypes.byref(handle)
            )
        )
        self.handle = handle
        self.frame_stride = self.lib.rfx_plan_frame_stride(self.handle)
        self.generic = bool(self.lib.rfx_plan_is_generic(self.handle))
        self.griffinlim_engine = GL_ENGINE_NAMES[self.lib.rfx_plan_griffinlim_engine(self.handle)]
        self._cparams = cp
        self.lstsq_ok = bool(self.lib.rfx_plan_lstsq_ok(self.handle))
        self.arena = WorkspaceArena(device, max_idle=max(1, int(os.environ.get("RFX_ARENA_IDLE", "4"))))
        self._consts: "collections.OrderedDict[T.Any, torch.Tensor]" = collections.OrderedDict()
        self._consts_lock = threading.Lock()

    def _workspace(self, nbytes: int) -> _Borrowed:
        """A scratch buffer of at least `nbytes` from the plan's arena for the duration of one call on the current stream."""
        return _Borrowed(self.arena, nbytes, self._stream())

    def release_workspaces(self) -> None:
        """Hands the idle scratch buffers back to torch's allocator (they are re-made on demand)."""
        self.arena.clear()

    def device_constant(self, key: T.Any, build: T.Callable[[], T.Any]) -> torch.Tensor:
        """Small host-built tables (decode LUT, encoder thresholds) uploaded ONCE per plan and key: an upload from pageable
        memory per call is a synchronous copy - the host would wait for the kernels queued before it, call after call."""
        with self._consts_lock:
            t = self._consts.get(key)
            if t is not None:
                self._consts.move_to_end(key)
                return t
        t = torch.as_tensor(build()).to(self.device)
        with self._consts_lock:
            self._consts[key] = t
            while len(self._consts) > 64:
                self._consts.popitem(last=False)
        return t

    def close(self) -> None:
        """Releases the plan's device memory now (it is released anyway when the last reference goes)."""
        arena = getattr(self, "arena", None)
        if arena is not None:
            arena.clear()
        handle, self.handle = getattr(self, "handle", None), None
        if handle:
            self.lib.rfx_plan_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- thin typed wrappers -----------------------------------------------------------------
    def _chk(self, t: torch.Tensor, dtype: T.Optional[torch.dtype] = None) -> torch.Tensor:
        """Tensors must live on THIS plan's GPU: its constant tables do, and kernels are queued on that device's stream."""
        if t.device != self.device:
            raise RfxError(f"tensor on {t.device} handed to a plan that lives on {self.device}")
        return (t if dtype is None else t.to(dtype)).contiguous()

    def _chk_slots(self, t: torch.Tensor, B: int, Tn: int, exact: bool = False) -> None:
        """magnitudes in slot layout hold the B * Tn frames of a call (`exact`: and nothing more)"""
        need = B * Tn * self.frame_stride
        if (t.numel() != need) if exact else (t.numel() < need):
            raise ValueError(f"magnitude slots hold {t.numel()} values, {B} x {Tn} frames {'are' if exact else 'need'} {need}")

    def _pair(self, name: str, loop: bool = False) -> T.Tuple[T.Any, T.Any]:
        """(workspace query, entry) of rfx_<name>, or with `loop` of its loop twin rfx_<name>_loop"""
        name = f"rfx_{name}_loop" if loop else f"rfx_{name}"
        return getattr(self.lib, name + "_workspace_bytes"), getattr(self.lib, name)

    def _chk_tiles(self, img: torch.Tensor) -> torch.Tensor:
        """tiles as the codec entries read them: an (N, H, W, 3) uint8 batch (`check_tiles`), contiguous, on the plan's device"""
        return self._chk(check_tiles(img))

    def _pcm_out(self, out: T.Optional[torch.Tensor], shape: T.Tuple[int, int, int]) -> torch.Tensor:
        """the (N, L, C) int16 destination of a PCM call: the caller's `out`, checked, or a fresh tensor"""
        if out is None:
            return torch.empty(shape, dtype=torch.int16, device=self.device)
        if out.device != self.device or out.dtype != torch.int16 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int16 tensor of shape {shape} on {self.device}")
        return out

    def _chk_guide(self, guide: torch.Tensor) -> torch.Tensor:
        """a guide as the library reads it: float32 on the plan's device, samples contiguous (a strided view of rows is passed as it is)"""
        if guide.device != self.device:
            raise ValueError(f"tensor on {guide.device}, plan on {self.device}")
        if guide.dtype != torch.float32 or guide.dim() != 2:
            raise ValueError(f"guide must be a (rows, Lg) float32 tensor, got {tuple(guide.shape)} {guide.dtype}")
        ok = guide.stride(1) == 1 and (guide.shape[0] == 1 or guide.stride(0) >= guide.shape[1])
        return guide if ok else guide.contiguous()

    def _chk_hold(self, hold: torch.Tensor, rows: int) -> torch.Tensor:
        """held frames as the library reads them: a contiguous (rows, 2) int32 tensor on the plan's device"""
        if hold.device != self.device:
            raise ValueError(f"tensor on {hold.device}, plan on {self.device}")
        if hold.dtype != torch.int32 or tuple(hold.shape) != (rows, 2):
            raise ValueError(f"hold must be a ({rows}, 2) int32 tensor of (head, tail) frames, got {tuple(hold.shape)} {hold.dtype}")
        return hold.contiguous()

    def _chk_hold_bins(self, hold_bins: torch.Tensor, rows: int, Tn: int) -> torch.Tensor:
        """held bins as the library reads them: a contiguous (rows, Tn, hold_mask_words) int32 tensor of bit masks on the plan's device"""
        if hold_bins.device != self.device:
            raise ValueError(f"tensor on {hold_bins.device}, plan on {self.device}")
        want = (rows, Tn, self.hold_mask_words)
        if hold_bins.dtype not in _MASK_DTYPES or tuple(hold_bins.shape) != want:
            raise ValueError(f"hold_bins must be a {want} int32 tensor of bit masks, got {tuple(hold_bins.shape)} {hold_bins.dtype}")
        return hold_bins.contiguous()

    @property
    def hold_mask_words(self) -> int:
        """words per frame of a masked call's bit mask: ceil(n_stft / 32) (rfx_hold_mask_words)"""
        return int(self.lib.rfx_hold_mask_words(self.handle))

    def hold_bins_from_bands(self, bands: torch.Tensor) -> torch.Tensor:
        """rfx_hold_bins_from_bands: a (B, n_mels, T) bool / uint8 per-band mask (nonzero = held), in the layout of the mel tensor,
        to the (B, T, hold_mask_words) int32 bin mask of `hold_bins=`: a bin is held where every band that reaches it is."""
        if bands.dim() != 3 or bands.shape[1] != self.n_mels:
            raise ValueError(f"expected a (B, {self.n_mels}, T) band mask, got {tuple(bands.shape)}")
        if bands.dtype == torch.bool:
            bands = bands.to(torch.uint8)
        bands = self._chk(bands, torch.uint8)
        B, _, Tn = bands.shape
        out = torch.empty((B, Tn, self.hold_mask_words), dtype=torch.int32, device=self.device)
        check(self.lib.rfx_hold_bins_from_bands(self.handle, bands.data_ptr(), B, Tn, out.data_ptr(), self._stream()))
        return out

    def _stream(self) -> int:
        return current_stream(self.device)

    def pack_magnitudes(self, lin_bft: torch.Tensor) -> torch.Tensor:
        lin_bft = self._chk(lin_bft, torch.float32)
        B, F, Tn = lin_bft.shape
        if F != self.n_stft:
            raise ValueError(f"expected {self.n_stft} linear bins, got {F}")
        out = torch.zeros((B * Tn, self.frame_stride), dtype=torch.float32, device=lin_bft.device)
        check(self.lib.rfx_pack_magnitudes(self.handle, lin_bft.data_ptr(), B, Tn, out.data_ptr(), self._stream()))
        return out

    def pack_complex(self, x_bft: torch.Tensor) -> torch.Tensor:
        x_bft = self._chk(x_bft, torch.complex64)
        B, F, Tn = x_bft.shape
        out = torch.zeros((B * Tn, self.frame_stride), dtype=torch.complex64, device=x_bft.device)
        check(self.lib.rfx_pack_complex(self.handle, x_bft.data_ptr(), B, Tn, out.data_ptr(), self._stream()))
        return out

    def unpack_complex(self, slots: torch.Tensor, B: int, Tn: int) -> torch.Tensor:
        slots = self._chk(slots, torch.complex64)
        out = torch.empty((B, self.n_stft, Tn), dtype=torch.complex64, device=slots.device)
        check(self.lib.rfx_unpack_complex(self.handle, slots.data_ptr(), B, Tn, out.data_ptr(), self._stream()))
        return out

    def _forward_frames(self, Lw: int, shape: T.Sequence[int], loop: bool) -> int:
        """frames a forward call makes of rows of Lw samples, or the call's refusal before any device work.  Plain: torch.stft's count,
        1 + (Lw + 2*(n_fft//2) - n_fft) // hop, and its error for a row no longer than the reflect padding.  loop: the row is one
        period of exactly hop * T samples, T = Lw // hop (`check_loop_samples`)."""
        if loop:
            check_loop_samples(self.hop_length, self.n_fft, Lw)
            return self.lib.rfx_stft_loop_frames(self.handle, Lw)
        if Lw <= self.n_fft // 2:
            # same condition under which torch.stft(pad_mode="reflect") raises in the reference
            raise RuntimeError(
                f"Argument #4: Padding size should be less than the corresponding input dimension, "
                f"but got: padding ({self.n_fft // 2}, {self.n_fft // 2}) at dimension 2 of input {list(shape)}"
            )
        return self.lib.rfx_stft_frames(self.handle, Lw)

    def stft(self, wave: torch.Tensor, want_mag: bool, want_spec: bool, loop: bool = False):
        """rfx_stft, or with `loop` rfx_stft_loop: the rows are whole periods and the transform is circular"""
        wave = self._chk(wave, torch.float32)
        B, Lw = wave.shape
        Tn = self._forward_frames(Lw, wave.shape, loop)
        mag = torch.empty((B * Tn, self.frame_stride), dtype=torch.float32, device=wave.device) if want_mag else None
        spec = torch.empty((B * Tn, self.frame_stride), dtype=torch.complex64, device=wave.device) if want_spec else None
        check(
            (self.lib.rfx_stft_loop if loop else self.lib.rfx_stft)(
                self.handle,
                wave.data_ptr(),
                B,
                Lw,
                mag.data_ptr() if mag is not None else None,
                spec.data_ptr() if spec is not None else None,
                self._stream(),
            )
        )
        return mag, spec, Tn

    def output_samples(self, Tn: int, loop: bool = False) -> int:
        """samples per row of a Griffin-Lim call of Tn frames: hop * (Tn - 1) (+ 1 for an odd n_fft), or the period hop * Tn of a loop call"""
        return (self.lib.rfx_griffinlim_loop_output_samples if loop else self.lib.rfx_griffinlim_output_samples)(self.handle, Tn)

    def _chk_peak_bins(self) -> None:
        if self.n_stft > 10240:
            raise ValueError(f"the spectral-peak start is not served for n_stft = {self.n_stft} above 10240 (RFX_ERR_UNSUPPORTED: a frame must fit the LDS)")

    def _inverse_call(self, entry: str, shape: T.Tuple[int, ...], rows: int, Tn: int, row_base: int, magnitude_hint: float,
                      extras: DecodeExtras, angles0_slots: T.Optional[torch.Tensor] = None) -> T.Tuple[T.Any, int, T.Optional[torch.Tensor]]:
        """What `griffinlim`, `waveform_from_mel` and `audio_from_image` share: the combination rules and this plan's own refusals,
        the extras' tensors as the library reads them, and from them (the call's options, its workspace need in bytes, the injected
        angles as the library reads them).  `entry`: the C entry's name between rfx_ and _workspace_bytes_ex, `shape`: its query's
        arguments; `rows`: the call's Griffin-Lim rows."""
        terms = extras.starts_and_holds()
        rules = functools.partial(check_call_rules, PLAN_WORDING, angles0_slots=angles0_slots, **terms)
        guide, hold, hold_bins = extras.guide, extras.hold, extras.hold_bins
        if extras.loop:
            rules("loop_holds")
            if self.griffinlim_engine == "chirp-z":
                raise ValueError("a loop decode is not served on the chirp-z engine (RFX_ERR_UNSUPPORTED)")
            check_loop_frames(self.hop_length, self.n_fft, Tn)
        if extras.peak_start:
            rules("peak_start")
            self._chk_peak_bins()
        if angles0_slots is not None:
            angles0_slots = self._chk(angles0_slots, torch.complex64)
        if guide is not None:
            rules("two_starts")
            guide = self._chk_guide(guide)
        if hold is not None:
            rules("hold_needs_guide")
            hold = self._chk_hold(hold, rows)
        if hold_bins is not None:
            rules("bins_need_guide", "bins_and_hold")
            hold_bins = self._chk_hold_bins(hold_bins, rows, Tn)
        terms.update(guide=guide, hold=hold, hold_bins=hold_bins)  # (as the library reads them)
        opt = call_options(rows=rows, row_base=row_base, magnitude_hint=magnitude_hint, lstsq=extras.lstsq, **terms)
        opt.keepalive = (guide, hold, hold_bins)  # (a copy `_chk_*` made lives as long as the options that point at it)
        # (0 for options the library refuses: the entry then reports its refusal itself)
        need = getattr(self.lib, f"rfx_{entry}_workspace_bytes_ex")(self.handle, *shape, ctypes.byref(opt))
        return opt, need, angles0_slots

    def peak_start(self, mag_slots: torch.Tensor, B: int, Tn: int) -> torch.Tensor:
        """rfx_peak_start: magnitudes in slot layout -> (B * Tn, frame_stride) complex64 initial angles in the layout `griffinlim`'s
        `angles0_slots` takes (what `pack_complex` makes), built from the magnitudes alone: spectral peaks, their interpolated
        frequencies integrated over the hop.  A row depends on its magnitudes only."""
        mag_slots = self._chk(mag_slots, torch.float32)
        self._chk_peak_bins()
        self._chk_slots(mag_slots, B, Tn)
        out = torch.empty((B * Tn, self.frame_stride), dtype=torch.complex64, device=mag_slots.device)
        if B == 0:
            return out
        with self._workspace(self.lib.rfx_peak_start_workspace_bytes(self.handle, B, Tn)) as ws:
            check(self.lib.rfx_peak_start(self.handle, mag_slots.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def griffinlim(
        self,
        mag_slots: torch.Tensor,
        B: int,
        Tn: int,
        n_iter: int,
        momentum: float = 0.99,
        angles0_slots: T.Optional[torch.Tensor] = None,
        seed: int = 0,
        workspace: T.Optional[torch.Tensor] = None,
        launch_ms: T.Optional[T.Any] = None,
        row_base: int = 0,
        magnitude_hint: float = 0.0,
        guide: T.Optional[torch.Tensor] = None,
        hold: T.Optional[torch.Tensor] = None,
        hold_bins: T.Optional[torch.Tensor] = None,
        loop: bool = False,
        peak_start: bool = False,
        extras: T.Optional[DecodeExtras] = None,
    ) -> torch.Tensor:
        """GriffinLim on magnitudes in slot layout -> (B, samples).  `row_base`: index of the call's first row in the caller's
        whole batch (the random phases of row r are drawn from (seed, row_base + r): chunked and sharded batches get the starts
        of the single call); `magnitude_hint`: an upper bound of the magnitudes if the caller knows one (rfx_call_options).
        `guide`: (B, Lg) float32 waveforms on the plan's device, any units; every row starts from the phase of its guide's STFT
        (the row cut or zero-padded to the output length) instead of random phases (rfx_guided_call_options): no randomness,
        `seed` and `row_base` then change nothing.  `hold`: (B, 2) int32 {head, tail} on the plan's device, with a guide: the
        first `head` and last `tail` frames of a row keep the guide's phase through the iterations (rfx_held_call_options).
        `hold_bins`: (B, Tn, hold_mask_words) int32 bit masks on the plan's device, with a guide and without `hold`: the set bins of
        every frame keep the guide's phase (rfx_masked_call_options; `hold_bins_from_bands` makes them from a mel-band mask).
        `loop`: the Tn columns are one period of a loop (rfx_loop_call_options): circular transforms, (B, hop_length * Tn) samples whose
        end runs into their start; without `hold` / `hold_bins`, Tn at least `loop_min_frames`.
        `peak_start`: start from the spectral-peak phases of the magnitudes (rfx_start_call_options; `peak_start` below) instead of
        random ones: no randomness, without `angles0_slots`, `guide`, `hold` or `hold_bins`.
        `extras`: the five as a ready `DecodeExtras` in place of the keywords (its `lstsq` is not Griffin-Lim's to read)."""
        mag_slots = self._chk(mag_slots, torch.float32)
        extras = DecodeExtras.fold(extras, guide=guide, hold=hold, hold_bins=hold_bins, loop=loop, peak_start=peak_start)
        extras = dataclasses.replace(extras, lstsq=False)  # (the library's Griffin-Lim refuses the flag)
        opt, need, angles0_slots = self._inverse_call("griffinlim", (B, Tn), B, Tn, row_base, magnitude_hint, extras, angles0_slots)
        self._chk_slots(mag_slots, B, Tn)
        if workspace is not None:
            workspace = self._chk(workspace)
        out = torch.empty((B, self.output_samples(Tn, extras.loop)), dtype=torch.float32, device=mag_slots.device)
        # no (or too small a) caller-owned workspace: the plan's arena
        with (self._workspace(need) if workspace is None or workspace.numel() < need else contextlib.nullcontext(workspace)) as ws:
            check(
                self.lib.rfx_griffinlim_ex(
                    self.handle,
                    mag_slots.data_ptr(),
                    angles0_slots.data_ptr() if angles0_slots is not None else None,
                    seed & 0xFFFFFFFFFFFFFFFF,
                    B,
                    Tn,
                    n_iter,
                    momentum,
                    out.data_ptr(),
                    ws.data_ptr(),
                    ws.numel(),
                    self._stream(),
                    ctypes.byref(opt),
                    ctypes.cast(launch_ms, c_void_p) if launch_ms is not None else None,  # ctypes float array of n_iter + 1 entries, filled after a stream sync
                )
            )
        return out

    def spectral_error(self, wave: torch.Tensor, mag_slots: torch.Tensor, B: int, Tn: int, loop: bool = False) -> torch.Tensor:
        """rfx_spectral_error: (B, L) waveforms, L = the samples Griffin-Lim makes of Tn frames, against magnitudes in slot layout
        -> (B, 2) float64, per row sum (|STFT(wave)| - mag)^2 and sum mag^2 over every bin of every frame once.  A row's two
        sums do not depend on the batch it is computed in.  Spectral convergence is sqrt(sums[:, 0] / sums[:, 1]).
        loop (rfx_spectral_error_loop): the rows are the hop * Tn samples of a loop decode and the STFT is the circular one."""
        wave = self._chk(wave, torch.float32)
        mag_slots = self._chk(mag_slots, torch.float32)
        B, Tn = int(B), int(Tn)
        if loop:
            check_loop_frames(self.hop_length, self.n_fft, Tn)
        L = self.output_samples(Tn, loop)
        if tuple(wave.shape) != (B, L):
            raise ValueError(f"{B} rows of {Tn} frames are waveforms of shape {(B, L)}, got {tuple(wave.shape)}")
        self._chk_slots(mag_slots, B, Tn)
        sums = torch.empty((B, 2), dtype=torch.float64, device=self.device)
        if B == 0:
            return sums
        query, entry = self._pair("spectral_error", loop)
        with self._workspace(max(1, query(self.handle, B, Tn))) as ws:
            check(entry(self.handle, wave.data_ptr(), mag_slots.data_ptr(), B, Tn, sums.data_ptr(), ws.data_ptr(),
                                              ws.numel(), self._stream()))
        return sums

    def unpack_magnitudes(self, slots: torch.Tensor, B: int, Tn: int) -> torch.Tensor:
        slots = self._chk(slots, torch.float32)
        out = torch.empty((B, self.n_stft, Tn), dtype=torch.float32, device=slots.device)
        check(self.lib.rfx_unpack_magnitudes(self.handle, slots.data_ptr(), B, Tn, out.data_ptr(), self._stream()))
        return out

    def mel_from_waveform(self, wave: torch.Tensor, loop: bool = False) -> torch.Tensor:
        """spectrogram_converter.py:165-185 on the device: (B, Lw) -> (B, n_mels, T).  loop (rfx_mel_from_waveform_loop): the rows
        are whole periods of hop * T samples and the transform is circular."""
        wave = self._chk(wave, torch.float32)
        B, Lw = wave.shape
        Tn = self._forward_frames(Lw, wave.shape, loop)
        need = (self.lib.rfx_mel_loop_workspace_bytes if loop else self.lib.rfx_mel_workspace_bytes)(self.handle, B, Lw)
        out = torch.empty((B, self.n_mels, Tn), dtype=torch.float32, device=wave.device)
        with self._workspace(need) as ws:
            check(
                (self.lib.rfx_mel_from_waveform_loop if loop else self.lib.rfx_mel_from_waveform)(
                    self.handle, wave.data_ptr(), B, Lw, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()
                )
            )
        return out

    def mel_scale(self, lin_bft: torch.Tensor) -> torch.Tensor:
        """MelScale.forward on (B, n_stft, T) magnitudes through the MFMA projection."""
        lin_bft = self._chk(lin_bft, torch.float32)
        B, F, Tn = lin_bft.shape
        if F != self.n_stft:
            raise ValueError(f"expected {self.n_stft} linear bins, got {F}")
        out = torch.empty((B, self.n_mels, Tn), dtype=torch.float32, device=lin_bft.device)
        with self._workspace(self.lib.rfx_mel_scale_workspace_bytes(self.handle, B, Tn)) as ws:
            check(self.lib.rfx_mel_scale(self.handle, lin_bft.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    # ---- backward of the forward path (include/rfx.h "BACKWARD of the forward path"; riffusion/_autograd.py) ----
    def stft_backward(self, grad_spec_slots: torch.Tensor, B: int, Lw: int) -> torch.Tensor:
        """rfx_stft_backward: the complex gradient of the STFT in slot layout (`pack_complex` of torch's (B, n_stft, T) gradient),
        B * T frames with T = the frames of rows of Lw samples -> the (B, Lw) float32 gradient of the waveform."""
        g = self._chk(grad_spec_slots, torch.complex64)
        Tn = self._forward_frames(Lw, (B, Lw), False)
        if g.numel() != B * Tn * self.frame_stride:
            raise ValueError(f"expected {B} * {Tn} frames of {self.frame_stride} complex slots, got {tuple(g.shape)}")
        out = torch.empty((B, Lw), dtype=torch.float32, device=self.device)
        with self._workspace(self.lib.rfx_stft_backward_workspace_bytes(self.handle, B, Lw)) as ws:
            check(self.lib.rfx_stft_backward(self.handle, g.data_ptr(), B, Lw, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def mel_scale_backward(self, grad_mel: torch.Tensor) -> torch.Tensor:
        """rfx_mel_scale_backward: (B, n_mels, T) -> (B, n_stft, T), the filterbank's adjoint"""
        g = self._chk(grad_mel, torch.float32)
        B, M, Tn = g.shape
        if M != self.n_mels:
            raise ValueError(f"expected {self.n_mels} mel bands, got {M}")
        out = torch.empty((B, self.n_stft, Tn), dtype=torch.float32, device=self.device)
        if B and Tn:
            check(self.lib.rfx_mel_scale_backward(self.handle, g.data_ptr(), B, Tn, out.data_ptr(), None, 0, self._stream()))
        return out

    def mel_from_waveform_backward(self, wave: torch.Tensor, grad_mel: torch.Tensor) -> torch.Tensor:
        """rfx_mel_from_waveform_backward: the (B, Lw) waveform `mel_from_waveform` was given and the (B, n_mels, T) gradient of
        its result -> the (B, Lw) gradient of the waveform.  The spectrum is formed again in the workspace; nothing was kept."""
        wave = self._chk(wave, torch.float32)
        g = self._chk(grad_mel, torch.float32)
        B, Lw = wave.shape
        Tn = self._forward_frames(Lw, wave.shape, False)
        if tuple(g.shape) != (B, self.n_mels, Tn):
            raise ValueError(f"expected a ({B}, {self.n_mels}, {Tn}) gradient, got {tuple(g.shape)}")
        out = torch.empty((B, Lw), dtype=torch.float32, device=self.device)
        with self._workspace(self.lib.rfx_mel_from_waveform_backward_workspace_bytes(self.handle, B, Lw)) as ws:
            check(self.lib.rfx_mel_from_waveform_backward(self.handle, wave.data_ptr(), g.data_ptr(), B, Lw, out.data_ptr(), ws.data_ptr(),
                                                          ws.numel(), self._stream()))
        return out

    # ---- inverse spectrogram (include/rfx.h "INVERSE SPECTROGRAM"; riffusion/_autograd.py: IstftFunction) ----
    def _istft_samples(self, B: int, Tn: int, loop: bool) -> int:
        """samples per row of an inverse-spectrogram call, or its refusal before any device work"""
        if B < 0 or Tn < 1:
            raise ValueError(f"expected B >= 0 rows of Tn >= 1 frames, got B = {B}, Tn = {Tn}")
        if loop:
            if self.griffinlim_engine == "chirp-z":
                raise RuntimeError("the chirp-z engine has no loop synthesis (RFX_ERR_UNSUPPORTED)")
            check_loop_frames(self.hop_length, self.n_fft, Tn)
        L = self.output_samples(Tn, loop)
        if L < 1:
            raise ValueError(f"{Tn} frames give no sample: a plain call needs hop_length * (Tn - 1) + n_fft % 2 >= 1")
        return L

    def istft(self, spec_slots: torch.Tensor, B: int, Tn: int, loop: bool = False) -> torch.Tensor:
        """rfx_istft, or with `loop` rfx_istft_loop: a complex spectrogram in slot layout (`pack_complex` of a (B, n_stft, Tn) tensor,
        or what `stft` returns), B * Tn frames -> the (B, L) float32 waveform torch.istft(center=True) gives, L = `output_samples`."""
        x = self._chk(spec_slots, torch.complex64)
        L = self._istft_samples(B, Tn, loop)
        if x.numel() != B * Tn * self.frame_stride:
            raise ValueError(f"expected {B} * {Tn} frames of {self.frame_stride} complex slots, got {tuple(x.shape)}")
        out = torch.empty((B, L), dtype=torch.float32, device=self.device)
        query, entry = self._pair("istft", loop)
        if B:
            with self._workspace(query(self.handle, B, Tn)) as ws:
                check(entry(self.handle, x.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def istft_backward(self, grad_wave: torch.Tensor, B: int, Tn: int, loop: bool = False, padded: bool = False) -> torch.Tensor:
        """rfx_istft_backward (loop: rfx_istft_backward_loop): the (B, L) float32 gradient of `istft`'s result -> the gradient of the
        spectrum in slot layout, B * Tn frames (`unpack_complex` gives torch's (B, n_stft, Tn) dL/dRe + i dL/dIm).  `padded` (tests,
        plain form): rfx_debug_istft_backward_padded, the circular transform of the zero-padded rows in the zero-extension twin's
        place - the same bytes."""
        if padded and loop:
            raise ValueError("padded is the plain form's test route")
        g = self._chk(grad_wave, torch.float32)
        L = self._istft_samples(B, Tn, loop)
        if tuple(g.shape) != (B, L):
            raise ValueError(f"expected a ({B}, {L}) gradient, got {tuple(g.shape)}")
        out = torch.empty((B * Tn, self.frame_stride), dtype=torch.complex64, device=self.device)
        query, entry = self._pair("debug_istft_backward_padded") if padded else self._pair("istft_backward", loop)
        if B:
            with self._workspace(query(self.handle, B, Tn)) as ws:
                check(entry(self.handle, g.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    # ---- time stretch (include/rfx.h "TIME STRETCH") ----
    def phase_vocoder(self, spec_slots: torch.Tensor, B: int, Tn: int, rate: float) -> T.Tuple[torch.Tensor, int]:
        """rfx_phase_vocoder: a complex spectrogram in slot layout, B * Tn frames (`pack_complex`, or what `stft` returns) -> the
        stretched one in the same layout and its frames per row, ceil(Tn / rate): torchaudio.functional.phase_vocoder with
        TimeStretch's phase advance.  rate == 1 gives a copy."""
        rate = check_stretch_rate(rate)
        x = self._chk(spec_slots, torch.complex64)
        if B < 0 or Tn < 1:
            raise ValueError(f"expected B >= 0 rows of Tn >= 1 frames, got B = {B}, Tn = {Tn}")
        if x.numel() != B * Tn * self.frame_stride:
            raise ValueError(f"expected {B} * {Tn} frames of {self.frame_stride} complex slots, got {tuple(x.shape)}")
        Tout = phase_vocoder_frames(Tn, rate)
        out = torch.empty((B * Tout, self.frame_stride), dtype=torch.complex64, device=self.device)
        if B:
            check(self.lib.rfx_phase_vocoder(self.handle, x.data_ptr(), B, Tn, rate, out.data_ptr(), self._stream()))
        return out, Tout

    def time_stretch_samples(self, Lw: int, rate: float) -> int:
        """samples per row `time_stretch` makes of rows of Lw samples, or the call's refusal before any device work"""
        rate = check_stretch_rate(rate)
        Tout = phase_vocoder_frames(self._forward_frames(Lw, (Lw,), False), rate)
        return self._istft_samples(1, Tout, False)

    def time_stretch(self, wave: torch.Tensor, rate: float) -> torch.Tensor:
        """rfx_time_stretch: (B, Lw) float32 -> (B, hop * (T_out - 1) (+ n_fft % 2)) float32, exactly `istft(phase_vocoder(stft(wave)))`
        on bounded groups of rows."""
        rate = check_stretch_rate(rate)
        wave = self._chk(wave, torch.float32)
        if wave.dim() != 2:
            raise ValueError(f"expected a (B, Lw) waveform, got {tuple(wave.shape)}")
        B, Lw = wave.shape
        L = self.time_stretch_samples(Lw, rate)
        out = torch.empty((B, L), dtype=torch.float32, device=self.device)
        if B:
            with self._workspace(self.lib.rfx_time_stretch_workspace_bytes(self.handle, B, Lw, rate)) as ws:
                check(self.lib.rfx_time_stretch(self.handle, wave.data_ptr(), B, Lw, rate, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    # ---- pitch shift (include/rfx.h "PITCH SHIFT") ----
    def pitch_shift(self, wave: torch.Tensor, n_steps: float, bins_per_octave: int = 12) -> torch.Tensor:
        """rfx_pitch_shift: (B, Lw) float32 -> (B, Lw) float32, torchaudio.functional.pitch_shift at the plan's STFT parameters and
        sample rate: exactly `time_stretch` at rate 2^(-n_steps / bins_per_octave), cut or zero-padded to round(Lw / rate) samples,
        `resample_sinc` from int(sample_rate / rate) to sample_rate, cut or zero-padded to Lw, on bounded groups of rows.
        n_steps == 0 gives a copy.  Where round(Lw / rate) exceeds the stretched row the missing samples are zeros, not the
        untrimmed tail torch.istft(length=) keeps (include/rfx.h states which output samples that can reach)."""
        n_steps, bins_per_octave = check_pitch_steps(n_steps, bins_per_octave)
        wave = self._chk(wave, torch.float32)
        if wave.dim() != 2:
            raise ValueError(f"expected a (B, Lw) waveform, got {tuple(wave.shape)}")
        B, Lw = wave.shape
        if n_steps == 0.0 or B == 0:
            return wave.clone()
        self._forward_frames(Lw, (Lw,), False)  # the refusal of a row too short, before any device work
        orig = int(self.lib.rfx_pitch_shift_resample_freq(self.handle, Lw, n_steps, bins_per_octave))
        need = int(self.lib.rfx_pitch_shift_workspace_bytes(self.handle, B, Lw, n_steps, bins_per_octave))
        if orig < 1 or need < 1:
            raise ValueError(f"pitch_shift: rows of {Lw} samples cannot be shifted by {n_steps} steps of 1/{bins_per_octave} octave "
                             "(the stretched length, the resampler's frequency or its output passes 2^31 - 1, or the stretch gives no sample)")
        sr = self.sample_rate
        first, taps = (None, None) if orig == sr else resample_sinc_table(orig, sr, device=self.device)
        out = torch.empty((B, Lw), dtype=torch.float32, device=self.device)
        with self._workspace(need) as ws:
            check(self.lib.rfx_pitch_shift(self.handle, wave.data_ptr(), B, Lw, n_steps, bins_per_octave, None if first is None else first.data_ptr(),
                                           None if taps is None else taps.data_ptr(), 0 if taps is None else int(taps.shape[0]), out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), self._stream()))
        return out

    # ---- fused spectral losses (include/rfx.h "FUSED SPECTRAL LOSSES"; riffusion/_autograd.py: SpectralLossFunction) ----
    def _loss_args(self, wave: torch.Tensor, mag_slots: torch.Tensor, loop: bool) -> T.Tuple[torch.Tensor, torch.Tensor, int, int, int]:
        wave = self._chk(wave, torch.float32)
        mag_slots = self._chk(mag_slots, torch.float32)
        B, Lw = wave.shape
        Tn = self._forward_frames(Lw, wave.shape, loop)
        self._chk_slots(mag_slots, B, Tn, exact=True)
        return wave, mag_slots, B, Lw, Tn

    def spectral_loss_sums(self, wave: torch.Tensor, mag_slots: torch.Tensor, log_floor: float = 0.0, loop: bool = False) -> torch.Tensor:
        """rfx_spectral_loss: (B, Lw) waveforms against target magnitudes in slot layout (`pack_magnitudes`) -> (B, 3) float64, per row
        sum (|STFT(wave)| - mag)^2, sum mag^2 and sum |ln max(|STFT(wave)|, log_floor) - ln max(mag, log_floor)| over every bin of
        every frame once; the first two are `spectral_error`'s bits.  log_floor 0: no log term, the third sum is 0.
        loop (rfx_spectral_loss_loop): the rows are whole periods of hop * T samples and the STFT is the circular one."""
        wave, mag_slots, B, Lw, _ = self._loss_args(wave, mag_slots, loop)
        f = spectral_loss_floor(log_floor)
        sums = torch.empty((B, 3), dtype=torch.float64, device=self.device)
        if B == 0:
            return sums
        query, entry = self._pair("spectral_loss", loop)
        with self._workspace(max(1, query(self.handle, B, Lw))) as ws:
            check(entry(self.handle, wave.data_ptr(), mag_slots.data_ptr(), B, Lw, f, sums.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return sums

    def spectral_loss_backward(self, wave: torch.Tensor, mag_slots: torch.Tensor, coef: torch.Tensor, log_floor: float = 0.0,
                               loop: bool = False) -> torch.Tensor:
        """rfx_spectral_loss_backward: the waveform and target of `spectral_loss_sums` and the (B, 2) float32 coefficients
        (c_sc, c_lg) of the rows -> the (B, Lw) float32 gradient of the waveform.  The spectrum is formed again in the workspace.
        loop (rfx_spectral_loss_backward_loop): the circular STFT's backward."""
        wave, mag_slots, B, Lw, _ = self._loss_args(wave, mag_slots, loop)
        coef = self._chk(coef, torch.float32)
        if tuple(coef.shape) != (B, 2):
            raise ValueError(f"expected ({B}, 2) coefficients, got {tuple(coef.shape)}")
        f = spectral_loss_floor(log_floor)
        out = torch.empty((B, Lw), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        query, entry = self._pair("spectral_loss_backward", loop)
        with self._workspace(max(1, query(self.handle, B, Lw))) as ws:
            check(entry(self.handle, wave.data_ptr(), mag_slots.data_ptr(), coef.data_ptr(), B, Lw, f, out.data_ptr(), ws.data_ptr(), ws.numel(),
                        self._stream()))
        return out

    def inverse_mel(
        self,
        mel: torch.Tensor,
        channels_per_clip: int,
        spec0: T.Optional[torch.Tensor] = None,
        seed: int = 0,
        row_base: int = 0,
        magnitude_hint: float = 0.0,
    ) -> torch.Tensor:
        """InverseMelScale (SGD): (B, n_mels, T) -> linear magnitudes in slot layout (B*T, stride).  `row_base`,
        `magnitude_hint`: as in `griffinlim` (row_base must be a multiple of channels_per_clip: clips are not split)."""
        mel = self._chk(mel, torch.float32)
        B, M, Tn = mel.shape
        if M != self.n_mels:
            raise ValueError(f"Expected an input with {self.n_mels} mel bins. Found: {M}")  # torchaudio's message
        if spec0 is not None:
            spec0 = self._chk(spec0, torch.float32)
            if tuple(spec0.shape) != (B, Tn, self.n_stft):
                raise ValueError(f"spec0 must be (B, T, n_stft) = {(B, Tn, self.n_stft)}, got {tuple(spec0.shape)}")
        need = self.lib.rfx_inverse_mel_workspace_bytes(self.handle, B, Tn)
        out = torch.empty((B * Tn, self.frame_stride), dtype=torch.float32, device=mel.device)
        opt = call_options(row_base=row_base, magnitude_hint=magnitude_hint)
        with self._workspace(need) as ws:
            check(
                self.lib.rfx_inverse_mel_ex(
                    self.handle,
                    mel.data_ptr(),
                    B,
                    Tn,
                    channels_per_clip,
                    spec0.data_ptr() if spec0 is not None else None,
                    seed & 0xFFFFFFFFFFFFFFFF,
                    out.data_ptr(),
                    ws.data_ptr(),
                    ws.numel(),
                    self._stream(),
                    ctypes.byref(opt),
                )
            )
        return out

    def require_lstsq(self) -> None:
        """Raises ValueError with the library's reason when the closed-form InverseMelScale does not serve this plan's bank
        (host only: nothing is queued on the GPU)."""
        if not self.lstsq_ok:
            why = lstsq_bank_report(self._cparams, self.melfb).why.decode()
            raise ValueError(f'inverse_mel="lstsq" does not serve this filterbank: {why}')

    def inverse_mel_lstsq(self, mel: torch.Tensor) -> torch.Tensor:
        """InverseMelScale, closed form (torchaudio >= 2.1: relu of the minimum-norm least-squares solution): (B, n_mels, T) ->
        linear magnitudes in slot layout (B*T, stride).  No seed: a frame's result depends on its mel column and the plan alone."""
        self.require_lstsq()
        mel = self._chk(mel, torch.float32)
        B, M, Tn = mel.shape
        if M != self.n_mels:
            raise ValueError(f"Expected an input with {self.n_mels} mel bins. Found: {M}")  # torchaudio's message
        out = torch.empty((B * Tn, self.frame_stride), dtype=torch.float32, device=mel.device)
        with self._workspace(max(1, self.lib.rfx_inverse_mel_lstsq_workspace_bytes(self.handle, B, Tn))) as ws:
            check(self.lib.rfx_inverse_mel_lstsq(self.handle, mel.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def inverse_mel_lstsq_backward(self, mel: torch.Tensor, grad_slots: torch.Tensor) -> torch.Tensor:
        """Gradient of `inverse_mel_lstsq` with respect to `mel` (rfx_inverse_mel_lstsq_backward): the forward's (B, n_mels, T) input
        and a gradient over its output in slot layout (B*T, stride) - `pack_magnitudes` of torch's (B, n_stft, T) gradient - ->
        (B, n_mels, T).  The relu's mask is formed again from `mel`; every bin counts once, from its first slot."""
        self.require_lstsq()
        mel = self._chk(mel, torch.float32)
        grad_slots = self._chk(grad_slots, torch.float32)
        B, M, Tn = mel.shape
        if M != self.n_mels:
            raise ValueError(f"Expected an input with {self.n_mels} mel bins. Found: {M}")
        if tuple(grad_slots.shape) != (B * Tn, self.frame_stride):
            raise ValueError(f"grad_slots must be (B*T, stride) = {(B * Tn, self.frame_stride)}, got {tuple(grad_slots.shape)}")
        out = torch.empty((B, M, Tn), dtype=torch.float32, device=mel.device)
        if B * Tn == 0:
            return out
        with self._workspace(max(1, self.lib.rfx_inverse_mel_lstsq_backward_workspace_bytes(self.handle, B, Tn))) as ws:
            check(self.lib.rfx_inverse_mel_lstsq_backward(self.handle, mel.data_ptr(), grad_slots.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(),
                                                          ws.numel(), self._stream()))
        return out

    # ---- guided decode, backward (include/rfx.h "GUIDED DECODE, BACKWARD"; riffusion/_autograd.py: GuidedDecodeFunction) ----
    def _guided_backward_args(self, guide: torch.Tensor, grad_wave: torch.Tensor, B: int, Tn: int, loop: bool) -> T.Tuple[torch.Tensor, torch.Tensor]:
        """the guide and the incoming gradient as the backward entries read them - contiguous (B, Lg) and (B, L) float32 - or the
        refusal of a call the forward refuses, before any device work"""
        if loop:
            if self.griffinlim_engine == "chirp-z":
                raise ValueError("a loop decode is not served on the chirp-z engine (RFX_ERR_UNSUPPORTED)")
            check_loop_frames(self.hop_length, self.n_fft, Tn)
        guide = self._chk_guide(guide).contiguous()
        g = self._chk(grad_wave, torch.float32)
        L = self.output_samples(Tn, loop)
        if guide.shape[0] != B or guide.shape[1] < 1:
            raise ValueError(f"guide must be ({B}, Lg >= 1), got {tuple(guide.shape)}")
        if tuple(g.shape) != (B, L):
            raise ValueError(f"expected a ({B}, {L}) gradient, got {tuple(g.shape)}")
        return guide, g

    def griffinlim_guided_backward(self, guide: torch.Tensor, grad_wave: torch.Tensor, Tn: int, loop: bool = False) -> torch.Tensor:
        """rfx_griffinlim_guided_backward (loop: its loop twin): the gradient of `griffinlim(mag_slots, ..., n_iter=0, guide=guide)` with
        respect to the magnitudes.  guide (B, Lg) float32, grad_wave (B, L) float32 -> (B*Tn, stride) float32 in slot layout, every
        position written.  The guide is analysed again; no gradient flows to it."""
        B = int(grad_wave.shape[0])
        guide, g = self._guided_backward_args(guide, grad_wave, B, Tn, loop)
        out = torch.empty((B * Tn, self.frame_stride), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        query, entry = self._pair("griffinlim_guided_backward", loop)
        with self._workspace(max(1, query(self.handle, B, Tn))) as ws:
            check(entry(self.handle, guide.data_ptr(), guide.shape[1], g.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def waveform_from_mel_guided_backward(self, mel: torch.Tensor, guide: torch.Tensor, grad_wave: torch.Tensor, loop: bool = False) -> torch.Tensor:
        """rfx_waveform_from_mel_guided_backward (loop: its loop twin): the gradient of
        `waveform_from_mel(mel, ..., n_iter=0, lstsq=True, guide=guide)` with respect to `mel` - `griffinlim_guided_backward`, then
        `inverse_mel_lstsq_backward`, in one workspace: the same bytes.  mel (B, n_mels, T), guide (B, Lg), grad_wave (B, L) ->
        (B, n_mels, T)."""
        self.require_lstsq()
        mel = self._chk(mel, torch.float32)
        B, M, Tn = mel.shape
        if M != self.n_mels:
            raise ValueError(f"Expected an input with {self.n_mels} mel bins. Found: {M}")
        guide, g = self._guided_backward_args(guide, grad_wave, B, Tn, loop)
        out = torch.empty((B, M, Tn), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        query, entry = self._pair("waveform_from_mel_guided_backward", loop)
        with self._workspace(max(1, query(self.handle, B, Tn))) as ws:
            check(entry(self.handle, mel.data_ptr(), guide.data_ptr(), guide.shape[1], g.data_ptr(), B, Tn, out.data_ptr(), ws.data_ptr(), ws.numel(),
                        self._stream()))
        return out

    # ---- codecs (no plan state needed, kept here for one binding site) -------------------------
    def image_decode(self, img_u8: torch.Tensor, stereo: bool, lut: torch.Tensor) -> torch.Tensor:
        """(N, H, W, 3) uint8 -> (N*C, H, W) float32."""
        img_u8 = self._chk_tiles(img_u8)
        lut = self._chk(lut, torch.float32)
        N, H, W, _ = img_u8.shape
        C = 2 if stereo else 1
        out = torch.empty((N * C, H, W), dtype=torch.float32, device=img_u8.device)
        check(self.lib.rfx_image_decode_u8(img_u8.data_ptr(), N, H, W, int(stereo), lut.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def image_encode(self, mel: torch.Tensor, stereo: bool, thresholds: torch.Tensor):
        """(N*C, M, T) float32 -> ((N, M, T, 3) uint8, per-clip max (N,))."""
        mel = self._chk(mel, torch.float32)
        thresholds = self._chk(thresholds, torch.float32)
        C = 2 if stereo else 1
        NC, M, Tn = mel.shape
        if NC % C:
            raise ValueError("batch must be a multiple of the channel count")
        N = NC // C
        img = torch.empty((N, M, Tn, 3), dtype=torch.uint8, device=mel.device)
        mx = torch.empty((N,), dtype=torch.float32, device=mel.device)
        check(self.lib.rfx_image_encode_u8(mel.data_ptr(), N, M, Tn, int(stereo), thresholds.data_ptr(), mx.data_ptr(), img.data_ptr(), self._stream()))
        return img, mx

    def resize_images(self, img_u8: torch.Tensor, out_h: int, out_w: int, resample: int) -> torch.Tensor:
        """PIL.Image.resize((out_w, out_h), resample) of every (H, W, 3) uint8 tile of an (N, H, W, 3) batch on this device, byte
        for byte (rfx_image_resize_u8; resample: PIL's LANCZOS, BILINEAR or BICUBIC).  Each axis's table is built on the host once
        per (in, out, filter) and kept on the device like the decode LUT."""
        img = self._chk_tiles(img_u8)
        resample, out_h, out_w = int(resample), int(out_h), int(out_w)
        if resample not in RESIZE_FILTERS:
            raise ValueError(f"resample must be one of PIL's {sorted(RESIZE_FILTERS.values())} ({sorted(RESIZE_FILTERS)}), got {resample}")
        N, H, W, _ = img.shape
        out = torch.empty((N, out_h, out_w, 3), dtype=torch.uint8, device=self.device)
        if N == 0:
            return out

        def table(n_in: int, n_out: int) -> T.Tuple[T.Optional[int], T.Optional[int]]:
            if n_in == n_out:
                return None, None
            t = self.device_constant(("resize", n_in, n_out, resample), lambda: resize_coefficients(n_in, n_out, resample))
            return t.data_ptr(), t.data_ptr() + 8 * n_out

        bx, kx = table(W, out_w)
        by, ky = table(H, out_h)
        need = self.lib.rfx_image_resize_workspace_bytes(N, H, W, out_h, out_w, resample)
        with self._workspace(max(need, 1)) as ws:
            check(self.lib.rfx_image_resize_u8(img.data_ptr(), N, H, W, out_h, out_w, resample, bx, kx, by, ky, out.data_ptr(),
                                               ws.data_ptr(), ws.numel(), self._stream()))
        return out

    @staticmethod
    def _used_bytes(ws: torch.Tensor, need: int, cap: int, sizes: T.List[int]) -> T.List[bytes]:
        """Image n's `sizes[n]` bytes at ws[need + n * cap], for every n: joined on the device, one copy down -> N `bytes`."""
        rows = ws[need:need + len(sizes) * cap].view(len(sizes), cap)
        return split_packed(torch.cat([rows[n, :size] for n, size in enumerate(sizes)]).cpu().numpy().tobytes(), sizes)

    def jpeg_scans(self, img_u8: torch.Tensor, quality: int = 75) -> T.List[bytes]:
        """The entropy-coded scan and EOI of every (H, W, 3) uint8 tile of an (N, H, W, 3) batch as Pillow's
        `Image.save(f, "JPEG", quality=quality)` writes them (rfx_jpeg_encode_u8) -> N `bytes`; a file is
        `image_util.jpeg_header(...)` + its scan.  The sizes are read once (the call's one synchronisation), then the used bytes of
        all scans come down in one copy.  Scans and scratch space come from the plan's arena."""
        img = self._chk_tiles(img_u8)
        N, H, W, _ = img.shape
        if N == 0:
            return []
        qt = self.device_constant(("jpeg_qtables", int(quality)), lambda: jpeg_quant_tables(quality).view(np.int16))
        cap = self.lib.rfx_jpeg_scan_capacity(H, W)
        need = self.lib.rfx_jpeg_encode_workspace_bytes(N, H, W)
        if cap == 0 or need == 0:  # a size the library refuses: its own words (nothing is launched)
            check(self.lib.rfx_jpeg_encode_u8(img.data_ptr(), N, H, W, qt.data_ptr(), None, None, None, self._stream()))
            raise RfxError(f"rfx_jpeg_encode_u8 took a {H} x {W} image it reports no capacity for")
        need = (need + 255) // 256 * 256
        sizes_d = torch.empty((N,), dtype=torch.int32, device=self.device)
        with self._workspace(need + N * cap) as ws:
            check(self.lib.rfx_jpeg_encode_u8(img.data_ptr(), N, H, W, qt.data_ptr(), ws.data_ptr() + need, sizes_d.data_ptr(), ws.data_ptr(),
                                              self._stream()))
            sizes = [int(v) for v in sizes_d.cpu()]
            if min(sizes) < 2 or max(sizes) > cap:
                raise RfxError(f"rfx_jpeg_encode_u8 reported scan sizes outside 2 .. {cap}")
            return self._used_bytes(ws, need, cap, sizes)

    def png_streams(self, img_u8: torch.Tensor, mode: str = "rgb") -> T.Tuple[T.List[bytes], np.ndarray, np.ndarray]:
        """The IDAT payload (a zlib stream: run-length + Huffman deflate, csrc/rfx_png_core.h) of every (H, W, 3) uint8 tile of an
        (N, H, W, 3) batch (rfx_png_encode_u8) -> (N `bytes`, the (N,) uint32 CRC-32 of b"IDAT" + stream, the (N,) int32 channels
        each tile was written with: 3, 1, or 0 where mode "gray" met a colour tile, whose stream is empty).  A file is
        `image_util.png_file(...)`.  mode: "rgb", "gray", or "auto" (grey where R = G = B, decided on the device).  The sizes, CRCs
        and channels are read once (the call's one synchronisation), then the used bytes of all streams come down in one copy."""
        img = self._chk_tiles(img_u8)
        if mode not in PNG_MODES:
            raise ValueError(f"mode must be one of {sorted(PNG_MODES)}, got {mode!r}")
        N, H, W, _ = img.shape
        if N == 0:
            return [], np.zeros(0, np.uint32), np.zeros(0, np.int32)
        m = PNG_MODES[mode]
        cap = self.lib.rfx_png_stream_capacity(H, W, 1 if m == 1 else 3)
        need = self.lib.rfx_png_encode_workspace_bytes(N, H, W)
        if cap == 0 or need == 0:  # a size the library refuses: its own words (nothing is launched)
            check(self.lib.rfx_png_encode_u8(img.data_ptr(), N, H, W, m, None, None, None, None, None, self._stream()))
            raise RfxError(f"rfx_png_encode_u8 took a {H} x {W} image it reports no capacity for")
        need = (need + 255) // 256 * 256
        meta_d = torch.empty((3, N), dtype=torch.int32, device=self.device)  # sizes, CRCs, channels
        with self._workspace(need + N * cap) as ws:
            check(self.lib.rfx_png_encode_u8(img.data_ptr(), N, H, W, m, ws.data_ptr() + need, meta_d[0].data_ptr(), meta_d[1].data_ptr(),
                                             meta_d[2].data_ptr(), ws.data_ptr(), self._stream()))
            meta = meta_d.cpu().numpy()
            sizes = [int(v) for v in meta[0]]
            if min(sizes) < 0 or max(sizes) > cap:
                raise RfxError(f"rfx_png_encode_u8 reported stream sizes outside 0 .. {cap}")
            return self._used_bytes(ws, need, cap, sizes), meta[1].view(np.uint32).copy(), meta[2].copy()

    def _run_decode(self, N: int, need: int, call: T.Callable[[int, T.Optional[int]], int], refused: str) -> np.ndarray:
        """`call(d_status, d_workspace)`, a decode entry, on a borrowed workspace of `need` bytes -> the (N,) int32 status, read back.
        `need == 0`: arguments the library refuses - its own words (nothing is launched), or `refused` should it take them."""
        status = torch.empty((N,), dtype=torch.int32, device=self.device)
        if need == 0:
            check(call(status.data_ptr(), None))
            raise RfxError(refused)
        with self._workspace(need) as ws:
            check(call(status.data_ptr(), ws.data_ptr()))
            return status.cpu().numpy()

    def jpeg_decode(self, scans: T.Sequence[bytes], H: int, W: int, qtables: np.ndarray, huffman: np.ndarray) -> T.Tuple[torch.Tensor, np.ndarray]:
        """N baseline 4:2:0 JPEG scans of H x W images (the entropy-coded bytes between the SOS header and EOI, with each image's
        (2, 64) quantisation tables in natural order and (4, 272) Huffman tables: `image_util.jpeg_parse`) -> the (N, H, W, 3) uint8
        pixels Pillow decodes, on this device, and the (N,) int32 status of every image (rfx_jpeg_decode_u8; 0: decoded, anything
        else: that image's pixels are undefined).  Offsets, tables and scans go up in one copy; reading the status is the call's
        one synchronisation."""
        N, H, W = len(scans), int(H), int(W)
        qtables = np.ascontiguousarray(qtables, dtype=np.uint16).reshape(N, 2, 64)
        huffman = np.ascontiguousarray(huffman, dtype=np.uint8).reshape(N, 4, 272)
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=self.device)
        if N == 0:
            return out, np.zeros(0, np.int32)
        host, offsets, at = pack_streams(scans, [qtables, huffman])
        up = torch.from_numpy(host).to(self.device)  # the one upload
        base = up.data_ptr()
        return out, self._run_decode(
            N, self.lib.rfx_jpeg_decode_workspace_bytes(N, H, W, int(offsets[-1])),
            lambda d_status, d_ws: self.lib.rfx_jpeg_decode_u8(base + at[3], offsets.ctypes.data, base, N, H, W, base + at[1], base + at[2],
                                                               out.data_ptr(), d_status, d_ws, self._stream()),
            f"rfx_jpeg_decode_u8 took {N} {H} x {W} images it reports no workspace for")

    def png_decode(self, streams: T.Sequence[bytes], H: int, W: int, color_type: int, palettes: T.Optional[np.ndarray] = None,
                   palette_entries: T.Optional[np.ndarray] = None) -> T.Tuple[torch.Tensor, np.ndarray]:
        """N zlib streams of H x W PNG images of one colour type (0, 2, 3 or 6; bit depth 8, not interlaced) - each the file's IDAT
        payloads concatenated: `image_util.png_parse` - with, for colour type 3, each image's (256, 3) palette and its entry count
        -> the (N, H, W, 3) uint8 pixels Pillow's `convert("RGB")` gives, on this device, and the (N,) int32 status of every image
        (rfx_png_decode_u8; 0: decoded, anything else: that image's pixels are undefined).  Offsets, palettes and streams go up in
        one copy; reading the status is the call's one synchronisation."""
        N = len(streams)
        H, W, color_type = int(H), int(W), int(color_type)
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=self.device)
        if N == 0:
            return out, np.zeros(0, np.int32)
        tables: T.List[np.ndarray] = []  # colour type 3: [entries, palettes]
        if color_type == 3:
            if palettes is None or palette_entries is None:
                raise ValueError("colour type 3 needs palettes and palette_entries")
            tables = [np.ascontiguousarray(palette_entries, dtype=np.int32).reshape(N), np.ascontiguousarray(palettes, dtype=np.uint8).reshape(N, 768)]
        host, offsets, at = pack_streams(streams, tables)
        up = torch.from_numpy(host).to(self.device)  # the one upload
        base = up.data_ptr()
        return out, self._run_decode(
            N, self.lib.rfx_png_decode_workspace_bytes(N, H, W, color_type, int(offsets[-1])),
            lambda d_status, d_ws: self.lib.rfx_png_decode_u8(base + at[-1], offsets.ctypes.data, base, N, H, W, color_type,
                                                              base + at[2] if tables else None, base + at[1] if tables else None,
                                                              out.data_ptr(), d_status, d_ws, self._stream()),
            f"rfx_png_decode_u8 took {N} {H} x {W} images of colour type {color_type} it reports no workspace for")

    def waveform_from_mel(self, mel: torch.Tensor, channels_per_clip: int, n_iter: int, momentum: float = 0.99, seed: int = 0,
                          row_base: int = 0, magnitude_hint: float = 0.0, lstsq: bool = False, guide: T.Optional[torch.Tensor] = None,
                          hold: T.Optional[torch.Tensor] = None, hold_bins: T.Optional[torch.Tensor] = None, loop: bool = False,
                          peak_start: bool = False, extras: T.Optional[DecodeExtras] = None) -> torch.Tensor:
        """spectrogram_converter.py:187-204 in one call: (B, n_mels, T) -> (B, hop * (T - 1)); `inverse_mel` (seed) + `griffinlim`
        (seed + 1), same bits, the linear magnitudes stay in the workspace.  `lstsq`: `inverse_mel_lstsq` in place of the SGD.
        `guide`: (B, Lg) float32 waveforms, `hold`: (B, 2) int32 held frames, `hold_bins`: (B, T, hold_mask_words) int32 held bins, as in
        `griffinlim`; `loop`: a loop decode, (B, hop * T) samples, as in `griffinlim`; `peak_start`: Griffin-Lim starts from the
        spectral-peak phases of the linear magnitudes (`peak_start`), as in `griffinlim`.  `extras`: the six as a ready `DecodeExtras`
        in place of the keywords."""
        extras = DecodeExtras.fold(extras, guide=guide, hold=hold, hold_bins=hold_bins, loop=loop, peak_start=peak_start, lstsq=lstsq)
        if extras.lstsq:
            self.require_lstsq()
        mel = self._chk(mel, torch.float32)
        B, M, Tn = mel.shape
        if M != self.n_mels:
            raise ValueError(f"Expected an input with {self.n_mels} mel bins. Found: {M}")  # torchaudio's message
        opt, need, _ = self._inverse_call("waveform_from_mel", (B, Tn), B, Tn, row_base, magnitude_hint, extras)
        out = torch.empty((B, self.output_samples(Tn, extras.loop)), dtype=torch.float32, device=mel.device)
        with self._workspace(need) as ws:
            check(self.lib.rfx_waveform_from_mel_ex(self.handle, mel.data_ptr(), B, Tn, channels_per_clip, seed & 0xFFFFFFFFFFFFFFFF, n_iter, momentum,
                                                    out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(), ctypes.byref(opt)))
        return out

    def audio_from_image_workspace(self, N: int, stereo: bool, Tn: int) -> torch.Tensor:
        """A caller-owned workspace for `audio_from_image` calls of up to N images of Tn frames (optional since round 6: without
        one the call borrows a buffer from the plan's arena)."""
        return torch.empty(self.lib.rfx_audio_from_image_workspace_bytes(self.handle, N, int(stereo), Tn), dtype=torch.uint8, device=self.device)

    def audio_from_image(self, img: torch.Tensor, stereo: bool, lut: torch.Tensor, n_iter: int, momentum: float = 0.99, seed: int = 0,
                         normalize: bool = True, out: T.Optional[torch.Tensor] = None, workspace: T.Optional[torch.Tensor] = None,
                         clip_base: int = 0, magnitude_hint: float = 0.0, lstsq: bool = False, guide: T.Optional[torch.Tensor] = None,
                         hold: T.Optional[torch.Tensor] = None, hold_bins: T.Optional[torch.Tensor] = None, loop: bool = False,
                         peak_start: bool = False, extras: T.Optional[DecodeExtras] = None):
        """spectrogram_image_converter.py:54-91 on the device in one call: (N, n_mels, T, 3) uint8 -> ((N, L, C) int16, per-clip peak (N,));
        `image_decode` + `waveform_from_mel` (clips of C rows) + `pcm16`, same bytes.  `out` as in `pcm16`.  `clip_base`: index of
        the call's first image in the caller's whole batch (row_base = clip_base * C); `magnitude_hint`: the image path's
        max_value (the largest entry of `lut`); `lstsq`: the closed-form InverseMelScale in place of the SGD; `guide`: (N * C, Lg)
        float32 waveforms, image after image and channel after channel, as in `griffinlim`; `hold`: (N * C, 2) int32 held frames, row
        for row with the guide; `hold_bins`: (N * C, T, hold_mask_words) int32 held bins, row for row as well; `loop`: a loop decode,
        L = hop * T PCM frames per clip, as in `griffinlim`; `peak_start`: the spectral-peak start, as in `griffinlim`.  `extras`: the
        six as a ready `DecodeExtras` in place of the keywords."""
        extras = DecodeExtras.fold(extras, guide=guide, hold=hold, hold_bins=hold_bins, loop=loop, peak_start=peak_start, lstsq=lstsq)
        img = self._chk_tiles(img)
        if extras.lstsq:
            self.require_lstsq()
        lut = self._chk(lut, torch.float32)
        N, H, W, _ = img.shape
        if H != self.n_mels:
            raise ValueError(f"expected (N, {self.n_mels}, T, 3) uint8 images, got {tuple(img.shape)}")
        C = 2 if stereo else 1
        opt, need, _ = self._inverse_call("audio_from_image", (N, int(stereo), W), N * C, W, clip_base * C, magnitude_hint, extras)
        L = self.output_samples(W, extras.loop)
        pcm = self._pcm_out(out, (N, L, C))
        if workspace is not None:
            workspace = self._chk(workspace)
        peak = torch.zeros((N,), dtype=torch.float32, device=img.device)
        with (self._workspace(need) if workspace is None or workspace.numel() < need else contextlib.nullcontext(workspace)) as ws:
            check(self.lib.rfx_audio_from_image_u8_ex(self.handle, img.data_ptr(), N, W, int(stereo), lut.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, n_iter, momentum,
                                                      int(normalize), peak.data_ptr(), pcm.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(), ctypes.byref(opt)))
        return pcm, peak

    def image_from_waveform(self, wave: torch.Tensor, stereo: bool, thresholds: torch.Tensor, loop: bool = False):
        """spectrogram_image_converter.py:30-51 on the device: (N*C, Lw) float32 -> ((N, n_mels, T, 3) uint8, per-clip max (N,));
        `mel_from_waveform` + `image_encode` in one call, byte for byte, without the (N*C, n_mels, T) tensor in between.
        loop (rfx_image_from_waveform_loop): the rows are whole periods of hop * T samples and the transform is circular."""
        wave = self._chk(wave, torch.float32)
        thresholds = self._chk(thresholds, torch.float32)
        C = 2 if stereo else 1
        NC, Lw = wave.shape
        if NC % C:
            raise ValueError("batch must be a multiple of the channel count")
        Tn = self._forward_frames(Lw, wave.shape, loop)
        N = NC // C
        img = torch.empty((N, self.n_mels, Tn, 3), dtype=torch.uint8, device=wave.device)
        mx = torch.empty((N,), dtype=torch.float32, device=wave.device)
        query, entry = self._pair("image_from_waveform", loop)
        with self._workspace(query(self.handle, N, int(stereo), Lw)) as ws:
            check(entry(self.handle, wave.data_ptr(), N, int(stereo), Lw, thresholds.data_ptr(), mx.data_ptr(),
                        img.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return img, mx

    def pcm16(self, wave: torch.Tensor, channels: int, normalize: bool = True, out: T.Optional[torch.Tensor] = None):
        """(N*C, L) float32 -> ((N, L, C) int16, per-clip peak (N,)).  `out`: preallocated contiguous (N, L, C) int16
        destination on this device (e.g. the rows of a batch-wide result), otherwise a fresh tensor."""
        wave = self._chk(wave, torch.float32)
        NC, L = wave.shape
        if NC % channels:
            raise ValueError("batch must be a multiple of the channel count")
        N = NC // channels
        pcm = self._pcm_out(out, (N, L, channels))
        peak = torch.zeros((N,), dtype=torch.float32, device=wave.device)
        check(self.lib.rfx_pcm16(wave.data_ptr(), N, channels, L, int(normalize), peak.data_ptr(), pcm.data_ptr(), self._stream()))
        return pcm, peak

    # ---- int16 post-processing (rfx_pcm.hip): audio_util.apply_filters / stitch_segments on the device ----------------------
    def filter_tables(self) -> T.Tuple[torch.Tensor, torch.Tensor]:
        """The two host-built tables of rfx_pcm16_apply_filters (gain by rms, boost by peak), uploaded once per plan."""
        from riffusion.util import audio_util

        return (self.device_constant(("pcm_gain_by_rms",), lambda: audio_util.filter_gain_by_rms().copy()),
                self.device_constant(("pcm_boost_by_peak", 0.1), lambda: audio_util.filter_boost_by_peak().copy()))

    def compress_tables(self) -> T.Tuple[int, T.Tuple[torch.Tensor, ...]]:
        """look_frames and the device copies of audio_util.compress_tables at this plan's rate (pydub's defaults), and the
        -10 dBFS gain table: uploaded once per plan."""
        from riffusion.util import audio_util

        rate = self.sample_rate
        look = audio_util.compress_tables(rate)[0]
        tabs = tuple(self.device_constant(("pcm_compress", rate, i), lambda i=i: audio_util.compress_tables(rate)[i].copy())
                     for i in range(1, 5))
        gain10 = self.device_constant(("pcm_gain_by_rms", -10), lambda: audio_util.filter_gain_by_rms(-10).copy())
        return look, tabs + (gain10,)

    def apply_filters(self, pcm: torch.Tensor, out: T.Optional[torch.Tensor] = None, compression: bool = False, *,
                      compress_form: str = "chunked", chunk_frames: int = 0, margin: float = COMPRESS_MARGIN,
                      flag_capacity: int = 1 << 16, stats: T.Optional[dict] = None) -> torch.Tensor:
        """audio_util.apply_filters(compression) on every clip of an (N, L, C) int16 batch on this device, byte for byte
        (audioop's arithmetic; clips of L * C < 2^23 samples).  `out`: destination of the same shape, `pcm` itself for in place;
        otherwise a fresh tensor.

        compression=True (rfx_pcm16_apply_filters_compressed, at this plan's sample rate): `compress_form` "chunked" or
        "sequential" and `chunk_frames` choose how the compressor's recurrence runs (same bytes); products within `margin` of an
        integer are recomputed with the host's pow, at most `flag_capacity` of them per call - beyond that the batch is filtered
        on the host.  This path synchronises the stream once (the flag count).  `stats`, when given, receives "n_flagged",
        "host_fallback" and "rounds" (the repair rounds per clip, a device tensor)."""
        from riffusion.util import audio_util

        if pcm.dtype != torch.int16 or pcm.dim() != 3:
            raise ValueError(f"expected an (N, L, C) int16 batch, got {tuple(pcm.shape)} {pcm.dtype}")
        N, L, C = pcm.shape
        if L * C >= audio_util.FILTER_EXACT_SAMPLES:
            raise ValueError(f"clips of {L} x {C} samples: the device filters are exact below 2^23 samples per clip")
        if out is not None and out.data_ptr() == pcm.data_ptr() and not pcm.is_contiguous():
            raise ValueError("in place needs a contiguous batch")
        src = self._chk(pcm)
        out = self._pcm_out(out, (N, L, C))
        if N == 0:
            return out
        gain, boost = self.filter_tables()
        if compression:
            return self._apply_filters_compressed(src, out, gain, boost, compress_form, chunk_frames, margin, flag_capacity, stats)
        with self._workspace(self.lib.rfx_pcm16_filters_workspace_bytes(N, L, C)) as ws:
            check(self.lib.rfx_pcm16_apply_filters(src.data_ptr(), N, L, C, gain.data_ptr(), boost.data_ptr(), out.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def _apply_filters_compressed(self, src: torch.Tensor, out: torch.Tensor, gain12: torch.Tensor, boost: torch.Tensor, form: str,
                                  chunk_frames: int, margin: float, flag_capacity: int, stats: T.Optional[dict]) -> torch.Tensor:
        from riffusion.util import audio_util

        if form not in COMPRESS_FORMS:
            raise ValueError(f"compress_form must be one of {sorted(COMPRESS_FORMS)}, got {form!r}")
        N, L, C = src.shape
        look, (above, max_att, inc, dec, gain10) = self.compress_tables()
        flags = torch.empty(max(1, flag_capacity) * COMPRESS_FLAG_BYTES, dtype=torch.uint8, device=self.device)
        rounds = torch.zeros(N, dtype=torch.int32, device=self.device)
        o = RfxCompressOptions(ctypes.sizeof(RfxCompressOptions), COMPRESS_FORMS[form], look, int(chunk_frames), gain10.data_ptr(),
                               gain12.data_ptr(), boost.data_ptr(), above.data_ptr(), max_att.data_ptr(), inc.data_ptr(),
                               dec.data_ptr(), float(margin), flags.data_ptr(), int(flag_capacity), rounds.data_ptr(), 0)
        with self._workspace(self.lib.rfx_pcm16_compress_filters_workspace_bytes(N, L, C)) as ws:
            check(self.lib.rfx_pcm16_apply_filters_compressed(src.data_ptr(), N, L, C, ctypes.byref(o), out.data_ptr(), ws.data_ptr(),
                                                              ws.numel(), self._stream()))
        fallback = o.n_flagged > flag_capacity
        if fallback:  # the flag list overflowed: out is unwritten and src intact - this batch is filtered on the host
            host = src.cpu().numpy()
            res = np.stack([audio_util.apply_filters(audio_util.PcmSegment(c, self.sample_rate), compression=True)._data for c in host])
            out.copy_(torch.from_numpy(res))
        if stats is not None:
            stats.update(n_flagged=int(o.n_flagged), host_fallback=bool(fallback), rounds=rounds)
        return out

    def stitch(self, pcm: torch.Tensor, frame_rate: int, crossfade_s: float) -> torch.Tensor:
        """audio_util.stitch_segments of the N clips of an (N, L, C) int16 batch on this device -> (frames, C) int16, byte for
        byte: audio_util.stitch_plan resolves pydub's millisecond arithmetic on the host, one kernel writes the samples."""
        from riffusion.util import audio_util

        if pcm.dtype != torch.int16 or pcm.dim() != 3:
            raise ValueError(f"expected an (N, L, C) int16 batch, got {tuple(pcm.shape)} {pcm.dtype}")
        pcm = self._chk(pcm)
        N, L, C = pcm.shape
        pieces, frames = audio_util.stitch_plan(N, L, frame_rate, crossfade_s)
        host = torch.from_numpy(pieces.view(np.uint8))
        dev = host.to(self.device)
        out = torch.empty((frames, C), dtype=torch.int16, device=self.device)
        check(self.lib.rfx_pcm16_stitch(pcm.data_ptr(), N, L, C, host.data_ptr(), dev.data_ptr(), len(pieces), frames, out.data_ptr(),
                                        self._stream()))
        return out


    # ---- int16 front end of the encode (rfx_pcm_in.hip): set_channels / set_frame_rate and the clip slicing on the device ---------
    def _chk_pcm(self, pcm: torch.Tensor) -> torch.Tensor:
        if pcm.dtype != torch.int16 or pcm.dim() != 2 or pcm.shape[1] not in (1, 2):
            raise ValueError(f"expected a (frames, 1 or 2) int16 recording, got {tuple(pcm.shape)} {pcm.dtype}")
        return self._chk(pcm)

    def resample_pcm(self, pcm: torch.Tensor, in_rate: int, out_rate: int, out_channels: T.Optional[int] = None) -> torch.Tensor:
        """PcmSegment / pydub `.set_channels(out_channels).set_frame_rate(out_rate)` of a (frames, C) int16 recording on this
        device, byte for byte (rfx_pcm16_resample: audioop.tomono / tostereo on the stored frames, then audioop.ratecv) ->
        (out_frames, out_channels) int16.  Equal rates only mix (or copy)."""
        pcm = self._chk_pcm(pcm)
        L, C = pcm.shape
        C_out = C if out_channels is None else int(out_channels)
        if C_out not in (1, 2):
            raise ValueError(f"out_channels must be 1 or 2, got {out_channels}")
        if L == 0:  # audioop.ratecv of no frames
            return torch.empty((0, C_out), dtype=torch.int16, device=self.device)
        K = resample_frames(L, in_rate, out_rate)
        out = torch.empty((K, C_out), dtype=torch.int16, device=self.device)
        check(self.lib.rfx_pcm16_resample(pcm.data_ptr(), L, C, int(in_rate), C_out, int(out_rate), out.data_ptr(), K, self._stream()))
        return out

    def _clip_starts(self, starts: T.Any, Lw: int) -> T.Tuple[torch.Tensor, torch.Tensor]:
        if not 0 < int(Lw) <= CLIP_FRAMES_MAX:  # the C entries take Lw as an int
            raise ValueError(f"clips must hold 1 .. {CLIP_FRAMES_MAX} frames, got {Lw}")
        host = torch.as_tensor(np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1)))
        return host, host.to(self.device)

    def clips_to_waveform(self, pcm: torch.Tensor, starts: T.Any, Lw: int, out_channels: int) -> torch.Tensor:
        """Clips of `Lw` frames at the frame offsets `starts` of a (frames, C) int16 recording on this device, mixed to
        `out_channels` after the slice -> (N * out_channels, Lw) float32: what
        `np.array([c.get_array_of_samples() for c in clip.set_channels(out_channels).split_to_mono()]).astype(np.float32)` gives
        for every clip, bit for bit (rfx_pcm16_clips_to_waveform).  A clip outside the recording is refused before any launch."""
        pcm = self._chk_pcm(pcm)
        L, C = pcm.shape
        host, dev = self._clip_starts(starts, Lw)
        N = int(host.numel())
        out = torch.empty((N * int(out_channels), int(Lw)), dtype=torch.float32, device=self.device)
        check(self.lib.rfx_pcm16_clips_to_waveform(pcm.data_ptr(), L, C, host.data_ptr(), dev.data_ptr(), N, int(Lw), int(out_channels),
                                                   out.data_ptr(), self._stream()))
        return out

    def image_from_pcm_clips(self, pcm: torch.Tensor, starts: T.Any, Lw: int, stereo: bool, thresholds: torch.Tensor, loop: bool = False):
        """`clips_to_waveform` (to 2 channels when `stereo`, else 1) + `image_from_waveform` in one call
        (rfx_image_from_pcm16_clips), same bytes: (frames, C) int16 -> ((N, n_mels, T, 3) uint8, per-clip max (N,)).  The float
        waveforms live in the call's workspace only.  loop (rfx_image_from_pcm16_clips_loop): every clip is a whole period of
        Lw = hop * T frames and the transform is circular."""
        pcm = self._chk_pcm(pcm)
        thresholds = self._chk(thresholds, torch.float32)
        L, C = pcm.shape
        Lw = int(Lw)
        if loop:
            check_loop_samples(self.hop_length, self.n_fft, Lw)
        host, dev = self._clip_starts(starts, Lw)
        N = int(host.numel())
        Tn = self._forward_frames(Lw, [N * (2 if stereo else 1), Lw], loop)
        img = torch.empty((N, self.n_mels, Tn, 3), dtype=torch.uint8, device=self.device)
        mx = torch.empty((N,), dtype=torch.float32, device=self.device)
        if N == 0:
            return img, mx
        query, entry = self._pair("image_from_pcm16_clips", loop)
        with self._workspace(query(self.handle, N, int(stereo), Lw)) as ws:
            check(entry(self.handle, pcm.data_ptr(), L, C, host.data_ptr(), dev.data_ptr(), N, Lw, int(stereo),
                        thresholds.data_ptr(), mx.data_ptr(), img.data_ptr(), ws.data_ptr(), ws.numel(),
                        self._stream()))
        return img, mx


# Plans are cached, least recently used first out: a plan pins its tables on the device (the dense filterbank alone is
# 18 MB at the default parameters), and a server that builds its parameters from image EXIF (cli.py:77-87) would otherwise
# grow the cache with every distinct parameter set for ever.  An evicted plan is destroyed when its last user lets go of it.
# The bound is PER DEVICE (round 5): one process driving eight GPUs with two parameter sets holds sixteen plans, and a miss on
# one GPU never evicts another GPU's plan (a rebuild is a filterbank construction, hipMallocs and an 18 MB upload; an eviction's
# hipFree synchronises its device).
PLAN_CACHE_SIZE = max(1, int(os.environ.get("RFX_PLAN_CACHE", "8")))
_plans: "collections.OrderedDict[T.Tuple[T.Any, int, str, str, str, str], Plan]" = collections.OrderedDict()
_plans_lock = threading.Lock()


def _evict_over_bound(plans: "collections.OrderedDict", dev_index: int, bound: int) -> None:
    """Drop the least recently used plans OF ONE DEVICE until at most `bound` of them are cached (key[1] is the device index)."""
    mine = [k for k in plans if k[1] == dev_index]  # OrderedDict iterates least recently used first
    for k in mine[: max(0, len(mine) - bound)]:
        del plans[k]  # dropped from the cache; freed when the last converter holding it goes


def get_plan(params: T.Any, device: T.Union[str, torch.device], gl_form: str = "auto", frame_engine: str = "auto",
             plan_layout: str = "auto", imel_form: str = "auto") -> Plan:
    """Plans are immutable and cached per (frozen params, device, options), at most PLAN_CACHE_SIZE of them per device (least
    recently used evicted): constructing a converter per request, as the reference's server does (server.py:159), costs a
    dictionary lookup.

    `gl_form` picks the Griffin-Lim device form (rfx_plan_options.gl_form): "auto" (per call, from the batch
    shape), "runs" (always the run-based fused kernel) or "frames" (always the per-frame kernel + fold);
    `frame_engine` = "generic" keeps Griffin-Lim of the 40 h / 10 h geometries (48 kHz ...) on the generic FFT engine
    instead of the row-family kernels (rfx_plan_options.frame_engine; cross-checks), "chirp-z" plans as "auto" and runs
    the geometries "auto" refuses - an FFT length with a prime factor above 13 - on the chirp-z engine; `plan_layout` = "generic" builds the
    generic plan also for the default geometry (rfx_plan_options.plan_layout; cross-checks of the specialised engine);
    `imel_form` = "groups" keeps InverseMelScale on the group kernels where "auto" takes the wave kernel
    (rfx_plan_options.imel_form; cross-checks)."""
    dev = resolve_device(device)  # 'cuda' is keyed by the GPU it means now, not bound for good to the first one used
    key = (params, dev.index, gl_form, frame_engine, plan_layout, imel_form)
    with _plans_lock:
        plan = _plans.get(key)
        if plan is None:
            plan = Plan(params, dev, gl_form, frame_engine, plan_layout, imel_form)
            _plans[key] = plan
            _evict_over_bound(_plans, dev.index, PLAN_CACHE_SIZE)
        else:
            _plans.move_to_end(key)
    return plan


def cached_plans() -> int:
    with _plans_lock:
        return len(_plans)
