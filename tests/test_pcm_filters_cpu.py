"""
CPU checks of the device post-processing (csrc/rfx_pcm.hip): the arithmetic header csrc/rfx_pcm_core.h is compiled for the host
together with tests/emu/rfx_pcm_emu.cpp and pinned, bit for bit, against CPython's audioop (what pydub and PcmSegment call) and
against PcmSegment's apply_filters and stitch_segments; the host halves (the two filter tables, the stitch planner) are checked
here as well.
"""
import ctypes
import math

import numpy as np
import pytest

import emu_build
from riffusion.util import audio_util
from riffusion.util.audio_util import PcmSegment

try:
    import audioop as _ao  # type: ignore
except ImportError:  # pragma: no cover
    _ao = None

I16P = ctypes.POINTER(ctypes.c_int16)
F64P = ctypes.POINTER(ctypes.c_double)
needs_audioop = pytest.mark.skipif(_ao is None, reason="audioop removed from this interpreter")


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared("rfx_pcm_emu.cpp", "-ffp-contract=off"))
    lib.emu_mul.argtypes, lib.emu_mul.restype = [ctypes.c_int, ctypes.c_double], ctypes.c_int
    lib.emu_add.argtypes, lib.emu_add.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_int
    lib.emu_rms.argtypes, lib.emu_rms.restype = [I16P, ctypes.c_int64], ctypes.c_uint
    lib.emu_max.argtypes, lib.emu_max.restype = [I16P, ctypes.c_int64], ctypes.c_uint
    lib.emu_apply_filters.argtypes = [I16P, ctypes.c_int, ctypes.c_int64, ctypes.c_int, F64P, F64P, I16P, F64P]
    lib.emu_stitch.argtypes = [I16P, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, I16P]
    return lib


def emu_filters(emu, batch: np.ndarray) -> np.ndarray:
    """(N, L, C) int16 -> the emulated device filters."""
    batch = np.ascontiguousarray(batch, dtype=np.int16)
    N, L, C = batch.shape
    out = np.empty_like(batch)
    gain, boost = audio_util.filter_gain_by_rms(), audio_util.filter_boost_by_peak()
    emu.emu_apply_filters(batch.ctypes.data_as(I16P), N, L, C, gain.ctypes.data_as(F64P), boost.ctypes.data_as(F64P),
                          out.ctypes.data_as(I16P), None)
    return out


def emu_stitch(emu, batch: np.ndarray, rate: int, crossfade_s: float) -> np.ndarray:
    batch = np.ascontiguousarray(batch, dtype=np.int16)
    N, L, C = batch.shape
    pieces, frames = audio_util.stitch_plan(N, L, rate, crossfade_s)
    out = np.empty((frames, C), dtype=np.int16)
    emu.emu_stitch(batch.ctypes.data_as(I16P), L, C, pieces.ctypes.data, len(pieces), frames, out.ctypes.data_as(I16P))
    return out


def adversarial_clips(rng, L: int, C: int):
    """Named (L, C) int16 clips: the edge cases of the filters and a few random ones."""
    z = np.zeros((L, C), np.int16)
    one_pos, one_neg = z.copy(), z.copy()
    one_pos[L // 2, 0], one_neg[L // 3, C - 1] = 1, -1
    full_neg = np.full((L, C), -32768, np.int16)
    full_pos = np.full((L, C), 32767, np.int16)
    alt = full_pos.copy()
    alt.reshape(-1)[::2] = -32768
    quiet = rng.integers(-3, 4, size=(L, C)).astype(np.int16)
    loud = rng.integers(-32768, 32768, size=(L, C)).astype(np.int16)
    music = (np.sin(np.arange(L * C) * 0.01).reshape(L, C) * 9000 + rng.normal(0, 300, (L, C))).astype(np.int16)
    spike = (rng.normal(0, 20, (L, C))).astype(np.int16)
    spike[L // 4, 0] = -32768
    return {"zeros": z, "one_pos": one_pos, "one_neg": one_neg, "full_neg": full_neg, "full_pos": full_pos, "alternating": alt,
            "quiet": quiet, "loud": loud, "music": music, "spike": spike}


# ---- audioop primitives ----------------------------------------------------------------------------------------------------
@needs_audioop
def test_mul_is_audioop_mul(emu):
    # NaN (0 * inf) is 0, the CPython x86-64 behaviour the device reproduces
    assert _ao.mul(np.array([1, 0, -1, 0, 5, -5], np.int16).tobytes(), 2, math.inf) == \
        np.array([32767, 0, -32768, 0, 32767, -32768], np.int16).tobytes()
    rng = np.random.default_rng(3)
    xs = np.concatenate([np.array([0, 1, -1, 2, -2, 32767, -32768, 32766, -32767], np.int16),
                         rng.integers(-32768, 32768, 400).astype(np.int16)])
    factors = [0.0, 1.0, math.inf, 1e-6, 0.5, 0.999999, 1.0000001, 2.0, 3.7, 8192.0, 1e300, 0.1 ** 5] + list(rng.uniform(0, 4, 20))
    factors += [audio_util.filter_gain_by_rms()[r] for r in (1, 2, 3, 100, 2000, 32768)]
    factors += [audio_util.filter_boost_by_peak()[p] for p in (1, 7, 1000, 30000, 32767, 32768)]
    for f in factors:
        want = np.frombuffer(_ao.mul(xs.tobytes(), 2, float(f)), np.int16)
        got = np.array([emu.emu_mul(int(x), float(f)) for x in xs], np.int16)
        assert np.array_equal(got, want), f


@needs_audioop
def test_add_rms_max_are_audioop(emu):
    rng = np.random.default_rng(4)
    a = np.concatenate([np.array([32767, -32768, 32767, -32768, 1], np.int16), rng.integers(-32768, 32768, 300).astype(np.int16)])
    b = np.concatenate([np.array([32767, -32768, -32768, 1, -1], np.int16), rng.integers(-32768, 32768, 300).astype(np.int16)])
    want = np.frombuffer(_ao.add(a.tobytes(), b.tobytes(), 2), np.int16)
    assert np.array_equal(np.array([emu.emu_add(int(x), int(y)) for x, y in zip(a, b)], np.int16), want)
    for name, clip in adversarial_clips(rng, 1003, 2).items():
        flat = np.ascontiguousarray(clip.reshape(-1))
        assert emu.emu_rms(flat.ctypes.data_as(I16P), flat.size) == _ao.rms(flat.tobytes(), 2), name
        assert emu.emu_max(flat.ctypes.data_as(I16P), flat.size) == _ao.max(flat.tobytes(), 2), name
    for n in (1, 2, 3, 17, 4096):  # the exact-square cases sqrt must not round across
        for v in (1, 181, 32767, -32768):
            flat = np.full(n, v, np.int16)
            assert emu.emu_rms(flat.ctypes.data_as(I16P), n) == _ao.rms(flat.tobytes(), 2)


# ---- the two tables --------------------------------------------------------------------------------------------------------
def test_tables_are_pcmsegment_expressions():
    gain, boost = audio_util.filter_gain_by_rms(), audio_util.filter_boost_by_peak()
    assert gain.shape == boost.shape == (32769,) and gain.dtype == boost.dtype == np.float64
    assert gain[0] == math.inf and boost[0] == 1.0
    for v in list(range(0, 300)) + list(range(300, 32769, 97)) + [32767, 32768]:
        seg = PcmSegment(np.array([-v if v == 32768 else v], np.int16), 44100)  # rms = max = |v|
        assert seg.rms == v and seg.max == v
        assert gain[v] == 10 ** (float(-12 - seg.dBFS) / 20), v
        if v:
            target_peak = seg.max_possible_amplitude * (10 ** (-float(0.1) / 20))
            assert boost[v] == 10 ** (float(20 * math.log(target_peak / seg.max, 10)) / 20), v


# ---- apply_filters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("L", [1, 441, 4410 + 17, 44100 * 2 + 3])  # 10 ms, not a whole millisecond, 2 s and a bit
def test_apply_filters_equals_pcmsegment(emu, L, C):
    rng = np.random.default_rng(L * 10 + C)
    clips = adversarial_clips(rng, L, C)
    names = list(clips)
    got = emu_filters(emu, np.stack([clips[k] for k in names]))
    for i, name in enumerate(names):
        want = audio_util.apply_filters(PcmSegment(clips[name], 44100), compression=False).get_array_of_samples()
        assert np.array_equal(got[i].reshape(-1), want), (name, L, C)


def test_apply_filters_edge_values(emu):
    gain = audio_util.filter_gain_by_rms()
    z = np.zeros((1, 1000, 1), np.int16)
    assert np.array_equal(emu_filters(emu, z), z)  # silence stays silence
    one = z.copy()
    one[0, 10, 0] = 1  # rms 0 -> f1 = inf: the sample saturates, the zeros stay 0 (0 * inf -> 0)
    out = emu_filters(emu, one)
    assert out[0, 10, 0] > 30000 and np.count_nonzero(out) == 1
    assert gain[0] == math.inf


# ---- stitch ----------------------------------------------------------------------------------------------------------------
def random_batch(rng, N, L, C):
    return rng.integers(-32768, 32768, size=(N, L, C)).astype(np.int16)


def host_stitch(batch, rate, crossfade_s):
    segs = [PcmSegment(c, rate) for c in batch]
    return audio_util.stitch_segments(segs, crossfade_s).get_array_of_samples()


@pytest.mark.parametrize("crossfade_s", [0.0, 0.05, 0.1, 0.101, 0.2])
@pytest.mark.parametrize("rate", [44100, 48000, 8000])
@pytest.mark.parametrize("frames_kind", ["whole", "odd"])
def test_stitch_equals_stitch_segments(emu, crossfade_s, rate, frames_kind):
    rng = np.random.default_rng(rate + int(crossfade_s * 1000))
    L = 441 * 511 if frames_kind == "whole" else 441 * 511 + 17
    L = L * rate // 44100 if rate != 44100 else L
    for N, C in ((1, 1), (2, 2), (5, 1)):
        batch = random_batch(rng, N, L, C)
        got = emu_stitch(emu, batch, rate, crossfade_s)
        want = host_stitch(batch, rate, crossfade_s)
        assert got.size == want.size and np.array_equal(got.reshape(-1), want), (N, C, L, rate, crossfade_s)


@pytest.mark.parametrize("crossfade_s", [0.0, 0.05, 0.2])
def test_stitch_37_clips(emu, crossfade_s):
    rng = np.random.default_rng(37)
    batch = random_batch(rng, 37, 441 * 511, 1)
    assert np.array_equal(emu_stitch(emu, batch, 44100, crossfade_s).reshape(-1), host_stitch(batch, 44100, crossfade_s))


@pytest.mark.parametrize("rate", [44100, 48000, 8000])
@pytest.mark.parametrize("C", [1, 2])
def test_stitch_short_clips(emu, rate, C):
    """10.6 ms clips (not a whole millisecond: the last frames are dropped, a crossfade-0 stitch keeps them) and 300 ms clips
    with crossfades of a third and of a half of a clip."""
    rng = np.random.default_rng(rate + C)
    short = int(round(10.6e-3 * rate))
    for N in (1, 2, 37):
        batch = random_batch(rng, N, short, C)
        assert np.array_equal(emu_stitch(emu, batch, rate, 0.0).reshape(-1), host_stitch(batch, rate, 0.0))
        assert np.array_equal(emu_stitch(emu, batch, rate, 0.005).reshape(-1), host_stitch(batch, rate, 0.005))
    mid = int(0.3 * rate) + 5
    for xf in (0.1, 0.15, 0.01):
        batch = random_batch(rng, 4, mid, C)
        assert np.array_equal(emu_stitch(emu, batch, rate, xf).reshape(-1), host_stitch(batch, rate, xf)), xf


@pytest.mark.parametrize("crossfade_s", [0.05, 0.1, 0.101, 0.2])
def test_stitch_too_long_crossfade_raises_like_append(crossfade_s):
    rate = 44100
    short = int(round(10.6e-3 * rate))
    segs = [PcmSegment(np.zeros((short, 1), np.int16), rate)] * 3
    with pytest.raises(ValueError) as host:
        audio_util.stitch_segments(segs, crossfade_s)
    with pytest.raises(ValueError) as planned:
        audio_util.stitch_plan(3, short, rate, crossfade_s)
    assert str(planned.value) == str(host.value)


def test_stitch_plan_reaching_a_previous_crossfade_is_refused():
    with pytest.raises(audio_util.StitchNotPlannable):
        audio_util.stitch_plan(3, 4410, 44100, 0.08)  # 100 ms clips, 80 ms crossfades


def test_stitch_pieces_stay_inside_the_batch():
    """What rfx_pcm16_stitch checks before it launches: every piece non-empty, every source frame inside its clip."""
    for N, L, rate, xf in ((37, 441 * 511, 44100, 0.2), (5, 441 * 511 + 17, 48000, 0.05), (4, 2405, 8000, 0.15)):
        pieces, frames = audio_util.stitch_plan(N, L, rate, xf)
        assert pieces.dtype.itemsize == 56 and pieces["out_start"][0] == 0
        count = np.diff(np.append(pieces["out_start"], frames))
        assert (count > 0).all()
        for src in ("a", "b"):
            clip, off = pieces[src + "_clip"], pieces[src + "_off"]
            used = (clip >= 0) & ((pieces["kind"] == 1) | (src == "a"))
            assert (clip[used] < N).all() and (off[used] >= 0).all() and (off[used] + count[used] <= L).all()


def test_emu_piece_layout_matches_dtype(emu):
    assert emu.emu_piece_bytes() == audio_util.STITCH_PIECE_DTYPE.itemsize
