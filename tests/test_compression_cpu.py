"""
CPU checks of apply_filters(compression=True): PcmSegment.compress_dynamic_range and the compression=True chain against a
literal per-frame transcription of pydub 0.25.1 (effects.compress_dynamic_range, from its published source), the host tables
against pydub's expressions entry by entry, and the device arithmetic (csrc/rfx_compress_core.h, compiled for the host with
tests/emu/rfx_compress_emu.cpp) against the host, in both forms of the recurrence and through the flag-and-patch path.
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
U16P = ctypes.POINTER(ctypes.c_uint16)
U8P = ctypes.POINTER(ctypes.c_uint8)
F64P = ctypes.POINTER(ctypes.c_double)
I32P = ctypes.POINTER(ctypes.c_int)
needs_audioop = pytest.mark.skipif(_ao is None, reason="audioop removed from this interpreter")


# ---- pydub 0.25.1, transcribed from its published source (pydub/effects.py compress_dynamic_range, pydub/utils.py
# db_to_float / ratio_to_db, pydub/audio_segment.py frame_count / get_sample_slice / rms / get_frame), frame by frame on audioop
def pydub_compress_dynamic_range(x: np.ndarray, frame_rate: int, threshold=-20.0, ratio=4.0, attack=5.0, release=50.0) -> np.ndarray:
    data = np.ascontiguousarray(x).tobytes()
    channels = x.shape[1]
    frame_width = 2 * channels
    max_val = len(data) // frame_width

    def db_to_float(db):
        db = float(db)
        return 10 ** (db / 20)

    def ratio_to_db(r):
        r = float(r)
        if r == 0:
            return -float("inf")
        return 20 * math.log(r, 10)

    def frame_count(ms=None):
        if ms is not None:
            return ms * (frame_rate / 1000.0)
        return float(len(data) // frame_width)

    def get_sample_slice(start, end):
        def bounded(val):
            return 0 if val < 0 else (max_val if val > max_val else val)

        return data[bounded(start) * frame_width:bounded(end) * frame_width]

    thresh_rms = 32768.0 * db_to_float(threshold)  # seg.max_possible_amplitude
    look_frames = int(frame_count(ms=attack))

    def rms_at(frame_i):
        return _ao.rms(get_sample_slice(frame_i - look_frames, frame_i), 2)

    def db_over_threshold(rms):
        if rms == 0:
            return 0.0
        db = ratio_to_db(rms / thresh_rms)
        return max(db, 0)

    output = []
    attenuation = 0.0
    attack_frames = frame_count(ms=attack)
    release_frames = frame_count(ms=release)
    for i in range(int(frame_count())):
        rms_now = rms_at(i)
        max_attenuation = (1 - (1.0 / ratio)) * db_over_threshold(rms_now)
        attenuation_inc = max_attenuation / attack_frames
        attenuation_dec = max_attenuation / release_frames
        if rms_now > thresh_rms and attenuation <= max_attenuation:
            attenuation += attenuation_inc
            attenuation = min(attenuation, max_attenuation)
        else:
            attenuation -= attenuation_dec
            attenuation = max(attenuation, 0)
        frame = data[i * frame_width:(i + 1) * frame_width]  # get_frame(i)
        if attenuation != 0.0:
            frame = _ao.mul(frame, 2, db_to_float(-attenuation))
        output.append(frame)
    return np.frombuffer(b"".join(output), dtype=np.int16).reshape(-1, channels)


def pydub_apply_filters_compressed(x: np.ndarray, frame_rate: int) -> np.ndarray:
    """audio_util.apply_filters(compression=True) as the reference writes it, on audioop (PcmSegment supplies normalize,
    apply_gain and dBFS, pinned elsewhere; the compressor is the transcription above)."""
    seg = PcmSegment(x, frame_rate).normalize(headroom=0.1)
    seg = seg.apply_gain(-10 - seg.dBFS)
    seg = PcmSegment(pydub_compress_dynamic_range(seg._data, frame_rate, threshold=-20.0, ratio=4.0, attack=5.0, release=50.0),
                     frame_rate)
    seg = seg.apply_gain(-12 - seg.dBFS)
    return seg.normalize(headroom=0.1)._data


def signals(rate: int, frames: int, C: int, rng) -> dict:
    t = np.arange(frames)
    out = {}
    out["silence"] = np.zeros((frames, C), np.int16)
    out["near_silence"] = rng.integers(-2, 3, size=(frames, C)).astype(np.int16)
    sq = np.where((t // max(1, rate // 441)) % 2 == 0, 32767, -32768).astype(np.int16)
    out["square_full_scale"] = np.repeat(sq[:, None], C, axis=1)
    burst = np.where((t // (rate // 20)) % 4 == 0, 1.0, 0.0) * np.sin(t * 0.07) * 24000
    burst = burst + np.sin(t * 0.011) * 3  # the quiet holds keep a little signal: every clip normalises
    out["bursts_then_quiet"] = np.stack([burst * (1.0 - 0.3 * c) for c in range(C)], axis=1).astype(np.int16)
    ramp = np.sin(t * 0.05) * np.linspace(0, 12000, frames)
    out["threshold_ramp"] = np.stack([ramp] * C, axis=1).astype(np.int16)
    music = np.sin(t * 0.013) * 8000 * (1 + np.sin(t * 0.0007)) + rng.normal(0, 600, frames)
    out["music"] = np.stack([music, music[::-1]][:C], axis=1).astype(np.int16)
    return out


RATES = [44100, 48000, 22050]


# ---- the host against the transcription ---------------------------------------------------------------------------------------
@needs_audioop
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("C", [1, 2])
def test_apply_filters_compression_equals_pydub_transcription(rate, C):
    rng = np.random.default_rng(rate + C)
    for seconds in (0.1, 0.5):
        frames = int(rate * seconds)
        for name, x in signals(rate, frames, C, rng).items():
            got = audio_util.apply_filters(PcmSegment(x, rate), compression=True)
            assert isinstance(got, PcmSegment) and got.frame_rate == rate
            want = pydub_apply_filters_compressed(x, rate)
            assert got._data.tobytes() == want.tobytes(), (name, seconds)


@needs_audioop
@pytest.mark.parametrize("C", [1, 2])
def test_apply_filters_compression_short_clip(C):
    """A clip shorter than look_frames (220 at 44.1 kHz): every window starts at frame 0."""
    rng = np.random.default_rng(5)
    for frames in (1, 2, 57, 219, 220, 221):
        x = (rng.normal(0, 9000, (frames, C))).astype(np.int16)
        got = audio_util.apply_filters(PcmSegment(x, 44100), compression=True)._data
        assert got.tobytes() == pydub_apply_filters_compressed(x, 44100).tobytes(), frames


@needs_audioop
def test_apply_filters_compression_full_decode_length():
    """One clip as long as a decoded tile (5 s at 44.1 kHz, 220 500 frames), loud passages and holds."""
    rng = np.random.default_rng(11)
    frames = 220500
    t = np.arange(frames)
    x = (np.sin(t * 0.02) * 20000 * ((t // 30000) % 2) + rng.normal(0, 80, frames)).astype(np.int16)[:, None]
    got = audio_util.apply_filters(PcmSegment(x, 44100), compression=True)._data
    assert got.tobytes() == pydub_apply_filters_compressed(x, 44100).tobytes()


@needs_audioop
@pytest.mark.parametrize("kw", [dict(threshold=-30.0, ratio=2.0, attack=2.0, release=20.0),
                                dict(threshold=-6.0, ratio=10.0, attack=10.0, release=100.0),
                                dict(threshold=-20.0, ratio=1.5, attack=0.5, release=5.0)])
def test_compress_dynamic_range_arguments(kw):
    rng = np.random.default_rng(3)
    for rate, C in ((44100, 1), (48000, 2), (22050, 2)):
        for name, x in signals(rate, int(rate * 0.3), C, rng).items():
            got = PcmSegment(x, rate).compress_dynamic_range(**kw)._data
            assert got.tobytes() == pydub_compress_dynamic_range(x, rate, **kw).tobytes(), (name, rate, C, kw)


def test_compression_false_unchanged_by_target_parameter():
    assert audio_util.filter_gain_by_rms().tobytes() == audio_util.filter_gain_by_rms(-12).tobytes()


# ---- the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_compress_tables_equal_pydub_expressions(rate):
    look, above, max_att, inc, dec = audio_util.compress_tables(rate)
    thresh_rms = 32768.0 * 10 ** (float(-20.0) / 20)
    attack_frames, release_frames = 5.0 * (rate / 1000.0), 50.0 * (rate / 1000.0)
    assert look == int(attack_frames) == {44100: 220, 48000: 240, 22050: 110}[rate]
    assert (attack_frames, release_frames) == {44100: (220.5, 2205.0), 48000: (240.0, 2400.0), 22050: (110.25, 1102.5)}[rate]
    assert int(np.flatnonzero(above)[0]) == 3277 and above.sum() == 32769 - 3277
    for rms in range(audio_util.FILTER_TABLE_SIZE):
        dbo = 0.0 if rms == 0 else max(20 * math.log(rms / thresh_rms, 10), 0)
        m = (1 - (1.0 / 4.0)) * dbo
        assert bool(above[rms]) == (rms > thresh_rms)
        assert max_att[rms].tobytes() == np.float64(m).tobytes()
        assert inc[rms].tobytes() == np.float64(m / attack_frames).tobytes()
        assert dec[rms].tobytes() == np.float64(m / release_frames).tobytes()


def test_gain10_table_equals_pydub_expressions():
    g = audio_util.filter_gain_by_rms(-10)
    assert math.isinf(g[0])
    for rms in range(1, audio_util.FILTER_TABLE_SIZE):
        dbfs = 20.0 * math.log(rms / 32768.0, 10)
        assert g[rms].tobytes() == np.float64(10 ** (float(-10 - dbfs) / 20)).tobytes()


# ---- the emulated kernels against the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared("rfx_compress_emu.cpp", "-ffp-contract=off"))
    lib.emu_window_rms.argtypes = [I16P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, U16P]
    lib.emu_attenuation.argtypes = [U16P, ctypes.c_int64, U8P, F64P, F64P, F64P, ctypes.c_int, ctypes.c_int64, F64P]
    lib.emu_attenuation.restype = ctypes.c_int
    lib.emu_apply_filters_compressed.argtypes = [I16P, ctypes.c_int, ctypes.c_int64, ctypes.c_int, F64P, F64P, F64P, U8P, F64P, F64P,
                                                 F64P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_double, I16P, F64P, I32P]
    lib.emu_apply_filters_compressed.restype = ctypes.c_int64
    return lib


def emu_filters(emu, batch: np.ndarray, rate: int, form: int, chunk: int = 0, margin: float = 2.0 ** -30):
    batch = np.ascontiguousarray(batch, dtype=np.int16)
    N, L, C = batch.shape
    look, above, max_att, inc, dec = audio_util.compress_tables(rate)
    out = np.empty_like(batch)
    att = np.empty((N, L), np.float64)
    rounds = np.empty(N, np.int32)
    tabs = [audio_util.filter_gain_by_rms(-10), audio_util.filter_gain_by_rms(), audio_util.filter_boost_by_peak()]
    flagged = emu.emu_apply_filters_compressed(batch.ctypes.data_as(I16P), N, L, C, *(t.ctypes.data_as(F64P) for t in tabs),
                                               above.ctypes.data_as(U8P), max_att.ctypes.data_as(F64P), inc.ctypes.data_as(F64P),
                                               dec.ctypes.data_as(F64P), look, form, chunk, margin, out.ctypes.data_as(I16P),
                                               att.ctypes.data_as(F64P), rounds.ctypes.data_as(I32P))
    return out, att, rounds, flagged


def host_attenuation(x: np.ndarray, rate: int) -> np.ndarray:
    """The compressor's input (normalize, gain to -10 dBFS) and the host's attenuation after every frame."""
    seg = PcmSegment(x, rate).normalize(headroom=0.1)
    seg = seg.apply_gain(-10 - seg.dBFS)
    look, above, max_att, inc, dec = audio_util.compress_tables(rate)
    return audio_util.compress_attenuation(audio_util.compress_window_rms(seg._data, look), above, max_att, inc, dec)


def host_filters(batch: np.ndarray, rate: int) -> np.ndarray:
    return np.stack([audio_util.apply_filters(PcmSegment(c, rate), compression=True)._data for c in batch])


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("C", [1, 2])
def test_emulator_equals_host(emu, rate, C):
    rng = np.random.default_rng(17 + C)
    frames = int(rate * 0.4)
    clips = signals(rate, frames, C, rng)
    batch = np.stack(list(clips.values()))
    want = host_filters(batch, rate)
    want_att = np.stack([host_attenuation(c, rate) for c in batch])
    for form, chunk in ((0, 0), (1, 0), (1, 1), (1, 7), (1, 220), (1, 256), (1, frames + 5)):
        got, att, rounds, _ = emu_filters(emu, batch, rate, form, chunk)
        assert got.tobytes() == want.tobytes(), (form, chunk)
        assert att.tobytes() == want_att.tobytes(), (form, chunk)
        if form == 0:
            assert not rounds.any()


def test_emulator_window_rms_equals_audioop(emu):
    rng = np.random.default_rng(2)
    for C in (1, 2):
        x = rng.integers(-32768, 32768, size=(1000, C)).astype(np.int16)
        for look in (0, 1, 220, 999, 1000, 1500):
            got = np.empty(1000, np.uint16)
            emu.emu_window_rms(x.ctypes.data_as(I16P), 1000, C, look, got.ctypes.data_as(U16P))
            assert got.astype(np.uint32).tolist() == audio_util.compress_window_rms(x, look).tolist()
            if _ao is not None:
                raw = x.tobytes()
                want = [_ao.rms(raw[max(0, i - look) * 2 * C:i * 2 * C], 2) for i in range(1000)]
                assert got.tolist() == want


def test_emulator_chunk_boundaries(emu):
    """Loud / quiet transitions placed exactly on chunk boundaries, and chunk lengths down to one frame: the repair rounds and
    the quiet chunks' pass-through give the sequential states bit for bit."""
    rate, L = 44100, 4096
    t = np.arange(L)
    for chunk in (1, 7, 64, 220, 256):
        x = np.full(L, 1, np.float64)
        for k in range(0, L // chunk, 3):  # loud chunks 0, 3, 6, ... start and end on the boundaries
            x[k * chunk:(k + 1) * chunk] = 25000 * np.sin(t[k * chunk:(k + 1) * chunk] * 0.3)
        batch = x.astype(np.int16)[None, :, None]
        want_att = host_attenuation(batch[0], rate)
        seq, seq_att, _, _ = emu_filters(emu, batch, rate, 0)
        got, att, rounds, _ = emu_filters(emu, batch, rate, 1, chunk)
        assert att.tobytes() == want_att.tobytes() == seq_att.tobytes(), chunk
        assert got.tobytes() == seq.tobytes() == host_filters(batch, rate).tobytes(), chunk
        assert (want_att != 0).any() and rounds[0] >= 1


def test_emulator_forced_patch_path(emu):
    """With the margin at its maximum every sample of non-zero attenuation is flagged and recomputed with the host's pow: the
    bytes are still the host's."""
    rate = 48000
    rng = np.random.default_rng(9)
    batch = np.stack(list(signals(rate, int(rate * 0.25), 2, rng).values()))
    want = host_filters(batch, rate)
    for form in (0, 1):
        got, att, _, flagged = emu_filters(emu, batch, rate, form, margin=1.0)
        assert got.tobytes() == want.tobytes()
        x2_nonzero = flagged > 0
        assert x2_nonzero and flagged <= int((att != 0).sum()) * 2
        got0, _, _, flagged0 = emu_filters(emu, batch, rate, form)
        assert got0.tobytes() == want.tobytes() and flagged0 < flagged
