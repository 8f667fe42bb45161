"""
CPU checks of the int16 front end of the encode (csrc/rfx_pcm_in.hip): the arithmetic header csrc/rfx_pcm_in_core.h is compiled
for the host together with tests/emu/rfx_pcm_in_emu.cpp and pinned, byte for byte, against CPython's audioop.ratecv / tomono /
tostereo (what pydub's and PcmSegment's set_frame_rate / set_channels call); audio_util.ratecv_np - the restatement
PcmSegment.set_frame_rate falls back to where audioop is gone - is pinned against both; the gather emulator against
slice_audio_into_clips + set_channels + the float32 conversion of spectrogram_image_from_audio; clip_frame_ranges against the
slicing it plans; and the C ABI's argument checks, which need no GPU.
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import emu_build
from riffusion.util import audio_util
from riffusion.util.audio_util import PcmSegment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
I16P = ctypes.POINTER(ctypes.c_int16)

# (in_rate, out_rate): the common pairs both ways, near-equal and odd rates, and coprime pairs near 2^20
RATE_PAIRS = [(48000, 44100), (44100, 48000), (44100, 22050), (22050, 44100), (44100, 8000), (8000, 44100), (44100, 96000),
              (96000, 44100), (44100, 16000), (16000, 44100), (44100, 32000), (32000, 44100), (44100, 11025), (11025, 44100),
              (44100, 44101), (44101, 44100), (12345, 44100), (44100, 12345), (999983, 1000003), (1000003, 999983), (1048573, 7),
              (7, 1048573), (44100, 44100)]
LENGTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 1000, 4410, 50001]  # (7 -> 1048573 stops at 63)


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared("rfx_pcm_in_emu.cpp", "-ffp-contract=off"))
    lib.emu_ratecv_frames.argtypes, lib.emu_ratecv_frames.restype = [ctypes.c_int64] * 3, ctypes.c_int64
    lib.emu_ratecv.argtypes = [I16P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, I16P, ctypes.c_int64]
    lib.emu_clips.argtypes = [I16P, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    lib.emu_tomono.argtypes, lib.emu_tomono.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


def emu_ratecv(emu, x: np.ndarray, in_rate: int, out_rate: int, out_channels=None, head: int = 0) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.int16)
    L, C = x.shape
    C_out = C if out_channels is None else out_channels
    K = emu.emu_ratecv_frames(L, in_rate, out_rate)
    out = np.full((K, C_out), 12345, np.int16)
    emu.emu_ratecv(x.ctypes.data_as(I16P), L, C, in_rate, C_out, out_rate, out.ctypes.data_as(I16P), head)
    return out


def emu_clips(emu, x: np.ndarray, starts, Lw: int, out_channels: int) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.int16)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    out = np.full((len(starts) * out_channels, Lw), np.nan, np.float32)
    emu.emu_clips(x.ctypes.data_as(I16P), x.shape[1], starts.ctypes.data, len(starts), Lw, out_channels, out.ctypes.data)
    return out


def audioop_ratecv(x: np.ndarray, in_rate: int, out_rate: int) -> np.ndarray:
    ao = pytest.importorskip("audioop")
    raw, _ = ao.ratecv(np.ascontiguousarray(x).tobytes(), 2, x.shape[1], in_rate, out_rate, None)
    return np.frombuffer(raw, np.int16).reshape(-1, x.shape[1])


def audioop_mix(x: np.ndarray, out_channels: int) -> np.ndarray:
    ao = pytest.importorskip("audioop")
    if out_channels == x.shape[1]:
        return x
    raw = ao.tomono(x.tobytes(), 2, 0.5, 0.5) if out_channels == 1 else ao.tostereo(x.tobytes(), 2, 1, 1)
    return np.frombuffer(raw, np.int16).reshape(-1, out_channels)


def track(rng, L: int, C: int) -> np.ndarray:
    """random frames with runs of both extremes (the interpolation's largest numerators, tomono's clip)"""
    x = rng.integers(-32768, 32768, size=(L, C)).astype(np.int16)
    if L >= 8:
        x[L // 4 : L // 4 + max(1, L // 8)] = -32768
        x[L // 2 : L // 2 + max(1, L // 8)] = 32767
        x[-1] = -32768
    return x


def golden_wavs():
    from scipy.io import wavfile

    wavs = sorted(glob.glob(os.path.join(GOLDEN, "clip_*.wav")))
    assert len(wavs) == 3
    return [wavfile.read(w)[1] for w in wavs]


# ---- ratecv: emulator and numpy restatement against audioop ----------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("in_rate,out_rate", RATE_PAIRS)
def test_ratecv_emulator_and_numpy_equal_audioop(emu, in_rate, out_rate, C):
    rng = np.random.default_rng(in_rate % 1000 + out_rate % 777 + C)
    for L in LENGTHS:
        if (in_rate, out_rate) == (7, 1048573) and L > 63:
            continue  # 150 000 output frames per input frame: 63 frames give 9.3 million, 50001 would give 7.5e9
        x = track(rng, L, C)
        want = audioop_ratecv(x, in_rate, out_rate)
        assert audio_util.ratecv_frames(L, in_rate, out_rate) == len(want) == emu.emu_ratecv_frames(L, in_rate, out_rate)
        assert np.array_equal(audio_util.ratecv_np(x, in_rate, out_rate), want), (L, "numpy")
        for head in (0, 3):  # the launcher's frames before the first 16-byte boundary
            assert np.array_equal(emu_ratecv(emu, x, in_rate, out_rate, head=head), want), (L, head)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("in_rate,out_rate", RATE_PAIRS)
def test_ratecv_numpy_equals_emulator(emu, in_rate, out_rate, C):
    """runs whatever the interpreter ships: the restatement set_frame_rate falls back to against the kernels' arithmetic"""
    rng = np.random.default_rng(in_rate % 991 + out_rate % 769 + C)
    for L in LENGTHS:
        if (in_rate, out_rate) == (7, 1048573) and L > 63:
            continue
        x = track(rng, L, C)
        assert np.array_equal(audio_util.ratecv_np(x, in_rate, out_rate), emu_ratecv(emu, x, in_rate, out_rate)), L


@pytest.mark.parametrize("out_channels", [1, 2])
@pytest.mark.parametrize("in_rate,out_rate", [(48000, 44100), (44100, 48000), (44100, 22050), (8000, 44100), (44100, 44101),
                                              (12345, 44100), (999983, 1000003), (44100, 44100)])
def test_mix_then_ratecv_equals_audioop(emu, in_rate, out_rate, out_channels):
    rng = np.random.default_rng(in_rate % 1000 + out_rate % 777 + 10 * out_channels)
    for L in (1, 2, 9, 1000, 50001):
        x = track(rng, L, 3 - out_channels)
        want = audioop_ratecv(audioop_mix(x, out_channels), in_rate, out_rate)
        assert np.array_equal(emu_ratecv(emu, x, in_rate, out_rate, out_channels), want), L
        seg = PcmSegment(x, in_rate).set_channels(out_channels).set_frame_rate(out_rate)
        assert np.array_equal(seg._data, want)


def test_tomono_is_audioop_tomono(emu):
    ao = pytest.importorskip("audioop")
    vals = [-32768, -32767, -3, -2, -1, 0, 1, 2, 3, 32766, 32767]
    pairs = np.array([(l, r) for l in vals for r in vals], np.int16)
    want = np.frombuffer(ao.tomono(pairs.tobytes(), 2, 0.5, 0.5), np.int16)
    got = np.array([emu.emu_tomono(int(l), int(r)) for l, r in pairs], np.int16)
    assert np.array_equal(got, want) and np.array_equal(PcmSegment._tomono_np(pairs), want)


@pytest.mark.parametrize("rate", [48000, 22050, 16000])
def test_golden_wavs_there_and_back(emu, rate):
    for x in golden_wavs():
        for src in (x, np.ascontiguousarray(x[:, :1])):
            there = audioop_ratecv(src, 44100, rate)
            assert np.array_equal(emu_ratecv(emu, src, 44100, rate), there)
            assert np.array_equal(audio_util.ratecv_np(src, 44100, rate), there)
            back = audioop_ratecv(there, rate, 44100)
            assert np.array_equal(emu_ratecv(emu, there, rate, 44100), back)
            assert np.array_equal(audio_util.ratecv_np(there, rate, 44100), back)
        mono = audioop_ratecv(audioop_mix(x, 1), 44100, rate)
        assert np.array_equal(emu_ratecv(emu, x, 44100, rate, 1), mono)


def test_set_frame_rate_without_audioop(monkeypatch):
    x = track(np.random.default_rng(5), 30001, 2)
    seg = PcmSegment(x, 48000)
    with_module = seg.set_frame_rate(44100)._data if audio_util._audioop is not None else None
    monkeypatch.setattr(audio_util, "_audioop", None)
    got = seg.set_frame_rate(44100)
    assert got.frame_rate == 44100 and got.channels == 2 and got._data.dtype == np.int16
    assert np.array_equal(got._data, audio_util.ratecv_np(x, 48000, 44100))
    if with_module is not None:
        assert np.array_equal(got._data, with_module)
    assert seg.set_frame_rate(48000) is seg
    mono = seg.set_channels(1).set_frame_rate(16000)
    assert mono.channels == 1 and mono._data.shape[0] == audio_util.ratecv_frames(30001, 48000, 16000)


def test_ratecv_np_refuses_what_it_cannot_hold_exact():
    x = np.zeros((10, 1), np.int16)
    with pytest.raises(ValueError, match="2\\^20"):
        audio_util.ratecv_np(x, 1048577, 7)
    with pytest.raises(ValueError):
        audio_util.ratecv_np(x, 0, 7)
    with pytest.raises(TypeError):
        audio_util.ratecv_np(x.astype(np.float32), 48000, 44100)
    assert audio_util.ratecv_np(x[:0], 48000, 44100).shape == (0, 1)


# ---- the host-only entry ------------------------------------------------------------------------------------------------------
def test_resample_frames_entry_equals_audioop(lib):
    from riffusion import _hip

    ao = pytest.importorskip("audioop")
    for in_rate, out_rate in RATE_PAIRS:
        for L in LENGTHS:
            if (in_rate, out_rate) == (7, 1048573) and L > 63:
                continue
            for C in (1, 2):
                raw, _ = ao.ratecv(bytes(2 * C * L), 2, C, in_rate, out_rate, None)
                assert _hip.resample_frames(L, in_rate, out_rate) == len(raw) // (2 * C), (in_rate, out_rate, L)
    # one hour at 96 kHz, and far beyond: 64-bit throughout
    assert _hip.resample_frames(345_600_000, 96000, 44100) == (345_600_000 - 1) * 147 // 320 + 1
    assert _hip.resample_frames(1 << 40, 44100, 48000) == ((1 << 40) - 1) * 160 // 147 + 1


def test_resample_frames_entry_refuses(lib):
    out = ctypes.c_int64(-7)
    for in_rate, out_rate in [(1048577, 7), (7, 1048577), (1 << 20, 1), (2097143, 2097169)]:
        assert lib.rfx_pcm16_resample_frames(100, in_rate, out_rate, ctypes.byref(out)) == -4
        assert b"2^20" in lib.rfx_last_error()
    assert lib.rfx_pcm16_resample_frames(100, 2 * 1048573, 14, ctypes.byref(out)) == 0 and out.value == 1  # reduces to 1048573 -> 7
    for args in [(0, 48000, 44100), (-1, 48000, 44100), (10, 0, 44100), (10, 48000, -1)]:
        assert lib.rfx_pcm16_resample_frames(*args, ctypes.byref(out)) == -1
    assert lib.rfx_pcm16_resample_frames(10, 48000, 44100, None) == -1


# ---- argument checks of the device entries: refused before any device work (NULL device pointers, no GPU) ------------------------
def test_entries_validate_before_any_device_work(lib):
    starts = (ctypes.c_int64 * 3)(0, 100, 780)
    S = ctypes.cast(starts, ctypes.c_void_p)
    K = audio_util.ratecv_frames(1000, 48000, 44100)
    cases = [
        (lambda: lib.rfx_pcm16_resample(None, 0, 2, 48000, 2, 44100, None, K, None), -1, b"in_frames"),
        (lambda: lib.rfx_pcm16_resample(None, -5, 2, 48000, 2, 44100, None, K, None), -1, b"in_frames"),
        (lambda: lib.rfx_pcm16_resample(None, 1000, 3, 48000, 2, 44100, None, K, None), -1, b"channel"),
        (lambda: lib.rfx_pcm16_resample(None, 1000, 2, 48000, 0, 44100, None, K, None), -1, b"channel"),
        (lambda: lib.rfx_pcm16_resample(None, 1000, 2, 0, 2, 44100, None, K, None), -1, b"rates"),
        (lambda: lib.rfx_pcm16_resample(None, 1000, 2, 1048577, 2, 7, None, 1, None), -4, b"2^20"),
        (lambda: lib.rfx_pcm16_resample(None, 1000, 2, 48000, 2, 44100, None, K + 1, None), -1, b"out_frames"),
        (lambda: lib.rfx_pcm16_resample(None, 1000, 2, 48000, 2, 44100, None, K, None), -1, b"null"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, S, None, -1, 220, 1, None, None), -1, b"negative"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 0, 2, S, None, 3, 220, 1, None, None), -1, b"positive"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, S, None, 3, 0, 1, None, None), -1, b"positive"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 4, S, None, 3, 220, 1, None, None), -1, b"channel"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, S, None, 3, 220, 3, None, None), -1, b"channel"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, None, None, 3, 220, 1, None, None), -1, b"h_starts"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, S, None, 3, 221, 1, None, None), -1, b"clip 2"),
        (lambda: lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, S, None, 3, 220, 1, None, None), -1, b"null"),
        (lambda: lib.rfx_image_from_pcm16_clips(None, None, 1000, 2, S, None, -1, 220, 0, None, None, None, None, 0, None), -1, b"negative"),
        (lambda: lib.rfx_image_from_pcm16_clips(None, None, 1000, 5, S, None, 3, 220, 0, None, None, None, None, 0, None), -1, b"channel"),
        (lambda: lib.rfx_image_from_pcm16_clips(None, None, 1000, 2, S, None, 3, 221, 1, None, None, None, None, 0, None), -1, b"clip 2"),
        (lambda: lib.rfx_image_from_pcm16_clips(None, None, 1000, 2, S, None, 3, 220, 1, None, None, None, None, 0, None), -1, b"null"),
    ]
    for call, code, word in cases:
        assert call() == code and word in lib.rfx_last_error(), (code, word, lib.rfx_last_error())
    # more output frames than one launch holds: refused, not truncated
    big = 1 << 42
    assert lib.rfx_pcm16_resample(None, big, 1, 44100, 1, 48000, None, audio_util.ratecv_frames(big, 44100, 48000), None) == -4
    assert b"one launch" in lib.rfx_last_error()
    neg = (ctypes.c_int64 * 1)(-1)
    assert lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, ctypes.cast(neg, ctypes.c_void_p), None, 1, 10, 1, None, None) == -1
    # no clips: nothing to do, nothing to check
    assert lib.rfx_pcm16_clips_to_waveform(None, 1000, 2, None, None, 0, 220, 1, None, None) == 0
    assert lib.rfx_image_from_pcm16_clips(None, None, 1000, 2, None, None, 0, 220, 0, None, None, None, None, 0, None) == 0
    assert lib.rfx_image_from_pcm16_clips_workspace_bytes(None, 4, 0, 220500) == 0


# ---- the clip gather -------------------------------------------------------------------------------------------------------------
def host_clip_waveforms(seg: PcmSegment, starts_s, duration_s: float, channels: int):
    """slice_audio_into_clips, then spectrogram_image_from_audio's set_channels and float32 conversion, per clip"""
    out = []
    for clip in audio_util.slice_audio_into_clips(seg, starts_s, duration_s):
        clip = clip.set_channels(channels)
        out.append(np.array([c.get_array_of_samples() for c in clip.split_to_mono()]).astype(np.float32))
    return out


def golden_track() -> PcmSegment:
    return PcmSegment(np.concatenate(golden_wavs()), 44100)


@pytest.mark.parametrize("in_channels,out_channels", [(2, 2), (2, 1), (1, 1), (1, 2)])
def test_gather_equals_host_slicing_golden_track(emu, in_channels, out_channels):
    seg = golden_track()
    if in_channels == 1:
        seg = seg.set_channels(1)
    starts_s = audio_util.clip_start_times(seg.duration_seconds, 5.0, 0.2)
    r = audio_util.clip_frame_ranges(int(seg.frame_count()), 44100, starts_s, 5.0)
    assert list(r.index) == [0, 1, 2] and r.frames == 220500 and not r.last_short and len(r.host_index) == 0
    assert list(r.starts) == [0, 211680, 423360]
    want = host_clip_waveforms(seg, starts_s, 5.0, out_channels)
    got = emu_clips(emu, seg._data, r.starts, r.frames, out_channels).reshape(3, out_channels, r.frames)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 8000])
@pytest.mark.parametrize("in_channels,out_channels", [(2, 2), (2, 1), (1, 1), (1, 2)])
def test_gather_equals_host_slicing_random_tracks(emu, rate, in_channels, out_channels):
    rng = np.random.default_rng(rate + in_channels * 3 + out_channels)
    seg = PcmSegment(track(rng, int(2.37 * rate) + 11, in_channels), rate)
    starts_s = np.arange(0, 2.0, 0.137)  # overlapping clips of 0.3 s, the last ones reach past the end
    r = audio_util.clip_frame_ranges(int(seg.frame_count()), rate, starts_s, 0.3)
    assert len(r.index) >= 10 and len(r.index) + len(r.host_index) == len(starts_s)
    whole = [starts_s[i] for i in r.index]
    # the planned clips, sliced by the host without the last-clip branch (they are not last: a sentinel follows)
    want = host_clip_waveforms(seg, whole + [0.0], 0.3, out_channels)[:-1]
    got = emu_clips(emu, seg._data, r.starts, r.frames, out_channels).reshape(len(whole), out_channels, r.frames)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_clip_frame_ranges_positions_and_short_last_clip():
    rate = 44100
    starts_s = np.arange(0, 20, 4.8)
    assert int(starts_s[3] * 1000) == 14399  # 14.399999999999999 s
    r = audio_util.clip_frame_ranges(20 * rate, rate, starts_s[:4], 5.0)
    assert list(r.index) == [0, 1, 2, 3] and r.frames == 220500 and not r.last_short
    assert list(r.starts) == [0, int(4800 * 44.1), int(9600 * 44.1), int(14399 * (rate / 1000.0))] and r.starts[3] == 634995
    # the fifth start (19.2 s) leaves 0.8 s: it is the last clip and takes the silence branch
    r = audio_util.clip_frame_ranges(20 * rate, rate, starts_s, 5.0)
    assert list(r.index) == [0, 1, 2, 3] and list(r.host_index) == [4] and r.last_short
    # the cases test_resize_cpu pins on the host slicing: 5.3 s of audio
    n = int(5.3 * rate)
    r = audio_util.clip_frame_ranges(n, rate, [0.0, 0.35], 5.0)  # 50 ms missing: the host path raises append's ValueError
    assert list(r.index) == [0] and list(r.host_index) == [1] and r.last_short
    r = audio_util.clip_frame_ranges(n, rate, [0.0, 0.8], 5.0)
    assert list(r.index) == [0] and list(r.host_index) == [1] and r.last_short
    # only the LAST clip has the branch: an earlier short clip is cut by the host, without silence
    r = audio_util.clip_frame_ranges(n, rate, [0.8, 0.0], 5.0)
    assert list(r.index) == [1] and list(r.host_index) == [0] and not r.last_short and list(r.starts) == [0]
    # every planned clip lies inside the track: what the C entry checks again
    for frames, rt, dur in ((751199, 44100, 5.0), (100003, 48000, 0.25), (50000, 22050, 0.1234)):
        st = np.arange(0, frames / rt, dur * 0.9)
        r = audio_util.clip_frame_ranges(frames, rt, st, dur)
        assert (r.starts >= 0).all() and (r.starts + r.frames <= frames).all()
        seg = PcmSegment(np.zeros((frames, 1), np.int16), rt)
        for i, a in zip(r.index, r.starts):
            ms = int(st[i] * 1000)
            clip = seg._slice_ms(ms, ms + int(dur * 1000))
            assert clip.frame_count() == r.frames and a == int(ms * (rt / 1000.0))


def test_cli_keeps_the_host_path_for_what_the_device_refuses():
    from riffusion import cli

    ok = PcmSegment(np.zeros((100, 2), np.int16), 48000)
    assert cli._device_convertible(ok, 44100) and cli._device_convertible(PcmSegment(np.zeros(100, np.int16), 22050), 44100)
    assert not cli._device_convertible(PcmSegment(np.zeros((100, 2), np.int16), 1048577), 44100)  # reduced rate past 2^20
    assert not cli._device_convertible(PcmSegment(np.zeros((100, 3), np.int16), 48000), 44100)  # pydub's own reduction
    assert not cli._device_convertible(PcmSegment(np.zeros((0, 2), np.int16), 48000), 44100)
