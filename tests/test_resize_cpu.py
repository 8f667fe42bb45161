"""
CPU checks of the tile resize (csrc/rfx_resize_core.h, compiled for the host with tests/emu/rfx_resize_emu.cpp): the emulated
kernels against PIL.Image.resize byte for byte - BICUBIC and LANCZOS (and BILINEAR) on audio-to-audio's 501 <-> 512, other
widths, both axes at once (the vertical pass over the uint8 intermediate), random content and the golden PNGs - the library's
host-only coefficient entry against the emulator's tables, and audio_util's ports of audio_to_audio's clip slicing.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
from PIL import Image

import emu_build
from riffusion.util import audio_util
from riffusion.util.audio_util import PcmSegment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILTERS = {"BICUBIC": Image.BICUBIC, "LANCZOS": Image.LANCZOS, "BILINEAR": Image.BILINEAR}
# (in (W, H), out (W, H)): audio-to-audio's pair, other widths, upscales from tiny tiles, and both axes changing
SIZES = [((501, 512), (512, 512)), ((512, 512), (501, 512)), ((500, 512), (512, 512)), ((512, 512), (500, 512)),
         ((512, 512), (7, 512)), ((1, 1), (32, 32)), ((17, 17), (512, 512)), ((401, 300), (333, 257)), ((512, 64), (64, 512)),
         ((512, 501), (512, 512)), ((96, 80), (97, 33))]


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared("rfx_resize_emu.cpp", "-ffp-contract=off"))
    lib.emu_resize_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p]
    lib.emu_resize_ksize.argtypes = [ctypes.c_int] * 3
    lib.emu_resize_coefficients.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _emu_resize(lib, tiles: np.ndarray, size, resample) -> np.ndarray:
    tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
    N, H, W, _ = tiles.shape
    out = np.empty((N, size[1], size[0], 3), np.uint8)
    assert lib.emu_resize_u8(tiles.ctypes.data, N, H, W, size[1], size[0], int(resample), out.ctypes.data) == 0
    return out


def _pil_resize(tiles: np.ndarray, size, resample) -> np.ndarray:
    return np.stack([np.asarray(Image.fromarray(t).resize(size, resample)) for t in tiles])


@pytest.mark.parametrize("name", sorted(FILTERS))
@pytest.mark.parametrize("src,dst", SIZES)
def test_emulator_equals_pillow_random(emu, name, src, dst):
    rng = np.random.default_rng(src[0] * 7 + dst[0])
    tiles = rng.integers(0, 256, size=(2, src[1], src[0], 3), dtype=np.uint8)
    tiles[1, :, : src[0] // 2] = 255  # flat regions and hard edges: the clamps at 0 and 255 and the overshoot of the lobes
    tiles[1, ::3, :, 1] = 0
    got = _emu_resize(emu, tiles, dst, FILTERS[name])
    assert np.array_equal(got, _pil_resize(tiles, dst, FILTERS[name]))


@pytest.mark.parametrize("name", ["BICUBIC", "LANCZOS"])
def test_emulator_equals_pillow_golden_pngs(emu, name):
    pngs = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "*.png")))
            if os.path.basename(p).split(".")[0] in ("og_beat", "agile", "marim", "motorway", "vibes")]
    assert len(pngs) == 5
    for path in pngs:
        tile = np.asarray(Image.open(path).convert("RGB"))[None]
        H, W = tile.shape[1:3]
        for dst in [(501, H), (int(np.ceil(W / 32) * 32) + 32, H), (W - W % 32 - 32, H - 64), (7, 9)]:
            got = _emu_resize(emu, tile, dst, FILTERS[name])
            assert np.array_equal(got, _pil_resize(tile, dst, FILTERS[name])), (path, dst)


def test_unchanged_size_is_a_copy(emu):
    tiles = np.random.default_rng(3).integers(0, 256, size=(3, 20, 30, 3), dtype=np.uint8)
    assert np.array_equal(_emu_resize(emu, tiles, (30, 20), Image.LANCZOS), tiles)


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_library_coefficients_equal_emulator(emu, name):
    """rfx_image_resize_coefficients (host only: no GPU) returns the planner's tables."""
    from riffusion import _hip

    for n_in, n_out in [(501, 512), (512, 501), (512, 7), (1, 32), (333, 1000)]:
        k = emu.emu_resize_ksize(n_in, n_out, FILTERS[name])
        bounds = np.zeros(2 * n_out, np.int32)
        kk = np.zeros(n_out * k, np.int32)
        assert emu.emu_resize_coefficients(n_in, n_out, FILTERS[name], bounds.ctypes.data, kk.ctypes.data) == k
        table = _hip.resize_coefficients(n_in, n_out, FILTERS[name])
        assert np.array_equal(table, np.concatenate([bounds, kk]))
        assert (bounds[1::2] <= k).all() and (bounds[::2] + bounds[1::2] <= n_in).all()


def test_library_refuses_bad_arguments():
    from riffusion import _hip

    for args in [(0, 5, Image.BICUBIC), (5, 0, Image.BICUBIC), (5, 16385, Image.BICUBIC), (5, 6, Image.NEAREST), (5, 6, 4), (5, 6, 5)]:
        with pytest.raises(_hip.RfxError):
            _hip.resize_coefficients(*args)


# ---- audio_to_audio.py's clip slicing ------------------------------------------------------------------------------------------
def _golden_track() -> PcmSegment:
    from scipy.io import wavfile

    wavs = sorted(glob.glob(os.path.join(GOLDEN, "clip_*.wav")))
    assert len(wavs) == 3
    return PcmSegment(np.concatenate([wavfile.read(w)[1] for w in wavs]), 44100)


def test_clip_start_times_of_the_golden_track():
    track = _golden_track()
    assert track.get_array_of_samples().size // 2 == 751199 and round(track.duration_seconds, 2) == 17.03
    starts = audio_util.clip_start_times(track.duration_seconds)
    assert np.array_equal(starts, np.arange(0, track.duration_seconds - 5.0, 4.8)) and len(starts) == 3
    clips = audio_util.slice_audio_into_clips(track, starts, 5.0)
    assert [int(t * 1000) for t in starts] == [0, 4800, 9600]
    assert [c.frame_count() for c in clips] == [220500.0] * 3
    for t, c in zip(starts, clips):
        a = int(int(t * 1000) * 44.1)
        assert np.array_equal(c._data, track._data[a : a + 220500])


def test_slice_positions_truncate_to_milliseconds():
    rate = 44100
    track = PcmSegment(np.arange(20 * rate, dtype=np.int64).astype(np.int16), rate)
    starts = np.arange(0, 20, 4.8)
    assert int(starts[3] * 1000) == 14399  # 14.399999999999999 s
    clips = audio_util.slice_audio_into_clips(track, starts[:4], 5.0)
    a = int(14399 * (rate / 1000.0))
    assert np.array_equal(clips[3]._data, track._data[a : a + 220500])
    assert all(c.frame_count() == 220500 for c in clips)


def test_last_clip_silence_branch_as_the_reference_has_it():
    rate = 44100
    x = (np.sin(np.arange(int(5.3 * rate)) * 0.05) * 8000).astype(np.int16)
    # 50 ms of the last clip missing: append's default 100 ms crossfade is longer than the silence -> ValueError, like pydub
    with pytest.raises(ValueError, match="Crossfade is longer"):
        audio_util.slice_audio_into_clips(PcmSegment(x, rate), [0.0, 0.35], 5.0)
    # 500 ms missing: the silence is crossfaded INTO the clip's end (100 ms), so the clip is 100 ms short of 5 s
    clips = audio_util.slice_audio_into_clips(PcmSegment(x, rate), [0.0, 0.8], 5.0)
    head = PcmSegment(x, rate)._slice_ms(800, 5800)
    want = head.append(PcmSegment.silent(duration=500))
    assert clips[0].frame_count() == 220500 and np.array_equal(clips[1]._data, want._data)
    assert len(clips[1]) == 4900
    # only the LAST clip gets the branch: an earlier short clip stays short
    short = audio_util.slice_audio_into_clips(PcmSegment(x, rate), [0.8, 0.0], 5.0)
    assert short[0].frame_count() == head.frame_count() and short[1].frame_count() == 220500


def test_pydub_silent_length():
    s = PcmSegment.silent(duration=155)
    assert s.frame_rate == 11025 and s.channels == 1 and s.frame_count() == int(11025 * 0.155)
