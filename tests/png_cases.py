"""
The inputs of the PNG writer's tests (TEST INFRASTRUCTURE ONLY), shared by tests/test_png_cpu.py, tests/test_png_decode_cpu.py and
tests/test_gpu_png.py: tile contents and sizes, the writer's host emulator (csrc/rfx_png_core.h compiled for the host with
tests/emu/rfx_png_emu.cpp), built once per process, its stream and file of a tile, Pillow's file of the same pixels, a file's chunks.
"""
import ctypes
import functools
import io
import os
import struct
import zlib

import numpy as np
from PIL import Image

import emu_build
from riffusion import _hip
from riffusion.util import image_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MONO_PNG = "clip_2_start_103694_ms_duration_5678_ms.png"
STEREO_PNG = "clip_2_start_103694_ms_duration_5678_ms_stereo.png"
# (H, W): one row; a last block of 1 row (33) and of 31 rows (31); row lengths of every residue mod 4
SIZES = [(1, 1), (1, 2), (3, 5), (31, 7), (32, 8), (33, 50), (65, 171), (70, 87)]
RUN_LENGTHS = (3, 4, 257, 258, 259, 260, 261, 262, 517)
SPECTROGRAM_TILES = ("agile.png", "marim.png", "motorway.png", "vibes.png", "og_beat.png", MONO_PNG, STEREO_PNG)
MASKS = ("mask_beat_lines_80.png", "mask_gradient_dark.png")
RATIO_BOUND = 1.02


def _golden(name):
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB")))


def _random(h, w):
    return np.random.default_rng(1000 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _mono(grey):
    return np.ascontiguousarray(np.repeat(np.asarray(grey, np.uint8)[:, :, None], 3, axis=2))


def _run_heavy(h, w):
    """few values in long stretches, colour: runs of every length up to whole rows, many of them across row ends"""
    rng = np.random.default_rng(7000 * h + w)
    flat = np.repeat(rng.integers(0, 4, size=h * w * 3 // 2 + 1), rng.integers(1, 12, size=h * w * 3 // 2 + 1))[:h * w * 3]
    return np.ascontiguousarray((flat * 85).astype(np.uint8).reshape(h, w, 3))


def _run_lengths_tile():
    """A grey tile whose rows are 1, 255, 1, 255, ... (a row and the next out of step), so that filter None wins every row, with
    stretches of zeros: rows 0 .. 8 hold one run each of exactly RUN_LENGTHS bytes; row 10 ends and row 11 begins with zeros (a run
    across a row end, through the filter byte 0); row 31 ends and row 32 begins with zeros (a run cut at the block's end)."""
    H, W = 40, 600
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.where((yy + xx) & 1, 255, 1).astype(np.uint8)
    for row, n in enumerate(RUN_LENGTHS):
        g[row, 20:20 + n] = 0
    g[10, W - 7:] = 0
    g[11, :5] = 0
    g[31, W - 9:] = 0
    g[32, :11] = 0
    return _mono(g)


CONTENTS = {
    **{f"random_{h}x{w}": functools.partial(_random, h, w) for h, w in SIZES},
    **{f"runs_{h}x{w}": functools.partial(_run_heavy, h, w) for h, w in SIZES},
    "zeros": lambda: np.zeros((70, 87, 3), np.uint8),
    "ones": lambda: np.full((33, 50, 3), 255, np.uint8),
    "mono_noise": lambda: _mono(np.random.default_rng(5).integers(0, 256, size=(65, 171), dtype=np.uint8)),
    "run_lengths": _run_lengths_tile,
    **{name: functools.partial(_golden, name) for name in SPECTROGRAM_TILES + MASKS},
}


def is_mono(tile):
    return bool((tile[:, :, 0] == tile[:, :, 1]).all() and (tile[:, :, 0] == tile[:, :, 2]).all())


@functools.lru_cache(maxsize=None)
def _tile(name):
    t = CONTENTS[name]()
    t.setflags(write=False)
    return t


def modes_of(name):
    return ("rgb", "gray", "auto") if is_mono(_tile(name)) else ("rgb", "auto")


CASES = [(name, mode) for name in CONTENTS for mode in modes_of(name)]


@functools.lru_cache(maxsize=1)
def _emu():
    lib = ctypes.CDLL(emu_build.shared("rfx_png_emu.cpp"))
    lib.emu_png_stream_capacity.restype = ctypes.c_uint64
    lib.emu_png_stream_capacity.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.emu_png_code_lengths.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_png_block_histogram.restype = None
    lib.emu_png_block_histogram.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.emu_png_encode_u8.restype = ctypes.c_int64
    lib.emu_png_encode_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emu_stream(tile, mode):
    """the emulator's (stream, CRC-32 of b"IDAT" + stream, channels, [blocks without a match, longest code, blocks limited])"""
    lib = _emu()
    tile = np.ascontiguousarray(tile, dtype=np.uint8)
    H, W, _ = tile.shape
    m = _hip.PNG_MODES[mode]
    cap = lib.emu_png_stream_capacity(H, W, 1 if m == 1 else 3)
    out = np.zeros(cap, np.uint8)
    crc, ch = ctypes.c_uint32(0), ctypes.c_int32(-1)
    stats = np.zeros(3, np.int64)
    n = lib.emu_png_encode_u8(tile.ctypes.data, H, W, m, out.ctypes.data, cap, ctypes.byref(crc), ctypes.byref(ch), stats.ctypes.data)
    assert 0 <= n <= cap, n  # (-1: the capacity would be passed)
    return out[:n].tobytes(), int(crc.value), int(ch.value), stats


def emu_file(tile, mode, exif=None):
    stream, crc, ch, _ = emu_stream(tile, mode)
    assert ch in (1, 3), (ch, (1, 3))
    return image_util.png_file(tile.shape[1], tile.shape[0], ch, stream, crc, image_util.png_exif_bytes(exif))


def pillow_image(tile, channels):
    return Image.fromarray(np.ascontiguousarray(tile if channels == 3 else tile[:, :, 0]))


def pillow_file(tile, channels, exif=None, **options):
    buf = io.BytesIO()
    pillow_image(tile, channels).save(buf, "PNG", **({} if exif is None else {"exif": exif}), **options)
    return buf.getvalue()


def chunks(data):
    """[(type, payload)] of a PNG file; every chunk's CRC is checked on the way"""
    assert data[:8] == image_util.PNG_SIGNATURE, (data[:8], image_util.PNG_SIGNATURE)
    out, at = [], 8
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload), kind
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data) and out[-1][0] == b"IEND", (at, len(data), out[-1][0])
    return out


def layout(parsed):
    """the chunk types in order, a file's consecutive IDATs as one (Pillow cuts its payload into IDATs of 64 KiB)"""
    kinds = [k for k, _ in parsed]
    return [k for i, k in enumerate(kinds) if not (k == b"IDAT" and i and kinds[i - 1] == b"IDAT")]


@functools.lru_cache(maxsize=None)
def _case(name, mode):
    """(emulator's file, channels, stats, Pillow's Z_RLE file of the same pixels in the same mode): computed once"""
    tile = _tile(name)
    stream, crc, ch, stats = emu_stream(tile, mode)
    got = image_util.png_file(tile.shape[1], tile.shape[0], ch, stream, crc)
    return got, ch, stats, pillow_file(tile, ch, compress_type=zlib.Z_RLE)


# ---- the code builder alone ----------------------------------------------------------------------------------------------------
def _fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def _build(counts, limit):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    lens = np.full(counts.size, 99, np.uint8)
    codes = np.zeros(counts.size, np.uint16)
    used = _emu().emu_png_code_lengths(counts.ctypes.data, counts.size, limit, lens.ctypes.data, codes.ctypes.data)
    assert used == int((counts > 0).sum()), (used, int((counts > 0).sum()))
    return lens.astype(np.int64), codes


def _unlimited_depth(counts):
    """the longest code of Huffman's tree over the used symbols"""
    import heapq

    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def _padded(values, n):
    return np.asarray(list(values) + [0] * (n - len(values)), np.uint32)


BUILDER_CASES = {
    "fib44_of_286": (_padded(_fib(44), 286), 15, True),
    "fib40_then_ones_all_286": (np.asarray(_fib(40) + [1] * 246, np.uint32), 15, True),
    "fib44_scattered": (np.roll(_padded(_fib(44), 286), 173), 15, True),
    "fib19": (np.asarray(_fib(19), np.uint32), 7, True),
    "fib12_of_19": (_padded([0, 0, 0] + _fib(12), 19), 7, True),
    "one_symbol_and_eob": (np.bincount([7, 256], weights=[500, 1], minlength=286).astype(np.uint32), 15, False),
    "two_symbols": (np.bincount([0, 285], weights=[3, 3], minlength=286).astype(np.uint32), 15, False),
    "all_286_equal": (np.full(286, 9, np.uint32), 15, False),
    "all_286_ramp": (np.arange(1, 287, dtype=np.uint32), 15, False),
    "all_19_equal": (np.full(19, 2, np.uint32), 7, False),
    "two_of_19": (_padded([0, 5, 0, 0, 1], 19), 7, False),
}
