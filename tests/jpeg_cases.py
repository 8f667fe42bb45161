"""
The inputs of the JPEG encoder's and decoder's tests (TEST INFRASTRUCTURE ONLY), shared by tests/test_jpeg_cpu.py and
tests/test_gpu_jpeg.py and by the decoder's tests: tile contents and sizes, Pillow's file of a tile, and the encoder's host emulator
(csrc/rfx_jpeg_core.h compiled for the host with tests/emu/rfx_jpeg_emu.cpp), built once per process.
"""
import ctypes
import functools
import io
import os

import numpy as np
from PIL import Image

import emu_build
from riffusion.util import image_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEREO_PNG = "clip_2_start_103694_ms_duration_5678_ms_stereo.png"
QUALITIES = (1, 50, 75, 95, 100)
# (H, W): 1 x 1; whole blocks and MCUs; a dummy Y block to the right (24 x 40), below (24 x 32) and both (23 x 37, 9 x 17); odd
# heights (chroma rows of one pixel row) and odd widths
SIZES = [(1, 1), (8, 8), (16, 16), (9, 17), (24, 32), (32, 40), (24, 40), (23, 37), (62, 33), (40, 24)]


def _golden(name):
    return np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB"))


def _random(h, w):
    return np.random.default_rng(1000 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _primaries():
    """saturated primaries and their complements in 16-pixel patches: the largest chroma DC steps"""
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]],
                       np.uint8)
    idx = (np.arange(3)[:, None] * 3 + np.arange(5)[None, :] * 5) % 8
    return np.ascontiguousarray(colours[np.kron(idx, np.ones((16, 16), np.int64))][:44, :75])


def _checkerboard():
    """a 1-pixel checkerboard of black and white: the largest AC magnitudes"""
    yy, xx = np.mgrid[0:40, 0:56]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def _impulses():
    """a flat tile with a few isolated bright and dark pixels: long zero runs before the last coefficients"""
    t = np.full((64, 80, 3), 90, np.uint8)
    for y, x, v in [(3, 5, 255), (20, 37, 0), (47, 62, 255), (63, 79, 140), (8, 71, 97), (33, 12, 60), (55, 30, 200)]:
        t[y, x] = v
    t[40, 41] = (255, 0, 0)
    return t


def _mono_noise():
    g = np.random.default_rng(5).integers(0, 256, size=(33, 50), dtype=np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


CONTENTS = {
    **{f"random_{h}x{w}": functools.partial(_random, h, w) for h, w in SIZES},
    "zeros": lambda: np.zeros((24, 40, 3), np.uint8),
    "ones": lambda: np.full((23, 37, 3), 255, np.uint8),
    "mono_noise": _mono_noise,
    "primaries": _primaries,
    "checkerboard": _checkerboard,
    "impulses": _impulses,
    "stereo_crop": lambda: np.ascontiguousarray(_golden(STEREO_PNG)[200:264, 300:396]),
    "stereo_full": lambda: _golden(STEREO_PNG),
    "og_beat": lambda: _golden("og_beat.png"),
}


@functools.lru_cache(maxsize=1)
def _emu():
    lib = ctypes.CDLL(emu_build.shared("rfx_jpeg_emu.cpp"))
    lib.emu_jpeg_quant_tables.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_jpeg_scan_capacity.restype = ctypes.c_uint64
    lib.emu_jpeg_scan_capacity.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.emu_jpeg_encode_u8.restype = ctypes.c_int64
    lib.emu_jpeg_encode_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p]
    return lib


def emu_file(tile, quality, exif=None):
    """(header + emulated scan, ZRL codes emitted)"""
    lib = _emu()
    tile = np.ascontiguousarray(tile, dtype=np.uint8)
    H, W, _ = tile.shape
    qt = np.zeros((2, 64), np.uint16)
    assert lib.emu_jpeg_quant_tables(quality, qt.ctypes.data, qt.ctypes.data + 128) == 0, quality
    cap = lib.emu_jpeg_scan_capacity(H, W)
    scan = np.zeros(cap, np.uint8)
    zrl = ctypes.c_int64(0)
    n = lib.emu_jpeg_encode_u8(tile.ctypes.data, H, W, qt.ctypes.data, scan.ctypes.data, cap, ctypes.byref(zrl))
    assert 2 <= n <= cap, n
    return image_util.jpeg_header(W, H, quality, image_util.jpeg_exif_bytes(exif), qtables=qt) + scan[:n].tobytes(), int(zrl.value)


def pillow_file(tile, quality, exif=None):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(tile)).save(buf, "JPEG", quality=quality, **({} if exif is None else {"exif": exif}))
    return buf.getvalue()
