"""
What the JPEG decoder's tests share (TEST INFRASTRUCTURE ONLY): Pillow's files and pixels, the decoder's host emulator
(csrc/rfx_jpeg_dec_core.h compiled for the host with tests/emu/rfx_jpeg_dec_emu.cpp) as a shared library and as the stand-alone
sanitizer program, each built once per process, and the damaged scans.
"""
import ctypes
import functools
import io

import numpy as np
from PIL import Image

import emu_build
from jpeg_cases import _random
from riffusion.util import image_util

EMU_SRC = "rfx_jpeg_dec_emu.cpp"
SMALL = [(1, 2), (2, 1), (2, 2), (3, 2), (3, 3), (4, 4), (5, 3), (5, 4), (5, 5), (6, 5)]  # around W = 4: replicated / filtered chroma


def pillow_jpeg(tile, quality, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(tile)).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=1)
def _emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC))
    lib.emu_jpeg_decode_u8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emu_decode(data):
    """(status, pixels, [most rounds of a group, subsequences, groups, rounds in all], scan) of a file jpeg_parse gives to the device"""
    info = image_util.jpeg_parse(data)
    assert info.ok_for_device, info.reason
    scan = np.frombuffer(data, np.uint8)[info.scan[0]:info.scan[1]].copy()
    out = np.zeros((info.height, info.width, 3), np.uint8)
    stats = np.zeros(4, np.int32)
    qt, huff = np.ascontiguousarray(info.qtables), np.ascontiguousarray(info.huffman)
    status = _emu().emu_jpeg_decode_u8(scan.ctypes.data, scan.size, info.height, info.width, qt.ctypes.data, huff.ctypes.data,
                                       out.ctypes.data, stats.ctypes.data)
    return status, out, stats, scan.tobytes()


# ---- damaged scans: the stand-alone sanitizer program ---------------------------------------------------------------------------
def damaged_scans(scan):
    """the four damaged versions of a scan the issue names"""
    third, two_thirds, mid = len(scan) // 3, 2 * len(scan) // 3, len(scan) // 2
    return {
        "truncated at a third": scan[:third],
        "truncated at two thirds": scan[:two_thirds],
        "one byte flipped mid-scan": scan[:mid] + bytes([scan[mid] ^ 0xFF]) + scan[mid + 1:],
        "an all-0xFF tail": scan[:two_thirds] + b"\xff" * (len(scan) - two_thirds),
    }


# a dozen subsequences, some twenty, and more than a group.  (Not every flipped byte damages a scan: the one in the middle of
# "stereo_crop" at quality 75 leaves a scan that codes another picture with the same number of blocks - the next test.)
DAMAGE_TILES = {"random_32x40": 75, "random_62x33": 95, "og_beat": 75}


@functools.lru_cache(maxsize=1)
def _sanitizer_program():
    return emu_build.sanitized_program(EMU_SRC, "-DRFX_JPD_EMU_MAIN", static=False)


def _conv(stereo=False, **kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, **kw), device="cuda")


def _three(h, w):
    a = _random(h, w)
    return [a, np.ascontiguousarray(a[::-1, ::-1] ^ 0x5A), np.repeat(a[:, :, :1] // 2, 3, axis=2)]
