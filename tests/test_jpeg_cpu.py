"""
CPU checks of the JPEG encoder (csrc/rfx_jpeg_core.h, compiled for the host with tests/emu/rfx_jpeg_emu.cpp, in the kernels'
stages) and of image_util.jpeg_header: header + emulated scan against the file Pillow writes on this machine -
`Image.fromarray(t).save(f, "JPEG", quality=q[, exif=e])` - byte for byte, no tolerance.  Random tiles at the sizes that have
dummy blocks to the right and below, odd and even remainders and chroma rows made of one pixel row; the contents that reach the
encoder's corners (flat, saturated primaries, a 1-pixel checkerboard, isolated impulses, the golden tiles) at qualities 1, 50,
75, 95 and 100; a file with the spectrogram EXIF; the library's quantisation tables against the ones Pillow reads back.
"""
import functools
import io

import numpy as np
import pytest
from PIL import Image

from jpeg_cases import CONTENTS, QUALITIES, STEREO_PNG, _checkerboard, _emu, _golden, _primaries, _random, emu_file, pillow_file
from riffusion import _hip
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import image_util

CASES = [(name, q) for name in CONTENTS for q in QUALITIES]


@functools.lru_cache(maxsize=None)
def _case(name, quality):
    """(emulator's file, Pillow's file, ZRLs): computed once, shared by the equality test and the conditions"""
    tile = CONTENTS[name]()
    got, zrl = emu_file(tile, quality)
    return got, pillow_file(tile, quality), zrl


def _scan_of(data):
    """the entropy-coded bytes of a baseline file: after the SOS segment, up to EOI"""
    at = 2
    while data[at + 1] != 0xDA:
        at += 2 + int.from_bytes(data[at + 2:at + 4], "big")
    return data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):-2]


@pytest.mark.parametrize("name,quality", CASES)
def test_emulator_file_equals_pillow(name, quality):
    got, want, _ = _case(name, quality)
    assert got == want


def test_the_set_reaches_byte_stuffing_and_zrl():
    """conditions, not measurements: Pillow's own scans hold stuffed 0xFF bytes and the emulator emitted ZRL codes, so neither
    path is left out of the comparison above"""
    results = [_case(name, q) for name, q in CASES]
    assert any(b"\xff\x00" in _scan_of(want) for _, want, _ in results)
    assert sum(zrl for _, _, zrl in results) > 0
    # ... and the checkerboard at quality 100 holds AC coefficients of the 10-bit category: magnitudes >= 512 after the division by 1
    assert _case("checkerboard", 100)[0] == _case("checkerboard", 100)[1]


def test_content_shapes():
    assert _golden(STEREO_PNG).shape == (512, 568, 3)
    assert _primaries().shape == (44, 75, 3) and _checkerboard().shape == (40, 56, 3)
    assert CONTENTS["stereo_crop"]().shape == (64, 96, 3)


def test_file_with_spectrogram_exif_equals_pillow():
    params = SpectrogramParams(stereo=True)
    exif_data = params.to_exif()
    exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(np.float32(12345678.0))
    tile = np.ascontiguousarray(_golden(STEREO_PNG)[100:164, 40:139])
    image = Image.fromarray(tile)
    image.getexif().update(exif_data.items())
    buf = io.BytesIO()
    image.save(buf, exif=image.getexif(), format="JPEG")  # the save of cli.py's flush: Pillow's default quality is 75
    exif = Image.Exif()
    exif.update(exif_data.items())
    got, _ = emu_file(tile, 75, exif)
    assert got == buf.getvalue()
    back = Image.open(io.BytesIO(got))
    assert SpectrogramParams.from_exif(back.getexif()) == params
    assert back.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] == 12345678.0


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 95, 100])
def test_library_quant_tables_equal_pillow(quality):
    tables = _hip.jpeg_quant_tables(quality)
    back = Image.open(io.BytesIO(pillow_file(_random(8, 8), quality))).quantization
    assert sorted(back) == [0, 1]
    for i in (0, 1):
        assert np.array_equal(tables[i], np.asarray(back[i])), (quality, i)  # Pillow hands the tables over in natural order
    emu = np.zeros((2, 64), np.uint16)
    assert _emu().emu_jpeg_quant_tables(quality, emu.ctypes.data, emu.ctypes.data + 128) == 0
    assert np.array_equal(emu, tables)


@pytest.mark.parametrize("quality", [0, 101, -1])
def test_quality_outside_1_to_100_is_refused(quality):
    lib = _hip.load_library()
    t = np.zeros((2, 64), np.uint16)
    assert lib.rfx_jpeg_quant_tables(quality, t.ctypes.data, t.ctypes.data + 128) == -4  # RFX_ERR_UNSUPPORTED
    assert b"quality" in lib.rfx_last_error() and not t.any()
    with pytest.raises(_hip.RfxError, match="quality"):
        _hip.jpeg_quant_tables(quality)


def test_capacity_and_workspace_queries():
    lib = _hip.load_library()
    # 2 * ceil(1660 bits * blocks / 8) + 2 (include/rfx.h)
    assert lib.rfx_jpeg_scan_capacity(512, 512) == 2 * ((1660 * 6 * 32 * 32 + 7) // 8) + 2
    assert lib.rfx_jpeg_scan_capacity(1, 1) == 2 * ((1660 * 6 + 7) // 8) + 2
    assert lib.rfx_jpeg_scan_capacity(17, 16) == lib.rfx_jpeg_scan_capacity(32, 16)
    assert lib.rfx_jpeg_scan_capacity(512, 65536) == 0 and lib.rfx_jpeg_scan_capacity(0, 8) == 0
    assert lib.rfx_jpeg_encode_workspace_bytes(1, 512, 65536) == 0 and lib.rfx_jpeg_encode_workspace_bytes(0, 8, 8) == 0
    assert lib.rfx_jpeg_encode_workspace_bytes(3, 512, 501) > 3 * 6 * 32 * 32 * 128
    assert _emu().emu_jpeg_scan_capacity(512, 501) == lib.rfx_jpeg_scan_capacity(512, 501)


def test_header_arguments():
    with pytest.raises(ValueError):
        image_util.jpeg_header(65536, 8, 75)
    with pytest.raises(ValueError):
        image_util.jpeg_header(8, 0, 75)
    with pytest.raises(ValueError):
        image_util.jpeg_header(8, 8, 75, b"Exif\0\0" + bytes(65534))
    assert image_util.jpeg_header(8, 8, 75) == pillow_file(np.zeros((8, 8, 3), np.uint8), 75)[:len(image_util.jpeg_header(8, 8, 75))]
