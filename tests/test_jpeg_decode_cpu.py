"""
CPU checks of the JPEG decoder (csrc/rfx_jpeg_dec_core.h, compiled for the host with tests/emu/rfx_jpeg_dec_emu.cpp, in the
kernels' stages and with the kernels' subsequences, groups and synchronisation rounds) and of image_util.jpeg_parse: the emulator's
pixels against `np.asarray(Image.open(f).convert("RGB"))` of the Pillow on this machine, byte for byte, no tolerance.  The files
are the ones Pillow writes from the contents and sizes of tests/test_jpeg_cpu.py at qualities 1, 50, 75, 95 and 100, with the
standard and with optimised Huffman tables; a file with the spectrogram EXIF; sizes of at most two chroma columns (libjpeg
replicates their chroma instead of filtering it).  Conditions on the set keep every path in the comparison.  Damaged scans go
through a stand-alone sanitizer build of the emulator: a non-zero status and no read outside the buffers.
"""
import functools
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from jpeg_cases import CONTENTS, QUALITIES, STEREO_PNG, _golden, _random
from jpeg_decode_cases import DAMAGE_TILES, SMALL, _emu, _sanitizer_program, damaged_scans, emu_decode, pillow_jpeg, pillow_pixels
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import image_util

FULL = ("stereo_full", "og_beat")  # the two full-size golden tiles: quality 75 only
CASES = [(name, q, opt) for name in CONTENTS for q in ((75,) if name in FULL else QUALITIES) for opt in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(name, quality, optimize):
    """(file, status, emulator's pixels, stats, scan): decoded once, shared by the equality test and the conditions"""
    data = pillow_jpeg(CONTENTS[name](), quality, optimize=optimize)
    return (data,) + emu_decode(data)


@pytest.mark.parametrize("name,quality,optimize", CASES)
def test_emulator_pixels_equal_pillow(name, quality, optimize):
    data, status, got, stats, _ = _case(name, quality, optimize)
    print(name, quality, optimize, "scan bytes, [max rounds, subsequences, groups, rounds]:", len(data), stats)
    assert status == 0
    assert np.array_equal(got, pillow_pixels(data))


@pytest.mark.parametrize("h,w", SMALL)
def test_sizes_around_two_chroma_columns(h, w):
    for q in (50, 90):
        data = pillow_jpeg(_random(h, w), q)
        status, got, _, _ = emu_decode(data)
        assert status == 0 and np.array_equal(got, pillow_pixels(data)), (h, w, q)


def test_the_set_reaches_every_path():
    """conditions, not measurements, on Pillow's own files: a stuffed FF 00, more than one synchronisation round, more
    subsequences than one group holds, a scan shorter than one subsequence, Huffman tables that are not Annex K's"""
    lib = _emu()
    sub_bits, group = lib.emu_jpeg_dec_sub_bits(), lib.emu_jpeg_dec_group()
    results = [_case(*c) for c in CASES]
    assert any(b"\xff\x00" in scan for *_, scan in results)
    assert any(stats[0] > 1 for _, _, _, stats, _ in results)
    assert any(stats[1] > group and stats[2] > 1 for _, _, _, stats, _ in results)
    tiny = _case("random_1x1", 75, False)
    assert 0 < len(tiny[4]) * 8 < sub_bits and tiny[3][1] == 1 and tiny[3][0] == 0
    # no group takes more rounds than it has subsequences
    assert all(stats[0] <= min(stats[1], group) for _, _, _, stats, _ in results)
    standard = {tc_th: bits + vals for tc_th, bits, vals in image_util.JPEG_HUFFMAN_TABLES}
    plain = image_util.jpeg_parse(_case("random_23x37", 75, False)[0]).huffman
    optimised = image_util.jpeg_parse(_case("random_23x37", 75, True)[0]).huffman
    for row, key in enumerate((0x00, 0x10, 0x01, 0x11)):
        assert plain[row].tobytes().rstrip(b"\0") == standard[key].rstrip(b"\0")
        assert optimised[row].tobytes() != plain[row].tobytes()
    assert b"\xff\xc4" in _case("random_23x37", 75, True)[0]


def test_file_with_spectrogram_exif():
    params = SpectrogramParams(stereo=True)
    exif = Image.Exif()
    exif.update(params.to_exif().items())
    exif[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(np.float32(12345678.0))
    data = pillow_jpeg(_golden(STEREO_PNG)[100:164, 40:139], 75, exif=exif)
    status, got, _, _ = emu_decode(data)
    assert status == 0 and np.array_equal(got, pillow_pixels(data))
    info = image_util.jpeg_parse(data)
    assert info.exif == Image.open(io.BytesIO(data)).info["exif"]
    back = Image.Exif()
    back.load(info.exif)
    assert SpectrogramParams.from_exif(back) == params and back[SpectrogramParams.ExifTags.MAX_VALUE.value] == 12345678.0
    assert dict(back) == dict(Image.open(io.BytesIO(data)).getexif())


@pytest.mark.parametrize("quality,optimize", [(1, False), (50, True), (75, False), (100, True)])
def test_parse_tables_and_size_equal_pillow(quality, optimize):
    data = pillow_jpeg(_random(23, 37), quality, optimize=optimize)
    info = image_util.jpeg_parse(data)
    opened = Image.open(io.BytesIO(data))
    assert info.ok_for_device and info.reason == "" and (info.width, info.height) == opened.size == (37, 23)
    assert sorted(opened.quantization) == [0, 1]
    for i in (0, 1):
        assert np.array_equal(info.qtables[i], np.asarray(opened.quantization[i]))  # natural order, as Pillow hands them over
    assert info.qtables.dtype == np.uint16 and info.huffman.shape == (4, 272) and info.huffman.dtype == np.uint8
    assert data[info.scan[1]:] == b"\xff\xd9" and data[info.scan[0] - 10:info.scan[0]] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert info.exif == b""


def test_parse_keeps_other_files_on_the_host():
    tile = _random(24, 40)
    cases = {
        "progressive": pillow_jpeg(tile, 75, progressive=True),
        "greyscale": (lambda b: (Image.fromarray(tile).convert("L").save(b, "JPEG"), b.getvalue())[1])(io.BytesIO()),
        "subsampling": pillow_jpeg(tile, 75, subsampling=0),
        "restart": pillow_jpeg(tile, 75, restart_marker_blocks=4),
        "not a JPEG": b"\x89PNG\r\n\x1a\n" + bytes(40),
        "empty": b"",
        "no EOI": pillow_jpeg(tile, 75)[:-2],
        "cut in a segment": pillow_jpeg(tile, 75)[:100],
    }
    for name, data in cases.items():
        info = image_util.jpeg_parse(data)
        assert not info.ok_for_device and info.reason, name
    assert "progressive" in image_util.jpeg_parse(cases["progressive"]).reason
    assert "greyscale" in image_util.jpeg_parse(cases["greyscale"]).reason
    assert "4:2:0" in image_util.jpeg_parse(cases["subsampling"]).reason
    assert "restart" in image_util.jpeg_parse(cases["restart"]).reason
    assert "not a JPEG" in image_util.jpeg_parse(cases["not a JPEG"]).reason
    assert (image_util.jpeg_parse(cases["progressive"]).width, image_util.jpeg_parse(cases["progressive"]).height) == (40, 24)
    # every prefix of a file parses without raising, and none but the whole file is the device's
    whole = pillow_jpeg(tile, 75)
    assert all(not image_util.jpeg_parse(whole[:n]).ok_for_device for n in range(0, len(whole), 7))


# ---- damaged scans: the stand-alone sanitizer program ---------------------------------------------------------------------------
def _run_sanitized(info, scan, tmp_path, tag):
    path = os.path.join(tmp_path, f"{tag}.bin")
    with open(path, "wb") as f:
        f.write(np.array([info.height, info.width, len(scan)], np.int32).tobytes())
        f.write(np.ascontiguousarray(info.qtables).tobytes() + np.ascontiguousarray(info.huffman).tobytes() + scan)
    done = subprocess.run([_sanitizer_program(), path], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]  # a sanitizer report ends the program with another code
    assert done.stdout.startswith("status ")
    return int(done.stdout.split()[1])


@pytest.mark.parametrize("name", sorted(DAMAGE_TILES))
def test_damaged_scans_give_a_status_and_no_read_out_of_bounds(name, tmp_path):
    data = pillow_jpeg(CONTENTS[name](), DAMAGE_TILES[name])
    info = image_util.jpeg_parse(data)
    scan = data[info.scan[0]:info.scan[1]]
    assert _run_sanitized(info, scan, str(tmp_path), "whole") == 0
    for i, (what, bad) in enumerate(damaged_scans(scan).items()):
        status = _run_sanitized(info, bad, str(tmp_path), f"bad{i}")
        print(name, what, "status", status)
        assert status != 0, what
    # a table that is no prefix code, and tables of nothing but zeros
    broken = info._replace(huffman=info.huffman.copy())
    broken.huffman[1, :16] = 255
    assert _run_sanitized(broken, scan, str(tmp_path), "table") == 2
    assert _run_sanitized(info._replace(huffman=np.zeros_like(info.huffman)), scan, str(tmp_path), "zeros") != 0
    assert _run_sanitized(info, b"", str(tmp_path), "none") != 0


def test_a_flipped_byte_that_leaves_a_valid_scan_decodes_as_pillow():
    """the decoder falls back into step after the flipped byte and the scan ends with its last block: nothing is wrong with
    such a scan, so the status is 0 - and the pixels are the ones Pillow decodes from the same bytes"""
    data = pillow_jpeg(CONTENTS["stereo_crop"](), 75)
    info = image_util.jpeg_parse(data)
    mid = info.scan[0] + (info.scan[1] - info.scan[0]) // 2
    bad = data[:mid] + bytes([data[mid] ^ 0xFF]) + data[mid + 1:]
    status, got, _, _ = emu_decode(bad)
    assert status == 0 and np.array_equal(got, pillow_pixels(bad)) and not np.array_equal(got, pillow_pixels(data))
