"""
The JPEG decoder's packed batch on the CPU: the cases of tests/test_gpu_jpeg_decode_seams.py - files from tests/jpeg_scan_writer.py
whose codewords, stuffed bytes and scan ends fall on the seams of the kernels (16-byte chunks shared by images, the 1024-chunk pass
of the unstuff scan, subsequences, groups, the 1024-MCU pass of the DC scan) - through emu_jpeg_decode_batch, which indexes stages
1 and 2 as the kernels do, as a shared library and as the stand-alone sanitizer program.  Statuses are the expected ones, pixels
equal the single-image emulator's of every scan decoded alone, and the coefficients, lengths and unstuffed bytes in the emulated
workspace equal what the writer wrote.  Every case asserts, from the writer's log or from the bytes, that it reaches its edge.
The writer itself is checked first: Pillow opens its picture files and the single-image emulator returns Pillow's pixels.
The large cases L1-L6 are the CPU twins of tests/test_gpu_jpeg_decode_large.py: scans longer than one trip of the copy kernel's
grid and than eight entropy groups, 64 images in one call, bad Huffman tables, the refusals before launch, the workspace's
previous contents.  Their builders assert their edges here, where no GPU is needed, and print what they reach.
"""
import numpy as np
import pytest

import jpeg_scan_writer as jw
from jpeg_cases import CONTENTS, STEREO_PNG, _golden
from jpeg_decode_batch_cases import (ANNEX_K, BUILDERS, Case, L3_PLACES, LARGE, MAX_SCAN_BYTES, ONES, Q75, STRESS, alone, build_case, build_large,
                                     check_stages, emu, emu_batch, emulator_blocks, layout, one_image, reach, sanitized_batch, written)
from jpeg_decode_cases import emu_decode, pillow_pixels
from riffusion.util import image_util


# ---- the writer, before it is a reference -----------------------------------------------------------------------------------------
PICTURES = {"stereo_crop_64x96": lambda: _golden(STEREO_PNG)[200:264, 300:396], "og_beat_crop_23x37": lambda: CONTENTS["og_beat"]()[40:63, 100:137],
            "stereo_crop_9x17": lambda: _golden(STEREO_PNG)[300:309, 17:34], "og_beat_crop_128x80": lambda: CONTENTS["og_beat"]()[256:384, 200:280]}


@pytest.mark.parametrize("name", sorted(PICTURES))
@pytest.mark.parametrize("tables", ["annex_k", "stress"])
def test_pillow_and_the_emulator_decode_the_writers_pictures(name, tables):
    tile = np.ascontiguousarray(PICTURES[name]())
    blocks = jw.picture_blocks(tile, Q75())
    data, log = jw.write_jpeg(blocks, tile.shape[0], tile.shape[1], Q75(), ANNEX_K if tables == "annex_k" else STRESS)
    want = pillow_pixels(data)
    assert want.shape == tile.shape and np.abs(want.astype(int) - tile).mean() < 12  # the picture, not noise
    info = image_util.jpeg_parse(data)
    assert info.ok_for_device and data[info.scan[0]:info.scan[1]] == log.scan and np.array_equal(info.qtables, Q75())
    status, got, _, _ = emu_decode(data)
    assert status == 0 and np.array_equal(got, want)
    assert log.unstuffed.replace(b"\xff", b"\xff\x00") == log.scan and 0 <= 8 * len(log.unstuffed) - log.total_bits < 8


def test_the_writer_refuses_values_outside_baseline():
    blocks = np.zeros((6, 64), np.int64)
    for at, value in ((0, 2048), (0, -2048), (5, 1024), (63, -1024)):
        bad = blocks.copy()
        bad[2, at] = value
        with pytest.raises(ValueError):
            jw.write_jpeg(bad, 16, 16, Q75(), ANNEX_K)
    blocks[2, 0], blocks[3, 0], blocks[2, 5] = 1023, -1024, -1023  # differences of +1023, -2047
    jw.write_jpeg(blocks, 16, 16, Q75(), ANNEX_K)


def test_the_stress_tables_are_what_the_cases_need():
    for tables in (STRESS, ONES, ANNEX_K):
        for t in tables:
            jw.canonical_codes(t)  # a prefix code
    dc, ac = jw.canonical_codes(STRESS[0]), jw.canonical_codes(STRESS[1])
    assert ac[0xFA][1] == 16 and ac[0x0A][1] == 16 and dc[11][1] == 16 == max(length for _, length in dc.values())
    lengths = {length for _, length in ac.values()}
    assert 9 in lengths and 10 in lengths
    # the decoder's derivation accepts them: an EOB-only image decodes with status 0
    for tables in (STRESS, ONES):
        img, _ = written(np.zeros((6, 64), np.int64), 16, 16, tables)
        assert alone(img.scan, 16, 16, img.qtables.tobytes(), tables.tobytes())[0] == 0


# ---- the batch path ---------------------------------------------------------------------------------------------------------------
def check_on_the_emulator(c: Case, tmp_path):
    """the case through the batch emulator and the sanitizer program: statuses, stages, pixels"""
    name = c.name
    for who, got in (("emulator", emu_batch(c)), ("sanitizer program", sanitized_batch(c, str(tmp_path)))):
        assert got.status.tolist() == c.status, (name, who)
        check_stages(c, got, who=who)
        for n, scan in enumerate(c.scans):
            status, want = alone(scan, c.H, c.W, c.qtables[n].tobytes(), c.huffman[n].tobytes())
            assert status == c.status[n], (name, n)
            if status == 0:
                assert np.array_equal(got.rgb[n], want), (name, who, n)
                if c.files[n] is not None:
                    assert np.array_equal(want, pillow_pixels(c.files[n])), (name, n)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_batch_emulation_equals_the_writer_and_the_single_image_emulator(name, tmp_path):
    check_on_the_emulator(build_case(name), tmp_path)


@pytest.mark.parametrize("off0", [16, 5, 37])
def test_first_offset_changes_nothing(off0):
    base, moved = emu_batch(build_case("U4_0")), emu_batch(build_case(f"U4_{off0}"))
    assert np.array_equal(base.status, moved.status) and np.array_equal(base.rgb, moved.rgb)


# ---- the large cases (tests/test_gpu_jpeg_decode_large.py runs the same ones on the device) ---------------------------------------
@pytest.mark.parametrize("name", list(LARGE))
def test_large_cases_on_the_emulator(name, tmp_path):
    """L1, L2, L4, S1: statuses as the case says, the unstuffed bytes and the writer's coefficients, pixels as Pillow's (stress
    images: as the single-image emulator's)"""
    c = build_large(name)
    reach(c)
    check_on_the_emulator(c, tmp_path)
    host = emu_batch(c)
    ref = emulator_blocks(c, host)  # (what the device's coefficients of Pillow's files are compared with)
    assert all(b is not None for b, s in zip(ref.blocks, c.status) if s == 0)
    check_stages(ref, host, stages=("coef",))


def test_l3_an_image_decodes_the_same_alone_and_at_any_place_of_64():
    c = build_large("L3")
    reach(c)
    whole = emu_batch(c)
    assert np.flatnonzero(whole.status).tolist() == list(L3_PLACES), whole.status
    for n in range(64):
        single = emu_batch(one_image(c, n))
        assert whole.status[n] == single.status[0] and np.array_equal(whole.rgb[n], single.rgb[0]), n
        if n not in L3_PLACES:
            assert np.array_equal(whole.rgb[n], pillow_pixels(c.files[n])), n
    print("L3: statuses of the damaged scans:", whole.status[list(L3_PLACES)])


def test_l5_refusals_before_anything_is_read():
    """the emulator's entry refuses a scan of kJpdMaxScanBytes + 1 as the device's does, and the layout takes kJpdMaxScanBytes"""
    canary = np.full(64, 0x5C, np.uint8)
    buffers = [canary.copy() for _ in range(5)]
    off = np.array([0, MAX_SCAN_BYTES + 1], np.int64)
    rc = emu().emu_jpeg_decode_batch(buffers[0].ctypes.data, off.ctypes.data, 1, 8, 8, buffers[1].ctypes.data, buffers[1].ctypes.data,
                                     buffers[2].ctypes.data, buffers[3].ctypes.data, buffers[4].ctypes.data)
    assert rc == -1 and all(np.array_equal(b, canary) for b in buffers)
    assert layout(1, 8, 8, MAX_SCAN_BYTES).total > MAX_SCAN_BYTES


def test_l6_the_workspace_s_previous_contents_change_nothing():
    c = build_large("L3_sound")
    a, b = emu_batch(c, fill=0xA5), emu_batch(c, fill=0x00)
    assert not a.status.any() and np.array_equal(a.status, b.status) and np.array_equal(a.rgb, b.rgb)
    for n in range(64):
        assert np.array_equal(a.rgb[n], pillow_pixels(c.files[n])), n
