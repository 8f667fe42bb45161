"""
CPU checks of the host side the JPEG and PNG file codecs share.  `images_from_jpeg_bytes` runs through a plan whose `jpeg_decode`
is the host emulator (tests/emu/rfx_jpeg_dec_emu.cpp, image by image), as `images_from_png_bytes` does in test_png_decode_cpu.py:
every tile and EXIF against `np.asarray(Image.open(f).convert("RGB"))` and `Image.open(f).getexif()`, byte for byte, no
tolerance - what can go wrong here is routing and indexing, not decoding.  Then the two numpy helpers of the bindings: the layout
of a decode's one upload (`_hip.pack_streams`) and the split of an encode's one download (`_hip.split_packed`).
"""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from jpeg_cases import _random
from jpeg_decode_cases import _emu, pillow_jpeg
from riffusion import _hip
from riffusion.spectrogram_image_converter import SpectrogramImageConverter
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import image_util


class EmuPlan:
    """Plan.jpeg_decode by the emulator, for images_from_jpeg_bytes without a GPU"""
    device = "cpu"

    def jpeg_decode(self, scans, H, W, qtables, huffman):
        qtables, huffman = np.ascontiguousarray(qtables, np.uint16), np.ascontiguousarray(huffman, np.uint8)
        assert qtables.shape == (len(scans), 2, 64) and huffman.shape == (len(scans), 4, 272)
        rgb = np.zeros((len(scans), H, W, 3), np.uint8)
        status, stats = np.zeros(len(scans), np.int32), np.zeros(4, np.int32)
        for n, data in enumerate(scans):
            scan = np.frombuffer(data, np.uint8).copy()
            status[n] = _emu().emu_jpeg_decode_u8(scan.ctypes.data, scan.size, H, W, qtables[n].ctypes.data, huffman[n].ctypes.data,
                                                  rgb[n].ctypes.data, stats.ctypes.data)
        return torch.from_numpy(rgb), status


def host_route(data):
    """(pixels, exif dict) as the host route gives them, or the exception's type"""
    try:
        with Image.open(io.BytesIO(data)) as im:
            return image_util.rgb_array_from_image(im), dict(im.getexif())
    except Exception as e:  # noqa: BLE001 - whatever Pillow raises is what the entry must raise
        return type(e)


@pytest.fixture
def conv(monkeypatch):
    conv = SpectrogramImageConverter(params=SpectrogramParams(), device="cuda")
    monkeypatch.setattr(conv.converter, "_plan", lambda: EmuPlan())
    return conv


def cut_scan(data, keep):
    """the file with only the first `keep` of its scan's bytes (headers and EOI stay: the device's to decode, and to report)"""
    info = image_util.jpeg_parse(data)
    return data[:info.scan[0]] + data[info.scan[0]:info.scan[1]][:int(keep * (info.scan[1] - info.scan[0]))] + data[info.scan[1]:]


def save(tile, fmt, **kw):
    buf = io.BytesIO()
    Image.fromarray(tile).save(buf, fmt, **kw)
    return buf.getvalue()


def test_three_files_of_one_size_come_back_as_one_batch(conv):
    files = [pillow_jpeg(_random(9, 21), q) for q in (30, 75, 95)]
    tiles, exifs = conv.images_from_jpeg_bytes(files)
    assert isinstance(tiles, np.ndarray) and tiles.shape == (3, 9, 21, 3) and tiles.dtype == np.uint8
    for data, tile, exif in zip(files, tiles, exifs):
        want = host_route(data)
        assert np.array_equal(tile, want[0]) and dict(exif) == want[1] == {}
    # one call that covers every file is the result as it is, in two calls the tiles are put together again: same bytes
    again, _ = conv.images_from_jpeg_bytes(files, tiles_per_call=2)
    assert isinstance(again, np.ndarray) and np.array_equal(again, tiles)


def test_mixed_list_goes_file_by_file_to_the_device_or_to_pillow(conv):
    small, square = pillow_jpeg(_random(5, 3), 75), pillow_jpeg(_random(16, 16), 90, optimize=True)
    progressive = pillow_jpeg(_random(16, 16), 75, progressive=True)
    grey = save(_random(5, 3)[..., 0], "JPEG")
    png = save(_random(7, 4), "PNG")
    cut = cut_scan(pillow_jpeg(_random(16, 16), 75), 0.5)
    files = [small, progressive, square, grey, png, cut, small, square]
    device = [image_util.jpeg_parse(f).ok_for_device for f in files]
    assert device == [True, False, True, False, False, True, True, True]
    info = image_util.jpeg_parse(cut)
    _, status = EmuPlan().jpeg_decode([cut[info.scan[0]:info.scan[1]]], 16, 16, info.qtables[None], info.huffman[None])
    assert status[0] != 0  # the device's to decode, Pillow's in the end
    tiles, exifs = conv.images_from_jpeg_bytes(files, tiles_per_call=1)
    assert isinstance(tiles, list) and len(tiles) == len(exifs) == len(files)
    for data, tile, exif in zip(files, tiles, exifs):
        want = host_route(data)
        assert not isinstance(want, type) and tile.dtype == np.uint8
        assert np.array_equal(tile, want[0]) and dict(exif) == want[1]
    # the same through calls of several files: the 16 x 16 group holds the damaged file between two good ones
    more, _ = conv.images_from_jpeg_bytes(files)
    assert all(np.array_equal(a, b) for a, b in zip(more, tiles))


def test_damage_pillow_cannot_read_raises_pillows_exception(conv):
    whole = pillow_jpeg(_random(16, 16), 75)
    for data in (whole[:-2], whole[:100], cut_scan(whole, 0.5)[:-2], b"", b"\xff\xd8" + bytes(40)):
        want = host_route(data)
        if isinstance(want, type):
            with pytest.raises(want):
                conv.images_from_jpeg_bytes([whole, data])
        else:
            tiles, exifs = conv.images_from_jpeg_bytes([whole, data])
            assert np.array_equal(tiles[1], want[0]) and dict(exifs[1]) == want[1]
    assert isinstance(host_route(b""), type) and isinstance(host_route(whole[:100]), type)


def test_file_with_the_spectrogram_exif(conv):
    params = SpectrogramParams(stereo=True)
    exif = Image.Exif()
    exif.update(params.to_exif().items())
    exif[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(np.float32(12345678.0))
    files = [pillow_jpeg(_random(12, 20), 75, exif=exif), pillow_jpeg(_random(12, 20), 75)]
    tiles, exifs = conv.images_from_jpeg_bytes(files)
    assert tiles.shape == (2, 12, 20, 3)
    for data, tile, got in zip(files, tiles, exifs):
        want = host_route(data)
        assert np.array_equal(tile, want[0]) and dict(got) == want[1]
    assert SpectrogramParams.from_exif(exifs[0]) == params and exifs[0][SpectrogramParams.ExifTags.MAX_VALUE.value] == 12345678.0
    assert dict(exifs[1]) == {}


def test_tiles_per_call_below_one_is_refused(conv):
    with pytest.raises(ValueError, match="tiles_per_call"):
        conv.images_from_jpeg_bytes([pillow_jpeg(_random(5, 3), 75)], tiles_per_call=0)
    assert conv.images_from_jpeg_bytes([]) == ([], [])


# ---- the bindings' numpy helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [[b"abc"], [b""], [b"\x01" * 17, b"", b"\x02\x03"], [b"", b"", b"x"]], ids=["one", "one_empty", "three", "three_two_empty"])
@pytest.mark.parametrize("tables", ["none", "jpeg", "png"])
def test_upload_layout(streams, tables):
    N = len(streams)
    rng = np.random.default_rng(N)
    arrays = {"none": [],
              "jpeg": [rng.integers(1, 256, (N, 2, 64)).astype(np.uint16), rng.integers(0, 256, (N, 4, 272)).astype(np.uint8)],
              "png": [rng.integers(0, 257, N).astype(np.int32), rng.integers(0, 256, (N, 768)).astype(np.uint8)]}[tables]
    host, offsets, at = _hip.pack_streams(streams, arrays)
    assert host.dtype == np.uint8 and host.ndim == 1 and offsets.dtype == np.int64
    assert offsets.tolist() == [sum(len(s) for s in streams[:n]) for n in range(N + 1)]
    # offsets at 0, the tables in order behind them, the streams on the next multiple of 16 and nothing after them
    assert len(at) == len(arrays) + 2 and at[0] == 0
    assert host[:8 * (N + 1)].tobytes() == offsets.tobytes()
    end = 8 * (N + 1)
    for a, table in zip(at[1:-1], arrays):
        assert a == end and host[a:a + table.nbytes].tobytes() == table.tobytes()
        end += table.nbytes
    assert at[-1] % 16 == 0 and 0 <= at[-1] - end < 16 and not host[end:at[-1]].any()
    assert host[at[-1]:].tobytes() == b"".join(streams) and host.size == at[-1] + int(offsets[-1])
    for n, s in enumerate(streams):
        assert host[at[-1] + offsets[n]:at[-1] + offsets[n + 1]].tobytes() == s


@pytest.mark.parametrize("parts", [[b"abc"], [b""], [b"ab", b"", b"cde"], [b"", b"", b""], []], ids=["one", "one_empty", "three", "all_empty", "none"])
def test_split_packed_gives_the_parts_back(parts):
    assert _hip.split_packed(b"".join(parts), [len(p) for p in parts]) == parts
