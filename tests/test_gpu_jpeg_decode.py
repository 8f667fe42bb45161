"""
The JPEG decoder on the device (csrc/rfx_jpeg_dec.hip): rfx_jpeg_decode_u8 and SpectrogramImageConverter.images_from_jpeg_bytes
equal `np.asarray(Image.open(f).convert("RGB"))` of the Pillow on this machine, byte for byte - batches of three different files
per call at sizes with dummy blocks, odd remainders and one pixel, with the standard and with optimised Huffman tables, tables
that differ inside a batch, the two full golden tiles; damaged scans give a status for their image alone and the others stay
exact; bad arguments are refused before anything is launched; the batch CLI's jpg grouping and loading give the tiles and params of
the Pillow loop.
"""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from jpeg_cases import CONTENTS, STEREO_PNG, _golden, _random
from jpeg_decode_cases import DAMAGE_TILES, _conv, _three, damaged_scans, pillow_jpeg, pillow_pixels

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (9, 17), (23, 37), (62, 33), (64, 96)]


def _decode(files):
    """the files of one size through Plan.jpeg_decode (the C ABI entry): (pixels as numpy, status)"""
    from riffusion.util import image_util

    plan = _conv().converter._plan()
    infos = [image_util.jpeg_parse(f) for f in files]
    assert all(i.ok_for_device for i in infos)
    rgb, status = plan.jpeg_decode([f[i.scan[0]:i.scan[1]] for f, i in zip(files, infos)], infos[0].height, infos[0].width,
                                   np.stack([i.qtables for i in infos]), np.stack([i.huffman for i in infos]))
    return rgb.cpu().numpy(), status


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("optimize", [False, True])
def test_batches_of_three_equal_pillow(h, w, optimize):
    for q in (1, 75, 100):
        files = [pillow_jpeg(t, q, optimize=optimize) for t in _three(h, w)]
        got, status = _decode(files)
        assert not status.any(), (q, status)
        for g, f in zip(got, files):
            assert np.array_equal(g, pillow_pixels(f)), (h, w, q, optimize)


def test_tables_that_differ_inside_a_batch():
    files = [pillow_jpeg(t, q, optimize=o) for t, q, o in zip(_three(62, 33), (1, 75, 100), (False, True, False))]
    got, status = _decode(files)
    assert not status.any()
    for g, f in zip(got, files):
        assert np.array_equal(g, pillow_pixels(f))


def test_full_golden_tiles():
    og, stereo = CONTENTS["og_beat"](), _golden(STEREO_PNG)[:, :512]
    files = [pillow_jpeg(og, 75), pillow_jpeg(stereo, 75), pillow_jpeg(og, 75, optimize=True)]
    got, status = _decode(files)
    assert got.shape == (3, 512, 512, 3) and not status.any()
    for g, f in zip(got, files):
        assert np.array_equal(g, pillow_pixels(f))


def test_images_from_jpeg_bytes_mixed_list_and_exif():
    from riffusion.spectrogram_params import SpectrogramParams

    conv = _conv(stereo=True)
    exif = conv.exif_with_max_value(12345678.0)
    files = [pillow_jpeg(_random(23, 37), 75, exif=exif), pillow_jpeg(_random(62, 33), 90), pillow_jpeg(_random(62, 33), 50, progressive=True),
             pillow_jpeg(_random(23, 37), 30, optimize=True)]
    want = [pillow_pixels(f) for f in files]
    tiles, exifs = conv.images_from_jpeg_bytes(files)
    assert isinstance(tiles, list) and len(tiles) == 4
    for t, w_ in zip(tiles, want):
        assert isinstance(t, np.ndarray) and np.array_equal(t, w_)
    dev, _ = conv.images_from_jpeg_bytes(files, return_device=True, tiles_per_call=1)
    assert all(t.is_cuda and np.array_equal(t.cpu().numpy(), w_) for t, w_ in zip(dev, want))
    assert SpectrogramParams.from_exif(exifs[0]) == conv.p and exifs[0][SpectrogramParams.ExifTags.MAX_VALUE.value] == 12345678.0
    assert all(isinstance(e, Image.Exif) for e in exifs) and not dict(exifs[1]) and not dict(exifs[2])
    # one size: one batch
    same, _ = conv.images_from_jpeg_bytes([files[0], files[3]])
    assert isinstance(same, np.ndarray) and same.shape == (2, 23, 37, 3) and np.array_equal(same[1], want[3])


def test_encoder_output_decodes_as_pillow_decodes_it():
    conv = _conv()
    x = np.stack([np.ascontiguousarray(_golden(STEREO_PNG)[200:264, 300:396]), _random(64, 96)])
    files = conv.jpeg_bytes_from_images(x, exif=conv.exif_with_max_value(5.0))
    tiles, exifs = conv.images_from_jpeg_bytes(files, return_device=True)
    assert isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.shape == (2, 64, 96, 3)
    for t, f in zip(tiles.cpu().numpy(), files):
        assert np.array_equal(t, pillow_pixels(f))
    assert [dict(e) for e in exifs] == [dict(Image.open(io.BytesIO(f)).getexif()) for f in files]


@pytest.mark.parametrize("name", sorted(DAMAGE_TILES))
def test_damaged_scans_flag_their_image_only(name):
    """the truncated, flipped and 0xFF-tailed scans of tests/test_jpeg_decode_cpu.py between two sound images of the same size"""
    from riffusion.util import image_util

    tile = CONTENTS[name]()
    good = pillow_jpeg(tile, DAMAGE_TILES[name])
    other = pillow_jpeg(np.ascontiguousarray(tile[::-1] ^ 0x33), 60, optimize=True)
    info, info_o = image_util.jpeg_parse(good), image_util.jpeg_parse(other)
    scan = good[info.scan[0]:info.scan[1]]
    plan = _conv().converter._plan()
    for what, bad in damaged_scans(scan).items():
        rgb, status = plan.jpeg_decode([other[info_o.scan[0]:info_o.scan[1]], bad, scan], info.height, info.width,
                                       np.stack([info_o.qtables, info.qtables, info.qtables]), np.stack([info_o.huffman, info.huffman, info.huffman]))
        print(name, what, "status", status)
        assert status[0] == 0 and status[1] != 0 and status[2] == 0, what
        rgb = rgb.cpu().numpy()
        assert np.array_equal(rgb[0], pillow_pixels(other)) and np.array_equal(rgb[2], pillow_pixels(good)), what


def test_images_from_jpeg_bytes_on_damaged_files_behaves_as_pillow():
    from riffusion.util import image_util

    conv = _conv()
    good = pillow_jpeg(CONTENTS["random_32x40"](), 75)
    info = image_util.jpeg_parse(good)
    scan = good[info.scan[0]:info.scan[1]]
    for what, bad in damaged_scans(scan).items():
        data = good[:info.scan[0]] + bad + b"\xff\xd9"
        try:
            want = pillow_pixels(data)
        except Exception as e:  # Pillow refuses the file: so does the entry, with Pillow's exception
            with pytest.raises(type(e)):
                conv.images_from_jpeg_bytes([good, data])
            continue
        tiles, _ = conv.images_from_jpeg_bytes([good, data])
        assert np.array_equal(tiles[0], pillow_pixels(good)) and np.array_equal(tiles[1], want), what


def test_bad_arguments_are_refused_before_launch():
    from riffusion import _hip

    lib = _hip.load_library()
    assert lib.rfx_jpeg_decode_workspace_bytes(1, 65536, 8, 100) == 0 and lib.rfx_jpeg_decode_workspace_bytes(1, 8, 65536, 100) == 0
    assert lib.rfx_jpeg_decode_workspace_bytes(0, 8, 8, 100) == 0 and lib.rfx_jpeg_decode_workspace_bytes(1, 0, 8, 100) == 0
    assert lib.rfx_jpeg_decode_workspace_bytes(3, 512, 501, 100000) > 3 * 6 * 32 * 32 * 128
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    off = np.array([0, 10], np.int64)

    def call(N, H, W, offsets=off, scans=p):
        return lib.rfx_jpeg_decode_u8(scans, offsets.ctypes.data, p + 2048, N, H, W, p + 1024, p + 1024, p + 512, p + 3072, p, None)

    assert call(1, 65536, 8) == -4 and b"65535" in lib.rfx_last_error()  # RFX_ERR_UNSUPPORTED
    assert call(1, 8, 65536) == -4
    assert call(0, 8, 8) == -1 and call(1, 0, 8) == -1  # RFX_ERR_INVALID
    assert call(1, 8, 8, offsets=np.array([10, 0], np.int64)) == -1
    assert call(1, 8, 8, scans=p + 8) == -1 and b"16 bytes" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert not buf.any()  # nothing ran
    with pytest.raises(_hip.RfxError):
        _conv().converter._plan().jpeg_decode([b"\0"], 8, 65536, np.ones((1, 2, 64)), np.zeros((1, 4, 272)))


def test_cli_jpg_loading_equals_the_pillow_loop(tmp_path):
    from riffusion import cli
    from riffusion.util import image_util

    mono, stereo = _conv(), _conv(stereo=True)
    tiles = {"a": (mono, _random(64, 96)), "b": (mono, _three(64, 96)[1]), "c": (stereo, _random(64, 96) // 2), "d": (mono, _random(32, 40))}
    for name, (conv, t) in tiles.items():
        image = Image.fromarray(t)
        image.getexif().update(dict(conv.exif_with_max_value(3.0 + len(name))).items())
        image.save(os.path.join(tmp_path, name + ".jpg"), exif=image.getexif(), format="JPEG")
        image.save(os.path.join(tmp_path, name + ".png"), exif=image.getexif(), format="PNG")
    Image.fromarray(_random(32, 40)).save(os.path.join(tmp_path, "e.jpg"), format="JPEG", progressive=True)  # no EXIF, host route

    def pillow_groups(ext):
        """the loop of images_to_audio_batch before it read jpg"""
        groups = {}
        for path in sorted(str(p) for p in tmp_path.glob("*." + ext)):
            with Image.open(path) as im:
                groups.setdefault((cli._params_from_image(im), im.size), []).append(path)
        out = {}
        for key, members in groups.items():
            stack = []
            for p in members:
                with Image.open(p) as im:
                    stack.append(image_util.rgb_array_from_image(im))
            out[key] = (members, np.stack(stack))
        return out

    want = pillow_groups("jpg")
    got = cli._tile_groups(sorted(str(p) for p in tmp_path.glob("*.jpg")), "jpg")
    assert {k: v for k, v in got.items()} == {k: v[0] for k, v in want.items()} and len(got) == 3
    for key, members in got.items():
        conv = _conv(stereo=key[0].stereo)
        loaded = cli._load_tiles(conv, members, "jpg")
        assert np.array_equal(torch.as_tensor(loaded).cpu().numpy(), want[key][1])
        # ... and the device decode of the same files, with the params of the group from their EXIF
        on_device, exifs = conv.images_from_jpeg_bytes([open(m, "rb").read() for m in members], return_device=True)
        assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), want[key][1])
        assert all(cli.SpectrogramParams.from_exif(e) == key[0] for e in exifs if dict(e))
    # png: the old loading, on the host
    want_png = pillow_groups("png")
    got_png = cli._tile_groups(sorted(str(p) for p in tmp_path.glob("*.png")), "png")
    assert got_png == {k: v[0] for k, v in want_png.items()}
    for key, members in got_png.items():
        loaded = cli._load_tiles(mono, members, "png")
        assert isinstance(loaded, np.ndarray) and np.array_equal(loaded, want_png[key][1])
