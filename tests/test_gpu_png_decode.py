"""
The PNG decoder on the device (csrc/rfx_png_dec.hip): rfx_png_decode_u8 through Plan.png_decode and
SpectrogramImageConverter.images_from_png_bytes equal the host emulator of the same code and
`np.asarray(Image.open(f).convert("RGB"))` of the Pillow on this machine, byte for byte - the ten golden files (the only full-size
inputs), Pillow's saves of small tiles in every mode and block kind, the device writer's files, the hand-built streams and filter
rows of tests/png_decode_cases.py, one call per (size, colour type); an image alone equals the image anywhere in batches of 3, 64
and 65 mixed streams; the damaged streams the sanitized emulator runs clean get the same statuses, beside good images that stay
exact; files the device does not read come back as the host route gives them; bad arguments are refused before anything is
launched; the batch CLI writes the same WAV bytes with either reader.
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_cases as C
from riffusion.util import image_util

pytestmark = pytest.mark.gpu


def _conv(**kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(**kw), device="cuda")


def _plan():
    return _conv().converter._plan()


def check_against_emulator_and_pillow(files):
    got = C.decode_files(_plan().png_decode, files)
    emu = C.decode_files(C.emu_decode, files)
    for name, data in files:
        assert got[name][0] == 0 == emu[name][0], (name, got[name][0], emu[name][0])
        assert np.array_equal(got[name][1], emu[name][1]), name
        assert np.array_equal(got[name][1], C.pillow_pixels(data)), name


def test_golden_files():
    check_against_emulator_and_pillow(C.golden_files())


def test_pillow_saves():
    check_against_emulator_and_pillow(C.pillow_saves())


def test_hand_built_streams_and_filters():
    check_against_emulator_and_pillow(C.hand_built() + C.filter_files())


def test_device_writer_files_come_back():
    conv = _conv()
    tile = C._golden_crop(70, 87)
    grey = np.repeat(tile[:, :, :1], 3, axis=2)
    files = conv.png_bytes_from_images(np.stack([tile, grey]), mode="rgb") + conv.png_bytes_from_images(np.stack([grey, tile]), mode="auto")
    check_against_emulator_and_pillow([(str(i), f) for i, f in enumerate(files)])
    tiles, _ = conv.images_from_png_bytes(files)
    assert np.array_equal(tiles, np.stack([tile, grey, grey, tile]))


def test_batch_invariance():
    """33 x 50 RGB streams of every block kind, mixed: an image alone equals the image at any place of a batch of 3, 64 and 65"""
    rng = np.random.default_rng(5)
    streams = []
    for k in range(65):
        tile = (C._golden_crop, C._random, C._runs)[k % 3](33, 50)
        tile = np.roll(tile, k, axis=1)
        data = C.pillow_png(Image.fromarray(tile), **list(C.SAVE_OPTIONS.values())[k % len(C.SAVE_OPTIONS)])
        streams.append(C.parts_of(data)[1])
    plan = _plan()
    alone = [plan.png_decode([s], 33, 50, 2)[0][0].cpu().numpy() for s in (streams[0], streams[1], streams[63], streams[64])]
    for n in (3, 64, 65):
        order = rng.permutation(n)
        rgb, status = plan.png_decode([streams[i] for i in order], 33, 50, 2)
        rgb = rgb.cpu().numpy()
        assert not status.any()
        want, _ = C.emu_decode([streams[i] for i in order], 33, 50, 2)
        assert np.array_equal(rgb, want)
        for which, i in enumerate((0, 1, 63, 64)):
            if i < n:
                assert np.array_equal(rgb[list(order).index(i)], alone[which]), (n, i)


def test_damaged_streams_flag_their_image_only():
    cases = C.damaged()
    good = cases[0][1]
    streams = [good] + [s for _, s, _ in cases] + [good]
    rgb, status = _plan().png_decode(streams, C.DAMAGE_H, C.DAMAGE_W, 2)
    rgb = rgb.cpu().numpy()
    want = C.pillow_pixels(C.damaged_file(good))
    assert status[0] == 0 and status[-1] == 0 and np.array_equal(rgb[0], want) and np.array_equal(rgb[-1], want)
    for (name, _, expected), got in zip(cases, status[1:-1]):
        assert got == expected, (name, got, expected)
    _, stream, pal, entries = C.palette_damage()
    rgb, status = _plan().png_decode([stream, stream], 2, 3, 3, np.stack([pal, pal]), [entries, entries + 1])
    assert list(status) == [12, 0]
    assert np.array_equal(rgb[1].cpu().numpy(), C.emu_decode([stream], 2, 3, 3, pal[None], [entries + 1])[0][0])


def _host(data):
    import io

    with Image.open(io.BytesIO(data)) as im:
        return image_util.rgb_array_from_image(im), dict(im.getexif())


def test_images_from_png_bytes_mixed_list_and_return_device():
    conv = _conv()
    golden = dict(C.golden_files())
    rgb16, interlaced, jpeg = C.host_only_files()
    damaged = C.damaged_file(dict((n, s) for n, s, _ in C.damaged())["left_over_byte"])
    files = [golden["og_beat_64.png"], C.pillow_saves()[5][1], rgb16, interlaced, jpeg, damaged, golden["og_beat_64.png"]]
    tiles, exifs = conv.images_from_png_bytes(files, tiles_per_call=1)
    on_device, _ = conv.images_from_png_bytes(files, return_device=True)
    assert isinstance(tiles, list) and len(tiles) == len(files)
    for data, tile, dev, exif in zip(files, tiles, on_device, exifs):
        want = _host(data)
        assert np.array_equal(tile, want[0]) and dict(exif) == want[1]
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want[0])
    same = [golden["agile.png"], golden["marim.png"], golden["og_beat.png"]]  # grey, grey, palette: one size, two calls, one batch
    batch, exifs = conv.images_from_png_bytes(same, return_device=True)
    assert batch.is_cuda and tuple(batch.shape) == (3, 512, 512, 3)
    for data, tile, exif in zip(same, batch.cpu().numpy(), exifs):
        assert np.array_equal(tile, _host(data)[0]) and dict(exif) == _host(data)[1]
    with pytest.raises(OSError):
        conv.images_from_png_bytes([C.damaged_file(dict((n, s) for n, s, _ in C.damaged())["adler_flipped"])])


def test_bad_arguments_are_refused_before_launch():
    from riffusion import _hip

    lib = _hip.load_library()
    q = lib.rfx_png_decode_workspace_bytes
    assert q(1, 65536, 8, 2, 100) == 0 and q(1, 8, 65536, 2, 100) == 0 and q(0, 8, 8, 2, 100) == 0 and q(1, 0, 8, 2, 100) == 0
    assert q(1, 8, 8, 4, 100) == 0 and q(1, 8, 8, 1, 100) == 0 and q(1, 8, 8, 2, (1 << 28) + 5) == 0
    assert q(2**31 - 1, 65535, 65535, 6, 100) == 0  # more filtered bytes than a launch indexes
    assert q(3, 512, 501, 2, 100000) == 3 * ((512 * (501 * 3 + 1) + 255) // 256 * 256)
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    off = np.array([0, 10], np.int64)

    def call(N, H, W, ct=2, offsets=off, streams=p, palettes=None):
        return lib.rfx_png_decode_u8(streams, offsets.ctypes.data, p + 2048, N, H, W, ct, palettes, palettes, p + 1024, p + 3072, p + 4096, None)

    assert call(1, 65536, 8) == -4 and b"65535" in lib.rfx_last_error()  # RFX_ERR_UNSUPPORTED
    assert call(1, 8, 65536) == -4
    assert call(1, 8, 8, offsets=np.array([0, 1 << 28], np.int64)) == -4 and b"2^28" in lib.rfx_last_error()
    assert call(0, 8, 8) == -1 and call(1, 0, 8) == -1 and call(1, 8, 8, ct=4) == -1  # RFX_ERR_INVALID
    assert call(1, 8, 8, offsets=np.array([10, 0], np.int64)) == -1
    assert call(1, 8, 8, ct=3) == -1  # no palette
    assert call(1, 8, 8, streams=p + 8) == -1 and b"16 bytes" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert not buf.any()  # nothing ran
    with pytest.raises(_hip.RfxError):
        _plan().png_decode([b"\0"], 8, 65536, 2)


def test_batch_cli_writes_the_same_wavs_with_either_reader(tmp_path):
    from riffusion import cli

    tiles = tmp_path / "tiles"
    tiles.mkdir()
    with Image.open(os.path.join(C.GOLDEN, "og_beat_64.png")) as im:
        exif = im.getexif()
        base = np.asarray(im.convert("RGB"))
    stereo = np.asarray(Image.open(os.path.join(C.GOLDEN, "clip_2_start_103694_ms_duration_5678_ms.png")).convert("RGB"))
    Image.fromarray(base).save(tiles / "a.png", exif=exif)
    Image.fromarray(base[:, ::-1]).convert("L").save(tiles / "b.png", exif=exif)
    Image.fromarray(np.ascontiguousarray(stereo[:, 100:164])).save(tiles / "c.png", exif=exif, optimize=True)
    Image.fromarray(np.ascontiguousarray(stereo[:, 300:364])).quantize(200).save(tiles / "d.png", exif=exif)
    for reader in ("pillow", "device"):
        torch.manual_seed(7)  # the decode draws its seed from torch's global generator
        cli.images_to_audio_batch(image_dir=str(tiles), output_dir=str(tmp_path / reader), griffin_lim_iters=2, png_reader=reader)
    names = sorted(os.listdir(tmp_path / "pillow"))
    assert names == ["a.wav", "b.wav", "c.wav", "d.wav"] == sorted(os.listdir(tmp_path / "device"))
    for n in names:
        assert (tmp_path / "pillow" / n).read_bytes() == (tmp_path / "device" / n).read_bytes(), n
