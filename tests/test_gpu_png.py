"""
The PNG writer on the device (csrc/rfx_png.hip): rfx_png_encode_u8's stream bytes, lengths, CRCs and channel flags equal the host
emulator's (tests/emu/rfx_png_emu.cpp, pinned against zlib and Pillow by tests/test_png_cpu.py), byte for byte - at the sizes of
the CPU list with random and run-heavy contents, on a 512 x 512 golden tile in all three modes, on the stereo tile, in a batch
that mixes grey and colour tiles in mode auto, and in mode gray around a colour tile.  No byte past a stream's length is written.
spectrogram_images_from_waveforms(as_png=True) and the CLI's --png-writer device give files that reopen to the pixels and EXIF of
the host route's.
"""
import glob
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from png_cases import SIZES, STEREO_PNG, _tile, chunks, emu_stream

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _conv(stereo=False, **kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, **kw), device="cuda")


def device_streams(tiles, mode):
    """rfx_png_encode_u8 on (N, H, W, 3) tiles with buffers of its own -> (streams, CRCs, channels); the bytes after every
    stream's length, to the end of its capacity slot and in a band after the last slot, must still hold the guard value"""
    from riffusion import _hip

    lib = _hip.load_library()
    tiles = np.array(tiles, dtype=np.uint8)  # (a copy: the shared tiles are read-only, and torch takes no such array)
    N, H, W, _ = tiles.shape
    m = _hip.PNG_MODES[mode]
    cap = lib.rfx_png_stream_capacity(H, W, 1 if m == 1 else 3)
    need = lib.rfx_png_encode_workspace_bytes(N, H, W)
    assert cap > 0 and need > 0
    img = torch.from_numpy(tiles).cuda()
    out = torch.full((N * cap + 256,), GUARD, dtype=torch.uint8, device="cuda")
    meta = torch.full((3, N), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _hip.check(lib.rfx_png_encode_u8(img.data_ptr(), N, H, W, m, out.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(),
                                     ws.data_ptr(), _hip.current_stream(torch.device("cuda", 0))))
    meta, out = meta.cpu().numpy(), out.cpu().numpy()
    streams = []
    for n in range(N):
        size = int(meta[0, n])
        assert 0 <= size <= cap
        assert (out[n * cap + size:(n + 1) * cap] == GUARD).all(), n
        streams.append(out[n * cap:n * cap + size].tobytes())
    assert (out[N * cap:] == GUARD).all()
    return streams, [int(v) for v in meta[1].view(np.uint32)], [int(v) for v in meta[2]]


def check_against_emulator(tiles, mode):
    got = device_streams(tiles, mode)
    for n, tile in enumerate(tiles):
        stream, crc, ch, _ = emu_stream(tile, mode)
        assert got[2][n] == ch, (n, mode)
        assert got[1][n] == crc, (n, mode)
        assert len(got[0][n]) == len(stream) and got[0][n] == stream, (n, mode)
    return got


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("content", ["random", "runs"])
def test_streams_equal_the_emulator(content, h, w):
    tile = _tile(f"{content}_{h}x{w}")
    for mode in ("rgb", "auto"):
        check_against_emulator(tile[None], mode)
    grey = np.ascontiguousarray(np.repeat(tile[:, :, 1:2], 3, axis=2))
    for mode in ("gray", "auto", "rgb"):
        check_against_emulator(grey[None], mode)


def test_golden_mono_tile_in_all_modes():
    tile = _tile("agile.png")
    assert tile.shape == (512, 512, 3)
    for mode in ("rgb", "gray", "auto"):
        _, _, channels = check_against_emulator(tile[None], mode)
        assert channels == [3 if mode == "rgb" else 1]


def test_stereo_tile():
    tile = _tile(STEREO_PNG)
    assert tile.shape == (512, 568, 3)
    for mode in ("rgb", "auto"):
        assert check_against_emulator(tile[None], mode)[2] == [3]


def test_run_lengths_and_constant_tiles():
    for name in ("run_lengths", "zeros", "ones"):
        for mode in ("rgb", "gray", "auto"):
            check_against_emulator(_tile(name)[None], mode)


def test_tall_and_wide_tiles():
    """32801 x 1: 1026 blocks, more than the 1024 threads that add up the bit counts of the blocks before a block, and a row of
    2 or 4 bytes; 3 x 2999: rows of many rounds for the filter's 256 threads, one block of 27 rounds for the token walk"""
    rng = np.random.default_rng(77)
    tall = np.repeat(rng.integers(0, 3, size=(32801, 1, 1), dtype=np.uint8) * 100, 3, axis=2)
    tall[::7, 0, 1] ^= 1
    wide = np.repeat(np.repeat(rng.integers(0, 256, size=(3, 300, 3), dtype=np.uint8), 10, axis=1)[:, :2999], 1, axis=2)
    for tile in (np.ascontiguousarray(tall), np.ascontiguousarray(wide)):
        check_against_emulator(tile[None], "rgb")
        check_against_emulator(np.ascontiguousarray(np.repeat(tile[:, :, :1], 3, axis=2))[None], "auto")


def test_auto_batch_mixes_grey_and_colour():
    """five tiles of one size, grey and colour in turn: the row length, the block sizes and the stream differ per tile in one call"""
    h, w = 65, 171
    tiles = np.stack([_tile(f"random_{h}x{w}"), _tile("mono_noise"), _tile(f"runs_{h}x{w}"), np.zeros((h, w, 3), np.uint8),
                      np.ascontiguousarray(_tile(f"random_{h}x{w}")[::-1, ::-1])])
    assert check_against_emulator(tiles, "auto")[2] == [3, 1, 3, 1, 3]
    check_against_emulator(tiles, "rgb")


def test_gray_batch_flags_the_colour_tile_and_keeps_its_neighbours():
    h, w = 33, 50
    grey = [np.ascontiguousarray(np.repeat(_tile(f"{c}_{h}x{w}")[:, :, :1], 3, axis=2)) for c in ("random", "runs")]
    tiles = np.stack([grey[0], _tile(f"random_{h}x{w}"), grey[1]])
    streams, crcs, channels = check_against_emulator(tiles, "gray")
    assert channels == [1, 0, 1] and streams[1] == b"" and crcs[1] == 0
    conv = _conv()
    with pytest.raises(ValueError, match="tile 1 is not grey"):
        conv.png_bytes_from_images(tiles, mode="gray")
    files = conv.png_bytes_from_images(tiles, mode="auto")
    assert [Image.open(io.BytesIO(f)).mode for f in files] == ["L", "RGB", "L"]


def test_files_and_tiles_per_call():
    from riffusion.util import image_util

    conv = _conv(stereo=True)
    h, w = 70, 87
    tiles = np.stack([_tile(f"random_{h}x{w}"), _tile("zeros"), _tile(f"runs_{h}x{w}"), np.ascontiguousarray(_tile(f"runs_{h}x{w}")[::-1]),
                      np.ascontiguousarray(np.repeat(_tile(f"random_{h}x{w}")[:, :, 2:], 3, axis=2))])
    exifs = [conv.exif_with_max_value(v) for v in (1.0, 2.0, 2.5e7, 3.0e7, 7.0)]
    for mode in ("rgb", "auto"):
        files = conv.png_bytes_from_images(tiles, exif=exifs, mode=mode)
        assert conv.png_bytes_from_images(torch.from_numpy(tiles).cuda(), exif=exifs, mode=mode, tiles_per_call=2) == files
        for tile, exif, data in zip(tiles, exifs, files):
            stream, crc, ch, _ = emu_stream(tile, mode)
            assert data == image_util.png_file(w, h, ch, stream, crc, image_util.png_exif_bytes(exif))
            assert [k for k, _ in chunks(data)] == [b"IHDR", b"eXIf", b"IDAT", b"IEND"]  # (chunks checks every CRC)
            back = Image.open(io.BytesIO(data))
            assert np.array_equal(np.asarray(back), tile if ch == 3 else tile[:, :, 0]) and dict(back.getexif()) == dict(exif)
    assert conv.png_bytes_from_images(tiles, exif=exifs[1], tiles_per_call=1)[1] == conv.png_bytes_from_images(tiles, exif=exifs)[1]
    with pytest.raises(ValueError, match="EXIF"):
        conv.png_bytes_from_images(tiles, exif=exifs[:2])
    for kw in ({"optimize": True}, {"compress_level": 6}, {"compress_type": 3}, {"bits": 8}):
        with pytest.raises(ValueError, match="not implemented"):
            conv.png_bytes_from_images(tiles, **kw)
    with pytest.raises(ValueError, match="mode"):
        conv.png_bytes_from_images(tiles, mode="grey")


def test_waveforms_as_png_reopen_to_their_own_images(golden_dir):
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util.audio_util import PcmSegment

    conv = _conv(stereo=False)
    seg = PcmSegment.from_wav(os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav")).set_channels(1)
    wave = np.array([c.get_array_of_samples() for c in seg.split_to_mono()]).astype(np.float32)
    batch = torch.from_numpy(wave)[None]
    images, max_values = conv.spectrogram_images_from_waveforms(batch)
    for png_mode, want_mode in (("rgb", "RGB"), ("auto", "L"), ("gray", "L")):
        files, max_png = conv.spectrogram_images_from_waveforms(batch, as_png=True, png_mode=png_mode)
        assert np.array_equal(np.asarray(max_values).view(np.int32), np.asarray(max_png).view(np.int32)) and len(files) == 1
        back = Image.open(io.BytesIO(files[0]))
        assert back.mode == want_mode and back.size == images[0].size
        assert np.array_equal(np.asarray(back.convert("RGB")), np.asarray(images[0]))
        assert SpectrogramParams.from_exif(back.getexif()) == conv.p
        assert back.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] == float(max_values[0])
        assert dict(back.getexif()) == dict(conv.exif_with_max_value(max_values[0]))
    with pytest.raises(ValueError, match="return_device"):
        conv.spectrogram_images_from_waveforms(batch, return_device=True, as_png=True)
    with pytest.raises(ValueError, match="give one"):
        conv.spectrogram_images_from_waveforms(batch, as_jpeg=True, as_png=True)
    track = PcmSegment.from_wav(os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav"))
    starts = [0.0, 0.35]
    clip_images, clip_max = conv.spectrogram_images_from_audio_clips(track, starts, 2.0)
    clip_files, _ = conv.spectrogram_images_from_audio_clips(track, starts, 2.0, as_png=True, png_mode="auto")
    for image, mx, data in zip(clip_images, clip_max, clip_files):
        back = Image.open(io.BytesIO(data))
        assert np.array_equal(np.asarray(back.convert("RGB")), np.asarray(image))
        assert back.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] == float(mx)


def test_cli_device_writer_against_the_pillow_writer(tmp_path, golden_dir):
    import shutil

    from riffusion import cli

    wavs = sorted(glob.glob(os.path.join(golden_dir, "clip_*.wav")))
    audio_dir = tmp_path / "audio"
    audio_dir.mkdir()
    for w in wavs:
        shutil.copy(w, audio_dir)
    runs = {}
    for name, extra in (("pillow", {}), ("default", {"png_writer": "pillow", "png_mode": "rgb"}), ("device", {"png_writer": "device"}),
                        ("auto", {"png_writer": "device", "png_mode": "auto"})):
        out = tmp_path / name
        cli.audio_to_images_batch(audio_dir=str(audio_dir), output_dir=str(out), image_extension="png", batch_size=2, mono=name == "auto", **extra)
        runs[name] = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
        assert len(runs[name]) == len(wavs)
    assert runs["default"] == runs["pillow"]  # the defaults keep every byte
    for name, data in runs["device"].items():
        want, back = Image.open(io.BytesIO(runs["pillow"][name])), Image.open(io.BytesIO(data))
        assert back.mode == want.mode == "RGB" and np.array_equal(np.asarray(back), np.asarray(want))
        assert dict(back.getexif()) == dict(want.getexif())
        assert [k for k, _ in chunks(data)] == [b"IHDR", b"eXIf", b"IDAT", b"IEND"]
    assert all(Image.open(io.BytesIO(d)).mode == "L" for d in runs["auto"].values())
    # audio-to-image: one clip
    one, two = tmp_path / "one.png", tmp_path / "two.png"
    cli.main(["audio-to-image", "--audio", wavs[0], "--image", str(one)])
    cli.main(["audio-to-image", "--audio", wavs[0], "--image", str(two), "--png-writer", "device", "--png-mode", "auto"])
    a, b = Image.open(str(one)), Image.open(str(two))
    assert b.mode == "L" and np.array_equal(np.asarray(a), np.asarray(b.convert("RGB"))) and dict(a.getexif()) == dict(b.getexif())
    with pytest.raises(SystemExit):
        cli.main(["audio-to-image", "--audio", wavs[0], "--image", str(two), "--png-mode", "gray"])


def test_refusals_before_any_launch():
    from riffusion import _hip

    conv = _conv()
    lib = conv.converter._plan().lib
    img = torch.zeros((1, 1, 65536, 3), dtype=torch.uint8, device="cuda")
    small = torch.full((256,), 7, dtype=torch.uint8, device="cuda")
    meta = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    rc = lib.rfx_png_encode_u8(img.data_ptr(), 1, 1, 65536, 0, small.data_ptr(), meta[0:].data_ptr(), meta[1:].data_ptr(), meta[2:].data_ptr(),
                               small.data_ptr(), _hip.current_stream(torch.device("cuda", 0)))
    assert rc == -4 and b"65535" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((meta == -1).all()) and bool((small == 7).all())
    with pytest.raises(_hip.RfxError, match="65535"):
        conv.converter._plan().png_streams(img)
