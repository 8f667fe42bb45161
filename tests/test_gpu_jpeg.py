"""
The JPEG encoder on the device (csrc/rfx_jpeg.hip): SpectrogramImageConverter.jpeg_bytes_from_images equals the file Pillow
writes on this machine - `Image.fromarray(t).save(f, "JPEG", quality=q[, exif=e])` - byte for byte, for the sizes and contents of
tests/test_jpeg_cpu.py alone and in a batch of three, for 64 full tiles in one call and for 512 x 501 tiles;
spectrogram_images_from_waveforms(as_jpeg=True) and the batch CLI write the files the Pillow save of the host route wrote; the
scan sizes stay inside rfx_jpeg_scan_capacity; bad arguments are refused before anything is launched.
"""
import glob
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import synthetic_tiles_u8
from jpeg_cases import CONTENTS, QUALITIES, pillow_file

pytestmark = pytest.mark.gpu


def _conv(stereo=False, **kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, **kw), device="cuda")


def _golden_waves(golden_dir):
    """the three golden clips as (C, samples) float32 at int16 scale, stereo"""
    from riffusion.util.audio_util import PcmSegment

    wavs = sorted(glob.glob(os.path.join(golden_dir, "clip_*.wav")))
    assert len(wavs) == 3
    out = []
    for w in wavs:
        seg = PcmSegment.from_wav(w).set_channels(2)
        assert seg.frame_rate == 44100
        out.append(np.array([c.get_array_of_samples() for c in seg.split_to_mono()]).astype(np.float32))
    return wavs, out


@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_files_equal_pillow_alone_and_in_a_batch_of_three(name):
    conv = _conv()
    tile = np.ascontiguousarray(CONTENTS[name]())
    other = np.ascontiguousarray(tile[::-1, ::-1] ^ 0x5A)  # the batch's last image is other content: offsets and sizes per image
    batch = np.stack([tile, tile, other])
    for q in QUALITIES:
        want, want_other = pillow_file(tile, q), pillow_file(other, q)
        assert want != want_other or tile.shape[:2] == (1, 1)
        one = conv.jpeg_bytes_from_images(tile[None], quality=q)
        assert isinstance(one, list) and len(one) == 1 and isinstance(one[0], bytes)
        assert one[0] == want, (name, q)
        three = conv.jpeg_bytes_from_images(torch.from_numpy(batch).cuda(), quality=q)  # a device tensor gives the same bytes
        assert three == [want, want, want_other], (name, q)
    assert conv.jpeg_bytes_from_images(batch, quality=75) == [pillow_file(t, 75) for t in batch]


def test_64_full_tiles_in_one_call():
    conv = _conv()
    tiles = synthetic_tiles_u8(64)
    files = conv.jpeg_bytes_from_images(tiles)
    assert len(files) == 64
    for t, f in zip(tiles, files):
        assert f == pillow_file(t, 75)
    # ... and the same tiles a few at a time: a tile's bytes do not depend on the batch it travels in
    assert conv.jpeg_bytes_from_images(tiles[:7], tiles_per_call=3) == files[:7]


def test_three_tiles_of_512_by_501():
    conv = _conv()
    tiles = synthetic_tiles_u8(3, 512, 501, seed=11)
    tiles[1, :, :, 0] = 0  # a stereo-like tile
    tiles[2] = np.repeat(tiles[2][:, :, :1] // 3, 3, axis=2)
    assert conv.jpeg_bytes_from_images(tiles, quality=95) == [pillow_file(t, 95) for t in tiles]


def test_exif_one_for_all_and_one_per_tile():
    conv = _conv(stereo=True)
    tiles = synthetic_tiles_u8(3, 40, 56, seed=3)
    exifs = [conv.exif_with_max_value(v) for v in (1.0, 2.5e7, 3.0e7)]
    assert conv.jpeg_bytes_from_images(tiles, exif=exifs) == [pillow_file(t, 75, e) for t, e in zip(tiles, exifs)]
    assert conv.jpeg_bytes_from_images(tiles, exif=exifs[1]) == [pillow_file(t, 75, exifs[1]) for t in tiles]
    with pytest.raises(ValueError, match="EXIF"):
        conv.jpeg_bytes_from_images(tiles, exif=exifs[:2])


def test_scan_sizes_stay_inside_the_capacity_and_nothing_past_them_is_returned():
    from riffusion import _hip

    conv = _conv()
    plan = conv.converter._plan()
    lib = plan.lib
    # the 1-pixel checkerboard at quality 100 is the longest scan a tile of its size gets here; noise is close
    tiles = np.stack([CONTENTS["checkerboard"](), synthetic_tiles_u8(1, 40, 56, seed=5)[0], np.zeros((40, 56, 3), np.uint8)])
    N, H, W, _ = tiles.shape
    cap = lib.rfx_jpeg_scan_capacity(H, W)
    need = lib.rfx_jpeg_encode_workspace_bytes(N, H, W)
    assert cap > 0 and need > 0
    qt = torch.from_numpy(_hip.jpeg_quant_tables(100).view(np.int16)).cuda()
    img = torch.from_numpy(tiles).cuda()
    scan = torch.full((N, cap), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(N, dtype=torch.int32, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _hip.check(lib.rfx_jpeg_encode_u8(img.data_ptr(), N, H, W, qt.data_ptr(), scan.data_ptr(), sizes.data_ptr(), ws.data_ptr(),
                                      _hip.current_stream(plan.device)))
    sizes, scan = sizes.cpu().numpy(), scan.cpu().numpy()
    files = conv.jpeg_bytes_from_images(tiles, quality=100)
    for n in range(N):
        assert 2 <= sizes[n] <= cap
        assert (scan[n, sizes[n]:] == 0xA5).all()  # the bytes past an image's size are not written ...
        assert files[n].endswith(scan[n, :sizes[n]].tobytes()) and files[n] == pillow_file(tiles[n], 100)  # ... and not returned
        assert len(files[n]) == len(_header(W, H, 100)) + sizes[n]


def _header(W, H, q):
    from riffusion.util import image_util

    return image_util.jpeg_header(W, H, q)


def test_waveforms_as_jpeg_equal_pillow_on_their_own_images(golden_dir):
    from riffusion.spectrogram_params import SpectrogramParams

    conv = _conv(stereo=True)
    _, waves = _golden_waves(golden_dir)
    lengths = sorted({w.shape[1] for w in waves})
    for length in lengths:  # (the golden clips are of two lengths, a sample apart: one call per length, as the CLI groups them)
        batch = torch.from_numpy(np.stack([w for w in waves if w.shape[1] == length]))
        images, max_values = conv.spectrogram_images_from_waveforms(batch)
        files, max_jpeg = conv.spectrogram_images_from_waveforms(batch, as_jpeg=True)
        assert np.array_equal(np.asarray(max_values).view(np.int32), np.asarray(max_jpeg).view(np.int32))
        assert len(files) == len(batch)
        for image, mx, data in zip(images, max_values, files):
            exif_data = conv.p.to_exif()
            exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(mx)
            image.getexif().update(exif_data.items())
            buf = io.BytesIO()
            image.save(buf, exif=image.getexif(), format="JPEG")
            assert data == buf.getvalue()
            back = Image.open(io.BytesIO(data))
            assert back.size == image.size and back.mode == "RGB"
            assert SpectrogramParams.from_exif(back.getexif()) == conv.p
            assert back.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] == float(mx)
    assert sum(w.shape[1] == lengths[0] for w in waves) + sum(w.shape[1] == lengths[-1] for w in waves) >= 3
    with pytest.raises(ValueError, match="return_device"):
        conv.spectrogram_images_from_waveforms(batch, return_device=True, as_jpeg=True)


def test_audio_clips_as_jpeg_equal_pillow_on_their_own_images(golden_dir):
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util.audio_util import PcmSegment

    conv = _conv(stereo=True)
    wavs, _ = _golden_waves(golden_dir)
    track = PcmSegment.from_wav(wavs[0])
    starts = [0.0, 0.35, 2.2]
    images, max_values = conv.spectrogram_images_from_audio_clips(track, starts, 2.0)
    files, max_jpeg = conv.spectrogram_images_from_audio_clips(track, starts, 2.0, as_jpeg=True)
    assert np.array_equal(np.asarray(max_values), np.asarray(max_jpeg)) and len(files) == len(starts)
    for image, mx, data in zip(images, max_values, files):
        assert data == pillow_file(np.asarray(image), 75, conv.exif_with_max_value(mx))
        assert Image.open(io.BytesIO(data)).getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] == float(mx)


@pytest.mark.parametrize("extension", ["jpg", "jpeg"])
def test_audio_to_images_batch_writes_the_files_pillow_wrote(tmp_path, golden_dir, extension):
    import shutil

    from riffusion import cli
    from riffusion.spectrogram_params import SpectrogramParams

    wavs, waves = _golden_waves(golden_dir)
    audio_dir, out_dir = tmp_path / "audio", tmp_path / "out"
    audio_dir.mkdir()
    for w in wavs:
        shutil.copy(w, audio_dir)
    cli.audio_to_images_batch(audio_dir=str(audio_dir), output_dir=str(out_dir), image_extension=extension, batch_size=2)
    # the host route's flush, restated: the images of spectrogram_images_from_waveforms, saved by Pillow with their EXIF
    params = SpectrogramParams(stereo=True)
    conv = _conv(stereo=True)
    names = []
    for w, wave in zip(wavs, waves):
        images, max_values = conv.spectrogram_images_from_waveforms(torch.from_numpy(wave)[None])
        image = images[0]
        exif_data = params.to_exif()
        exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(max_values[0])
        image.getexif().update(exif_data.items())
        ref = tmp_path / "ref.jpg"
        image.save(str(ref), exif=image.getexif(), format="JPEG")
        names.append(os.path.splitext(os.path.basename(w))[0] + "." + extension)
        assert (out_dir / names[-1]).read_bytes() == ref.read_bytes(), w
    assert sorted(p.name for p in out_dir.iterdir()) == sorted(names)


def test_refusals_before_any_launch():
    from riffusion import _hip

    conv = _conv()
    lib = conv.converter._plan().lib
    t = np.zeros((2, 64), np.uint16)
    for quality in (0, 101):
        assert lib.rfx_jpeg_quant_tables(quality, t.ctypes.data, t.ctypes.data + 128) == -4  # RFX_ERR_UNSUPPORTED
        assert b"quality" in lib.rfx_last_error()
        with pytest.raises(ValueError, match="quality"):
            conv.jpeg_bytes_from_images(np.zeros((1, 8, 8, 3), np.uint8), quality=quality)
    # W = 65536: refused on the sizes alone, with buffers that would be far too small had anything been launched
    img = torch.zeros((1, 1, 65536, 3), dtype=torch.uint8, device="cuda")
    small = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    qt = torch.from_numpy(_hip.jpeg_quant_tables(75).view(np.int16)).cuda()
    rc = lib.rfx_jpeg_encode_u8(img.data_ptr(), 1, 1, 65536, qt.data_ptr(), small.data_ptr(), sizes.data_ptr(), small.data_ptr(),
                                _hip.current_stream(torch.device("cuda", 0)))
    assert rc == -4 and b"65535" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert int(sizes[0]) == -1 and bool((small == 7).all())
    assert lib.rfx_jpeg_scan_capacity(1, 65536) == 0 and lib.rfx_jpeg_encode_workspace_bytes(1, 1, 65536) == 0
    with pytest.raises(_hip.RfxError, match="65535"):  # the library's words, through the plan ...
        conv.converter._plan().jpeg_scans(img)
    with pytest.raises(ValueError, match="65535"):  # ... and the header's, before the plan is asked
        conv.jpeg_bytes_from_images(img)
    for kw in ({"subsampling": 0}, {"optimize": True}, {"progressive": True}, {"optimize": False}):
        with pytest.raises(ValueError, match="not implemented"):
            conv.jpeg_bytes_from_images(np.zeros((1, 8, 8, 3), np.uint8), **kw)
