"""
Tile resize on the device (csrc/rfx_resize.hip): SpectrogramImageConverter.resize_images equals PIL.Image.resize byte for byte,
pipeline_input_from_images equals the pipeline's preprocess_image bit for bit, and the reference's audio-to-audio chain - slice,
encode, widen to 512, a stand-in for diffusion, quantise, shrink back, decode, filter, stitch - gives the same int16 bytes on
the device as on the host.
"""
import glob
import os

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import synthetic_tiles_u8

pytestmark = pytest.mark.gpu

SIZES = [((501, 512), (512, 512)), ((512, 512), (501, 512)), ((500, 512), (512, 512)), ((512, 512), (7, 512)),
         ((1, 1), (32, 32)), ((17, 17), (512, 512)), ((401, 300), (333, 257)), ((512, 64), (64, 512)), ((512, 501), (512, 512))]


def _conv(stereo=False, iters=32, **kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, num_griffin_lim_iters=iters, **kw), device="cuda")


def _pil(tiles: np.ndarray, size, resample) -> np.ndarray:
    return np.stack([np.asarray(Image.fromarray(t).resize(size, resample)) for t in tiles])


@pytest.mark.parametrize("resample", [Image.BICUBIC, Image.LANCZOS, Image.BILINEAR])
@pytest.mark.parametrize("src,dst", SIZES)
def test_resize_equals_pillow(src, dst, resample):
    conv = _conv()
    rng = np.random.default_rng(src[0] + 3 * dst[1])
    for n in (1, 3):
        tiles = rng.integers(0, 256, size=(n, src[1], src[0], 3), dtype=np.uint8)
        tiles[-1, :, : src[0] // 3] = 255
        got = conv.resize_images(tiles, dst, resample)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (n, dst[1], dst[0], 3)
        assert np.array_equal(got.cpu().numpy(), _pil(tiles, dst, resample)), (n, src, dst, resample)


@pytest.mark.parametrize("resample", [Image.BICUBIC, Image.LANCZOS])
def test_resize_64_tiles_and_offset_views(resample):
    conv = _conv()
    tiles = synthetic_tiles_u8(64, 512, 512, seed=5)
    dev = torch.from_numpy(tiles).cuda()
    for src, dst in [(dev, (501, 512)), (dev[:, :, :501].contiguous(), (512, 512)), (dev[:, :500].contiguous(), (512, 512))]:
        want = _pil(src.cpu().numpy(), dst, resample)
        assert np.array_equal(conv.resize_images(src, dst, resample).cpu().numpy(), want)
    # a batch that starts at an odd byte offset (staging head / tail and the byte-store path)
    flat = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=3 * 512 * 501 * 3 + 5, dtype=np.uint8)).cuda()
    view = flat[5:].view(3, 512, 501, 3)
    assert np.array_equal(conv.resize_images(view, (512, 512), resample).cpu().numpy(), _pil(view.cpu().numpy(), (512, 512), resample))
    assert np.array_equal(conv.resize_images(view, (300, 200), resample).cpu().numpy(), _pil(view.cpu().numpy(), (300, 200), resample))


@pytest.mark.parametrize("stereo", [False, True])
def test_resize_of_device_encoded_tiles(stereo, golden_dir):
    from scipy.io import wavfile

    conv = _conv(stereo)
    wavs = sorted(glob.glob(os.path.join(golden_dir, "clip_*.wav")))
    x = np.stack([wavfile.read(w)[1][:220500] for w in wavs]).astype(np.float32)  # (3, 220500, 2)
    wave = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if stereo else x[:, :, :1].transpose(0, 2, 1)))
    img, mx = conv.spectrogram_images_from_waveforms(wave, return_device=True)
    assert img.is_cuda and tuple(img.shape) == (3, 512, 501, 3) and mx.is_cuda
    pil, _ = conv.spectrogram_images_from_waveforms(wave)
    host = np.stack([np.asarray(p) for p in pil])
    assert np.array_equal(img.cpu().numpy(), host)
    wide = conv.scale_images_to_32_stride(img)
    assert np.array_equal(wide.cpu().numpy(), _pil(host, (512, 512), Image.BICUBIC))
    for resample in (Image.BICUBIC, Image.LANCZOS):
        assert np.array_equal(conv.resize_images(wide, (501, 512), resample).cpu().numpy(), _pil(wide.cpu().numpy(), (501, 512), resample))


def _preprocess_image(image: Image.Image) -> torch.Tensor:
    """riffusion_pipeline.py:439-452, transcribed."""
    w, h = image.size
    w, h = map(lambda x: x - x % 32, (w, h))
    image = image.resize((w, h), resample=Image.LANCZOS)
    image_np = np.array(image).astype(np.float32) / 255.0
    image_np = image_np[None].transpose(0, 3, 1, 2)
    return 2.0 * torch.from_numpy(image_np) - 1.0


def test_pipeline_input_equals_preprocess_image():
    conv = _conv()
    rng = np.random.default_rng(11)
    for shape in [(2, 512, 512), (1, 512, 501), (3, 300, 517)]:
        tiles = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
        got = conv.pipeline_input_from_images(tiles)
        want = torch.cat([_preprocess_image(Image.fromarray(t)) for t in tiles])
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.cpu().view(torch.int32), want.contiguous().view(torch.int32)), shape


def test_resize_refuses_bad_arguments():
    from riffusion import _hip

    conv = _conv()
    tiles = synthetic_tiles_u8(1, 16, 16)
    for size, resample in [((0, 16), Image.BICUBIC), ((16, 16385), Image.BICUBIC)]:
        with pytest.raises(_hip.RfxError):
            conv.resize_images(tiles, size, resample)
    for resample in (Image.NEAREST, Image.BOX, Image.HAMMING):
        with pytest.raises(ValueError):
            conv.resize_images(tiles, (20, 20), resample)


# ---- audio-to-audio, host route against device route ---------------------------------------------------------------------------
STANDIN_LUT = ((np.arange(256, dtype=np.float64) / 255.0) ** 0.8).astype(np.float32)


def _standin_host(tiles: np.ndarray) -> np.ndarray:
    """A fixed map of 512-wide tiles to the pipeline's float NHWC output in [0, 1]: a per-byte curve and a horizontal flip."""
    return STANDIN_LUT[tiles][:, :, ::-1, :]


def _standin_device(tiles: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(STANDIN_LUT).to(tiles.device)[tiles.long()].flip(2)


def _scale_image_to_32_stride(image: Image.Image) -> Image.Image:
    """streamlit/tasks/audio_to_audio.py:419-425, transcribed."""
    closest_width = int(np.ceil(image.width / 32) * 32)
    closest_height = int(np.ceil(image.height / 32) * 32)
    return image.resize((closest_width, closest_height), Image.BICUBIC)


def _track(golden_dir, n_wavs=3):
    from scipy.io import wavfile

    from riffusion.util.audio_util import PcmSegment

    wavs = sorted(glob.glob(os.path.join(golden_dir, "clip_*.wav")))[:n_wavs]
    return PcmSegment(np.concatenate([wavfile.read(w)[1] for w in wavs]), 44100)


def _host_route(conv, clips, seed):
    from riffusion.util import audio_util

    tiles = []
    for clip in clips:
        init_image = conv.spectrogram_image_from_audio(clip)
        wide = _scale_image_to_32_stride(init_image)
        out = _standin_host(np.asarray(wide)[None])
        image = Image.fromarray((out * 255).round().astype("uint8")[0])  # numpy_to_pil
        tiles.append(np.asarray(image.resize(init_image.size, Image.BICUBIC)))
    pcm = conv.audio_from_spectrogram_images(np.stack(tiles), seed=seed, apply_filters=True)
    segs = [audio_util.PcmSegment(c, conv.p.sample_rate) for c in pcm]
    return audio_util.stitch_segments(segs, 0.2).get_array_of_samples()


def _device_route(conv, clips, seed, tiles_per_call=64):
    C = 2 if conv.p.stereo else 1
    wave = torch.from_numpy(np.stack([np.asarray(c.set_channels(C)._data, np.float32).T for c in clips]))
    img, _ = conv.spectrogram_images_from_waveforms(wave, return_device=True)
    wide = conv.scale_images_to_32_stride(img)
    pipe_out = _standin_device(wide)
    assert img.is_cuda and wide.is_cuda and pipe_out.is_cuda
    pcm = conv.audio_from_spectrogram_image_sequence(pipe_out, crossfade_s=0.2, seed=seed, apply_filters=True, return_device=True,
                                                     tiles_per_call=tiles_per_call, size=(img.shape[2], img.shape[1]))
    assert pcm.is_cuda
    return pcm.cpu().numpy().reshape(-1)


def test_audio_to_audio_chain_mono(golden_dir):
    from riffusion.util import audio_util

    conv = _conv()
    track = _track(golden_dir)
    starts = audio_util.clip_start_times(track.duration_seconds, 5.0, 0.2)
    clips = audio_util.slice_audio_into_clips(track, starts, 5.0)
    assert len(clips) == 3
    want = _host_route(conv, clips, seed=7)
    _, frames = audio_util.stitch_plan(3, 220500, 44100, 0.2)
    assert frames == 643860 and want.size == frames
    for per_call in (64, 2):
        got = _device_route(conv, clips, seed=7, tiles_per_call=per_call)
        assert got.dtype == np.int16 and np.array_equal(got, want), (per_call, int((got != want).sum()))


def test_audio_to_audio_chain_stereo_20k(golden_dir):
    from riffusion.util import audio_util

    conv = _conv(stereo=True, min_frequency=10, max_frequency=20000)
    track = _track(golden_dir, n_wavs=2)
    starts = audio_util.clip_start_times(track.duration_seconds, 5.0, 0.2)
    clips = audio_util.slice_audio_into_clips(track, starts, 5.0)
    assert len(clips) == 2
    want = _host_route(conv, clips, seed=7)
    got = _device_route(conv, clips, seed=7)
    assert np.array_equal(got, want), int((got != want).sum())


def test_sequence_of_mixed_widths_stitches_on_the_host():
    from riffusion.util import audio_util

    conv = _conv(iters=8)
    a, b = synthetic_tiles_u8(1, 512, 501, seed=1)[0], synthetic_tiles_u8(1, 512, 300, seed=2)[0]
    got = conv.audio_from_spectrogram_image_sequence([a, b], crossfade_s=0.2, seed=3, return_device=True).cpu().numpy()
    pa = conv.audio_from_spectrogram_images(a[None], seed=3, apply_filters=True)[0]
    pb = conv.audio_from_spectrogram_images(np.stack([b, b]), seed=3, apply_filters=True)[1]  # b as the sequence's clip 1
    want = audio_util.stitch_segments([audio_util.PcmSegment(pa, 44100), audio_util.PcmSegment(pb, 44100)], 0.2)
    assert np.array_equal(got.reshape(-1), want.get_array_of_samples())
    # with a size, every tile is resized first and the device stitch runs
    got = conv.audio_from_spectrogram_image_sequence([a, b], crossfade_s=0.2, seed=3, size=(501, 512), return_device=True)
    tiles = np.stack([a, _pil(b[None], (501, 512), Image.BICUBIC)[0]])
    pcm = conv.audio_from_spectrogram_images(tiles, seed=3, apply_filters=True)
    want = audio_util.stitch_segments([audio_util.PcmSegment(c, 44100) for c in pcm], 0.2)
    assert np.array_equal(got.cpu().numpy().reshape(-1), want.get_array_of_samples())
