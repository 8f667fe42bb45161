"""
The decode's post-processing on the device (csrc/rfx_pcm.hip): audio_util.apply_filters(compression=False) and
audio_util.stitch_segments give the same bytes on the MI355X as on the host - through Plan.apply_filters / Plan.stitch, the
batch entry point's apply_filters=True, audio_from_spectrogram_image_sequence and the per-clip reference methods.
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from helpers import synthetic_tiles_u8

pytestmark = pytest.mark.gpu


def _conv(stereo=False, iters=8, **kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, num_griffin_lim_iters=iters, **kw), device="cuda")


def _host_filters(pcm: np.ndarray, rate: int) -> np.ndarray:
    from riffusion.util import audio_util

    out = np.empty_like(pcm)
    for i, clip in enumerate(pcm):
        seg = audio_util.apply_filters(audio_util.PcmSegment(clip, rate), compression=False)
        out[i] = seg.get_array_of_samples().reshape(clip.shape)
    return out


def _og_beat(golden_dir):
    from riffusion.util import image_util

    return np.asarray(image_util.rgb_array_from_image(Image.open(os.path.join(golden_dir, "og_beat_64.png"))))[None]


@pytest.mark.parametrize("stereo", [False, True])
def test_batch_filters_equal_host_filters(stereo, golden_dir):
    conv = _conv(stereo)
    rate = conv.p.sample_rate
    cases = [synthetic_tiles_u8(1, seed=1), synthetic_tiles_u8(7, seed=2), _og_beat(golden_dir)]
    quiet = np.full((2, 512, 512, 3), 255, np.uint8)  # near silence: every pixel 255 or 254
    quiet[0, ::7, ::5] = 254
    quiet[1, 100, 200] = 254
    cases.append(quiet)
    if not stereo:
        cases.append(synthetic_tiles_u8(64, seed=3))
    for tiles in cases:
        raw = conv.audio_from_spectrogram_images(tiles, seed=99)
        want = _host_filters(raw, rate)
        for per_call in (64, 5):
            got = conv.audio_from_spectrogram_images(tiles, seed=99, tiles_per_call=per_call, apply_filters=True)
            assert got.dtype == np.int16 and np.array_equal(got, want), (tiles.shape, per_call, int((got != want).sum()))
        dev = conv.audio_from_spectrogram_images(tiles, seed=99, apply_filters=True, return_device=True)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)


def test_filters_refuse_return_waveform():
    conv = _conv()
    with pytest.raises(ValueError):
        conv.audio_from_spectrogram_images(synthetic_tiles_u8(1, 512, 64), return_waveform=True, apply_filters=True)


def _edge_batch(rng, L, C):
    clips = [np.zeros((L, C), np.int16), np.full((L, C), -32768, np.int16), np.full((L, C), 32767, np.int16),
             rng.integers(-3, 4, size=(L, C)).astype(np.int16), rng.integers(-32768, 32768, size=(L, C)).astype(np.int16),
             (rng.normal(0, 2000, (L, C))).astype(np.int16)]
    one_pos, one_neg, alt = clips[0].copy(), clips[0].copy(), clips[2].copy()
    one_pos[L // 2, 0] = 1
    one_neg[L // 3, C - 1] = -1
    alt.reshape(-1)[::2] = -32768
    return np.stack(clips + [one_pos, one_neg, alt])


@pytest.mark.parametrize("L,C", [(1, 1), (3, 2), (441, 2), (4427, 1), (225351, 1), (225351, 2), (88203, 2)])
def test_plan_apply_filters_equals_pcmsegment(L, C):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    plan = _hip.get_plan(SpectrogramParams(), "cuda:0")
    batch = _edge_batch(np.random.default_rng(L + C), L, C)
    want = _host_filters(batch, 44100)
    dev = torch.from_numpy(batch).cuda()
    assert np.array_equal(plan.apply_filters(dev).cpu().numpy(), want)
    # in place, and on an odd offset into a bigger buffer (the unaligned head / tail of the 16-byte passes)
    flat = torch.zeros(batch.size + 3, dtype=torch.int16, device="cuda")
    view = flat[3:].view(batch.shape)
    view.copy_(dev)
    assert plan.apply_filters(view, out=view).data_ptr() == view.data_ptr()
    assert np.array_equal(view.cpu().numpy(), want)
    assert int(flat[:3].abs().sum()) == 0


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("rate", [44100, 48000])
def test_sequence_equals_host_stitch_of_host_filtered_clips(stereo, rate):
    from riffusion.util import audio_util

    conv = _conv(stereo, sample_rate=rate)
    tiles = synthetic_tiles_u8(4, 512, 128, seed=rate + stereo)  # 1.27 s clips (44.1 kHz), 1.27 s (48 kHz)
    raw = conv.audio_from_spectrogram_images(tiles, seed=5)
    clips = [audio_util.PcmSegment(c, rate) for c in _host_filters(raw, rate)]
    for xf in (0.0, 0.05, 0.2):
        want = audio_util.stitch_segments(clips, xf).get_array_of_samples()
        got = conv.audio_from_spectrogram_image_sequence(tiles, crossfade_s=xf, seed=5)
        assert got.frame_rate == rate and got.channels == (2 if stereo else 1)
        assert np.array_equal(np.asarray(got.get_array_of_samples()), want), xf
        dev = conv.audio_from_spectrogram_image_sequence(tiles, crossfade_s=xf, seed=5, return_device=True, tiles_per_call=3)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy().reshape(-1), want)
    # one tile: the clip itself; a crossfade longer than a clip: append's ValueError
    one = conv.audio_from_spectrogram_image_sequence(tiles[:1], crossfade_s=0.2, seed=5)
    assert np.array_equal(np.asarray(one.get_array_of_samples()), clips[0].get_array_of_samples())
    with pytest.raises(ValueError, match="Crossfade is longer"):
        conv.audio_from_spectrogram_image_sequence(tiles[:, :, :8], crossfade_s=0.2, seed=5)


def test_sequence_of_36_full_tiles_with_the_audio_to_audio_crossfade():
    from riffusion.util import audio_util

    conv = _conv(iters=4)
    tiles = synthetic_tiles_u8(36, seed=36)
    raw = conv.audio_from_spectrogram_images(tiles, seed=8)
    want = audio_util.stitch_segments([audio_util.PcmSegment(c, 44100) for c in _host_filters(raw, 44100)], 0.2)
    got = conv.audio_from_spectrogram_image_sequence(tiles, seed=8)
    assert np.array_equal(np.asarray(got.get_array_of_samples()), want.get_array_of_samples())


def test_plan_stitch_of_random_clips():
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    plan = _hip.get_plan(SpectrogramParams(), "cuda:0")
    rng = np.random.default_rng(11)
    for N, L, C, rate, xf in ((37, 441 * 511, 1, 44100, 0.2), (5, 441 * 511 + 17, 2, 48000, 0.05), (3, 4427, 1, 44100, 0.0),
                              (4, 2405, 2, 8000, 0.15)):
        batch = rng.integers(-32768, 32768, size=(N, L, C)).astype(np.int16)
        want = audio_util.stitch_segments([audio_util.PcmSegment(c, rate) for c in batch], xf).get_array_of_samples()
        got = plan.stitch(torch.from_numpy(batch).cuda(), rate, xf)
        assert np.array_equal(got.cpu().numpy().reshape(-1), want), (N, L, C, rate, xf)


def test_reference_methods_filter_on_the_device(golden_dir):
    from riffusion.util import audio_util

    conv = _conv()
    img = Image.open(os.path.join(golden_dir, "og_beat_64.png"))
    torch.manual_seed(3)
    seg = conv.audio_from_spectrogram_image(img)
    torch.manual_seed(3)
    raw = conv.audio_from_spectrogram_images(_og_beat(golden_dir))
    want = audio_util.apply_filters(audio_util.segment_from_pcm16(raw[0], 44100), compression=False)
    assert np.array_equal(np.asarray(seg.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
    # SpectrogramConverter.audio_from_spectrogram: the same filters after its own decode
    sc = conv.converter
    mel = np.random.default_rng(2).uniform(0, 3e6, size=(1, 512, 64)).astype(np.float32)
    torch.manual_seed(4)
    filtered = sc.audio_from_spectrogram(mel)
    torch.manual_seed(4)
    unfiltered = sc.audio_from_spectrogram(mel, apply_filters=False)
    want = audio_util.apply_filters(unfiltered, compression=False)
    assert np.array_equal(np.asarray(filtered.get_array_of_samples()), np.asarray(want.get_array_of_samples()))
