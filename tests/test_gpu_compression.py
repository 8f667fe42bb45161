"""
apply_filters(compression=True) on the device (csrc/rfx_compress.hip + the compression=False filters of csrc/rfx_pcm.hip):
the same bytes on the MI355X as audio_util.apply_filters(PcmSegment, compression=True) on the host - through Plan.apply_filters
in both forms of the compressor's recurrence and through the flag-and-patch path, the batch entry point, the tile sequence and
the batch CLI.
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


def _host(pcm: np.ndarray, rate: int) -> np.ndarray:
    from riffusion.util import audio_util

    return np.stack([audio_util.apply_filters(audio_util.PcmSegment(c, rate), compression=True)._data for c in pcm])


def _og_beat(golden_dir):
    from riffusion.util import image_util

    return np.asarray(image_util.rgb_array_from_image(Image.open(os.path.join(golden_dir, "og_beat_64.png"))))[None]


def _near_silent():
    quiet = np.full((2, 512, 512, 3), 255, np.uint8)  # near silence: every pixel 255 or 254
    quiet[0, ::7, ::5] = 254
    quiet[1, 100, 200] = 254
    return quiet


_CASES = {}


def _cases(stereo, golden_dir):
    """Decoded PCM batches (N = 1, 7, og_beat, near silence) and their host-filtered bytes, once per channel count."""
    if stereo not in _CASES:
        conv = _conv(stereo)
        rate = conv.p.sample_rate
        out = []
        for tiles in (synthetic_tiles_u8(1, seed=1), synthetic_tiles_u8(7, seed=2), _og_beat(golden_dir), _near_silent()):
            raw = conv.audio_from_spectrogram_images(tiles, seed=99)
            out.append((raw, _host(raw, rate)))
        _CASES[stereo] = (conv, out)
    return _CASES[stereo]


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("form", ["chunked", "sequential"])
def test_plan_compressed_equals_host(stereo, form, golden_dir):
    conv, cases = _cases(stereo, golden_dir)
    plan = conv.converter._plan()
    for raw, want in cases:
        src = torch.from_numpy(raw).cuda()
        stats = {}
        got = plan.apply_filters(src, compression=True, compress_form=form, stats=stats)
        assert np.array_equal(got.cpu().numpy(), want), (raw.shape, form, int((got.cpu().numpy() != want).sum()))
        assert np.array_equal(src.cpu().numpy(), raw)  # out of place: the input is untouched
        assert not stats["host_fallback"]
        if form == "sequential":
            assert not stats["rounds"].any()
        inplace = src.clone()
        assert plan.apply_filters(inplace, out=inplace, compression=True, compress_form=form).data_ptr() == inplace.data_ptr()
        assert np.array_equal(inplace.cpu().numpy(), want)


@pytest.mark.parametrize("form", ["chunked", "sequential"])
def test_plan_compressed_forced_patch_path(form, golden_dir):
    """margin 1.0: every product of non-zero attenuation is recomputed with the host's pow - the same bytes (plumbing of the
    patch path).  A list too small for them: the batch is filtered on the host instead - the same bytes again."""
    conv, cases = _cases(False, golden_dir)
    plan = conv.converter._plan()
    for raw, want in cases[:3]:
        src = torch.from_numpy(raw).cuda()
        stats = {}
        got = plan.apply_filters(src, compression=True, compress_form=form, margin=1.0, flag_capacity=raw.size, stats=stats)
        assert np.array_equal(got.cpu().numpy(), want)
        assert stats["n_flagged"] > 0 and not stats["host_fallback"]
    raw, want = cases[0]
    src = torch.from_numpy(raw).cuda()
    stats = {}
    got = plan.apply_filters(src, out=src, compression=True, compress_form=form, margin=1.0, flag_capacity=16, stats=stats)
    assert stats["host_fallback"] and stats["n_flagged"] > 16
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("chunk", [1, 7, 220, 256, 10 ** 6])
def test_plan_compressed_chunk_lengths(chunk, golden_dir):
    conv, cases = _cases(True, golden_dir)
    plan = conv.converter._plan()
    raw, want = cases[1]
    got = plan.apply_filters(torch.from_numpy(raw).cuda(), compression=True, chunk_frames=chunk)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("C", [1, 2])
def test_plan_compressed_48k(C):
    """A 48 kHz plan (look_frames 240): PCM batches straight into Plan.apply_filters, both forms."""
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    plan = _hip.get_plan(SpectrogramParams(sample_rate=48000), "cuda:0")
    rng = np.random.default_rng(C)
    L = 48000
    t = np.arange(L)
    clips = [np.sin(t * 0.02) * 20000 * ((t // 6000) % 2) + rng.normal(0, 50, L), rng.normal(0, 3000, L),
             np.sin(t * 0.05) * np.linspace(0, 15000, L), np.where((t // 100) % 2 == 0, 32767.0, -32768.0)]
    raw = np.stack([np.stack([c * (1 - 0.25 * k) for k in range(C)], axis=1) for c in clips]).astype(np.int16)
    want = _host(raw, 48000)
    for form in ("chunked", "sequential"):
        got = plan.apply_filters(torch.from_numpy(raw).cuda(), compression=True, compress_form=form)
        assert np.array_equal(got.cpu().numpy(), want), form


def test_batch_entry_compression(golden_dir):
    conv = _conv(False)
    rate = conv.p.sample_rate
    tiles = synthetic_tiles_u8(7, seed=2)
    want = _host(conv.audio_from_spectrogram_images(tiles, seed=99), rate)
    for per_call in (64, 3):
        got = conv.audio_from_spectrogram_images(tiles, seed=99, tiles_per_call=per_call, apply_filters=True, compression=True)
        assert np.array_equal(got, want), per_call
    dev = conv.audio_from_spectrogram_images(tiles, seed=99, apply_filters=True, compression=True, return_device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    with pytest.raises(ValueError):
        conv.audio_from_spectrogram_images(tiles, seed=99, compression=True)
    # 64 tiles in one call: clips 0, 31 and 63 against the host
    big = synthetic_tiles_u8(64, seed=3)
    raw = conv.audio_from_spectrogram_images(big, seed=7)
    got = conv.audio_from_spectrogram_images(big, seed=7, apply_filters=True, compression=True)
    for i in (0, 31, 63):
        assert np.array_equal(got[i], _host(raw[i:i + 1], rate)[0]), i


@pytest.mark.parametrize("stereo", [False, True])
def test_sequence_compression(stereo):
    from riffusion.util import audio_util

    conv = _conv(stereo)
    rate = conv.p.sample_rate
    tiles = synthetic_tiles_u8(4, 512, 128, seed=5 + stereo)
    raw = conv.audio_from_spectrogram_images(tiles, seed=3)
    clips = [audio_util.PcmSegment(c, rate) for c in _host(raw, rate)]
    for xf in (0.0, 0.2):
        want = audio_util.stitch_segments(clips, xf).get_array_of_samples()
        got = conv.audio_from_spectrogram_image_sequence(tiles, crossfade_s=xf, seed=3, compression=True)
        assert np.array_equal(np.asarray(got.get_array_of_samples()), want), xf


def test_cli_compression_flag(golden_dir, tmp_path):
    """images-to-audio-batch --compression writes the host filter's bytes of the same decode (the decode's seed is drawn from
    torch's generator: seeded alike for both runs)."""
    from riffusion import cli
    from riffusion.util import audio_util

    tiles = tmp_path / "tiles"
    tiles.mkdir()
    for i in range(2):
        Image.open(os.path.join(golden_dir, "og_beat_64.png")).save(str(tiles / f"t{i}.png"))
    torch.manual_seed(1234)
    cli.main(["images-to-audio-batch", "--image-dir", str(tiles), "--output-dir", str(tmp_path / "raw"), "--no-filters"])
    torch.manual_seed(1234)
    cli.main(["images-to-audio-batch", "--image-dir", str(tiles), "--output-dir", str(tmp_path / "wavs"), "--compression"])
    for i in range(2):
        raw = audio_util.PcmSegment.from_wav(str(tmp_path / "raw" / f"t{i}.wav"))
        got = audio_util.PcmSegment.from_wav(str(tmp_path / "wavs" / f"t{i}.wav"))
        want = audio_util.apply_filters(raw, compression=True)
        assert got.frame_rate == raw.frame_rate and np.array_equal(got._data, want._data), i
