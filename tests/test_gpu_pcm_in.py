"""
The int16 front end of the encode on the device (csrc/rfx_pcm_in.hip): Plan.resample_pcm equals PcmSegment.set_channels /
set_frame_rate (audioop.ratecv, or the restatement tests/test_pcm_in_cpu.py proves equal to it) byte for byte;
Plan.clips_to_waveform equals the host's slicing, mix and float32 conversion bit for bit; the fused rfx_image_from_pcm16_clips
gives the image bytes and MAX_VALUE bits of rfx_image_from_waveform on host-built waveforms;
SpectrogramImageConverter.spectrogram_images_from_audio_clips equals per-clip spectrogram_image_from_audio over
slice_audio_into_clips; and the batch CLI writes the files the host path wrote.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GIB = 1 << 30


def _conv(stereo=False, **kw):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=stereo, **kw), device="cuda")


def _plan():
    return _conv().converter._plan()


def _golden(golden_dir):
    from scipy.io import wavfile

    wavs = sorted(glob.glob(os.path.join(golden_dir, "clip_*.wav")))
    assert len(wavs) == 3
    return [wavfile.read(w)[1] for w in wavs]


def _host_resample(x: np.ndarray, in_rate: int, out_rate: int, out_channels=None) -> np.ndarray:
    from riffusion.util.audio_util import PcmSegment

    seg = PcmSegment(x, in_rate)
    if out_channels is not None:
        seg = seg.set_channels(out_channels)
    return seg.set_frame_rate(out_rate)._data


def _device_resample(plan, x: np.ndarray, in_rate: int, out_rate: int, out_channels=None) -> np.ndarray:
    out = plan.resample_pcm(torch.from_numpy(np.ascontiguousarray(x)).cuda(), in_rate, out_rate, out_channels)
    assert out.is_cuda and out.dtype == torch.int16
    return out.cpu().numpy()


def _random_track(rng, L: int, C: int) -> np.ndarray:
    x = rng.integers(-32768, 32768, size=(L, C)).astype(np.int16)
    if L >= 16:
        x[L // 4 : L // 4 + L // 16] = -32768
        x[L // 2 : L // 2 + L // 16] = 32767
    return x


# ---- resample ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 22050, 16000])
def test_resample_golden_wavs_there_and_back(golden_dir, rate):
    plan = _plan()
    for x in _golden(golden_dir):
        for out_channels in (None, 1):
            there = _host_resample(x, 44100, rate, out_channels)
            assert np.array_equal(_device_resample(plan, x, 44100, rate, out_channels), there)
            assert np.array_equal(_device_resample(plan, there, rate, 44100), _host_resample(there, rate, 44100))
        mono = np.ascontiguousarray(x[:, :1])
        assert np.array_equal(_device_resample(plan, mono, 44100, rate, 2), _host_resample(mono, 44100, rate, 2))


def test_resample_240_s_stereo_48k(golden_dir):
    plan = _plan()
    x = _random_track(np.random.default_rng(48), 240 * 48000, 2)
    for out_channels in (None, 1):
        got = _device_resample(plan, x, 48000, 44100, out_channels)
        want = _host_resample(x, 48000, 44100, out_channels)
        assert got.shape == want.shape and len(got) == (len(x) - 1) * 147 // 160 + 1 == 10_584_000 and np.array_equal(got, want)


@pytest.mark.parametrize("in_rate,out_rate", [(48000, 44100), (44100, 48000), (8000, 44100), (96000, 44100), (44100, 44101), (12345, 44100),
                                              (999983, 1000003), (1048573, 7), (44100, 44100)])
def test_resample_short_and_odd_lengths(in_rate, out_rate):
    plan = _plan()
    rng = np.random.default_rng(in_rate % 1000 + out_rate % 777)
    for L in (1, 2, 7, 8, 9, 1000, 50001):
        for C, C_out in ((1, None), (2, None), (2, 1), (1, 2)):
            x = _random_track(rng, L, C)
            got = _device_resample(plan, x, in_rate, out_rate, C_out)
            assert np.array_equal(got, _host_resample(x, in_rate, out_rate, C_out)), (L, C, C_out)


def test_resample_into_unaligned_views():
    """outputs that start off a 16-byte boundary (the kernel's head frames) and inputs that start at any frame"""
    from riffusion import _hip
    from riffusion.util import audio_util

    plan = _plan()
    x = _random_track(np.random.default_rng(9), 30011, 2)
    want = _host_resample(x, 48000, 44100)
    K = audio_util.ratecv_frames(len(x), 48000, 44100)
    for shift in (1, 2, 3):
        src = torch.zeros((len(x) + shift, 2), dtype=torch.int16, device="cuda")
        src[shift:] = torch.from_numpy(x).cuda()
        dst = torch.full((K + shift + 8, 2), 77, dtype=torch.int16, device="cuda")
        _hip.check(plan.lib.rfx_pcm16_resample(src[shift:].data_ptr(), len(x), 2, 48000, 2, 44100, dst[shift:].data_ptr(), K, plan._stream()))
        host = dst.cpu().numpy()
        assert np.array_equal(host[shift : shift + K], want) and (host[:shift] == 77).all() and (host[shift + K :] == 77).all()


def test_resample_refuses_bad_arguments():
    from riffusion import _hip

    plan = _plan()
    x = torch.zeros((100, 2), dtype=torch.int16, device="cuda")
    with pytest.raises(_hip.RfxError, match="2\\^20"):
        plan.resample_pcm(x, 1048577, 7)
    with pytest.raises(ValueError):
        plan.resample_pcm(x.float(), 48000, 44100)
    with pytest.raises(ValueError):
        plan.resample_pcm(x, 48000, 44100, out_channels=3)
    out = torch.zeros((50, 2), dtype=torch.int16, device="cuda")
    assert plan.lib.rfx_pcm16_resample(x.data_ptr(), 100, 2, 48000, 2, 44100, out.data_ptr(), 50, plan._stream()) == -1  # 92 frames
    assert tuple(plan.resample_pcm(x[:0], 48000, 44100).shape) == (0, 2)


def test_resample_past_2_31_bytes_of_output_offset():
    """590 M stereo frames at 48 kHz -> 542 M frames, 2.17 GB: output byte offsets pass 2^31.  The track is made on the device;
    windows of the result are held against audioop on the host: a window that starts at input frame m * 160 (48 000 -> 44 100
    reduces to 160 -> 147) starts at output frame m * 147 with audioop's counter at 0, where the output is the current sample
    alone - the resample of the window on its own gives the same frames."""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * GIB:
        pytest.skip(f"needs 8 GiB of free device memory, {free / GIB:.1f} GiB free")
    plan = _plan()
    L = 590_000_000
    x = torch.randint(-32768, 32768, (L, 2), dtype=torch.int16, device="cuda", generator=torch.Generator("cuda").manual_seed(31))
    out = plan.resample_pcm(x, 48000, 44100)
    K = (L - 1) * 147 // 160 + 1
    assert tuple(out.shape) == (K, 2) and K * 4 > (1 << 31)
    W = 200_000
    for m in (0, ((1 << 31) // 4) // 147 - 500, ((1 << 31) // 4) // 160 - 500, (L - W) // 160):
        window = x[m * 160 : m * 160 + W].cpu().numpy()
        want = _host_resample(window, 48000, 44100)
        got = out[m * 147 : m * 147 + len(want)].cpu().numpy()
        assert np.array_equal(got, want), m
    assert (L - W) // 160 * 147 + len(want) == K  # the last window ends where the track does
    del x, out
    torch.cuda.empty_cache()


# ---- gather and the fused call ----------------------------------------------------------------------------------------------------
def _host_waveforms(x: np.ndarray, starts, Lw: int, C: int) -> np.ndarray:
    """per clip: the slice, set_channels, then spectrogram_image_from_audio's float32 (channels, samples) array"""
    from riffusion.util.audio_util import PcmSegment

    rows = []
    for a in starts:
        clip = PcmSegment(x[a : a + Lw], 44100).set_channels(C)
        rows.append(np.array([c.get_array_of_samples() for c in clip.split_to_mono()]).astype(np.float32))
    return np.stack(rows)  # (N, C, Lw)


@pytest.mark.parametrize("N", [1, 4, 64])
@pytest.mark.parametrize("in_channels,stereo", [(2, True), (2, False), (1, False), (1, True)])
def test_gather_and_fused_call_equal_host_waveforms(golden_dir, N, in_channels, stereo):
    conv = _conv(stereo)
    plan = conv.converter._plan()
    C = 2 if stereo else 1
    rng = np.random.default_rng(N * 10 + in_channels)
    # music from the golden clips and a stretch of noise; clips of 5 s every 0.37 s: they overlap
    x = np.concatenate(_golden(golden_dir) + [_random_track(rng, 500_000, 2)])
    x = np.ascontiguousarray(x[:, :in_channels])
    Lw = 220500
    starts = ((np.arange(N) * 16317) % (len(x) - Lw)).astype(np.int64)
    starts[-1] = len(x) - Lw  # the last clip ends with the recording
    want = _host_waveforms(x, starts, Lw, C)
    pcm = torch.from_numpy(x).cuda()
    got = plan.clips_to_waveform(pcm, starts, Lw, C)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N * C, Lw)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.reshape(N * C, Lw).view(np.int32))
    # the fused entry against rfx_image_from_waveform on the host-built waveforms
    from riffusion.util import image_util

    power = float(conv.p.power_for_image)
    thr = plan.device_constant(("encode_thresholds", power), lambda: image_util.encode_thresholds(power))
    img_w, mx_w = plan.image_from_waveform(torch.from_numpy(want.reshape(N * C, Lw)).cuda(), stereo, thr)
    img, mx = plan.image_from_pcm_clips(pcm, starts, Lw, stereo, thr)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (N, 512, 501, 3)
    assert torch.equal(img, img_w) and torch.equal(mx.view(torch.int32), mx_w.view(torch.int32))


def test_gather_refuses_clips_outside_the_recording():
    from riffusion import _hip

    plan = _plan()
    pcm = torch.zeros((1000, 2), dtype=torch.int16, device="cuda")
    for starts in ([0, 781], [-1], [1000]):
        with pytest.raises(_hip.RfxError, match="outside the recording"):
            plan.clips_to_waveform(pcm, starts, 220, 1)
    assert tuple(plan.clips_to_waveform(pcm, [], 220, 2).shape) == (0, 220)
    assert tuple(plan.clips_to_waveform(pcm, [780], 220, 2).shape) == (2, 220)


# ---- the Python method ------------------------------------------------------------------------------------------------------------
def _per_clip_reference(conv, segment, starts_s, duration_s):
    """the parent path: host set_frame_rate, slice_audio_into_clips, spectrogram_image_from_audio per clip"""
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    seg = segment.set_frame_rate(conv.p.sample_rate)
    images = [conv.spectrogram_image_from_audio(c) for c in audio_util.slice_audio_into_clips(seg, starts_s, duration_s)]
    return images, [im.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] for im in images]


def _assert_same_images(got, want):
    images, maxima = got
    want_images, want_maxima = want
    assert len(images) == len(want_images)
    for a, b in zip(images, want_images):
        assert a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b))
    assert [float(m) for m in maxima] == [float(m) for m in want_maxima]


@pytest.mark.parametrize("stereo", [False, True])
def test_images_from_audio_clips_golden_track(golden_dir, stereo):
    from riffusion.util import audio_util
    from riffusion.util.audio_util import PcmSegment

    conv = _conv(stereo)
    track = PcmSegment(np.concatenate(_golden(golden_dir)), 44100)
    starts_s = audio_util.clip_start_times(track.duration_seconds, 5.0, 0.2)
    assert len(starts_s) == 3
    _assert_same_images(conv.spectrogram_images_from_audio_clips(track, starts_s, 5.0), _per_clip_reference(conv, track, starts_s, 5.0))
    img, mx = conv.spectrogram_images_from_audio_clips(track, starts_s, 5.0, return_device=True)
    assert img.is_cuda and tuple(img.shape) == (3, 512, 501, 3) and mx.is_cuda and tuple(mx.shape) == (3,)
    # a mono track into the same converter
    mono = track.set_channels(1)
    _assert_same_images(conv.spectrogram_images_from_audio_clips(mono, starts_s, 5.0), _per_clip_reference(conv, mono, starts_s, 5.0))


def test_images_from_audio_clips_48k_input_and_short_last_clip(golden_dir):
    from riffusion.util.audio_util import PcmSegment

    conv = _conv()
    track48 = PcmSegment(np.concatenate(_golden(golden_dir)), 44100).set_frame_rate(48000)  # a 48 kHz recording of the same music
    assert track48.frame_rate == 48000
    starts_s = np.arange(0, 17.0, 4.8)  # 0, 4.8, 9.6, 14.4: the last clip has 2.6 s of audio, the rest is the silence branch
    got = conv.spectrogram_images_from_audio_clips(track48, starts_s, 5.0)
    want = _per_clip_reference(conv, track48, starts_s, 5.0)
    widths = [im.size[0] for im in want[0]]
    assert widths[:3] == [501, 501, 501] and 480 < widths[3] < 501  # append's crossfade takes 100 ms off the last clip
    _assert_same_images(got, want)
    tiles, mx = conv.spectrogram_images_from_audio_clips(track48, starts_s, 5.0, return_device=True)
    assert isinstance(tiles, list) and [int(t.shape[1]) for t in tiles] == widths and tuple(mx.shape) == (4,)
    # less than 100 ms missing from the last clip: the reference's append raises, and so does this
    with pytest.raises(ValueError, match="Crossfade is longer"):
        conv.spectrogram_images_from_audio_clips(track48, [0.0, 12.08], 5.0)
    with pytest.raises(ValueError, match="Crossfade is longer"):
        _per_clip_reference(conv, track48, [0.0, 12.08], 5.0)


# ---- the batch CLI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
def test_audio_to_images_batch_writes_the_parent_paths_files(tmp_path, golden_dir, mono):
    from scipy.io import wavfile

    from riffusion import cli
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util.audio_util import PcmSegment

    x = _golden(golden_dir)[0][: 2 * 44100]
    audio_dir, out_dir, ref_dir = tmp_path / "audio", tmp_path / "out", tmp_path / "ref"
    audio_dir.mkdir(), ref_dir.mkdir()
    files = {
        "a_44k_stereo": PcmSegment(x, 44100),
        "b_48k_stereo": PcmSegment(x, 44100).set_frame_rate(48000),
        "c_44k_mono": PcmSegment(x, 44100).set_channels(1),
        "d_22k_mono": PcmSegment(x, 44100).set_channels(1).set_frame_rate(22050),
        "e_48k_stereo_again": PcmSegment(x[::-1].copy(), 44100).set_frame_rate(48000),
        "f_16k_stereo": PcmSegment(x, 44100).set_frame_rate(16000),
    }
    for name, seg in files.items():
        seg.export(str(audio_dir / (name + ".wav")), format="wav")
    cli.audio_to_images_batch(audio_dir=str(audio_dir), output_dir=str(out_dir), image_extension="png", mono=mono, batch_size=2)
    # the parent path, inline: host set_channels / set_frame_rate, the float waveform, spectrogram_images_from_waveforms
    params = SpectrogramParams(stereo=not mono)
    conv = _conv(stereo=not mono)
    channels = 1 if mono else 2
    for name in files:
        seg = PcmSegment.from_wav(str(audio_dir / (name + ".wav")))
        if seg.channels != channels:
            seg = seg.set_channels(channels)
        if seg.frame_rate != params.sample_rate:
            seg = seg.set_frame_rate(params.sample_rate)
        wave = np.array([c.get_array_of_samples() for c in seg.split_to_mono()]).astype(np.float32)
        images, max_values = conv.spectrogram_images_from_waveforms(torch.from_numpy(wave)[None])
        exif_data = params.to_exif()
        exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(max_values[0])
        images[0].getexif().update(exif_data.items())
        images[0].save(str(ref_dir / (name + ".png")), exif=images[0].getexif(), format="PNG")
        assert (out_dir / (name + ".png")).read_bytes() == (ref_dir / (name + ".png")).read_bytes(), name
    assert sorted(p.name for p in out_dir.iterdir()) == sorted(n + ".png" for n in files)
