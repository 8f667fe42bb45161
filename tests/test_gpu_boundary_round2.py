"""
Boundary rows that had no test in round 1: the numpy / segment-level members of SpectrogramConverter,
the diffusion hand-off (f3), the sharded batch entry point over RCCL (e), plan / device bookkeeping, and the edge cases
of the one-instruction phase projection.
"""
import os
import socket

import numpy as np
import pytest
import torch

from helpers import oracle, snr_db, synthetic_tiles_u8, synthetic_wave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def params():
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramParams()


def test_spectrogram_from_audio_matches_oracle(O, params, golden_dir):
    """a3, reference spectrogram_converter.py:101-125: segment -> (channels, n_mels, T) float32 numpy."""
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.util import audio_util

    seg = audio_util.PcmSegment.from_wav(os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav"))
    conv = SpectrogramConverter(params, device="cuda")
    got = conv.spectrogram_from_audio(seg)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (2, 512, 1 + 250400 // 441)
    wave = torch.from_numpy(np.array([c.get_array_of_samples() for c in seg.split_to_mono()]).astype(np.float32))
    ref = O.mel_amplitudes_from_waveform(wave, O.params_from(params)).numpy()
    assert np.abs(got - ref).max() <= 1e-4 * ref.max()
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) <= 1e-4
    assert got.max() == pytest.approx(46801012.0, rel=1e-5)  # the EXIF MAX_VALUE of the reference's golden PNG
    with pytest.raises(AssertionError):
        conv.spectrogram_from_audio(audio_util.PcmSegment(np.zeros((9000, 1), np.int16), 48000))  # :114


def test_audio_from_spectrogram_returns_segment(O, params):
    """a9, reference spectrogram_converter.py:127-163: (channels, n_mels, T) numpy -> audio segment; peak-normalised
    int16 (audio_util.py:22-28), filters optional."""
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.util import audio_util

    conv = SpectrogramConverter(params, device="cuda")
    T = 64
    mel = O.spectrogram_from_image_u8(synthetic_tiles_u8(1, 512, T)[0], 0.25, True, 30e6)  # (2, 512, 64) numpy
    torch.manual_seed(3)
    seg = conv.audio_from_spectrogram(mel, apply_filters=False)
    assert seg.channels == 2 and seg.frame_rate == 44100 and seg.sample_width == 2
    assert seg.frame_count() == 441 * (T - 1)
    x = np.asarray(seg.get_array_of_samples()).reshape(-1, 2)
    assert np.abs(x.astype(np.int32)).max() == 32767  # joint peak normalisation: the larger channel hits full scale
    # same call through the torch-level seam with the same seed gives the same PCM (the member only adds the codec tail)
    torch.manual_seed(3)
    wave = conv.waveform_from_mel_amplitudes(torch.from_numpy(mel).cuda())
    assert np.array_equal(x, O.pcm16_from_waveform(wave.cpu().numpy(), normalize=True))
    # default apply_filters=True: gain to -12 dBFS, 0.1 dB headroom (audio_util.py:39-72)
    torch.manual_seed(3)
    filt = conv.audio_from_spectrogram(mel)
    assert filt.frame_count() == seg.frame_count()
    want = audio_util.apply_filters(seg, compression=False)
    assert np.array_equal(np.asarray(filt.get_array_of_samples()), np.asarray(want.get_array_of_samples()))


def test_diffusion_handoff_device_tensors(params):
    """f3, reference riffusion_pipeline.py:427-434: the decoder takes the pipeline's tensors without leaving the GPU - a uint8
    tensor on the device, or the float [0, 1] NHWC tensor quantised like numpy_to_pil ((x * 255).round().astype(uint8))."""
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    conv = SpectrogramImageConverter(params, device="cuda")
    rng = np.random.default_rng(5)
    unit = rng.random((2, 512, 48, 3), dtype=np.float32)  # what (image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1) holds
    unit[0, 0, 0] = [0.5 / 255, 1.5 / 255, 2.5 / 255]  # exact ties: round half to even, like numpy
    unit[0, 0, 1] = [0.0, 1.0, 254.5 / 255]
    want_u8 = (unit * 255).round().astype("uint8")  # diffusers numpy_to_pil
    got_u8 = conv.quantize_pipeline_images(torch.from_numpy(unit).cuda())
    assert got_u8.is_cuda and got_u8.dtype == torch.uint8
    assert np.array_equal(got_u8.cpu().numpy(), want_u8)

    pcm_np = conv.audio_from_spectrogram_images(want_u8, seed=21)  # host uint8 (what PIL would hand over)
    pcm_dev = conv.audio_from_spectrogram_images(torch.from_numpy(want_u8).cuda(), seed=21)  # device uint8
    pcm_float = conv.audio_from_spectrogram_images(torch.from_numpy(unit).cuda(), seed=21)  # the pipeline's float tensor
    assert pcm_np.shape == (2, 441 * 47, 1) and pcm_np.dtype == np.int16
    assert np.array_equal(pcm_np, pcm_dev) and np.array_equal(pcm_np, pcm_float)


def test_sharded_batch_over_rccl_world_size_1(params):
    """e: the product entry point with a process group (backend nccl = RCCL), one rank: same PCM as without a group."""
    import torch.distributed as dist

    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    conv = SpectrogramImageConverter(params, device="cuda")
    tiles = synthetic_tiles_u8(5, 512, 40, seed=8)
    plain = conv.audio_from_spectrogram_images(tiles, seed=77, tiles_per_call=2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0,
                            device_id=torch.device("cuda", torch.cuda.current_device()))
    try:
        sharded = conv.audio_from_spectrogram_images(tiles, seed=77, group=dist.group.WORLD, tiles_per_call=2)
        t = torch.ones(1, device="cuda")
        dist.all_reduce(t)  # the collective bench.py counts ranks with
        assert float(t) == 1.0
    finally:
        dist.destroy_process_group()
    assert sharded.shape == (5, 441 * 39, 1)
    assert np.array_equal(plain, sharded)


def test_plan_is_keyed_by_resolved_device_and_rejects_foreign_tensors(params):
    from riffusion import _hip

    a = _hip.get_plan(params, "cuda")
    b = _hip.get_plan(params, f"cuda:{torch.cuda.current_device()}")
    assert a is b and a.device == torch.device("cuda", torch.cuda.current_device())
    before = torch.cuda.current_device()
    with pytest.raises(_hip.RfxError):
        a.mel_from_waveform(torch.zeros(1, 9000))  # CPU tensor handed to a GPU plan
    with pytest.raises(_hip.RfxError):
        _hip.get_plan(params, "cpu")
    assert torch.cuda.current_device() == before  # plan creation / entry points leave the current device alone
    # non-default stream: work is queued on the tensor's device's CURRENT stream
    s = torch.cuda.Stream()
    wave = synthetic_wave(1, 441 * 30).cuda()
    ref = a.mel_from_waveform(wave)
    with torch.cuda.stream(s):
        out = a.mel_from_waveform(wave)
    s.synchronize()
    assert torch.equal(out, ref)


def test_projection_edge_cases_zero_and_tiny_spectra(O, params):
    """angles / (|angles| + 1e-16) at the bottom of the range: all-zero magnitudes stay exactly zero and finite (0 / 1e-16
    in the reference), and a spectrum 13 orders of magnitude below audio scale still tracks the oracle."""
    from riffusion import _hip

    plan = _hip.get_plan(params, "cuda")
    op = O.params_from(params)
    B, T = 1, 30
    g = torch.Generator().manual_seed(2)
    a0 = torch.rand(B, op.n_stft, T, dtype=torch.complex64, generator=g)
    zero = torch.zeros(B, op.n_stft, T)
    out = plan.griffinlim(plan.pack_magnitudes(zero.cuda()), B, T, 3, 0.99, angles0_slots=plan.pack_complex(a0.cuda())).cpu()
    assert torch.equal(out, torch.zeros_like(out))
    assert torch.equal(O.griffinlim(zero, op, angles0=a0, n_iter=3), torch.zeros_like(out))
    for scale in (1e-6, 1.0, 1e7):
        mag = torch.rand(B, op.n_stft, T, generator=g) * scale
        mag[:, ::7] = 0.0  # exact zeros inside a live spectrum
        want = O.griffinlim(mag, op, angles0=a0, n_iter=4)
        got = plan.griffinlim(plan.pack_magnitudes(mag.cuda()), B, T, 4, 0.99, angles0_slots=plan.pack_complex(a0.cuda())).cpu()
        s = snr_db(want, got)
        print(f"scale {scale:g}: {s:.1f} dB after 4 iterations")
        assert bool(torch.isfinite(got).all()) and s >= 95.0


def test_round_trip_like_the_reference_spectrogram_converter_test(O, golden_dir):
    """reference test/spectrogram_converter_test.py:23-84: audio -> spectrogram -> audio without the image step, on its own
    clip and its own parameter set (20 Hz .. 20 kHz), checking what it checks (channels, frame rate, sample width) plus the
    duration and that the reconstruction's mel spectrogram stays close to the input's."""
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    original = audio_util.PcmSegment.from_wav(os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav")).set_channels(1)
    params = SpectrogramParams(sample_rate=original.frame_rate, stereo=False, step_size_ms=10, min_frequency=20, max_frequency=20000,
                               num_frequencies=512)
    conv = SpectrogramConverter(params=params, device="cuda")
    spectrogram = conv.spectrogram_from_audio(original)
    torch.manual_seed(0)
    result = conv.audio_from_spectrogram(spectrogram, apply_filters=True)
    assert result.channels == original.channels == 1
    assert result.frame_rate == original.frame_rate and result.sample_width == original.sample_width
    assert abs(result.duration_seconds - original.duration_seconds) <= 0.011  # truncated to whole hops (10 ms)
    # reconstruction quality: mel spectrogram of the output vs the input's, gain removed (apply_filters rescales)
    back = conv.spectrogram_from_audio(result)
    n = min(back.shape[-1], spectrogram.shape[-1])
    a, b = spectrogram[..., :n].ravel().astype(np.float64), back[..., :n].ravel().astype(np.float64)
    gain = float(a @ b / (b @ b))
    rel = float(np.linalg.norm(a - gain * b) / np.linalg.norm(a))
    print(f"round trip 20 Hz .. 20 kHz: mel spectrogram of the reconstruction within {rel:.3f} (relative L2) of the input's")
    assert rel < 0.35
