"""
The chirp-z frame engine on the device (csrc/rfx_czt.hip, opt-in: frame_engine="chirp-z"): STFT geometries whose FFT length has a prime
factor above 13 - refused under "auto" - against the CPU oracle, stage by stage and through the drop-in classes.  Three geometries:
an even n_fft at the reference's default durations (42.57 kHz: 17028 = 4 * 9 * 11 * 43), a small even one with a short window
(4.73 kHz: 1892 = 4 * 11 * 43, win 473, hop 47) and an odd, prime one with win == n_fft (10.09 kHz at 100 / 100 ms: 1009).
Gates are the generic engine's (tests/test_gpu_generic_geometry.py).
"""
import numpy as np
import pytest
import torch

from helpers import mask_ill_conditioned_bins, oracle, snr_db, synthetic_tiles_u8, synthetic_wave

pytestmark = pytest.mark.gpu

GEOMETRIES = {
    17028: dict(sample_rate=42570),
    1892: dict(sample_rate=4730, max_frequency=2000),
    1009: dict(sample_rate=10090, padded_duration_ms=100, window_duration_ms=100, max_frequency=4000),
}


@pytest.fixture(scope="module")
def O():
    return oracle()


def _params(n_fft, **extra):
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams(**GEOMETRIES[n_fft], **extra)
    assert p.n_fft == n_fft
    return p


def _plan(p):
    from riffusion import _hip

    plan = _hip.get_plan(p, "cuda", frame_engine="chirp-z")
    assert plan.generic and plan.griffinlim_engine == "chirp-z"
    return plan


@pytest.mark.parametrize("n_fft", sorted(GEOMETRIES))
def test_forward_matches_oracle(O, n_fft):
    p = _params(n_fft)
    assert p.n_fft == n_fft
    op = O.params_from(p)
    plan = _plan(p)
    assert plan.n_stft == n_fft // 2 + 1 and plan.frame_stride % 64 == 0
    wave = synthetic_wave(2, p.hop_length * 57 + 13, seed=n_fft)
    ref = O.stft_complex(wave, op)
    mag, spec, Tn = plan.stft(wave.cuda(), want_mag=True, want_spec=True)
    got = plan.unpack_complex(spec, 2, Tn).cpu()
    assert got.shape == ref.shape and Tn == 1 + (wave.shape[1] + 2 * (n_fft // 2) - n_fft) // p.hop_length
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"n_fft {n_fft} (win {p.win_length}, hop {p.hop_length}): chirp-z STFT rel err {err:.2e} (gate 3e-6)")
    assert err <= 3e-6
    assert float((plan.unpack_magnitudes(mag, 2, Tn).cpu() - ref.abs()).abs().max() / ref.abs().max()) <= 3e-6
    # mel amplitudes: the reference's 1e-4 gates
    mel_ref = O.mel_amplitudes_from_waveform(wave, op)
    mel = plan.mel_from_waveform(wave.cuda()).cpu()
    assert (mel - mel_ref).abs().max() <= 1e-4 * mel_ref.max()
    assert torch.linalg.norm(mel - mel_ref) / torch.linalg.norm(mel_ref) <= 1e-4
    with pytest.raises(RuntimeError):
        plan.mel_from_waveform(torch.zeros(1, n_fft // 2).cuda())  # reflect padding needs more than n_fft/2 samples


@pytest.mark.parametrize("n_fft", sorted(GEOMETRIES))
def test_griffinlim_matches_oracle(O, n_fft):
    p = _params(n_fft)
    assert p.n_fft == n_fft
    op = O.params_from(p)
    plan = _plan(p)
    B, T = 2, 46
    g = torch.Generator().manual_seed(n_fft)
    mag = torch.rand(B, op.n_stft, T, generator=g) * 1000
    a0 = torch.rand(B, op.n_stft, T, dtype=torch.complex64, generator=g)
    S, A = plan.pack_magnitudes(mag.cuda()), plan.pack_complex(a0.cuda())
    for n, floor in ((0, 110.0), (1, 100.0)):  # initial synthesis, first iteration: still well conditioned
        want = O.griffinlim(mag, op, angles0=a0, n_iter=n)
        got = plan.griffinlim(S, B, T, n, 0.99, angles0_slots=A).cpu()
        assert got.shape == want.shape == (B, p.hop_length * (T - 1) + (n_fft & 1))
        s = snr_db(want, got)
        print(f"n_fft {n_fft} chirp-z griffinlim n_iter={n}: {s:.1f} dB (floor {floor:.1f})")
        assert s >= floor
    # four iterations (momentum path): the bins whose `rebuilt - m tprev` is nearly zero masked out (helpers.mask_ill_conditioned_bins)
    want = O.griffinlim(mag, op, angles0=a0, n_iter=4)
    got = plan.griffinlim(S, B, T, 4, 0.99, angles0_slots=A).cpu()
    magm, n_masked = mask_ill_conditioned_bins(O, mag, op, a0, 4)
    wantm = O.griffinlim(magm, op, angles0=a0, n_iter=4)
    gotm = plan.griffinlim(plan.pack_magnitudes(magm.cuda()), B, T, 4, 0.99, angles0_slots=A).cpu()
    sm, s = snr_db(wantm, gotm), snr_db(want, got)
    print(f"n_fft {n_fft} chirp-z griffinlim n_iter=4: {sm:.1f} dB masked ({n_masked} bins; floor 95.0) / {s:.1f} unmasked (floor 45.0)")
    assert sm >= 95.0 and s >= 45.0
    # production RNG path: finite, reproducible per seed
    w1 = plan.griffinlim(S, B, T, 3, 0.99, seed=5)
    w2 = plan.griffinlim(S, B, T, 3, 0.99, seed=5)
    assert bool(torch.isfinite(w1).all()) and torch.equal(w1, w2)


@pytest.mark.parametrize("n_fft", sorted(GEOMETRIES))
def test_seam_matches_oracle_and_is_reproducible(O, n_fft):
    """The torch-level seam with injected initial values (SGD-30 + GL-4) against the oracle, then the production path: three clips
    decoded in one call are byte-equal to the same clips decoded as 1 + 2 with the same seed."""
    from riffusion.spectrogram_converter import SpectrogramConverter

    p = _params(n_fft, num_griffin_lim_iters=4, max_mel_iters=30)
    assert p.n_fft == n_fft
    op = O.params_from(p)
    T = 40
    wave = synthetic_wave(1, p.hop_length * (T - 1) + 3, seed=n_fft)
    mel_ref = O.mel_amplitudes_from_waveform(wave, op)
    Tn = mel_ref.shape[-1]
    g = torch.Generator().manual_seed(1)
    spec0 = torch.rand(1, Tn, op.n_stft, generator=g)
    angles0 = torch.rand(1, op.n_stft, Tn, dtype=torch.complex64, generator=g)
    want = O.waveform_from_mel_amplitudes(mel_ref, op, spec0=spec0, angles0=angles0)
    conv = SpectrogramConverter(p, "cuda", frame_engine="chirp-z")
    got = conv.waveform_from_mel_amplitudes(mel_ref.cuda(), spec0=spec0.cuda(), angles0=angles0.cuda()).cpu()
    s = snr_db(want, got)
    print(f"n_fft {n_fft} chirp-z inverse (SGD-30 + GL-4) {s:.1f} dB (floor 80.0)")
    assert got.shape == want.shape and s >= 80.0
    plan = conv._plan()
    assert plan.griffinlim_engine == "chirp-z"
    mel3 = (torch.rand(3, p.num_frequencies, 24, generator=g) ** 3 * 2e6).cuda()
    whole = plan.waveform_from_mel(mel3, 1, 4, seed=9)
    parts = torch.cat([plan.waveform_from_mel(mel3[:1], 1, 4, seed=9, row_base=0), plan.waveform_from_mel(mel3[1:], 1, 4, seed=9, row_base=1)])
    assert bool(torch.isfinite(whole).all()) and float(whole.abs().max()) > 0 and torch.equal(whole, parts)
    # closed-form InverseMelScale on the same plan (engine dispatch only), where the bank admits it (at the two small geometries
    # many of the 512 filters are narrower than a bin: the closed form refuses a bank with empty filters on every engine)
    assert plan.lstsq_ok or n_fft != 17028
    if plan.lstsq_ok:
        lsq = conv.waveform_from_mel_amplitudes(mel_ref.cuda(), angles0=angles0.cuda(), inverse_mel="lstsq")
        assert lsq.shape == got.shape and bool(torch.isfinite(lsq).all()) and float(lsq.abs().max()) > 0


def test_images_round_trip_at_17028(O):
    """The drop-in classes: tile -> audio (right rate / length), audio -> tile: the oracle's image of the same PCM (its own STFT, mel
    and image codec on the CPU), to within one grey level on at most one pixel in a thousand (the gate of tests/test_oracle_golden.py)."""
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    p = _params(17028, num_griffin_lim_iters=8, max_mel_iters=30)
    assert p.n_fft == 17028 and p.hop_length == 425
    conv = SpectrogramImageConverter(p, device="cuda", frame_engine="chirp-z")
    tiles = synthetic_tiles_u8(1, 512, 60, seed=4)
    pcm = conv.audio_from_spectrogram_images(tiles, seed=1)
    assert pcm.shape == (1, 425 * 59, 1) and pcm.dtype == np.int16 and np.abs(pcm.astype(np.int32)).max() == 32767
    waves = torch.from_numpy(pcm.transpose(0, 2, 1).astype(np.float32))  # (N, C, samples)
    images, _ = conv.spectrogram_images_from_waveforms(waves)
    assert len(images) == 1 and images[0].size == (1 + 425 * 59 // 425, 512)
    want = O.image_u8_from_spectrogram(O.mel_amplitudes_from_waveform(waves[0], O.params_from(p)).numpy(), p.power_for_image)
    got = np.array(images[0].convert("RGB"))
    diff = np.abs(got.astype(int) - want.astype(int))
    print(f"n_fft 17028 chirp-z tile of the decoded PCM vs the oracle's: {int(diff.max())} levels at most, {float((diff == 0).mean()):.5f} of the pixels equal")
    assert got.shape == want.shape and diff.max() <= 1 and (diff == 0).mean() >= 0.999 and want.std() > 10
    image = conv.spectrogram_image_from_audio(audio_util.PcmSegment(pcm[0], 42570))
    assert np.array_equal(np.array(image.convert("RGB")), got)
    assert image.size == images[0].size and SpectrogramParams.from_exif(image.getexif()).sample_rate == 42570


@pytest.mark.parametrize("n_fft", sorted(GEOMETRIES))
def test_auto_still_refuses(n_fft):
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter

    p = _params(n_fft, max_mel_iters=31)  # (a parameter set no other test has planned)
    assert p.n_fft == n_fft
    with pytest.raises(_hip.RfxError, match="prime factor above 13"):
        _hip.get_plan(p, "cuda")
    with pytest.raises(_hip.RfxError, match="prime factor above 13"):
        SpectrogramConverter(p, "cuda").mel_amplitudes_from_waveform(torch.zeros(1, 4 * n_fft))
