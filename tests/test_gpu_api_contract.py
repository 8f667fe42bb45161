"""GPU tests of the boundary contract: errors, re-entrancy, plan cache, edge shapes."""
import ctypes
import time
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest
import torch

import helpers
from helpers import synthetic_tiles_u8, synthetic_wave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def params():
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramParams()


def test_plan_cache_and_cheap_construction(params):
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    SpectrogramConverter(params, device="cuda")._plan()
    assert _hip.get_plan(params, "cuda") is _hip.get_plan(SpectrogramParams(), "cuda")
    t0 = time.perf_counter()
    for _ in range(50):  # the reference's server builds a converter per request (server.py:159)
        SpectrogramConverter(SpectrogramParams(), device="cuda")._plan()
    assert (time.perf_counter() - t0) / 50 < 2e-3


def test_errors_match_reference_behaviour(params):
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(params, device="cuda")
    with pytest.raises(RuntimeError, match="Padding size should be less than"):  # torch.stft's reflect-pad error
        conv.mel_amplitudes_from_waveform(torch.zeros(1, 8820))
    conv.mel_amplitudes_from_waveform(torch.zeros(1, 8821))  # smallest legal input
    with pytest.raises(ValueError, match="mel bins"):  # torchaudio InverseMelScale's check
        conv.waveform_from_mel_amplitudes(torch.zeros(1, 100, 16))
    # other sample rates run on the generic engine; only FFT lengths with a prime factor above 13 are refused, with a reason
    assert SpectrogramConverter(SpectrogramParams(sample_rate=48000), device="cuda").mel_amplitudes_from_waveform(torch.zeros(1, 30000)).shape == (1, 512, 63)
    with pytest.raises(_hip.RfxError, match="prime factor"):
        SpectrogramConverter(SpectrogramParams(sample_rate=42570), device="cuda").mel_amplitudes_from_waveform(torch.zeros(1, 30000))
    plan = _hip.get_plan(params, "cuda")
    with pytest.raises(_hip.RfxError, match="multiple of channels_per_clip"):
        plan.inverse_mel(torch.zeros(3, 512, 8, device="cuda"), 2)
    # too small a workspace is an error code, not a crash
    S = torch.zeros(2 * 24, plan.frame_stride, device="cuda")
    out = torch.empty(2, 441 * 23, device="cuda")
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    rc = plan.lib.rfx_griffinlim(plan.handle, S.data_ptr(), None, 0, 2, 24, 2, ctypes.c_float(0.99), out.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _hip.current_stream())
    assert rc == -3 and b"workspace" in plan.lib.rfx_last_error()


def test_edge_shapes(params):
    """Shortest legal clips (22 frames: reflect padding needs > 8820 samples), odd batches, and the
    reference's own failure below that."""
    import riffusion_oracle as O
    from riffusion import _hip

    plan = _hip.get_plan(params, "cuda")
    op = O.params_from(params)
    with pytest.raises(_hip.RfxError, match="Padding size should be less than"):
        plan.griffinlim(torch.zeros(10, plan.frame_stride, device="cuda"), 1, 10, 2, 0.99)
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        O.griffinlim(torch.rand(1, op.n_stft, 10), op, n_iter=2)
    # zero iterations = one ISTFT: legal for any T >= 2
    g = torch.Generator().manual_seed(0)
    mag = torch.rand(1, op.n_stft, 2, generator=g)
    a0 = torch.rand(1, op.n_stft, 2, dtype=torch.complex64, generator=g)
    ref0 = O.griffinlim(mag, op, angles0=a0, n_iter=0)
    got0 = plan.griffinlim(plan.pack_magnitudes(mag.cuda()), 1, 2, 0, 0.99, angles0_slots=plan.pack_complex(a0.cuda())).cpu()
    assert got0.shape == ref0.shape == (1, 441) and (got0 - ref0).abs().max() / ref0.abs().max() < 1e-5
    for T, B in ((22, 1), (23, 3), (31, 2)):
        g = torch.Generator().manual_seed(T)
        mag = torch.rand(B, op.n_stft, T, generator=g) * 100
        a0 = torch.rand(B, op.n_stft, T, dtype=torch.complex64, generator=g)
        ref = O.griffinlim(mag, op, angles0=a0, n_iter=2)
        got = plan.griffinlim(plan.pack_magnitudes(mag.cuda()), B, T, 2, 0.99, angles0_slots=plan.pack_complex(a0.cuda())).cpu()
        assert got.shape == ref.shape == (B, 441 * (T - 1))
        assert (got - ref).abs().max() / ref.abs().max() < 1e-4


def test_shared_converter_is_reentrant(params):
    """One converter used from a ThreadPool, as the reference's batch CLI does (cli.py:172-204)."""
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    ic = SpectrogramImageConverter(params, device="cuda")
    tiles = synthetic_tiles_u8(6, 512, 24, seed=3)

    def job(i):
        return ic.audio_from_spectrogram_images(tiles[i : i + 1], seed=100 + i)

    serial = [job(i) for i in range(6)]
    with ThreadPool(3) as pool:
        threaded = pool.map(job, range(6))
    for a, b in zip(serial, threaded):
        assert np.array_equal(a, b)
    # and seeds matter / repeat
    assert not np.array_equal(serial[0], ic.audio_from_spectrogram_images(tiles[0:1], seed=999))
    assert np.array_equal(serial[0], ic.audio_from_spectrogram_images(tiles[0:1], seed=100))


def test_forward_batch_equals_per_clip(params):
    from riffusion import _hip

    plan = _hip.get_plan(params, "cuda")
    wave = synthetic_wave(5, 441 * 37 + 100, seed=12).cuda()
    full = plan.mel_from_waveform(wave)
    for i in range(5):
        assert torch.equal(full[i : i + 1], plan.mel_from_waveform(wave[i : i + 1]))


def test_cli_round_trips_like_the_reference_tests(golden_dir, tmp_path):
    """reference test/image_to_audio_test.py:40-67 and test/audio_to_image_test.py:57-99 through our CLI."""
    import os

    from PIL import Image

    from riffusion import cli
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    png = os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms_stereo.png")
    wav_out = str(tmp_path / "out.wav")
    cli.main(["image-to-audio", "--image", png, "--audio", wav_out, "--device", "cuda"])
    seg = audio_util.PcmSegment.from_wav(wav_out)
    assert seg.frame_rate == 44100 and seg.channels == 2
    assert abs(seg.duration_seconds - 5.678) < 0.010 + 1.0 / 100  # duration within one hop of the clip (reference: 10 ms)
    png_out = str(tmp_path / "out.png")
    cli.main(["audio-to-image", "--audio", os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav"),
              "--image", png_out, "--stereo"])
    im = Image.open(png_out)
    assert im.mode == "RGB" and im.size == (568, 512) and np.all(np.array(im)[..., 0] == 0)
    assert SpectrogramParams.from_exif(im.getexif()) == SpectrogramParams(stereo=True)
    gold = np.array(Image.open(png).convert("RGB"))
    assert np.abs(np.array(im).astype(int) - gold.astype(int)).max() <= 1
    # batch command: three copies of a tile decode in one GPU call
    tiles = tmp_path / "tiles"
    tiles.mkdir()
    for i in range(3):
        Image.open(os.path.join(golden_dir, "og_beat_64.png")).save(str(tiles / f"t{i}.png"))
    cli.main(["images-to-audio-batch", "--image-dir", str(tiles), "--output-dir", str(tmp_path / "wavs")])
    assert sorted(os.listdir(tmp_path / "wavs")) == ["t0.wav", "t1.wav", "t2.wav"]


def test_cli_other_sample_rates_and_batch_flags(golden_dir, tmp_path):
    """The reference takes the sample rate from the input file (cli.py:43): a 48 kHz clip goes through the generic engine, and
    `audio-to-images-batch` resamples mixed-rate files to --sample-rate, skips what it cannot read and defaults to stereo jpg
    (cli.py:134-204)."""
    import os

    from PIL import Image

    from riffusion import cli
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    src = audio_util.PcmSegment.from_wav(os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav"))
    wav48 = str(tmp_path / "clip48.wav")
    src.set_frame_rate(48000).export(wav48, format="wav")
    png48 = str(tmp_path / "clip48.png")
    cli.main(["audio-to-image", "--audio", wav48, "--image", png48])
    im = Image.open(png48)
    p = SpectrogramParams.from_exif(im.getexif())
    assert p.sample_rate == 48000 and p.n_fft == 19200 and im.size[1] == 512 and im.size[0] == 1 + int(48000 * 250400 / 44100) // 480
    back = str(tmp_path / "back48.wav")
    cli.main(["image-to-audio", "--image", png48, "--audio", back])
    seg = audio_util.PcmSegment.from_wav(back)
    assert seg.frame_rate == 48000 and seg.channels == 1 and abs(seg.duration_seconds - 5.678) < 0.02

    clips = tmp_path / "clips"
    clips.mkdir()
    src.export(str(clips / "a.wav"), format="wav")
    src.set_frame_rate(22050).set_channels(1).export(str(clips / "b.wav"), format="wav")
    (clips / "broken.wav").write_bytes(b"not a wav file")
    out = tmp_path / "images"
    cli.main(["audio-to-images-batch", "--audio-dir", str(clips), "--output-dir", str(out)])
    assert sorted(os.listdir(out)) == ["a.jpg", "b.jpg"]  # the unreadable file is skipped, like the reference does
    for name in ("a.jpg", "b.jpg"):
        with Image.open(str(out / name)) as im:
            q = SpectrogramParams.from_exif(im.getexif())
            assert q.stereo is True and q.sample_rate == 44100 and im.size[1] == 512 and abs(im.size[0] - 568) <= 1
    cli.main(["audio-to-images-batch", "--audio-dir", str(clips), "--output-dir", str(tmp_path / "mono"), "--mono",
              "--image-extension", "png", "--limit", "1"])
    assert os.listdir(tmp_path / "mono") == ["a.png"]


# ---- the workspace of an inverse call comes from the call's own options (rfx_*_workspace_bytes_ex) -----------------------------------------
_EX_PLANS = {"specialised": dict(), "row-family-48k": dict(sample_rate=48000), "generic-11025": dict(sample_rate=11025, max_frequency=5512)}
_EX_B, _EX_T = 2, 41  # the smallest loop of these geometries is 40 frames (41 at 11025 Hz), the reflect rule needs 22


@pytest.mark.parametrize("what", ["loop+start", "loop+guide", "guide"])
@pytest.mark.parametrize("name", sorted(_EX_PLANS))
def test_workspace_query_by_options_is_sharp(name, what):
    """Combinations that had no query of their own: the size the library answers for the call's options is the size the entry
    asks for, to the byte - one byte less is RFX_ERR_WORKSPACE before any launch, the size itself runs."""
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    plan = _hip.get_plan(SpectrogramParams(**_EX_PLANS[name]), "cuda")
    assert plan.griffinlim_engine == name.rsplit("-", 1)[0] and plan.n_stft <= 10240
    lib, B, T = plan.lib, _EX_B, _EX_T
    loop = what.startswith("loop")
    L = plan.output_samples(T, loop)
    guide = synthetic_wave(B, L, seed=303).cuda()
    guided = dict(d_guide=guide.data_ptr(), guide_stride=L, guide_samples=L)
    fields = {"loop+start": dict(loop=1, start=1), "loop+guide": dict(guided, loop=1), "guide": guided}[what]
    plain = lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)
    need = helpers.need(lib, "griffinlim", plan.handle, B, T, **fields)
    assert plain > 0 and helpers.need(lib, "griffinlim", plan.handle, B, T) == plain == lib.rfx_griffinlim_workspace_bytes_ex(plan.handle, B, T, None)
    # a guide is staged in buffers the first launch leaves free: it adds nothing; the start's bytes lie behind the call's, looped or not
    assert helpers.need(lib, "griffinlim", plan.handle, B, T, **guided) == plain
    loop_need = helpers.need(lib, "griffinlim", plan.handle, B, T, loop=1)
    assert helpers.need(lib, "griffinlim", plan.handle, B, T, **dict(guided, loop=1)) == loop_need > 0
    assert helpers.need(lib, "griffinlim", plan.handle, B, T, loop=1, start=1) == loop_need + helpers.need(lib, "griffinlim", plan.handle, B, T, start=1) - plain
    assert need == {"loop+start": helpers.need(lib, "griffinlim", plan.handle, B, T, loop=1, start=1), "loop+guide": loop_need, "guide": plain}[what]

    opt = _hip.RfxStartCallOptions(struct_size=ctypes.sizeof(_hip.RfxStartCallOptions), **fields)
    stream = _hip.current_stream(torch.device("cuda"))
    S = plan.pack_magnitudes((torch.rand(B, plan.n_stft, T, generator=torch.Generator().manual_seed(11)) * 1000.0).cuda())

    def sharp(run, need, out, sentinel):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert run(ws.data_ptr(), need - 1) == -3 and b"workspace too small" in lib.rfx_last_error()
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
        assert run(ws.data_ptr(), need) == 0, lib.rfx_last_error()
        torch.cuda.synchronize()
        assert not bool((out == sentinel).all())

    out = torch.full((B, L), 123.0, device="cuda")
    sharp(lambda ws, n: lib.rfx_griffinlim_ex(plan.handle, S.data_ptr(), None, 5, B, T, 1, 0.99, out.data_ptr(), ws, n, stream, ctypes.byref(opt), None),
          need, out, 123.0)
    assert bool(torch.isfinite(out).all())
    if name != "specialised" or what != "loop+start":
        return
    # the fused entries, on the default plan
    mel = torch.rand(B, plan.n_mels, T, generator=torch.Generator().manual_seed(1)).cuda() * 1e6
    need_w = helpers.need(lib, "waveform_from_mel", plan.handle, B, T, **fields)
    assert need_w == helpers.need(lib, "waveform_from_mel", plan.handle, B, T, loop=1) + need - loop_need
    out.fill_(123.0)
    sharp(lambda ws, n: lib.rfx_waveform_from_mel_ex(plan.handle, mel.data_ptr(), B, T, 1, 3, 1, 0.99, out.data_ptr(), ws, n, stream, ctypes.byref(opt)),
          need_w, out, 123.0)
    need_a = helpers.need(lib, "audio_from_image", plan.handle, B, 0, T, **fields)
    assert need_a == helpers.need(lib, "audio_from_image", plan.handle, B, 0, T, loop=1) + need - loop_need
    tiles = torch.randint(0, 256, (B, plan.n_mels, T, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    pcm = torch.full((B, L, 1), 77, dtype=torch.int16, device="cuda")
    peak = torch.zeros(B, device="cuda")
    sharp(lambda ws, n: lib.rfx_audio_from_image_u8_ex(plan.handle, tiles.data_ptr(), B, T, 0, lut.data_ptr(), 3, 1, 0.99, 1, peak.data_ptr(), pcm.data_ptr(),
                                                        ws, n, stream, ctypes.byref(opt)), need_a, pcm, 77)
