"""
The closed-form InverseMelScale on the device (csrc/rfx_imel_lstsq.hip; include/rfx.h: rfx_inverse_mel_lstsq,
RFX_CALL_INVERSE_MEL_LSTSQ) and what is built on it: Plan.inverse_mel_lstsq, the fused calls with the flag, the `inverse_mel`
keyword of the converters and --inverse-mel of the CLI.

Shapes, the smallest that can still go wrong: the default plan with B = 3, T = 37 (no multiple of the 16 frames an expand
workgroup stages nor of the 64 lanes of a solve wave; slot-major frames with twice-held bins and padding), the same with
mel_scale_norm = "slaney" (weights that do not sum to one), and 8 kHz with 64 filters, B = 2, T = 21 (plain bin-ordered frames,
fewer filters than one batch of sweep steps times four).

Bounds.  Device against emulator, batch invariance, both copies of a bin, padding, the fused calls against their parts and the
power-of-two scaling are bit equality.  Against torch's float64 lstsq: at most 2 times the distance of torch's own float32 "gels"
on the same input, overall and for the worst single frame (tests/test_imel_lstsq_cpu.py).
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import imel_lstsq_cases as cpu
from imel_lstsq_cases import CANARY, DEVICE_CASES as CASES, _bits, _mel, _params, _plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return cpu.emulator()


_cases = {}


def _case(name):
    """(plan, fb, tables, B, T, mel on the host, device slots, emulator result, float64 lstsq, float32 lstsq): once per case"""
    if name not in _cases:
        kw, B, T = CASES[name]
        plan = _plan(**kw)
        op, cp, fb = cpu.bank(**kw)
        assert torch.equal(fb, plan.melfb) and plan.lstsq_ok
        _, tables = cpu.report(cp, fb, tables=True)
        mel = _mel(plan.n_mels, B, T)
        slots = plan.inverse_mel_lstsq(mel.cuda())
        torch.cuda.synchronize()
        _cases[name] = (plan, fb, tables, B, T, mel, slots)
    return _cases[name]


def test_layouts_are_what_the_shapes_were_chosen_for():
    assert not _case("default")[0].generic and not _case("norm_slaney")[0].generic and _case("8khz_64")[0].generic
    assert _case("default")[0].frame_stride == 9408 and _case("8khz_64")[0].frame_stride % 64 == 0


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_emulator_and_meets_the_gate(emu, name):  # noqa: F811
    plan, fb, tables, B, T, mel, slots = _case(name)
    got = plan.unpack_magnitudes(slots, B, T).cpu()
    want = cpu.emu_run(emu, fb, tables, mel)
    assert got.shape == want.shape == (B, plan.n_stft, T)
    assert _bits(got) == _bits(want)
    ref = cpu.lstsq_reference(fb, mel, torch.float64)
    torch32 = cpu.distances(cpu.lstsq_reference(fb, mel, torch.float32), ref)
    ours = cpu.distances(got, ref)
    print(f"{name}: device rel-L2 {ours[0]:.2e} (worst frame {ours[1]:.2e}); torch float32 gels {torch32[0]:.2e} (worst frame {torch32[1]:.2e})")
    assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1]


@pytest.mark.parametrize("name", list(CASES))
def test_padding_is_zero_and_both_copies_of_a_bin_are_equal(name):
    plan, fb, tables, B, T, mel, slots = _case(name)
    # where every bin lives: pack a frame whose bin f holds f + 1 (padding packs as 0)
    ramp = (torch.arange(plan.n_stft, dtype=torch.float32, device="cuda") + 1.0).reshape(1, -1, 1)
    pos_bin = plan.pack_magnitudes(ramp).reshape(-1).round().long() - 1  # -1: padding
    assert pos_bin.numel() == plan.frame_stride and int((pos_bin >= 0).sum()) >= plan.n_stft
    frames = slots.reshape(B * T, plan.frame_stride)
    assert bool((frames[:, pos_bin < 0] == 0).all()) and _bits(frames[:, pos_bin < 0]) == bytes(4 * B * T * int((pos_bin < 0).sum()))
    plain = plan.unpack_magnitudes(slots, B, T).permute(0, 2, 1).reshape(B * T, plan.n_stft)
    held = pos_bin >= 0
    assert _bits(frames[:, held]) == _bits(plain[:, pos_bin[held]])  # every copy of every bin is the bin's value
    twice = int(held.sum()) - plan.n_stft
    assert twice == (0 if plan.generic else 440)
    assert bool(torch.isfinite(frames).all()) and bool((frames >= 0).all())


@pytest.mark.parametrize("name", list(CASES))
def test_workspace_canary_and_row_alone(name):
    plan, fb, tables, B, T, mel, slots = _case(name)
    lib = plan.lib
    need = lib.rfx_inverse_mel_lstsq_workspace_bytes(plan.handle, B, T)
    assert need >= B * plan.n_mels * T * 4
    ws = torch.full((need + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((B * T * plan.frame_stride + CANARY // 4,), -7.0, dtype=torch.float32, device="cuda")
    d_mel = mel.cuda()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.rfx_inverse_mel_lstsq(plan.handle, d_mel.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((out[B * T * plan.frame_stride:] == -7.0).all())
    assert _bits(out[:B * T * plan.frame_stride]) == _bits(slots)
    assert lib.rfx_inverse_mel_lstsq(plan.handle, d_mel.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need - 1, stream) == -3
    # row 1 converted alone
    alone = plan.inverse_mel_lstsq(d_mel[1:2].contiguous())
    assert _bits(alone) == _bits(slots.reshape(B, T * plan.frame_stride)[1])


@pytest.mark.parametrize("max_value", [1.0, 1e20])
@pytest.mark.parametrize("name", list(CASES))
def test_power_of_two_scaling_is_exact(name, max_value):
    plan = _case(name)[0]
    mel = _mel(plan.n_mels, 1, 5, max_value=max_value).cuda()
    base = plan.inverse_mel_lstsq(mel)
    assert bool((base > 0).any()) and bool(torch.isfinite(base).all())
    for k in (-12, 9):
        assert _bits(plan.inverse_mel_lstsq(mel * 2.0 ** k)) == _bits(base * 2.0 ** k), k


# ---- the fused calls ---------------------------------------------------------------------------------------------------------------
def _tiles_u8(N, M, T, seed=11):
    return np.random.default_rng(seed).integers(0, 256, size=(N, M, T, 3), dtype=np.uint8)


@pytest.mark.parametrize("stereo", [False, True])
def test_fused_calls_equal_their_parts(stereo):
    from riffusion import _hip
    from riffusion.util import image_util

    plan = _plan()
    N, T, n_iter, seed, max_value = (2 if stereo else 3), 37, 4, 21, 30e6
    C = 2 if stereo else 1
    B = N * C
    tiles = torch.from_numpy(_tiles_u8(N, plan.n_mels, T)).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, max_value), lambda: image_util.decode_lut(0.25, max_value))
    mel = plan.image_decode(tiles, stereo, lut)
    for row_base, hint in ((0, 0.0), (2 * C, max_value)):
        lin = plan.inverse_mel_lstsq(mel)
        wave2 = plan.griffinlim(lin, B, T, n_iter, 0.99, seed=seed + 1, row_base=row_base, magnitude_hint=hint)
        wave1 = plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, row_base=row_base, magnitude_hint=hint, lstsq=True)
        assert _bits(wave1) == _bits(wave2), (row_base, hint)
        sgd = plan.waveform_from_mel(mel, C, n_iter, 0.99, seed=seed, row_base=row_base, magnitude_hint=hint)
        assert _bits(sgd) != _bits(wave1)
        pcm2, peak2 = plan.pcm16(wave2, C, normalize=True)
        pcm1, peak1 = plan.audio_from_image(tiles, stereo, lut, n_iter, 0.99, seed=seed, clip_base=row_base // C, magnitude_hint=hint, lstsq=True)
        assert _bits(pcm1) == _bits(pcm2) and _bits(peak1) == _bits(peak2), (row_base, hint)
    assert _hip.call_options(lstsq=True).flags == 1 and _hip.call_options().flags == 0


def test_the_two_stages_refuse_the_flag():
    from riffusion import _hip

    plan = _plan()
    lib = plan.lib
    B, T = 1, 22
    flagged = _hip.call_options(lstsq=True)
    mel = torch.ones((B, plan.n_mels, T), device="cuda")
    slots = torch.zeros((B * T, plan.frame_stride), device="cuda")
    ws = torch.empty(max(lib.rfx_inverse_mel_workspace_bytes(plan.handle, B, T), lib.rfx_griffinlim_workspace_bytes(plan.handle, B, T)),
                     dtype=torch.uint8, device="cuda")
    wave = torch.zeros((B, lib.rfx_griffinlim_output_samples(plan.handle, T)), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.rfx_inverse_mel_ex(plan.handle, mel.data_ptr(), B, T, 1, None, 0, slots.data_ptr(), ws.data_ptr(), ws.numel(), stream, ctypes.byref(flagged))
    assert rc == -1 and b"flags" in lib.rfx_last_error()
    rc = lib.rfx_griffinlim_ex(plan.handle, slots.data_ptr(), None, 0, B, T, 1, 0.99, wave.data_ptr(), ws.data_ptr(), ws.numel(), stream,
                               ctypes.byref(flagged), None)
    assert rc == -1 and b"flags" in lib.rfx_last_error()
    unknown = _hip.RfxCallOptions(24, 2, 0, 0.0, 0.0)
    rc = lib.rfx_waveform_from_mel_ex(plan.handle, mel.data_ptr(), B, T, 1, 0, 1, 0.99, wave.data_ptr(), ws.data_ptr(), ws.numel(), stream, ctypes.byref(unknown))
    assert rc == -1 and b"flags" in lib.rfx_last_error()


def test_a_singular_bank_is_refused_before_any_launch():
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter

    plan = _plan(num_frequencies=1024)
    lib = plan.lib
    assert lib.rfx_plan_lstsq_ok(plan.handle) == 0 and not plan.lstsq_ok
    assert lib.rfx_inverse_mel_lstsq_workspace_bytes(plan.handle, 1, 22) == 0
    B, T = 1, 22
    sentinel = 12345.0
    mel = torch.ones((B, plan.n_mels, T), device="cuda")
    wave = torch.full((B, lib.rfx_griffinlim_output_samples(plan.handle, T)), sentinel, device="cuda")
    need = lib.rfx_waveform_from_mel_workspace_bytes(plan.handle, B, T)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    flagged = _hip.call_options(lstsq=True)
    rc = lib.rfx_waveform_from_mel_ex(plan.handle, mel.data_ptr(), B, T, 1, 0, 1, 0.99, wave.data_ptr(), ws.data_ptr(), need, stream, ctypes.byref(flagged))
    assert rc == -1 and b"pivot" in lib.rfx_last_error()
    slots = torch.full((B * T, plan.frame_stride), sentinel, device="cuda")
    assert lib.rfx_inverse_mel_lstsq(plan.handle, mel.data_ptr(), B, T, slots.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert b"pivot" in lib.rfx_last_error()
    tiles = torch.zeros((1, plan.n_mels, T, 3), dtype=torch.uint8, device="cuda")
    lut = torch.ones(256, device="cuda")
    peak = torch.full((1,), sentinel, device="cuda")
    pcm = torch.full((1, wave.shape[1], 1), 77, dtype=torch.int16, device="cuda")
    need_img = lib.rfx_audio_from_image_workspace_bytes(plan.handle, 1, 0, T)
    ws_img = torch.full((need_img,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.rfx_audio_from_image_u8_ex(plan.handle, tiles.data_ptr(), 1, T, 0, lut.data_ptr(), 0, 1, 0.99, 1, peak.data_ptr(), pcm.data_ptr(),
                                        ws_img.data_ptr(), need_img, stream, ctypes.byref(flagged))
    assert rc == -1 and b"pivot" in lib.rfx_last_error()
    torch.cuda.synchronize()
    # nothing was launched: outputs and workspaces are as they were
    assert bool((wave == sentinel).all()) and bool((slots == sentinel).all()) and bool((pcm == 77).all()) and bool((peak == sentinel).all())
    assert bool((ws == 0xA5).all()) and bool((ws_img == 0xA5).all())
    # the Python layer raises ValueError with the library's reason
    conv = SpectrogramConverter(_params(num_frequencies=1024), device="cuda")
    with pytest.raises(ValueError, match="pivot"):
        conv.waveform_from_mel_amplitudes(mel, seed=1, inverse_mel="lstsq")
    with pytest.raises(ValueError, match="pivot"):
        plan.inverse_mel_lstsq(mel)


# ---- Python ------------------------------------------------------------------------------------------------------------------------
TILES = ["og_beat", "agile", "marim"]


def _golden_tiles(golden_dir, width=40):
    from riffusion.util import image_util

    out = []
    for name in TILES:
        with Image.open(os.path.join(golden_dir, f"{name}.png")) as im:
            out.append(np.ascontiguousarray(np.asarray(image_util.rgb_array_from_image(im)))[:, 100:100 + width])
    return np.stack(out)


def test_batch_decode_with_the_keyword(golden_dir):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    conv = SpectrogramImageConverter(_params(num_griffin_lim_iters=4), device="cuda")
    tiles = _golden_tiles(golden_dir)
    assert tiles.shape == (3, 512, 40, 3)
    results = [conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel="lstsq", tiles_per_call=k) for k in (1, 2, 3)]
    assert results[0].dtype == np.int16 and results[0].shape[0] == 3 and np.abs(results[0]).max() > 0
    assert results[0].tobytes() == results[1].tobytes() == results[2].tobytes()
    pcm, err = conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel="lstsq", return_error=True)
    assert pcm.tobytes() == results[0].tobytes() and err.shape == (3,) and np.isfinite(err).all() and (err > 0).all()
    sgd = conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel="sgd")
    default = conv.audio_from_spectrogram_images(tiles, seed=7)
    assert sgd.tobytes() == default.tobytes() and sgd.tobytes() != results[0].tobytes()
    # with the other options: filters, a resize, float waveforms
    filtered = conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel="lstsq", apply_filters=True)
    assert filtered.shape == results[0].shape and filtered.tobytes() != results[0].tobytes()
    resized = conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel="lstsq", size=(32, 512))
    assert resized.shape[1] == 441 * 31
    wave = conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel="lstsq", return_waveform=True)
    assert wave.shape == (3, 1, 441 * 39) and wave.dtype == np.float32
    from riffusion.util import audio_util

    seq = conv.audio_from_spectrogram_image_sequence(tiles, crossfade_s=0.1, apply_filters=False, seed=7, inverse_mel="lstsq")
    want = audio_util.stitch_segments([audio_util.PcmSegment(clip, 44100) for clip in results[0]], 0.1)
    assert bytes(seq.get_array_of_samples()) == bytes(want.get_array_of_samples())
    for bad in ("x", "", None):
        with pytest.raises(ValueError, match="inverse_mel"):
            conv.audio_from_spectrogram_images(tiles, seed=7, inverse_mel=bad)
    with pytest.raises(ValueError, match="inverse_mel"):
        conv.converter.waveform_from_mel_amplitudes(torch.ones((1, 512, 24)), seed=1, inverse_mel="x")


def test_cli_flag_reaches_the_call(golden_dir, tmp_path, monkeypatch):
    from riffusion import cli
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    tile = Image.fromarray(_golden_tiles(golden_dir)[0], mode="RGB")
    tile.getexif().update(_params(num_griffin_lim_iters=2).to_exif().items())
    src = tmp_path / "tiles"
    src.mkdir()
    tile.save(str(src / "t0.png"), exif=tile.getexif(), format="PNG")
    seen = []
    real = SpectrogramImageConverter.audio_from_spectrogram_images

    def spy(self, *a, **kw):
        seen.append(kw.get("inverse_mel"))
        return real(self, *a, **kw)

    monkeypatch.setattr(SpectrogramImageConverter, "audio_from_spectrogram_images", spy)
    cli.main(["image-to-audio", "--image", str(src / "t0.png"), "--audio", str(tmp_path / "one.wav"), "--inverse-mel", "lstsq"])
    cli.main(["images-to-audio-batch", "--image-dir", str(src), "--output-dir", str(tmp_path / "wavs"), "--inverse-mel", "lstsq"])
    cli.main(["images-to-audio-batch", "--image-dir", str(src), "--output-dir", str(tmp_path / "wavs_sgd")])
    assert seen == ["lstsq", "lstsq", "sgd"]
    assert os.path.getsize(tmp_path / "one.wav") > 44 and os.listdir(tmp_path / "wavs") == ["t0.wav"]
    with pytest.raises(SystemExit):
        cli.main(["image-to-audio", "--image", "a", "--audio", "b", "--inverse-mel", "x"])
