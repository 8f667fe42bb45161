"""
CPU checks of loop FORWARD calls (include/rfx.h: rfx_stft_loop and the other *_loop forward entries): a row is one period of
P = hop T samples, frame t, element i reads x[(hop t + i - n_fft // 2) mod P].

* The length rule, rfx_debug_loop_samples, at four parameter sets: legal lengths pass; P - 1, P + 1, one hop below the smallest
  legal length, 0 and a negative length are refused and the message names the nearest legal lengths (the one below and the one
  above; below the smallest legal length there is none below, and the message says "none").  `_hip.check_loop_samples` agrees case
  for case.
* The read positions: tests/emu/rfx_loop_fwd_emu.cpp walks `loop_read_index` of csrc/rfx_loop_core.h the way each engine's forward
  kernel forms a frame's positions - generic / chirp-z, row family, the specialised engine's hop blocks, and the sliding prefetch of
  its fused kernel over runs of frames - and must equal tests/loop_oracle.py's `_scatter_index` at T = the smallest frame count and
  one more; no position handed to the wrap may leave [-P, 2 P).
* The emulator and a `main` of its own (tests/emu/rfx_loop_fwd_emu_main.cpp) are also built as a stand-alone program with
  -fsanitize=address,undefined and run here: nothing sanitized is loaded into Python.
* The CLI flags and the keyword checks that need no device.
"""
import ctypes
import subprocess
import types

import numpy as np
import pytest

import emu_build
import loop_oracle

EMU_SRC = "rfx_loop_fwd_emu.cpp"
EMU_MAIN = "rfx_loop_fwd_emu_main.cpp"

# (sample_rate, n_fft, win, hop): the default, 48 kHz, 11.025 kHz, one odd n_fft
PARAMS = [(44100, 17640, 4410, 441), (48000, 19200, 4800, 480), (11025, 4410, 1102, 110), (10010, 1001, 251, 26)]
IDS = ["default", "48k", "11025", "odd-nfft"]


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.emu_loop_samples_valid.argtypes = lib.emu_loop_samples_frames.argtypes = [i, i, ll]
    lib.emu_loop_samples_below.argtypes = lib.emu_loop_samples_above.argtypes = [i, i, ll]
    lib.emu_loop_samples_below.restype = lib.emu_loop_samples_above.restype = ll
    lib.emu_fwd_gather_gen.argtypes = lib.emu_fwd_gather_fam.argtypes = [i, i, i, i, i, vp]
    lib.emu_fwd_gather_blocks.argtypes = [i, i, i, vp]
    lib.emu_fwd_gather_run.argtypes = [i, i, i, i, i, vp]
    return lib


def _geo(n_fft, win, hop):
    return types.SimpleNamespace(n_fft=n_fft, win_length=win, hop_length=hop)


# ---- the length rule -------------------------------------------------------------------------------------------------------------------------

def _lengths(n_fft, hop):
    """(legal lengths, [(refused length, nearest legal below or None, nearest legal above)])"""
    need = -(-n_fft // hop)
    lo, big = hop * need, hop * 512
    legal = [lo, big]
    refused = [(lo - 1, None, lo), (lo + 1, lo, lo + hop), (big - 1, big - hop, big), (big + 1, big, big + hop), (hop * (need - 1), None, lo),
               (0, None, lo), (-1, None, lo), (-hop, None, lo)]
    return legal, refused


@pytest.mark.parametrize("rate,n_fft,win,hop", PARAMS, ids=IDS)
def test_length_rule_and_its_message(lib, emu, rate, n_fft, win, hop):
    from riffusion import _hip

    cp = _hip.RfxParams(rate, n_fft, win, hop, 512, 200)
    legal, refused = _lengths(n_fft, hop)
    assert legal[0] >= n_fft > legal[0] - hop
    for P in legal:
        assert lib.rfx_debug_loop_samples(ctypes.byref(cp), P) == 0
        _hip.check_loop_samples(hop, n_fft, P)
        assert _hip.loop_nearest_samples(hop, n_fft, P) == (P, P)
        assert emu.emu_loop_samples_valid(hop, n_fft, P) == 1 and emu.emu_loop_samples_frames(hop, n_fft, P) == P // hop
        assert emu.emu_loop_samples_below(hop, n_fft, P) == P == emu.emu_loop_samples_above(hop, n_fft, P)
    for Lw, below, above in refused:
        assert lib.rfx_debug_loop_samples(ctypes.byref(cp), Lw) == -1, Lw
        msg = lib.rfx_last_error().decode()
        assert f"got {Lw}:" in msg and f"{above} ({above // hop} frames) above" in msg, msg
        assert (f"{below} ({below // hop} frames) below" if below else "none below") in msg, msg
        with pytest.raises(ValueError) as e:
            _hip.check_loop_samples(hop, n_fft, Lw)
        assert str(e.value) == msg
        assert emu.emu_loop_samples_valid(hop, n_fft, Lw) == 0 == emu.emu_loop_samples_frames(hop, n_fft, Lw)
        assert emu.emu_loop_samples_below(hop, n_fft, Lw) == (below or 0) and emu.emu_loop_samples_above(hop, n_fft, Lw) == above
        assert _hip.loop_nearest_samples(hop, n_fft, Lw) == (below or 0, above)
    assert lib.rfx_debug_loop_samples(None, legal[0]) == -1 == lib.rfx_debug_loop_nearest_samples(None, legal[0], None, None)
    # a loop decode's output length is a legal input and gives its frames back
    for T in (legal[0] // hop, 512):
        assert lib.rfx_debug_loop_frames(ctypes.byref(cp), T) == 0 == lib.rfx_debug_loop_samples(ctypes.byref(cp), hop * T)


def test_entries_answer_zero_or_refuse_without_a_plan(lib):
    assert lib.rfx_stft_loop_frames(None, 17640) == 0
    assert lib.rfx_mel_loop_workspace_bytes(None, 1, 17640) == 0 == lib.rfx_image_from_waveform_loop_workspace_bytes(None, 1, 0, 17640)
    assert lib.rfx_image_from_pcm16_clips_loop_workspace_bytes(None, 1, 0, 17640) == 0 == lib.rfx_spectral_error_loop_workspace_bytes(None, 1, 40)
    assert lib.rfx_stft_loop(None, None, 1, 17640, None, None, None) == -1 and b"rfx_stft_loop" in lib.rfx_last_error()
    assert lib.rfx_mel_from_waveform_loop(None, None, 1, 17640, None, None, 0, None) == -1 and b"rfx_mel_from_waveform_loop" in lib.rfx_last_error()
    assert lib.rfx_image_from_waveform_loop(None, None, 1, 0, 17640, None, None, None, None, 0, None) == -1
    assert b"rfx_image_from_waveform_loop" in lib.rfx_last_error()
    assert lib.rfx_spectral_error_loop(None, None, None, 1, 40, None, None, 0, None) == -1 and b"rfx_spectral_error_loop" in lib.rfx_last_error()
    assert lib.rfx_spectral_error_loop(None, None, None, 0, 40, None, None, 0, None) == 0  # B == 0 is a no-op, as the plain entry's


# ---- the read positions ------------------------------------------------------------------------------------------------------------------------

def _cases():
    for (rate, n_fft, win, hop), name in zip(PARAMS, IDS):
        need = -(-n_fft // hop)
        for T in (need, need + 1):
            yield pytest.param(n_fft, win, hop, T, id=f"{name}-T{T}")


@pytest.mark.parametrize("n_fft,win,hop,T", list(_cases()))
def test_every_engine_reads_the_oracles_samples(emu, n_fft, win, hop, T):
    left = (n_fft - win) // 2
    want = loop_oracle._scatter_index(_geo(n_fft, win, hop), T).numpy()[left:left + win].astype(np.int32)  # (win, T)
    assert want.min() == 0 and want.max() == hop * T - 1
    assert any((np.diff(want[:, t]) < 0).any() for t in range(T))  # some window reaches across the loop point
    fam = n_fft == 4 * win and win % 10 == 0
    blocks = fam and win == 10 * hop and n_fft // 2 - left == 5 * hop
    for t in range(T):
        idx = np.full(win + 8, -77, np.int32)
        assert emu.emu_fwd_gather_gen(n_fft, win, hop, T, t, idx.ctypes.data) == 0
        assert np.array_equal(idx[:win], want[:, t]) and (idx[win:] == -77).all(), t
        if fam:
            got = np.full(win + 8, -77, np.int32)
            assert emu.emu_fwd_gather_fam(n_fft, win, hop, T, t, got.ctypes.data) == 0
            assert np.array_equal(got, idx), t
        if blocks:
            got = np.full(win + 8, -77, np.int32)
            assert emu.emu_fwd_gather_blocks(hop, T, t, got.ctypes.data) == 0
            assert np.array_equal(got, idx), t
    if not blocks:
        return
    # the fused kernel's runs: every split of the row the host can choose (1 .. 64 frames per workgroup, the last run short), and the
    # unequal runs of the skewed dispatch; the look-ahead past a run's end - past the row's end for the last run - stays in range
    for slide in (1, 0):
        for per in (1, 2, 3, 7, 16, T - 1, T, 64):
            for f0 in range(0, T, per):
                f1 = min(T, f0 + per)
                run = np.full((f1 - f0) * win + 8, -77, np.int32)
                assert emu.emu_fwd_gather_run(hop, T, f0, f1, slide, run.ctypes.data) == 0, (per, f0)
                assert np.array_equal(run[:-8].reshape(f1 - f0, win), want[:, f0:f1].T) and (run[-8:] == -77).all(), (per, f0)


def test_sanitized_stand_alone_emulator():
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program, in the
    environment the test itself runs in; the sanitizers' runtimes are linked statically, so the program carries them itself"""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr


# ---- the keywords and flags that need no device ------------------------------------------------------------------------------------------------

def test_converter_refuses_a_clip_that_is_no_whole_loop_with_lengths_in_samples_and_ms():
    from riffusion.spectrogram_converter import LoopLengthError, SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(), device="cpu")
    conv.check_loop_samples(512 * 441)
    conv.check_loop_samples(40 * 441)
    with pytest.raises(LoopLengthError) as e:
        conv.check_loop_samples(250400)  # the 5678 ms golden clips
    msg = str(e.value)
    assert "250047 samples (5670.000 ms) below" in msg and "250488 samples (5680.000 ms) above" in msg and "nothing is trimmed or padded" in msg
    with pytest.raises(ValueError, match=r"none below and 17640 samples \(400.000 ms\) above"):
        conv.check_loop_samples(17199)
    import torch

    with pytest.raises(LoopLengthError):  # before any device work: this converter has no device
        conv.mel_amplitudes_from_waveform(torch.zeros(1, 250400), loop=True)


def test_keywords_default_to_false_and_return_loop_error_needs_loop():
    import inspect

    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    for fn in (_hip.Plan.stft, _hip.Plan.mel_from_waveform, _hip.Plan.image_from_waveform, _hip.Plan.image_from_pcm_clips, _hip.Plan.spectral_error,
               SpectrogramConverter.spectrogram_from_audio, SpectrogramConverter.mel_amplitudes_from_waveform, SpectrogramConverter.spectral_convergence,
               SpectrogramImageConverter.spectrogram_image_from_audio, SpectrogramImageConverter.spectrogram_images_from_waveforms,
               SpectrogramImageConverter.spectrogram_images_from_audio_clips):
        assert inspect.signature(fn).parameters["loop"].default is False, fn
    assert inspect.signature(SpectrogramImageConverter.audio_from_spectrogram_images).parameters["return_loop_error"].default is False
    conv = SpectrogramImageConverter(SpectrogramParams(), device="cpu")
    tiles = np.zeros((1, 512, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="return_loop_error=True is the circular spectral error of a loop decode: it needs loop=True"):
        conv.audio_from_spectrogram_images(tiles, return_loop_error=True)
    with pytest.raises(ValueError, match="loop does not go with return_error=True"):
        conv.audio_from_spectrogram_images(tiles, loop=True, return_error=True)
    with pytest.raises(ValueError, match="return_loop_error does not go with `group`"):
        conv.audio_from_spectrogram_images(tiles, loop=True, return_loop_error=True, group=True)


def test_cli_flags():
    from riffusion import cli

    p = cli.build_parser()
    assert vars(p.parse_args(["audio-to-image", "--audio", "a.wav", "--image", "b.png"]))["loop"] is False
    assert vars(p.parse_args(["audio-to-image", "--audio", "a.wav", "--image", "b.png", "--loop"]))["loop"] is True
    args = vars(p.parse_args(["image-to-audio", "--image", "b.png", "--audio", "a.wav", "--loop", "--print-error"]))
    assert args["loop"] is True and args["print_error"] is True
    assert vars(p.parse_args(["image-to-audio", "--image", "b.png", "--audio", "a.wav"]))["print_error"] is False


def test_cli_print_error_needs_loop(capsys):
    from riffusion import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["image-to-audio", "--image", "b.png", "--audio", "a.wav", "--print-error"])
    assert e.value.code == 2 and "--print-error needs --loop" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--print-error needs --loop"):
        cli.image_to_audio(image="b.png", audio="a.wav", print_error=True)
