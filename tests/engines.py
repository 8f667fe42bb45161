"""
The Griffin-Lim engines the device tests run on (TEST INFRASTRUCTURE ONLY), and what the tests of the guided, held, masked and loop
calls share besides: the clip of tests/golden/, the guided calls' shape, exact comparison on bytes.
"""
import os
import wave

import numpy as np
import torch

CLIP2 = "clip_2_start_103694_ms_duration_5678_ms"
B, T = 3, 33  # the guided, held and masked calls: two whole groups of 16 frames plus one frame per row; runs that cross row boundaries

ENGINES = {  # name: (rfx_plan_griffinlim_engine's answer, SpectrogramParams keywords, get_plan keywords)
    "specialised": ("specialised", dict(), dict()),
    "row-family-48k": ("row-family", dict(sample_rate=48000), dict()),
    "generic-11025": ("generic", dict(sample_rate=11025, max_frequency=5512), dict()),
    "chirp-z-1009": ("chirp-z", dict(sample_rate=10090, padded_duration_ms=100, window_duration_ms=100, max_frequency=4000), dict(frame_engine="chirp-z")),
}
# the same with the specialised engine in both of its Griffin-Lim forms
ENGINES_BY_FORM = {"specialised-runs": ("specialised", dict(), dict(gl_form="runs")), "specialised-frames": ("specialised", dict(), dict(gl_form="frames")),
                   **{name: row for name, row in ENGINES.items() if name != "specialised"}}
LOOPING = ["specialised", "row-family-48k", "generic-11025"]  # the engines that take loop calls


def plan_for(name):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    engine, kw, plan_kw = (ENGINES.get(name) or ENGINES_BY_FORM[name])
    p = SpectrogramParams(**kw)
    plan = _hip.get_plan(p, "cuda", **plan_kw)
    assert plan.griffinlim_engine == engine, (name, plan.griffinlim_engine)
    return p, plan


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def stft64(x, op, O):
    return torch.stft(x.double(), n_fft=op.n_fft, hop_length=op.hop_length, win_length=op.win_length, window=O.hann_window(op).double(),
                      center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)


def clip2_segment(golden_dir, frames=64, start=44100):
    """(oracle, default oracle params, (2, L) float32 samples of `frames` frames of the clip from sample `start`)"""
    import riffusion_oracle as O
    from riffusion.spectrogram_params import SpectrogramParams

    op = O.params_from(SpectrogramParams())
    with wave.open(os.path.join(golden_dir, CLIP2 + ".wav")) as w:
        assert w.getframerate() == op.sample_rate and w.getsampwidth() == 2 and w.getnchannels() == 2, w.getparams()
        pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    seg = pcm[start:start + op.hop_length * (frames - 1)].astype(np.float32)
    return O, op, torch.from_numpy(seg.T.copy())  # (2, L)
