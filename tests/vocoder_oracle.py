"""
The oracle of the time stretch (include/rfx.h, "TIME STRETCH"), shared by tests/test_vocoder_cpu.py and tests/test_gpu_vocoder.py:
a transcription of torchaudio.functional.phase_vocoder as torchaudio.transforms.TimeStretch calls it, statement by statement,
parameterised by dtype - float64 is the reference of every gate, float32 is torch's own error, which sets the gate.

One departure, in both dtypes: the time steps are taken in float64 (torchaudio takes them in the spectrogram's real dtype).  At a
near-integer i * rate a float32 arange can pick another frame pair than a float64 one; that ambiguity is torch's and not what is
under test, and the library forms i * rate in double.
"""
import math

import torch


def _cdtype(dtype):
    return torch.complex64 if dtype == torch.float32 else torch.complex128


def frames(T, rate):
    """frames of a stretched spectrogram of T frames: the length of torch.arange(0, T, rate)"""
    return len(torch.arange(0, T, rate, dtype=torch.float64))


def phase_advance(hop_length, n_stft, dtype=torch.float64, device=None):
    """torchaudio.transforms.TimeStretch's buffer: linspace(0, pi * hop_length, n_freq)[..., None]"""
    return torch.linspace(0, math.pi * hop_length, n_stft, dtype=dtype, device=device)[..., None]


def phase_vocoder(X, rate, hop_length, dtype=torch.float64):
    """(..., n_stft, T) complex -> (..., n_stft, ceil(T / rate)) complex of `dtype`'s precision, on X's device"""
    if rate == 1.0:
        return X.to(_cdtype(dtype))
    spec = X.to(_cdtype(dtype))
    shape = spec.size()
    spec = spec.reshape([-1] + list(shape[-2:]))
    adv = phase_advance(hop_length, shape[-2], dtype, spec.device)
    time_steps = torch.arange(0, spec.size(-1), rate, dtype=torch.float64, device=spec.device)
    alphas = (time_steps % 1.0).to(dtype)
    phase_0 = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    spec_0 = spec.index_select(-1, time_steps.long())
    spec_1 = spec.index_select(-1, (time_steps + 1).long())
    angle_0, angle_1 = spec_0.angle(), spec_1.angle()
    norm_0, norm_1 = spec_0.abs(), spec_1.abs()
    phase = angle_1 - angle_0 - adv
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + adv
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    out = torch.polar(mag, phase_acc)
    return out.reshape(shape[:-2] + out.shape[-2:])
