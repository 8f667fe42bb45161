"""
The oracle of the time stretch (include/rfx.h, "TIME STRETCH"), shared by tests/test_vocoder_cpu.py and tests/test_gpu_vocoder.py:
a transcription of torchaudio.functional.phase_vocoder as torchaudio.transforms.TimeStretch calls it, statement by statement,
parameterised by dtype - float64 is the reference of every gate, float32 is torch's own error, which sets the gate.

The time steps are stated here and not left to torch: step i lies at the double product i * rate, i = 0 .. frames(T, rate) - 1,
`torch.arange(n, dtype=float64) * rate` - include/rfx.h's and csrc/rfx_vocoder_core.h's definition, x = (double)i * rate,
i0 = floor(x), alpha = (float)(x - i0), the same numbers on every backend.  That is the one departure from torchaudio, in both dtypes:
torchaudio takes `torch.arange(0, T, rate)` in the spectrogram's real dtype.  What torch's own arange computes for step i (float32 or
float64, on the CPU or a device) is not the product: where i * rate lies within rounding of an integer it may land on the other
side of it (2/3 at i = 21: 13.999999999999998 against 14.0) and so pick the neighbouring frame pair - the same magnitude to
rounding, since alpha is then next to 0 or 1, but another phase increment, and from that step on another phase trajectory.
tools/survey_vocoder_steps.py counts the rates at which that happens (profiles/time_stretch_steps.txt); that ambiguity is torch's
and not what is under test.  Only the COUNT of steps is still arange's: `frames` is the length of torch.arange(0, T, rate), which
rfx_phase_vocoder_frames is held to (tests/test_vocoder_cpu.py: test_frame_count_is_torch_aranges).
"""
import math

import torch


def _cdtype(dtype):
    return torch.complex64 if dtype == torch.float32 else torch.complex128


def frames(T, rate):
    """frames of a stretched spectrogram of T frames: the length of torch.arange(0, T, rate)"""
    return len(torch.arange(0, T, rate, dtype=torch.float64))


def steps(T, rate, device=None):
    """the positions of the output steps, float64: (double)i * rate for i < frames(T, rate) - one rounding each, never a running sum"""
    return torch.arange(frames(T, rate), dtype=torch.float64, device=device) * rate


def pairs(T, rate, dtype=torch.float64, device=None):
    """(i0 (n,) int64, alpha (n,) `dtype`) of the steps: the first frame of a step's pair and the weight of the second, as
    `phase_vocoder` below takes them"""
    time_steps = steps(T, rate, device)
    return time_steps.long(), (time_steps % 1.0).to(dtype)


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
    i0, alphas = pairs(spec.size(-1), rate, dtype, spec.device)  # torchaudio: time_steps.long(), (time_steps % 1.0), (time_steps + 1).long()
    phase_0 = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    spec_0 = spec.index_select(-1, i0)
    spec_1 = spec.index_select(-1, i0 + 1)
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
