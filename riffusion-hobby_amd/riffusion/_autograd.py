"""
Autograd for the forward members of `SpectrogramConverter`: `spectrogram_func`, `mel_scaler` and
`mel_amplitudes_from_waveform` are differentiable in the reference (torchaudio's Spectrogram(power=None), MelScale, torch.abs),
and here their gradients run on the device (include/rfx.h, "BACKWARD of the forward path").

Three `torch.autograd.Function`s over a `_hip.Plan`.  Each forward makes the call the member makes without autograd - the same
bytes - and saves the least it can: the fused function saves the waveform only (the backward re-analyses it; a kept spectrum
would be 2.3 GB at 64 stereo tiles).  The backwards are `once_differentiable`: a double backward raises.
The inverse members (InverseMelScale's SGD, Griffin-Lim) and the loop encode have no backward.
"""
import typing as T

import torch
from torch.autograd.function import once_differentiable


def wants_grad(x: torch.Tensor) -> bool:
    """does a call on `x` have to record a graph?  Otherwise the members make the plain call: same bytes, nothing saved."""
    return torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad


class StftFunction(torch.autograd.Function):
    """(B, Lw) float32 -> (B, n_stft, T) complex64; backward: rfx_stft_backward on torch's complex gradient dL/dRe + i dL/dIm"""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, wave: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        B, Lw = wave.shape
        _, spec, Tn = plan.stft(wave, want_mag=False, want_spec=True)
        ctx.plan, ctx.shape = plan, (B, Lw)
        return plan.unpack_complex(spec, B, Tn)

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, grad: torch.Tensor) -> T.Tuple[None, torch.Tensor]:  # type: ignore[override]
        B, Lw = ctx.shape
        return None, ctx.plan.stft_backward(ctx.plan.pack_complex(grad.to(torch.complex64)), B, Lw)


class MelScaleFunction(torch.autograd.Function):
    """(B, n_stft, T) float32 -> (B, n_mels, T); backward: the filterbank's adjoint (rfx_mel_scale_backward)"""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, lin: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        ctx.plan = plan
        return plan.mel_scale(lin)

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, grad: torch.Tensor) -> T.Tuple[None, torch.Tensor]:  # type: ignore[override]
        return None, ctx.plan.mel_scale_backward(grad)


class MelFromWaveformFunction(torch.autograd.Function):
    """(B, Lw) float32 -> (B, n_mels, T); backward: rfx_mel_from_waveform_backward, which forms the spectrum again"""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, wave: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        ctx.plan = plan
        ctx.save_for_backward(wave)
        return plan.mel_from_waveform(wave)

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, grad: torch.Tensor) -> T.Tuple[None, torch.Tensor]:  # type: ignore[override]
        (wave,) = ctx.saved_tensors
        return None, ctx.plan.mel_from_waveform_backward(wave, grad)


def stft(plan: T.Any, wave: torch.Tensor) -> torch.Tensor:
    return StftFunction.apply(plan, wave)


def mel_scale(plan: T.Any, lin: torch.Tensor) -> torch.Tensor:
    return MelScaleFunction.apply(plan, lin)


def mel_from_waveform(plan: T.Any, wave: torch.Tensor) -> torch.Tensor:
    return MelFromWaveformFunction.apply(plan, wave)
