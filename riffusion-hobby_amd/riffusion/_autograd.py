"""
Autograd for the forward members of `SpectrogramConverter`: `spectrogram_func`, `mel_scaler` and
`mel_amplitudes_from_waveform` are differentiable in the reference (torchaudio's Spectrogram(power=None), MelScale, torch.abs),
and here their gradients run on the device (include/rfx.h, "BACKWARD of the forward path").

Three `torch.autograd.Function`s over a `_hip.Plan`.  Each forward makes the call the member makes without autograd - the same
bytes - and saves the least it can: the fused function saves the waveform only (the backward re-analyses it; a kept spectrum
would be 2.3 GB at 64 stereo tiles).  The backwards are `once_differentiable`: a double backward raises.
The iterative inverse members (InverseMelScale's SGD, Griffin-Lim) and the loop encode have no backward.

A fourth function, `SpectralLossFunction`, is the pair of the multi-resolution STFT loss - spectral convergence and log-magnitude L1 -
fused with the transform (include/rfx.h, "FUSED SPECTRAL LOSSES"): the forward leaves three double sums per row, the backward is the
fused backward with another per-bin factor.  It serves the circular STFT too: the loop STFT's only backward.

A fifth, `IstftFunction`, is the inverse spectrogram (include/rfx.h, "INVERSE SPECTROGRAM"): complex STFT -> audio, plain and loop.  The
map is linear, so it saves nothing and its backward is the adjoint.

A sixth, `InverseMelLstsqFunction`, is the closed-form InverseMelScale (`inverse_mel_scaler(..., inverse_mel="lstsq")`; include/rfx.h,
rfx_inverse_mel_lstsq_backward), differentiable as torchaudio >= 2.1's relu(lstsq(...)) is: a linear map and a relu.  It saves the mel
input only; the relu's mask is formed again in the backward.  With it a loss on audio reaches a model's mel tiles:
mel -> inverse_mel_scaler(lstsq) -> torch.polar(., phase) -> waveform_from_spectrogram -> spectral_losses.

A seventh, `GuidedDecodeFunction`, is that chain with the phase of a reference clip as ONE call: the phase-guided decode at zero
Griffin-Lim iterations with the closed-form inverse, `waveform_from_mel_amplitudes(mel, guide=clip, inverse_mel="lstsq",
griffin_lim_iters=0)` (include/rfx.h, "GUIDED DECODE, BACKWARD").  It saves `mel` and the guide; forward and backward stay in slot
layout from end to end - no (B, n_stft, T) tensor, real or complex, is formed.  The guide is a constant.
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


def convergence_from_sums(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """`SpectrogramConverter.convergence_from_sums` (the converter module imports this one)"""
    from riffusion.spectrogram_converter import SpectrogramConverter

    return SpectrogramConverter.convergence_from_sums(num, den)


def loss_coefficients(sums: torch.Tensor, n: int, g_sc: torch.Tensor, g_lg: torch.Tensor, log_floor: float) -> torch.Tensor:
    """the (B, 2) float32 coefficients rfx_spectral_loss_backward takes, from the saved sums and the incoming gradients, with torch
    operations on the sums' device (nothing is read back): c_sc = g_sc / sqrt(num den) where num > 0 and den > 0, else 0 - the zero
    subgradient torch.linalg.vector_norm gives at 0, and no gradient against a silent target - and c_lg = g_lg / n (0 without a floor)"""
    num, den = sums[:, 0], sums[:, 1]
    live = (num > 0) & (den > 0)
    root = torch.sqrt(torch.where(live, num * den, torch.ones_like(num)))
    c_sc = torch.where(live, g_sc.to(torch.float64) / root, torch.zeros_like(num))
    c_lg = g_lg.to(torch.float64) / n if log_floor > 0 else torch.zeros_like(num)
    return torch.stack([c_sc, c_lg], dim=1).to(torch.float32)


class SpectralLossFunction(torch.autograd.Function):
    """(B, Lw) float32 waveform, target magnitude slots -> (convergence, log_magnitude), each (B,) float64 (include/rfx.h, "FUSED
    SPECTRAL LOSSES").  Saves the waveform and the (B, 3) sums and keeps a reference to the target slots; the backward forms the
    per-row coefficients on the device and calls rfx_spectral_loss_backward, which re-analyses the waveform.  The target gets no
    gradient: one that requires grad raises."""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, wave: torch.Tensor, slots: torch.Tensor, log_floor: float, loop: bool,  # type: ignore[override]
                n: int) -> T.Tuple[torch.Tensor, torch.Tensor]:
        sums = plan.spectral_loss_sums(wave, slots, log_floor, loop)
        ctx.plan, ctx.slots, ctx.log_floor, ctx.loop, ctx.n = plan, slots, log_floor, loop, n
        ctx.save_for_backward(wave, sums)
        return convergence_from_sums(sums[:, 0], sums[:, 1]), sums[:, 2] / n

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, g_sc: torch.Tensor, g_lg: torch.Tensor):  # type: ignore[override]
        wave, sums = ctx.saved_tensors
        coef = loss_coefficients(sums, ctx.n, g_sc, g_lg, ctx.log_floor)
        return None, ctx.plan.spectral_loss_backward(wave, ctx.slots, coef, ctx.log_floor, ctx.loop), None, None, None, None


def spectral_losses(plan: T.Any, wave: torch.Tensor, slots: torch.Tensor, log_floor: float, loop: bool) -> T.Tuple[torch.Tensor, torch.Tensor]:
    """(convergence, log_magnitude) of (B, Lw) `wave` against the target `slots`; log_floor 0.0: no log term (log_magnitude is all
    zero).  With a waveform that requires grad the pair carries a grad_fn; otherwise the forward call alone, nothing saved."""
    if isinstance(slots, torch.Tensor) and slots.requires_grad:
        raise RuntimeError("spectral_losses: the target receives no gradient; detach it")
    n = plan.n_stft * plan._forward_frames(int(wave.shape[-1]), wave.shape, loop)
    if wants_grad(wave):
        return SpectralLossFunction.apply(plan, wave, slots, log_floor, loop, n)
    sums = plan.spectral_loss_sums(wave.detach(), slots, log_floor, loop)
    return convergence_from_sums(sums[:, 0], sums[:, 1]), sums[:, 2] / n


class IstftFunction(torch.autograd.Function):
    """(B, n_stft, T) complex64 -> (B, L) float32, torch.istft(center=True) or with `loop` the circular synthesis (include/rfx.h,
    "INVERSE SPECTROGRAM").  The map is linear: nothing is saved, the backward is its adjoint (rfx_istft_backward) and returns torch's
    complex gradient dL/dRe + i dL/dIm."""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, spec: torch.Tensor, loop: bool) -> torch.Tensor:  # type: ignore[override]
        B, _, Tn = spec.shape
        ctx.plan, ctx.shape, ctx.loop = plan, (B, Tn), loop
        return plan.istft(plan.pack_complex(spec), B, Tn, loop)

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, grad: torch.Tensor) -> T.Tuple[None, torch.Tensor, None]:  # type: ignore[override]
        B, Tn = ctx.shape
        slots = ctx.plan.istft_backward(grad.to(torch.float32).contiguous(), B, Tn, ctx.loop)
        return None, ctx.plan.unpack_complex(slots, B, Tn), None


def istft(plan: T.Any, spec: torch.Tensor, loop: bool = False) -> torch.Tensor:
    """the (B, L) waveform of a (B, n_stft, T) complex64 spectrogram; with a spectrum that requires grad the result carries a
    grad_fn, otherwise the forward call alone"""
    if wants_grad(spec):
        return IstftFunction.apply(plan, spec, loop)
    B, _, Tn = spec.shape
    return plan.istft(plan.pack_complex(spec.detach()), B, Tn, loop)


class InverseMelLstsqFunction(torch.autograd.Function):
    """(B, n_mels, T) float32 -> (B, n_stft, T): the closed-form InverseMelScale, relu(fb G^-1 mel).  Saves `mel` only; the backward
    (rfx_inverse_mel_lstsq_backward) forms the relu's mask again from it, bit for bit the forward's."""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, mel: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        B, _, Tn = mel.shape
        ctx.plan = plan
        ctx.save_for_backward(mel)
        return plan.unpack_magnitudes(plan.inverse_mel_lstsq(mel), B, Tn)

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, grad: torch.Tensor) -> T.Tuple[None, torch.Tensor]:  # type: ignore[override]
        (mel,) = ctx.saved_tensors
        return None, ctx.plan.inverse_mel_lstsq_backward(mel, ctx.plan.pack_magnitudes(grad.to(torch.float32).contiguous()))


def inverse_mel_lstsq(plan: T.Any, mel: torch.Tensor) -> torch.Tensor:
    """the (B, n_stft, T) closed-form InverseMelScale of (B, n_mels, T) `mel`; with a `mel` that requires grad the result carries a
    grad_fn, otherwise the forward call alone, nothing saved"""
    if wants_grad(mel):
        return InverseMelLstsqFunction.apply(plan, mel)
    B, _, Tn = mel.shape
    return plan.unpack_magnitudes(plan.inverse_mel_lstsq(mel.detach()), B, Tn)


class GuidedDecodeFunction(torch.autograd.Function):
    """(B, n_mels, T) float32 mel, (B, Lg) float32 guide -> (B, L) float32: ISTFT(relu(lstsq(mel)) a / |a|), a = STFT(guide) - the
    guided decode with no Griffin-Lim iteration, the bytes of `Plan.waveform_from_mel(..., lstsq=True, guide=guide, n_iter=0)`.  Saves
    `mel` and the guide; the backward (rfx_waveform_from_mel_guided_backward) analyses the guide again and forms the relu's mask
    again.  The guide gets no gradient."""

    @staticmethod
    def forward(ctx: T.Any, plan: T.Any, mel: torch.Tensor, guide: torch.Tensor, loop: bool, seed: int) -> torch.Tensor:  # type: ignore[override]
        ctx.plan, ctx.loop = plan, loop
        ctx.save_for_backward(mel, guide)
        return plan.waveform_from_mel(mel, int(mel.shape[0]), 0, 0.99, seed=seed, lstsq=True, guide=guide, loop=loop)

    @staticmethod
    @once_differentiable
    def backward(ctx: T.Any, grad: torch.Tensor) -> T.Tuple[None, torch.Tensor, None, None, None]:  # type: ignore[override]
        mel, guide = ctx.saved_tensors
        return None, ctx.plan.waveform_from_mel_guided_backward(mel, guide, grad.to(torch.float32).contiguous(), ctx.loop), None, None, None


def guided_decode(plan: T.Any, mel: torch.Tensor, guide: torch.Tensor, loop: bool, seed: int) -> torch.Tensor:
    """the (B, L) zero-iteration guided decode of a (B, n_mels, T) `mel` that requires grad; a guide that requires grad raises, as
    the spectral losses' target does"""
    if guide.requires_grad:
        raise RuntimeError("waveform_from_mel_amplitudes: the guide receives no gradient; detach it")
    return GuidedDecodeFunction.apply(plan, mel, guide, loop, seed)


def stft(plan: T.Any, wave: torch.Tensor) -> torch.Tensor:
    return StftFunction.apply(plan, wave)


def mel_scale(plan: T.Any, lin: torch.Tensor) -> torch.Tensor:
    return MelScaleFunction.apply(plan, lin)


def mel_from_waveform(plan: T.Any, wave: torch.Tensor) -> torch.Tensor:
    return MelFromWaveformFunction.apply(plan, wave)
