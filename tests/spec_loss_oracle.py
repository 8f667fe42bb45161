"""
Reference values of the fused spectral losses (include/rfx.h, "FUSED SPECTRAL LOSSES") by torch.autograd, in float64 and in float32,
shared by tests/test_spectral_loss_cpu.py and tests/test_gpu_spectral_loss.py.  Both losses are stated with torch's own operations:

    convergence   = torch.linalg.vector_norm(|X| - M) / torch.linalg.vector_norm(M)                         per row
    log_magnitude = mean | torch.log(torch.clamp(|X|, min=f)) - torch.log(torch.clamp(M, min=f)) |          per row

The STFT is the oracle's: `riffusion_oracle.stft_complex` through tests/mel_backward_oracle.py for the plain form,
`loop_oracle.loop_stft` for the loop form.  Two things are given:

* `end_to_end`: the losses and the waveform gradient of sum_b g_sc[b] convergence[b] + g_lg[b] log_magnitude[b] through that STFT;
* `from_spectrum`: the same gradient FROM A GIVEN SPECTRUM - X is a leaf, dL/dX is evaluated there (sign and clamp decisions taken
  on the given values), and pushed through the STFT's backward (`mel_backward_oracle.stft_grad` or its loop twin).
"""
import torch

import loop_oracle
import mel_backward_oracle as MBO
import riffusion_oracle as O


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def losses_of_magnitudes(a, M, f):
    """(convergence (B,), log_magnitude (B,) or None) of magnitudes a against the target M, both (B, n_stft, T), in a's dtype"""
    sc = torch.linalg.vector_norm(a - M, dim=(1, 2)) / torch.linalg.vector_norm(M, dim=(1, 2))
    if f is None:
        return sc, None
    return sc, (torch.log(torch.clamp(a, min=f)) - torch.log(torch.clamp(M, min=f))).abs().mean(dim=(1, 2))


def _weighted(a, M, f, g_sc, g_lg):
    sc, lg = losses_of_magnitudes(a, M, f)
    total = (g_sc.to(a.dtype) * sc).sum()
    if lg is not None and g_lg is not None:
        total = total + (g_lg.to(a.dtype) * lg).sum()
    return sc, lg, total


def stft(wave, op, loop, dtype=torch.float64):
    """the oracle's complex STFT of (B, Lw) `wave` in `dtype`, plain or circular; differentiable when `wave` is"""
    if loop:
        return loop_oracle.loop_stft(O, wave, op, dtype)
    with MBO._oracle_dtype(dtype):
        return O.stft_complex(wave.to(dtype), op)


def end_to_end(wave, M, op, f, g_sc, g_lg, loop=False, dtype=torch.float64):
    """(convergence, log_magnitude or None, waveform gradient (B, Lw)) through the oracle's STFT in `dtype`"""
    w = wave.detach().to(dtype).requires_grad_(True)
    sc, lg, total = _weighted(stft(w, op, loop, dtype).abs(), M.detach().to(dtype), f, g_sc, g_lg)
    total.backward()
    return sc.detach(), None if lg is None else lg.detach(), w.grad


def spectrum_grad(X, M, f, g_sc, g_lg, dtype=torch.float64):
    """dL/dX (torch's convention, dL/dRe + i dL/dIm) at the given spectrum X (B, n_stft, T), in `dtype`"""
    x = X.detach().to(_cdtype(dtype)).requires_grad_(True)
    _weighted(x.abs(), M.detach().to(dtype), f, g_sc, g_lg)[2].backward()
    return x.grad


def loop_stft_grad(wave, g_spec, op, dtype=torch.float64):
    """the loop twin of `mel_backward_oracle.stft_grad`: the waveform gradient of the circular STFT for the complex gradient g_spec"""
    w = wave.detach().to(dtype).requires_grad_(True)
    loop_oracle.loop_stft(O, w, op, dtype).backward(g_spec.detach().to(_cdtype(dtype)))
    return w.grad


def from_spectrum(wave, X, M, op, f, g_sc, g_lg, loop=False, dtype=torch.float64):
    """the waveform gradient from the given spectrum X: dL/dX there, then the STFT's backward (the waveform gives the shape only:
    the transform is linear)"""
    gx = spectrum_grad(X, M, f, g_sc, g_lg, dtype)
    return loop_stft_grad(wave, gx, op, dtype) if loop else MBO.stft_grad(wave, gx, op, dtype)
