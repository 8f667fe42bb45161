"""
Reference gradients of the forward path by torch.autograd through oracle/riffusion_oracle.py's own forward - `stft_complex`,
`torch.abs`, `mel_scale`, `mel_amplitudes_from_waveform`, untouched - in float64 and in float32.  The oracle builds its window and
its filterbank in float32; for the float64 figures the two builders are wrapped for the duration of a call so that they return the
same float32 VALUES as float64 tensors (torch.stft and matmul want one dtype), and restored afterwards.
"""
import contextlib

import torch

import riffusion_oracle as O


@contextlib.contextmanager
def _oracle_dtype(dtype):
    if dtype == torch.float32:
        yield
        return
    window, bank = O.hann_window, O.mel_filterbank
    O.hann_window = lambda p: window(p).to(dtype)
    O.mel_filterbank = lambda p: bank(p).to(dtype)
    try:
        yield
    finally:
        O.hann_window, O.mel_filterbank = window, bank


def stft(wave: torch.Tensor, op, dtype=torch.float64) -> torch.Tensor:
    """the oracle's complex STFT of (B, Lw) `wave` in `dtype`"""
    with _oracle_dtype(dtype):
        return O.stft_complex(wave.detach().to(dtype), op)


def mel_from_waveform_grad(wave: torch.Tensor, g_mel: torch.Tensor, op, dtype=torch.float64) -> torch.Tensor:
    """d <mel_amplitudes_from_waveform(wave), g_mel> / d wave: (B, Lw) in `dtype`"""
    w = wave.detach().to(dtype).requires_grad_(True)
    with _oracle_dtype(dtype):
        O.mel_amplitudes_from_waveform(w, op).backward(g_mel.detach().to(dtype))
    return w.grad


def stft_grad(wave: torch.Tensor, g_spec: torch.Tensor, op, dtype=torch.float64) -> torch.Tensor:
    """the gradient torch gives the waveform for the complex gradient `g_spec` (B, n_stft, T) of its STFT (dL/dRe + i dL/dIm)"""
    w = wave.detach().to(dtype).requires_grad_(True)
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    with _oracle_dtype(dtype):
        O.stft_complex(w, op).backward(g_spec.detach().to(cdtype))
    return w.grad


def mel_scale_grad(lin: torch.Tensor, g_mel: torch.Tensor, op, dtype=torch.float64) -> torch.Tensor:
    """d <mel_scale(lin), g_mel> / d lin: (B, n_stft, T) in `dtype`"""
    x = lin.detach().to(dtype).requires_grad_(True)
    O.mel_scale(x, O.mel_filterbank(op).to(dtype)).backward(g_mel.detach().to(dtype))
    return x.grad


def loss_grad(wave: torch.Tensor, target: torch.Tensor, op, dtype=torch.float64) -> torch.Tensor:
    """the gradient of 0.5 || mel_amplitudes_from_waveform(wave) - target ||^2"""
    w = wave.detach().to(dtype).requires_grad_(True)
    with _oracle_dtype(dtype):
        (0.5 * (O.mel_amplitudes_from_waveform(w, op) - target.detach().to(dtype)).pow(2).sum()).backward()
    return w.grad
