"""
The oracle of the inverse spectrogram (include/rfx.h, "INVERSE SPECTROGRAM"), shared by tests/test_istft_cpu.py and
tests/test_gpu_istft.py: torch.istft as torchaudio's InverseSpectrogram calls it, the circular synthesis of tests/loop_oracle.py,
and their gradients by torch.autograd, in float64 (the reference of every gate) and float32 (torch's own error, which sets the gate).
`p` is an OracleParams (oracle/riffusion_oracle.py: params_from), `O` the oracle module.
"""
import torch

import loop_oracle


def _cdtype(dtype):
    return torch.complex64 if dtype == torch.float32 else torch.complex128


def samples(p, T, loop=False):
    """samples per row of T frames: torch.istft's length, hop (T - 1) (+ 1 for an odd n_fft), or the period hop T of a loop"""
    return p.hop_length * T if loop else p.hop_length * (T - 1) + p.n_fft % 2


def istft(O, X, p, dtype=torch.float64, loop=False):
    """(B, n_stft, T) complex -> (B, L)"""
    if loop:
        return loop_oracle.loop_istft(O, X, p, dtype)
    return torch.istft(X.to(_cdtype(dtype)), n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=O.hann_window(p).to(dtype),
                       center=True, normalized=False, onesided=True)


def stft(O, x, p, dtype=torch.float64, loop=False):
    """(B, L) -> (B, n_stft, T): torch.stft(center=True, reflect) or the circular analysis"""
    if loop:
        return loop_oracle.loop_stft(O, x, p, dtype)
    return torch.stft(x.to(dtype), n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=O.hann_window(p).to(dtype), center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)


def istft_grad(O, X, g, p, dtype=torch.float64, loop=False):
    """the gradient of sum(istft(X) * g) with respect to X, torch's convention dL/dRe + i dL/dIm: (B, n_stft, T) complex"""
    leaf = X.to(_cdtype(dtype)).clone().requires_grad_(True)
    istft(O, leaf, p, dtype, loop).backward(g.to(dtype))
    return leaf.grad.detach()


def adjoint_defect(y, g, X, G):
    """| <y, g> - Re <X, G> | / | <y, g> | accumulated in float64: y = istft(X) (B, L), G the gradient for g.  Re <X, G> counts every
    one-sided bin once with G in torch's convention, which carries the weights c_k."""
    lhs = float((y.double() * g.double()).sum())
    rhs = float((X.real.double() * G.real.double() + X.imag.double() * G.imag.double()).sum())
    return abs(lhs - rhs) / abs(lhs), lhs, rhs


def loss_through_istft_grad(O, X, target_mag, p, dtype=torch.float64, length=None, log_floor=None):
    """the gradient with respect to X of the sum over rows of the spectral convergence of the waveform istft(X), cut or zero-padded
    to `length`, against target magnitudes (B, n_stft, T') - the composed oracle of waveform_from_spectrogram -> spectral_losses
    With `log_floor`: of the log-magnitude term mean | ln max(a, f) - ln max(m, f) | alone (its end-to-end figure is a property of the
    forward transform, tests/test_gpu_spectral_loss.py: recorded, not gated)."""
    leaf = X.to(_cdtype(dtype)).clone().requires_grad_(True)
    y = istft(O, leaf, p, dtype)
    if length is not None:
        L = y.shape[-1]
        y = y[:, :length] if length <= L else torch.nn.functional.pad(y, (0, length - L))
    a = stft(O, y, p, dtype).abs()
    m = target_mag.to(dtype)
    if log_floor is None:
        loss = torch.sqrt((a - m).pow(2).sum((1, 2)) / m.pow(2).sum((1, 2)))
    else:
        loss = (torch.log(a.clamp_min(log_floor)) - torch.log(m.clamp_min(log_floor))).abs().mean((1, 2))
    loss.sum().backward()
    return leaf.grad.detach()
