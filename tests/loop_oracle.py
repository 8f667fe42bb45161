"""
The loop variant of the oracle's Griffin-Lim, shared by tests/test_loop_decode_cpu.py and tests/test_gpu_loop_decode.py
(include/rfx.h: rfx_loop_call_options).  A row of T frames is the STFT of a signal with period P = hop T: frames are taken modulo
P and the overlap-add is circular.  With h = n_fft // 2, left = (n_fft - win) // 2 and w the window zero-padded to n_fft:

  analysis   frame t, element i is x[(hop t + i - h) mod P] w[i], then the real FFT: torch.stft(center=False) of
             x[P - h:] || x || x[:n_fft - h] with the last frame dropped;
  synthesis  y[m] = (sum of w[i] frame_t[i] over hop t + i - h = m mod P) / env[m], env[m] the same sum of w[i]^2; P samples.

`loop_griffinlim` is oracle.griffinlim as it stands with these two transforms in the place of torch.stft(center=True, reflect) and
torch.istft: the start, the momentum with tprev = 0 first, the 1e-16 guard and the final synthesis are the oracle's.
"""
from fractions import Fraction

import numpy as np
import torch


def min_frames(p):
    """the smallest T a loop call takes: hop T >= n_fft"""
    return -(-p.n_fft // p.hop_length)


def padded_window(O, p, dtype=torch.float32):
    w = torch.zeros(p.n_fft, dtype=dtype)
    left = (p.n_fft - p.win_length) // 2
    w[left:left + p.win_length] = O.hann_window(p).to(dtype)
    return w


def loop_stft(O, x, p, dtype=torch.float32):
    """(B, P) -> (B, n_stft, T) complex, P = hop T >= n_fft"""
    x = x.to(dtype)
    P, h = x.shape[-1], p.n_fft // 2
    assert P % p.hop_length == 0 and P >= p.n_fft
    ext = torch.cat([x[..., P - h:], x, x[..., :p.n_fft - h]], dim=-1)
    X = torch.stft(ext, n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=O.hann_window(p).to(dtype), center=False,
                   normalized=False, onesided=True, return_complex=True)
    assert X.shape[-1] == P // p.hop_length + 1
    return X[..., :-1]


def _scatter_index(p, T):
    """(n_fft, T) int64: the sample (hop t + i - h) mod P of element i of frame t"""
    i = torch.arange(p.n_fft)[:, None]
    t = torch.arange(T)[None, :]
    return (p.hop_length * t + i - p.n_fft // 2) % (p.hop_length * T)


def loop_env(O, p, T, dtype=torch.float32):
    """(P,) circular window envelope"""
    w = padded_window(O, p, dtype)
    env = torch.zeros(p.hop_length * T, dtype=dtype)
    env.index_add_(0, _scatter_index(p, T).reshape(-1), (w * w)[:, None].expand(p.n_fft, T).reshape(-1))
    return env


def loop_istft(O, X, p, dtype=torch.float32):
    """(B, n_stft, T) complex -> (B, P), P = hop T >= n_fft"""
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    X = X.to(cdtype)
    B, _, T = X.shape
    assert p.hop_length * T >= p.n_fft
    frames = torch.fft.irfft(X, n=p.n_fft, dim=1) * padded_window(O, p, dtype)[None, :, None]
    y = torch.zeros(B, p.hop_length * T, dtype=dtype)
    y.index_add_(1, _scatter_index(p, T).reshape(-1), frames.reshape(B, -1))
    return y / loop_env(O, p, T, dtype)[None]


def loop_griffinlim(O, spec, p, angles0, n_iter, dtype=torch.float32, momentum=0.99):
    """oracle.griffinlim(spec, p, angles0=angles0, n_iter=n_iter, dtype=dtype) on the circular transforms -> (B, hop T)"""
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    spec = spec.to(dtype)
    mom = momentum / (1 + momentum)
    angles = angles0.to(cdtype)
    tprev = torch.tensor(0.0, dtype=dtype)
    for _ in range(n_iter):
        rebuilt = loop_stft(O, loop_istft(O, spec * angles, p, dtype), p, dtype)
        angles = rebuilt
        if momentum:
            angles = angles - tprev * mom
        angles = angles.div(angles.abs().add(1e-16))
        tprev = rebuilt
    return loop_istft(O, spec * angles, p, dtype)


def loop_spectral_convergence(O, x, spec, p):
    """|| |loop_stft(x)| - S || / || S || in float64, over the whole batch"""
    S = spec.double()
    return float((loop_stft(O, x.double(), p, torch.float64).abs() - S).norm() / S.norm())


def seam_figure(x):
    """the step across the loop point, |x[0] - x[-1]|, over the RMS sample-to-sample step of the clip, per row of (B, P) -> (B,) float64"""
    x = torch.as_tensor(x).double()
    steps = x[..., 1:] - x[..., :-1]
    return ((x[..., 0] - x[..., -1]).abs() / steps.pow(2).mean(-1).sqrt()).numpy()


# ---- the envelope table as the device sums it: float32, one fma chain per entry, oldest covering frame first -------------------------

def _round_f32(fr):
    """the float32 nearest to the Fraction fr, ties to even"""
    f = np.float32(float(fr))
    cands = {f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))}
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def env_table_f32(window, n_fft, hop):
    """env[r], r < hop: with q = r + n_fft // 2 - left, the sum of w[j]^2 over j = q - hop t, t = ceil((q - win + 1) / hop) ..
    floor(q / hop), as a float32 fma chain in increasing t (decreasing j), every fma rounded once"""
    w = np.asarray(window, dtype=np.float32)
    win = len(w)
    off = n_fft // 2 - (n_fft - win) // 2
    out = np.zeros(hop, dtype=np.float32)
    for r in range(hop):
        q = r + off
        tlo, thi = -((win - 1 - q) // hop), q // hop
        e = np.float32(0)
        for t in range(tlo, thi + 1):
            wj = Fraction(float(w[q - hop * t]))
            e = _round_f32(wj * wj + Fraction(float(e)))
        out[r] = e
    return out


def fold_f64(frames, window, n_fft, hop):
    """the circular fold of windowed-by-the-fold frames in float64: frames (T, win) un-windowed synthesis frames, window (win,) ->
    (sum of w y, sum of |w y|, env), each (P,) float64"""
    frames = np.asarray(frames, dtype=np.float64)
    w = np.asarray(window, dtype=np.float64)
    T, win = frames.shape
    P, left = hop * T, (n_fft - win) // 2
    idx = (hop * np.arange(T)[:, None] + left + np.arange(win)[None, :] - n_fft // 2) % P
    num, mag, env = np.zeros(P), np.zeros(P), np.zeros(P)
    np.add.at(num, idx, frames * w)
    np.add.at(mag, idx, np.abs(frames * w))
    np.add.at(env, idx, np.broadcast_to(w * w, frames.shape))
    return num, mag, env
