"""
Oracles of the windowed-sinc resampler (include/rfx.h "SINC RESAMPLE"), torch on the CPU.  torchaudio is not installed where the
tests run, so its two functions are transcribed:

* `dense_kernel` / `dense_resample`: torchaudio.functional.functional._get_sinc_resample_kernel (resampling_method =
  "sinc_interp_hann") and _apply_sinc_resample_kernel, statement by statement, parameterised by dtype.
    dtype = float64                       the reference of every figure
    dtype = float32 throughout            what functional.resample computes on a float32 waveform (`resample_f32`)
    float64 kernel rounded to float32     what transforms.Resample holds and applies (`resample_f32_kernel64`)
* `sparse_table` / `sparse_resample`: the same formulas in float64 evaluated only on the taps with |t| < lowpass_filter_width - the
  dense kernel of 33037 -> 44100 would take 11.7 GB.  A table is (first (n,), count (n,), weights (ntaps, n)): per phase the offset of
  its first kept tap from q o, the number of kept taps, and the weights tap-major, zero past the phase's run.
* `sparse_weights` / `sparse_resample_f32`: the two float32 computations where no dense kernel fits: the kernel's statements in
  `dtype` on the kept taps alone (float32: functional.resample's kernel; float64 rounded: transforms.Resample's), then a float32 sum
  over the taps in ascending order, product and sum rounded separately.  conv1d's own summation order is not stated by torch; on the
  pairs that have a dense kernel the two forms land within a few tenths of a dB of each other (tests/test_resample_cpu.py prints both).

Definitions: o = orig / g, n = new / g, g = gcd; base = min(o, n) rolloff; width = ceil(lpw o / base); L samples give
K = ceil(n L / o).
"""
import math

import numpy as np
import torch


def geometry(orig, new, lpw=6, rolloff=0.99):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * rolloff
    return o, n, base, math.ceil(lpw * o / base)


def frames(L, orig, new):
    o, n, _, _ = geometry(orig, new)
    return -((-n * L) // o)


def dense_kernel(orig, new, dtype, lpw=6, rolloff=0.99, device=None):
    """_get_sinc_resample_kernel(orig, new, gcd, lpw, rolloff, "sinc_interp_hann", device, dtype) before its final cast: (n, 1, 2 width + o)"""
    o, n, base_freq, width = geometry(orig, new, lpw, rolloff)
    idx = torch.arange(-width, width + o, dtype=dtype, device=device)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=dtype, device=device)[:, None, None] / n + idx
    t *= base_freq
    t = t.clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t *= math.pi
    scale = base_freq / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels, width


def apply_dense(waveform, orig, new, kernel, width):
    """_apply_sinc_resample_kernel on (B, L) rows, in the kernel's dtype"""
    o, n, _, _ = geometry(orig, new)
    num_wavs, length = waveform.shape
    w = torch.nn.functional.pad(waveform.to(kernel.dtype), (width, width + o))
    resampled = torch.nn.functional.conv1d(w[:, None], kernel, stride=o)
    resampled = resampled.transpose(1, 2).reshape(num_wavs, -1)
    return resampled[..., : math.ceil(n * length / o)]


def dense_resample(waveform, orig, new, dtype, lpw=6, rolloff=0.99):
    if int(orig) == int(new):
        return waveform.to(dtype)
    k, width = dense_kernel(orig, new, dtype, lpw, rolloff)
    return apply_dense(waveform, orig, new, k, width)


def resample_f32(waveform, orig, new):
    """functional.resample on a float32 waveform: kernel and sum in float32"""
    return dense_resample(waveform.float(), orig, new, torch.float32)


def resample_f32_kernel64(waveform, orig, new):
    """transforms.Resample: the kernel made in float64 and rounded once, the sum in float32"""
    k, width = dense_kernel(orig, new, torch.float64)
    return apply_dense(waveform.float(), orig, new, k.float(), width)


# ---- the sparse form ---------------------------------------------------------------------------------------------------------------------

def _t(o, n, base, width, p, i):
    """t of tap i of phase p before the clamp: the dense kernel's float64 operations in its order"""
    return (np.asarray(-p, np.float64) / np.float64(n) + np.asarray(i - width, np.float64) / np.float64(o)) * np.float64(base)


def sparse_table(orig, new, lpw=6, rolloff=0.99):
    """(first (n,) int64, count (n,) int64, weights (ntaps, n) float64): the dense float64 kernel's taps with |t| < lpw"""
    o, n, base, width = geometry(orig, new, lpw, rolloff)
    half = o * lpw / base
    span = int(math.ceil(2 * half)) + 6
    p = np.arange(n, dtype=np.int64)
    lo = np.floor(width + o * p / n - half).astype(np.int64) - 2
    i = lo[None, :] + np.arange(span, dtype=np.int64)[:, None]  # (span, n) candidates, a superset of every phase's run
    t = _t(o, n, base, width, p[None, :], i)
    kept = (np.abs(t) < lpw) & (i >= 0) & (i < 2 * width + o)
    count = kept.sum(0)
    start = kept.argmax(0)
    assert (count > 0).all() and all(kept[s:s + c, q].all() for q, (s, c) in enumerate(zip(start, count)) if q < 64)  # one run per phase
    ntaps = int(count.max())
    rows = start[None, :] + np.arange(ntaps)[:, None]
    tt = np.take_along_axis(t, np.minimum(rows, span - 1), 0)
    window = np.cos(tt * math.pi / lpw / 2) ** 2
    tp = tt * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(tp == 0, 1.0, np.sin(tp) / tp) * (window * (base / o))
    w = np.where(np.arange(ntaps)[:, None] < count[None, :], w, 0.0)
    first = np.take_along_axis(i, start[None, :], 0)[0] - width
    return first, count, w


def sparse_resample(waveform, orig, new, lpw=6, rolloff=0.99, table=None):
    """(B, L) -> (B, K) float64: the sum over the kept taps only"""
    if int(orig) == int(new):
        return waveform.double()
    o, n, _, _ = geometry(orig, new, lpw, rolloff)
    first, _, w = table if table is not None else sparse_table(orig, new, lpw, rolloff)
    x = waveform.double().numpy()
    B, L = x.shape
    K = -((-n * L) // o)
    j = np.arange(K, dtype=np.int64)
    q, p = j // n, j % n
    at = q * o + first[p]
    out = np.zeros((B, K))
    for k in range(w.shape[0]):
        idx = at + k
        ok = (idx >= 0) & (idx < L)
        out += np.where(ok[None, :], x[:, np.clip(idx, 0, L - 1)], 0.0) * w[k, p][None, :]
    return torch.from_numpy(out)


def sparse_weights(orig, new, dtype, lpw=6, rolloff=0.99, table=None):
    """(ntaps, n) float32: dense_kernel's statements in `dtype`, evaluated on the taps `table` keeps, rounded to float32 at the end"""
    o, n, base_freq, width = geometry(orig, new, lpw, rolloff)
    first, count, w64 = table if table is not None else sparse_table(orig, new, lpw, rolloff)
    ntaps = w64.shape[0]
    i = torch.from_numpy(first + width)[None, :] + torch.arange(ntaps)[:, None]  # (ntaps, n) tap indices of the dense kernel
    idx = (i - width).to(dtype) / o
    t = (-torch.arange(n)).to(dtype)[None, :] / n + idx
    t *= base_freq
    t = t.clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t *= math.pi
    scale = base_freq / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    kernels[torch.arange(ntaps)[:, None] >= torch.from_numpy(count)[None, :]] = 0
    return kernels.float()


def sparse_resample_f32(waveform, orig, new, weights, table):
    """(B, L) float32 -> (B, K) float32: the sum over the kept taps in float32, ascending, product and sum rounded separately"""
    o, n, _, _ = geometry(orig, new)
    first = table[0]
    x = waveform.float().numpy()
    w = weights.numpy()
    B, L = x.shape
    K = -((-n * L) // o)
    j = np.arange(K, dtype=np.int64)
    q, p = j // n, j % n
    at = q * o + first[p]
    out = np.zeros((B, K), np.float32)
    for k in range(w.shape[0]):
        idx = at + k
        ok = (idx >= 0) & (idx < L)
        out = out + np.where(ok[None, :], x[:, np.clip(idx, 0, L - 1)], np.float32(0)) * w[k, p][None, :]
    return torch.from_numpy(out)
