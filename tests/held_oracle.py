"""
The held variant of the oracle's Griffin-Lim loop, shared by tests/test_held_frames_cpu.py and tests/test_gpu_held_frames.py
(include/rfx.h: rfx_held_call_options).  oracle.griffinlim as it stands, with one line more: after the projection
`angles = angles.div(angles.abs().add(1e-16))` the angles of the held frames are set back to the start's, a0.  Everything else -
the momentum term, tprev = rebuilt for all frames, the final ISTFT - is the oracle's.
"""
import numpy as np
import torch


def held_mask(holds, T):
    """(B, T) bool: frame t of row r is held iff t < h or t >= T - l, h = clamp(head, 0, T), l = clamp(tail, 0, T - h)"""
    holds = np.asarray(holds, dtype=np.int64).reshape(-1, 2)
    mask = np.zeros((holds.shape[0], T), dtype=bool)
    for r, (head, tail) in enumerate(holds):
        h = min(max(int(head), 0), T)
        l = min(max(int(tail), 0), T - h)
        mask[r, :h] = True
        mask[r, T - l:] = True
    return torch.from_numpy(mask)


def held_griffinlim(O, specgram, p, angles0, holds, n_iter, momentum=0.99, dtype=torch.float32):
    """oracle.griffinlim(specgram, p, angles0=angles0, n_iter=n_iter) with the frames of `holds` ((B, 2) {head, tail}) held at angles0"""
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    spec = specgram.to(dtype)
    mom = momentum / (1 + momentum)
    a0 = angles0.to(cdtype)
    angles = a0
    window = O.hann_window(p).to(dtype)
    held = held_mask(holds, spec.shape[-1])[:, None, :].expand(spec.shape)

    def _istft(x):
        return torch.istft(x, n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=window, center=True, normalized=False,
                           onesided=True, length=None)

    def _stft(x):
        return torch.stft(x, n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=window, center=True, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True)

    tprev = torch.tensor(0.0, dtype=dtype)
    for _ in range(n_iter):
        rebuilt = _stft(_istft(spec * angles))
        angles = rebuilt
        if momentum:
            angles = angles - tprev * mom
        angles = angles.div(angles.abs().add(1e-16))
        angles = torch.where(held, a0, angles)
        tprev = rebuilt
    return _istft(spec * angles)


def held_only_samples(holds, T, p):
    """(B, L) bool: the samples of each row that only held frames reach.  Frame t's window covers the samples
    [hop t - win // 2, hop t - win // 2 + win) of the clip (those inside [0, L)); a sample no frame reaches is not counted."""
    mask = held_mask(holds, T).numpy()
    L = p.hop_length * (T - 1) + (p.n_fft & 1)
    free_hits = np.zeros((mask.shape[0], L), dtype=np.int64)
    any_hits = np.zeros((mask.shape[0], L), dtype=np.int64)
    left = (p.n_fft - p.win_length) // 2 - p.n_fft // 2  # first sample of frame 0's window
    for t in range(T):
        lo, hi = max(0, p.hop_length * t + left), min(L, p.hop_length * t + left + p.win_length)
        if lo < hi:
            any_hits[:, lo:hi] += 1
            free_hits[~mask[:, t], lo:hi] += 1
    return torch.from_numpy((free_hits == 0) & (any_hits > 0))


def db(ref, x):
    """10 log10(sum ref^2 / sum (ref - x)^2) in double; inf when equal"""
    ref, x = ref.double(), x.double()
    err = float((ref - x).pow(2).sum())
    return float("inf") if err == 0.0 else 10.0 * float(np.log10(float(ref.pow(2).sum()) / err))
