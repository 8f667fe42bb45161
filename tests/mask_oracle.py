"""
The masked variant of the oracle's Griffin-Lim loop, shared by tests/test_hold_mask_cpu.py and tests/test_gpu_hold_mask.py
(include/rfx.h: rfx_masked_call_options).  tests/held_oracle.py's loop with a per-bin mask in place of per-frame spans: after the
projection `angles = angles.div(angles.abs().add(1e-16))`, `angles = torch.where(held, a0, angles)` with `held` a (B, n_stft, T)
boolean.  Two forms of the same loop:

  where form   the definition, as above;
  split form   what the device runs (csrc/rfx_holdmask_core.h): S_held = S where held, S_free = S - S_held, c = ISTFT(S_held a0);
               the unheld loop on S_free, with c added to every estimate: x_k = ISTFT(S_free proj(STFT(x_{k-1}) - m STFT(x_{k-2}))) + c,
               x_0 = ISTFT(S a0).
"""
import numpy as np
import torch


def pack_bits(held):
    """(B, n_stft, T) bool -> (B, T, ceil(n_stft / 32)) int32: bin b of a frame is bit b & 31 of word b >> 5; unused tail bits 0"""
    held = np.asarray(held, dtype=bool)
    B, F, T = held.shape
    words = (F + 31) // 32
    bits = np.zeros((B, T, words * 32), dtype=np.uint8)
    bits[:, :, :F] = held.transpose(0, 2, 1)
    packed = np.packbits(bits.reshape(B, T, words, 32), axis=-1, bitorder="little")  # (B, T, words, 4) bytes, little-endian words
    return np.ascontiguousarray(packed).view("<u4").reshape(B, T, words).astype(np.uint32).view(np.int32)


def unpack_bits(words, n_stft):
    """(B, T, words) int32 -> (B, n_stft, T) bool; bits at or above n_stft are dropped"""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[0], w.shape[1], -1)[:, :, :n_stft].astype(bool).transpose(0, 2, 1)


def bin_bands(fb):
    """(n_stft, n_mels) filterbank -> (lo, hi) int16 arrays: first and last band with a nonzero weight at each bin, -1 / -1 for none"""
    nz = np.asarray(fb) != 0
    any_ = nz.any(axis=1)
    lo = np.where(any_, nz.argmax(axis=1), -1).astype(np.int16)
    hi = np.where(any_, nz.shape[1] - 1 - nz[:, ::-1].argmax(axis=1), -1).astype(np.int16)
    return lo, hi


def bins_from_bands(bands, lo, hi):
    """(B, n_mels, T) bool per-band mask -> (B, n_stft, T) bool: bin f is held at t iff it has a band range and every band of
    [lo_f, hi_f] is held at t"""
    bands = np.asarray(bands) != 0
    B, M, T = bands.shape
    free = np.concatenate([np.zeros((B, 1, T), np.int64), np.cumsum(~bands, axis=1)], axis=1)  # free bands below m
    ok = lo >= 0
    l, h = np.where(ok, lo, 0).astype(np.int64), np.where(ok, hi, 0).astype(np.int64)
    return (free[:, h + 1, :] - free[:, l, :] == 0) & ok[None, :, None]


def masked_griffinlim(O, S, p, angles0, held, n_iter, dtype=torch.float32, split=False, momentum=0.99):
    """oracle.griffinlim(S, p, angles0=angles0, n_iter=n_iter) with the bins of `held` ((B, n_stft, T) bool) held at angles0, in the
    `where` form or the split form"""
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    spec = S.to(dtype)
    mom = momentum / (1 + momentum)
    a0 = angles0.to(cdtype)
    held = torch.as_tensor(np.asarray(held), dtype=torch.bool)
    window = O.hann_window(p).to(dtype)

    def _istft(x):
        return torch.istft(x, n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=window, center=True, normalized=False,
                           onesided=True, length=None)

    def _stft(x):
        return torch.stft(x, n_fft=p.n_fft, hop_length=p.hop_length, win_length=p.win_length, window=window, center=True, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True)

    tprev = torch.tensor(0.0, dtype=dtype)
    if not split:
        angles = a0
        for _ in range(n_iter):
            rebuilt = _stft(_istft(spec * angles))
            angles = rebuilt
            if momentum:
                angles = angles - tprev * mom
            angles = angles.div(angles.abs().add(1e-16))
            angles = torch.where(held, a0, angles)
            tprev = rebuilt
        return _istft(spec * angles)
    x = _istft(spec * a0)
    if n_iter == 0:
        return x
    zero = torch.zeros((), dtype=dtype)
    s_free = torch.where(held, zero, spec)
    c = _istft(torch.where(held, spec, zero) * a0)
    for _ in range(n_iter):
        rebuilt = _stft(x)
        angles = rebuilt
        if momentum:
            angles = angles - tprev * mom
        angles = angles.div(angles.abs().add(1e-16))
        tprev = rebuilt
        x = _istft(s_free * angles) + c
    return x


def kept_bin_fidelity_db(G, X, held):
    """10 log10(sum |G|^2 / sum |G - X|^2) over the held bins, in double"""
    held = torch.as_tensor(np.asarray(held), dtype=torch.bool)
    G, X = G.to(torch.complex128)[held], X.to(torch.complex128)[held]
    return 10.0 * float(torch.log10(G.abs().pow(2).sum() / (G - X).abs().pow(2).sum()))
