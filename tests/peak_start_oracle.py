"""
The spectral-peak start of Griffin-Lim (include/rfx.h: rfx_peak_start), restated in numpy: TEST ORACLE ONLY.

Row r is one clip-channel, t the frame, m[k] the float32 magnitude of bin k = 0 .. F - 1, N = n_fft.

Decisions, in float32 on the float32 inputs:
  thr = 1e-5f * max_k m[k], one float32 multiply (NaN entries skipped; comparisons with NaN are false);
  k is a peak iff 1 <= k <= F - 2, m[k] > m[k-1], m[k] >= m[k+1] and m[k] > thr;
  with the peaks p_0 < p_1 < ..., bin j belongs to p_i for the smallest i with j <= (p_i + p_{i+1}) // 2, to the last peak if none.
Arithmetic, in float64 from the float32 inputs:
  a, b, c = m[p-1], m[p], m[p+1]; delta = clamp(0.5 (a - c) / (a - 2 b + c), -0.5, 0.5); pos = p + delta;
  phase in turns; a frame without a peak has phase 0 everywhere and cuts the chain; the first frame of a chain (t = 0, or after a
  frame without a peak) has phi[p] = 0; otherwise, q the peak of frame t - 1 that owns bin p,
  phi_t[p] = frac(phi_{t-1}[q] + 0.5 (pos_{t-1}[q] + pos_t[p]) hop / N);
  angles0[r, k, t] = (-1)^k exp(2 pi i phi_t[owner(k)]).
"""
import numpy as np


def frame_peaks(m: np.ndarray) -> np.ndarray:
    """indices of the peaks of one float32 frame, increasing"""
    m = np.asarray(m, np.float32)
    F = m.shape[0]
    with np.errstate(invalid="ignore"):
        finite = m[~np.isnan(m)]
        mx = np.float32(finite.max()) if finite.size else np.float32(-np.inf)
        thr = np.float32(1e-5) * mx
        k = np.arange(1, F - 1)
        ok = (m[k] > m[k - 1]) & (m[k] >= m[k + 1]) & (m[k] > thr)
    return k[ok]


def frame_owners(peaks: np.ndarray, F: int) -> np.ndarray:
    """owner (a peak's bin) of every bin; -1 everywhere without peaks"""
    if len(peaks) == 0:
        return np.full(F, -1, np.int64)
    mids = (peaks[:-1] + peaks[1:]) // 2  # bin j belongs to p_i for the smallest i with j <= mids[i]
    idx = np.searchsorted(mids, np.arange(F), side="left")
    return peaks[idx]


def frame_positions(m: np.ndarray, peaks: np.ndarray) -> np.ndarray:
    m = np.asarray(m, np.float32).astype(np.float64)
    a, b, c = m[peaks - 1], m[peaks], m[peaks + 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = np.clip(0.5 * (a - c) / (a - 2.0 * b + c), -0.5, 0.5)
    return peaks + delta


def peak_start(mag: np.ndarray, hop: int, n_fft: int, details: bool = False):
    """mag (B, F, T) float32 -> angles0 (B, F, T) complex128; with details also the per-row, per-frame peak lists"""
    mag = np.asarray(mag, np.float32)
    B, F, Tn = mag.shape
    out = np.zeros((B, F, Tn), np.complex128)
    sign = np.where(np.arange(F) % 2 == 1, -1.0, 1.0)
    all_peaks = []
    for r in range(B):
        row_peaks = []
        prev = None  # (owners, phi by bin, pos by bin) of the previous frame; None: a chain starts
        for t in range(Tn):
            m = mag[r, :, t]
            peaks = frame_peaks(m)
            row_peaks.append(peaks)
            if len(peaks) == 0:
                out[r, :, t] = sign
                prev = None
                continue
            owners = frame_owners(peaks, F)
            pos = frame_positions(m, peaks)
            if prev is None:
                phi = np.zeros(len(peaks))
            else:
                q = prev[0][peaks]
                x = prev[1][q] + 0.5 * (prev[2][q] + pos) * hop / n_fft
                phi = x - np.floor(x)
            phi_by_bin = np.zeros(F)
            pos_by_bin = np.zeros(F)
            phi_by_bin[peaks] = phi
            pos_by_bin[peaks] = pos
            out[r, :, t] = sign * np.exp(2j * np.pi * phi_by_bin[owners])
            prev = (owners, phi_by_bin, pos_by_bin)
        all_peaks.append(row_peaks)
    return (out, all_peaks) if details else out
