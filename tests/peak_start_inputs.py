"""
Inputs of the spectral-peak start tests (tests/test_peak_start_cpu.py, tests/test_gpu_peak_start.py): crafted frames that hold every
decision case of the start once, and a row of real InverseMelScale output.  TEST INFRASTRUCTURE ONLY.
"""
import os

import numpy as np
import torch

import peak_start_oracle


def tonal_frame(F: int, t: int, rng: np.random.Generator) -> np.ndarray:
    """a few drifting partials on a low noise floor: peaks move by a fraction of a bin per frame, some appear and vanish"""
    k = np.arange(F, dtype=np.float64)
    m = 0.02 * rng.random(F)
    for i, c in enumerate(np.linspace(0.04, 0.9, 9)):
        centre = c * F + 0.37 * t * (1 + i % 3) - 0.2 * i
        amp = 50.0 * (1 + i) * (1.0 if (t + i) % 7 else 0.0)
        m += amp * np.exp(-0.5 * ((k - centre) / (1.5 + 0.2 * i)) ** 2)
    return m.astype(np.float32)


def crafted_row(F: int, T: int, seed: int = 3):
    """(F, T) float32 magnitudes and {case name: frame index}.  Cases: zero, constant, max0_monotone, plateau, edges, two_apart,
    midpoint, threshold, nan; the frames around `zero` are tonal so that a chain is cut and restarted there."""
    assert F >= 200 and T >= 16
    rng = np.random.default_rng(seed)
    m = np.stack([tonal_frame(F, t, rng) for t in range(T)], axis=1)
    at = {}

    def put(name, t, frame):
        m[:, t] = frame
        at[name] = t

    put("zero", 3, np.zeros(F, np.float32))
    put("constant", 5, np.full(F, 3.0, np.float32))
    put("max0_monotone", 6, np.linspace(9.0, 1.0, F).astype(np.float32))
    f = np.zeros(F, np.float32)
    f[10] = f[11] = 5.0
    put("plateau", 8, f)
    f = np.zeros(F, np.float32)
    f[1], f[F - 2] = 4.0, 3.0
    put("edges", 9, f)
    f = np.zeros(F, np.float32)
    f[20], f[21], f[22] = 5.0, 1.0, 4.0
    put("two_apart", 10, f)
    f = np.zeros(F, np.float32)
    f[30] = f[33] = 2.0   # an odd distance: (30 + 33) // 2 = 31
    f[40] = f[44] = 2.0   # an even distance: 42 goes to the lower peak
    put("midpoint", 11, f)
    f = np.zeros(F, np.float32)
    f[50] = 1000.0
    thr = np.float32(1e-5) * np.float32(1000.0)
    f[100] = np.nextafter(thr, np.float32(np.inf), dtype=np.float32)
    f[110] = np.nextafter(thr, np.float32(0), dtype=np.float32)
    f[120] = thr
    put("threshold", 12, f)
    f = m[:, 13].copy()
    f[59], f[60], f[61], f[62] = 7.0, np.nan, 9.0, 1.0
    put("nan", 13, f)
    return m, at


def assert_crafted_cases(peaks, at, F):
    """every case is in the input, read from the restatement's peak lists of the crafted row"""
    for name in ("zero", "constant", "max0_monotone"):
        assert len(peaks[at[name]]) == 0, name
    assert len(peaks[at["zero"] - 1]) > 0 and len(peaks[at["zero"] + 1]) > 0  # a chain is cut and restarted
    assert len(peaks[at["constant"] - 1]) > 0 and len(peaks[at["constant"] + 1]) == 0 and len(peaks[at["max0_monotone"] + 1]) > 0
    assert list(peaks[at["plateau"]]) == [10]
    assert list(peaks[at["edges"]]) == [1, F - 2]
    assert list(peaks[at["two_apart"]]) == [20, 22]
    assert list(peaks[at["midpoint"]]) == [30, 33, 40, 44]
    own = peak_start_oracle.frame_owners(peaks[at["midpoint"]], F)
    assert list(own[29:46]) == [30, 30, 30, 33, 33, 33, 33, 33, 40, 40, 40, 40, 40, 40, 44, 44, 44] and own[0] == 30 and own[F - 1] == 44
    assert list(peaks[at["threshold"]]) == [50, 100]  # just over the threshold; just under and equal to it are not peaks
    p = list(peaks[at["nan"]])
    assert 59 not in p and 60 not in p and 61 not in p  # the neighbours of a NaN are no peaks, whatever their size


def tile_mel(O, golden_dir: str, name: str, lo: int, hi: int) -> torch.Tensor:
    """(1, n_mels, hi - lo) mel amplitudes of columns lo:hi of a golden seed tile, channel R"""
    from PIL import Image

    rgb = np.asarray(Image.open(os.path.join(golden_dir, name + ".png")).convert("RGB"))
    return torch.from_numpy(np.ascontiguousarray(O.spectrogram_from_image_u8(rgb)[:, :, lo:hi]))


def tile_magnitudes(O, p, golden_dir: str, name: str, lo: int, hi: int) -> torch.Tensor:
    """(1, n_stft, hi - lo) linear magnitudes: the oracle's SGD InverseMelScale from manual_seed(7)"""
    return O.inverse_mel_scale_sgd(tile_mel(O, golden_dir, name, lo, hi), p, generator=torch.Generator().manual_seed(7))
