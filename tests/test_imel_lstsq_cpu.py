"""
CPU checks of the closed-form InverseMelScale (csrc/rfx_imel_lstsq.hip, include/rfx.h: rfx_inverse_mel_lstsq).

* The host analysis (rfx_debug_lstsq_bank, no GPU): ok for six banks of the reference's family, its float32 tables against a
  float64 L D L^T of fb^T fb built here with numpy; refusals of num_frequencies = 1024 (a pivot), of a bin with three filters
  and of an all-zero filter.
* The arithmetic header csrc/rfx_imel_lstsq_core.h, compiled for the host with tests/emu/rfx_imel_lstsq_emu.cpp, against
  torch.relu(torch.linalg.lstsq(fb.T[None].double(), mel[None].double(), driver="gels").solution).
  Gate: the library the closed form replaces is torch's lstsq in float32, so its own distance from the float64 result is what
  float32 can be asked for: the emulator's relative L2 distance must be at most 2 times torch's float32 "gels" distance, measured
  in the same test on the same input, overall and for the worst single frame.  (2: room for another fixed operation order.)
"""
import ctypes

import numpy as np
import pytest
import torch

from imel_lstsq_cases import bank, distances, emu_run, emulator, image_mel, lstsq_reference, report

BANKS = {
    "default": {},
    "norm_slaney": dict(mel_scale_norm="slaney"),
    "type_slaney": dict(mel_scale_type="slaney"),
    "20hz_20khz": dict(min_frequency=20, max_frequency=20000),
    "48khz": dict(sample_rate=48000),
    "8khz_64": dict(sample_rate=8000, num_frequencies=64, max_frequency=4000),
}


@pytest.fixture(scope="module")
def emu():
    return emulator()


def ldl_float64(fb: torch.Tensor):
    """D and the sub-diagonal of L of fb^T fb = L D L^T, in float64; also how far fb^T fb is from tridiagonal"""
    G = (fb.double().T @ fb.double()).numpy()
    M = G.shape[0]
    off = np.abs(np.triu(G, 2)).max() if M > 2 else 0.0
    d, e = np.diag(G), np.diag(G, 1)
    D, l = np.zeros(M), np.zeros(M)
    D[0] = d[0]
    for m in range(M - 1):
        l[m] = e[m] / D[m]
        D[m + 1] = d[m + 1] - l[m] * e[m]
    return D, l, d, off


def consistent_mel(fb, T, seed=1):
    g = torch.Generator().manual_seed(seed)
    lin = torch.rand(fb.shape[0], T, generator=g) ** 4 * 3e7
    return (fb.T @ lin)[None].contiguous()


# ---- the host analysis -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BANKS))
def test_bank_is_served_and_the_tables_are_the_float64_factors(name):
    op, cp, fb = bank(**BANKS[name])
    rep, tables = report(cp, fb, tables=True)
    assert rep.ok == 1 and rep.why == b"", rep.why
    D, l, d, off = ldl_float64(fb)
    assert off == 0.0, "fb^T fb is not tridiagonal"
    neg_l, inv_d = tables
    # float32 rounding of the float64 factors: half an ulp, 2^-24 relative; the two float64 factorisations differ by their
    # summation order (1e-16 times cond(G) <= 100), which can move a value across a rounding boundary: one ulp
    assert np.all(np.abs(neg_l.astype(np.float64) + l) <= 2.0 ** -23 * np.abs(l))
    assert np.all(np.abs(inv_d.astype(np.float64) - 1.0 / D) <= 2.0 ** -23 / D)
    assert neg_l[-1] == 0.0
    ratio = (D / d).min()
    print(f"{name}: smallest pivot / diagonal {ratio:.4f} (library {rep.min_pivot_ratio:.4f} at {rep.min_pivot})")
    assert abs(rep.min_pivot_ratio - ratio) <= 1e-9 and rep.min_pivot == int(np.argmin(D / d))


def test_1024_filters_are_refused_with_the_pivot():
    op, cp, fb = bank(num_frequencies=1024)
    rep = report(cp, fb)
    assert rep.ok == 0 and b"pivot" in rep.why and rep.min_pivot >= 0 and rep.min_pivot_ratio <= 2.0 ** -20, rep.why
    assert f"pivot {rep.min_pivot} ".encode() in rep.why


def test_handmade_banks_are_refused():
    op, cp, fb = bank(**BANKS["8khz_64"])
    three = fb.clone()
    f = int(torch.nonzero(three[:, 10])[0])
    three[f, 9:12] = torch.tensor([0.25, 0.5, 0.25])
    rep = report(cp, three)
    assert rep.ok == 0 and b"more than two adjacent" in rep.why and rep.min_pivot == -1, rep.why
    apart = fb.clone()
    apart[f, :] = 0.0
    apart[f, 9], apart[f, 12] = 0.5, 0.5
    rep = report(cp, apart)
    assert rep.ok == 0 and b"more than two adjacent" in rep.why, rep.why
    empty = fb.clone()
    empty[:, 20] = 0.0
    rep = report(cp, empty)
    assert rep.ok == 0 and b"pivot 20 " in rep.why and rep.min_pivot == 20 and rep.min_pivot_ratio == 0.0, rep.why


def test_report_struct_size_is_checked():
    from riffusion import _hip

    op, cp, fb = bank(**BANKS["8khz_64"])
    lib = _hip.load_library()
    bad = _hip.RfxLstsqBankReport(struct_size=4)
    assert lib.rfx_debug_lstsq_bank(ctypes.byref(cp), fb.data_ptr(), ctypes.byref(bad)) == -1 and b"struct_size" in lib.rfx_last_error()
    short = _hip.RfxLstsqBankReport(struct_size=8)  # a caller that only wants the flag
    assert lib.rfx_debug_lstsq_bank(ctypes.byref(cp), fb.data_ptr(), ctypes.byref(short)) == 0 and short.ok == 1


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def gate(emu, fb, tables, mel, label):
    ref = lstsq_reference(fb, mel, torch.float64)
    torch32 = distances(lstsq_reference(fb, mel, torch.float32), ref)
    got = emu_run(emu, fb, tables, mel)
    ours = distances(got, ref)
    print(f"{label}: emulator rel-L2 {ours[0]:.2e} (worst frame {ours[1]:.2e}); torch float32 gels {torch32[0]:.2e} (worst frame {torch32[1]:.2e})")
    assert torch.isfinite(got).all() and (got >= 0).all()
    assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1]
    return got


@pytest.mark.parametrize("name,T", [("default", 24), ("8khz_64", 37)])
def test_emulator_against_lstsq_on_consistent_input(emu, name, T):
    op, cp, fb = bank(**BANKS[name])
    _, tables = report(cp, fb, tables=True)
    gate(emu, fb, tables, consistent_mel(fb, T), f"{name}, mel = fb^T lin")


@pytest.mark.parametrize("name,T", [("default", 24), ("8khz_64", 37)])
def test_emulator_against_lstsq_on_a_random_tile(emu, name, T):
    """Measured (sequential float32 sweeps): default bank 5.8e-8 overall / 6.8e-8 worst frame against torch's float32 gels at
    1.4e-7 / 1.6e-7; 8 kHz, 64 filters 5.8e-8 / 7.4e-8 against 1.7e-7 / 2.7e-7.  The float32 recurrence is the closer one on
    this input too: it stays float32."""
    op, cp, fb = bank(**BANKS[name])
    _, tables = report(cp, fb, tables=True)
    mel = image_mel(fb.shape[1], T)
    assert tuple(mel.shape) == (1, fb.shape[1], T)
    gate(emu, fb, tables, mel, f"{name}, random uint8 tile at max_value 30e6")


@pytest.mark.parametrize("name", ["default", "8khz_64"])
def test_bins_outside_the_bank_are_exactly_zero_and_scale_is_exact(emu, name):
    from helpers import plan_bank_report

    op, cp, fb = bank(**BANKS[name])
    _, tables = report(cp, fb, tables=True)
    rep = plan_bank_report(op)
    mel = image_mel(fb.shape[1], 5)
    got = emu_run(emu, fb, tables, mel)
    outside = np.r_[0:rep.f_lo, rep.f_hi:fb.shape[0]]
    assert len(outside) > 0 and (fb[outside] == 0).all() and (fb[rep.f_lo:rep.f_hi].sum(1) > 0).all()
    assert (got[:, outside] == 0).all() and got[:, outside].numpy().tobytes() == bytes(4 * got[:, outside].numel())
    assert (got[:, rep.f_lo:rep.f_hi] > 0).any()
    for k in (-40, 7, 60):  # every step is linear and rounds alike at every power of two
        assert torch.equal(emu_run(emu, fb, tables, mel * 2.0 ** k), got * 2.0 ** k)
    # a frame's result is its own column's: alone, and next to others
    assert torch.equal(emu_run(emu, fb, tables, mel[:, :, 2:3].contiguous()), got[:, :, 2:3])
