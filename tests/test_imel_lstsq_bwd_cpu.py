"""
CPU checks of the backward of the closed-form InverseMelScale (include/rfx.h: rfx_inverse_mel_lstsq_backward; kernel
lsq_collect_kernel of csrc/rfx_imel_lstsq.hip between two solves).

* tests/emu/rfx_imel_lstsq_bwd_emu.cpp runs the arithmetic header's sweeps, mask and per-filter sum on the tables the library
  reports, against float64 torch autograd of relu(lstsq(fb.T, mel).solution) on the three banks of tests/test_gpu_imel_lstsq.py.
  Gate, overall and worst frame: at most twice the distance of float32 torch autograd on the same input - the forward's rule.
  The float32 and float64 masks may disagree where the value before the relu is nearly 0; that is taken out of the comparison, not
  out of the code: from the float64 reference alone, positions with |v| < 1e-3 (fb |y|) get a zero incoming gradient, and they may
  be at most 0.5 % of the positions that have a filter.
* The adjoint identity <gx * mask, J d> = <g_mel, d> with J = fb G^-1 in float64.
* The mask is the forward emulator's x > 0: a gradient that lives only where x == 0 gives all-zero bits.
* The host lists (rfx_debug_lstsq_collect): once per (filter, bin), ascending, the bank's weights, one position per bin.
* The emulator with a main of its own, built with -fsanitize=address,undefined and run as a program.  Nothing sanitized is loaded
  into Python.
* The autograd routing on a fake plan; include/rfx.h as C99 with the new entries.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
from imel_lstsq_bwd_cases import (EMU_SRC, GUARD_SHARE, distances, emu_backward, emulators, frame_stride, guarded_gradient, lists, to_slots,
                                  torch_gradient)
from imel_lstsq_cases import bank, emu_run, image_mel, report

EMU_MAIN = "rfx_imel_lstsq_bwd_emu_main.cpp"
CASES = {  # the banks and frame counts the gate is stated for
    "default": ({}, 9),
    "norm_slaney": (dict(mel_scale_norm="slaney"), 9),
    "8khz_64": (dict(sample_rate=8000, num_frequencies=64, max_frequency=4000), 21),
}


@pytest.fixture(scope="module")
def emus():
    return emulators()


def tiles(M, T):
    """two image tiles (seeds 3 and 4): not in the range of fb^T, so a good share of the relu is closed"""
    return torch.cat([image_mel(M, T, seed=3), image_mel(M, T, seed=4)]).contiguous()


@pytest.fixture(scope="module")
def case_data():
    """per case, computed once: bank, tables, lists, stride, input, guarded gradient, float64 and float32 torch gradients"""
    cache = {}

    def get(name):
        if name not in cache:
            kw, T = CASES[name]
            op, cp, fb = bank(**kw)
            _, tables = report(cp, fb, tables=True)
            lst = lists(cp, fb)
            mel = tiles(fb.shape[1], T)
            gx, share, open64 = guarded_gradient(fb, mel)
            ref, _ = torch_gradient(fb, mel, gx, torch.float64)
            g32, _ = torch_gradient(fb, mel, gx, torch.float32)
            cache[name] = dict(op=op, cp=cp, fb=fb, tables=tables, lists=lst, stride=frame_stride(op), mel=mel, gx=gx, share=share, open64=open64,
                               ref=ref, g32=g32)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_emulator_against_float64_autograd(emus, case_data, name):
    """Measured: marked share 0.054 % / 0.049 % / 0.045 %; torch float32's own distance 1.0e-6 / 1.1e-6 / 0.7e-6 overall."""
    fwd, bwd = emus
    d = case_data(name)
    assert d["share"] <= GUARD_SHARE, d["share"]
    closed = 1.0 - float(d["open64"].sum()) / float((d["fb"] != 0).any(dim=1).sum() * d["mel"].shape[0] * d["mel"].shape[2])
    got = emu_backward(bwd, d["fb"], d["tables"], d["lists"], d["mel"], to_slots(d["gx"], d["lists"], d["stride"]))
    ours, torch32 = distances(got, d["ref"]), distances(d["g32"], d["ref"])
    # outside the marked positions the float32 mask is float64's
    x = emu_run(fwd, d["fb"], d["tables"], d["mel"])
    differ = ((x > 0) != d["open64"]) & (d["gx"] != 0)
    print(f"{name}: marked share {d['share']:.3%}, closed {closed:.1%}, masks differ at {int(differ.sum())} unmarked positions; emulator rel-L2 "
          f"{ours[0]:.2e} (worst frame {ours[1]:.2e}); torch float32 autograd {torch32[0]:.2e} (worst frame {torch32[1]:.2e})")
    assert torch.isfinite(got).all() and 0.1 < closed < 0.6
    assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1]


@pytest.mark.parametrize("name", ["default", "8khz_64"])
def test_adjoint_identity(emus, case_data, name):
    """<gx * mask, J d> = <g_mel, d> for J = fb G^-1 in float64 and the emulator's own mask.  g_mel is float32: its rounding, 2^-24 per
    step amplified by cond(G) <= 100 (tests/test_imel_lstsq_cpu.py), stays below 1e-5 of |gx * mask| |J d|."""
    fwd, bwd = emus
    d = case_data(name)
    fb, mel, gx = d["fb"], d["mel"], d["gx"]
    mask = emu_run(fwd, fb, d["tables"], mel) > 0
    g_mel = emu_backward(bwd, fb, d["tables"], d["lists"], mel, to_slots(gx, d["lists"], d["stride"]))
    delta = torch.randn(mel.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    Jd = fb.double() @ torch.linalg.solve(fb.double().T @ fb.double(), delta)
    lhs, rhs = float(((gx * mask).double() * Jd).sum()), float((g_mel.double() * delta).sum())
    scale = float((gx * mask).double().norm() * Jd.norm())
    print(f"{name}: <gx mask, J d> {lhs:.9e}, <g_mel, d> {rhs:.9e}, difference {abs(lhs - rhs) / scale:.2e} of the norms' product")
    assert abs(lhs - rhs) <= 1e-5 * scale


@pytest.mark.parametrize("name", ["default", "8khz_64"])
def test_the_mask_is_the_forwards(emus, case_data, name):
    fwd, bwd = emus
    d = case_data(name)
    fb, mel = d["fb"], d["mel"]
    x = emu_run(fwd, fb, d["tables"], mel)
    gx = torch.where(x == 0, torch.full_like(x, 3.0) + torch.arange(x.shape[1], dtype=torch.float32)[None, :, None], torch.zeros_like(x))
    assert (gx != 0).any() and ((x == 0) & ((fb != 0).any(dim=1)[None, :, None])).any()
    got = emu_backward(bwd, fb, d["tables"], d["lists"], mel, to_slots(gx, d["lists"], d["stride"]))
    assert got.numpy().tobytes() == bytes(4 * got.numel())
    # ... and the scale is exact, and a frame's result is its own
    g1 = emu_backward(bwd, fb, d["tables"], d["lists"], mel, to_slots(d["gx"], d["lists"], d["stride"]))
    for k in (-40, 40):
        assert torch.equal(emu_backward(bwd, fb, d["tables"], d["lists"], mel, to_slots(d["gx"] * 2.0 ** k, d["lists"], d["stride"])), g1 * 2.0 ** k)
    one = emu_backward(bwd, fb, d["tables"], d["lists"], mel[1:, :, 2:3].contiguous(), to_slots(d["gx"][1:, :, 2:3], d["lists"], d["stride"]))
    assert torch.equal(one, g1[1:, :, 2:3])


@pytest.mark.parametrize("name", list(CASES))
def test_host_lists(case_data, name):
    d = case_data(name)
    fb, (ptr, bins, pos, w), stride = d["fb"].numpy(), d["lists"], d["stride"]
    F, M = fb.shape
    assert ptr[0] == 0 and ptr[-1] == len(bins) == len(pos) == len(w) == int((fb != 0).sum())
    where = {}
    for m in range(M):
        run = bins[ptr[m]:ptr[m + 1]]
        assert np.array_equal(run, np.nonzero(fb[:, m])[0])  # once per (filter, bin), ascending
        assert np.array_equal(w[ptr[m]:ptr[m + 1]], fb[run, m])
        for f, p in zip(run, pos[ptr[m]:ptr[m + 1]]):
            assert where.setdefault(int(f), int(p)) == int(p)  # one position per bin, whichever filter asks
    ps = np.array(sorted(where.values()))
    assert len(np.unique(ps)) == len(ps) and ps.min() >= 0 and ps.max() < stride
    # first filter and weights as the forward reads them: a filter's run holds the w1 bins of m - 1, then the w0 bins of m
    first = np.array([np.nonzero(fb[f])[0][0] if fb[f].any() else -1 for f in range(F)])
    for m in range(M):
        kinds = first[bins[ptr[m]:ptr[m + 1]]]
        assert set(kinds) <= {m - 1, m} and np.all(np.diff(kinds) >= 0)
    if name == "8khz_64":  # a plain bin-ordered layout
        assert all(f == p for f, p in where.items())


def test_lists_of_a_refused_bank_are_refused():
    from riffusion import _hip

    op, cp, fb = bank(num_frequencies=1024)
    with pytest.raises(Exception, match="pivot"):
        _hip.lstsq_collect_lists(cp, fb)
    lib, n = _hip.load_library(), ctypes.c_int32(0)
    op, cp, fb = bank(**CASES["8khz_64"][0])
    few = np.zeros(3, np.int32)
    assert lib.rfx_debug_lstsq_collect(ctypes.byref(cp), fb.data_ptr(), None, few.ctypes.data, None, None, 3, ctypes.byref(n)) == -1
    assert b"capacity" in lib.rfx_last_error() and n.value > 3


def test_sanitized_stand_alone_emulator():
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program; the sanitizers'
    runtimes are linked statically, so the program carries them itself"""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-ffp-contract=off", "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr


# ---- the autograd routing, on a plan that needs no device --------------------------------------------------------------------------
class FakePlan:
    """x = relu(A mel) with a fixed A (n_stft, n_mels), slots = plain frames: the calls the member and the Function make, counted"""

    n_stft, n_mels, frame_stride, lstsq_ok = 7, 3, 7, True

    def __init__(self):
        self.A = torch.randn(7, 3, generator=torch.Generator().manual_seed(2))
        self.calls = []

    def require_lstsq(self):
        self.calls.append("require")

    def inverse_mel_lstsq(self, mel):
        self.calls.append("forward")
        B, M, T = mel.shape
        return torch.relu(self.A @ mel).permute(0, 2, 1).reshape(B * T, 7).contiguous()

    def unpack_magnitudes(self, slots, B, T):
        return slots.reshape(B, T, 7).permute(0, 2, 1).contiguous()

    def pack_magnitudes(self, x):
        B, F, T = x.shape
        return x.permute(0, 2, 1).reshape(B * T, F).contiguous()

    def inverse_mel_lstsq_backward(self, mel, grad_slots):
        self.calls.append("backward")
        B, M, T = mel.shape
        g = grad_slots.reshape(B, T, 7).permute(0, 2, 1)
        return self.A.T @ (g * (self.A @ mel > 0))

    def inverse_mel(self, mel, B, spec0=None, seed=0):
        self.calls.append(("sgd", seed))
        return self.pack_magnitudes(torch.ones(mel.shape[0], 7, mel.shape[2]))


@pytest.fixture()
def converter(monkeypatch):
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(), device="cpu")
    plan = FakePlan()
    monkeypatch.setattr(conv, "_plan", lambda: plan)
    return conv, plan


def test_member_routing_on_a_fake_plan(converter):
    from riffusion import _autograd

    conv, plan = converter
    mel = torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(1))
    plain = conv.inverse_mel_scaler(mel, inverse_mel="lstsq")
    assert plain.grad_fn is None and not plain.requires_grad and tuple(plain.shape) == (2, 7, 5)
    m = mel.clone().requires_grad_(True)
    with torch.no_grad():
        assert conv.inverse_mel_scaler(m, inverse_mel="lstsq").grad_fn is None
    assert "backward" not in plan.calls
    out = conv.inverse_mel_scaler(m, inverse_mel="lstsq")
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    gx = torch.randn(out.shape, generator=torch.Generator().manual_seed(3))
    out.backward(gx)
    assert plan.calls.count("backward") == 1
    ref = mel.clone().requires_grad_(True)
    torch.relu(plan.A @ ref).backward(gx)
    assert torch.allclose(m.grad, ref.grad, rtol=1e-6, atol=1e-6)
    # mel is the only saved tensor
    direct = _autograd.inverse_mel_lstsq(plan, m)
    assert type(direct.grad_fn).__name__ == "InverseMelLstsqFunctionBackward"
    saved = direct.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].data_ptr() == m.data_ptr() and tuple(saved[0].shape) == (2, 3, 5)
    # leading dimensions, as mel_scaler takes them
    lead = conv.inverse_mel_scaler(mel.reshape(2, 1, 3, 5).expand(2, 4, 3, 5), inverse_mel="lstsq")
    assert tuple(lead.shape) == (2, 4, 7, 5) and torch.equal(lead[:, 2], plain)
    assert tuple(conv.inverse_mel_scaler(mel[0], inverse_mel="lstsq").shape) == (7, 5)


def test_double_backward_raises(converter):
    conv, plan = converter
    m = torch.randn(1, 3, 4, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    out = conv.inverse_mel_scaler(m, inverse_mel="lstsq")
    (g,) = torch.autograd.grad(out, m, torch.ones_like(out, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_keyword_refusals_and_the_default(converter):
    conv, plan = converter
    mel = torch.ones(1, 3, 4)
    with pytest.raises(ValueError, match="spec0"):
        conv.inverse_mel_scaler(mel, inverse_mel="lstsq", spec0=torch.ones(1, 4, 7))
    with pytest.raises(ValueError, match="seed"):
        conv.inverse_mel_scaler(mel, inverse_mel="lstsq", seed=3)
    with pytest.raises(ValueError, match="inverse_mel must be one of"):
        conv.inverse_mel_scaler(mel, inverse_mel="pinv")
    assert plan.calls == []
    # the default is the SGD call, and a gradient-requiring input still gives a tensor without grad_fn
    out = conv.inverse_mel_scaler(mel.clone().requires_grad_(True), seed=9)
    assert plan.calls == [("sgd", 9)] and out.grad_fn is None
    assert torch.equal(conv.inverse_mel_scaler(mel, seed=9, inverse_mel="sgd"), out)


def test_header_compiles_as_c99_with_the_entries(tmp_path):
    emu_build.header_compiles_as_c99(
        tmp_path,
        '#include "rfx.h"\n'
        "size_t q(const rfx_plan* p) { return rfx_inverse_mel_lstsq_backward_workspace_bytes(p, 1, 41); }\n"
        "int r(const rfx_plan* p, const float* mel, const float* gx, float* g, void* ws) {\n"
        "  return rfx_inverse_mel_lstsq_backward(p, mel, gx, 1, 41, g, ws, 0, 0); }\n"
        "int s(const rfx_params* p, const float* fb, int32_t* a, float* w, int32_t* n) {\n"
        "  return rfx_debug_lstsq_collect(p, fb, a, a, a, w, 0, n); }\n")
    from riffusion import _hip

    lib = _hip.load_library()
    assert lib.rfx_inverse_mel_lstsq_backward_workspace_bytes(None, 1, 41) == 0
    assert lib.rfx_inverse_mel_lstsq_backward(None, None, None, 1, 41, None, None, 0, None) == -1 and b"null argument" in lib.rfx_last_error()
