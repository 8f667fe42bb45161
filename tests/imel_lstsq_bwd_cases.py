"""
What the tests of the closed-form InverseMelScale's gradient share (TEST INFRASTRUCTURE ONLY; tests/test_imel_lstsq_bwd_cpu.py,
tests/test_gpu_imel_lstsq_bwd.py and the guided decode's gradient tests): the host emulator (csrc/rfx_imel_lstsq_bwd_core.h compiled
for the host with tests/emu/rfx_imel_lstsq_bwd_emu.cpp) beside the forward's, built once per process, the gather lists, gradients in
slot layout, torch autograd as the reference, and the guard that leaves out the positions where float32 cannot decide the relu.
"""
import ctypes
import functools

import numpy as np
import torch

import emu_build
import imel_lstsq_cases

EMU_SRC = "rfx_imel_lstsq_bwd_emu.cpp"
GUARD = 1e-3        # |v| < GUARD * (fb |y|): the relu's side is not decided in float32
GUARD_SHARE = 5e-3  # ... which may hold for this share of the positions with a filter


@functools.lru_cache(maxsize=1)
def emulators():
    """(the forward's emulator, the backward's)"""
    bwd = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    bwd.emu_inverse_mel_lstsq_backward.argtypes = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    return imel_lstsq_cases.emulator(), bwd


def lists(cp, fb):
    from riffusion import _hip

    return _hip.lstsq_collect_lists(cp, fb)


def frame_stride(op):
    from helpers import plan_bank_report

    return int(plan_bank_report(op).frame_stride)


def to_slots(g_bft: torch.Tensor, lst, stride: int, fill=np.nan) -> np.ndarray:
    """(B, F, T) gradient -> [B * T][stride] with every bin at the position the lists name, `fill` everywhere else"""
    ptr, bins, pos, w = lst
    B, F, T = g_bft.shape
    out = np.full((B * T, stride), fill, np.float32)
    out[:, pos] = g_bft.permute(0, 2, 1).reshape(B * T, F).numpy()[:, bins]
    return out


def emu_backward(bwd, fb, tables, lst, mel, gx_slots):
    """mel (B, M, T) float32 tensor, gx [B * T][stride] float32 array -> g_mel (B, M, T) float32 tensor by the emulator"""
    neg_l, inv_d = tables
    ptr, bins, pos, w = lst
    F, M = fb.shape
    B, _, T = mel.shape
    mel = np.ascontiguousarray(mel.numpy(), dtype=np.float32)
    fbn = np.ascontiguousarray(fb.numpy(), dtype=np.float32)
    gx_slots = np.ascontiguousarray(gx_slots, dtype=np.float32)
    assert gx_slots.shape[0] == B * T, (gx_slots.shape[0], B * T)
    out = np.full((B, M, T), np.nan, np.float32)
    bwd.emu_inverse_mel_lstsq_backward(fbn.ctypes.data, neg_l.ctypes.data, inv_d.ctypes.data, ptr.ctypes.data, bins.ctypes.data, pos.ctypes.data,
                                       w.ctypes.data, mel.ctypes.data, gx_slots.ctypes.data, B, F, M, T, gx_slots.shape[1], None, out.ctypes.data)
    return torch.from_numpy(out)


def torch_gradient(fb, mel, gx, dtype):
    """d <gx, relu(lstsq(fb.T, mel).solution)> / d mel by torch autograd in `dtype`, and the forward's result"""
    m = mel.to(dtype).clone().requires_grad_(True)
    x = torch.relu(torch.linalg.lstsq(fb.T[None].to(dtype), m, driver="gels").solution)
    (g,) = torch.autograd.grad(x, m, gx.to(dtype))
    return g, x.detach()


def guarded_gradient(fb, mel, seed=11):
    """a random (B, F, T) gradient, zero where float64 cannot tell float32 which side of the relu a position is on; the marked share"""
    G = fb.double().T @ fb.double()
    y = torch.linalg.solve(G, mel.double())
    v, bound = fb.double() @ y, fb.double() @ y.abs()
    reached = (fb != 0).any(dim=1)[None, :, None].expand_as(v)
    marked = (v.abs() < GUARD * bound) & reached
    gx = torch.randn(v.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    gx[marked] = 0.0
    share = float(marked.sum()) / float(reached.sum())
    return gx, share, (v > 0) & reached


def distances(g, ref):
    diff = g.double() - ref
    return float(diff.norm() / ref.norm()), float((diff.norm(dim=1) / ref.norm(dim=1)).max())
