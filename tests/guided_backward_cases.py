"""
What the tests of the guided decode's gradient share (TEST INFRASTRUCTURE ONLY; tests/test_guided_backward_cpu.py and
tests/test_gpu_guided_backward.py): the seeded guides and upstream gradients, the projection tables, the host emulator
(csrc/rfx_guide_bwd_core.h compiled for the host with tests/emu/rfx_guide_bwd_emu.cpp), built once per process, the relu guard and
the torch autograd chain that is the reference.
"""
import ctypes
import functools

import numpy as np
import torch

import emu_build
import imel_lstsq_bwd_cases as bcpu
import istft_oracle as IO

EMU_SRC = "rfx_guide_bwd_emu.cpp"


@functools.lru_cache(maxsize=1)
def emulator():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    lib.emu_guide_stage_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.emu_guide_project.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def inputs(B, L, seed=23):
    """seeded Gaussian guide rows (B, L) in about the units of a float waveform, and a seeded Gaussian g_w (B, L)"""
    g = torch.Generator().manual_seed(seed + B + L)
    return (0.1 * torch.randn((B, L), generator=g)).contiguous(), torch.randn((B, L), generator=g).contiguous()


def tables(cp):
    """(xpos_bin, s2x) of rfx_debug_guide_project_tables: int32 arrays of one frame's positions"""
    from riffusion import _hip

    lib = _hip.load_library()
    n = ctypes.c_int32(0)
    _hip.check(lib.rfx_debug_guide_project_tables(ctypes.byref(cp), None, None, 0, ctypes.byref(n)))
    xpos_bin, s2x = np.full(n.value, -2, np.int32), np.full(n.value, -2, np.int32)
    _hip.check(lib.rfx_debug_guide_project_tables(ctypes.byref(cp), xpos_bin.ctypes.data, s2x.ctypes.data, n.value, ctypes.byref(n)))
    return xpos_bin, s2x


def plain_tables(n_stft, stride):
    """the tables of a plan with plain frames (position = bin), as every generic plan has them"""
    t = np.full(stride, -1, np.int32)
    t[:n_stft] = np.arange(n_stft, dtype=np.int32)
    return t, t.copy()


def emu_stage_rows(emu, guide, L):
    """(B, Lg) float32 guide -> the (B, L) rows the backward's forward transform analyses"""
    g = np.ascontiguousarray(guide.numpy(), dtype=np.float32)
    out = np.full((g.shape[0], L), np.nan, np.float32)
    emu.emu_guide_stage_rows(g.ctypes.data, g.shape[1], g.shape[0], L, out.ctypes.data)
    return torch.from_numpy(out)


def emu_project(emu, G, A, xpos_bin, s2x):
    """G, A: (frames, stride) complex64 slot cubes -> g_S (frames, stride) float32 in the magnitude slot layout"""
    g = np.ascontiguousarray(torch.view_as_real(G.contiguous()).numpy(), dtype=np.float32)
    a = np.ascontiguousarray(torch.view_as_real(A.contiguous()).numpy(), dtype=np.float32)
    frames, stride = G.shape
    assert A.shape == G.shape and len(xpos_bin) == stride == len(s2x), (A.shape, G.shape, len(xpos_bin), stride, len(s2x))
    out = np.full((frames, stride), np.nan, np.float32)
    emu.emu_guide_project(g.ctypes.data, a.ctypes.data, xpos_bin.ctypes.data, s2x.ctypes.data, frames, stride, stride, out.ctypes.data)
    return torch.from_numpy(out)


def relu_guard(fb, mel):
    """(keep (B, F, T) bool, marked share): imel_lstsq_bwd_cases.guarded_gradient's marking of the relu's undecided positions"""
    gx, share, _ = bcpu.guarded_gradient(fb, mel)
    return gx != 0, share


def fit(guide, L):
    """the guide cut or zero-padded at its end to L samples"""
    return guide[:, :L] if guide.shape[1] >= L else torch.nn.functional.pad(guide, (0, L - guide.shape[1]))


def torch_chain(O, op, fb, mel, guide, g_w, loop, dtype, keep):
    """(g_S (B, F, T), g_mel (B, M, T)) of w = istft(x a / |a|), x = relu(lstsq(mel)) [times `keep`], a = stft(guide), by torch
    autograd in `dtype`: g_S with respect to the magnitudes themselves (no guard), g_mel through the guarded relu"""
    a = IO.stft(O, fit(guide, g_w.shape[1]).to(dtype), op, dtype, loop)
    u = a / a.abs()
    leaf = mel.to(dtype).clone().requires_grad_(True)
    x = torch.relu(torch.linalg.lstsq(fb.T[None].to(dtype), leaf, driver="gels").solution)
    S = x.detach().clone().requires_grad_(True)
    IO.istft(O, S * u, op, dtype, loop).backward(g_w.to(dtype))
    IO.istft(O, (x * keep.to(dtype)) * u, op, dtype, loop).backward(g_w.to(dtype))
    return S.grad.detach(), leaf.grad.detach()
