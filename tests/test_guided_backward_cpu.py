"""
CPU checks of the backward of the zero-iteration guided decode (include/rfx.h: rfx_griffinlim_guided_backward,
rfx_waveform_from_mel_guided_backward; kernels guide_stage_rows_kernel of csrc/rfx_guide.hip and guide_project_kernel of
csrc/rfx_guide_bwd.hip), and the helpers tests/test_gpu_guided_backward.py shares.

tests/emu/rfx_guide_bwd_emu.cpp runs the arithmetic header's staging and projection (rfx_guide_core.h) over the tables the library
reports (rfx_debug_guide_project_tables).  Around it the chain is restated in float32 torch where no host emulator covers an engine's
frame transform - the STFT of the staged guide, the synthesis adjoint G - and closed by the host emulator of the closed form's backward
(tests/emu/rfx_imel_lstsq_bwd_emu.cpp):
    g_w -> G (float32 torch) ; guide -> staged (emulator) -> a (float32 torch) ; (G, a) -> g_S (emulator) -> g_mel (emulator)

* Against float64 torch autograd of istft(x a / |a|), x = relu(lstsq(mel)), composed from tests/istft_oracle.py and
  test_imel_lstsq_cpu.lstsq_reference's expression: g_S and g_mel at most twice the distance of the same chain in float32 torch,
  overall and for the worst frame.  The inputs - Gaussian guide rows, a Gaussian g_w, image-tile mels - keep float32 torch itself well
  behaved: its own distance stays below 1e-4, overall and in the worst frame (measured: 2e-6 and 1.3e-5).  For g_mel the relu's edge
  is taken out of the comparison as tests/test_imel_lstsq_bwd_cpu.py takes it out: the positions float64 cannot decide for float32
  pass no gradient, in all chains, and are at most GUARD_SHARE of the positions with a filter.
* Exact consequences, bit for bit: a silent guide row gives a zero gradient row; a guide shorter than the clip equals the same guide
  zero-padded by the caller; guide * 2^m gives the same bytes; g_w * 2^k gives g_S * 2^k.
* The tables: every bin has a slot, a slot's position holds its bin, padding maps to padding.
* The entries' null-argument refusals and queries without a GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

import imel_lstsq_bwd_cases as bcpu
import imel_lstsq_cases as cpu
import istft_oracle as IO
from guided_backward_cases import emu_project, emu_stage_rows, emulator, inputs, relu_guard, tables, torch_chain

CASES = {  # name: (SpectrogramParams keywords, B, T, loop)
    "default": (dict(), 2, 23, False),
    "8khz_64": (dict(sample_rate=8000, num_frequencies=64, max_frequency=4000), 2, 24, False),
    "default-loop": (dict(), 2, 41, True),
}


@pytest.fixture(scope="module")
def O():
    import riffusion_oracle

    return riffusion_oracle


@pytest.fixture(scope="module")
def emu():
    return emulator()


@pytest.fixture(scope="module")
def emus():
    return bcpu.emulators()


# ---- the emulator chain -------------------------------------------------------------------------------------------------------------
def to_cube(X, xpos_bin):
    """(B, F, T) complex -> (B * T, stride) complex64: every position holds its bin's value (padding: NaN - it must not matter)"""
    B, F, T = X.shape
    flat = X.to(torch.complex64).permute(0, 2, 1).reshape(B * T, F)
    out = torch.full((B * T, len(xpos_bin)), complex(float("nan"), float("nan")), dtype=torch.complex64)
    held = torch.from_numpy(xpos_bin >= 0)
    out[:, held] = flat[:, torch.from_numpy(xpos_bin[xpos_bin >= 0]).long()]
    return out


def from_slots(slots, pos_bin, B, T, F):
    """(B * T, stride) magnitude slots -> (B, F, T): every bin from its first slot"""
    first = np.full(F, -1, np.int64)
    for p in range(len(pos_bin) - 1, -1, -1):
        if pos_bin[p] >= 0:
            first[pos_bin[p]] = p
    assert (first >= 0).all()
    return slots[:, torch.from_numpy(first)].reshape(B, T, F).permute(0, 2, 1).contiguous()


_cases = {}


def _case(O, emu, name):  # noqa: F811
    if name not in _cases:
        kw, B, T, loop = CASES[name]
        op, cp, fb = cpu.bank(**kw)
        L = IO.samples(op, T, loop)
        mel = torch.cat([cpu.image_mel(fb.shape[1], T, seed=3 + i) for i in range(B)]).contiguous()
        guide, g_w = inputs(B, L)
        xpos_bin, s2x = tables(cp)
        pos_bin = np.where(s2x >= 0, xpos_bin[np.maximum(s2x, 0)], -1)
        G32 = IO.istft_grad(O, torch.zeros((B, fb.shape[0], T), dtype=torch.complex64), g_w, op, torch.float32, loop)

        def stage(gd, gw_scale=1.0):
            A = IO.stft(O, emu_stage_rows(emu, gd, L), op, torch.float32, loop)
            return emu_project(emu, to_cube(G32 * gw_scale, xpos_bin), to_cube(A, xpos_bin), xpos_bin, s2x)

        _cases[name] = dict(op=op, cp=cp, fb=fb, B=B, T=T, L=L, loop=loop, mel=mel, guide=guide, g_w=g_w, xpos_bin=xpos_bin, s2x=s2x, pos_bin=pos_bin,
                            stage=stage, gS_slots=stage(guide))
    return _cases[name]


@pytest.mark.parametrize("name", list(CASES))
def test_tables(name):
    kw, B, T, loop = CASES[name]
    op, cp, fb = cpu.bank(**kw)
    xpos_bin, s2x = tables(cp)
    F = fb.shape[0]
    assert len(xpos_bin) == len(s2x) == bcpu.frame_stride(op) and len(s2x) % 4 == 0
    assert xpos_bin.min() == -1 and s2x.min() == -1 and s2x.max() < len(xpos_bin)
    assert set(xpos_bin[xpos_bin >= 0]) == set(range(F))
    pos_bin = np.where(s2x >= 0, xpos_bin[np.maximum(s2x, 0)], -1)
    assert set(pos_bin[pos_bin >= 0]) == set(range(F)) and (pos_bin[s2x >= 0] >= 0).all()
    # the counted copy of the closed form's backward holds the bin the projection writes there
    ptr, bins, pos, w = bcpu.lists(cp, fb)
    assert np.array_equal(pos_bin[pos], bins)
    twice = int((pos_bin >= 0).sum()) - F
    assert twice == (440 if not kw else 0)
    # a magnitude slot's spectrum position is one of its own: no two slots share one
    assert len(np.unique(s2x[s2x >= 0])) == int((s2x >= 0).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_emulator_chain_against_float64_autograd(O, emu, emus, name):  # noqa: F811
    fwd, bwd = emus
    d = _case(O, emu, name)
    fb, mel, B, T = d["fb"], d["mel"], d["B"], d["T"]
    F = fb.shape[0]
    keep, share = relu_guard(fb, mel)
    assert share <= bcpu.GUARD_SHARE
    gS64, gm64 = torch_chain(O, d["op"], fb, mel, d["guide"], d["g_w"], d["loop"], torch.float64, keep)
    gS32, gm32 = torch_chain(O, d["op"], fb, mel, d["guide"], d["g_w"], d["loop"], torch.float32, keep)
    slots = d["gS_slots"]
    assert bool(torch.isfinite(slots).all())  # every float written and finite, padding included
    assert bool((slots[:, torch.from_numpy(d["pos_bin"] < 0)] == 0).all())
    gS = from_slots(slots, d["pos_bin"], B, T, F)
    _, tabs = cpu.report(d["cp"], fb, tables=True)
    lst = bcpu.lists(d["cp"], fb)
    keep_slots = torch.from_numpy(bcpu.to_slots(keep.to(torch.float32), lst, slots.shape[1], fill=0.0))
    gmel = bcpu.emu_backward(bwd, fb, tabs, lst, mel, (slots * keep_slots).numpy())
    for what, got, g32, ref in (("g_S", gS, gS32, gS64), ("g_mel", gmel, gm32, gm64)):
        ours, torch32 = bcpu.distances(got, ref), bcpu.distances(g32, ref)
        print(f"{name} {what}: emulator chain rel-L2 {ours[0]:.2e} (worst frame {ours[1]:.2e}); float32 torch chain {torch32[0]:.2e} (worst frame "
              f"{torch32[1]:.2e}); marked share {share:.3%}")
        # (an ill-conditioned phase - a guide bin with |a| near 0 - would cost float32 torch whole digits: 1e-4 is a thousand roundings)
        assert torch32[0] < 1e-4 and torch32[1] < 1e-4, "the inputs must keep float32 torch itself well behaved"
        assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1], what


@pytest.mark.parametrize("name", ["default", "8khz_64"])
def test_exact_consequences(O, emu, name):  # noqa: F811
    d = _case(O, emu, name)
    B, T, L, stage, ref = d["B"], d["T"], d["L"], d["stage"], d["gS_slots"]
    bits = lambda t: t.numpy().tobytes()  # noqa: E731
    silent = d["guide"].clone()
    silent[1] = 0
    got = stage(silent).reshape(B, T, -1)
    assert bool((got[1] == 0).all()) and bits(got[0]) == bits(ref.reshape(B, T, -1)[0]) and bool((ref.reshape(B, T, -1)[1] != 0).any())
    short = d["guide"][:, : L - 1001].contiguous()
    a = stage(short)
    assert bits(a) == bits(stage(torch.nn.functional.pad(short, (0, 1001)))) and bits(a) != bits(ref)
    assert bits(stage(torch.cat([d["guide"], torch.full((B, 77), 1e9)], dim=1))) == bits(ref)
    for m in (-20, 9, 100):
        assert bits(stage(d["guide"] * 2.0 ** m)) == bits(ref), m
    for k in (-40, 40):
        assert bits(stage(d["guide"], 2.0 ** k)) == bits(ref * 2.0 ** k), k


def test_staging_is_the_forwards(emu):  # noqa: F811
    """fit, peak and power of two as the forward's staging has them (tests/test_guided_start_cpu.py): the peak lands in [2^14, 2^15)"""
    g = torch.Generator().manual_seed(1)
    guide = torch.randn((3, 1000), generator=g) * torch.tensor([[1e-20], [3.0], [7e12]])
    guide[1, 500:] = 0
    out = emu_stage_rows(emu, guide, 1300)
    assert out.shape == (3, 1300) and bool((out[:, 1000:] == 0).all())
    peak = out.abs().amax(dim=1)
    assert bool((peak >= 2.0 ** 14).all()) and bool((peak < 2.0 ** 15).all())
    ratio = out[:, :1000] / guide
    for r in range(3):
        vals = ratio[r][guide[r] != 0]
        assert bool((vals == vals[0]).all()) and float(torch.log2(vals[0])) == round(float(torch.log2(vals[0])))
    cut = emu_stage_rows(emu, guide, 400)
    assert cut.shape == (3, 400) and bool((cut[1] != 0).all())


def test_entries_without_a_gpu():
    from riffusion import _hip

    lib = _hip.load_library()
    for stem in ("rfx_griffinlim_guided_backward", "rfx_waveform_from_mel_guided_backward"):
        for form in ("", "_loop"):
            assert getattr(lib, f"{stem}{form}_workspace_bytes")(None, 1, 41) == 0
    assert lib.rfx_griffinlim_guided_backward(None, None, 1, None, 1, 41, None, None, 0, None) == -1 and b"null argument" in lib.rfx_last_error()
    assert lib.rfx_griffinlim_guided_backward_loop(None, None, 1, None, -1, 41, None, None, 0, None) == -1 and b"negative" in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_guided_backward(None, None, None, 1, None, 1, 41, None, None, 0, None) == -1
    assert b"rfx_waveform_from_mel_guided_backward: null argument" in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_guided_backward_loop(None, None, None, 1, None, 0, 41, None, None, 0, None) == 0
    n = ctypes.c_int32(0)
    assert lib.rfx_debug_guide_project_tables(None, None, None, 0, ctypes.byref(n)) == -1


def test_autograd_routing_on_a_fake_plan():
    """GuidedDecodeFunction saves mel and the guide, hands the backward entry what it takes and refuses a second differentiation"""
    from riffusion import _autograd

    calls = []

    class Plan:
        def waveform_from_mel(self, mel, cpc, n_iter, momentum, seed=0, lstsq=False, guide=None, loop=False):
            calls.append(("fwd", cpc, n_iter, lstsq, loop, tuple(guide.shape)))
            return mel.sum(dim=1) * 2.0

        def waveform_from_mel_guided_backward(self, mel, guide, grad, loop):
            calls.append(("bwd", tuple(mel.shape), tuple(guide.shape), grad.dtype, grad.is_contiguous(), loop))
            return grad[:, None, :].expand_as(mel) * 2.0

    mel = torch.rand((2, 4, 5), requires_grad=True)
    guide = torch.rand((2, 9))
    out = _autograd.guided_decode(Plan(), mel, guide, True, 7)
    assert out.grad_fn is not None
    out.backward(torch.ones((2, 5), dtype=torch.float64).to(torch.float32).t().contiguous().t())
    assert calls == [("fwd", 2, 0, True, True, (2, 9)), ("bwd", (2, 4, 5), (2, 9), torch.float32, True, True)]
    assert torch.equal(mel.grad, torch.full((2, 4, 5), 2.0))
    with pytest.raises(RuntimeError, match="guide"):
        _autograd.guided_decode(Plan(), mel, guide.clone().requires_grad_(True), False, 0)
