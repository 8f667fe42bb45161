"""
The backward of the closed-form InverseMelScale on the device (csrc/rfx_imel_lstsq.hip: lsq_collect_kernel; include/rfx.h:
rfx_inverse_mel_lstsq_backward) and what is built on it: Plan.inverse_mel_lstsq_backward, InverseMelLstsqFunction and
SpectrogramConverter.inverse_mel_scaler(..., inverse_mel="lstsq").

Shapes: those of tests/test_gpu_imel_lstsq.py, the smallest that can still go wrong - the default plan with B = 3, T = 37 (no
multiple of the 16 frames a collect workgroup stages nor of the 64 lanes of a solve wave; the slot cube with twice-held bins and
padding), the same with mel_scale_norm = "slaney", and 8 kHz with 64 filters, B = 2, T = 21 (plain bin-ordered frames, fewer
filters than the collect workgroup has lanes).

Bounds.  Device against emulator, the uncounted positions, batch invariance and the power-of-two scaling are bit equality.
Against float64 torch autograd: at most 2 times the distance of float32 torch autograd on the same input, overall and for the worst
frame, with the guard of tests/test_imel_lstsq_bwd_cpu.py on the incoming gradient.  End to end (mel -> lstsq -> polar -> istft ->
spectral convergence) the same rule against the chain composed from the oracles in float64 and float32.
"""
import numpy as np
import pytest
import torch

import imel_lstsq_bwd_cases as bcpu
import imel_lstsq_cases as cpu
import istft_oracle as IO
import spec_loss_oracle as SLO
from imel_lstsq_cases import CANARY, DEVICE_CASES as CASES, _bits, _mel, _params, _plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emus():
    return bcpu.emulators()


_cases = {}


def _case(name):
    """per case, once: plan, bank, tables, lists, the input, a guarded gradient (host, and packed on the device), the device result"""
    if name not in _cases:
        kw, B, T = CASES[name]
        plan = _plan(**kw)
        op, cp, fb = cpu.bank(**kw)
        assert torch.equal(fb, plan.melfb) and plan.lstsq_ok
        _, tables = cpu.report(cp, fb, tables=True)
        lst = bcpu.lists(cp, fb)
        mel = _mel(plan.n_mels, B, T)
        gx, share, open64 = bcpu.guarded_gradient(fb, mel)
        gx_slots = plan.pack_magnitudes(gx.cuda())
        got = plan.inverse_mel_lstsq_backward(mel.cuda(), gx_slots)
        torch.cuda.synchronize()
        _cases[name] = dict(plan=plan, op=op, fb=fb, tables=tables, lists=lst, B=B, T=T, mel=mel, gx=gx, share=share, gx_slots=gx_slots, got=got)
    return _cases[name]


def _positions(plan):
    """bin of every position of a frame (-1: padding): pack a frame whose bin f holds f + 1"""
    ramp = (torch.arange(plan.n_stft, dtype=torch.float32, device="cuda") + 1.0).reshape(1, -1, 1)
    return plan.pack_magnitudes(ramp).reshape(-1).round().long().cpu() - 1


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_emulator_and_meets_the_gate(emus, name):  # noqa: F811
    fwd, bwd = emus
    d = _case(name)
    plan, fb, mel, gx = d["plan"], d["fb"], d["mel"], d["gx"]
    assert tuple(d["gx_slots"].shape) == (d["B"] * d["T"], plan.frame_stride)
    want = bcpu.emu_backward(bwd, fb, d["tables"], d["lists"], mel, d["gx_slots"].cpu().numpy())
    got = d["got"].cpu()
    assert got.shape == want.shape == mel.shape
    assert _bits(got) == _bits(want)
    assert d["share"] <= bcpu.GUARD_SHARE
    ref, _ = bcpu.torch_gradient(fb, mel, gx, torch.float64)
    g32, _ = bcpu.torch_gradient(fb, mel, gx, torch.float32)
    ours, torch32 = bcpu.distances(got, ref), bcpu.distances(g32, ref)
    print(f"{name}: marked share {d['share']:.3%}; device rel-L2 {ours[0]:.2e} (worst frame {ours[1]:.2e}); torch float32 autograd {torch32[0]:.2e} "
          f"(worst frame {torch32[1]:.2e})")
    assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1]


def test_a_bank_with_five_vectors_per_lane_equals_the_emulator(emus):  # noqa: F811
    """the collect kernel is instantiated per number of 16-byte vectors a lane masks: the three cases take 3 and 1, the 20 Hz .. 20 kHz
    bank (7991 bins with a filter in 2208 vectors of the slot cube, runs of up to 107 bins) takes 5"""
    fwd, bwd = emus
    kw, B, T = dict(min_frequency=20, max_frequency=20000), 1, 17
    plan = _plan(**kw)
    op, cp, fb = cpu.bank(**kw)
    _, tables = cpu.report(cp, fb, tables=True)
    lst = bcpu.lists(cp, fb)
    assert plan.lstsq_ok and 4 * 512 < len(np.unique(lst[2] // 4)) <= 5 * 512
    mel = _mel(plan.n_mels, B, T)
    gx = torch.randn((B, plan.n_stft, T), generator=torch.Generator().manual_seed(2))
    gx_slots = plan.pack_magnitudes(gx.cuda())
    got = plan.inverse_mel_lstsq_backward(mel.cuda(), gx_slots)
    want = bcpu.emu_backward(bwd, fb, tables, lst, mel, gx_slots.cpu().numpy())
    assert bool((got != 0).any()) and _bits(got) == _bits(want)


@pytest.mark.parametrize("name", list(CASES))
def test_only_the_counted_copy_of_a_bin_matters(name):
    d = _case(name)
    plan, fb, (ptr, bins, pos, w) = d["plan"], d["fb"], d["lists"]
    pos_bin = _positions(plan)
    counted = torch.zeros(plan.frame_stride, dtype=torch.bool)
    counted[torch.from_numpy(np.unique(pos)).long()] = True
    # the listed position of a bin holds that bin
    assert np.array_equal(pos_bin[torch.from_numpy(pos).long()].numpy(), bins)
    reached = torch.cat([(fb != 0).any(dim=1), torch.zeros(1, dtype=torch.bool)])[pos_bin]  # (index -1: padding, not reached)
    padding = pos_bin < 0
    other_copy = (pos_bin >= 0) & reached & ~counted
    unreached = (pos_bin >= 0) & ~reached
    assert int(counted.sum()) == int((fb != 0).any(dim=1).sum()) and int(padding.sum()) > 0 and int(unreached.sum()) > 0
    twice = int((pos_bin >= 0).sum()) - plan.n_stft
    assert twice == (0 if plan.generic else 440) and int(other_copy.sum()) <= twice
    if not plan.generic:
        assert int(other_copy.sum()) > 0
    mel_d = d["mel"].cuda()
    for mask, value in ((padding, float("nan")), (other_copy, float("nan")), (unreached, 3e30)):
        if int(mask.sum()) == 0:
            continue
        junk = d["gx_slots"].clone()
        junk[:, mask.cuda()] = value
        assert _bits(plan.inverse_mel_lstsq_backward(mel_d, junk)) == _bits(d["got"])


@pytest.mark.parametrize("name", list(CASES))
def test_workspace_canary_inputs_and_row_alone(name):
    d = _case(name)
    plan, B, T = d["plan"], d["B"], d["T"]
    lib = plan.lib
    need = lib.rfx_inverse_mel_lstsq_backward_workspace_bytes(plan.handle, B, T)
    assert need >= 2 * B * plan.n_mels * T * 4
    n = B * plan.n_mels * T
    ws = torch.full((need + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((n + CANARY // 4,), -7.0, dtype=torch.float32, device="cuda")
    d_mel, d_gx = d["mel"].cuda(), d["gx_slots"].clone()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.rfx_inverse_mel_lstsq_backward(plan.handle, d_mel.data_ptr(), d_gx.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((out[n:] == -7.0).all())
    assert _bits(out[:n]) == _bits(d["got"])
    assert _bits(d_mel) == _bits(d["mel"]) and _bits(d_gx) == _bits(d["gx_slots"])
    # a short workspace and misaligned slots are refused
    assert lib.rfx_inverse_mel_lstsq_backward(plan.handle, d_mel.data_ptr(), d_gx.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need - 1, stream) == -3
    assert lib.rfx_inverse_mel_lstsq_backward(plan.handle, d_mel.data_ptr(), d_gx.data_ptr() + 4, B, T, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert b"16-byte aligned" in lib.rfx_last_error()
    assert lib.rfx_inverse_mel_lstsq_backward(plan.handle, d_mel.data_ptr(), d_gx.data_ptr(), 0, T, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    # row 1 alone
    alone = plan.inverse_mel_lstsq_backward(d_mel[1:2].contiguous(), d_gx[T:2 * T].contiguous())
    assert _bits(alone) == _bits(d["got"][1:2])


@pytest.mark.parametrize("name", list(CASES))
def test_power_of_two_scaling_is_exact(name):
    d = _case(name)
    plan = d["plan"]
    assert bool((d["got"] != 0).any()) and bool(torch.isfinite(d["got"]).all())
    mel_d = d["mel"].cuda()
    for k in (-40, 40):
        assert _bits(plan.inverse_mel_lstsq_backward(mel_d, d["gx_slots"] * 2.0 ** k)) == _bits(d["got"] * 2.0 ** k), k


def test_a_singular_bank_is_refused_before_any_launch():
    from riffusion.spectrogram_converter import SpectrogramConverter

    plan = _plan(num_frequencies=1024)
    lib = plan.lib
    B, T, sentinel = 1, 22, 12345.0
    assert not plan.lstsq_ok and lib.rfx_inverse_mel_lstsq_backward_workspace_bytes(plan.handle, B, T) == 0
    mel = torch.ones((B, plan.n_mels, T), device="cuda")
    gx = torch.ones((B * T, plan.frame_stride), device="cuda")
    out = torch.full((B, plan.n_mels, T), sentinel, device="cuda")
    ws = torch.full((2 * B * plan.n_mels * T * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.rfx_inverse_mel_lstsq_backward(plan.handle, mel.data_ptr(), gx.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), ws.numel(), stream) == -1
    assert b"pivot" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((ws == 0xA5).all())
    with pytest.raises(ValueError, match="pivot"):
        plan.inverse_mel_lstsq_backward(mel, gx)
    conv = SpectrogramConverter(_params(num_frequencies=1024), device="cuda")
    with pytest.raises(ValueError, match="pivot"):
        conv.inverse_mel_scaler(mel, inverse_mel="lstsq")


# ---- the member --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "8khz_64"])
def test_the_member(name):
    from riffusion.spectrogram_converter import SpectrogramConverter

    d = _case(name)
    plan, B, T = d["plan"], d["B"], d["T"]
    conv = SpectrogramConverter(_params(**CASES[name][0]), device="cuda")
    mel_d = d["mel"].cuda()
    want = plan.unpack_magnitudes(plan.inverse_mel_lstsq(mel_d), B, T)
    plain = conv.inverse_mel_scaler(mel_d, inverse_mel="lstsq")
    assert plain.grad_fn is None and _bits(plain) == _bits(want)
    leaf = mel_d.clone().requires_grad_(True)
    with torch.no_grad():
        assert conv.inverse_mel_scaler(leaf, inverse_mel="lstsq").grad_fn is None
    out = conv.inverse_mel_scaler(leaf, inverse_mel="lstsq")
    assert out.grad_fn is not None and _bits(out) == _bits(want)
    out.backward(d["gx"].cuda())
    assert _bits(leaf.grad) == _bits(d["got"])
    # leading dimensions, and a CPU leaf: autograd carries the copy
    cpu_leaf = d["mel"][:2].reshape(2, 1, plan.n_mels, T).clone().requires_grad_(True)
    lead = conv.inverse_mel_scaler(cpu_leaf, inverse_mel="lstsq")
    assert tuple(lead.shape) == (2, 1, plan.n_stft, T) and _bits(lead) == _bits(want[:2])
    lead.backward(d["gx"][:2].reshape(2, 1, plan.n_stft, T).cuda())
    assert cpu_leaf.grad.device.type == "cpu" and _bits(cpu_leaf.grad.reshape(2, plan.n_mels, T)) == _bits(d["got"][:2])
    with pytest.raises(ValueError, match="seed"):
        conv.inverse_mel_scaler(mel_d, inverse_mel="lstsq", seed=1)


def test_the_default_form_is_todays_call():
    from riffusion.spectrogram_converter import SpectrogramConverter

    plan = _plan()
    conv = SpectrogramConverter(_params(), device="cuda")
    mel = _mel(plan.n_mels, 1, 22).cuda()
    today = plan.unpack_magnitudes(plan.inverse_mel(mel, 1, spec0=None, seed=conv._seed(5)), 1, 22)
    default = conv.inverse_mel_scaler(mel.clone().requires_grad_(True), seed=5)
    assert default.grad_fn is None and _bits(default) == _bits(today)
    assert _bits(conv.inverse_mel_scaler(mel, seed=5, inverse_mel="sgd")) == _bits(today)


def test_end_to_end_from_a_loss_on_audio_to_the_mel_tile():
    """mel -> lstsq -> torch.polar(x, fixed phase) -> waveform_from_spectrogram -> spectral_losses(...).convergence.sum().backward(),
    against the same chain composed from the oracles in float64, at most twice the distance of that chain in float32 torch"""
    import riffusion_oracle as O
    from riffusion.spectrogram_converter import SpectrogramConverter

    name = "8khz_64"
    d = _case(name)
    plan, op, fb, B = d["plan"], d["op"], d["fb"], d["B"]
    # the case's T = 21 gives hop * 20 = 1600 samples, exactly the n_fft / 2 of reflect padding torch.stft refuses to analyse: the
    # shortest chain that exists has 22 frames; 24 is no multiple of the 16 staged frames either
    T = 24
    mel = _mel(plan.n_mels, B, T)
    g = torch.Generator().manual_seed(17)
    phase = (torch.rand((B, plan.n_stft, T), generator=g, dtype=torch.float64) * 2 - 1) * np.pi
    target = cpu.lstsq_reference(fb, _mel(plan.n_mels, B, T, seed=7), torch.float32).contiguous()

    def oracle(dtype):
        leaf = mel.to(dtype).clone().requires_grad_(True)
        x = torch.relu(torch.linalg.lstsq(fb.T[None].to(dtype), leaf, driver="gels").solution)
        y = IO.istft(O, torch.polar(x, phase.to(dtype)), op, dtype)
        a = SLO.stft(y, op, False, dtype).abs()
        loss = SLO.losses_of_magnitudes(a, target.to(dtype), None)[0].sum()
        loss.backward()
        return leaf.grad.detach(), float(loss.detach())

    ref, loss64 = oracle(torch.float64)
    g32, loss32 = oracle(torch.float32)
    conv = SpectrogramConverter(_params(**CASES[name][0]), device="cuda")
    leaf = mel.cuda().requires_grad_(True)
    x = conv.inverse_mel_scaler(leaf, inverse_mel="lstsq")
    wave = conv.waveform_from_spectrogram(torch.polar(x, phase.to(torch.float32).cuda()))
    loss = conv.spectral_losses(wave, target.cuda()).convergence.sum()
    loss.backward()
    got = leaf.grad.cpu()
    assert bool(torch.isfinite(got).all()) and bool((got != 0).any())
    ours, torch32 = bcpu.distances(got, ref), bcpu.distances(g32, ref)
    print(f"end to end: loss {float(loss.detach()):.6f} (float64 {loss64:.6f}, float32 torch {loss32:.6f}); device gradient rel-L2 {ours[0]:.2e} "
          f"(worst frame {ours[1]:.2e}); float32 torch chain {torch32[0]:.2e} (worst frame {torch32[1]:.2e})")
    assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1]
