"""
The backward of the zero-iteration guided decode on the device (csrc/rfx_guide_bwd.hip: guide_project_kernel; csrc/rfx_api_guided.hip;
include/rfx.h: rfx_griffinlim_guided_backward, rfx_waveform_from_mel_guided_backward and their loop forms) and what is built on it:
Plan.griffinlim_guided_backward, Plan.waveform_from_mel_guided_backward, GuidedDecodeFunction and
SpectrogramConverter.waveform_from_mel_amplitudes(..., inverse_mel="lstsq", guide=..., griffin_lim_iters=0).

Shapes, the smallest that can still go wrong: the default plan with B = 3, T = 37 (no multiple of 16 frames or 64 lanes; the slot
cube with twice-held bins and padding), the same with mel_scale_norm = "slaney", one case on each other frame engine whose bank the
closed form serves (row family at 48 kHz, generic at 11025 Hz; T >= 24 so that the guide outgrows the reflect padding), and the
loop form on each of the three with T = 41 >= n_fft / hop, no multiple of 16.  The chirp-z plan of tests/engines.py
has more filters than bins: the closed form does not serve it, so it takes the stage entry only.

Inputs: seeded Gaussian guide rows (every bin's phase is well conditioned in float32), `_mel` of tests/test_gpu_imel_lstsq.py, a
seeded Gaussian g_w.

Bounds.  Device against emulator, fused against stages, the member's bytes, batch invariance, the silent row, the short guide and the
power-of-two scalings are bit equality.  Against float64 torch autograd of istft(x a / |a|): at most 2 times the distance of the same
chain in float32 torch, overall and for the worst frame; for g_mel with the guard of tests/test_imel_lstsq_bwd_cpu.py on the relu's
edge (the positions float64 cannot decide for float32 pass no gradient, in all three chains; their share stays below GUARD_SHARE).
"""
import pytest
import torch

import guided_backward_cases as gcpu
import imel_lstsq_bwd_cases as bcpu
import imel_lstsq_cases as cpu
import istft_oracle as IO
import spec_loss_oracle as SLO
from engines import ENGINES
from imel_lstsq_cases import CANARY, _bits, _mel, _params

pytestmark = pytest.mark.gpu

CASES = {  # name: (engine of ENGINES, SpectrogramParams keywords on top of the engine's, B, T, loop)
    "default": ("specialised", dict(), 3, 37, False),
    "norm_slaney": ("specialised", dict(mel_scale_norm="slaney"), 3, 37, False),
    "row-family-48k": ("row-family-48k", dict(), 2, 24, False),
    "generic-11025": ("generic-11025", dict(), 2, 25, False),
    "default-loop": ("specialised", dict(), 3, 41, True),
    "row-family-48k-loop": ("row-family-48k", dict(), 2, 41, True),
    "generic-11025-loop": ("generic-11025", dict(), 2, 41, True),
}
_cases = {}


@pytest.fixture(scope="module")
def emu():
    return gcpu.emulator()


@pytest.fixture(scope="module")
def O():
    import riffusion_oracle

    torch.set_num_threads(min(16, torch.get_num_threads()))
    return riffusion_oracle


def _kw(name):
    engine, extra, B, T, loop = CASES[name]
    return dict(ENGINES[engine][1], **extra), ENGINES[engine][2]


def _case(name):
    """per case, once: plan, bank, the inputs on the host and the device, the two entries' results"""
    if name not in _cases:
        from riffusion import _hip

        engine, extra, B, T, loop = CASES[name]
        kw, plan_kw = _kw(name)
        plan = _hip.get_plan(_params(**kw), "cuda:0", **plan_kw)
        assert plan.griffinlim_engine == ENGINES[engine][0] and plan.lstsq_ok
        op, cp, fb = cpu.bank(**kw)
        assert torch.equal(fb, plan.melfb)
        L = plan.output_samples(T, loop)
        mel = _mel(plan.n_mels, B, T)
        guide, g_w = gcpu.inputs(B, L)
        d = dict(plan=plan, op=op, cp=cp, fb=fb, B=B, T=T, L=L, loop=loop, mel=mel, guide=guide, g_w=g_w, mel_d=mel.cuda(), guide_d=guide.cuda(),
                 g_w_d=g_w.cuda())
        d["gS"] = plan.griffinlim_guided_backward(d["guide_d"], d["g_w_d"], T, loop)
        d["gmel"] = plan.waveform_from_mel_guided_backward(d["mel_d"], d["guide_d"], d["g_w_d"], loop)
        torch.cuda.synchronize()
        _cases[name] = d
    return _cases[name]


def _emulated_stage(emu, plan, cp, guide, g_w_d, B, T, L, loop, frame_engine="auto"):  # noqa: F811
    """the stage entry restated: the device's own adjoint and forward transform around the host emulator's staging and projection"""
    staged = gcpu.emu_stage_rows(emu, guide, L)
    _, A, Tn = plan.stft(staged.cuda(), want_mag=False, want_spec=True, loop=loop)
    assert Tn == T
    G = plan.istft_backward(g_w_d, B, T, loop)
    xpos_bin, s2x = gcpu.tables(cp) if frame_engine == "auto" else gcpu.plain_tables(plan.n_stft, plan.frame_stride)
    assert len(s2x) == plan.frame_stride
    return gcpu.emu_project(emu, G.cpu(), A.cpu(), xpos_bin, s2x)


@pytest.mark.parametrize("name", list(CASES))
def test_stage_entry_equals_the_emulator(emu, name):  # noqa: F811
    d = _case(name)
    plan, B, T = d["plan"], d["B"], d["T"]
    assert tuple(d["gS"].shape) == (B * T, plan.frame_stride)
    want = _emulated_stage(emu, plan, d["cp"], d["guide"], d["g_w_d"], B, T, d["L"], d["loop"])
    assert bool(torch.isfinite(d["gS"]).all()) and bool((d["gS"] != 0).any())
    assert _bits(d["gS"]) == _bits(want)


def test_stage_entry_on_the_chirp_z_engine(emu):  # noqa: F811
    """more filters than bins: the closed form does not serve this plan, the stage entry does; its loop form is refused"""
    from riffusion import _hip

    engine, kw, plan_kw = ENGINES["chirp-z-1009"]
    plan = _hip.get_plan(_params(**kw), "cuda:0", **plan_kw)
    assert plan.griffinlim_engine == engine and not plan.lstsq_ok
    B, T = 2, 24
    L = plan.output_samples(T)
    guide, g_w = gcpu.inputs(B, L)
    got = plan.griffinlim_guided_backward(guide.cuda(), g_w.cuda(), T)
    want = _emulated_stage(emu, plan, None, guide, g_w.cuda(), B, T, L, False, frame_engine="chirp-z")
    assert bool((got != 0).any()) and _bits(got) == _bits(want)
    lib, stream = plan.lib, torch.cuda.current_stream().cuda_stream
    assert lib.rfx_griffinlim_guided_backward_loop_workspace_bytes(plan.handle, B, 41) == 0
    assert lib.rfx_waveform_from_mel_guided_backward_workspace_bytes(plan.handle, B, T) == 0
    out = torch.full_like(got, 12345.0)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    gl = torch.zeros((B, plan.hop_length * 41), device="cuda")
    assert lib.rfx_griffinlim_guided_backward_loop(plan.handle, guide.cuda().data_ptr(), L, gl.data_ptr(), B, 41, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   stream) == -4
    assert b"chirp-z" in lib.rfx_last_error()
    mel, gmel = torch.ones((B, plan.n_mels, T), device="cuda"), torch.full((B, plan.n_mels, T), 12345.0, device="cuda")
    assert lib.rfx_waveform_from_mel_guided_backward(plan.handle, mel.data_ptr(), guide.cuda().data_ptr(), L, g_w.cuda().data_ptr(), B, T, gmel.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), stream) == -1
    assert b"closed-form InverseMelScale does not serve this plan" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all()) and bool((gmel == 12345.0).all()) and bool((ws == 0xA5).all())


@pytest.mark.parametrize("name", list(CASES))
def test_fused_entry_equals_its_stages(name):
    d = _case(name)
    plan = d["plan"]
    assert tuple(d["gmel"].shape) == tuple(d["mel"].shape)
    assert bool(torch.isfinite(d["gmel"]).all()) and bool((d["gmel"] != 0).any())
    assert _bits(d["gmel"]) == _bits(plan.inverse_mel_lstsq_backward(d["mel_d"], d["gS"]))


@pytest.mark.parametrize("name", list(CASES))
def test_accuracy_against_float64_autograd(O, name):
    d = _case(name)
    plan, fb, B, T = d["plan"], d["fb"], d["B"], d["T"]
    keep, share = gcpu.relu_guard(fb, d["mel"])
    assert share <= bcpu.GUARD_SHARE
    gS64, gm64 = gcpu.torch_chain(O, d["op"], fb, d["mel"], d["guide"], d["g_w"], d["loop"], torch.float64, keep)
    gS32, gm32 = gcpu.torch_chain(O, d["op"], fb, d["mel"], d["guide"], d["g_w"], d["loop"], torch.float32, keep)
    gS = plan.unpack_magnitudes(d["gS"], B, T).cpu()
    gmel = plan.inverse_mel_lstsq_backward(d["mel_d"], d["gS"] * plan.pack_magnitudes(keep.to(torch.float32).cuda())).cpu()
    for what, got, g32, ref in (("g_S", gS, gS32, gS64), ("g_mel", gmel, gm32, gm64)):
        ours, torch32 = bcpu.distances(got, ref), bcpu.distances(g32, ref)
        print(f"{name} {what}: device rel-L2 {ours[0]:.2e} (worst frame {ours[1]:.2e}); float32 torch chain {torch32[0]:.2e} (worst frame "
              f"{torch32[1]:.2e}); marked share {share:.3%}")
        assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1], what


@pytest.mark.parametrize("name", ["default", "generic-11025", "default-loop"])
def test_exact_consequences(name):
    d = _case(name)
    plan, B, T, L, loop = d["plan"], d["B"], d["T"], d["L"], d["loop"]
    # a silent guide row gives a zero gradient row, the other rows keep their bytes
    silent = d["guide_d"].clone()
    silent[1] = 0
    got = plan.griffinlim_guided_backward(silent, d["g_w_d"], T, loop).reshape(B, T, -1)
    assert bool((got[1] == 0).all()) and _bits(got[0]) == _bits(d["gS"].reshape(B, T, -1)[0])
    gm = plan.waveform_from_mel_guided_backward(d["mel_d"], silent, d["g_w_d"], loop)
    assert bool((gm[1] == 0).all()) and _bits(gm[2 if B > 2 else 0]) == _bits(d["gmel"][2 if B > 2 else 0])
    # a guide shorter than the clip is the same guide padded with zeros by the caller; a longer one is cut
    short = d["guide_d"][:, : L - 1001].contiguous()
    padded = torch.nn.functional.pad(short, (0, 1001))
    a = plan.griffinlim_guided_backward(short, d["g_w_d"], T, loop)
    assert _bits(a) == _bits(plan.griffinlim_guided_backward(padded, d["g_w_d"], T, loop)) and _bits(a) != _bits(d["gS"])
    longer = torch.cat([d["guide_d"], torch.full((B, 77), 1e9, device="cuda")], dim=1)
    assert _bits(plan.griffinlim_guided_backward(longer, d["g_w_d"], T, loop)) == _bits(d["gS"])
    # the guide's units do not matter, the gradient's scale is exact
    for m in (-20, 9):
        assert _bits(plan.griffinlim_guided_backward(d["guide_d"] * 2.0 ** m, d["g_w_d"], T, loop)) == _bits(d["gS"]), m
    for k in (-40, 40):
        assert _bits(plan.griffinlim_guided_backward(d["guide_d"], d["g_w_d"] * 2.0 ** k, T, loop)) == _bits(d["gS"] * 2.0 ** k), k
        assert _bits(plan.waveform_from_mel_guided_backward(d["mel_d"], d["guide_d"], d["g_w_d"] * 2.0 ** k, loop)) == _bits(d["gmel"] * 2.0 ** k), k


@pytest.mark.parametrize("name", ["default", "generic-11025", "default-loop"])
def test_contract(name):
    d = _case(name)
    plan, B, T, L, loop = d["plan"], d["B"], d["T"], d["L"], d["loop"]
    lib, stream = plan.lib, torch.cuda.current_stream().cuda_stream
    sfx = "_loop" if loop else ""
    stage, stage_q = getattr(lib, "rfx_griffinlim_guided_backward" + sfx), getattr(lib, f"rfx_griffinlim_guided_backward{sfx}_workspace_bytes")
    fused, fused_q = getattr(lib, "rfx_waveform_from_mel_guided_backward" + sfx), getattr(lib, f"rfx_waveform_from_mel_guided_backward{sfx}_workspace_bytes")
    guide, g_w, mel = d["guide_d"].clone(), d["g_w_d"].clone(), d["mel_d"].clone()
    ns, nm = B * T * plan.frame_stride, B * plan.n_mels * T
    # the stage entry: canaries behind the workspace and the output, inputs untouched
    need = stage_q(plan.handle, B, T)
    assert need >= 2 * ns * 8
    ws = torch.full((need + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((ns + CANARY // 4,), -7.0, dtype=torch.float32, device="cuda")
    assert stage(plan.handle, guide.data_ptr(), L, g_w.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((out[ns:] == -7.0).all()) and _bits(out[:ns]) == _bits(d["gS"])
    assert _bits(guide) == _bits(d["guide"]) and _bits(g_w) == _bits(d["g_w"])
    # ... and the fused entry
    need_f = fused_q(plan.handle, B, T)
    assert need_f >= ns * 4 + need
    ws_f = torch.full((need_f + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    out_f = torch.full((nm + CANARY // 4,), -7.0, dtype=torch.float32, device="cuda")
    assert fused(plan.handle, mel.data_ptr(), guide.data_ptr(), L, g_w.data_ptr(), B, T, out_f.data_ptr(), ws_f.data_ptr(), need_f, stream) == 0
    torch.cuda.synchronize()
    assert bool((ws_f[need_f:] == 0xA5).all()) and bool((out_f[nm:] == -7.0).all()) and _bits(out_f[:nm]) == _bits(d["gmel"])
    assert _bits(guide) == _bits(d["guide"]) and _bits(g_w) == _bits(d["g_w"]) and _bits(mel) == _bits(d["mel"])
    # refusals, before any launch: a short workspace, misaligned pointers, a null pointer; B == 0 is a no-op
    out.fill_(-7.0)
    out_f.fill_(-7.0)
    assert stage(plan.handle, guide.data_ptr(), L, g_w.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need - 1, stream) == -3
    assert fused(plan.handle, mel.data_ptr(), guide.data_ptr(), L, g_w.data_ptr(), B, T, out_f.data_ptr(), ws_f.data_ptr(), need_f - 1, stream) == -3
    assert stage(plan.handle, guide.data_ptr(), L, g_w.data_ptr(), B, T, out.data_ptr() + 4, ws.data_ptr(), need, stream) == -1
    assert b"16-byte aligned" in lib.rfx_last_error()
    assert stage(plan.handle, guide.data_ptr() + 2, L, g_w.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert fused(plan.handle, mel.data_ptr(), guide.data_ptr(), L, g_w.data_ptr(), B, T, out_f.data_ptr(), ws_f.data_ptr() + 8, need_f, stream) == -1
    assert fused(plan.handle, mel.data_ptr(), guide.data_ptr(), L, g_w.data_ptr() + 1, B, T, out_f.data_ptr(), ws_f.data_ptr(), need_f, stream) == -1
    assert stage(plan.handle, None, L, g_w.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert stage(plan.handle, guide.data_ptr(), 0, g_w.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert stage(plan.handle, guide.data_ptr(), L, g_w.data_ptr(), 0, T, out.data_ptr(), ws.data_ptr(), need, stream) == 0
    # more than 2^31 - 1 frames; a frame count the form does not serve
    assert stage_q(plan.handle, 1 << 26, 64) == 0 and fused_q(plan.handle, 1 << 26, 64) == 0
    assert stage(plan.handle, guide.data_ptr(), L, g_w.data_ptr(), 1 << 26, 64, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert b"2^31" in lib.rfx_last_error()
    few = 3
    assert stage_q(plan.handle, B, few) == 0
    assert stage(plan.handle, guide.data_ptr(), L, g_w.data_ptr(), B, few, out.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert (b"loop call needs" if loop else b"Padding size") in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((out_f == -7.0).all())
    # row 1 alone is row 1 of the batch
    alone = plan.griffinlim_guided_backward(guide[1:2].contiguous(), g_w[1:2].contiguous(), T, loop)
    assert _bits(alone) == _bits(d["gS"][T:2 * T])
    alone = plan.waveform_from_mel_guided_backward(mel[1:2].contiguous(), guide[1:2].contiguous(), g_w[1:2].contiguous(), loop)
    assert _bits(alone) == _bits(d["gmel"][1:2])


def test_a_singular_bank_is_refused_before_any_launch():
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter

    plan = _hip.get_plan(_params(num_frequencies=1024), "cuda:0")
    lib = plan.lib
    B, T, sentinel = 1, 24, 12345.0
    L = plan.output_samples(T)
    assert not plan.lstsq_ok and lib.rfx_waveform_from_mel_guided_backward_workspace_bytes(plan.handle, B, T) == 0
    assert lib.rfx_waveform_from_mel_guided_backward_loop_workspace_bytes(plan.handle, B, 41) == 0
    mel = torch.ones((B, plan.n_mels, T), device="cuda")
    guide, g_w = (t.cuda() for t in gcpu.inputs(B, L))
    out = torch.full((B, plan.n_mels, T), sentinel, device="cuda")
    ws = torch.full((1 << 24,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.rfx_waveform_from_mel_guided_backward(plan.handle, mel.data_ptr(), guide.data_ptr(), L, g_w.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), stream) == -1
    assert b"pivot" in lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((ws == 0xA5).all())
    with pytest.raises(ValueError, match="pivot"):
        plan.waveform_from_mel_guided_backward(mel, guide, g_w)
    conv = SpectrogramConverter(_params(num_frequencies=1024), device="cuda")
    with pytest.raises(ValueError, match="pivot"):
        conv.waveform_from_mel_amplitudes(mel.requires_grad_(True), guide=guide, inverse_mel="lstsq", griffin_lim_iters=0)


# ---- the member --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "generic-11025", "default-loop"])
def test_the_member(name):
    from riffusion.spectrogram_converter import SpectrogramConverter

    d = _case(name)
    plan, B, T, L, loop = d["plan"], d["B"], d["T"], d["L"], d["loop"]
    kw, plan_kw = _kw(name)
    conv = SpectrogramConverter(_params(**kw), device="cuda", **plan_kw)
    mel_d, guide = d["mel_d"], d["guide_d"]
    today = plan.waveform_from_mel(mel_d, B, 0, 0.99, seed=0, lstsq=True, guide=guide, loop=loop)
    call = dict(guide=guide, inverse_mel="lstsq", loop=loop)
    leaf = mel_d.clone().requires_grad_(True)
    out = conv.waveform_from_mel_amplitudes(leaf, griffin_lim_iters=0, **call)
    assert out.grad_fn is not None and tuple(out.shape) == (B, L) and _bits(out) == _bits(today)
    out.backward(d["g_w_d"])
    assert _bits(leaf.grad) == _bits(d["gmel"])
    with pytest.raises(RuntimeError):  # once differentiable
        leaf2 = mel_d.clone().requires_grad_(True)
        o2 = conv.waveform_from_mel_amplitudes(leaf2, griffin_lim_iters=0, **call)
        (g2,) = torch.autograd.grad(o2, leaf2, d["g_w_d"], create_graph=True)
        g2.sum().backward()
    # every other call is the plain one: no grad mode, no grad on the input, the SGD, iterations, a held call
    with torch.no_grad():
        plain = conv.waveform_from_mel_amplitudes(leaf, griffin_lim_iters=0, **call)
    assert plain.grad_fn is None and _bits(plain) == _bits(today)
    plain = conv.waveform_from_mel_amplitudes(mel_d, griffin_lim_iters=0, **call)
    assert plain.grad_fn is None and _bits(plain) == _bits(today)
    two = conv.waveform_from_mel_amplitudes(leaf, griffin_lim_iters=2, **call)
    assert two.grad_fn is None and _bits(two) == _bits(plan.waveform_from_mel(mel_d, B, 2, 0.99, seed=conv._seed(None), lstsq=True, guide=guide, loop=loop))
    sgd = conv.waveform_from_mel_amplitudes(leaf, griffin_lim_iters=0, guide=guide, inverse_mel="sgd", loop=loop, seed=5)
    assert sgd.grad_fn is None and _bits(sgd) == _bits(plan.waveform_from_mel(mel_d, B, 0, 0.99, seed=conv._seed(5), guide=guide, loop=loop))
    if not loop:
        held = conv.waveform_from_mel_amplitudes(leaf, griffin_lim_iters=0, hold_frames=(2, 2), **call)
        assert held.grad_fn is None and _bits(held) == _bits(today)
        assert conv.waveform_from_mel_amplitudes(leaf, inverse_mel="lstsq", griffin_lim_iters=0).grad_fn is None  # no guide
    # the params' count is the default
    assert conv.waveform_from_mel_amplitudes(leaf, **call).grad_fn is None
    # leading dimensions, and a CPU leaf: autograd carries the copy
    cpu_leaf = d["mel"][:2].reshape(2, 1, plan.n_mels, T).clone().requires_grad_(True)
    lead = conv.waveform_from_mel_amplitudes(cpu_leaf, guide=d["guide"][:2].reshape(2, 1, L), inverse_mel="lstsq", loop=loop, griffin_lim_iters=0)
    assert tuple(lead.shape) == (2, 1, L) and _bits(lead) == _bits(today[:2])
    lead.backward(d["g_w_d"][:2].reshape(2, 1, L))
    assert cpu_leaf.grad.device.type == "cpu" and _bits(cpu_leaf.grad.reshape(2, plan.n_mels, T)) == _bits(d["gmel"][:2])
    # the guide is a constant
    with pytest.raises(RuntimeError, match="guide"):
        conv.waveform_from_mel_amplitudes(leaf, guide=guide.clone().requires_grad_(True), inverse_mel="lstsq", loop=loop, griffin_lim_iters=0)
    with pytest.raises(ValueError, match="griffin_lim_iters"):
        conv.waveform_from_mel_amplitudes(leaf, griffin_lim_iters=-1, **call)


def test_end_to_end_from_a_loss_on_audio_to_the_mel_tile(O):
    """mel -> waveform_from_mel_amplitudes(guide, lstsq, 0 iterations) -> spectral_losses(...).convergence.sum().backward(), against the
    same chain composed from the oracles in float64, at most twice the distance of that chain in float32 torch: the end-to-end test of
    tests/test_gpu_imel_lstsq_bwd.py with its three middle calls replaced by the member"""
    from riffusion.spectrogram_converter import SpectrogramConverter

    kw = dict(sample_rate=8000, num_frequencies=64, max_frequency=4000)
    conv = SpectrogramConverter(_params(**kw), device="cuda")
    plan = conv._plan()
    op, cp, fb = cpu.bank(**kw)
    B, T = 2, 24
    L = plan.output_samples(T)
    mel = _mel(plan.n_mels, B, T)
    guide, _ = gcpu.inputs(B, L)
    target = cpu.lstsq_reference(fb, _mel(plan.n_mels, B, T, seed=7), torch.float32).contiguous()

    def oracle(dtype):
        leaf = mel.to(dtype).clone().requires_grad_(True)
        x = torch.relu(torch.linalg.lstsq(fb.T[None].to(dtype), leaf, driver="gels").solution)
        a = IO.stft(O, guide.to(dtype), op, dtype)
        y = IO.istft(O, x * (a / a.abs()), op, dtype)
        m = SLO.stft(y, op, False, dtype).abs()
        loss = SLO.losses_of_magnitudes(m, target.to(dtype), None)[0].sum()
        loss.backward()
        return leaf.grad.detach(), float(loss.detach())

    ref, loss64 = oracle(torch.float64)
    g32, loss32 = oracle(torch.float32)
    leaf = mel.cuda().requires_grad_(True)
    wave = conv.waveform_from_mel_amplitudes(leaf, guide=guide.cuda(), inverse_mel="lstsq", griffin_lim_iters=0)
    loss = conv.spectral_losses(wave, target.cuda()).convergence.sum()
    loss.backward()
    got = leaf.grad.cpu()
    assert bool(torch.isfinite(got).all()) and bool((got != 0).any())
    ours, torch32 = bcpu.distances(got, ref), bcpu.distances(g32, ref)
    print(f"end to end: loss {float(loss.detach()):.6f} (float64 {loss64:.6f}, float32 torch {loss32:.6f}); device gradient rel-L2 {ours[0]:.2e} "
          f"(worst frame {ours[1]:.2e}); float32 torch chain {torch32[0]:.2e} (worst frame {torch32[1]:.2e})")
    assert ours[0] <= 2 * torch32[0] and ours[1] <= 2 * torch32[1]
