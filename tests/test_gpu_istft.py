"""
The inverse spectrogram on the device (include/rfx.h, "INVERSE SPECTROGRAM": rfx_istft, rfx_istft_loop, rfx_istft_backward,
rfx_istft_backward_loop; Plan.istft / istft_backward; SpectrogramConverter.waveform_from_spectrogram).

Shapes: B = 3 rows of T = 41 frames on the four engines of tests/engines.py (the chirp-z one gives the odd n_fft = 1009;
41 is the smallest T a loop takes on every engine and no multiple of 16); on the specialised engine also B = 5, T = 120, and loop at
T = 40.  The last row is all zero.  X is the float64 oracle STFT of helpers.synthetic_wave rounded to complex64, with a seeded
complex perturbation of the same size added (no consistent spectrogram: an edited one); g is a seeded randn.

Parity by the project's rule, nothing fixed in advance: every case measures, each against the float64 oracle (tests/istft_oracle.py),
    dev   the device result          o32   the float32 oracle's result (torch.istft / its autograd; loop: the circular synthesis)
and requires dev >= o32 - 6 dB (tests/test_gpu_held_frames.py).  The backward adds the slack of tests/test_gpu_mel_backward.py:
max(0, fwd_o32 - fwd_dev), the two figures of the forward STFT on g over the envelope - the backward contains that forward.  Figures
are printed.  The exact properties compare bits.

The plain backward runs the zero-extension twin of the engine's forward frame kernel; rfx_debug_istft_backward_padded runs the loop
twin on u padded with zeros to the period P' = hop ceil((L + n_fft) / hop).  The two must agree bit for bit, on all four engines (the
chirp-z engine has a loop FORWARD transform, so nothing is skipped).
"""
import pytest
import torch

import istft_oracle as IO
from engines import ENGINES, LOOPING, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave

pytestmark = pytest.mark.gpu

FORMS = [(name, 3, 41, False) for name in ENGINES] + [(name, 3, 41, True) for name in LOOPING] + [("specialised", 5, 120, False), ("specialised", 3, 40, True)]
FORM_IDS = [f"{name}-B{b}-T{t}{'-loop' if loop else ''}" for name, b, t, loop in FORMS]
_CASES = {}


@pytest.fixture(scope="module")
def O():
    return oracle()


def _vr(x):
    return torch.view_as_real(x.resolve_conj())


def _case(O, name, B, T, loop):
    """inputs, plan and oracle figures of a form, computed once and left unchanged"""
    key = (name, B, T, loop)
    if key not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        L = IO.samples(op, T, loop)
        gen = torch.Generator().manual_seed(77 + T + B)
        wave = synthetic_wave(B, L, seed=303)
        X = IO.stft(O, wave, op, torch.float64, loop)
        assert X.shape[-1] == T
        rms = float(X.abs().pow(2).mean().sqrt())
        X = X + 0.7071 * rms * torch.complex(torch.randn(X.shape, generator=gen, dtype=torch.float64), torch.randn(X.shape, generator=gen, dtype=torch.float64))
        X = X.to(torch.complex64)
        X[-1] = 0
        g = torch.randn(B, L, generator=gen)
        g[-1] = 0
        y64, y32 = IO.istft(O, X, op, torch.float64, loop), IO.istft(O, X, op, torch.float32, loop)
        G64, G32 = IO.istft_grad(O, X, g, op, torch.float64, loop), IO.istft_grad(O, X, g, op, torch.float32, loop)
        # the forward STFT the backward contains: of g over the envelope (u), zero-extended - its device figure against torch's
        _CASES[key] = dict(p=p, plan=plan, op=op, L=L, X=X, g=g, y64=y64, y32=y32, G64=G64, G32=G32)
    return _CASES[key]


def _fwd_slack(O, c, loop):
    """max(0, fwd_o32 - fwd_dev) of the forward STFT on the case's gradient rows (reflect or circular: the device's own entry)"""
    if "slack" not in c:
        plan, op, g = c["plan"], c["op"], c["g"]
        ref = IO.stft(O, g, op, torch.float64, loop)
        _, spec, Tn = plan.stft(g.cuda(), want_mag=False, want_spec=True, loop=loop)
        fwd_dev = snr_db(_vr(ref), _vr(plan.unpack_complex(spec, g.shape[0], Tn).cpu()))
        fwd_o32 = snr_db(_vr(ref), _vr(IO.stft(O, g, op, torch.float32, loop)))
        c["slack"], c["fwd"] = max(0.0, fwd_o32 - fwd_dev), (fwd_dev, fwd_o32)
    return c["slack"]


def _gate(what, dev, r64, r32, slack=0.0):
    d, o = snr_db(r64, dev), snr_db(r64, r32)
    print(f"{what}: dev {d:.1f} dB, o32 {o:.1f} dB, slack {slack:.1f} dB")
    assert torch.isfinite(dev).all()
    assert d >= o - 6.0 - slack, (what, d, o, slack)


def _istft(c, X, loop):
    plan = c["plan"]
    B, _, T = X.shape
    return plan.istft(plan.pack_complex(X.cuda()), B, T, loop)


def _grad(c, g, T, loop):
    plan = c["plan"]
    return plan.unpack_complex(plan.istft_backward(g.cuda(), g.shape[0], T, loop), g.shape[0], T)


@pytest.mark.parametrize("name,B,T,loop", FORMS, ids=FORM_IDS)
def test_forward_parity_scale_and_bits(O, name, B, T, loop):
    c = _case(O, name, B, T, loop)
    X = c["X"]
    y = _istft(c, X, loop)
    assert tuple(y.shape) == (B, c["L"]) and y.dtype == torch.float32
    _gate(f"{name} B{B} T{T} loop={loop} forward", y.cpu(), c["y64"], c["y32"])
    # scale: the map is linear, no range table
    for e in (-40, 40):
        ys = _istft(c, X * 2.0 ** e, loop)
        assert torch.isfinite(ys).all()
        _gate(f"{name} B{B} T{T} loop={loop} forward, X * 2^{e}", (ys.double() * 2.0 ** -e).cpu(), c["y64"], c["y32"])
    # bits: two calls, a row alone, the silent row
    assert _bits(_istft(c, X, loop)) == _bits(y)
    for r in (0, B - 1):
        assert _bits(_istft(c, X[r:r + 1], loop)) == _bits(y[r:r + 1]), r
    assert not y[-1].any()


@pytest.mark.parametrize("name,B,T,loop", FORMS, ids=FORM_IDS)
def test_backward_parity_scale_and_bits(O, name, B, T, loop):
    c = _case(O, name, B, T, loop)
    g = c["g"]
    slack = _fwd_slack(O, c, loop)
    print(f"forward STFT on g: dev {c['fwd'][0]:.1f} dB, o32 {c['fwd'][1]:.1f} dB")
    G = _grad(c, g, T, loop)
    assert tuple(G.shape) == (B, c["plan"].n_stft, T) and G.dtype == torch.complex64
    _gate(f"{name} B{B} T{T} loop={loop} backward", _vr(G.cpu()), _vr(c["G64"]), _vr(c["G32"]), slack)
    for e in (-40, 40):
        Gs = _grad(c, g * 2.0 ** e, T, loop)
        assert torch.isfinite(_vr(Gs)).all()
        _gate(f"{name} B{B} T{T} loop={loop} backward, g * 2^{e}", _vr(Gs.cpu()).double() * 2.0 ** -e, _vr(c["G64"]), _vr(c["G32"]), slack)
    # the zero-imaginary rule, as bits
    assert not G.imag[:, 0].any()
    if c["op"].n_fft % 2 == 0:
        assert not G.imag[:, -1].any()
    assert G.imag[0, 1].any()
    # bits: two calls, a row alone, the silent row, the slots' padding
    assert _bits(_grad(c, g, T, loop)) == _bits(G)
    for r in (0, B - 1):
        assert _bits(_grad(c, g[r:r + 1], T, loop)) == _bits(G[r:r + 1]), r
    assert not _vr(G[-1]).any()
    plan = c["plan"]
    slots = plan.istft_backward(g.cuda(), B, T, loop)
    # pack_complex's layout: the padding is zero, conjugate slots are conjugated and both slots of a doubled bin are filled - each
    # with the value the transform formed for it, so the two agree to rounding, not to the bit
    ref = plan.pack_complex(plan.unpack_complex(slots, B, T))
    assert torch.equal(ref == 0, slots == 0)
    assert float((ref - slots).abs().max()) <= 1e-5 * float(slots.abs().max())


PLAIN = [(name, b, t) for name, b, t, loop in FORMS if not loop]


@pytest.mark.parametrize("name,B,T", PLAIN, ids=[f"{name}-B{b}-T{t}" for name, b, t in PLAIN])
def test_zero_extension_twin_equals_the_padded_loop(O, name, B, T):
    """frame t < T of the zero-extension twin on u equals frame t of the loop twin on u padded with zeros to P': the two backward
    routes write the same gradient slots, bit for bit - also for a gradient with large values at both ends of the row, where a
    reflected or wrapped read would show"""
    c = _case(O, name, B, T, False)
    plan, g = c["plan"], c["g"].cuda()
    edge = g.clone()
    edge[:, :7] = 1e6
    edge[:, -7:] = -1e6
    for what, grad in (("case", g), ("edges", edge)):
        twin = plan.istft_backward(grad, B, T)
        padded = plan.istft_backward(grad, B, T, padded=True)
        assert twin.abs().max() > 0 and _bits(twin) == _bits(padded), what
    lib = plan.lib
    assert lib.rfx_debug_istft_backward_padded_workspace_bytes(plan.handle, B, T) > lib.rfx_istft_backward_workspace_bytes(plan.handle, B, T) > 0


@pytest.mark.parametrize("name,B,T,loop", FORMS, ids=FORM_IDS)
def test_adjoint_identity(O, name, B, T, loop):
    """<istft(X), g> and Re <X, G> in float64: the relative difference of the device pair is at most four times the float32 oracle
    pair's of this run - both are sums of float32 roundings of the same size, the factor covers the different summation order"""
    c = _case(O, name, B, T, loop)
    y, G = _istft(c, c["X"], loop).cpu(), _grad(c, c["g"], T, loop).cpu()
    dev, lhs, rhs = IO.adjoint_defect(y, c["g"], c["X"], G)
    o32, lhs32, rhs32 = IO.adjoint_defect(c["y32"], c["g"], c["X"], c["G32"])
    print(f"{name} B{B} T{T} loop={loop}: device <y,g> {lhs:.9e} Re<X,G> {rhs:.9e} rel {dev:.2e}; float32 oracle {lhs32:.9e} {rhs32:.9e} rel {o32:.2e}")
    assert dev <= 4.0 * o32, (dev, o32)


@pytest.mark.parametrize("name,T", [(n, 41) for n in LOOPING] + [("specialised", 40)], ids=[f"{n}-T41" for n in LOOPING] + ["specialised-T40"])
def test_loop_rolls_are_exact(O, name, T):
    c = _case(O, name, 3, T, True)
    hop = c["op"].hop_length
    y, G = _istft(c, c["X"], True), _grad(c, c["g"], T, True)
    for k in (1, 16, T - 1):
        assert _bits(_istft(c, torch.roll(c["X"], k, dims=-1), True)) == _bits(torch.roll(y, k * hop, dims=-1)), k
        assert _bits(_grad(c, torch.roll(c["g"], k * hop, dims=-1), T, True)) == _bits(torch.roll(G, k, dims=-1)), k


@pytest.mark.parametrize("name", list(ENGINES))
def test_round_trip_through_the_members(O, name):
    """waveform_from_spectrogram(spectrogram_func(w)) against w of hop (T - 1) samples; the gate is float32 torch's own round trip - 6 dB"""
    from riffusion.spectrogram_converter import SpectrogramConverter

    c = _case(O, name, 3, 41, False)
    p, op = c["p"], c["op"]
    conv = SpectrogramConverter(p, device="cuda", **ENGINES[name][2])
    w = synthetic_wave(3, IO.samples(op, 41), seed=404)  # hop (T - 1), one sample more for the odd n_fft
    back = conv.waveform_from_spectrogram(conv.spectrogram_func(w.cuda())).cpu()
    t32 = IO.istft(O, IO.stft(O, w, op, torch.float32), op, torch.float32)
    assert back.shape == w.shape == t32.shape
    d, o = snr_db(w, back), snr_db(w, t32)
    print(f"{name} round trip: dev {d:.1f} dB, float32 torch {o:.1f} dB")
    assert d >= o - 6.0


@pytest.mark.parametrize("name", list(ENGINES))
def test_autograd_end_to_end(O, name):
    from riffusion.spectrogram_converter import SpectrogramConverter

    c = _case(O, name, 3, 41, False)
    p, plan, op, X, L = c["p"], c["plan"], c["op"], c["X"], c["L"]
    conv = SpectrogramConverter(p, device="cuda", **ENGINES[name][2])
    for length in (None, L - 37, L + 53):
        Lw = L if length is None else length
        target = IO.stft(O, synthetic_wave(3, Lw, seed=505), op, torch.float32).abs()
        leaf = X.cuda().requires_grad_(True)
        y = conv.waveform_from_spectrogram(leaf, length=length)
        assert y.grad_fn is not None and tuple(y.shape) == (3, Lw)
        conv.spectral_losses(y, target).convergence.sum().backward()
        r64 = IO.loss_through_istft_grad(O, X, target, op, torch.float64, length)
        r32 = IO.loss_through_istft_grad(O, X, target, op, torch.float32, length)
        _gate(f"{name} X -> waveform(length={length}) -> spectral_losses", _vr(leaf.grad.cpu()), _vr(r64), _vr(r32), _fwd_slack(O, c, False))
        # the log-magnitude term through the same backward: its end-to-end figures are printed, not gated - its 1 / a weighting makes
        # them a property of the forward transform (tests/test_gpu_spectral_loss.py); finite, and the silent row's gradient zero
        floor = float(0.1 * target[:-1].median())
        leaf_lg = X.cuda().requires_grad_(True)
        conv.spectral_losses(conv.waveform_from_spectrogram(leaf_lg, length=length), target, log_floor=floor).log_magnitude.sum().backward()
        l64 = IO.loss_through_istft_grad(O, X, target, op, torch.float64, length, floor)
        l32 = IO.loss_through_istft_grad(O, X, target, op, torch.float32, length, floor)
        print(f"{name} X -> waveform(length={length}) -> log magnitude (not gated): dev {snr_db(_vr(l64), _vr(leaf_lg.grad.cpu())):.1f} dB, "
              f"o32 {snr_db(_vr(l64), _vr(l32)):.1f} dB")
        assert torch.isfinite(_vr(leaf_lg.grad)).all() and leaf_lg.grad.abs().max() > 0 and not _vr(leaf_lg.grad[-1]).any()
    # the forward's bytes are the bytes without autograd; no_grad records nothing; a double backward raises
    leaf = X.cuda().requires_grad_(True)
    y = conv.waveform_from_spectrogram(leaf)
    assert _bits(y) == _bits(conv.waveform_from_spectrogram(X.cuda())) == _bits(_istft(c, X, False))
    with torch.no_grad():
        assert conv.waveform_from_spectrogram(leaf).grad_fn is None
    y.backward(c["g"].cuda())
    assert _bits(leaf.grad) == _bits(_grad(c, c["g"], 41, False))
    # a double backward raises: the backward is once_differentiable
    leaf2 = X.cuda().requires_grad_(True)
    y2 = conv.waveform_from_spectrogram(leaf2)
    (gx,) = torch.autograd.grad(y2, leaf2, torch.ones_like(y2, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.abs().sum().backward()
    # a CPU leaf with a leading dimension: autograd carries the copies
    cpu_leaf = X[None].clone().requires_grad_(True)
    out = conv.waveform_from_spectrogram(cpu_leaf)
    assert tuple(out.shape) == (1, 3, L)
    out.backward(c["g"].cuda()[None])
    assert cpu_leaf.grad.device.type == "cpu" and _bits(cpu_leaf.grad[0]) == _bits(leaf.grad)
    # the loop member is the loop entry
    if name in LOOPING:
        cl = _case(O, name, 3, 41, True)
        assert _bits(conv.waveform_from_spectrogram(cl["X"], loop=True)) == _bits(_istft(cl, cl["X"], True))


def test_contract(O):
    from riffusion import _hip

    c = _case(O, "specialised", 3, 41, False)
    plan, lib, B, T, L = c["plan"], c["plan"].lib, 3, 41, c["L"]
    s = plan._stream()
    X = plan.pack_complex(c["X"].cuda())
    g = c["g"].cuda()
    q = {n: getattr(lib, n + "_workspace_bytes") for n in ("rfx_istft", "rfx_istft_loop", "rfx_istft_backward", "rfx_istft_backward_loop")}
    need = {n: f(plan.handle, B, T) for n, f in q.items()}
    assert all(v > 0 for v in need.values()), need
    # 0 where refused: no frames, a plain T without a sample, a loop T below the minimum
    assert q["rfx_istft"](plan.handle, B, 1) == 0 == q["rfx_istft_backward"](plan.handle, B, 0)
    assert q["rfx_istft_loop"](plan.handle, B, 39) == 0 == q["rfx_istft_backward_loop"](plan.handle, B, 39)
    # bounded: a batch past the group size asks for about one group
    assert q["rfx_istft"](plan.handle, 4096, 512) <= (256 << 20) + (1 << 20) and q["rfx_istft_backward"](plan.handle, 4096, 512) <= (256 << 20) + (1 << 20)
    ws = torch.empty(max(need.values()) + 64, dtype=torch.uint8, device="cuda")
    wave = torch.full((B, 441 * 41), 123.0, device="cuda")
    slots = torch.full((B * T, plan.frame_stride), 123.0, dtype=torch.complex64, device="cuda")

    def fwd(entry="rfx_istft", x_p=X.data_ptr(), t=T, out_p=wave.data_ptr(), ws_p=ws.data_ptr(), ws_n=None, b=B):
        return getattr(lib, entry)(plan.handle, x_p, b, t, out_p, ws_p, need[entry] if ws_n is None else ws_n, s)

    def bwd(entry="rfx_istft_backward", g_p=g.data_ptr(), t=T, out_p=slots.data_ptr(), ws_p=ws.data_ptr(), ws_n=None, b=B):
        return getattr(lib, entry)(plan.handle, g_p, b, t, out_p, ws_p, need[entry] if ws_n is None else ws_n, s)

    refused = [fwd(x_p=None), fwd(out_p=None), fwd(ws_p=None), fwd(x_p=X.data_ptr() + 8), fwd(ws_p=ws.data_ptr() + 4), fwd(out_p=wave.data_ptr() + 2),
               fwd(t=1), fwd(t=0), fwd(b=-1), bwd(g_p=None), bwd(out_p=None), bwd(ws_p=None), bwd(out_p=slots.data_ptr() + 8), bwd(ws_p=ws.data_ptr() + 4),
               bwd(g_p=g.data_ptr() + 2), bwd(t=1)]
    assert all(rc == -1 for rc in refused), refused
    assert fwd(ws_n=need["rfx_istft"] - 1) == -3 and bwd(ws_n=need["rfx_istft_backward"] - 1) == -3
    assert fwd("rfx_istft_loop", ws_n=need["rfx_istft_loop"] - 1) == -3 and bwd("rfx_istft_backward_loop", ws_n=need["rfx_istft_backward_loop"] - 1) == -3
    for entry, call in (("rfx_istft_loop", fwd), ("rfx_istft_backward_loop", bwd)):
        assert call(entry, t=39) == -1 and b"at least 40 frames" in lib.rfx_last_error(), lib.rfx_last_error()
    assert fwd(b=0) == 0 == bwd(b=0)  # a no-op
    torch.cuda.synchronize()
    assert (wave == 123.0).all() and (slots == 123.0).all()
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not (wave[:, :L] == 123.0).all() and (wave.flatten()[B * L:] == 123.0).all() and not (slots == 123.0).any()
    # the chirp-z engine has no loop synthesis: -4 from both loop entries, 0 from their queries, nothing written
    pz, planz = _plan("chirp-z-1009")
    assert lib.rfx_istft_loop_workspace_bytes(planz.handle, B, T) == 0 == lib.rfx_istft_backward_loop_workspace_bytes(planz.handle, B, T)
    assert lib.rfx_istft_loop(planz.handle, X.data_ptr(), B, T, wave.data_ptr(), ws.data_ptr(), ws.numel(), s) == -4
    assert lib.rfx_istft_backward_loop(planz.handle, g.data_ptr(), B, T, slots.data_ptr(), ws.data_ptr(), ws.numel(), s) == -4
    # the Python layer refuses before any device work
    with pytest.raises(ValueError, match="at least 40"):
        plan.istft(X, B, 39, loop=True)
    with pytest.raises(ValueError, match="frames of"):
        plan.istft(X, B, T + 1)
    with pytest.raises(ValueError, match="gradient"):
        plan.istft_backward(g[:, :-1], B, T)
    with pytest.raises(_hip.RfxError):
        plan.istft(X.cpu(), B, T)
