"""
The fused spectral losses on the device (include/rfx.h, "FUSED SPECTRAL LOSSES": rfx_spectral_loss, rfx_spectral_loss_backward and their
loop forms; riffusion/_autograd.py: SpectralLossFunction; SpectrogramConverter.spectral_losses).

Shapes: B = 3 rows of T = 41 frames on the four engines of tests/engines.py, plain (Lw = hop * 40 + 17) and loop
(Lw = hop * 41, all four engines); on the specialised engine also the loop minimum T = 40 and one plain batch that crosses the
backward's 256 MiB group boundary (found from the size query; about 52 rows).  Inputs: helpers.synthetic_wave with the last row all
zero; the target is the float64 oracle's magnitudes times a seeded U[0.5, 2) per bin, the silent row's target U[0, 1000);
log_floor = 0.1 x the median oracle magnitude of the non-silent rows (the log gradient weights a bin by 1 / a: the floor is part of
the design of the test, not a tolerance).

Gradient gates, against torch.autograd (tests/spec_loss_oracle.py), every figure printed before it is asserted:
* arithmetic gate, each term alone and both: r64 / r32 are the oracle's gradient FROM THE DEVICE'S OWN SPECTRUM in float64 / float32;
  snr(r64, dev) >= snr(r64, r32) - 6 dB, the project's 6 dB rule.  Both sides decide sign and clamp on the same values.
* end-to-end gate, convergence term: tests/test_gpu_mel_backward.py's, unchanged: dev >= o32 - 6 dB - max(0, fwd_o32 - fwd_dev) against
  end-to-end float64 autograd.  The log term's end-to-end figures are printed, not gated: its small-bin weighting makes them a property
  of the forward transform.
Sums: num and den are Plan.spectral_error's bits; against numpy float64 on the device's own magnitudes num and den are within
n 2^-52 relative and lsum within n 2^-52 + 4 * 2^-52 * sum(|ln a'| + |ln m'|) / lsum - the summation bound plus two logarithms per term at
up to 2 ulp each (the device's and numpy's).  The exact properties compare bits.
"""
import numpy as np
import pytest
import torch

import spec_loss_oracle as SLO
from engines import ENGINES, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave

pytestmark = pytest.mark.gpu

SHAPES = [(name, loop, 41) for name in ENGINES for loop in (False, True)] + [("specialised", True, 40)]
SHAPE_IDS = [f"{name}-{'loop' if loop else 'plain'}-T{t}" for name, loop, t in SHAPES]
G_SC = torch.tensor([0.7, 1.3, 0.9], dtype=torch.float64)
G_LG = torch.tensor([-0.4, 0.9, 1.1], dtype=torch.float64)
TERMS = {"convergence": (G_SC, None), "log": (torch.zeros(3, dtype=torch.float64), G_LG), "both": (G_SC, G_LG)}
_CASES = {}


@pytest.fixture(scope="module")
def O():
    return oracle()


def _case(O, name, loop, frames):
    """the inputs of a shape, the device plan, the device's own spectrum and the forward figures: computed once, never modified"""
    key = (name, loop, frames)
    if key not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        B, Lw = 3, p.hop_length * frames if loop else p.hop_length * (frames - 1) + 17
        wave = synthetic_wave(B, Lw)
        wave[-1] = 0.0
        x64 = SLO.stft(wave, op, loop)
        assert x64.shape == (B, op.n_stft, frames)
        gen = torch.Generator().manual_seed(4321 + Lw)
        target = x64.abs() * (0.5 + 1.5 * torch.rand(x64.shape, generator=gen, dtype=torch.float64))
        target[-1] = torch.rand(target[-1].shape, generator=gen, dtype=torch.float64) * 1000.0
        target = target.to(torch.float32)
        floor = float(np.float32(0.1 * float(x64[:-1].abs().median())))
        mag, spec, tn = plan.stft(wave.cuda(), want_mag=True, want_spec=True, loop=loop)
        assert tn == frames
        x_dev = plan.unpack_complex(spec, B, frames).cpu()
        x32 = SLO.stft(wave, op, loop, torch.float32)
        _CASES[key] = dict(p=p, plan=plan, op=op, B=B, Lw=Lw, T=frames, loop=loop, wave=wave, target=target, floor=floor, x_dev=x_dev,
                           mag_slots=mag, slots=plan.pack_magnitudes(target.cuda()), n=op.n_stft * frames,
                           fwd_dev=snr_db(torch.view_as_real(x64), torch.view_as_real(x_dev)),
                           fwd_o32=snr_db(torch.view_as_real(x64), torch.view_as_real(x32)))
    return _CASES[key]


def _entry_grad(c, g_sc, g_lg, wave=None, slots=None, scale=1.0):
    """the entry-level gradient: sums, the production coefficients, rfx_spectral_loss_backward"""
    from riffusion import _autograd

    plan, f = c["plan"], c["floor"] if g_lg is not None else 0.0
    wave = c["wave"].cuda() if wave is None else wave
    slots = c["slots"] if slots is None else slots
    sums = plan.spectral_loss_sums(wave, slots, f, c["loop"])
    coef = _autograd.loss_coefficients(sums, c["n"], g_sc.cuda()[:wave.shape[0]], (g_lg if g_lg is not None else torch.zeros_like(g_sc)).cuda()[:wave.shape[0]], f)
    return plan.spectral_loss_backward(wave, slots, coef * scale, f, c["loop"]), coef


@pytest.mark.parametrize("name,loop,frames", SHAPES, ids=SHAPE_IDS)
def test_sums_against_spectral_error_and_numpy(O, name, loop, frames):
    c = _case(O, name, loop, frames)
    plan, B, Tn, f = c["plan"], c["B"], c["T"], c["floor"]
    wave = c["wave"].cuda()
    sums = plan.spectral_loss_sums(wave, c["slots"], f, loop)
    assert sums.shape == (B, 3) and sums.dtype == torch.float64 and bool(torch.isfinite(sums).all())
    nolog = plan.spectral_loss_sums(wave, c["slots"], 0.0, loop)
    assert _bits(nolog[:, :2]) == _bits(sums[:, :2]) and not nolog[:, 2].any()
    # num and den are rfx_spectral_error's bits where that entry takes the shape: rows of the samples Griffin-Lim makes of T frames
    L = plan.output_samples(Tn, loop)
    w_err = wave[:, :L].contiguous()
    assert _bits(plan.spectral_loss_sums(w_err, c["slots"], f, loop)[:, :2]) == _bits(plan.spectral_error(w_err, c["slots"], B, Tn, loop=loop))
    # numpy float64 on the device's own magnitudes
    a = plan.unpack_magnitudes(c["mag_slots"], B, Tn).cpu().double().numpy()
    m = c["target"].double().numpy()
    n, eps = c["n"], 2.0 ** -52
    got = sums.cpu().numpy()
    for r in range(B):
        num, den = ((a[r] - m[r]) ** 2).sum(), (m[r] ** 2).sum()
        la, lm = np.log(np.maximum(a[r], f)), np.log(np.maximum(m[r], f))
        lsum = np.abs(la - lm).sum()
        if lsum == 0.0:  # the silent row: its spectrum and its whole target lie below the floor, every term is ln f - ln f
            assert got[r, 2] == 0.0 and r == B - 1
            bound, rel_l = 0.0, 0.0
        else:
            bound, rel_l = n * eps + 4 * eps * (np.abs(la) + np.abs(lm)).sum() / lsum, abs(got[r, 2] - lsum) / lsum
        figs = (abs(got[r, 0] - num) / num, abs(got[r, 1] - den) / den, rel_l)
        print(f"{name} {'loop' if loop else 'plain'} T{Tn} row {r}: relative error of num {figs[0]:.3g}, den {figs[1]:.3g} (bound {n * eps:.3g}), lsum {figs[2]:.3g} (bound {bound:.3g})")
        assert figs[0] <= n * eps and figs[1] <= n * eps and figs[2] <= bound


@pytest.mark.parametrize("name,loop,frames", SHAPES, ids=SHAPE_IDS)
def test_gradient_arithmetic_gate(O, name, loop, frames):
    c = _case(O, name, loop, frames)
    for what, (g_sc, g_lg) in TERMS.items():
        dev = _entry_grad(c, g_sc, g_lg)[0].cpu()
        f = c["floor"] if g_lg is not None else None
        r64 = SLO.from_spectrum(c["wave"], c["x_dev"], c["target"], c["op"], f, g_sc, g_lg, loop, torch.float64)
        r32 = SLO.from_spectrum(c["wave"], c["x_dev"], c["target"], c["op"], f, g_sc, g_lg, loop, torch.float32)
        d, o = snr_db(r64, dev), snr_db(r64, r32)
        print(f"{name} {'loop' if loop else 'plain'} T{frames} {what}, from the device's spectrum: dev {d:.1f} dB, r32 {o:.1f} dB")
        assert tuple(dev.shape) == (c["B"], c["Lw"]) and bool(torch.isfinite(dev).all())
        assert d >= o - 6.0, (what, d, o)


@pytest.mark.parametrize("name,loop,frames", SHAPES, ids=SHAPE_IDS)
def test_gradient_end_to_end_gate(O, name, loop, frames):
    c = _case(O, name, loop, frames)
    slack = max(0.0, c["fwd_o32"] - c["fwd_dev"])
    for what, (g_sc, g_lg) in TERMS.items():
        dev = _entry_grad(c, g_sc, g_lg)[0].cpu()
        f = c["floor"] if g_lg is not None else None
        sc64, lg64, r64 = SLO.end_to_end(c["wave"], c["target"], c["op"], f, g_sc, g_lg, loop, torch.float64)
        _, _, r32 = SLO.end_to_end(c["wave"], c["target"], c["op"], f, g_sc, g_lg, loop, torch.float32)
        d, o = snr_db(r64, dev), snr_db(r64, r32)
        print(f"{name} {'loop' if loop else 'plain'} T{frames} {what}, end to end: dev {d:.1f} dB, o32 {o:.1f} dB, fwd_dev {c['fwd_dev']:.1f} dB, "
              f"fwd_o32 {c['fwd_o32']:.1f} dB")
        if what == "convergence":  # the gate of tests/test_gpu_mel_backward.py; the log term's figures are printed only
            assert d >= o - 6.0 - slack, (what, d, o, slack)
    # the losses themselves, against the float64 oracle.  The float32 transform leaves a bin about 2^-24 log2(n_fft) = 1e-6 of the
    # frame's RMS off; at the floor, a tenth of the median, that is 1e-5 of the bin in ln a, and far less under the mean: 1e-4 leaves
    # an order of magnitude and sits four orders below the losses' dependence on the target (U[0.5, 2) per bin)
    from riffusion.spectrogram_converter import SpectrogramConverter

    sums = c["plan"].spectral_loss_sums(c["wave"].cuda(), c["slots"], c["floor"], loop).cpu()
    sc, lg = SpectrogramConverter.convergence_from_sums(sums[:, 0], sums[:, 1]), sums[:, 2] / c["n"]
    print(f"{name} {'loop' if loop else 'plain'} T{frames} losses: largest relative distance to the float64 oracle, convergence "
          f"{float(((sc - sc64).abs() / sc64).max()):.3g}, log magnitude {float(((lg - lg64).abs() / lg64)[:-1].max()):.3g} (the silent row's is 0 on both sides)")
    assert torch.allclose(sc, sc64, rtol=1e-4, atol=0) and torch.allclose(lg, lg64, rtol=1e-4, atol=0)


@pytest.mark.parametrize("name,loop,frames", SHAPES, ids=SHAPE_IDS)
def test_exact_properties(O, name, loop, frames):
    c = _case(O, name, loop, frames)
    plan, B, f = c["plan"], c["B"], c["floor"]
    wave = c["wave"].cuda()
    got, coef = _entry_grad(c, G_SC, G_LG)
    assert float(got[:-1].abs().max()) > 0
    # zero incoming gradients; the silent row; two calls
    assert not plan.spectral_loss_backward(wave, c["slots"], torch.zeros_like(coef), f, loop).any()
    assert not got[-1].any() and bool(torch.isfinite(got).all())
    assert _bits(_entry_grad(c, G_SC, G_LG)[0]) == _bits(got)
    # a row alone
    for r in range(B):
        alone = plan.spectral_loss_backward(wave[r:r + 1], c["slots"].reshape(B, -1)[r:r + 1].reshape(-1, c["slots"].shape[-1]), coef[r:r + 1], f, loop)
        assert _bits(alone) == _bits(got[r:r + 1]), r
        s1 = plan.spectral_loss_sums(wave[r:r + 1], c["slots"].reshape(B, -1)[r:r + 1].reshape(-1, c["slots"].shape[-1]), f, loop)
        assert _bits(s1) == _bits(plan.spectral_loss_sums(wave, c["slots"], f, loop)[r:r + 1]), r
    # incoming gradients times 2^+-20
    for e in (-20, 20):
        assert _bits(plan.spectral_loss_backward(wave, c["slots"], coef * 2.0 ** e, f, loop) * 2.0 ** -e) == _bits(got), e
    # the target equal to the row's own magnitudes: convergence 0, an exactly zero convergence gradient
    own = plan.spectral_loss_sums(wave, c["mag_slots"], f, loop)
    assert not own[:, 0].any() and not own[:, 2].any()
    g_own, coef_own = _entry_grad(c, G_SC, None, slots=c["mag_slots"])
    assert not coef_own.any() and not g_own.any()
    if loop:  # rolling the waveform and the target's columns by k hops rolls the gradient by k hop samples, bit for bit
        hop = c["p"].hop_length
        for k in (1, 16, frames - 1):
            wk = torch.roll(wave, k * hop, dims=-1).contiguous()
            sk = plan.pack_magnitudes(torch.roll(c["target"], k, dims=-1).contiguous().cuda())
            assert _bits(plan.spectral_loss_backward(wk, sk, coef, f, loop)) == _bits(torch.roll(got, k * hop, dims=-1)), k


def test_rows_on_both_sides_of_the_backward_group_boundary(O):
    """specialised engine, plain, T = 41: a batch two rows past the backward's group of max(1, 256 MiB / row bytes) rows"""
    c = _case(O, "specialised", False, 41)
    plan, lib, Lw, Tn, f = c["plan"], c["plan"].lib, c["Lw"], c["T"], c["floor"]
    query = lib.rfx_spectral_loss_backward_workspace_bytes
    group = next(b for b in range(1, 4096) if query(plan.handle, b, Lw) == query(plan.handle, b + 1, Lw))
    assert 40 <= group <= 64 and query(plan.handle, 4096, Lw) <= (256 << 20) + 768
    B = group + 2
    wave = synthetic_wave(B, Lw, seed=77).cuda()
    mag, _, _ = plan.stft(wave, want_mag=True, want_spec=False)
    gen = torch.Generator().manual_seed(9)
    slots = (mag * (0.5 + 1.5 * torch.rand(mag.shape, generator=gen)).cuda()).contiguous()
    coef = (torch.rand(B, 2, generator=gen) + 0.5).cuda() * torch.tensor([1e-6, 1e-5]).cuda()
    got = plan.spectral_loss_backward(wave, slots, coef, f)
    sums = plan.spectral_loss_sums(wave, slots, f)
    assert bool(torch.isfinite(got).all()) and float(got[-1].abs().max()) > 0
    assert _bits(plan.spectral_loss_backward(wave, slots, coef, f)) == _bits(got)
    rows = slots.reshape(B, -1)
    for r in (0, group - 1, group, B - 1):
        sr = rows[r:r + 1].reshape(Tn, -1)
        assert _bits(plan.spectral_loss_backward(wave[r:r + 1], sr, coef[r:r + 1], f)) == _bits(got[r:r + 1]), r
        assert _bits(plan.spectral_loss_sums(wave[r:r + 1], sr, f)) == _bits(sums[r:r + 1]), r
    pair = slice(group - 1, group + 1)  # the two rows at the seam, as a batch of their own
    assert _bits(plan.spectral_loss_backward(wave[pair], rows[pair].reshape(2 * Tn, -1), coef[pair], f)) == _bits(got[pair])


@pytest.mark.parametrize("name", list(ENGINES))
def test_members(O, name):
    from riffusion.spectrogram_converter import SpectralLosses, SpectrogramConverter

    for loop in (False, True):
        c = _case(O, name, loop, 41)
        plan, f, B, Tn = c["plan"], c["floor"], c["B"], c["T"]
        conv = SpectrogramConverter(c["p"], device="cuda", **ENGINES[name][2])
        w = c["wave"].cuda().requires_grad_(True)
        out = conv.spectral_losses(w, c["target"].cuda(), log_floor=f, loop=loop)
        assert isinstance(out, SpectralLosses) and out.convergence.grad_fn is not None and out.log_magnitude.grad_fn is not None
        assert out.convergence.shape == out.log_magnitude.shape == (B,) and out.convergence.dtype == out.log_magnitude.dtype == torch.float64
        (out.convergence.sum() + out.log_magnitude.sum()).backward()
        ones = torch.ones(B, dtype=torch.float64)
        assert _bits(w.grad) == _bits(_entry_grad(c, ones, ones)[0])
        # without a gradient-requiring waveform, or under no_grad: the forward call alone, the same bytes
        plain = conv.spectral_losses(w.detach(), magnitude_slots=c["slots"], log_floor=f, loop=loop)
        assert plain.convergence.grad_fn is None and _bits(plain.convergence) == _bits(out.convergence) and _bits(plain.log_magnitude) == _bits(out.log_magnitude)
        with torch.no_grad():
            assert conv.spectral_losses(w, magnitude_slots=c["slots"], log_floor=f, loop=loop).convergence.grad_fn is None
        # log_floor=None: no log term, the convergence-only gradient
        w2 = c["wave"].cuda().requires_grad_(True)
        only = conv.spectral_losses(w2, magnitude_slots=c["slots"], loop=loop)
        assert only.log_magnitude is None and _bits(only.convergence) == _bits(out.convergence)
        only.convergence.sum().backward()
        assert _bits(w2.grad) == _bits(_entry_grad(c, ones, None)[0])
        # the existing member's value, bit for bit, where it takes the length
        L = plan.output_samples(Tn, loop)
        w_err = c["wave"][:, :L].contiguous().cuda()
        assert _bits(conv.spectral_losses(w_err, c["target"].cuda(), loop=loop).convergence) == _bits(conv.spectral_convergence(w_err, c["target"].cuda(), loop=loop))
        # the target equal to the waveform's own magnitudes: convergence 0 and a zero gradient
        w3 = c["wave"].cuda().requires_grad_(True)
        own = conv.spectral_losses(w3, magnitude_slots=c["mag_slots"], loop=loop)
        own.convergence.sum().backward()
        assert not own.convergence.any() and not w3.grad.any()
        with pytest.raises(RuntimeError, match="target receives no gradient"):
            conv.spectral_losses(w, c["target"].cuda().requires_grad_(True), loop=loop)
    # the loop ENCODE keeps its refusal
    conv = SpectrogramConverter(c["p"], device="cuda", **ENGINES[name][2])
    with pytest.raises(RuntimeError, match="the loop encode has no backward yet"):
        conv.mel_amplitudes_from_waveform(c["wave"].cuda().requires_grad_(True), loop=True)


def test_refusals_leave_the_outputs_untouched(O):
    from riffusion import _hip

    for loop in (False, True):
        c = _case(O, "specialised", loop, 41)
        plan, lib, B, Lw, f = c["plan"], c["plan"].lib, c["B"], c["Lw"], c["floor"]
        tag = "_loop" if loop else ""
        fwd, bwd = getattr(lib, "rfx_spectral_loss" + tag), getattr(lib, "rfx_spectral_loss_backward" + tag)
        q_fwd, q_bwd = getattr(lib, f"rfx_spectral_loss{tag}_workspace_bytes"), getattr(lib, f"rfx_spectral_loss_backward{tag}_workspace_bytes")
        need_f, need_b = q_fwd(plan.handle, B, Lw), q_bwd(plan.handle, B, Lw)
        assert 0 < need_f < need_b
        bad_len = Lw + 1 if loop else plan.n_fft // 2
        assert q_fwd(plan.handle, B, bad_len) == 0 == q_bwd(plan.handle, B, bad_len) and q_fwd(plan.handle, 0, Lw) == 0
        wave, slots = c["wave"].cuda(), c["slots"]
        coef = torch.ones(B, 2, device="cuda")
        ws = torch.empty(need_b + 64, dtype=torch.uint8, device="cuda")
        sums = torch.full((B, 3), 123.0, dtype=torch.float64, device="cuda")
        out = torch.full((B, Lw), 123.0, device="cuda")
        s = plan._stream()

        def forward(wave_p=wave.data_ptr(), m_p=slots.data_ptr(), lw=Lw, floor=f, sums_p=sums.data_ptr(), ws_p=ws.data_ptr(), ws_n=need_f):
            return fwd(plan.handle, wave_p, m_p, B, lw, floor, sums_p, ws_p, ws_n, s)

        def backward(wave_p=wave.data_ptr(), m_p=slots.data_ptr(), c_p=coef.data_ptr(), lw=Lw, floor=f, out_p=out.data_ptr(), ws_p=ws.data_ptr(), ws_n=need_b):
            return bwd(plan.handle, wave_p, m_p, c_p, B, lw, floor, out_p, ws_p, ws_n, s)

        short = [forward(ws_n=need_f - 1), backward(ws_n=need_b - 1)]
        refused = [forward(wave_p=None), forward(m_p=None), forward(sums_p=None), forward(ws_p=None), forward(m_p=slots.data_ptr() + 4),
                   forward(ws_p=ws.data_ptr() + 4), forward(sums_p=sums.data_ptr() + 4), forward(wave_p=wave.data_ptr() + 2), forward(lw=bad_len),
                   forward(floor=-1.0), forward(floor=float("nan")), forward(floor=float("inf")), forward(floor=1e-19),
                   backward(wave_p=None), backward(m_p=None), backward(c_p=None), backward(out_p=None), backward(ws_p=None),
                   backward(m_p=slots.data_ptr() + 4), backward(ws_p=ws.data_ptr() + 4), backward(out_p=out.data_ptr() + 2), backward(c_p=coef.data_ptr() + 2),
                   backward(lw=bad_len), backward(floor=-1.0), backward(floor=float("nan")), backward(floor=1e-19)]
        torch.cuda.synchronize()
        assert short == [-3, -3] and all(rc == -1 for rc in refused), (short, refused)  # RFX_ERR_WORKSPACE, RFX_ERR_INVALID
        assert (sums == 123.0).all() and (out == 123.0).all()
        if loop:
            assert forward(lw=Lw + 1) == -1 and b"nearest legal lengths" in lib.rfx_last_error()
            assert backward(lw=Lw + 1) == -1 and b"nearest legal lengths" in lib.rfx_last_error() and b"rfx_spectral_loss_backward_loop" in lib.rfx_last_error()
        assert forward() == 0 and backward() == 0
        torch.cuda.synchronize()
        assert not (sums == 123.0).any() and not (out[:-1] == 123.0).all()
        with pytest.raises(ValueError):
            plan.spectral_loss_sums(wave, slots, -1.0, loop)
        with pytest.raises(_hip.RfxError):
            plan.spectral_loss_sums(wave.cpu(), slots, f, loop)
