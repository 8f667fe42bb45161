"""
The forward path's backward on the device (include/rfx.h, "BACKWARD of the forward path": rfx_stft_backward,
rfx_mel_scale_backward, rfx_mel_from_waveform_backward; riffusion/_autograd.py).

Shapes are (engine, B, Lw): B = 3 rows of T = 41 frames on the four engines of tests/engines.py; on the specialised
engine also B = 5, T = 120 (two frames per workgroup in the forward launch) and Lw = n_fft // 2 + 1 (both reflect partners reach
every sample).  Inputs are helpers.synthetic_wave with the last row all zero, gradients come from a seeded torch.randn.

Parity is against torch.autograd through the oracle's own forward (tests/mel_backward_oracle.py).  No SNR floor is fixed in advance:
every case measures, in the same run and each against the float64 oracle,
    dev      the device gradient                 o32      the float32 oracle gradient
    fwd_dev  the device's complex STFT           fwd_o32  the float32 oracle's complex STFT, on the same input
and requires dev >= o32 - 6 dB - max(0, fwd_o32 - fwd_dev).  The 6 dB is the rule of tests/test_gpu_held_frames.py and of the loop
tests; the second term lets the backward trail torch by as much as the forward already does on that input - the backward contains
that forward, whose own distance the existing tests pin.  The four figures are printed.  The exact properties compare bits.
"""
import os

import numpy as np
import pytest
import torch

import mel_backward_oracle as MBO
from engines import CLIP2, ENGINES, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    return oracle()


def _lw(name, frames):
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams(**ENGINES[name][1])
    return p.n_fft // 2 + 1 if frames is None else p.hop_length * (frames - 1) + 17


SHAPES = [(name, 3, 41) for name in ENGINES] + [("specialised", 5, 120), ("specialised", 2, None)]
SHAPE_IDS = [f"{name}-B{b}-{'short' if t is None else 'T%d' % t}" for name, b, t in SHAPES]
_CASES = {}


def _case(O, name, B, frames):
    """the inputs of a shape, the device plan and the oracle's figures, computed once"""
    key = (name, B, frames)
    if key not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        Lw = _lw(name, frames)
        wave = synthetic_wave(B, Lw)
        wave[-1] = 0.0
        Tn = 1 + (Lw + 2 * (p.n_fft // 2) - p.n_fft) // p.hop_length
        gen = torch.Generator().manual_seed(1234 + Lw)
        g_mel = torch.randn(B, p.num_frequencies, Tn, generator=gen)
        x64 = MBO.stft(wave, op)
        _, spec, tn = plan.stft(wave.cuda(), want_mag=False, want_spec=True)
        assert tn == Tn == x64.shape[-1]
        fwd_dev = snr_db(torch.view_as_real(x64), torch.view_as_real(plan.unpack_complex(spec, B, Tn).cpu()))
        fwd_o32 = snr_db(torch.view_as_real(x64), torch.view_as_real(MBO.stft(wave, op, torch.float32)))
        _CASES[key] = dict(p=p, plan=plan, op=op, Lw=Lw, T=Tn, wave=wave, g_mel=g_mel, gen=gen, fwd_dev=fwd_dev, fwd_o32=fwd_o32,
                           r64=MBO.mel_from_waveform_grad(wave, g_mel, op), r32=MBO.mel_from_waveform_grad(wave, g_mel, op, torch.float32))
    return _CASES[key]


def _gate(c, what, dev, r64, r32):
    """the assertion of the module docstring, the four figures printed first"""
    d, o = snr_db(r64, dev), snr_db(r64, r32)
    slack = max(0.0, c["fwd_o32"] - c["fwd_dev"])
    print(f"{what}: dev {d:.1f} dB, o32 {o:.1f} dB, fwd_dev {c['fwd_dev']:.1f} dB, fwd_o32 {c['fwd_o32']:.1f} dB")
    assert torch.isfinite(dev).all()
    assert d >= o - 6.0 - slack, (what, d, o, slack)


@pytest.mark.parametrize("name,B,frames", SHAPES, ids=SHAPE_IDS)
def test_fused_entry_against_autograd(O, name, B, frames):
    c = _case(O, name, B, frames)
    plan, wave, g = c["plan"], c["wave"].cuda(), c["g_mel"].cuda()
    got = plan.mel_from_waveform_backward(wave, g)
    assert tuple(got.shape) == (B, c["Lw"])
    _gate(c, f"{name} B{B} Lw{c['Lw']} fused", got.cpu(), c["r64"], c["r32"])
    # bits: the silent row, a zero gradient, two calls, a row alone
    assert not got[-1].any()
    assert not plan.mel_from_waveform_backward(wave, torch.zeros_like(g)).any()
    assert _bits(plan.mel_from_waveform_backward(wave, g)) == _bits(got)
    for r in (0, B - 1):
        assert _bits(plan.mel_from_waveform_backward(wave[r:r + 1], g[r:r + 1])) == _bits(got[r:r + 1]), r
    # scale: 2^-40 and 2^40 times the gradient meet the same relative gate, every value finite
    for e in (-40, 40):
        scaled = plan.mel_from_waveform_backward(wave, g * 2.0 ** e)
        assert torch.isfinite(scaled).all()
        _gate(c, f"{name} B{B} Lw{c['Lw']} fused, g_mel * 2^{e}", (scaled * 2.0 ** -e).cpu(), c["r64"], c["r32"])


@pytest.mark.parametrize("name,B,frames", SHAPES, ids=SHAPE_IDS)
def test_stft_and_mel_scale_entries_against_autograd(O, name, B, frames):
    c = _case(O, name, B, frames)
    plan, op, wave, Tn = c["plan"], c["op"], c["wave"], c["T"]
    gen = torch.Generator().manual_seed(99 + c["Lw"])
    g_spec = torch.complex(torch.randn(B, plan.n_stft, Tn, generator=gen), torch.randn(B, plan.n_stft, Tn, generator=gen))
    got = plan.stft_backward(plan.pack_complex(g_spec.cuda()), B, c["Lw"])
    _gate(c, f"{name} B{B} Lw{c['Lw']} stft", got.cpu(), MBO.stft_grad(wave, g_spec, op), MBO.stft_grad(wave, g_spec, op, torch.float32))
    assert _bits(plan.stft_backward(plan.pack_complex(g_spec.cuda()), B, c["Lw"])) == _bits(got)
    assert _bits(plan.stft_backward(plan.pack_complex(g_spec[1:2].cuda()), 1, c["Lw"])) == _bits(got[1:2])
    assert not plan.stft_backward(plan.pack_complex(torch.zeros_like(g_spec).cuda()), B, c["Lw"]).any()
    lin = torch.rand(B, plan.n_stft, Tn, generator=gen) * 1000.0
    got_l = plan.mel_scale_backward(c["g_mel"].cuda())
    assert tuple(got_l.shape) == (B, plan.n_stft, Tn)
    _gate(c, f"{name} B{B} T{Tn} mel_scale", got_l.cpu(), MBO.mel_scale_grad(lin, c["g_mel"], op), MBO.mel_scale_grad(lin, c["g_mel"], op, torch.float32))
    assert _bits(plan.mel_scale_backward(c["g_mel"][:1].cuda())) == _bits(got_l[:1])


@pytest.mark.parametrize("name", list(ENGINES))
def test_members_through_backward(O, name):
    from riffusion.spectrogram_converter import SpectrogramConverter

    c = _case(O, name, 3, 41)
    p, plan, op, B, Tn = c["p"], c["plan"], c["op"], 3, c["T"]
    conv = SpectrogramConverter(p, device="cuda", **ENGINES[name][2])
    # mel_amplitudes_from_waveform: a device leaf; the forward's bytes are the bytes without autograd
    w = c["wave"].cuda().requires_grad_(True)
    mel = conv.mel_amplitudes_from_waveform(w)
    assert mel.grad_fn is not None and mel.requires_grad
    assert _bits(mel) == _bits(conv.mel_amplitudes_from_waveform(w.detach()))
    with torch.no_grad():
        assert conv.mel_amplitudes_from_waveform(w).grad_fn is None
    mel.backward(c["g_mel"].cuda())
    _gate(c, f"{name} member mel_amplitudes_from_waveform", w.grad.cpu(), c["r64"], c["r32"])
    assert _bits(w.grad) == _bits(plan.mel_from_waveform_backward(w.detach(), c["g_mel"].cuda()))
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        mel.backward(c["g_mel"].cuda())
    # a CPU leaf: autograd carries the copy to the device and the gradient back
    w_cpu = c["wave"].clone().requires_grad_(True)
    conv.mel_amplitudes_from_waveform(w_cpu).backward(c["g_mel"].cuda())
    assert w_cpu.grad.device.type == "cpu" and _bits(w_cpu.grad) == _bits(w.grad)
    # spectrogram_func, with a leading dimension
    gen = torch.Generator().manual_seed(5)
    g_spec = torch.complex(torch.randn(1, B, plan.n_stft, Tn, generator=gen), torch.randn(1, B, plan.n_stft, Tn, generator=gen))
    w2 = c["wave"].cuda()[None].requires_grad_(True)
    spec = conv.spectrogram_func(w2)
    assert tuple(spec.shape) == (1, B, plan.n_stft, Tn) and _bits(spec) == _bits(conv.spectrogram_func(w2.detach()))
    spec.backward(g_spec.cuda())
    _gate(c, f"{name} member spectrogram_func", w2.grad[0].cpu(), MBO.stft_grad(c["wave"], g_spec[0], op), MBO.stft_grad(c["wave"], g_spec[0], op, torch.float32))
    # mel_scaler
    lin = (torch.rand(B, plan.n_stft, Tn, generator=gen) * 1000.0).cuda().requires_grad_(True)
    out = conv.mel_scaler(lin)
    assert _bits(out) == _bits(conv.mel_scaler(lin.detach()))
    out.backward(c["g_mel"].cuda())
    _gate(c, f"{name} member mel_scaler", lin.grad.cpu(), MBO.mel_scale_grad(lin.detach().cpu(), c["g_mel"], op),
          MBO.mel_scale_grad(lin.detach().cpu(), c["g_mel"], op, torch.float32))
    # the chain of the two members and torch.abs is the fused member's gradient, up to rounding
    w3 = c["wave"].cuda().requires_grad_(True)
    conv.mel_scaler(conv.spectrogram_func(w3).abs()).backward(c["g_mel"].cuda())
    _gate(c, f"{name} members chained through torch.abs", w3.grad.cpu(), c["r64"], c["r32"])


def test_product_level_loss_on_golden_clip(O, golden_dir):
    """golden clip 2, stereo, its first 17 657 samples, through mel_amplitudes_from_waveform with the loss 0.5 ||mel - target||^2"""
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    seg = audio_util.PcmSegment.from_wav(os.path.join(golden_dir, CLIP2 + ".wav")).set_channels(2)
    Lw = 441 * 40 + 17
    wave = torch.from_numpy(np.array([ch.get_array_of_samples() for ch in seg.split_to_mono()]).astype(np.float32))[:, :Lw].contiguous()
    p = SpectrogramParams(stereo=True)
    op = O.params_from(p)
    conv = SpectrogramConverter(p, device="cuda")
    plan = conv._plan()
    x64 = MBO.stft(wave, op)
    _, spec, Tn = plan.stft(wave.cuda(), want_mag=False, want_spec=True)
    c = dict(fwd_dev=snr_db(torch.view_as_real(x64), torch.view_as_real(plan.unpack_complex(spec, 2, Tn).cpu())),
             fwd_o32=snr_db(torch.view_as_real(x64), torch.view_as_real(MBO.stft(wave, op, torch.float32))))
    target = 0.5 * O.mel_amplitudes_from_waveform(wave, op)
    w = wave.cuda().requires_grad_(True)
    loss = 0.5 * (conv.mel_amplitudes_from_waveform(w) - target.cuda()).pow(2).sum()
    loss.backward()
    _gate(c, "golden clip 2, stereo, 0.5 ||mel - target||^2", w.grad.cpu(), MBO.loss_grad(wave, target, op), MBO.loss_grad(wave, target, op, torch.float32))


def test_refusals_leave_the_output_untouched(O):
    from riffusion import _hip

    c = _case(O, "specialised", 3, 41)
    plan, lib, B, Lw, Tn = c["plan"], c["plan"].lib, 3, c["Lw"], c["T"]
    wave, g = c["wave"].cuda(), c["g_mel"].cuda()
    gs = plan.pack_complex(torch.zeros(B, plan.n_stft, Tn, dtype=torch.complex64).cuda())
    need_f = lib.rfx_mel_from_waveform_backward_workspace_bytes(plan.handle, B, Lw)
    need_s = lib.rfx_stft_backward_workspace_bytes(plan.handle, B, Lw)
    assert 0 < need_s < need_f and lib.rfx_mel_from_waveform_backward_workspace_bytes(plan.handle, B, plan.n_fft // 2) == 0
    # bounded: a batch past the group size asks for no more than 256 MiB and three alignment gaps
    assert lib.rfx_mel_from_waveform_backward_workspace_bytes(plan.handle, 4096, 512 * 441) <= (256 << 20) + 768
    ws = torch.empty(need_f + 64, dtype=torch.uint8, device="cuda")
    out = torch.full((B, Lw), 123.0, device="cuda")
    s = plan._stream()

    def fused(wave_p=wave.data_ptr(), g_p=g.data_ptr(), lw=Lw, out_p=out.data_ptr(), ws_p=ws.data_ptr(), ws_n=need_f):
        return lib.rfx_mel_from_waveform_backward(plan.handle, wave_p, g_p, B, lw, out_p, ws_p, ws_n, s)

    def stft(g_p=gs.data_ptr(), lw=Lw, out_p=out.data_ptr(), ws_p=ws.data_ptr(), ws_n=need_s):
        return lib.rfx_stft_backward(plan.handle, g_p, B, lw, out_p, ws_p, ws_n, s)

    refused = [fused(lw=plan.n_fft // 2), fused(wave_p=None), fused(g_p=None), fused(ws_p=None), fused(ws_p=ws.data_ptr() + 4), fused(ws_n=need_f - 1),
               fused(out_p=out.data_ptr() + 2), stft(lw=plan.n_fft // 2), stft(g_p=None), stft(g_p=gs.data_ptr() + 8), stft(ws_p=ws.data_ptr() + 4),
               stft(ws_n=need_s - 1), lib.rfx_mel_scale_backward(plan.handle, None, B, Tn, out.data_ptr(), None, 0, s),
               lib.rfx_mel_scale_backward(plan.handle, g.data_ptr(), B, 0, out.data_ptr(), None, 0, s)]
    torch.cuda.synchronize()
    assert all(rc in (-1, -3) for rc in refused), refused
    assert refused[5] == refused[11] == -3  # RFX_ERR_WORKSPACE
    assert (out == 123.0).all()
    assert fused() == 0 and not (out == 123.0).all()
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        plan.mel_from_waveform_backward(wave[:, :plan.n_fft // 2], g)
    with pytest.raises(_hip.RfxError):
        plan.mel_from_waveform_backward(wave.cpu(), g)


def test_loop_encode_with_a_gradient_raises(O):
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter(SpectrogramParams(), device="cuda")
    w = synthetic_wave(1, 441 * 41).cuda()
    assert conv.mel_amplitudes_from_waveform(w, loop=True).shape[-1] == 41  # as before without a gradient
    with pytest.raises(RuntimeError, match="the loop encode has no backward yet"):
        conv.mel_amplitudes_from_waveform(w.requires_grad_(True), loop=True)
