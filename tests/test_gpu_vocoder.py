"""
The time stretch on the device (include/rfx.h, "TIME STRETCH": rfx_phase_vocoder, rfx_time_stretch; Plan.phase_vocoder / time_stretch;
SpectrogramConverter.time_stretch_spectrogram / time_stretch).

Shapes: B = 3 rows of T = 41 frames (no multiple of 16) and of T = 2 frames on the four engines of tests/engines.py, and
B = 1, T = 512 on the specialised engine.  Inputs, oracle and emulator are those of tests/test_vocoder_cpu.py: X is seeded complex64
noise over the oracle STFT of helpers.synthetic_wave, the last row all zero (B > 1); rates 1.25, 0.75, 1.1, 0.9.

The kernel, through pack_complex -> Plan.phase_vocoder -> unpack_complex.  Every figure is an SNR against the float64 oracle
(tests/vocoder_oracle.py); `dev` the device's, `o32` the float32 oracle's, `emu` the host emulator's; all printed.
    T = 41, T = 2     dev >= o32 - 6 dB        the project's rule (tests/test_gpu_held_frames.py)
    T = 512           dev >= o32               no allowance: the wrapped-turns formulation must beat float32 torch outright
    everywhere        dev >= emu - 6 dB        the device's atan2f / hypotf / sincospif against the host's
    X * 2^+-40        the same gates after unscaling (the magnitudes are hypotf's, the angles scale-free)
Bits: pack_complex(unpack_complex(out)) == out - both slots of a doubled bin agree, conjugate slots are conjugates, padding is zero;
a row alone equals the row in the batch; rate = 1 is a copy; the zero row leaves as zeros.

The wide rates (RATES_WIDE of tests/test_vocoder_cpu.py: bpm ratios with near-integer products, rates >= 2, <= 0.5 and >= T), T = 41 on
the four engines, T = 3 and T = 1 on two; the oracle's step positions are the double products i * rate, the header's definition.  The
same gates and bits; X * 2^+-40 at 3.0 and 0.125 only.  T_out = 1 is gated against the emulator alone (dev >= emu - 6 dB) and its
distance to o32 printed (-2.3 to -2.6 dB): the emulator itself is 4 - 5 dB below an o32 at float32's rounding floor, and the CPU test
carries that gate.  The structured input and the noise-free analysis of tests/test_vocoder_cpu.py with both gates, on the whole and
per slice; there a figure is capped at the float64 oracle's own rounding floor (319.1 dB) before the device is held to it - on the
special bins at rate 3 the device's exact zeros score 319.5 dB, the oracle's own sin(pi), where the emulator repeats the oracle's
error and scores 464.  THE LAUNCH SEAM: 65536 + 7 rows of two frames - the second trip of launch_vocoder's loop over 65535 rows - rows
on both sides of the seam equal the same rows stretched alone.

The member: Plan.time_stretch(w, rate) equals Plan.istft(Plan.phase_vocoder(Plan.stft(w))) bit for bit, for B = 3 and for one row more
than a row group (the group's size read from the workspace query); SpectrogramConverter.time_stretch equals it for a (1, 3, L) input
and under `length=`; rates 1.25, 0.9, 1, 2/3 and 3.  A 440 Hz sine stretched at 2/3 and 3 keeps its spectral peak within one bin of
440 Hz.  Its figure against the float64 chain stft -> oracle vocoder -> istft is printed and NOT gated: the analysis'
rounding of near-silent bins feeds angle(), and the float32 chain differs there as well.

Contract: a workspace one byte short is -3, NULL pointers are -1, canary bytes past both outputs stay, B = 0 is a no-op.
"""
import math

import pytest
import torch

import istft_oracle as IO
import vocoder_oracle as VO
from engines import ENGINES, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave
from vocoder_cases import (RATES, RATES_WIDE, REF_FLOOR_DB, SINE_RATES, STRUCTURED_RATES, WIDE_IDS, WIDE_SHAPES, _vr, emulator, oracle_figures,
                           oracle_pair, run_emu, sine_analysis, spectrogram, structured)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def emu():
    return emulator()


SHAPES = [(name, 3, T) for T in (41, 2) for name in ENGINES] + [("specialised", 1, 512)]
SHAPE_IDS = [f"{name}-B{b}-T{t}" for name, b, t in SHAPES]


def _stretch(plan, X, rate):
    """(B, n_stft, T) on the host -> (slots out, (B, n_stft, T_out) on the host)"""
    B, _, T = X.shape
    out, Tout = plan.phase_vocoder(plan.pack_complex(X.cuda()), B, T, rate)
    assert Tout == VO.frames(T, rate) and tuple(out.shape) == (B * Tout, plan.frame_stride) and out.dtype == torch.complex64
    return out, plan.unpack_complex(out, B, Tout).cpu()


@pytest.mark.parametrize("name,B,T", SHAPES, ids=SHAPE_IDS)
def test_kernel_parity_scale_and_bits(O, emu, name, B, T):
    _, plan = _plan(name)
    _, op, X = spectrogram(O, name, B, T)
    allowance = 0.0 if T == 512 else 6.0
    for rate in RATES:
        r64, o32 = oracle_figures(O, name, B, T, rate)
        e = snr_db(_vr(r64), _vr(run_emu(emu, X, op.hop_length, rate)))
        out, Y = _stretch(plan, X, rate)
        d = snr_db(_vr(r64), _vr(Y))
        print(f"{name} B{B} T{T} rate {rate}: dev {d:.1f} dB, o32 {o32:.1f} dB, emu {e:.1f} dB")
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all()
        assert d >= o32 - allowance, (name, T, rate, d, o32)
        assert d >= e - 6.0, (name, T, rate, d, e)
        # the layout: every slot of the result is its bin's value as rfx_pack_complex would write it, the padding zero
        assert _bits(plan.pack_complex(Y.cuda())) == _bits(out), rate
        if B > 1:
            assert not _vr(Y[-1]).any()
            for r in (0, B - 1):
                assert _bits(_stretch(plan, X[r:r + 1], rate)[1]) == _bits(Y[r:r + 1]), (rate, r)
        for s in (-40, 40):
            Ys = _stretch(plan, X * 2.0 ** s, rate)[1]
            assert torch.isfinite(_vr(Ys)).all()
            ds = snr_db(_vr(r64), _vr(Ys).double() * 2.0 ** -s)
            print(f"    X * 2^{s}: dev {ds:.1f} dB")
            assert ds >= o32 - allowance and ds >= e - 6.0, (name, T, rate, s, ds, o32, e)
    slots = plan.pack_complex(X.cuda())
    copy, Tout = plan.phase_vocoder(slots, B, T, 1.0)
    assert Tout == T and copy.data_ptr() != slots.data_ptr() and _bits(copy) == _bits(slots)


@pytest.mark.parametrize("name,T", WIDE_SHAPES, ids=WIDE_IDS)
def test_kernel_parity_at_the_wide_rates(O, emu, name, T):
    """RATES_WIDE at T = 41 on the four engines, at T = 3 and T = 1 on two.  T_out = 1 is gated against the emulator alone: the emulator
    itself sits 5 dB below a float32 oracle that is at float32's rounding floor (the CPU test carries that gate), which leaves no
    room to ask 6 dB of the device's atan2f / hypotf / sincospif as well; its distance to o32 is printed."""
    _, plan = _plan(name)
    _, op, X = spectrogram(O, name, 3, T)
    for rate in RATES_WIDE:
        r64, o32 = oracle_figures(O, name, 3, T, rate)
        e = snr_db(_vr(r64), _vr(run_emu(emu, X, op.hop_length, rate)))
        out, Y = _stretch(plan, X, rate)
        d = snr_db(_vr(r64), _vr(Y))
        print(f"{name} T{T} rate {rate:.4g}: T_out {Y.shape[-1]}, dev {d:.1f} dB, o32 {o32:.1f} dB ({d - o32:+.1f}), emu {e:.1f} dB")
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all()
        if Y.shape[-1] > 1:
            assert d >= o32 - 6.0, (name, T, rate, d, o32)
        assert d >= e - 6.0, (name, T, rate, d, e)
        assert _bits(plan.pack_complex(Y.cuda())) == _bits(out), rate
        assert not _vr(Y[-1]).any()
        for r in (0, 2):
            assert _bits(_stretch(plan, X[r:r + 1], rate)[1]) == _bits(Y[r:r + 1]), (rate, r)
        if rate in (3.0, 0.125):  # the scaled runs, at one rate above 2 and one below 1/2 only
            for s in (-40, 40):
                Ys = _stretch(plan, X * 2.0 ** s, rate)[1]
                assert torch.isfinite(_vr(Ys)).all()
                ds = snr_db(_vr(r64), _vr(Ys).double() * 2.0 ** -s)
                print(f"    X * 2^{s}: dev {ds:.1f} dB")
                assert (ds >= o32 - 6.0 or Y.shape[-1] == 1) and ds >= e - 6.0, (name, T, rate, s, ds, o32, e)


def test_kernel_parity_on_structured_input(O, emu):
    _, plan = _plan("specialised")
    op, X, slices = structured(O)
    for rate in STRUCTURED_RATES:
        r64, r32 = oracle_pair(X, rate, op.hop_length)
        E = run_emu(emu, X, op.hop_length, rate)
        out, Y = _stretch(plan, X, rate)
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all() and not _vr(Y[-1]).any()
        for what, at in [("whole", (slice(None), slice(None)))] + list(slices.items()):
            d, e, o32 = snr_db(_vr(r64[at]), _vr(Y[at])), snr_db(_vr(r64[at]), _vr(E[at])), snr_db(_vr(r64[at]), _vr(r32[at]))
            print(f"structured rate {rate:.4g}, {what}: dev {d:.1f} dB, o32 {o32:.1f} dB, emu {e:.1f} dB")
            assert d >= o32 - 6.0, (rate, what, d, o32)
            assert d >= min(e, REF_FLOOR_DB) - 6.0, (rate, what, d, e)  # (capped at the float64 oracle's own rounding floor, 319.1 dB)
        i0 = VO.pairs(41, rate)[0]
        both = (i0 >= 10) & (i0 + 1 <= 19)  # a step whose two frames are both zero leaves with magnitude exactly 0
        assert bool(both.any()) and not _vr(Y[0][:, both]).any(), rate
        assert _bits(plan.pack_complex(Y.cuda())) == _bits(out), rate
        for r in (0, 1):
            assert _bits(_stretch(plan, X[r:r + 1], rate)[1]) == _bits(Y[r:r + 1]), (rate, r)


def test_kernel_parity_on_a_noise_free_analysis(O, emu):
    _, plan = _plan("specialised")
    op, X = sine_analysis(O)
    for rate in SINE_RATES:
        r64, r32 = oracle_pair(X, rate, op.hop_length)
        e, o32 = snr_db(_vr(r64), _vr(run_emu(emu, X, op.hop_length, rate))), snr_db(_vr(r64), _vr(r32))
        Y = _stretch(plan, X, rate)[1]
        d = snr_db(_vr(r64), _vr(Y))
        print(f"440 Hz sine rate {rate:.4g}: dev {d:.1f} dB, o32 {o32:.1f} dB, emu {e:.1f} dB")
        assert tuple(Y.shape) == tuple(r64.shape) and torch.isfinite(_vr(Y)).all()
        assert d >= o32 - 6.0 and d >= e - 6.0, (rate, d, o32, e)


def test_rows_past_one_launch():
    """65536 + 7 rows of two frames at rate 0.75: the kernel's second launch starts at row 65535 with its pointers moved on.  The
    engine is the one of the four with the smallest frame whose input plus output stay below 4 GiB; the noise is made in slot layout
    on the device and passed through unpack -> pack once, so that the slots of a frame are consistent."""
    B, T, rate = 65536 + 7, 2, 0.75
    Tout = VO.frames(T, rate)
    assert Tout == 3
    for name in sorted(ENGINES, key=lambda n: _plan(n)[1].frame_stride):
        plan = _plan(name)[1]
        total = B * (T + Tout) * plan.frame_stride * 8
        print(f"{name}: frame_stride {plan.frame_stride}, {B} rows: {B * T * plan.frame_stride * 8 / 2 ** 20:.0f} MiB in, {B * Tout * plan.frame_stride * 8 / 2 ** 20:.0f} MiB out")
        if total <= 4 << 30:
            break
    else:
        raise AssertionError("no engine's frames fit 4 GiB")
    gen = torch.Generator(device="cuda").manual_seed(99)
    slots = torch.view_as_complex(torch.randn((B * T, plan.frame_stride, 2), generator=gen, device="cuda", dtype=torch.float32))
    slots = plan.pack_complex(plan.unpack_complex(slots, B, T))
    out, n = plan.phase_vocoder(slots, B, T, rate)
    assert n == Tout and tuple(out.shape) == (B * Tout, plan.frame_stride)
    for r in (0, 1, 65534, 65535, 65536, B - 1):
        alone, _ = plan.phase_vocoder(slots[r * T:(r + 1) * T], 1, T, rate)
        assert bool(alone.abs().sum() > 0) and torch.equal(torch.view_as_real(alone).view(torch.int32), torch.view_as_real(out[r * Tout:(r + 1) * Tout]).view(torch.int32)), r


def _composition(plan, w, rate):
    B = w.shape[0]
    _, spec, T = plan.stft(w, want_mag=False, want_spec=True)
    out, Tout = plan.phase_vocoder(spec, B, T, rate)
    return plan.istft(out, B, Tout), T, Tout


def _group_rows(plan, Lw, rate):
    """rows of a group of rfx_time_stretch: the workspace stops growing there"""
    q = plan.lib.rfx_time_stretch_workspace_bytes
    sizes = [q(plan.handle, b, Lw, rate) for b in range(1, 258)]
    assert sizes[0] > 0
    return next(b for b in range(1, 257) if sizes[b - 1] == sizes[b])


@pytest.mark.parametrize("name", list(ENGINES))
def test_member_is_the_composition(O, name):
    p, plan = _plan(name)
    op = O.params_from(p)
    Lw = IO.samples(op, 41)
    w = synthetic_wave(3, Lw, seed=11).cuda()
    w[-1] = 0
    for rate in (1.25, 0.9, 1.0, 2 / 3, 3.0):
        want, T, Tout = _composition(plan, w, rate)
        got = plan.time_stretch(w, rate)
        assert T == 41 and tuple(got.shape) == (3, IO.samples(op, Tout)) == tuple(want.shape)
        assert plan.time_stretch_samples(Lw, rate) == got.shape[1] == plan.lib.rfx_time_stretch_samples(plan.handle, Lw, rate)
        assert _bits(got) == _bits(want), rate
        assert not got[-1].any()
    # not gated: the float64 chain stft -> oracle vocoder -> istft
    X64 = IO.stft(O, w.cpu(), op, torch.float64)
    for rate in (1.25, 0.9):
        ref = IO.istft(O, VO.phase_vocoder(X64, rate, op.hop_length, torch.float64), op, torch.float64)
        X32 = IO.stft(O, w.cpu(), op, torch.float32)
        o32 = IO.istft(O, VO.phase_vocoder(X32, rate, op.hop_length, torch.float32), op, torch.float32)
        print(f"{name} member rate {rate}: dev {snr_db(ref[:-1], plan.time_stretch(w, rate).cpu()[:-1]):.1f} dB, float32 chain {snr_db(ref[:-1], o32[:-1]):.1f} dB (not gated)")


@pytest.mark.parametrize("rate", [2 / 3, 3.0], ids=["2/3", "3"])
def test_member_keeps_a_sine_where_it_is(rate):
    """a time stretch moves no frequency: the 440 Hz sine of tests/test_gpu_pitch_shift.py leaves with its spectral peak at 440 Hz"""
    p, plan = _plan("specialised")
    Lw, sr = p.hop_length * 40, p.sample_rate
    t = torch.arange(Lw, dtype=torch.float64) / sr
    w = (8000 * torch.sin(2 * math.pi * 440.0 * t)).float().reshape(1, Lw).cuda()
    y = plan.time_stretch(w, rate).cpu().double()[0]
    L = y.shape[0]
    assert L == plan.time_stretch_samples(Lw, rate)
    spec = torch.fft.rfft(y * torch.hann_window(L, dtype=torch.float64)).abs()
    peak = float(spec.argmax()) * sr / L
    print(f"rate {rate:.4g}: {L} samples, peak at {peak:.1f} Hz (bins of {sr / L:.2f} Hz)")
    assert bool(torch.isfinite(y).all()) and abs(peak - 440.0) <= sr / L


def test_member_over_two_row_groups_and_the_converter(O):
    from riffusion.spectrogram_converter import SpectrogramConverter

    p, plan = _plan("specialised")
    op = O.params_from(p)
    Lw, rate = IO.samples(op, 41), 1.25
    group = _group_rows(plan, Lw, rate)
    assert 1 < group < 256
    w = synthetic_wave(group + 1, Lw, seed=12).cuda()
    want, _, Tout = _composition(plan, w, rate)
    assert _bits(plan.time_stretch(w, rate)) == _bits(want)
    # the converter: leading dimensions kept, `length` cuts or pads with zeros, a host input goes to the device
    conv = SpectrogramConverter(p, device="cuda")
    L = IO.samples(op, Tout)
    y = conv.time_stretch(w[:3].cpu().reshape(1, 3, Lw), rate)
    assert tuple(y.shape) == (1, 3, L) and y.is_cuda and _bits(y[0]) == _bits(want[:3])
    assert _bits(conv.time_stretch(w[:3], rate, length=1000)) == _bits(want[:3, :1000])
    padded = conv.time_stretch(w[:3], rate, length=L + 37)
    assert tuple(padded.shape) == (3, L + 37) and _bits(padded[:, :L]) == _bits(want[:3]) and not padded[:, L:].any()
    assert tuple(conv.time_stretch(w[0], rate).shape) == (L,)
    # ... and the spectrogram member is pack -> kernel -> unpack
    X = spectrogram(O, "specialised", 3, 41)[2]
    S = conv.time_stretch_spectrogram(X.reshape(1, 3, *X.shape[1:]), 0.75)
    assert tuple(S.shape) == (1, 3, plan.n_stft, VO.frames(41, 0.75)) and _bits(S[0].cpu()) == _bits(_stretch(plan, X, 0.75)[1])


def test_command_line_stretches_a_stereo_clip(tmp_path):
    import numpy as np

    from riffusion import cli
    from riffusion.util import audio_util

    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    pcm = (np.random.default_rng(3).standard_normal((20000, 2)) * 3000).astype(np.int16)
    audio_util.PcmSegment(pcm, 44100).export(src, format="wav")
    cli.main(["time-stretch", "--audio", src, "--output", dst, "--bpm-from", "120", "--bpm-to", "100"])
    seg = cli._load_segment(dst)
    frames = 1 + 20000 // 441  # 46; at rate 100 / 120 they become ceil(55.2) = 56
    assert seg.channels == 2 and int(seg.frame_rate) == 44100 and int(seg.frame_count()) == 441 * (56 - 1), frames
    out = np.array(seg.get_array_of_samples()).reshape(-1, 2)
    assert np.abs(out.astype(np.int32)).max() >= 32766 and out[:, 0].any() and out[:, 1].any()  # channels are rows; the PCM tail peak-normalises


def test_contract_workspace_nulls_canaries_and_no_rows(O):
    p, plan = _plan("specialised")
    op = O.params_from(p)
    lib, h = plan.lib, plan.handle
    B, T, rate = 2, 41, 1.25
    Lw, Tout = IO.samples(op, T), VO.frames(T, rate)
    L, fs = IO.samples(op, Tout), plan.frame_stride
    slots = plan.pack_complex(spectrogram(O, "specialised", 3, 41)[2][:B].cuda())
    w = synthetic_wave(B, Lw, seed=13).cuda()
    need = lib.rfx_time_stretch_workspace_bytes(h, B, Lw, rate)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((B * Tout * fs + 16,), 3.0 + 5.0j, dtype=torch.complex64, device="cuda")  # 16 canary values behind the frames
    wave = torch.full((B * L + 16,), 7.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    # refusals come before any launch and leave the outputs untouched
    assert lib.rfx_time_stretch(h, w.data_ptr(), B, Lw, rate, wave.data_ptr(), ws.data_ptr(), need - 1, s) == -3
    for args in ((None, w.data_ptr(), wave.data_ptr(), ws.data_ptr()), (h, None, wave.data_ptr(), ws.data_ptr()), (h, w.data_ptr(), None, ws.data_ptr()),
                 (h, w.data_ptr(), wave.data_ptr(), None)):
        assert lib.rfx_time_stretch(args[0], args[1], B, Lw, rate, args[2], args[3], need, s) == -1
    assert lib.rfx_time_stretch(h, w.data_ptr(), B, Lw, float("nan"), wave.data_ptr(), ws.data_ptr(), need, s) == -1
    assert lib.rfx_time_stretch(h, w.data_ptr(), B, op.n_fft // 2, rate, wave.data_ptr(), ws.data_ptr(), need, s) == -1  # rfx_stft's refusal
    assert lib.rfx_time_stretch(h, w.data_ptr(), B, Lw, 100.0, wave.data_ptr(), ws.data_ptr(), need, s) == -1  # one frame: rfx_istft's refusal
    for args in ((None, slots.data_ptr(), out.data_ptr()), (h, None, out.data_ptr()), (h, slots.data_ptr(), None)):
        assert lib.rfx_phase_vocoder(args[0], args[1], B, T, rate, args[2], s) == -1
    assert lib.rfx_phase_vocoder(h, slots.data_ptr(), B, T, 0.0, out.data_ptr(), s) == -1
    assert lib.rfx_phase_vocoder(h, slots.data_ptr(), B, T, rate, slots.data_ptr(), s) == -1  # not in place
    # B == 0 is a no-op
    assert lib.rfx_phase_vocoder(h, slots.data_ptr(), 0, T, rate, out.data_ptr(), s) == 0
    assert lib.rfx_time_stretch(h, w.data_ptr(), 0, Lw, rate, wave.data_ptr(), ws.data_ptr(), need, s) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0 + 5.0j).all()) and bool((wave == 7.0).all())
    # the calls write their frames and samples and nothing behind them
    assert lib.rfx_phase_vocoder(h, slots.data_ptr(), B, T, rate, out.data_ptr(), s) == 0
    assert lib.rfx_time_stretch(h, w.data_ptr(), B, Lw, rate, wave.data_ptr(), ws.data_ptr(), need, s) == 0
    torch.cuda.synchronize()
    assert bool((out[B * Tout * fs:] == 3.0 + 5.0j).all()) and bool((wave[B * L:] == 7.0).all())
    assert _bits(out[:B * Tout * fs]) == _bits(plan.phase_vocoder(slots, B, T, rate)[0])
    assert _bits(wave[:B * L]) == _bits(plan.time_stretch(w, rate))
