"""
The pitch shift on the device (include/rfx.h "PITCH SHIFT"; csrc/rfx_api_resample.hip) on the four frame engines of
tests/engines.py, rows of 41 frames, B = 3 with the last row all zero.

Composition, bit for bit, at n_steps +2, -5 and 0: Plan.pitch_shift(w, n) equals
    time_stretch(w, 2^(-n / 12)) -> cut or zero-pad to round(Lw / rate) -> resample_sinc(int(sample_rate / rate) -> sample_rate)
    -> cut or zero-pad to Lw
made of the separate members on all rows at once (n = 0: the input's bits); the same for one row more than a row group, the group's
size read from the workspace query; SpectrogramConverter.pitch_shift equals it for a (1, 3, L) host input.  The output has the
input's shape.
The routes beside those: shifts too small to move the frequency (n_steps = +1e-9: int(sample_rate / rate) == sample_rate, the fused
entry copies the stretched rows with other row pitches and reads no table - NULL tables accepted, canaries stay; n_steps = -1e-9:
44099 -> 44100, 44100 phases, composition in bits and the chain gate), at 40 hops and at 41 hops less a sample; the octaves +-12 on
the four engines (the vocoder at exactly 0.5 and 2.0, the resampler at 2/1 and 1/2: bits and the chain gate); +-24 (4/1, 1/4) and
0.5 on the specialised engine in bits.
Direction: a 440 Hz sine shifted by +12 on the specialised engine has its spectral peak within one bin of 880 Hz.
PARITY against the float64 chain oracle STFT -> tests/vocoder_oracle.py -> torch.istft -> tests/resample_oracle.py, printed for the
whole rows and gated on the samples outside the stated departure (where round(Lw / rate) exceeds the stretched row, torch.istft keeps
its untrimmed tail and the library pads zeros; include/rfx.h gives the outputs that can reach: j >= floor((Ls - 6 o / base) n / o)):
    dev >= f32 - 6 dB   the same chain in float32 (the resampler as the all-float32 sparse form), the project's rule
The two chains cut or pad the float64 / float32 torch.istft result exactly as the library does, so the departure is in neither.
An input that requires grad raises; the command line shifts a short generated stereo wav.
Contract: a workspace one byte short is -3, NULL pointers and an overlap are -1, canary values past the output stay, B = 0 is a no-op.
"""
import math

import numpy as np
import pytest
import torch

import istft_oracle as IO
import resample_oracle as RO
import vocoder_oracle as VO
from engines import ENGINES, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave

pytestmark = pytest.mark.gpu

STEPS = [2, -5, 0]


@pytest.fixture(scope="module")
def O():
    return oracle()


def _fix(y, length):
    L = y.shape[-1]
    return y[..., :length] if length <= L else torch.nn.functional.pad(y, (0, length - L))


def _terms(sr, Lw, n_steps):
    """(rate, len_stretch, orig) as torchaudio.functional.pitch_shift forms them"""
    rate = 2.0 ** (-float(n_steps) / 12)
    return rate, int(round(Lw / rate)), int(sr / rate)


def _composition(plan, w, n_steps):
    from riffusion import _hip

    if n_steps == 0:
        return w.clone()
    rate, len_stretch, orig = _terms(plan.sample_rate, w.shape[1], n_steps)
    assert orig == plan.lib.rfx_pitch_shift_resample_freq(plan.handle, w.shape[1], float(n_steps), 12)
    stretched = _fix(plan.time_stretch(w, rate), len_stretch).contiguous()
    if orig == plan.sample_rate:  # a shift too small to move int(sample_rate / rate): torchaudio's resample returns its input
        return _fix(stretched, w.shape[1]).contiguous()
    return _fix(_hip.resample_sinc(stretched, orig, plan.sample_rate), w.shape[1]).contiguous()


def _group_rows(plan, Lw, n_steps):
    """rows of a group of rfx_pitch_shift: the workspace stops growing there"""
    q = plan.lib.rfx_pitch_shift_workspace_bytes
    sizes = [q(plan.handle, b, Lw, float(n_steps), 12) for b in range(1, 258)]
    assert sizes[0] > 0
    return next(b for b in range(1, 257) if sizes[b - 1] == sizes[b])


def _chain(O, w, op, sr, n_steps, dtype):
    """the oracle chain in `dtype` -> ((B, Lw) result, Ls, len_stretch, orig)"""
    Lw = w.shape[1]
    rate, len_stretch, orig = _terms(sr, Lw, n_steps)
    X = IO.stft(O, w, op, dtype)
    y = IO.istft(O, VO.phase_vocoder(X, rate, op.hop_length, dtype), op, dtype)
    Ls = y.shape[1]
    y = _fix(y, len_stretch)
    table = RO.sparse_table(orig, sr)
    if dtype == torch.float64:
        r = RO.sparse_resample(y, orig, sr, table=table)
    else:
        r = RO.sparse_resample_f32(y, orig, sr, RO.sparse_weights(orig, sr, torch.float32, table=table), table)
    return _fix(r, Lw), Ls, len_stretch, orig


def _chain_parity(O, name, plan, op, w, n_steps):
    """the chain gate on rows w (the last one zero): dev >= f32 - 6 dB on the samples outside the stated departure; returns their count"""
    sr, Lw = plan.sample_rate, w.shape[1]
    r64, Ls, len_stretch, orig = _chain(O, w.cpu(), op, sr, n_steps, torch.float64)
    r32 = _chain(O, w.cpu(), op, sr, n_steps, torch.float32)[0]
    got = plan.pitch_shift(w, n_steps).cpu()
    o, n, base, _ = RO.geometry(orig, sr)
    clear = Lw if len_stretch <= Ls else min(Lw, max(0, math.floor((Ls - 6 * o / base) * n / o)))  # outputs the departure cannot reach
    d, f = snr_db(r64[:-1, :clear], got[:-1, :clear]), snr_db(r64[:-1, :clear], r32[:-1, :clear])
    print(f"{name} n_steps {n_steps:+.3g}: {orig} -> {sr}, Ls {Ls}, len_stretch {len_stretch}, {clear} of {Lw} samples outside the departure: "
          f"dev {d:.1f} dB, float32 chain {f:.1f} dB; whole rows: dev {snr_db(r64[:-1], got[:-1]):.1f} dB, float32 chain {snr_db(r64[:-1], r32[:-1]):.1f} dB")
    assert d >= f - 6.0, (name, n_steps, d, f)
    return clear


@pytest.mark.parametrize("name", list(ENGINES))
def test_member_is_the_composition_and_parity(O, name):
    p, plan = _plan(name)
    op = O.params_from(p)
    sr, Lw = p.sample_rate, IO.samples(op, 41)
    w = synthetic_wave(3, Lw, seed=21).cuda()
    w[-1] = 0
    for n_steps in STEPS:
        want = _composition(plan, w, n_steps)
        got = plan.pitch_shift(w, n_steps)
        assert tuple(got.shape) == tuple(w.shape) == tuple(want.shape) and got.dtype == torch.float32
        assert got.data_ptr() != w.data_ptr() and _bits(got) == _bits(want), n_steps
        assert not got[-1].any()
    for n_steps in STEPS[:2]:
        assert _chain_parity(O, name, plan, op, w, n_steps) > Lw // 2


@pytest.mark.parametrize("n_steps", [12, -12])
@pytest.mark.parametrize("name", list(ENGINES))
def test_octaves_on_every_engine(O, name, n_steps):
    """the vocoder at exactly 0.5 and 2.0, the resampler at 2/1 and 1/2 (5512/11025 an octave down at 11025 Hz): composition in bits and the chain gate.  Rows of 41 frames; of
    61 where the departure would leave no more than half of a 41-frame row clear."""
    p, plan = _plan(name)
    op = O.params_from(p)
    for frames in (41, 61):
        Lw = IO.samples(op, frames)
        rate, len_stretch, orig = _terms(p.sample_rate, Lw, n_steps)
        assert rate == 2.0 ** (-n_steps // 12)
        if n_steps > 0 or p.sample_rate % 2 == 0:  # (an octave down at 11025 Hz: int(11025 / 2) = 5512 -> 11025, 5512 phases' worth of a pair)
            assert RO.geometry(orig, p.sample_rate)[:2] == ((2, 1) if n_steps > 0 else (1, 2))
        w = synthetic_wave(3, Lw, seed=25).cuda()
        w[-1] = 0
        got = plan.pitch_shift(w, n_steps)
        assert _bits(got) == _bits(_composition(plan, w, n_steps)) and not got[-1].any()
        clear = _chain_parity(O, name, plan, op, w, n_steps)
        if clear > Lw // 2:
            break
    assert clear > Lw // 2


@pytest.mark.parametrize("n_steps", [24, -24, 0.5])
def test_two_octaves_and_a_quarter_tone(n_steps):
    """rates 0.25 and 4 with the pairs 4/1 and 1/4, and a shift that is no whole semitone: composition in bits"""
    p, plan = _plan("specialised")
    Lw = p.hop_length * 40
    w = synthetic_wave(3, Lw, seed=26).cuda()
    w[-1] = 0
    orig = _terms(p.sample_rate, Lw, n_steps)[2]
    if abs(n_steps) == 24:
        assert RO.geometry(orig, p.sample_rate)[:2] == ((4, 1) if n_steps > 0 else (1, 4))
    got = plan.pitch_shift(w, n_steps)
    assert tuple(got.shape) == (3, Lw) and bool(torch.isfinite(got).all()) and bool(got[:-1].abs().sum(1).gt(0).all())
    assert _bits(got) == _bits(_composition(plan, w, n_steps)) and not got[-1].any()


@pytest.mark.parametrize("extra", [0, 1], ids=["40-hops", "41-hops-less-a-sample"])
def test_shifts_too_small_to_move_the_frequency(O, extra):
    """n_steps = +1e-9: int(sample_rate / rate) == sample_rate, the resampler returns its input and the fused entry copies the
    stretched rows (row pitches differ: the stretched row has a frame more) - no table is read, so NULL tables are accepted.
    n_steps = -1e-9: the frequency is sample_rate - 1, the pair 44099 -> 44100 of 44100 phases."""
    p, plan = _plan("specialised")
    op = O.params_from(p)
    lib, h, sr = plan.lib, plan.handle, p.sample_rate
    Lw = p.hop_length * 40 + extra * (p.hop_length - 1)
    w = synthetic_wave(3, Lw, seed=27).cuda()
    w[-1] = 0
    # the copy route
    up = 1e-9
    assert lib.rfx_pitch_shift_resample_freq(h, Lw, up, 12) == sr == _terms(sr, Lw, up)[2]
    want = _composition(plan, w, up)
    got = plan.pitch_shift(w, up)
    assert tuple(got.shape) == (3, Lw) and _bits(got) == _bits(want) and not got[-1].any() and bool(got[:-1].abs().sum(1).gt(0).all())
    assert _bits(got) != _bits(w)  # (the vocoder ran: no copy of the input)
    need = lib.rfx_pitch_shift_workspace_bytes(h, 3, Lw, up, 12)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((3 * Lw + 16,), 7.0, device="cuda")  # 16 canary values behind the samples
    s = torch.cuda.current_stream().cuda_stream
    assert lib.rfx_pitch_shift(h, w.data_ptr(), 3, Lw, up, 12, None, None, 0, out.data_ptr(), ws.data_ptr(), need, s) == 0, lib.rfx_last_error()
    torch.cuda.synchronize()
    assert bool((out[3 * Lw:] == 7.0).all()) and _bits(out[:3 * Lw]) == _bits(want)
    # one hertz down: the pair of 44100 phases
    down = -1e-9
    assert lib.rfx_pitch_shift_resample_freq(h, Lw, down, 12) == sr - 1 == _terms(sr, Lw, down)[2]
    got = plan.pitch_shift(w, down)
    assert _bits(got) == _bits(_composition(plan, w, down)) and not got[-1].any()
    assert _chain_parity(O, "specialised", plan, op, w, down) > Lw // 2


def test_composition_where_the_stretched_row_is_padded():
    """hop - 1 samples more than 40 hops: still 41 frames, so round(Lw / rate) exceeds the stretched row and step 2 pads"""
    p, plan = _plan("specialised")
    Lw = p.hop_length * 41 - 1
    w = synthetic_wave(3, Lw, seed=24).cuda()
    for n_steps in (2, -5):
        rate, len_stretch, _ = _terms(p.sample_rate, Lw, n_steps)
        assert len_stretch > plan.time_stretch_samples(Lw, rate)
        assert _bits(plan.pitch_shift(w, n_steps)) == _bits(_composition(plan, w, n_steps)), n_steps


def test_member_over_two_row_groups_and_the_converter():
    from riffusion.spectrogram_converter import SpectrogramConverter

    p, plan = _plan("specialised")
    Lw = p.hop_length * 40
    for n_steps in (2, -5):
        group = _group_rows(plan, Lw, n_steps)
        assert 1 < group < 256
        w = synthetic_wave(group + 1, Lw, seed=22).cuda()
        want = _composition(plan, w, n_steps)
        assert _bits(plan.pitch_shift(w, n_steps)) == _bits(want), n_steps
    # the converter: leading dimensions kept, a host input goes to the device
    conv = SpectrogramConverter(p, device="cuda")
    y = conv.pitch_shift(w[:3].cpu().reshape(1, 3, Lw), -5)
    assert tuple(y.shape) == (1, 3, Lw) and y.is_cuda and _bits(y[0]) == _bits(want[:3])
    assert tuple(conv.pitch_shift(w[0], -5).shape) == (Lw,)
    assert _bits(conv.pitch_shift(w[:3], 0)) == _bits(w[:3])
    assert _bits(conv.pitch_shift(w[:3], -10, bins_per_octave=24)) == _bits(want[:3])  # the same fraction of an octave
    with pytest.raises(RuntimeError, match="no backward"):
        conv.pitch_shift(w[:3].clone().requires_grad_(), 2)


def test_an_octave_up_doubles_a_sine():
    p, plan = _plan("specialised")
    Lw, sr = p.hop_length * 40, p.sample_rate
    t = torch.arange(Lw, dtype=torch.float64) / sr
    w = (8000 * torch.sin(2 * math.pi * 440.0 * t)).float().reshape(1, Lw).cuda()
    y = plan.pitch_shift(w, 12).cpu().double()[0]
    spec = torch.fft.rfft(y * torch.hann_window(Lw, dtype=torch.float64)).abs()
    peak = float(spec.argmax()) * sr / Lw
    print(f"peak at {peak:.1f} Hz (bins of {sr / Lw:.2f} Hz)")
    assert abs(peak - 880.0) <= sr / Lw


def test_command_line_shifts_a_stereo_clip(tmp_path):
    from riffusion import cli
    from riffusion.util import audio_util

    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    pcm = (np.random.default_rng(3).standard_normal((20000, 2)) * 3000).astype(np.int16)
    audio_util.PcmSegment(pcm, 44100).export(src, format="wav")
    cli.main(["pitch-shift", "--audio", src, "--output", dst, "--semitones", "-5"])
    seg = cli._load_segment(dst)
    assert seg.channels == 2 and int(seg.frame_rate) == 44100 and int(seg.frame_count()) == 20000  # the duration stays
    out = np.array(seg.get_array_of_samples()).reshape(-1, 2)
    assert np.abs(out.astype(np.int32)).max() >= 32766 and out[:, 0].any() and out[:, 1].any()  # channels are rows; the PCM tail peak-normalises


def test_contract_workspace_nulls_canaries_and_no_rows():
    from riffusion import _hip

    p, plan = _plan("specialised")
    lib, h = plan.lib, plan.handle
    B, Lw, n_steps = 2, p.hop_length * 40, 2.0
    orig = lib.rfx_pitch_shift_resample_freq(h, Lw, n_steps, 12)
    assert orig == 49500
    first, taps = _hip.resample_sinc_table(orig, p.sample_rate, device="cuda")
    f, t, nt = first.data_ptr(), taps.data_ptr(), int(taps.shape[0])
    w = synthetic_wave(B, Lw, seed=23).cuda()
    need = lib.rfx_pitch_shift_workspace_bytes(h, B, Lw, n_steps, 12)
    assert need > 0 and lib.rfx_pitch_shift_workspace_bytes(h, B, Lw, 0.0, 12) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((B * Lw + 16,), 7.0, device="cuda")  # 16 canary values behind the samples
    s = torch.cuda.current_stream().cuda_stream
    call = lib.rfx_pitch_shift
    # refusals come before any launch and leave the output untouched
    assert call(h, w.data_ptr(), B, Lw, n_steps, 12, f, t, nt, out.data_ptr(), ws.data_ptr(), need - 1, s) == -3
    for a in ((None, w.data_ptr(), f, t, out.data_ptr(), ws.data_ptr()), (h, None, f, t, out.data_ptr(), ws.data_ptr()), (h, w.data_ptr(), None, t, out.data_ptr(), ws.data_ptr()),
              (h, w.data_ptr(), f, None, out.data_ptr(), ws.data_ptr()), (h, w.data_ptr(), f, t, None, ws.data_ptr()), (h, w.data_ptr(), f, t, out.data_ptr(), None)):
        assert call(a[0], a[1], B, Lw, n_steps, 12, a[2], a[3], nt, a[4], a[5], need, s) == -1 and b"null" in lib.rfx_last_error()
    assert call(h, w.data_ptr(), B, Lw, float("nan"), 12, f, t, nt, out.data_ptr(), ws.data_ptr(), need, s) == -1
    assert call(h, w.data_ptr(), B, Lw, n_steps, 0, f, t, nt, out.data_ptr(), ws.data_ptr(), need, s) == -1
    assert call(h, w.data_ptr(), B, Lw, n_steps, 12, f, t, 0, out.data_ptr(), ws.data_ptr(), need, s) == -1
    assert call(h, w.data_ptr(), B, p.n_fft // 2, n_steps, 12, f, t, nt, out.data_ptr(), ws.data_ptr(), need, s) == -1  # rfx_stft's refusal
    assert call(h, w.data_ptr(), B, Lw, n_steps, 12, f, t, nt, w.data_ptr() + 4 * Lw, ws.data_ptr(), need, s) == -1 and b"overlap" in lib.rfx_last_error()
    assert call(h, w.data_ptr(), 0, Lw, n_steps, 12, f, t, nt, out.data_ptr(), ws.data_ptr(), need, s) == 0  # B == 0 is a no-op
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the call writes its samples and nothing behind them; n_steps == 0 copies without a table or a workspace
    assert call(h, w.data_ptr(), B, Lw, n_steps, 12, f, t, nt, out.data_ptr(), ws.data_ptr(), need, s) == 0
    torch.cuda.synchronize()
    assert bool((out[B * Lw:] == 7.0).all()) and _bits(out[:B * Lw]) == _bits(plan.pitch_shift(w, n_steps))
    assert call(h, w.data_ptr(), B, Lw, 0.0, 12, None, None, 0, out.data_ptr(), None, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((out[B * Lw:] == 7.0).all()) and _bits(out[:B * Lw]) == _bits(w)
