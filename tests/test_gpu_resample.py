"""
The windowed-sinc resampler on the device (include/rfx.h "SINC RESAMPLE"; csrc/rfx_resample.hip) against the float64 oracle
(tests/resample_oracle.py, a transcription of torchaudio.functional.resample), with the inputs and gates of tests/test_resample_cpu.py.

Cases: B = 3 rows, the last all zero; L = 5 (shorter than the filter), 2000, and 3001 (K is no multiple of a workgroup's 256 outputs);
pairs 2/1 and 1/2, 55/49, 160/147 and 147/160, 7787/7350 (more phases than outputs at L = 2000: only q = 0) and 33037/44100.
PARITY: every figure is an SNR against the float64 oracle, all printed.
    dev >= f32         the all-float32 oracle, what functional.resample computes on a float32 waveform: outright
    dev >= k64 - 6 dB  the float64 kernel rounded to float32, what transforms.Resample computes: the project's rule
(33037/44100 has no dense kernel: its two figures are the sparse float32 forms, as on the CPU.)
Bits: dev == the host emulator; a row alone == the row in the batch, also at B = 5, one row more than a thread's four; x * 2^+-40
gives the result * 2^+-40 exactly; the zero row leaves as zeros; orig == new is a copy; an input delayed by o samples gives the output
delayed by n; `audio_util.resample_waveform` is the same call with leading dimensions kept and a host input moved to the device.
The wider cases (WIDE_CASES of tests/test_resample_cpu.py, with its inputs and its two sparse float32 figures): integer decimation 4/1
and 12/1 (n = 1: one phase, every lane reads the same weight, up to 145 taps), 1/4 and 1/12 (o = 1), 3/2, and 44099/44100 and
44100/44099 (the pairs a tiny pitch shift produces: 44100 and 44099 phases, far more than outputs) at L = 1, 2, 255, 1000; the filters
(lowpass_filter_width, rolloff) = (1, 0.99), (16, 0.99), (64, 0.9476), (6, 1.0), (6, 0.5) at 55/49, 1/2, 2/1; 160/147 at K = 255 .. 258
around a workgroup's 256 outputs.  Bits == the emulator, the two parity gates, the zero row, a row alone.  Row blocks: B = 4, 8, 9
(one full block of a thread's four rows, two, two and a row) at 3/2 against the emulator in bits.  THE LAUNCH SEAM: 65535 * 4 + 5 rows
of 8 samples at 1/2 - the second trip of launch_resample_sinc's loop over 65535 row blocks - rows on both sides of the seam equal the
same rows resampled alone.
Contract: canary values past the output stay; NULL pointers, bad frequencies, an overlap and a misalignment are -1 and a table past
the cap -4, the output untouched; B = 0 is a no-op.
"""
import pytest
import torch

import resample_oracle as RO
from engines import bits as _bits
from helpers import snr_db
from resample_cases import LENGTHS, PAIRS, WIDE_CASES, WIDE_IDS, emulator, gates, run_emu, wave, wide_gates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return emulator()


def _dev(x, orig, new, lpw=6, rolloff=0.99):
    from riffusion import _hip

    y = _hip.resample_sinc(x.cuda(), orig, new, lpw, rolloff)
    assert y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0], RO.frames(x.shape[1], orig, new))
    return y.cpu()


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("orig,new", PAIRS)
def test_parity_and_bits(emu, orig, new, L):
    o, n, _, _ = RO.geometry(orig, new)
    r64, f32, k64 = gates(orig, new, L)
    x = wave(L)
    y = _dev(x, orig, new)
    d = snr_db(r64[:-1], y[:-1])
    print(f"{orig}/{new} L{L}: dev {d:.1f} dB, all-float32 {f32:.1f} dB, float32-rounded kernel {k64:.1f} dB")
    assert torch.isfinite(y).all()
    assert d >= f32, (orig, new, L, d, f32)
    assert d >= k64 - 6.0, (orig, new, L, d, k64)
    assert _bits(y) == _bits(run_emu(emu, x, orig, new))  # the emulator, bit for bit
    assert not y[-1].any()  # the zero row leaves as zeros
    for r in (0, 2):
        assert _bits(_dev(x[r:r + 1], orig, new)) == _bits(y[r:r + 1]), r
    x5 = wave(L, B=5, seed=1)  # one row more than a thread carries
    y5 = _dev(x5, orig, new)
    assert _bits(y5) == _bits(run_emu(emu, x5, orig, new))
    for r in (3, 4):
        assert _bits(_dev(x5[r:r + 1], orig, new)) == _bits(y5[r:r + 1]), r
    for e in (40, -40):
        assert _bits(_dev(x * 2.0 ** e, orig, new)) == _bits(y * 2.0 ** e), e
    yd = _dev(torch.nn.functional.pad(x, (o, 0)), orig, new)  # delayed by o samples: the output is delayed by n
    assert yd.shape[1] == y.shape[1] + n and _bits(yd[:, n:]) == _bits(y)


@pytest.mark.parametrize("orig,new,L,lpw,rolloff", WIDE_CASES, ids=WIDE_IDS)
def test_parity_and_bits_at_the_wide_cases(emu, orig, new, L, lpw, rolloff):
    r64, f32, k64 = wide_gates(orig, new, L, lpw, rolloff)
    x = wave(L)
    y = _dev(x, orig, new, lpw, rolloff)
    d = snr_db(r64[:-1], y[:-1])
    print(f"{orig}/{new} L{L} lpw {lpw} rolloff {rolloff:.4g}: K {y.shape[1]}, dev {d:.1f} dB, all-float32 {f32:.1f} dB, float32-rounded kernel {k64:.1f} dB")
    assert tuple(y.shape) == tuple(r64.shape) and torch.isfinite(y).all()
    assert _bits(y) == _bits(run_emu(emu, x, orig, new, lpw=lpw, rolloff=rolloff))  # the emulator, bit for bit
    assert d >= f32, (orig, new, L, d, f32)
    assert d >= k64 - 6.0, (orig, new, L, d, k64)
    assert not y[-1].any()  # the zero row leaves as zeros
    for r in (0, 2):
        assert _bits(_dev(x[r:r + 1], orig, new, lpw, rolloff)) == _bits(y[r:r + 1]), r


@pytest.mark.parametrize("B", [4, 8, 9])
def test_row_blocks_are_the_emulators(emu, B):
    """one full block of a thread's four rows, two, two and a row: the last block's clamped rows are read and not stored"""
    x = wave(1000, B=B, seed=2)
    y = _dev(x, 3, 2)
    assert _bits(y) == _bits(run_emu(emu, x, 3, 2))
    assert not y[-1].any() and bool(y[:-1].abs().sum(1).gt(0).all())


def test_rows_past_one_launch():
    """65535 * 4 + 5 rows: the kernel's second launch starts at row 262140 with its pointers moved on"""
    from riffusion import _hip

    B, L = 65535 * 4 + 5, 8
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(4321), dtype=torch.float32).cuda()  # every row its own content
    y = _hip.resample_sinc(x, 1, 2)
    assert tuple(y.shape) == (B, 16)
    print(f"{B} rows: {x.numel() * 4 / 2 ** 20:.1f} MiB in, {y.numel() * 4 / 2 ** 20:.1f} MiB out")
    for r in (0, 262139, 262140, 262141, B - 1):
        alone = _hip.resample_sinc(x[r:r + 1], 1, 2)
        assert bool(alone.any()) and _bits(alone.cpu()) == _bits(y[r:r + 1].cpu()), r
    # ... and every row: two calls of fewer rows than one launch takes, the cut away from the seam
    halves = torch.cat([_hip.resample_sinc(x[:200000], 1, 2), _hip.resample_sinc(x[200000:], 1, 2)])
    assert torch.equal(halves.view(torch.int32), y.view(torch.int32))


def test_equal_frequencies_copy_and_the_wrapper():
    from riffusion import _hip
    from riffusion.util import audio_util

    x = wave(2000).cuda()
    y = _hip.resample_sinc(x, 44100, 44100)
    assert y.data_ptr() != x.data_ptr() and _bits(y.cpu()) == _bits(x.cpu())
    want = _hip.resample_sinc(x, 48000, 44100)
    got = audio_util.resample_waveform(x.cpu().reshape(1, 3, 2000), 48000, 44100)  # a host input goes to the device; leading dimensions stay
    assert got.is_cuda and tuple(got.shape) == (1, 3, want.shape[1]) and _bits(got[0].cpu()) == _bits(want.cpu())
    assert tuple(audio_util.resample_waveform(x[0], 48000, 44100).shape) == (want.shape[1],)
    assert _bits(audio_util.resample_waveform(x.double(), 96000, 88200).cpu()) == _bits(want.cpu())  # the reduced pair decides
    first, taps = _hip.resample_sinc_table(48000, 44100, device="cuda")
    assert _hip.resample_sinc_table(48000, 44100, device="cuda")[1].data_ptr() == taps.data_ptr()  # uploaded once
    assert tuple(first.shape) == (147,) and tuple(taps.shape) == (14, 147)


def test_contract_nulls_canaries_and_no_rows():
    from riffusion import _hip

    lib = _hip.load_library()
    B, L, orig, new = 3, 3001, 55, 49
    K = RO.frames(L, orig, new)
    first, taps = _hip.resample_sinc_table(orig, new, device="cuda")
    nt = int(taps.shape[0])
    x = wave(L).cuda()
    out = torch.full((B * K + 16,), 7.0, device="cuda")  # 16 canary values behind the samples
    s = torch.cuda.current_stream().cuda_stream
    f, t, xi, oo = first.data_ptr(), taps.data_ptr(), x.data_ptr(), out.data_ptr()
    call = lib.rfx_resample_sinc
    # refusals come before any launch and leave the output untouched
    for args in ((None, f, t, oo), (xi, None, t, oo), (xi, f, None, oo), (xi, f, t, None)):
        assert call(args[0], B, L, orig, new, args[1], args[2], nt, args[3], s) == -1 and b"null" in lib.rfx_last_error()
    assert call(xi, B, L, 0, new, f, t, nt, oo, s) == -1 and call(xi, B, L, orig, -3, f, t, nt, oo, s) == -1
    assert call(xi, B, 0, orig, new, f, t, nt, oo, s) == -1 and call(xi, -1, L, orig, new, f, t, nt, oo, s) == -1
    assert call(xi, B, L, orig, new, f, t, 0, oo, s) == -1
    assert call(xi + 2, B, L, orig, new, f, t, nt, oo, s) == -1 and call(xi, B, L, orig, new, f, t, nt, oo + 2, s) == -1
    assert call(xi, B, L, orig, new, f, t, nt, xi + 4 * L, s) == -1 and b"overlap" in lib.rfx_last_error()
    assert call(xi, 1, 5, 1, 2 ** 23 + 1, f, t, nt, oo, s) == -4
    assert call(xi, 0, L, orig, new, f, t, nt, oo, s) == 0  # B == 0 is a no-op
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the call writes its samples and nothing behind them
    assert call(xi, B, L, orig, new, f, t, nt, oo, s) == 0
    torch.cuda.synchronize()
    assert bool((out[B * K:] == 7.0).all())
    assert _bits(out[:B * K].cpu()) == _bits(_hip.resample_sinc(x, orig, new).cpu())
