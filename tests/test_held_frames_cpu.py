"""
CPU checks of held frames (include/rfx.h: rfx_held_call_options): a guided Griffin-Lim call keeps the first `head` and the last
`tail` frames of a row at the guide's phase through every iteration.

* The compaction of the free frames into a list (csrc/rfx_guide.hip): the arithmetic header csrc/rfx_guide_core.h is compiled for
  the host together with tests/emu/rfx_hold_emu.cpp, which walks the logical threads of the three launches, and the list and its
  count are checked against numpy, exactly.  Buffers start as a sentinel: every entry below the count is written, none beyond it.
* `hold_frames_for` against a brute-force count over frames.
* The layout of the grown options struct against the header, and the refusals that need no device.
* The definition, on the oracle (tests/held_oracle.py): 64 frames of golden clip 2, the guide the clip with a span zeroed.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import held_oracle
import helpers
from engines import clip2_segment

EMU_SRC = "rfx_hold_emu.cpp"
SENTINEL = -0x12345678


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    lib.emu_hold_list_words.argtypes = [ctypes.c_longlong, ctypes.c_int]
    lib.emu_hold_list_words.restype = ctypes.c_longlong
    lib.emu_hold_list.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    lib.emu_hold_list.restype = None
    lib.emu_hold_is_held.argtypes = [ctypes.c_int] * 4
    return lib


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


def compact(emu, holds, T):
    """(the list's entries below the count, the count, the whole buffer)"""
    holds = np.ascontiguousarray(holds, np.int32).reshape(-1, 2)
    B = holds.shape[0]
    words = emu.emu_hold_list_words(B, T)
    assert B * T + 1 <= words <= B * T + 1 + -(-B // emu.emu_hold_chunk_rows()) + 3 and words % 4 == 0
    buf = np.full(words, SENTINEL, np.int32)
    emu.emu_hold_list(holds.ctypes.data, B, T, buf.ctypes.data)
    count = int(buf[B * T])
    return buf[:count], count, buf


def expected_list(holds, T):
    mask = held_oracle.held_mask(holds, T).numpy()
    return np.flatnonzero(~mask.reshape(-1)).astype(np.int32)


# ---- the compaction's emulator against numpy --------------------------------------------------------------------------------------------

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MIXED = [(0, 0), (33, 0), (0, 33), (7, 3), (20, 20), (40, 1), (1, 40), (-5, 4), (4, -5), (-1, -1), (INT_MAX, INT_MAX), (INT_MIN, INT_MIN), (INT_MAX, INT_MIN),
         (INT_MIN, INT_MAX), (16, 17), (17, 17)]


@pytest.mark.parametrize("T", [33, 16, 2, 61])
def test_compaction_lists_the_free_frames_in_order(emu, T):
    got, count, buf = compact(emu, MIXED, T)
    want = expected_list(MIXED, T)
    assert count == len(want) and np.array_equal(got, want)
    B = len(MIXED)
    assert (buf[count:B * T] == SENTINEL).all()  # nothing is written between the last entry and the count
    assert (np.diff(got) > 0).all()


@pytest.mark.parametrize("pair,free", [((0, 0), 33), ((33, 0), 0), ((0, 33), 0), ((100, 100), 0), ((-3, -3), 33), ((30, 30), 0), ((10, 30), 0), ((10, 20), 3)])
def test_compaction_of_one_row(emu, pair, free):
    got, count, buf = compact(emu, [pair], 33)
    assert count == free and np.array_equal(got, expected_list([pair], 33))
    assert (buf[count:33] == SENTINEL).all()


def test_held_predicate_matches_its_definition(emu):
    T = 9
    for head in (-2, 0, 1, 4, 9, 12):
        for tail in (-2, 0, 1, 5, 9, 12):
            h = min(max(head, 0), T)
            l = min(max(tail, 0), T - h)
            for t in range(T):
                assert bool(emu.emu_hold_is_held(t, head, tail, T)) == (t < h or t >= T - l), (head, tail, t)


def test_compaction_past_65535_rows_and_chunk_boundaries(emu):
    """70 001 rows of three frames: 69 chunks of 1024 rows, the last one partial; pairs drawn so that chunks differ in their counts"""
    rng = np.random.default_rng(7)
    B, T = 70001, 3
    holds = rng.integers(-2, 5, (B, 2)).astype(np.int32)
    holds[1024 * 3:1024 * 5] = (3, 0)  # two whole chunks with nothing free
    got, count, buf = compact(emu, holds, T)
    want = expected_list(holds, T)
    assert count == len(want) and np.array_equal(got, want)
    assert (buf[count:B * T] == SENTINEL).all()
    # everything free, and nothing free
    got, count, _ = compact(emu, np.zeros((B, 2), np.int32), T)
    assert count == B * T and np.array_equal(got, np.arange(B * T, dtype=np.int32))
    got, count, buf = compact(emu, np.full((B, 2), 2, np.int32), T)
    assert count == 0 and (buf[:B * T] == SENTINEL).all()


def test_a_rows_part_of_the_list_does_not_depend_on_the_other_rows_pairs(emu):
    T = 33
    a = [(0, 0), (7, 3), (33, 0)]
    b = [(5, 5), (7, 3), (0, 0)]
    la, lb = compact(emu, a, T)[0], compact(emu, b, T)[0]
    assert np.array_equal(la[(la >= T) & (la < 2 * T)], lb[(lb >= T) & (lb < 2 * T)])


# ---- hold_frames_for -------------------------------------------------------------------------------------------------------------------

def _brute_force(p, n_known, T=2000):
    """frames t whose window [hop t - win // 2, hop t - win // 2 + win) reaches no sample at or beyond n_known (the known audio is
    [0, n_known); what lies before the clip is the reflection of known audio)"""
    count = 0
    for t in range(T):
        if p.hop_length * t - p.win_length // 2 + p.win_length <= n_known:
            count += 1
        else:
            break
    return count


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=48000), dict(sample_rate=16000, window_duration_ms=64, step_size_ms=8, max_frequency=8000)],
                         ids=["default", "48k", "16k-64ms"])
def test_hold_frames_for_counts_the_frames_inside_the_known_audio(kw):
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams(**kw)
    assert p.hold_frames_for() == (0, 0)
    for seconds in (0.0, 0.01, p.win_length / 2 / p.sample_rate, 0.0499, 0.05, 0.051, 0.2, 0.24, 1.0, 2.5):
        n = int(seconds * p.sample_rate)
        # win_length is even in these geometries: the window's right end is hop t + win // 2
        want = _brute_force(p, n)
        assert p.hold_frames_for(head_s=seconds) == (want, 0), seconds
        assert p.hold_frames_for(tail_s=seconds) == (0, want), seconds
        assert p.hold_frames_for(seconds, seconds) == (want, want)
    # the stated rule
    n = 8820
    assert p.hold_frames_for(head_s=n / p.sample_rate)[0] == (0 if n < p.win_length // 2 else (n - p.win_length // 2) // p.hop_length + 1)


def test_hold_rows_takes_a_pair_or_an_array_and_clamps():
    from riffusion.spectrogram_converter import hold_rows

    assert hold_rows((3, 4), 2, 10).tolist() == [[3, 4], [3, 4]]
    assert hold_rows(np.array([[1, 2], [50, -3]]), 2, 10).tolist() == [[1, 2], [10, 0]]
    got = hold_rows(torch.tensor([[2 ** 40, 0]]), 1, 10)
    assert got.dtype == torch.int32 and got.tolist() == [[10, 0]]
    for bad in ((1, 2, 3), np.zeros((3, 2), np.int64), (0.5, 1.0)):
        with pytest.raises(ValueError):
            hold_rows(bad, 2, 10)


# ---- rfx_held_call_options: layout and the refusals that need no device ------------------------------------------------------------------------

def test_held_options_layout_matches_the_header(repo_root, tmp_path):
    from riffusion import _hip

    exe = emu_build.header_compiles_as_c99(
        tmp_path,
        '#include <stddef.h>\n#include <stdio.h>\n#include "rfx.h"\n'
        "#define O(f) (int)offsetof(rfx_held_call_options, f)\n"
        "int main(void) {\n"
        '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(rfx_guided_call_options), (int)sizeof(rfx_held_call_options), O(flags), O(row_base),\n'
        "         O(magnitude_hint), O(reserved), O(d_guide), O(guide_stride), O(guide_samples), O(reserved2), O(d_hold_frames), O(reserved3), rfx_version());\n"
        "  return 0;\n}\n",
        link=True, extra=("-Wextra",))
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    H, G = _hip.RfxHeldCallOptions, _hip.RfxGuidedCallOptions
    assert got[:2] == [ctypes.sizeof(G), ctypes.sizeof(H)] == [48, 64]
    assert got[2:12] == [H.flags.offset, H.row_base.offset, H.magnitude_hint.offset, H.reserved.offset, H.d_guide.offset, H.guide_stride.offset,
                         H.guide_samples.offset, H.reserved2.offset, H.d_hold_frames.offset, H.reserved3.offset]
    # the guided-size prefix is the guided struct
    assert [getattr(H, f).offset for f, _ in G._fields_] == [getattr(G, f).offset for f, _ in G._fields_]
    assert (H.d_hold_frames.offset, H.reserved3.offset) == (48, 56)


def test_held_options_builder():
    from riffusion import _hip

    g = torch.zeros(3, 50)
    hold = torch.tensor([[0, 0], [7, 3], [33, 0]], dtype=torch.int32)
    assert isinstance(_hip.call_options(rows=3, row_base=2), _hip.RfxCallOptions)
    assert isinstance(_hip.call_options(guide=g, rows=3), _hip.RfxGuidedCallOptions)
    o = _hip.call_options(guide=g[:, :40], hold=hold, rows=3, row_base=2, magnitude_hint=5.0, lstsq=True)
    assert (o.struct_size, o.flags, o.row_base, o.magnitude_hint) == (64, 1, 2, 5.0)
    assert (o.d_guide, o.guide_stride, o.guide_samples, o.reserved2, o.d_hold_frames, o.reserved3) == (g.data_ptr(), 50, 40, 0, hold.data_ptr(), 0)
    with pytest.raises(ValueError, match="needs a guide"):
        _hip.call_options(hold=hold, rows=3)
    for bad in (hold[:2], hold.long(), hold.t(), hold[:, :1], torch.zeros(3, 4, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError):
            _hip.call_options(guide=g, hold=bad, rows=3)


def _held(d_guide=0x1000, d_hold=0x2000, reserved3=0, size=None):
    from riffusion import _hip

    return _hip.RfxHeldCallOptions(ctypes.sizeof(_hip.RfxHeldCallOptions) if size is None else size, 0, 0, 0.0, 0.0, d_guide, 100, 100, 0, d_hold, reserved3)


def _gl_ex(lib, opt):
    return lib.rfx_griffinlim_ex(None, None, None, 0, 1, 30, 0, 0.5, None, None, 0, None, ctypes.byref(opt), None)


@pytest.mark.parametrize("kw,word", [(dict(d_guide=None), b"needs a guide"), (dict(d_hold=0x2002), b"aligned"), (dict(reserved3=1), b"reserved3"),
                                     (dict(reserved3=1, d_hold=None), b"reserved3")])
def test_held_options_are_refused_before_any_device_work(lib, kw, word):
    """the options are read before the plan and the buffers are looked at: null everything else, no GPU needed"""
    opt = _held(**kw)
    assert _gl_ex(lib, opt) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_ex(None, None, 1, 30, 1, 0, 1, 0.5, None, None, 0, None, ctypes.byref(opt)) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_audio_from_image_u8_ex(None, None, 1, 30, 0, None, 0, 1, 0.5, 1, None, None, None, 0, None, ctypes.byref(opt)) == -1
    assert word in lib.rfx_last_error()
    assert helpers.queries_refuse(lib, opt, word)


def test_inverse_mel_refuses_held_frames_and_shorter_structs_ignore_the_tail(lib):
    opt = _held(d_guide=None)
    assert lib.rfx_inverse_mel_ex(None, None, 1, 1, 1, None, 0, None, None, 0, None, ctypes.byref(opt)) == -1 and b"holds no frames" in lib.rfx_last_error()
    # a valid held struct passes the options and fails on the null plan; the guided size ignores the tail
    assert _gl_ex(lib, _held()) == -1 and b"null argument" in lib.rfx_last_error()
    assert _gl_ex(lib, _held(reserved3=1, size=48)) == -1 and b"null argument" in lib.rfx_last_error()
    # the workspace queries answer 0 for a held call without a plan, like their drivers' own
    assert helpers.need(lib, "griffinlim", None, 3, 33, **helpers.HELD) == 0 == helpers.need(lib, "waveform_from_mel", None, 3, 33, **helpers.HELD)
    assert helpers.need(lib, "audio_from_image", None, 3, 0, 33, **helpers.HELD) == 0


def test_cli_hold_flags_need_a_guide(capsys):
    from riffusion import cli

    for flags in (["--hold-head-ms", "100"], ["--hold-tail-ms", "100"], ["--hold-head-ms", "100", "--hold-tail-ms", "50"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["image-to-audio", "--image", "x.png", "--audio", "y.wav", *flags])
        assert e.value.code == 2 and "--guide-audio" in capsys.readouterr().err


# ---- the definition, on the oracle -------------------------------------------------------------------------------------------------------

FRAMES, START, ZERO_LO, ZERO_HI = 64, 44100, 8820, 19404
HOLD = (16, 15)


@pytest.fixture(scope="module")
def clip2(golden_dir):
    """(oracle, params, true magnitudes (1, n_stft, 64) of the mono clip, a0 of the guide: the clip with [8820, 19404) zeroed)"""
    O, op, wav = clip2_segment(golden_dir, FRAMES, START)
    x = wav.mean(dim=0, keepdim=True)
    mag = O.stft_complex(x, op).abs()
    guide = x.clone()
    guide[:, ZERO_LO:ZERO_HI] = 0
    G = O.stft_complex(guide, op)
    return O, op, mag, G / (G.abs() + 1e-16)


@pytest.mark.parametrize("n_iter", [0, 1, 4])
def test_oracle_nothing_held_is_the_guided_call(clip2, n_iter):
    O, op, mag, a0 = clip2
    assert torch.equal(held_oracle.held_griffinlim(O, mag, op, a0, [(0, 0)], n_iter), O.griffinlim(mag, op, angles0=a0, n_iter=n_iter))


@pytest.mark.parametrize("pair", [(FRAMES, 0), (0, FRAMES), (30, 34), (100, 100)])
def test_oracle_everything_held_is_the_start(clip2, pair):
    O, op, mag, a0 = clip2
    assert torch.equal(held_oracle.held_griffinlim(O, mag, op, a0, [pair], 4), O.griffinlim(mag, op, angles0=a0, n_iter=0))


def test_oracle_held_only_samples_do_not_move(clip2):
    """samples that only held frames reach keep their n_iter = 0 values; the start-only guided decode drifts (44.6 dB at 4 iterations
    when this was written: a figure, not a gate)"""
    O, op, mag, a0 = clip2
    start = O.griffinlim(mag, op, angles0=a0, n_iter=0)
    only = held_oracle.held_only_samples([HOLD], FRAMES, op)
    # the first free frame, 16, starts at 16 hop - win // 2; the last one, 48, ends at 48 hop + win // 2
    assert int(only.sum()) == (16 * op.hop_length - op.win_length // 2) + (start.shape[1] - (48 * op.hop_length + op.win_length // 2))
    held = held_oracle.held_griffinlim(O, mag, op, a0, [HOLD], 4)
    free = O.griffinlim(mag, op, angles0=a0, n_iter=4)
    assert torch.equal(held[only], start[only])
    assert not torch.equal(held[~only], start[~only])
    print(f"kept samples vs. their n_iter = 0 values at 4 iterations: start-only {held_oracle.db(start[only], free[only]):.1f} dB, held equal; "
          f"spectral convergence start-only {O.spectral_convergence(free, mag, op):.4f}, held {O.spectral_convergence(held, mag, op):.4f}")
