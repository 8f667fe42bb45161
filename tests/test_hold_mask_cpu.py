"""
CPU checks of masked calls (include/rfx.h: rfx_masked_call_options): a guided Griffin-Lim call keeps chosen bins of chosen frames at
the guide's phase through every iteration.

* The definition and the form the device runs, on the oracle (tests/mask_oracle.py): in float64 the split form - iterate on S_free,
  add c = ISTFT(S_held a0) - equals the `where` form to 1e-12; the table of DESIGN 4.1 (kept-bin fidelity and spectral convergence, held
  against start-only) is re-derived and printed, its directions asserted.  Inputs: 64 frames of golden clip 2 from sample 44100
  (mono mix) as the guide; target magnitudes the guide's in the kept bins and clip 0's elsewhere; kept bins those below bin 1444
  (3.6 kHz) in every frame, plus every 8th frame entirely.
* The two kernels' arithmetic (csrc/rfx_holdmask_core.h) is compiled for the host with tests/emu/rfx_holdmask_emu.cpp and checked
  against numpy, exactly: the split in the three slot orders, the band-to-bin expansion.
* rfx_debug_bin_bands against a numpy restatement from `_hip.mel_filterbank`.
* The layout of the grown options struct against the header, and the refusals that need no device.
* `image_util.hold_mask_from_image` on two fixtures: tests/golden/mask_gradient_dark.png and tests/golden/mask_beat_lines_80.png are
  verbatim copies of the reference's `seed_images/mask_gradient_dark.png` and `seed_images/mask_beat_lines_80.png` (512 x 512,
  palette mode), two of the stock masks of its partial regeneration.
"""
import ctypes
import os
import subprocess
import wave

import numpy as np
import pytest
import torch

import emu_build
import helpers
import mask_oracle

EMU_SRC = "rfx_holdmask_emu.cpp"
SPEC, PLAIN, TABLE = 0, 1, 2  # kHoldMaskSpec / kHoldMaskPlain / kHoldMaskTable


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    lib.emu_holdmask_slot_bin.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.emu_holdmask_split.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5
    lib.emu_holdmask_split.restype = None
    lib.emu_holdmask_bands.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4
    lib.emu_holdmask_bands.restype = None
    return lib


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


# ---- the definition and the split form, on the oracle -------------------------------------------------------------------------------------

FRAMES, START, KEPT_BELOW = 64, 44100, 1444


def _mono(golden_dir, name, op):
    with wave.open(os.path.join(golden_dir, name)) as w:
        assert w.getframerate() == op.sample_rate and w.getsampwidth() == 2 and w.getnchannels() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    seg = pcm[START:START + op.hop_length * (FRAMES - 1)].astype(np.float64).mean(axis=1)
    return torch.from_numpy(seg[None].copy())


@pytest.fixture(scope="module")
def inputs(golden_dir):
    """(oracle, params, S (1, n_stft, 64) float64, G the guide's STFT, a0, held (1, n_stft, 64) bool)"""
    import riffusion_oracle as O
    from riffusion.spectrogram_params import SpectrogramParams

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    op = O.params_from(SpectrogramParams())
    window = O.hann_window(op).double()

    def stft(x):
        return torch.stft(x, n_fft=op.n_fft, hop_length=op.hop_length, win_length=op.win_length, window=window, center=True, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True)

    G = stft(_mono(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav", op))
    other = stft(_mono(golden_dir, "clip_0_start_15795_ms_duration_5678_ms.wav", op)).abs()
    held = np.zeros((1, op.n_stft, FRAMES), dtype=bool)
    held[:, :KEPT_BELOW, :] = True
    held[:, :, ::8] = True
    S = torch.where(torch.from_numpy(held), G.abs(), other)
    return O, op, S, G, G / (G.abs() + 1e-16), held, stft


@pytest.fixture(scope="module")
def where64(inputs):
    """the `where` form in float64 at the table's iteration counts, computed once"""
    O, op, S, G, a0, held, _ = inputs
    return {n: mask_oracle.masked_griffinlim(O, S, op, a0, held, n, dtype=torch.float64) for n in (0, 4, 8, 32)}


@pytest.mark.parametrize("n_iter", [4, 32])
def test_split_form_equals_the_where_form_in_float64(inputs, where64, n_iter):
    O, op, S, G, a0, held, _ = inputs
    split = mask_oracle.masked_griffinlim(O, S, op, a0, held, n_iter, dtype=torch.float64, split=True)
    rel = float((split - where64[n_iter]).norm() / where64[n_iter].norm())
    print(f"split form against where form, float64, n_iter = {n_iter}: {rel:.2e} relative")
    assert rel <= 1e-12


def test_holding_keeps_the_kept_bins_near_the_source(inputs, where64):
    """the table behind DESIGN 4.1's figures, re-derived: kept-bin fidelity 10 log10(sum |G|^2 / sum |G - X|^2) over the kept bins and spectral
    convergence against the call's magnitudes, held against start-only.  Figures are printed; the directions at n_iter = 32 are
    asserted."""
    O, op, S, G, a0, held, stft = inputs
    none = np.zeros_like(held)

    def figures(x):
        X = stft(x)
        return mask_oracle.kept_bin_fidelity_db(G, X, held), float((X.abs() - S).norm() / S.norm())

    rows = {}
    for n in (0, 4, 8, 32):
        free = mask_oracle.masked_griffinlim(O, S, op, a0, none, n, dtype=torch.float64)
        rows[n] = (figures(where64[n]), figures(free))
        (hf, hs), (ff, fs) = rows[n]
        print(f"n_iter {n:2d}: kept-bin fidelity held / start-only {hf:.1f} / {ff:.1f} dB, spectral convergence {hs:.4f} / {fs:.4f}")
    assert rows[0][0] == rows[0][1]
    assert rows[32][0][0] > rows[32][1][0]  # held keeps the kept bins closer to the source than start-only does
    assert rows[32][1][0] < rows[0][1][0]   # start-only drifts away from its own start


def test_oracle_exact_consequences(inputs):
    O, op, S, G, a0, held, _ = inputs
    S32, a32 = S.float(), a0.to(torch.complex64)
    none, all_ = np.zeros_like(held), np.ones_like(held)
    start = O.griffinlim(S32, op, angles0=a32, n_iter=0)
    for split in (False, True):
        assert torch.equal(mask_oracle.masked_griffinlim(O, S32, op, a32, held, 0, split=split), start)
        assert torch.equal(mask_oracle.masked_griffinlim(O, S32, op, a32, none, 2, split=split), O.griffinlim(S32, op, angles0=a32, n_iter=2))
        assert torch.equal(mask_oracle.masked_griffinlim(O, S32, op, a32, all_, 2, split=split), start)


# ---- the split's emulator against numpy -----------------------------------------------------------------------------------------------------

def _spec_bin_of():
    """bin of every position of the specialised layout (-1: padding), from the layout's forward statement (csrc/rfx_core.h): slot
    (k1, ka, kb) holds k = k1 + 40 (ka + 21 kb), or 17640 - k above 8820; thread q = 21 k1 + ka sits at qp = q + q // 63; float
    arrays hold four consecutive kb per 16 bytes, kb = 20 behind them"""
    binof = np.full(9408, -1, np.int64)
    for k1 in range(21):
        for ka in range(21):
            q = k1 * 21 + ka
            qp = q + q // 63
            for kb in range(21):
                k = k1 + 40 * (ka + 21 * kb)
                pos = ((kb >> 2) * 448 + qp) * 4 + (kb & 3) if kb < 20 else 20 * 448 + qp
                assert binof[pos] == -1
                binof[pos] = 17640 - k if k > 8820 else k
    return binof


def _table_bin_of(n_stft, stride, rng):
    """a slot order in the row family's manner: every bin once, some twice, padding positions in between"""
    bins = np.concatenate([rng.permutation(n_stft), rng.integers(0, n_stft, stride - n_stft - 7)])
    binof = np.full(stride, -1, np.int64)
    binof[rng.permutation(stride)[:len(bins)]] = bins
    return binof


def _masks(n_stft, B, T, rng):
    """(B, n_stft, T) bool: random rows, and rows whose edges are off word boundaries"""
    held = rng.random((B, n_stft, T)) < 0.5
    held[0] = False
    held[1] = True
    held[2] = False
    held[2, 31] = True
    held[2, 33] = True
    held[2, n_stft - 1] = True
    held[3] = True
    held[3, 32] = False
    held[3, n_stft - 1, ::2] = False
    return held


def _split(emu, layout, S, bits, binof, B, T, stride, n_stft, want_held):
    X = np.full_like(S, 123.0)
    table = np.ascontiguousarray(binof, np.int32)
    emu.emu_holdmask_split(layout, S.ctypes.data, X.ctypes.data, bits.ctypes.data, table.ctypes.data, B, T, stride, n_stft, int(want_held))
    return X


@pytest.mark.parametrize("layout,n_stft,stride", [(SPEC, 8821, 9408), (PLAIN, 505, 508), (TABLE, 505, 600)], ids=["specialised", "plain", "table"])
def test_split_matches_numpy(emu, layout, n_stft, stride):
    rng = np.random.default_rng(3)
    B, T = 5, 3
    valid = n_stft - 32 * (emu.emu_holdmask_words(n_stft) - 1)
    assert valid == {8821: 21, 505: 25}[n_stft]
    binof = _spec_bin_of() if layout == SPEC else _table_bin_of(n_stft, stride, rng) if layout == TABLE else \
        np.where(np.arange(stride) < n_stft, np.arange(stride), -1)
    if layout == SPEC:
        assert emu.emu_holdmask_spec_stride() == stride and (np.bincount(binof[binof >= 0], minlength=n_stft) >= 1).all()
        assert int((np.bincount(binof[binof >= 0], minlength=n_stft) == 2).sum()) == 440  # the bins the layout stores twice
    table = np.ascontiguousarray(binof, np.int32)
    got_map = np.array([emu.emu_holdmask_slot_bin(layout, p, n_stft, table.ctypes.data) for p in range(stride)])
    assert np.array_equal(got_map, binof)
    held = _masks(n_stft, B, T, rng)
    bits = mask_oracle.pack_bits(held)
    assert np.array_equal(mask_oracle.unpack_bits(bits, n_stft), held)
    S = (rng.random((B * T, stride)) * 1000 + 1).astype(np.float32)  # nonzero everywhere, padding included
    frames = held.transpose(0, 2, 1).reshape(B * T, n_stft)  # [frame][bin]
    at = np.where(binof >= 0, binof, 0)
    pos_held = frames[:, at] & (binof >= 0)
    pos_free = ~frames[:, at] & (binof >= 0)
    x_held = _split(emu, layout, S, bits, binof, B, T, stride, n_stft, True)
    x_free = _split(emu, layout, S, bits, binof, B, T, stride, n_stft, False)
    assert np.array_equal(x_held, np.where(pos_held, S, np.float32(0)))
    assert np.array_equal(x_free, np.where(pos_free, S, np.float32(0)))
    assert np.array_equal((x_held + x_free)[:, binof >= 0], S[:, binof >= 0]) and not (x_held + x_free)[:, binof < 0].any()
    # bits set past n_stft change nothing
    dirty = bits.copy()
    dirty[:, :, -1] |= np.uint32((0xFFFFFFFF << valid) & 0xFFFFFFFF).astype(np.int32)
    assert not np.array_equal(dirty, bits)
    assert np.array_equal(_split(emu, layout, S, dirty, binof, B, T, stride, n_stft, True), x_held)
    assert np.array_equal(_split(emu, layout, S, dirty, binof, B, T, stride, n_stft, False), x_free)


# ---- band to bin ----------------------------------------------------------------------------------------------------------------------------

def _bank(**kw):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams(**kw)
    n_stft = p.n_fft // 2 + 1
    fb = _hip.mel_filterbank(n_stft, float(p.min_frequency), float(p.max_frequency), p.num_frequencies, p.sample_rate, p.mel_scale_norm, p.mel_scale_type)
    cp = _hip.RfxParams(p.sample_rate, p.n_fft, p.win_length, p.hop_length, p.num_frequencies, p.max_mel_iters)
    return p, cp, fb.to(torch.float32).contiguous(), n_stft


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=11025, max_frequency=5512)], ids=["default", "generic-11025"])
def test_bin_bands_and_their_expansion(emu, kw):
    from riffusion import _hip

    p, cp, fb, n_stft = _bank(**kw)
    lo, hi = _hip.bin_bands(cp, fb)
    want_lo, want_hi = mask_oracle.bin_bands(fb.numpy())
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    has = lo >= 0
    assert has.any() and (lo[has] <= hi[has]).all() and (hi[~has] == -1).all() and int(hi.max()) == p.num_frequencies - 1
    freqs = np.arange(n_stft) * (p.sample_rate / 2) / (n_stft - 1)
    assert not has[freqs > p.max_frequency].any()  # no filter reaches a bin above max_frequency
    if not kw:
        assert (freqs > p.max_frequency).any()
    # the expansion of a contiguous held band range [m0, m1] holds exactly the bins whose [lo, hi] lies inside it
    M, T = p.num_frequencies, 4
    bands = np.zeros((3, M, T), dtype=np.uint8)
    m0, m1 = M // 4, 2 * M // 3
    bands[0, m0:m1 + 1, :] = 1
    bands[1, :, 1] = 255  # one frame entirely
    bands[2] = 1
    bands[2, M // 2, 2] = 0  # one band free at one frame
    out = np.full((3, T, (n_stft + 31) // 32), 0x5A5A5A5A, np.uint32)
    emu.emu_holdmask_bands(bands.ctypes.data, lo.ctypes.data, hi.ctypes.data, out.ctypes.data, 3, M, T, n_stft)
    got = mask_oracle.unpack_bits(out.view(np.int32), n_stft)
    inside = has & (lo >= m0) & (hi <= m1)
    assert inside.any() and np.array_equal(got[0], np.repeat(inside[:, None], T, axis=1))
    assert np.array_equal(got[1][:, 1], has) and not got[1][:, [0, 2, 3]].any()
    touched = has & (lo <= M // 2) & (hi >= M // 2)
    assert np.array_equal(got[2][:, 2], has & ~touched) and np.array_equal(got[2][:, 0], has)
    assert np.array_equal(got, mask_oracle.bins_from_bands(bands, lo, hi))
    assert np.array_equal(out.view(np.int32), mask_oracle.pack_bits(got))  # every bit written, the unused tail bits 0


def test_bin_bands_refusals(lib):
    from riffusion import _hip

    cp = _hip.RfxParams(44100, 17640, 4410, 441, 512, 200)
    assert lib.rfx_debug_bin_bands(ctypes.byref(cp), None, None, None) == -1 and b"null argument" in lib.rfx_last_error()
    assert lib.rfx_hold_mask_words(None) == 0
    assert lib.rfx_hold_bins_from_bands(None, None, 1, 1, None, None) == -1 and b"null argument" in lib.rfx_last_error()


# ---- rfx_masked_call_options: layout and the refusals that need no device --------------------------------------------------------------------

def test_masked_options_layout_matches_the_header(repo_root, tmp_path):
    from riffusion import _hip

    exe = emu_build.header_compiles_as_c99(
        tmp_path,
        '#include <stddef.h>\n#include <stdio.h>\n#include "rfx.h"\n'
        "#define O(f) (int)offsetof(rfx_masked_call_options, f)\n"
        "int main(void) {\n"
        '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(rfx_held_call_options), (int)sizeof(rfx_masked_call_options), O(flags),\n'
        "         O(row_base), O(magnitude_hint), O(reserved), O(d_guide), O(guide_stride), O(guide_samples), O(reserved2), O(d_hold_frames), O(reserved3),\n"
        "         O(d_hold_bins), O(hold_words), O(reserved4));\n"
        "  return 0;\n}\n",
        link=True, extra=("-Wextra",))
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M, H = _hip.RfxMaskedCallOptions, _hip.RfxHeldCallOptions
    assert got[:2] == [ctypes.sizeof(H), ctypes.sizeof(M)] == [64, 80]
    assert got[2:] == [getattr(M, f).offset for f, _ in M._fields_[1:]]
    assert [getattr(M, f).offset for f, _ in H._fields_] == [getattr(H, f).offset for f, _ in H._fields_]  # the held-size prefix is the held struct
    assert (M.d_hold_bins.offset, M.hold_words.offset, M.reserved4.offset) == (64, 72, 76)


def test_masked_options_builder():
    from riffusion import _hip

    g = torch.zeros(3, 50)
    pairs = torch.zeros(3, 2, dtype=torch.int32)
    bits = torch.zeros(3, 33, 276, dtype=torch.int32)
    assert isinstance(_hip.call_options(rows=3, row_base=2), _hip.RfxCallOptions)
    assert isinstance(_hip.call_options(guide=g, rows=3), _hip.RfxGuidedCallOptions)
    assert isinstance(_hip.call_options(guide=g, hold=pairs, rows=3), _hip.RfxHeldCallOptions)
    o = _hip.call_options(guide=g[:, :40], hold_bins=bits, rows=3, row_base=2, magnitude_hint=5.0, lstsq=True)
    assert (o.struct_size, o.flags, o.row_base, o.magnitude_hint) == (80, 1, 2, 5.0)
    assert (o.d_guide, o.guide_stride, o.guide_samples, o.reserved2, o.d_hold_frames, o.reserved3) == (g.data_ptr(), 50, 40, 0, None, 0)
    assert (o.d_hold_bins, o.hold_words, o.reserved4) == (bits.data_ptr(), 276, 0)
    with pytest.raises(ValueError, match="needs a guide"):
        _hip.call_options(hold_bins=bits, rows=3)
    with pytest.raises(ValueError, match="together with hold"):
        _hip.call_options(guide=g, hold=pairs, hold_bins=bits, rows=3)
    for bad in (bits[:2], bits.long(), bits[:, :, ::2], bits[0], bits.float()):
        with pytest.raises(ValueError):
            _hip.call_options(guide=g, hold_bins=bad, rows=3)


def _masked(d_guide=0x1000, d_pairs=None, d_bins=0x3000, hold_words=276, reserved4=0, size=None):
    from riffusion import _hip

    return _hip.RfxMaskedCallOptions(ctypes.sizeof(_hip.RfxMaskedCallOptions) if size is None else size, 0, 0, 0.0, 0.0, d_guide, 100, 100, 0, d_pairs,
                                     0, d_bins, hold_words, reserved4)


def _gl_ex(lib, opt):
    return lib.rfx_griffinlim_ex(None, None, None, 0, 1, 30, 0, 0.5, None, None, 0, None, ctypes.byref(opt), None)


@pytest.mark.parametrize("kw,word", [(dict(d_guide=None), b"needs a guide"), (dict(d_bins=0x3002), b"aligned"), (dict(reserved4=1), b"reserved4"),
                                     (dict(reserved4=1, d_bins=None), b"reserved4"), (dict(d_pairs=0x2000), b"d_hold_frames")])
def test_masked_options_are_refused_before_any_device_work(lib, kw, word):
    """the options are read before the plan and the buffers are looked at: null everything else, no GPU needed"""
    opt = _masked(**kw)
    assert _gl_ex(lib, opt) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_ex(None, None, 1, 30, 1, 0, 1, 0.5, None, None, 0, None, ctypes.byref(opt)) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_audio_from_image_u8_ex(None, None, 1, 30, 0, None, 0, 1, 0.5, 1, None, None, None, 0, None, ctypes.byref(opt)) == -1
    assert word in lib.rfx_last_error()
    assert helpers.queries_refuse(lib, opt, word)


def test_inverse_mel_refuses_a_mask_and_shorter_structs_ignore_the_tail(lib):
    opt = _masked(d_guide=None)
    assert lib.rfx_inverse_mel_ex(None, None, 1, 1, 1, None, 0, None, None, 0, None, ctypes.byref(opt)) == -1 and b"holds no bins" in lib.rfx_last_error()
    # a valid masked struct passes the options and fails on the null plan; the three shorter sizes ignore the tail
    assert _gl_ex(lib, _masked()) == -1 and b"null argument" in lib.rfx_last_error()
    for size in (24, 48, 64):
        assert _gl_ex(lib, _masked(reserved4=1, d_bins=0x3002, size=size)) == -1 and b"null argument" in lib.rfx_last_error(), size
    # the workspace queries answer 0 for a masked call without a plan, like their drivers' own
    assert helpers.need(lib, "griffinlim", None, 3, 33, **helpers.MASKED) == 0 == helpers.need(lib, "waveform_from_mel", None, 3, 33, **helpers.MASKED)
    assert helpers.need(lib, "audio_from_image", None, 3, 0, 33, **helpers.MASKED) == 0


def test_cli_hold_mask_needs_a_guide_and_excludes_the_span_flags(capsys):
    from riffusion import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["image-to-audio", "--image", "x.png", "--audio", "y.wav", "--hold-mask", "m.png"])
    assert e.value.code == 2 and "--guide-audio" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["image-to-audio", "--image", "x.png", "--audio", "y.wav", "--guide-audio", "g.wav", "--hold-mask", "m.png", "--hold-head-ms", "100"])
    assert e.value.code == 2 and "--hold-head-ms" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["image-to-audio", "--image", "x.png", "--audio", "y.wav", "--guide-audio", "g.wav", "--hold-mask", "m.png", "--hold-keep-threshold", "1.5"])
    assert e.value.code == 2 and "--hold-keep-threshold" in capsys.readouterr().err


def test_hold_mask_rows_takes_one_mask_or_one_per_entry():
    from riffusion.spectrogram_converter import hold_mask_rows

    one = np.zeros((4, 6), dtype=bool)
    one[1, 2] = True
    rows = hold_mask_rows(one, 3, 4, 6)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (3, 4, 6) and rows.sum() == 3 and bool(rows[:, 1, 2].all())
    per = np.stack([one, ~one, one]).astype(np.float32) * 0.25  # nonzero = held
    assert torch.equal(hold_mask_rows(torch.from_numpy(per), 3, 4, 6), torch.from_numpy(np.stack([one, ~one, one]).astype(np.uint8)))
    for bad in (one[:3], one[:, :5], per[:2], np.zeros((3, 4, 6, 1))):
        with pytest.raises(ValueError):
            hold_mask_rows(bad, 3, 4, 6)


# ---- the mask of an image ------------------------------------------------------------------------------------------------------------------

def test_hold_mask_from_image_on_the_reference_masks(golden_dir):
    from PIL import Image

    from riffusion.util import image_util

    gradient = Image.open(os.path.join(golden_dir, "mask_gradient_dark.png"))
    lines = Image.open(os.path.join(golden_dir, "mask_beat_lines_80.png"))
    assert gradient.size == lines.size == (512, 512)
    held = image_util.hold_mask_from_image(gradient)
    assert held.dtype == bool and held.shape == (512, 512)
    assert (held == held[:, :1]).all()  # rows constant: a frequency mask
    assert held.sum() == 157 * 512 and abs(held.mean() - 0.307) < 5e-4  # 30.7 % of the pixels at the default threshold
    # Y is flipped as spectrogram_from_image does: the image's dark rows are its top ones, the highest bands
    lum = np.asarray(gradient.convert("L"))
    assert np.array_equal(held, (1.0 - lum[::-1] / 255.0) >= 0.5) and held[-1].all() and not held[0].any()
    assert image_util.hold_mask_from_image(gradient, 0.0).all() and not image_util.hold_mask_from_image(gradient, 1.0).any()
    # the beat lines are light grey on white: nothing is kept at 0.5; at a threshold inside its histogram a strict, non-empty subset
    assert not image_util.hold_mask_from_image(lines).any()
    keep = 1.0 - np.asarray(lines.convert("L"), dtype=np.float64) / 255.0
    levels = np.unique(keep)
    threshold = float(levels[len(levels) // 2])
    some = image_util.hold_mask_from_image(lines, threshold)
    assert 0 < some.sum() < some.size and some.sum() == (keep >= threshold).sum()
    assert not (some == some[:, :1]).all()  # a time-frequency pattern, not a frequency mask
    with pytest.raises(ValueError):
        image_util.hold_mask_from_image(lines, 1.5)
