"""
CPU checks of loop calls (include/rfx.h: rfx_loop_call_options): a tile's T columns are the STFT of a signal with period hop T, and
the decode's end runs into its start.

* The index rules, the folds and the envelope of csrc/rfx_loop_core.h, compiled for the host with tests/emu/rfx_loop_emu.cpp, against
  tests/loop_oracle.py in float32: the default geometry at T = 40 (period == n_fft: every frame wraps) and T = 49, 11.025 kHz at
  T = 41, and one odd n_fft.  Every frame's gathered index set is exact; the envelope table equals the float32 fma chain bit for bit;
  the folded audio of random frames is within float32 rounding of a float64 fold; all P samples are written and none beyond.
  The bound of the fold: a chain of n <= ceil(win / hop) terms carries at most n u sum |w y| (u = 2^-24; one more u per term where the
  frames were windowed in float32 before the fold), the float32 envelope n u relative, its reciprocal and the product one u each:
  (2 n + 4) u sum |w y| / env.
* Rolling the frames by k rolls the folded audio by k hop, bit for bit.
* The oracle itself in float64: the circular pair reconstructs, is roll-equivariant, and its envelope is constant to 1e-6.
* The layout of the grown options struct against the header, the shorter sizes, every refusal that needs no device, the CLI flags.
"""
import ctypes
import os
import subprocess
import types
import wave

import numpy as np
import pytest
import torch

import emu_build
import helpers
import loop_oracle

EMU_SRC = "rfx_loop_emu.cpp"
U = 2.0 ** -24

# (n_fft, win, hop, T)
GEOMETRIES = [(17640, 4410, 441, 40), (17640, 4410, 441, 49), (4410, 1102, 110, 41), (1001, 251, 26, 39)]
IDS = ["default-T40", "default-T49", "11025-T41", "odd-nfft-T39"]


@pytest.fixture(scope="module")
def O():
    import riffusion_oracle

    return riffusion_oracle


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_loop_gather.argtypes = [i, i, i, i, i, vp]
    lib.emu_loop_gather_blocks.argtypes = [i, i, i, vp]
    lib.emu_loop_env.argtypes = [vp, i, i, i, vp]
    lib.emu_loop_renv.argtypes = [vp, i, i, i, ctypes.c_float, vp]
    lib.emu_loop_fold_sum.argtypes = [vp, i, i, vp, i, i, i, i, vp]
    lib.emu_loop_fold_fma.argtypes = [vp, i, vp, vp, i, i, i, i, vp]
    for f in (lib.emu_loop_gather, lib.emu_loop_gather_blocks, lib.emu_loop_env, lib.emu_loop_renv, lib.emu_loop_fold_sum, lib.emu_loop_fold_fma):
        f.restype = None
    return lib


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


def _geo(n_fft, win, hop):
    return types.SimpleNamespace(n_fft=n_fft, win_length=win, hop_length=hop)


def _window(O, g):
    return np.ascontiguousarray(O.hann_window(g).numpy())


# ---- the emulator against the oracle --------------------------------------------------------------------------------------------------------

def test_validity_rule(emu):
    assert emu.emu_loop_min_frames(441, 17640) == 40 and emu.emu_loop_min_frames(110, 4410) == 41 and emu.emu_loop_min_frames(26, 1001) == 39
    assert emu.emu_loop_valid(441, 40, 17640) == 1 and emu.emu_loop_valid(441, 39, 17640) == 0
    assert emu.emu_loop_valid(110, 41, 4410) == 1 and emu.emu_loop_valid(110, 40, 4410) == 0
    for P in (1, 7, 17640):
        assert [emu.emu_loop_wrap(p, P) for p in (-P, -1, 0, P - 1, P, 2 * P - 1)] == [0, P - 1, 0, P - 1, 0, P - 1]


@pytest.mark.parametrize("n_fft,win,hop,T", GEOMETRIES, ids=IDS)
def test_gathered_index_set_of_every_frame_is_exact(emu, n_fft, win, hop, T):
    g = _geo(n_fft, win, hop)
    left = (n_fft - win) // 2
    want = loop_oracle._scatter_index(g, T).numpy()[left:left + win]  # (win, T)
    assert want.min() == 0 and want.max() == hop * T - 1
    for t in range(T):
        idx = np.full(win + 8, -77, np.int32)
        emu.emu_loop_gather(n_fft, win, hop, T, t, idx.ctypes.data)
        assert np.array_equal(idx[:win], want[:, t]) and (idx[win:] == -77).all(), t
        if win == 10 * hop and n_fft // 2 - left == 5 * hop:  # the specialised kernel's block form of the same rule
            blk = np.full(win + 8, -77, np.int32)
            emu.emu_loop_gather_blocks(hop, T, t, blk.ctypes.data)
            assert np.array_equal(blk, idx), t
    if hop * T == n_fft:  # period == n_fft: every padded frame covers the period exactly once, wrapping at the loop point
        full = loop_oracle._scatter_index(g, T).numpy()
        assert all(np.array_equal(np.sort(full[:, t]), np.arange(n_fft)) for t in range(T))
    assert any((np.diff(want[:, t]) < 0).any() for t in range(T))  # some window reaches across the loop point


@pytest.mark.parametrize("n_fft,win,hop,T", GEOMETRIES, ids=IDS)
def test_envelope_table_is_the_float32_fma_chain(O, emu, n_fft, win, hop, T):
    w = _window(O, _geo(n_fft, win, hop))
    env = np.full(hop + 8, np.float32(-5), np.float32)
    emu.emu_loop_env(w.ctypes.data, n_fft, win, hop, env.ctypes.data)
    want = loop_oracle.env_table_f32(w, n_fft, hop)
    assert np.array_equal(env[:hop].view(np.uint32), want.view(np.uint32)) and (env[hop:] == -5).all()
    # ... and is the oracle's circular envelope, sample m at entry m mod hop
    full = loop_oracle.loop_env(O, _geo(n_fft, win, hop), T, torch.float64).numpy()
    assert np.allclose(np.tile(env[:hop], T), full, rtol=16 * U, atol=0)
    renv = np.zeros(hop, np.float32)
    emu.emu_loop_renv(w.ctypes.data, n_fft, win, hop, ctypes.c_float(2.0 / n_fft), renv.ctypes.data)
    assert np.array_equal(renv, np.float32(2.0 / n_fft) / env[:hop])


def _fold(emu, kind, frames, w, renv, n_fft, win, hop, T, pitch, shift):
    """the emulator's fold of (T, win) frames laid out [T][pitch] at `shift`, into a sentinel-filled buffer: (out (P,), guard)"""
    P = hop * T
    rows = np.zeros((T, pitch), np.float32)
    out = np.full(P + 64, np.float32(np.nan), np.float32)
    if kind == "fma":
        assert shift == 0
        rows[:, :win] = frames
        emu.emu_loop_fold_fma(rows.ctypes.data, pitch, w.ctypes.data, renv.ctypes.data, n_fft, win, hop, T, out.ctypes.data)
    else:
        rows[:, shift:shift + win] = frames * w  # windowed in float32, as the generic kernels store them
        emu.emu_loop_fold_sum(rows.ctypes.data, pitch, shift, renv.ctypes.data, n_fft, win, hop, T, out.ctypes.data)
    return out[:P], out[P:]


@pytest.mark.parametrize("kind", ["fma", "sum"])
@pytest.mark.parametrize("n_fft,win,hop,T", GEOMETRIES, ids=IDS)
def test_fold_matches_a_float64_fold_and_writes_exactly_the_period(O, emu, kind, n_fft, win, hop, T):
    rng = np.random.default_rng(5)
    w = _window(O, _geo(n_fft, win, hop))
    frames = rng.standard_normal((T, win)).astype(np.float32)
    renv = np.zeros(hop, np.float32)
    emu.emu_loop_renv(w.ctypes.data, n_fft, win, hop, ctypes.c_float(1.0), renv.ctypes.data)
    pitch, shift = (win + 6, 0) if kind == "fma" else (win + 7, 3)
    out, guard = _fold(emu, kind, frames, w, renv, n_fft, win, hop, T, pitch, shift)
    assert not np.isnan(out).any() and np.isnan(guard).all()  # all P samples written, none beyond
    num, mag, env = loop_oracle.fold_f64(frames, w, n_fft, hop)
    n = -(-win // hop)
    bound = (2 * n + 4) * U * mag / env
    err = np.abs(out.astype(np.float64) - num / env)
    print(f"{kind} fold, n_fft {n_fft} T {T}: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("kind", ["fma", "sum"])
@pytest.mark.parametrize("n_fft,win,hop,T", GEOMETRIES, ids=IDS)
def test_rolled_frames_fold_to_rolled_audio_bit_for_bit(O, emu, kind, n_fft, win, hop, T):
    rng = np.random.default_rng(6)
    w = _window(O, _geo(n_fft, win, hop))
    frames = rng.standard_normal((T, win)).astype(np.float32)
    renv = np.zeros(hop, np.float32)
    emu.emu_loop_renv(w.ctypes.data, n_fft, win, hop, ctypes.c_float(1.0), renv.ctypes.data)
    pitch, shift = (win, 0) if kind == "fma" else (win + 8, 4)
    base, _ = _fold(emu, kind, frames, w, renv, n_fft, win, hop, T, pitch, shift)
    for k in (1, 16, T - 1):
        rolled, _ = _fold(emu, kind, np.roll(frames, k, axis=0), w, renv, n_fft, win, hop, T, pitch, shift)
        assert np.array_equal(rolled.view(np.uint32), np.roll(base, k * hop).view(np.uint32)), k


# ---- the oracle itself, float64 ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def default_params(O):
    from riffusion.spectrogram_params import SpectrogramParams

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return O.params_from(SpectrogramParams())


@pytest.mark.parametrize("T", [40, 64])
def test_oracle_pair_reconstructs_and_is_roll_equivariant(O, default_params, T):
    p = default_params
    P = p.hop_length * T
    x = torch.randn(2, P, dtype=torch.float64, generator=torch.Generator().manual_seed(T))
    X = loop_oracle.loop_stft(O, x, p, torch.float64)
    assert tuple(X.shape) == (2, p.n_stft, T)
    back = loop_oracle.loop_istft(O, X, p, torch.float64)
    rel = float((back - x).norm() / x.norm())
    print(f"T = {T}: loop_istft(loop_stft(x)) against x: {rel:.2e} relative")
    assert tuple(back.shape) == (2, P) and rel <= 1e-12
    for k in (1, 16, T - 1):
        Xr = loop_oracle.loop_stft(O, torch.roll(x, k * p.hop_length, dims=-1), p, torch.float64)
        assert float((Xr - torch.roll(X, k, dims=-1)).norm() / X.norm()) <= 1e-12, k
        yr = loop_oracle.loop_istft(O, torch.roll(X, k, dims=-1), p, torch.float64)
        assert float((yr - torch.roll(back, k * p.hop_length, dims=-1)).norm() / back.norm()) <= 1e-12, k
    # the definition's own words: frame t, element i is x[(hop t + i - h) mod P] w[i]
    w = loop_oracle.padded_window(O, p, torch.float64)
    t = T - 1
    frame = x[0, (p.hop_length * t + torch.arange(p.n_fft) - p.n_fft // 2) % P] * w
    assert float((torch.fft.rfft(frame) - X[0, :, t]).abs().max()) <= 1e-9 * float(X.abs().max())


def test_oracle_envelope_is_constant_at_the_default_geometry(O, default_params):
    env = loop_oracle.loop_env(O, default_params, 40, torch.float64)
    lo, hi = float(env.min()), float(env.max())
    print(f"circular envelope of the float32 Hann window: {lo:.7f} .. {hi:.7f}")
    assert hi - lo <= 1e-6 and abs(lo - 3.75) <= 1e-6
    assert torch.equal(env, loop_oracle.loop_env(O, default_params, 40, torch.float64)[:441].repeat(40))


def test_loop_decode_has_an_ordinary_step_at_the_loop_point(O, default_params, golden_dir):
    """the issue's indication, one case: a 40-frame excerpt of golden clip 2 made loopable by a 50 ms crossfade, 8 iterations from one
    random start - the seam figure of the loop decode against the reflect decode of the same columns.  Figures printed; the direction
    asserted."""
    p = default_params
    T = 40
    P = p.hop_length * T
    with wave.open(os.path.join(golden_dir, "clip_2_start_103694_ms_duration_5678_ms.wav")) as wv:
        pcm = np.frombuffer(wv.readframes(wv.getnframes()), np.int16).reshape(-1, 2)
    fade = int(0.05 * p.sample_rate)
    seg = pcm[44100:44100 + P + fade].astype(np.float64).mean(axis=1)
    ramp = np.linspace(0.0, 1.0, fade)
    x = seg[:P].copy()
    x[:fade] = seg[P:P + fade] * (1 - ramp) + seg[:fade] * ramp  # the clip's end fades into its start
    S = loop_oracle.loop_stft(O, torch.from_numpy(x[None]), p, torch.float64).abs()
    a0 = torch.rand(S.shape, dtype=torch.complex128, generator=torch.Generator().manual_seed(1))
    looped = loop_oracle.loop_griffinlim(O, S, p, a0, 8, torch.float64)
    plain = O.griffinlim(S, p, angles0=a0, n_iter=8, dtype=torch.float64)
    assert tuple(looped.shape) == (1, P) and tuple(plain.shape) == (1, P - p.hop_length)
    fl, fp = float(loop_oracle.seam_figure(looped)[0]), float(loop_oracle.seam_figure(plain)[0])
    print(f"seam figure at 8 iterations: loop decode {fl:.2f}, reflect decode of the same columns {fp:.2f}")
    assert fl < fp


# ---- rfx_loop_call_options: layout and the refusals that need no device ----------------------------------------------------------------------

def test_loop_options_layout_matches_the_header(repo_root, tmp_path):
    from riffusion import _hip

    exe = emu_build.header_compiles_as_c99(
        tmp_path,
        '#include <stddef.h>\n#include <stdio.h>\n#include "rfx.h"\n'
        "#define O(f) (int)offsetof(rfx_loop_call_options, f)\n"
        "int main(void) {\n"
        '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(rfx_masked_call_options), (int)sizeof(rfx_loop_call_options), O(flags),\n'
        "         O(row_base), O(magnitude_hint), O(reserved), O(d_guide), O(guide_stride), O(guide_samples), O(reserved2), O(d_hold_frames), O(reserved3),\n"
        "         O(d_hold_bins), O(hold_words), O(reserved4), O(loop), O(reserved5));\n"
        "  return 0;\n}\n",
        link=True, extra=("-Wextra",))
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    Lp, M = _hip.RfxLoopCallOptions, _hip.RfxMaskedCallOptions
    assert got[:2] == [ctypes.sizeof(M), ctypes.sizeof(Lp)] == [80, 88]
    assert got[2:] == [getattr(Lp, f).offset for f, _ in Lp._fields_[1:]]
    assert [getattr(Lp, f).offset for f, _ in M._fields_] == [getattr(M, f).offset for f, _ in M._fields_]  # the masked-size prefix is the masked struct
    assert (Lp.loop.offset, Lp.reserved5.offset) == (80, 84)


def test_loop_options_builder():
    from riffusion import _hip

    g = torch.zeros(3, 50)
    pairs = torch.zeros(3, 2, dtype=torch.int32)
    bits = torch.zeros(3, 33, 276, dtype=torch.int32)
    assert isinstance(_hip.call_options(rows=3, row_base=2), _hip.RfxCallOptions)
    assert isinstance(_hip.call_options(guide=g, hold_bins=bits, rows=3), _hip.RfxMaskedCallOptions)
    o = _hip.call_options(rows=3, row_base=2, magnitude_hint=5.0, lstsq=True, loop=True)
    assert (o.struct_size, o.flags, o.row_base, o.magnitude_hint) == (88, 1, 2, 5.0)
    assert (o.d_guide, o.guide_stride, o.guide_samples, o.d_hold_frames, o.d_hold_bins, o.hold_words, o.loop, o.reserved5) == (None, 0, 0, None, None, 0, 1, 0)
    o = _hip.call_options(guide=g[:, :40], rows=3, loop=True)
    assert (o.d_guide, o.guide_stride, o.guide_samples, o.loop) == (g.data_ptr(), 50, 40, 1)
    for kw in (dict(hold=pairs), dict(hold_bins=bits)):
        with pytest.raises(ValueError, match="loop together with"):
            _hip.call_options(guide=g, rows=3, loop=True, **kw)


def _loop(loop=1, reserved5=0, d_guide=None, d_pairs=None, d_bins=None, size=None):
    from riffusion import _hip

    return _hip.RfxLoopCallOptions(ctypes.sizeof(_hip.RfxLoopCallOptions) if size is None else size, 0, 0, 0.0, 0.0, d_guide, 100 if d_guide else 0,
                                   100 if d_guide else 0, 0, d_pairs, 0, d_bins, 276 if d_bins else 0, 0, loop, reserved5)


def _gl_ex(lib, opt):
    return lib.rfx_griffinlim_ex(None, None, None, 0, 1, 41, 0, 0.5, None, None, 0, None, ctypes.byref(opt), None)


@pytest.mark.parametrize("kw,word", [(dict(loop=2), b"loop must be 0 or 1"), (dict(loop=0xFFFFFFFF), b"loop must be 0 or 1"), (dict(reserved5=1), b"reserved5"),
                                     (dict(loop=0, reserved5=7), b"reserved5"), (dict(d_guide=0x1000, d_pairs=0x2000), b"loop together with"),
                                     (dict(d_guide=0x1000, d_bins=0x3000), b"loop together with")])
def test_loop_options_are_refused_before_any_device_work(lib, kw, word):
    """the options are read before the plan and the buffers are looked at: null everything else, no GPU needed"""
    opt = _loop(**kw)
    assert _gl_ex(lib, opt) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_ex(None, None, 1, 41, 1, 0, 1, 0.5, None, None, 0, None, ctypes.byref(opt)) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_audio_from_image_u8_ex(None, None, 1, 41, 0, None, 0, 1, 0.5, 1, None, None, None, 0, None, ctypes.byref(opt)) == -1
    assert word in lib.rfx_last_error()
    assert helpers.queries_refuse(lib, opt, word)


def test_inverse_mel_refuses_a_loop_and_shorter_structs_ignore_the_tail(lib):
    assert lib.rfx_inverse_mel_ex(None, None, 1, 1, 1, None, 0, None, None, 0, None, ctypes.byref(_loop())) == -1 and b"decodes no loop" in lib.rfx_last_error()
    # a valid loop struct (plain, or with a guide) passes the options and fails on the null plan; so does loop = 0
    for opt in (_loop(), _loop(d_guide=0x1000), _loop(loop=0), _loop(loop=0, d_guide=0x1000, d_bins=0x3000)):
        assert _gl_ex(lib, opt) == -1 and b"null argument" in lib.rfx_last_error()
    # a masked-size caller (and the three shorter sizes) is unaffected by whatever lies behind its struct
    for size in (24, 48, 64, 80):
        assert _gl_ex(lib, _loop(loop=2, reserved5=9, size=size)) == -1 and b"null argument" in lib.rfx_last_error(), size
    # flags == 2 stays refused: the loop is not a flag bit
    from riffusion import _hip

    assert _gl_ex(lib, _hip.RfxCallOptions(24, 2, 0, 0.0, 0.0)) == -1 and b"flags" in lib.rfx_last_error()
    # the queries answer 0 for a loop call without a plan, like their drivers' own
    assert helpers.need(lib, "griffinlim", None, 3, 41, loop=1) == 0 == helpers.need(lib, "waveform_from_mel", None, 3, 41, loop=1)
    assert helpers.need(lib, "audio_from_image", None, 3, 0, 41, loop=1) == 0 == lib.rfx_griffinlim_loop_output_samples(None, 41)


@pytest.mark.parametrize("rate,n_fft,win,hop,need", [(44100, 17640, 4410, 441, 40), (11025, 4410, 1102, 110, 41)])
def test_too_few_frames_are_refused_with_the_smallest_count_in_the_message(lib, rate, n_fft, win, hop, need):
    from riffusion import _hip

    cp = _hip.RfxParams(rate, n_fft, win, hop, 512, 200)
    assert lib.rfx_debug_loop_frames(ctypes.byref(cp), need) == 0 == lib.rfx_debug_loop_frames(ctypes.byref(cp), 512)
    for T in (need - 1, 2, 0):
        assert lib.rfx_debug_loop_frames(ctypes.byref(cp), T) == -1
        msg = lib.rfx_last_error()
        assert b"hop_length * T >= n_fft" in msg and f"at least {need} frames, got {T}".encode() in msg
    assert lib.rfx_debug_loop_frames(None, 41) == -1
    assert _hip.loop_min_frames(hop, n_fft) == need
    _hip.check_loop_frames(hop, n_fft, need)
    with pytest.raises(ValueError, match=f"at least {need} frames, got {need - 1}"):
        _hip.check_loop_frames(hop, n_fft, need - 1)


def test_cli_loop_excludes_the_hold_flags(capsys):
    from riffusion import cli

    base = ["image-to-audio", "--image", "x.png", "--audio", "y.wav", "--loop"]
    for extra in (["--guide-audio", "g.wav", "--hold-mask", "m.png"], ["--guide-audio", "g.wav", "--hold-head-ms", "100"],
                  ["--guide-audio", "g.wav", "--hold-tail-ms", "100"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2 and "--loop does not go with" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--loop does not go with"):
        cli.image_to_audio(image="x.png", audio="y.wav", guide_audio="g.wav", hold_mask="m.png", loop=True)
    args = vars(cli.build_parser().parse_args(["images-to-audio-batch", "--image-dir", "a", "--output-dir", "b", "--loop"]))
    assert args["loop"] is True
    assert vars(cli.build_parser().parse_args(["images-to-audio-batch", "--image-dir", "a", "--output-dir", "b"]))["loop"] is False
