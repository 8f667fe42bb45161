"""
CPU checks of the phase-guided Griffin-Lim start (include/rfx.h: rfx_guided_call_options).

* The staging kernels (csrc/rfx_guide.hip): the arithmetic header csrc/rfx_guide_core.h is compiled for the host together with
  tests/emu/rfx_guide_emu.cpp, which walks the logical threads of both kernels, and checked against numpy byte for byte - every
  factor is a power of two, so the expected value is exact: the fitted sample times 2^(15 - k) for a row peak in [2^(k-1), 2^k),
  times 2^j where the kernels of the specialised engine multiply by row_scale[2 r] = 2^-j.
* The definition, on the oracle: starting Griffin-Lim from the phase of the clip a tile was made of beats the random start
  (spectral convergence against the magnitudes it inverts, 64 frames of golden clip 2 through the uint8 tile), and a silent guide
  gives silence.
* The layout of the grown options struct against the header, and the refusals that need no device.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import helpers
from engines import clip2_segment

EMU_SRC = "rfx_guide_emu.cpp"


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    lib.emu_guide_stage.argtypes = [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    lib.emu_guide_stage.restype = None
    return lib


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


def lpad_of(L):
    return -(-L // 64) * 64


def stage(emu, guide, L, row_scale=None, want_zero=True):
    """(staged rows (B, Lpad), the zeroed partner buffer or None); both start as NaN: every element must be written"""
    guide = np.ascontiguousarray(guide, np.float32)
    B, Lg = guide.shape
    Lpad = lpad_of(L)
    dst = np.full((B, Lpad), np.nan, np.float32)
    zero = np.full((B, Lpad), np.nan, np.float32) if want_zero else None
    rs = None if row_scale is None else np.ascontiguousarray(row_scale, np.float32)
    emu.emu_guide_stage(guide.ctypes.data, Lg, Lg, B, L, Lpad, rs.ctypes.data if rs is not None else None, dst.ctypes.data,
                        zero.ctypes.data if zero is not None else None)
    return dst, zero


def expected(guide, L, j=None):
    """numpy's statement of the staging: exact, every factor being a power of two (float64 holds the products)"""
    guide = np.asarray(guide, np.float32)
    B, Lg = guide.shape
    out = np.zeros((B, lpad_of(L)), np.float64)
    n = min(Lg, L)
    out[:, :n] = guide[:, :n]
    for r in range(B):
        peak = np.abs(out[r]).max()
        if peak > 0:
            k = int(np.frexp(np.float32(peak))[1])
            out[r] = np.ldexp(out[r], 15 - k + (0 if j is None else int(j[r])))
    res = out.astype(np.float32)
    assert np.array_equal(res.astype(np.float64), out)  # nothing was rounded
    return res


def gl_exponent(lib, max_value):
    e, j = ctypes.c_int(), ctypes.c_int()
    assert lib.rfx_debug_range_exponents(max_value, 0, ctypes.byref(e), ctypes.byref(j)) == 0
    return j.value


def same_bytes(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---- the staging kernels' emulator against numpy ------------------------------------------------------------------------------------

L_FIT = 2 * 4096 + 700  # three chunks, the last one partial; Lpad = 8896 > L


@pytest.mark.parametrize("Lg", [1, 5, L_FIT - 100, L_FIT, L_FIT + 100, 4096, 4097])
def test_guide_fit_cuts_or_zero_pads_to_the_output_length(emu, Lg):
    rng = np.random.default_rng(Lg)
    guide = (rng.standard_normal((3, Lg)) * 8000).astype(np.float32)
    dst, zero = stage(emu, guide, L_FIT)
    want = expected(guide, L_FIT)
    assert same_bytes(dst, want)
    assert not dst[:, min(Lg, L_FIT):].any() and np.abs(dst[:, :min(Lg, L_FIT)]).max() >= 2.0 ** 14
    assert same_bytes(zero, np.zeros_like(zero))
    # the peak is the fitted row's: samples behind L do not count
    if Lg > L_FIT:
        loud = guide.copy()
        loud[:, L_FIT:] *= 1e6
        assert same_bytes(stage(emu, loud, L_FIT)[0], dst)


@pytest.mark.parametrize("peak", [1e-30, 1.0, 32767.0, 1e30])
def test_guide_peak_lands_between_two_to_the_14_and_15(emu, peak):
    rng = np.random.default_rng(11)
    guide = rng.uniform(-1, 1, (2, 5000)).astype(np.float32)
    guide[0, 1234] = 1.0
    guide[1, 4999] = -1.0
    guide = (guide.astype(np.float64) * peak).astype(np.float32)
    dst, _ = stage(emu, guide, 5000, want_zero=False)
    assert same_bytes(dst, expected(guide, 5000))
    top = np.abs(dst).max(axis=1)
    assert ((top >= 2.0 ** 14) & (top < 2.0 ** 15)).all()


@pytest.mark.parametrize("max_value", [1e-6, 30e6, 1e20])
@pytest.mark.parametrize("peak", [1e-30, 32767.0, 1e30])
def test_guide_times_the_row_factor_is_the_ranged_guide(emu, lib, max_value, peak):
    """the specialised engine's kernels multiply what they load by row_scale[2 r] = 2^-j: the stored value accounts for it"""
    j = gl_exponent(lib, max_value)
    rng = np.random.default_rng(5)
    guide = (rng.uniform(-1, 1, (2, 3000)) * peak).astype(np.float32)
    table = np.array([[2.0 ** -j, 1e-32], [2.0 ** -j, 1e-32]], np.float32)
    dst, _ = stage(emu, guide, 3000, row_scale=table, want_zero=False)
    assert same_bytes(dst, expected(guide, 3000, j=[j, j]))
    analysed = dst * np.float32(2.0 ** -j)  # what MODE 1 analyses
    assert np.isfinite(dst).all() and np.isfinite(analysed).all()
    assert same_bytes(analysed, stage(emu, guide, 3000, want_zero=False)[0])
    top = np.abs(analysed).max(axis=1)
    assert ((top >= 2.0 ** 14) & (top < 2.0 ** 15)).all() and (np.abs(dst).max(axis=1) > 0).all()


def test_guide_times_a_power_of_two_stages_the_same_bytes(emu):
    rng = np.random.default_rng(3)
    guide = (rng.standard_normal((2, 6001)) * 8000).astype(np.float32)
    base, _ = stage(emu, guide, 6001, want_zero=False)
    for n in (5, -7):
        assert same_bytes(stage(emu, np.ldexp(guide, n), 6001, want_zero=False)[0], base)


def test_silent_guide_row_stages_zeros(emu):
    rng = np.random.default_rng(4)
    guide = (rng.standard_normal((3, 5000)) * 100).astype(np.float32)
    guide[1] = 0.0
    table = np.array([[2.0 ** 7, 1e-32]] * 3, np.float32)
    for rs in (None, table):
        dst, zero = stage(emu, guide, 4800, row_scale=rs)
        assert not np.isnan(dst).any() and not dst[1].any() and dst[0].any() and dst[2].any()
        assert same_bytes(zero, np.zeros_like(zero))


def test_a_staged_row_does_not_depend_on_its_batch(emu):
    rng = np.random.default_rng(6)
    guide = (rng.standard_normal((4, 9000)) * np.array([[1e-3], [1.0], [3e4], [1e9]])).astype(np.float32)
    whole, _ = stage(emu, guide, 8800, want_zero=False)
    for r in range(4):
        assert same_bytes(stage(emu, guide[r:r + 1], 8800, want_zero=False)[0][0], whole[r])


# ---- the definition, on the oracle ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clip2(golden_dir):
    return clip2_segment(golden_dir)


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_oracle_guided_start_beats_the_random_start(clip2, stereo):
    """waveform -> mel -> uint8 tile -> mel -> SGD magnitudes; Griffin-Lim (4) from the clip's phase against Griffin-Lim (4) from
    torch.rand, both scored against the magnitudes they invert.  The oracle measured 0.036 against 0.24 - 0.25."""
    O, op, wav = clip2
    x = wav if stereo else wav.mean(dim=0, keepdim=True)
    mel = O.mel_amplitudes_from_waveform(x, op)
    tile = O.image_u8_from_spectrogram(mel.numpy(), op.power_for_image)
    back = torch.from_numpy(O.spectrogram_from_image_u8(tile, op.power_for_image, stereo=stereo).copy())
    gen = torch.Generator().manual_seed(1)
    lin = O.inverse_mel_scale_sgd(back, op, generator=gen)
    G = O.stft_complex(x, op)
    assert G.shape == lin.shape
    guided = O.griffinlim(lin, op, angles0=G / (G.abs() + 1e-16), n_iter=4)
    random = O.griffinlim(lin, op, generator=gen, n_iter=4)
    sc_guided, sc_random = O.spectral_convergence(guided, lin, op), O.spectral_convergence(random, lin, op)
    print(f"spectral convergence at n_iter = 4 ({'stereo' if stereo else 'mono'}): guided {sc_guided:.4f}, random {sc_random:.4f}")
    assert sc_guided < 0.5 * sc_random
    silent = torch.zeros_like(G)
    out = O.griffinlim(lin, op, angles0=silent / (silent.abs() + 1e-16), n_iter=4)
    assert float(out.abs().max()) == 0.0


# ---- rfx_guided_call_options: layout and the refusals that need no device ----------------------------------------------------------------

def test_guided_options_layout_matches_the_header(repo_root, tmp_path):
    from riffusion import _hip

    exe = emu_build.header_compiles_as_c99(
        tmp_path,
        '#include <stddef.h>\n#include <stdio.h>\n#include "rfx.h"\n'
        "#define O(f) (int)offsetof(rfx_guided_call_options, f)\n"
        "int main(void) {\n"
        '  printf("%d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(rfx_call_options), (int)sizeof(rfx_guided_call_options), O(flags), O(row_base),\n'
        "         O(magnitude_hint), O(reserved), O(d_guide), O(guide_stride), O(guide_samples), O(reserved2), rfx_version());\n"
        "  return 0;\n}\n",
        link=True, extra=("-Wextra",))
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G, S = _hip.RfxGuidedCallOptions, _hip.RfxCallOptions
    assert got[:2] == [ctypes.sizeof(S), ctypes.sizeof(G)] == [24, 48]
    assert got[2:10] == [G.flags.offset, G.row_base.offset, G.magnitude_hint.offset, G.reserved.offset, G.d_guide.offset,
                         G.guide_stride.offset, G.guide_samples.offset, G.reserved2.offset]
    # the old-size prefix is the old struct
    assert [G.flags.offset, G.row_base.offset, G.magnitude_hint.offset] == [S.flags.offset, S.row_base.offset, S.magnitude_hint.offset] == [4, 8, 16]
    assert got[10] == 2 and _hip.load_library().rfx_version() == 2


def test_guided_options_builder():
    from riffusion import _hip

    assert isinstance(_hip.call_options(rows=3, row_base=2), _hip.RfxCallOptions)
    g = torch.zeros(3, 50)
    o = _hip.call_options(guide=g[:, :40], rows=3, row_base=2, magnitude_hint=5.0, lstsq=True)
    assert (o.struct_size, o.flags, o.row_base, o.magnitude_hint) == (48, 1, 2, 5.0)
    assert (o.d_guide, o.guide_stride, o.guide_samples, o.reserved2) == (g.data_ptr(), 50, 40, 0)
    for bad in (g[:2], g.double(), g[:, ::2], g[0]):
        with pytest.raises(ValueError):
            _hip.call_options(guide=bad, rows=3)


def _guided(d_guide=0x1000, stride=100, samples=100, reserved=0.0, reserved2=0, size=None):
    from riffusion import _hip

    return _hip.RfxGuidedCallOptions(ctypes.sizeof(_hip.RfxGuidedCallOptions) if size is None else size, 0, 0, 0.0, reserved, d_guide, stride,
                                     samples, reserved2)


def _gl_ex(lib, opt):
    return lib.rfx_griffinlim_ex(None, None, None, 0, 1, 30, 0, 0.5, None, None, 0, None, ctypes.byref(opt), None)


@pytest.mark.parametrize("kw,word", [(dict(samples=0), b"guide_samples"), (dict(samples=-3), b"guide_samples"), (dict(stride=99), b"guide_stride"),
                                     (dict(d_guide=0x1002), b"aligned"), (dict(reserved=1.0), b"reserved"), (dict(reserved2=1), b"reserved2"),
                                     (dict(reserved=float("nan")), b"reserved")])
def test_guided_options_are_refused_before_any_device_work(lib, kw, word):
    """the options are read before the plan and the buffers are looked at: null everything else, no GPU needed"""
    opt = _guided(**kw)
    assert _gl_ex(lib, opt) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_ex(None, None, 1, 30, 1, 0, 1, 0.5, None, None, 0, None, ctypes.byref(opt)) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_audio_from_image_u8_ex(None, None, 1, 30, 0, None, 0, 1, 0.5, 1, None, None, None, 0, None, ctypes.byref(opt)) == -1
    assert word in lib.rfx_last_error()
    assert helpers.queries_refuse(lib, opt, word)


def test_inverse_mel_refuses_a_guide_and_reserved_is_checked_on_the_short_struct(lib):
    from riffusion import _hip

    opt = _guided()
    assert lib.rfx_inverse_mel_ex(None, None, 1, 1, 1, None, 0, None, None, 0, None, ctypes.byref(opt)) == -1 and b"takes no guide" in lib.rfx_last_error()
    short = _hip.RfxCallOptions(24, 0, 0, 0.0, 1.0)
    assert _gl_ex(lib, short) == -1 and b"reserved must be 0" in lib.rfx_last_error()
    # a valid guided struct passes the options and fails on the null plan; the old size ignores the tail
    assert _gl_ex(lib, _guided()) == -1 and b"null argument" in lib.rfx_last_error()
    assert _gl_ex(lib, _guided(samples=0, size=24)) == -1 and b"null argument" in lib.rfx_last_error()
