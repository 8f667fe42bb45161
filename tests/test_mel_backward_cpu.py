"""
CPU checks of the forward path's backward (include/rfx.h, "BACKWARD of the forward path"; csrc/rfx_mel_bwd_core.h).

* tests/emu/rfx_mel_bwd_emu.cpp runs the core's statement - the adjoint table's sum, the zero rule, the three taps of the fold - in
  double over four geometries (default, 48 kHz, 11.025 kHz, one odd n_fft) and three row lengths - n_fft // 2 + 1, where both reflect
  partners reach every sample; n_fft // 2 + hop + 3; hop * 40 + 17 - and must agree with float64 torch.autograd through the oracle's
  own forward (tests/mel_backward_oracle.py) to a relative L2 of 1e-10, for the fused path and for the complex STFT gradient.  The
  same statement in numpy measured 5e-14 .. 3e-16; the gate leaves three orders for the summation order at n_fft 19200 and sits
  far below any index mistake.  A silent row gives exact zeros, as torch's abs backward does.
* The adjoint table of rfx_debug_mel_adjoint reproduces fb @ g exactly in double for the default, the slaney-normalised, the
  slaney-scale and the 20 Hz - 20 kHz banks.
* The emulator and a `main` of its own are also built as a stand-alone program with -fsanitize=address,undefined and run: the adjoint
  defects it prints are the ones the unsanitized build returns.  Nothing sanitized is loaded into Python.
* include/rfx.h compiles as C99 with the new entries; the entries answer 0 or refuse without a plan.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import mel_backward_oracle as MBO
from helpers import oracle

EMU_SRC = "rfx_mel_bwd_emu.cpp"
EMU_MAIN = "rfx_mel_bwd_emu_main.cpp"

# OracleParams keywords of the four geometries of tests/test_loop_encode_cpu.py: (n_fft, win, hop) = (17640, 4410, 441),
# (19200, 4800, 480), (4410, 1102, 110), (1001, 251, 26); 64 bands keep the float64 reference quick
GEOMETRIES = {
    "default": dict(),
    "48k": dict(sample_rate=48000),
    "11025": dict(sample_rate=11025, max_frequency=5512),
    "odd-nfft": dict(sample_rate=10010, padded_duration_ms=100, window_duration_ms=25.1, step_size_ms=2.6, max_frequency=5000),
}
GEO_SIZES = {"default": (17640, 4410, 441), "48k": (19200, 4800, 480), "11025": (4410, 1102, 110), "odd-nfft": (1001, 251, 26)}
GATE = 1e-10


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_mel_bwd_frames.argtypes = [i, i, i, i]
    lib.emu_mel_from_waveform_backward.argtypes = [i, i, i, i, i, vp, vp, vp, vp, vp, vp, i, vp, vp]
    lib.emu_stft_backward.argtypes = [i, i, i, i, vp, vp, vp, vp]
    lib.emu_mel_adjoint_apply.argtypes = [i, vp, vp, vp, i, vp, vp]
    lib.emu_stft_adjoint_defect.argtypes = [i, i, i, i, ctypes.c_uint, vp]
    lib.emu_stft_adjoint_defect.restype = d
    return lib


def _adjoint_table(lib, op, fb):
    """rfx_debug_mel_adjoint: (first, count, weights [n_stft][width], width)"""
    from riffusion import _hip

    cp = _hip.RfxParams(op.sample_rate, op.n_fft, op.win_length, op.hop_length, op.num_frequencies, op.max_mel_iters)
    fb = fb.to(torch.float32).contiguous()
    width = ctypes.c_int32(0)
    _hip.check(lib.rfx_debug_mel_adjoint(ctypes.byref(cp), fb.data_ptr(), None, None, None, 0, ctypes.byref(width)))
    first, count = np.zeros(op.n_stft, np.int32), np.zeros(op.n_stft, np.int32)
    wt = np.zeros((op.n_stft, width.value), np.float32)
    _hip.check(lib.rfx_debug_mel_adjoint(ctypes.byref(cp), fb.data_ptr(), first.ctypes.data, count.ctypes.data, wt.ctypes.data, width.value,
                                         ctypes.byref(width)))
    return first, count, wt, width.value


def _rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _cases():
    for name, (n_fft, win, hop) in GEO_SIZES.items():
        for Lw in (n_fft // 2 + 1, n_fft // 2 + hop + 3, hop * 40 + 17):
            yield pytest.param(name, Lw, id=f"{name}-Lw{Lw}")


@pytest.mark.parametrize("name,Lw", list(_cases()))
def test_emulator_agrees_with_float64_autograd(O, lib, emu, name, Lw):
    op = O.OracleParams(num_frequencies=64, **GEOMETRIES[name])
    n_fft, win, hop = GEO_SIZES[name]
    assert (op.n_fft, op.win_length, op.hop_length) == (n_fft, win, hop)
    g = torch.Generator().manual_seed(Lw)
    wave = torch.randn(1, Lw, generator=g, dtype=torch.float64) * 8000
    X = MBO.stft(wave, op)[0]  # (n_stft, T) complex128
    Tn = X.shape[-1]
    assert emu.emu_mel_bwd_frames(n_fft, win, hop, Lw) == Tn
    window = O.hann_window(op).double().numpy()
    xre, xim = np.ascontiguousarray(X.real.numpy()), np.ascontiguousarray(X.imag.numpy())
    first, count, wt, width = _adjoint_table(lib, op, O.mel_filterbank(op))
    # the fused path
    g_mel = torch.randn(1, op.num_frequencies, Tn, generator=g, dtype=torch.float64)
    want = MBO.mel_from_waveform_grad(wave, g_mel, op)[0].numpy()
    gm, got = np.ascontiguousarray(g_mel[0].numpy()), np.full(Lw, 123.0)
    assert emu.emu_mel_from_waveform_backward(n_fft, win, hop, Lw, op.num_frequencies, window.ctypes.data, xre.ctypes.data, xim.ctypes.data,
                                              first.ctypes.data, count.ctypes.data, wt.ctypes.data, width, gm.ctypes.data, got.ctypes.data) == Tn
    fused = _rel_l2(got, want)
    # the complex gradient of the STFT alone
    g_spec = torch.complex(torch.randn(1, op.n_stft, Tn, generator=g, dtype=torch.float64), torch.randn(1, op.n_stft, Tn, generator=g, dtype=torch.float64))
    want_s = MBO.stft_grad(wave, g_spec, op)[0].numpy()
    gre, gim = np.ascontiguousarray(g_spec[0].real.numpy()), np.ascontiguousarray(g_spec[0].imag.numpy())
    got_s = np.full(Lw, 123.0)
    assert emu.emu_stft_backward(n_fft, win, hop, Lw, window.ctypes.data, gre.ctypes.data, gim.ctypes.data, got_s.ctypes.data) == Tn
    spec = _rel_l2(got_s, want_s)
    print(f"{name} Lw {Lw} T {Tn}: relative L2 against float64 autograd, fused {fused:.3g}, stft {spec:.3g}")
    assert fused <= GATE and spec <= GATE
    # the zero rule: a silent row has an exactly zero gradient, in torch and here
    silent = torch.zeros(1, Lw, dtype=torch.float64)
    assert not MBO.mel_from_waveform_grad(silent, g_mel, op).any()
    zeros = np.zeros_like(xre)
    assert emu.emu_mel_from_waveform_backward(n_fft, win, hop, Lw, op.num_frequencies, window.ctypes.data, zeros.ctypes.data, zeros.ctypes.data,
                                              first.ctypes.data, count.ctypes.data, wt.ctypes.data, width, gm.ctypes.data, got.ctypes.data) == Tn
    assert not got.any()


BANKS = {"default": dict(), "slaney-norm": dict(mel_scale_norm="slaney"), "slaney-scale": dict(mel_scale_type="slaney"),
         "20Hz-20kHz": dict(min_frequency=20, max_frequency=20000)}


@pytest.mark.parametrize("bank", list(BANKS))
def test_adjoint_table_reproduces_the_bank(O, lib, emu, bank):
    op = O.OracleParams(**BANKS[bank])
    fb = O.mel_filterbank(op)
    first, count, wt, width = _adjoint_table(lib, op, fb)
    fbn = fb.numpy()
    nz = fbn != 0
    assert width == int(count.max()) >= 1 and wt.shape == (op.n_stft, width)
    for k in range(0, op.n_stft, 97):  # the table is the bank's non-zero run of every bin
        idx = np.flatnonzero(nz[k])
        assert count[k] == (idx[-1] - idx[0] + 1 if idx.size else 0)
        if idx.size:
            assert first[k] == idx[0] and np.array_equal(wt[k, :count[k]], fbn[k, first[k]:first[k] + count[k]]) and not wt[k, count[k]:].any()
    assert np.array_equal(count, np.where(nz.any(1), nz.shape[1] - np.argmax(nz[:, ::-1], 1) - np.argmax(nz, 1), 0))
    g = np.random.default_rng(5).standard_normal(op.num_frequencies)
    got = np.full(op.n_stft, 123.0)
    emu.emu_mel_adjoint_apply(op.n_stft, first.ctypes.data, count.ctypes.data, wt.ctypes.data, width, g.ctypes.data, got.ctypes.data)
    # fb @ g in double, every bin's sum over its non-zero weights in increasing band order (at most `width` terms: exact in any order for two)
    want = np.array([sum(float(fbn[k, m]) * g[m] for m in np.flatnonzero(nz[k])) for k in range(op.n_stft)])
    assert np.array_equal(got, want)
    assert np.allclose(got, fbn.astype(np.float64) @ g, rtol=0, atol=1e-15 * np.abs(g).max() * width)


def test_table_query_refusals(O, lib):
    from riffusion import _hip

    op = O.OracleParams()
    fb = O.mel_filterbank(op).contiguous()
    cp = _hip.RfxParams(op.sample_rate, op.n_fft, op.win_length, op.hop_length, op.num_frequencies, op.max_mel_iters)
    width = ctypes.c_int32(0)
    assert lib.rfx_debug_mel_adjoint(None, fb.data_ptr(), None, None, None, 0, ctypes.byref(width)) == -1
    assert lib.rfx_debug_mel_adjoint(ctypes.byref(cp), fb.data_ptr(), None, None, None, 0, None) == -1
    wt = np.full((op.n_stft, 1), 123.0, np.float32)
    assert lib.rfx_debug_mel_adjoint(ctypes.byref(cp), fb.data_ptr(), None, None, wt.ctypes.data, 1, ctypes.byref(width)) == -1
    assert b"capacity" in lib.rfx_last_error() and width.value == 2 and (wt == 123.0).all()


def test_entries_answer_zero_or_refuse_without_a_plan(lib):
    assert lib.rfx_stft_backward_workspace_bytes(None, 1, 17657) == 0 == lib.rfx_mel_from_waveform_backward_workspace_bytes(None, 1, 17657)
    assert lib.rfx_mel_scale_backward_workspace_bytes(None, 1, 41) == 0
    assert lib.rfx_stft_backward(None, None, 1, 17657, None, None, 0, None) == -1 and b"rfx_stft_backward" in lib.rfx_last_error()
    assert lib.rfx_mel_from_waveform_backward(None, None, None, 1, 17657, None, None, 0, None) == -1
    assert b"rfx_mel_from_waveform_backward" in lib.rfx_last_error()
    assert lib.rfx_mel_scale_backward(None, None, 1, 41, None, None, 0, None) == -1 and b"rfx_mel_scale_backward" in lib.rfx_last_error()
    # B == 0 is a no-op
    assert lib.rfx_stft_backward(None, None, 0, 17657, None, None, 0, None) == 0 == lib.rfx_mel_scale_backward(None, None, 0, 41, None, None, 0, None)
    assert lib.rfx_mel_from_waveform_backward(None, None, None, 0, 17657, None, None, 0, None) == 0


def test_sanitized_stand_alone_emulator(emu):
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program; the sanitizers'
    runtimes are linked statically, so the program carries them itself.  Its figures are the unsanitized build's."""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-ffp-contract=off", "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("defect ")]
    assert len(lines) == 12
    for _, n_fft, win, hop, Lw, figure in lines:
        here = emu.emu_stft_adjoint_defect(int(n_fft), int(win), int(hop), int(Lw), 7, None)
        assert float(figure) <= GATE and here <= GATE
        assert abs(float(figure) - here) <= 1e-13, (n_fft, Lw, figure, here)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    emu_build.header_compiles_as_c99(
        tmp_path,
        '#include "rfx.h"\n'
        "size_t q(const rfx_plan* p) { return rfx_stft_backward_workspace_bytes(p, 1, 17657) + rfx_mel_scale_backward_workspace_bytes(p, 1, 41)\n"
        "    + rfx_mel_from_waveform_backward_workspace_bytes(p, 1, 17657); }\n"
        "int f(const rfx_plan* p, const float* w, const float* g, float* o, void* ws, int32_t* n) {\n"
        "  return rfx_mel_from_waveform_backward(p, w, g, 1, 17657, o, ws, 0, 0) + rfx_stft_backward(p, ws, 1, 17657, o, ws, 0, 0)\n"
        "    + rfx_mel_scale_backward(p, g, 1, 41, o, 0, 0, 0) + rfx_debug_mel_adjoint(0, w, n, n, o, 2, n); }\n")


def test_autograd_routing_needs_no_device():
    """`wants_grad` decides the routing; a loop encode of a waveform that requires grad raises before any device work"""
    from riffusion import _autograd
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    w = torch.zeros(1, 512 * 441, requires_grad=True)
    assert _autograd.wants_grad(w) and not _autograd.wants_grad(w.detach())
    with torch.no_grad():
        assert not _autograd.wants_grad(w)
    conv = SpectrogramConverter(SpectrogramParams(), device="cpu")
    with pytest.raises(RuntimeError, match="the loop encode has no backward yet"):
        conv.mel_amplitudes_from_waveform(w, loop=True)
    from riffusion import _hip

    for name in ("stft_backward", "mel_scale_backward", "mel_from_waveform_backward"):
        assert callable(getattr(_hip.Plan, name))
