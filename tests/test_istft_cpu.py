"""
CPU checks of the inverse spectrogram (include/rfx.h, "INVERSE SPECTROGRAM"; csrc/rfx_istft_core.h).

* tests/emu/rfx_istft_emu.cpp runs the core's statement in double - the staging, the analysis (as the circular one of the zero-padded period),
  the slot weights - over an odd and an even FFT length, (n_fft, win, hop) = (1001, 251, 26) and (1000, 250, 26), plain at T = 7 and
  T = 45 and loop at T = 45, against float64 torch.autograd through torch.istft and the circular synthesis (tests/istft_oracle.py).
  Gate: relative L2 of 1e-10.  The emulator's transforms are plain sums of n_fft terms in double: their error is about
  sqrt(n_fft) * 1e-16 = 3e-15 relative, the gate leaves four orders for it and sits far below any index or weight mistake (a wrong
  c_k is a relative error of 0.5 in that bin, a wrong pad one of order 1 in the edge frames).
* The zero-outside rule equals the circular read of the padded period, position by position, and the padded period is the fewest
  whole hops that hold L + n_fft samples (the device comparison of the two routes, as bits, is in tests/test_gpu_istft.py).
* The imaginary part of the gradient is exactly zero in bin 0 and in the Nyquist bin of the even length - and not in the last bin of
  the odd one.
* The adjoint identity <istft(X), g> = Re <X, G> in float64, the forward from the emulator's own synthesis.
* Python layer: argument checks of waveform_from_spectrogram, `length`, and the no_grad path records nothing (on a stand-in plan
  that runs torch.istft: the autograd wiring, not the device).
* The emulator and a `main` of its own are also built as a stand-alone program with -fsanitize=address,undefined and run, into heap
  buffers of exactly the documented sizes.  Nothing sanitized is loaded into Python.
* include/rfx.h compiles as C99 with the new entries; the entries answer 0 or refuse without a plan.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import istft_oracle as IO
from helpers import oracle

EMU_SRC = "rfx_istft_emu.cpp"
EMU_MAIN = "rfx_istft_emu_main.cpp"
GEOMETRIES = {
    "odd-nfft": dict(sample_rate=10010, padded_duration_ms=100, window_duration_ms=25.1, step_size_ms=2.6, max_frequency=5000),
    "even-nfft": dict(sample_rate=10000, padded_duration_ms=100, window_duration_ms=25, step_size_ms=2.6, max_frequency=5000),
}
GEO_SIZES = {"odd-nfft": (1001, 251, 26), "even-nfft": (1000, 250, 26)}
CASES = [(geo, T, loop) for geo in GEOMETRIES for T, loop in ((7, False), (45, False), (45, True))]
CASE_IDS = [f"{geo}-T{T}{'-loop' if loop else ''}" for geo, T, loop in CASES]
GATE = 1e-10


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_istft_samples.argtypes = [i, i, i, i]
    lib.emu_istft_pad_frames.argtypes = [i, i, i]
    lib.emu_zero_outside_defects.argtypes = [i, i, i]
    lib.emu_zero_outside_defects.restype = ctypes.c_longlong
    lib.emu_istft_stage.argtypes = [i, i, i, i, i, i, vp, vp, vp, i]
    lib.emu_istft_backward.argtypes = [i, i, i, i, i, i, vp, vp, vp, vp]
    lib.emu_istft_forward.argtypes = [i, i, i, i, i, vp, vp, vp, vp]
    return lib


def _params(O, geo):
    from riffusion.spectrogram_params import SpectrogramParams

    op = O.params_from(SpectrogramParams(**GEOMETRIES[geo]))
    assert (op.n_fft, op.win_length, op.hop_length) == GEO_SIZES[geo]
    return op


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rel(ref, x):
    return float((ref - x).abs().pow(2).sum().sqrt() / ref.abs().pow(2).sum().sqrt())


def _emu_backward(emu, op, window, g, T, loop, tab_scaled):
    n_stft = op.n_fft // 2 + 1
    re, im = np.zeros((n_stft, T)), np.zeros((n_stft, T))
    emu.emu_istft_backward(op.n_fft, op.win_length, op.hop_length, T, int(loop), int(tab_scaled), _ptr(window), _ptr(g), _ptr(re), _ptr(im))
    return torch.complex(torch.from_numpy(re), torch.from_numpy(im))


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_zero_outside_is_the_circular_read_of_the_padded_period(emu, geo):
    n_fft, _, hop = GEO_SIZES[geo]
    for T in (2, 7, 41, 45):
        L = emu.emu_istft_samples(n_fft, hop, T, 0)
        Tp = emu.emu_istft_pad_frames(hop, n_fft, L)
        assert hop * Tp >= L + n_fft > hop * (Tp - 1), (T, Tp)
        assert emu.emu_zero_outside_defects(n_fft, hop, T) == 0, T


@pytest.mark.parametrize("geo,T,loop", CASES, ids=CASE_IDS)
def test_staging_divides_by_the_envelope_and_pads_with_zeros(O, emu, geo, T, loop):
    op = _params(O, geo)
    window = O.hann_window(op).double().numpy().copy()
    L = IO.samples(op, T, loop)
    pitch = op.hop_length * (T if loop else emu.emu_istft_pad_frames(op.hop_length, op.n_fft, L))
    g = np.random.default_rng(3).standard_normal(L)
    # the envelope the oracle divides by: istft of the spectrum of an impulse train is not needed - the synthesis of ones over env is
    # linear in the frames, so env = (overlap-added w^2) comes from the oracle's own loop_env, or for the plain form from the definition
    if loop:
        import loop_oracle

        env = loop_oracle.loop_env(O, op, T, torch.float64).numpy()
    else:
        w = np.zeros(op.n_fft)
        left = (op.n_fft - op.win_length) // 2
        w[left:left + op.win_length] = window
        env = np.zeros(L + op.n_fft)
        for t in range(T):
            env[op.hop_length * t:op.hop_length * t + op.n_fft] += w * w
        env = env[op.n_fft // 2:op.n_fft // 2 + L]
    for tab_scaled in (0, 1):
        u = np.full(pitch, 7.0)
        emu.emu_istft_stage(op.n_fft, op.win_length, op.hop_length, T, int(loop), tab_scaled, _ptr(window), _ptr(g), _ptr(u), pitch)
        want = g / env * (2.0 / op.n_fft if tab_scaled else 1.0)
        assert np.abs(u[:L] - want).max() <= 1e-13 * np.abs(want).max()
        assert not u[L:].any()


@pytest.mark.parametrize("geo,T,loop", CASES, ids=CASE_IDS)
def test_backward_against_autograd_and_the_adjoint_identity(O, emu, geo, T, loop):
    op = _params(O, geo)
    n_stft, L = op.n_fft // 2 + 1, IO.samples(op, T, loop)
    window = O.hann_window(op).double().numpy().copy()
    gen = torch.Generator().manual_seed(11 + T)
    X = torch.complex(torch.randn(1, n_stft, T, generator=gen, dtype=torch.float64), torch.randn(1, n_stft, T, generator=gen, dtype=torch.float64))
    g = torch.randn(1, L, generator=gen, dtype=torch.float64)
    want = IO.istft_grad(O, X, g, op, torch.float64, loop)[0]
    for tab_scaled in (0, 1):  # the two table kinds of the engines give the same gradient
        got = _emu_backward(emu, op, window, g[0].numpy().copy(), T, loop, tab_scaled)
        rel = _rel(want, got)
        print(f"{geo} T{T} loop={loop} tab_scaled={tab_scaled}: backward rel L2 {rel:.2e}")
        assert rel <= GATE
        # the zero-imaginary rule, as bits
        assert not got.imag[0].any()
        if op.n_fft % 2 == 0:
            assert not got.imag[-1].any()
        else:
            assert got.imag[-1].any()
        assert got.imag[1].any()
    # the forward by the definition against torch.istft / the circular synthesis, and the adjoint identity in float64
    y = np.zeros(L)
    xr, xi = X[0].real.numpy().copy(), X[0].imag.numpy().copy()
    emu.emu_istft_forward(op.n_fft, op.win_length, op.hop_length, T, int(loop), _ptr(window), _ptr(xr), _ptr(xi), _ptr(y))
    y = torch.from_numpy(y)[None]
    assert _rel(IO.istft(O, X, op, torch.float64, loop), y) <= GATE
    defect, lhs, rhs = IO.adjoint_defect(y, g, X, got[None])
    print(f"{geo} T{T} loop={loop}: <y, g> = {lhs:.15e}, Re <X, G> = {rhs:.15e}, relative difference {defect:.2e}")
    assert defect <= GATE


def test_sanitized_stand_alone_emulator():
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program; the sanitizers'
    runtimes are linked statically, so the program carries them itself"""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-ffp-contract=off", "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr
    figures = [float(ln.split()[-1]) for ln in run.stdout.splitlines() if ln.startswith("defect ")]
    assert len(figures) == 12 and max(figures) <= GATE, figures


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------

class _TorchPlan:
    """a stand-in for _hip.Plan whose slots are the (B, n_stft, T) tensor itself and whose istft is torch's: the autograd wiring of
    riffusion/_autograd.py and the converter's `length` handling run without a device"""

    def __init__(self, O, op):
        self.O, self.op, self.n_stft, self.calls = O, op, op.n_fft // 2 + 1, []

    def pack_complex(self, x):
        return x

    def unpack_complex(self, slots, B, Tn):
        return slots

    def istft(self, slots, B, Tn, loop=False):
        self.calls.append("istft")
        return IO.istft(self.O, slots, self.op, torch.float32, loop)

    def istft_backward(self, g, B, Tn, loop=False):
        self.calls.append("istft_backward")
        X = torch.zeros(B, self.n_stft, Tn, dtype=torch.complex64)
        with torch.enable_grad():  # a once_differentiable backward runs with grad mode off
            return IO.istft_grad(self.O, X, g, self.op, torch.float32, loop)


@pytest.fixture()
def conv(O, monkeypatch):
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams(**GEOMETRIES["even-nfft"])
    c = SpectrogramConverter(p, device="cpu")
    plan = _TorchPlan(O, O.params_from(p))
    monkeypatch.setattr(c, "_plan", lambda: plan)
    return c, plan


def test_member_argument_checks(conv):
    c, plan = conv
    X = torch.zeros(2, plan.n_stft, 9, dtype=torch.complex64)
    with pytest.raises(ValueError, match="complex"):
        c.waveform_from_spectrogram(X.abs())
    with pytest.raises(ValueError, match="linear bins"):
        c.waveform_from_spectrogram(X[:, :-1])
    with pytest.raises(ValueError, match="no frames"):
        c.waveform_from_spectrogram(X[..., :0])
    with pytest.raises(ValueError, match="length"):
        c.waveform_from_spectrogram(X, length=-1)
    with pytest.raises(ValueError, match="n_stft, T"):
        c.waveform_from_spectrogram(torch.zeros(plan.n_stft, dtype=torch.complex64))
    assert plan.calls == []  # every refusal comes before the plan is used


def test_member_length_and_leading_dimensions(conv):
    c, plan = conv
    gen = torch.Generator().manual_seed(2)
    X = torch.complex(torch.randn(2, 3, plan.n_stft, 9, generator=gen), torch.randn(2, 3, plan.n_stft, 9, generator=gen))
    L = 26 * 8
    y = c.waveform_from_spectrogram(X)
    assert tuple(y.shape) == (2, 3, L) and y.dtype == torch.float32
    want = torch.istft(X.reshape(6, plan.n_stft, 9), 1000, 26, 250, window=torch.hann_window(250), center=True)
    assert torch.equal(y.reshape(6, L), want)
    for n in (0, 100, L, L + 37):
        cut = c.waveform_from_spectrogram(X, length=n)
        # up to L torch.istft(length=) is the same cut; past L the member pads with zeros (torch keeps its untrimmed tail there)
        ref = (torch.istft(X.reshape(6, plan.n_stft, 9), 1000, 26, 250, window=torch.hann_window(250), center=True, length=n) if 0 < n <= L
               else torch.nn.functional.pad(want, (0, n - L)) if n else want[:, :0])
        assert tuple(cut.shape) == (2, 3, n) and torch.equal(cut.reshape(6, n), ref), n
    assert tuple(c.waveform_from_spectrogram(X[0, 0]).shape) == (L,)


def test_member_records_a_graph_only_when_asked(conv):
    c, plan = conv
    gen = torch.Generator().manual_seed(4)
    X = torch.complex(torch.randn(2, plan.n_stft, 9, generator=gen), torch.randn(2, plan.n_stft, 9, generator=gen))
    assert c.waveform_from_spectrogram(X).grad_fn is None
    leaf = X.clone().requires_grad_(True)
    with torch.no_grad():
        assert c.waveform_from_spectrogram(leaf).grad_fn is None
    assert plan.calls == ["istft", "istft"]
    y = c.waveform_from_spectrogram(leaf, length=300)  # longer than L = 208: the padding gets no gradient, the cut none either
    assert y.grad_fn is not None and tuple(y.shape) == (2, 300)
    g = torch.randn(2, 300, generator=gen)
    y.backward(g)
    assert plan.calls[-1] == "istft_backward" and leaf.grad.shape == X.shape
    ref = X.clone().requires_grad_(True)
    torch.nn.functional.pad(torch.istft(ref, 1000, 26, 250, window=torch.hann_window(250), center=True), (0, 92)).backward(g)
    assert torch.allclose(leaf.grad, ref.grad, rtol=1e-5, atol=1e-9)
    # nothing is saved, and the backward is once-differentiable
    leaf2 = X.clone().requires_grad_(True)
    y2 = c.waveform_from_spectrogram(leaf2)
    (gx,) = torch.autograd.grad(y2, leaf2, torch.ones_like(y2, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.abs().sum().backward()


# ---- the header and the entries without a plan ------------------------------------------------------------------------------------------

ENTRIES = ["rfx_istft", "rfx_istft_loop", "rfx_istft_backward", "rfx_istft_backward_loop"]


def test_entries_without_a_plan():
    from riffusion import _hip

    lib = _hip.load_library()
    for name in ENTRIES:
        assert getattr(lib, name + "_workspace_bytes")(None, 1, 41) == 0
        assert getattr(lib, name)(None, None, 0, 41, None, None, 0, None) == 0  # B == 0 is a no-op
        assert getattr(lib, name)(None, None, 1, 41, None, None, 0, None) == -1 and name.encode() + b": " in lib.rfx_last_error()
        assert getattr(lib, name)(None, None, -1, 41, None, None, 0, None) == -1


def test_header_compiles_as_c99_with_the_entries(tmp_path):
    emu_build.header_compiles_as_c99(
        tmp_path,
        '#include "rfx.h"\n'
        "size_t q(const rfx_plan* p) { return rfx_istft_workspace_bytes(p, 1, 41) + rfx_istft_loop_workspace_bytes(p, 1, 41)\n"
        "  + rfx_istft_backward_workspace_bytes(p, 1, 41) + rfx_istft_backward_loop_workspace_bytes(p, 1, 41); }\n"
        "int r(const rfx_plan* p, void* x, float* y, void* ws) {\n"
        "  return rfx_istft(p, x, 1, 41, y, ws, 0, 0) + rfx_istft_loop(p, x, 1, 41, y, ws, 0, 0)\n"
        "  + rfx_istft_backward(p, y, 1, 41, x, ws, 0, 0) + rfx_istft_backward_loop(p, y, 1, 41, x, ws, 0, 0); }\n")
