"""
CPU checks of the fused spectral losses (include/rfx.h, "FUSED SPECTRAL LOSSES"; csrc/rfx_spec_loss_core.h).

* tests/emu/rfx_spec_loss_emu.cpp runs the core's slot rule, the plain fold and the circular fold in double over the four geometries of
  tests/engines.ENGINES, at Lw = hop * 40 + 17 (plain) and hop * 41 (loop), and must agree with float64 torch.autograd
  (tests/spec_loss_oracle.py) to the relative L2 of tests/test_mel_backward_cpu.py, 1e-10: the same statement up to the order of the
  sums.  Each term alone and both together; the silent row is exact zeros.
* The circular fold is the adjoint of loop_oracle's circular framing: the defect <A x, y> - <x, A^T y> relative to |A x| |y| stays
  below 1e-12 (double sums of at most hop * T * 10 products: 1e-16 times a few thousand).  The core's own float32 chains
  (spec_loss_loop_sample, both frame families) agree with the double fold to float32 rounding.
* The three sums on the logical threads of the two kernels against numpy.
* The emulator and a `main` of its own are built as a stand-alone program with -fsanitize=address,undefined and run.  Nothing sanitized
  is loaded into Python.
* include/rfx.h compiles as C99 with the new entries; they answer 0 or refuse without a plan.
* The autograd routing, on a fake plan that needs no device.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import loop_oracle
import spec_loss_oracle as SLO
from engines import ENGINES
from helpers import oracle

EMU_SRC = "rfx_spec_loss_emu.cpp"
EMU_MAIN = "rfx_spec_loss_emu_main.cpp"
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
    vp, i, d, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
    lib.emu_spec_loss_frames.argtypes = [i, i, i, i, i]
    lib.emu_spec_loss_backward.argtypes = [i, i, i, i, i, vp, vp, vp, vp, d, d, d, vp]
    lib.emu_loop_fold.argtypes = [i, i, i, i, vp, vp]
    lib.emu_loop_fold_f32.argtypes = [i, i, i, i, i, i, vp, vp, vp]
    lib.emu_loop_adjoint_defect.argtypes = [i, i, i, i, ctypes.c_uint]
    lib.emu_loop_adjoint_defect.restype = d
    lib.emu_spec_loss_sums.argtypes = [vp, vp, i, i, i, f, vp]
    lib.emu_spec_loss_floor_ok.argtypes = [f]
    return lib


def _op(O, name):
    from riffusion.spectrogram_params import SpectrogramParams

    return O.params_from(SpectrogramParams(**ENGINES[name][1]))


def _rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


@pytest.mark.parametrize("loop", [False, True], ids=["plain", "loop"])
@pytest.mark.parametrize("name", list(ENGINES))
def test_emulator_agrees_with_float64_autograd(O, emu, name, loop):
    op = _op(O, name)
    n_fft, win, hop = op.n_fft, op.win_length, op.hop_length
    Lw = hop * 41 if loop else hop * 40 + 17
    gen = torch.Generator().manual_seed(Lw)
    wave = torch.randn(2, Lw, generator=gen, dtype=torch.float64) * 8000
    wave[1] = 0.0
    X = SLO.stft(wave, op, loop)
    Tn = X.shape[-1]
    assert Tn == 41 == emu.emu_spec_loss_frames(n_fft, win, hop, Lw, int(loop))
    M = X.abs() * (0.5 + 1.5 * torch.rand(X.shape, generator=gen, dtype=torch.float64))
    M[1] = torch.rand(M[1].shape, generator=gen, dtype=torch.float64) * 1000.0
    f = 0.1 * float(X[0].abs().median())
    window = O.hann_window(op).double().numpy()
    g_sc, g_lg = torch.tensor([0.7, 1.3], dtype=torch.float64), torch.tensor([-0.4, 0.9], dtype=torch.float64)
    n = op.n_stft * Tn
    for what, gs, gl in (("convergence", g_sc, None), ("log", torch.zeros(2, dtype=torch.float64), g_lg), ("both", g_sc, g_lg)):
        sc, lg, want = SLO.end_to_end(wave, M, op, f if gl is not None else None, gs, gl, loop)
        num = (X.abs() - M).pow(2).sum(dim=(1, 2))
        den = M.pow(2).sum(dim=(1, 2))
        for r in range(2):
            c_sc = float(gs[r] / torch.sqrt(num[r] * den[r])) if float(num[r]) > 0 and float(den[r]) > 0 else 0.0
            c_lg = float(gl[r]) / n if gl is not None else 0.0
            xre, xim = np.ascontiguousarray(X[r].real.numpy()), np.ascontiguousarray(X[r].imag.numpy())
            tgt, got = np.ascontiguousarray(M[r].numpy()), np.full(Lw, 123.0)
            assert emu.emu_spec_loss_backward(n_fft, win, hop, Lw, int(loop), window.ctypes.data, xre.ctypes.data, xim.ctypes.data, tgt.ctypes.data,
                                              c_sc, c_lg, f if gl is not None else 0.0, got.ctypes.data) == Tn
            if r == 1:  # the silent row: exact zeros, in torch and here
                assert not got.any() and not want[1].any()
                continue
            fig = _rel_l2(got, want[0].numpy())
            print(f"{name} {'loop' if loop else 'plain'} Lw {Lw} {what}: relative L2 against float64 autograd {fig:.3g}")
            assert fig <= GATE


@pytest.mark.parametrize("name", list(ENGINES))
def test_circular_fold_is_the_adjoint_of_the_circular_framing(O, emu, name):
    op = _op(O, name)
    n_fft, win, hop = op.n_fft, op.win_length, op.hop_length
    left = (n_fft - win) // 2
    for Tn in (loop_oracle.min_frames(op), 41):
        P = hop * Tn
        rng = np.random.default_rng(Tn)
        x, y = rng.standard_normal(P), rng.standard_normal((Tn, win))
        w = O.hann_window(op).double().numpy()
        idx = loop_oracle._scatter_index(op, Tn).numpy()[left:left + win].T  # (T, win): the sample window element j of frame t reads
        ax = w[None, :] * x[idx]
        back = np.full(P, 123.0)
        wy = np.ascontiguousarray(w[None, :] * y)
        emu.emu_loop_fold(n_fft, win, hop, Tn, wy.ctypes.data, back.ctypes.data)
        defect = abs(float((ax * y).sum()) - float((x * back).sum())) / float(np.linalg.norm(ax) * np.linalg.norm(y))
        own = emu.emu_loop_adjoint_defect(n_fft, win, hop, Tn, 7)
        print(f"{name} T {Tn}: adjoint defect of the circular fold {defect:.3g} against loop_oracle's framing, {own:.3g} against the emulator's own")
        assert defect <= 1e-12 and own <= 1e-12
        # the scatter of loop_oracle's synthesis (index_add_) is the same operator: term for term up to the order of the sums
        ref = np.zeros(P)
        np.add.at(ref, idx, wy)
        assert np.abs(back - ref).max() <= 1e-12 * np.abs(ref).max()
        # the core's float32 chains, both frame families, against the double fold
        pitch, shift = win + 9, 3
        fr = np.zeros((Tn, pitch), np.float32)
        fr[:, shift:shift + win] = wy.astype(np.float32)
        out32 = np.full(P, 123.0, np.float32)
        emu.emu_loop_fold_f32(n_fft, win, hop, Tn, pitch, shift, fr.ctypes.data, None, out32.ctypes.data)
        y32, w32, out_fma = np.ascontiguousarray(y.astype(np.float32)), np.ascontiguousarray(w.astype(np.float32)), np.full(P, 123.0, np.float32)
        emu.emu_loop_fold_f32(n_fft, win, hop, Tn, win, 0, y32.ctypes.data, w32.ctypes.data, out_fma.ctypes.data)
        scale = np.abs(back).max()
        assert np.abs(out32 - back).max() <= 2e-6 * scale and np.abs(out_fma - back).max() <= 2e-6 * scale


def test_three_sums_on_the_logical_threads(emu):
    """num and den are exact here (values are small multiples of 1/8); lsum within n 2^-52 plus the logarithms' ulps of numpy's"""
    rng = np.random.default_rng(3)
    Tn, fs, n_stft = 9, 1028, 1025
    a = (rng.integers(0, 4096, (Tn, fs)) / 8.0).astype(np.float32)
    m = (rng.integers(0, 4096, (Tn, fs)) / 8.0).astype(np.float32)
    f = np.float32(20.0)
    got = np.zeros(3)
    emu.emu_spec_loss_sums(a.ctypes.data, m.ctypes.data, Tn, fs, n_stft, f, got.ctypes.data)
    A, M = a[:, :n_stft].astype(np.float64), m[:, :n_stft].astype(np.float64)
    terms = np.abs(np.log(np.maximum(A, f)) - np.log(np.maximum(M, f)))
    n = Tn * n_stft
    assert got[0] == ((A - M) ** 2).sum() and got[1] == (M ** 2).sum()
    bound = n * 2.0 ** -52 + 4 * 2.0 ** -52 * (np.abs(np.log(np.maximum(A, f))) + np.abs(np.log(np.maximum(M, f)))).sum() / terms.sum()
    assert abs(got[2] - terms.sum()) <= bound * terms.sum()
    emu.emu_spec_loss_sums(a.ctypes.data, m.ctypes.data, Tn, fs, n_stft, 0.0, got.ctypes.data)
    assert got[0] == ((A - M) ** 2).sum() and got[1] == (M ** 2).sum() and got[2] == 0.0
    ok = [emu.emu_spec_loss_floor_ok(v) for v in (0.0, 1e-18, 1.0, 3e38, -1.0, 1e-19, float("inf"), float("nan"))]
    assert ok == [1, 1, 1, 1, 0, 0, 0, 0]


def test_sanitized_stand_alone_emulator(emu):
    """the emulator with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program; the sanitizers'
    runtimes are linked statically, so the program carries them itself.  Its figures are the unsanitized build's."""
    exe = emu_build.sanitized_program([EMU_SRC, EMU_MAIN], "-ffp-contract=off", "-fno-omit-frame-pointer")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ERROR" not in run.stderr, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("defect ")]
    assert len(lines) == 8
    for _, n_fft, win, hop, Tn, figure in lines:
        here = emu.emu_loop_adjoint_defect(int(n_fft), int(win), int(hop), int(Tn), 7)
        assert float(figure) <= 1e-12 and here <= 1e-12 and abs(float(figure) - here) <= 1e-14, (n_fft, Tn, figure, here)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    emu_build.header_compiles_as_c99(
        tmp_path,
        '#include "rfx.h"\n'
        "size_t q(const rfx_plan* p) { return rfx_spectral_loss_workspace_bytes(p, 1, 17657) + rfx_spectral_loss_loop_workspace_bytes(p, 1, 18081)\n"
        "    + rfx_spectral_loss_backward_workspace_bytes(p, 1, 17657) + rfx_spectral_loss_backward_loop_workspace_bytes(p, 1, 18081); }\n"
        "int f(const rfx_plan* p, const float* w, const float* m, const float* c, double* s, float* o, void* ws) {\n"
        "  return rfx_spectral_loss(p, w, m, 1, 17657, 0.5f, s, ws, 0, 0) + rfx_spectral_loss_loop(p, w, m, 1, 18081, 0.0f, s, ws, 0, 0)\n"
        "    + rfx_spectral_loss_backward(p, w, m, c, 1, 17657, 0.5f, o, ws, 0, 0)\n"
        "    + rfx_spectral_loss_backward_loop(p, w, m, c, 1, 18081, 0.5f, o, ws, 0, 0); }\n")


def test_entries_answer_zero_or_refuse_without_a_plan(lib):
    for q in (lib.rfx_spectral_loss_workspace_bytes, lib.rfx_spectral_loss_loop_workspace_bytes, lib.rfx_spectral_loss_backward_workspace_bytes,
              lib.rfx_spectral_loss_backward_loop_workspace_bytes):
        assert q(None, 1, 18081) == 0
    for name in ("rfx_spectral_loss", "rfx_spectral_loss_loop"):
        assert getattr(lib, name)(None, None, None, 1, 18081, 0.5, None, None, 0, None) == -1 and name.encode() in lib.rfx_last_error()
        assert getattr(lib, name)(None, None, None, 0, 18081, 0.5, None, None, 0, None) == 0  # B == 0 is a no-op
        assert getattr(lib, name)(None, None, None, -1, 18081, 0.5, None, None, 0, None) == -1
    for name in ("rfx_spectral_loss_backward", "rfx_spectral_loss_backward_loop"):
        assert getattr(lib, name)(None, None, None, None, 1, 18081, 0.5, None, None, 0, None) == -1 and name.encode() in lib.rfx_last_error()
        assert getattr(lib, name)(None, None, None, None, 0, 18081, 0.5, None, None, 0, None) == 0


class _FakePlan:
    """what _autograd.spectral_losses asks of a plan, on the CPU: fixed sums, and a backward that records its arguments"""

    n_stft = 5

    def __init__(self):
        self.calls = []

    def _forward_frames(self, Lw, shape, loop):
        return Lw // 4

    def spectral_loss_sums(self, wave, slots, log_floor, loop):
        self.calls.append(("sums", log_floor, loop))
        B = wave.shape[0]
        return torch.tensor([[4.0, 16.0, 30.0 if log_floor else 0.0]] * B, dtype=torch.float64)

    def spectral_loss_backward(self, wave, slots, coef, log_floor, loop):
        self.calls.append(("backward", coef.clone(), log_floor, loop))
        return torch.ones_like(wave)


def test_autograd_routing_on_a_fake_plan():
    from riffusion import _autograd, _hip
    from riffusion.spectrogram_converter import SpectralLosses, SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    plan, slots = _FakePlan(), torch.zeros(6, 8)
    w = torch.zeros(2, 12)
    # no graph without requires_grad, nor under no_grad
    sc, lg = _autograd.spectral_losses(plan, w, slots, 0.5, False)
    assert sc.grad_fn is None and lg.grad_fn is None and sc.dtype == lg.dtype == torch.float64
    assert torch.equal(sc, torch.full((2,), 0.5, dtype=torch.float64)) and torch.equal(lg, torch.full((2,), 2.0, dtype=torch.float64))  # sqrt(4/16), 30/15
    wg = w.clone().requires_grad_(True)
    with torch.no_grad():
        assert _autograd.spectral_losses(plan, wg, slots, 0.5, False)[0].grad_fn is None
    assert [c[0] for c in plan.calls] == ["sums", "sums"]
    # a graph with it: the coefficients are g / sqrt(num den) and g / n
    sc, lg = _autograd.spectral_losses(plan, wg, slots, 0.5, True)
    assert sc.grad_fn is not None and lg.grad_fn is not None
    (3.0 * sc.sum() + 6.0 * lg[0]).backward()
    kind, coef, floor, loop = plan.calls[-1]
    assert kind == "backward" and floor == 0.5 and loop is True and coef.dtype == torch.float32
    assert torch.equal(coef, torch.tensor([[3.0 / 8.0, 6.0 / 15.0], [3.0 / 8.0, 0.0]], dtype=torch.float32))
    assert torch.equal(wg.grad, torch.ones_like(w))
    with pytest.raises(RuntimeError, match="second time|once_differentiable|already been freed"):
        sc.sum().backward()
    # no floor: the log coefficient is zero whatever arrives
    plan.calls.clear()
    wg2 = w.clone().requires_grad_(True)
    sc, lg = _autograd.spectral_losses(plan, wg2, slots, 0.0, False)
    (sc.sum() + lg.sum()).backward()
    assert plan.calls[0] == ("sums", 0.0, False) and torch.equal(plan.calls[-1][1][:, 1], torch.zeros(2))
    # the target gets no gradient
    with pytest.raises(RuntimeError, match="target receives no gradient"):
        _autograd.spectral_losses(plan, wg, slots.clone().requires_grad_(True), 0.5, False)
    # a silent target or an exact fit: no convergence gradient (the zero subgradient)
    sums = torch.tensor([[0.0, 16.0, 1.0], [4.0, 0.0, 1.0]], dtype=torch.float64)
    assert not _autograd.loss_coefficients(sums, 15, torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), 0.5).any()
    # the member: argument rules before any device work; log_floor=None is "no log term"
    conv = SpectrogramConverter(SpectrogramParams(), device="cpu")
    with pytest.raises(ValueError, match="takes the target once"):
        conv.spectral_losses(w)
    with pytest.raises(ValueError, match="takes the target once"):
        conv.spectral_losses(w, slots, magnitude_slots=slots)
    with pytest.raises(RuntimeError, match="target receives no gradient"):
        conv.spectral_losses(w, torch.zeros(2, 5, 3, requires_grad=True))
    with pytest.raises(ValueError, match="log_floor"):
        conv.spectral_losses(w, torch.zeros(2, 5, 3), log_floor=-1.0)
    with pytest.raises(ValueError):
        conv.spectral_losses(torch.zeros(2, 441 * 41 + 1), torch.zeros(2, 5, 3), loop=True)
    assert _hip.spectral_loss_floor(None) == 0.0 and _hip.spectral_loss_floor(0.1) == float(np.float32(0.1))
    conv._plan = lambda: type("P", (_FakePlan,), {"pack_magnitudes": lambda self, m: slots})()
    out = conv.spectral_losses(w, torch.zeros(2, 5, 3))
    assert isinstance(out, SpectralLosses) and out.log_magnitude is None and torch.equal(out.convergence, torch.full((2,), 0.5, dtype=torch.float64))
    assert conv.spectral_losses(w, magnitude_slots=slots, log_floor=0.5).log_magnitude is not None
    for name in ("spectral_loss_sums", "spectral_loss_backward"):
        assert callable(getattr(_hip.Plan, name))
