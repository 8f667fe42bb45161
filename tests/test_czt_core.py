"""
CPU checks of the CHIRP-Z frame transform shared by the gfx950 kernels of rfx_czt.hip (csrc/rfx_czt_core.h): FFT lengths with a prime
factor above 13, which the mixed-radix passes cannot factor, run as a circular convolution with a chirp at the smallest factorable
length >= 2 nc - 1 (Bluestein).  The header is compiled for the host together with tests/emu/rfx_czt_emu.cpp, which loops the logical
threads phase by phase, and compared with numpy's float64 real FFT; then what plan creation decides for such lengths (no GPU:
rfx_debug_plan_bank).

Gates: the project's 3e-6 (real FFT and inverse) and 5e-6 (fused Griffin-Lim frame) of the largest value, as the mixed-radix engine
in tests/test_gen_core.py.  Every case prints what it measures; profiles/chirpz.txt records the figures (tools/probe_chirpz.py).
"""
import ctypes
import os

import numpy as np
import pytest

import emu_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = ctypes.POINTER(ctypes.c_float)
IP = ctypes.POINTER(ctypes.c_int)
RADICES = {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(emu_build.shared("rfx_czt_emu.cpp"))


def fft_len(n_fft):
    return n_fft // 2 if n_fft % 2 == 0 else n_fft


def factorable(n):
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


def largest_lengths(max_nc):
    """The largest even and the largest odd n_fft the chirp-z engine is planned for: FFT length at most max_nc, not factorable."""
    even = next(2 * nc for nc in range(max_nc, 0, -1) if not factorable(nc))
    odd = next(n for n in range(max_nc if max_nc % 2 else max_nc - 1, 0, -2) if not factorable(n))
    return even, odd


# 34 = 2 * 17, 86 = 2 * 43, 94 = 2 * 47, 1892 = 4 * 11 * 43, 2072 = 8 * 7 * 37 (44.1 kHz at 47 ms), 17028 = 4 * 9 * 11 * 43 (42.57 kHz);
# odd: 17, 1009 (prime), 4099 (prime); "even" / "odd": the largest the plan accepts
LENGTHS = [34, 86, 94, 1892, 2072, 17028, 17, 1009, 4099, "even", "odd"]


def resolve(emu, n_fft):
    if isinstance(n_fft, str):
        even, odd = largest_lengths(emu.emu_czt_max_nc())
        return even if n_fft == "even" else odd
    return n_fft


def test_pass_length_is_the_smallest_factorable_one(emu):
    radix = np.zeros(16, np.int32)
    for n_fft in (34, 1892, 17028, 1009, 4099) + largest_lengths(emu.emu_czt_max_nc()):
        nc = fft_len(n_fft)
        assert not factorable(nc)
        M = ctypes.c_int(0)
        k = emu.emu_czt_plan(n_fft, ctypes.byref(M), radix.ctypes.data_as(IP))
        assert k > 0 and int(np.prod(radix[:k].astype(np.int64))) == M.value and set(int(r) for r in radix[:k]) <= RADICES
        assert M.value == next(m for m in range(2 * nc - 1, 4 * nc) if factorable(m))
    # the LDS limit: one more element of FFT length and the buffer of the convolution no longer fits
    max_nc = emu.emu_czt_max_nc()
    M = ctypes.c_int(0)
    assert emu.emu_czt_plan(max_nc, ctypes.byref(M), radix.ctypes.data_as(IP)) > 0 or factorable(max_nc)
    nxt = next(n for n in range(max_nc + 1, 2 * max_nc) if not factorable(n))
    assert emu.emu_czt_plan(2 * nxt, ctypes.byref(M), radix.ctypes.data_as(IP)) == 0
    # 8 bytes x (buffer + lo + hi + lo2 + hi2) against 160 KiB, for the limit's own pass length
    even, _ = largest_lengths(max_nc)
    assert emu.emu_czt_plan(even, ctypes.byref(M), radix.ctypes.data_as(IP)) > 0
    assert 8 * (M.value + 256 + M.value // 128 + 1 + (even // 2) // 128 + 2) <= 160 * 1024


@pytest.mark.parametrize("n_fft", [34, 1892, 1009, 17028])
def test_tables_match_float64(emu, n_fft):
    """c[n] = exp(-i pi n^2 / nc) and H = FFT_M(wrapped conj c) / M, rounded once from double: within half an ulp of the float64
    values numpy gives (|c| = 1, so 6e-8 absolute; H relative to its largest entry)."""
    nc = fft_len(n_fft)
    M = ctypes.c_int(0)
    radix = np.zeros(16, np.int32)
    assert emu.emu_czt_plan(n_fft, ctypes.byref(M), radix.ctypes.data_as(IP)) > 0
    M = M.value
    for ps in (0, 5):
        c = np.zeros(2 * nc, np.float32)
        h = np.zeros(2 * M, np.float32)
        assert emu.emu_czt_tables(n_fft, ps, c.ctypes.data_as(FP), h.ctypes.data_as(FP)) == 0
        n = np.arange(nc, dtype=np.int64)
        want_c = np.exp(-1j * np.pi * ((n * n) % (2 * nc)).astype(np.float64) / nc)
        assert np.abs(c.view(np.complex64) - want_c).max() <= 6.1e-8
        b = np.zeros(M, np.complex128)
        b[:nc] = np.conj(want_c)
        b[M - nc + 1:] = np.conj(want_c[1:][::-1])
        want_h = np.fft.fft(b) / M
        assert np.abs(h.view(np.complex64) - want_h).max() <= 6.1e-8 * np.abs(want_h).max()


@pytest.mark.parametrize("n_fft", LENGTHS)
def test_real_fft_and_inverse_match_numpy(emu, n_fft):
    n_fft = resolve(emu, n_fft)
    rng = np.random.default_rng(n_fft)
    x = rng.standard_normal(n_fft).astype(np.float32)
    out = np.zeros(2 * (n_fft // 2 + 1), np.float32)
    assert emu.emu_czt_rfft(n_fft, x.ctypes.data_as(FP), out.ctypes.data_as(FP), 96, 0) == 0
    ref = np.fft.rfft(x.astype(np.float64))
    err = np.abs(out.view(np.complex64) - ref).max() / np.abs(ref).max()
    own = np.abs(np.fft.rfft(x).astype(np.complex64) - ref).max() / np.abs(ref).max()
    # inverse of an arbitrary one-sided spectrum; imaginary parts of DC / Nyquist are ignored like numpy's / torch's irfft
    X = (rng.standard_normal(n_fft // 2 + 1) + 1j * rng.standard_normal(n_fft // 2 + 1)).astype(np.complex64)
    back = np.zeros(n_fft, np.float32)
    assert emu.emu_czt_irfft(n_fft, X.view(np.float32).ctypes.data_as(FP), back.ctypes.data_as(FP), 64, 0) == 0
    want = np.fft.irfft(X.astype(np.complex128), n_fft)
    err_inv = np.abs(back - want).max() / np.abs(want).max()
    print(f"n_fft {n_fft}: chirp-z rfft {err:.2e}, irfft {err_inv:.2e} of the largest value (numpy float32 rfft vs float64: {own:.2e}; gate 3e-6)")
    assert err < 3e-6, err
    assert err_inv < 3e-6, err_inv
    # determinism: neither the thread count (each phase partitions its elements over the threads) nor the LDS padding (element i
    # at i + (i >> ps): data moves, arithmetic does not) changes a bit
    for nthr, ps in ((7, 0), (96, 4), (512, 6)):
        out2 = np.zeros_like(out)
        assert emu.emu_czt_rfft(n_fft, x.ctypes.data_as(FP), out2.ctypes.data_as(FP), nthr, ps) == 0
        assert np.array_equal(out, out2)
        back2 = np.zeros_like(back)
        assert emu.emu_czt_irfft(n_fft, X.view(np.float32).ctypes.data_as(FP), back2.ctypes.data_as(FP), nthr, ps) == 0
        assert np.array_equal(back, back2)


@pytest.mark.parametrize("n_fft", LENGTHS)
def test_fused_frame_update_matches_numpy(emu, n_fft):
    """One frame of the fused Griffin-Lim kernel: rfft -> S * X / (|X| + 1e-16) -> irfft, with [chirp, projection, conj chirp]
    pairwise IN PLACE between the two convolutions (czt_pair_compute)."""
    n_fft = resolve(emu, n_fft)
    rng = np.random.default_rng(n_fft + 2)
    x = rng.standard_normal(n_fft).astype(np.float32)
    S = (np.abs(rng.standard_normal(n_fft // 2 + 1)) * 100).astype(np.float32)
    out = np.zeros(n_fft, np.float32)
    assert emu.emu_czt_gl_frame(n_fft, x.ctypes.data_as(FP), S.ctypes.data_as(FP), out.ctypes.data_as(FP), 64, 0) == 0
    X = np.fft.rfft(x.astype(np.float64))
    want = np.fft.irfft(S.astype(np.float64) * X / (np.abs(X) + 1e-16), n_fft)
    err = np.abs(out - want).max() / np.abs(want).max()
    print(f"n_fft {n_fft}: chirp-z fused Griffin-Lim frame {err:.2e} of the largest value (gate 5e-6)")
    assert err < 5e-6, err
    for nthr, ps in ((13, 0), (64, 4), (512, 6)):
        out2 = np.zeros_like(out)
        assert emu.emu_czt_gl_frame(n_fft, x.ctypes.data_as(FP), S.ctypes.data_as(FP), out2.ctypes.data_as(FP), nthr, ps) == 0
        assert np.array_equal(out, out2)


# ---- planning (librfx.so on the host: rfx_debug_plan_bank) ------------------------------------------------------------------------
CHIRPZ = 2  # RFX_ENGINE_CHIRPZ


def _report(n_fft, win, hop, frame_engine, sample_rate=44100):
    from riffusion import _hip

    lib = _hip.load_library()
    cp = _hip.RfxParams(sample_rate, n_fft, win, hop, 512, 200)
    opt = _hip.RfxPlanOptions(ctypes.sizeof(_hip.RfxPlanOptions), 0, 0, frame_engine, 0, 0)
    report = _hip.RfxPlanBankReport(struct_size=ctypes.sizeof(_hip.RfxPlanBankReport))
    _hip.check(lib.rfx_debug_plan_bank(ctypes.byref(cp), None, ctypes.byref(opt), ctypes.byref(report)))
    return report


def test_plan_takes_the_chirpz_engine_only_when_asked_and_needed(emu):
    from riffusion import _hip

    assert _hip.FRAME_ENGINES == {"auto": 0, "generic": 1} and _hip.OPT_IN_FRAME_ENGINES == {"chirp-z": CHIRPZ}
    assert _hip.GL_ENGINE_NAMES[3] == "chirp-z"
    with open(os.path.join(ROOT, "include", "rfx.h")) as f:
        assert "RFX_ENGINE_CHIRPZ = 2" in f.read()
    # 42.57 kHz at the default 400 / 100 / 10 ms: 17028 = 4 * 9 * 11 * 43
    r = _report(17028, 4257, 425, CHIRPZ, 42570)
    assert r.engine == 3 and r.fft_length == 8514 and r.pass_length >= 2 * 8514 - 1 and factorable(r.pass_length)
    assert r.pass_length == next(m for m in range(2 * 8514 - 1, 4 * 8514) if factorable(m))
    assert r.frame_stride == (17028 // 2 + 1 + 63) // 64 * 64
    assert r.czt_chirp_elems == 8514 and r.czt_h_elems >= r.pass_length  # (the LDS padding of the buffer is part of H's layout)
    # without the option: refused, in the words it always had
    for engine in (0, 1):
        with pytest.raises(_hip.RfxError, match=r"FFT length 8514 \(from n_fft = 17028\) has a prime factor above 13; implemented radices: 2, 3, 4, 5, 7, 11, 13"):
            _report(17028, 4257, 425, engine, 42570)
    # a length the mixed-radix engines factor ignores the option: planned exactly as under AUTO
    for n_fft, win, hop, rate in ((19200, 4800, 480, 48000), (4410, 1102, 110, 11025), (17640, 4410, 441, 44100), (3465, 3465, 346, 34650)):
        a, z = _report(n_fft, win, hop, 0, rate), _report(n_fft, win, hop, CHIRPZ, rate)
        assert bytes(a) == bytes(z) and a.engine != 3 and a.czt_chirp_elems == 0 and a.pass_length == a.fft_length
    # odd and small lengths
    assert _report(1009, 1009, 100, CHIRPZ, 10090).engine == 3 and _report(34, 34, 3, CHIRPZ).pass_length == 33
    # the LDS limit: the largest lengths plan, the next unfactorable ones are refused with the limits in the message
    max_nc = emu.emu_czt_max_nc()
    even, odd = largest_lengths(max_nc)
    for n_fft in (even, odd):
        r = _report(n_fft, n_fft // 4, n_fft // 40, CHIRPZ)
        assert r.engine == 3 and r.fft_length == fft_len(n_fft)
        # buffer as H lays it out (padding included) + lo + hi + lo2 + hi2, 8 bytes each, inside the LDS of a CU
        assert 8 * (r.czt_h_elems + 256 + r.pass_length // 128 + 1 + r.fft_length // 128 + 2) <= 160 * 1024
    past_even = next(2 * nc for nc in range(max_nc + 1, 2 * max_nc) if not factorable(nc))
    past_odd = next(n for n in range(max_nc + 1, 2 * max_nc) if n % 2 and not factorable(n))
    limits = f"largest supported: n_fft {2 * max_nc} when even, {max_nc if max_nc % 2 else max_nc - 1} when odd"
    for n_fft in (past_even, past_odd):
        with pytest.raises(_hip.RfxError, match="chirp-z engine's convolution buffer .* do not fit the 160 KiB of LDS .*" + limits):
            _report(n_fft, n_fft // 4, n_fft // 40, CHIRPZ)
    # an engine code the library does not know
    with pytest.raises(_hip.RfxError, match="frame_engine"):
        _report(17028, 4257, 425, 3, 42570)


def test_python_layer_names_the_engine():
    """The name goes through Plan's option check (unknown names are refused on the host, before any device call), the converters
    carry it, and the command line offers it."""
    import inspect

    from riffusion import _hip, cli
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    with pytest.raises(ValueError, match="chirp-z"):
        _hip.Plan(SpectrogramParams(), "cuda", frame_engine="fastest")
    for cls in (SpectrogramConverter, SpectrogramImageConverter):
        spec = inspect.signature(cls.__init__).parameters["frame_engine"]
        assert spec.kind is inspect.Parameter.KEYWORD_ONLY and spec.default == "auto"
    p = SpectrogramParams(sample_rate=42570)
    assert SpectrogramImageConverter(p, device="cpu", frame_engine="chirp-z").converter.frame_engine == "chirp-z"
    assert SpectrogramConverter(p, device="cpu").frame_engine == "auto"
    for argv in (["audio-to-image", "--audio", "a.wav", "--image", "b.png"], ["image-to-audio", "--image", "b.png", "--audio", "a.wav"],
                 ["images-to-audio-batch", "--image-dir", "a", "--output-dir", "b"], ["audio-to-images-batch", "--audio-dir", "a", "--output-dir", "b"]):
        assert cli.build_parser().parse_args(argv).frame_engine == "auto"
        assert cli.build_parser().parse_args(argv + ["--frame-engine", "chirp-z"]).frame_engine == "chirp-z"
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(argv + ["--frame-engine", "generic"])
