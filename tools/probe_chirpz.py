"""Chirp-z engine against the generic engine: B synthetic 512-frame tiles decoded (tiles -> audio) and B clips encoded (audio -> mel)
at 42.57 kHz (n_fft 17028 = 4 * 9 * 11 * 43: chirp-z, opt-in) and at the nearest sample rate whose FFT length the mixed-radix passes
factor (generic engine), plus the transform's measured errors: the device's STFT against torch.stft in float64 on the host, and the
host emulator (tests/emu/rfx_czt_emu.cpp) against numpy's float64 FFT.  Writes profiles/chirpz.txt.

    python tools/probe_chirpz.py            (B=64 RATE=42570 by default)
"""
import ctypes, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))
import numpy as np, torch
from riffusion import _hip
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import image_util

B, T = int(os.environ.get("B", 64)), 512
RATE = int(os.environ.get("RATE", 42570))
FP = ctypes.POINTER(ctypes.c_float)


def factorable(n):
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


def fft_len(rate):
    n_fft = SpectrogramParams(sample_rate=rate).n_fft
    return n_fft // 2 if n_fft % 2 == 0 else n_fft


def measure(rate, engine):
    p = SpectrogramParams(sample_rate=rate, max_frequency=min(10000, rate // 2))
    plan = _hip.get_plan(p, "cuda", frame_engine=engine)
    tiles = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(B, 512, T, 3), dtype=np.uint8)).cuda()
    lut = torch.from_numpy(image_util.decode_lut(0.25, 30e6)).cuda()
    wave_in = torch.randn(B, p.hop_length * (T - 1), device="cuda") * 8000
    best = [1e30, 1e30, 1e30, 1e30]
    for rep in range(3):
        torch.cuda.synchronize(); t0 = time.time()
        wave = plan.griffinlim(plan.inverse_mel(plan.image_decode(tiles, False, lut), 1, seed=rep), B, T, 32, 0.99, seed=rep + 1)
        plan.pcm16(wave, channels=1, normalize=True)
        torch.cuda.synchronize(); t1 = time.time()
        mel = plan.mel_from_waveform(wave_in)
        torch.cuda.synchronize(); t2 = time.time()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(); lin = plan.inverse_mel(plan.image_decode(tiles, False, lut), 1, seed=9); e[1].record()
        plan.griffinlim(lin, B, T, 32, 0.99, seed=3); e[2].record(); torch.cuda.synchronize()
        best = [min(a, b) for a, b in zip(best, (t1 - t0, t2 - t1, e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])))]
    # the device's STFT of one short clip against torch.stft in float64 on the host
    w1 = (torch.randn(1, p.hop_length * 40 + 5, generator=torch.Generator().manual_seed(1)) * 8000)
    ref = torch.stft(w1.double(), p.n_fft, p.hop_length, p.win_length, torch.hann_window(p.win_length, dtype=torch.float64), center=True,
                     pad_mode="reflect", return_complex=True)
    ref32 = torch.stft(w1, p.n_fft, p.hop_length, p.win_length, torch.hann_window(p.win_length), center=True, pad_mode="reflect", return_complex=True)
    _, spec, Tn = plan.stft(w1.cuda(), want_mag=False, want_spec=True)
    err = float((plan.unpack_complex(spec, 1, Tn).cpu() - ref).abs().max() / ref.abs().max())
    own = float((ref32 - ref).abs().max() / ref.abs().max())
    line = (f"{rate} Hz, n_fft {p.n_fft} [{plan.griffinlim_engine}]: decode {B} tiles {1e3 * best[0]:.1f} ms = {B / best[0]:.0f} tiles/s (InverseMelScale {best[2]:.1f} ms, "
            f"Griffin-Lim 32 {best[3]:.1f} ms); forward {1e3 * best[1]:.2f} ms = {B / best[1]:.0f} images/s; STFT vs torch.stft float64 {err:.2e} of the largest bin "
            f"(torch.stft float32: {own:.2e}); finite={bool(torch.isfinite(mel).all())}")
    return line, B / best[0], B / best[1]


def emulator_errors():
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "librfx_czt_emu.so")
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "emu", "rfx_czt_emu.cpp")], check=True)
        emu = ctypes.CDLL(so)
        rows = []
        max_nc = emu.emu_czt_max_nc()  # the largest even and odd n_fft the plan accepts for this engine
        even = next(2 * nc for nc in range(max_nc, 0, -1) if not factorable(nc))
        odd = next(n for n in range(max_nc if max_nc % 2 else max_nc - 1, 0, -2) if not factorable(n))
        for n_fft in (34, 86, 94, 1892, 2072, 17028, 17, 1009, 4099, even, odd):
            rng = np.random.default_rng(n_fft)
            x = rng.standard_normal(n_fft).astype(np.float32)
            out = np.zeros(2 * (n_fft // 2 + 1), np.float32)
            emu.emu_czt_rfft(n_fft, x.ctypes.data_as(FP), out.ctypes.data_as(FP), 96, 0)
            ref = np.fft.rfft(x.astype(np.float64))
            err = np.abs(out.view(np.complex64) - ref).max() / np.abs(ref).max()
            own = np.abs(np.fft.rfft(x).astype(np.complex64) - ref).max() / np.abs(ref).max()
            S = (np.abs(rng.standard_normal(n_fft // 2 + 1)) * 100).astype(np.float32)
            o = np.zeros(n_fft, np.float32)
            emu.emu_czt_gl_frame(n_fft, x.ctypes.data_as(FP), S.ctypes.data_as(FP), o.ctypes.data_as(FP), 64, 0)
            want = np.fft.irfft(S.astype(np.float64) * ref / (np.abs(ref) + 1e-16), n_fft)
            X = (rng.standard_normal(n_fft // 2 + 1) + 1j * rng.standard_normal(n_fft // 2 + 1)).astype(np.complex64)
            back = np.zeros(n_fft, np.float32)
            emu.emu_czt_irfft(n_fft, X.view(np.float32).ctypes.data_as(FP), back.ctypes.data_as(FP), 64, 0)
            wi = np.fft.irfft(X.astype(np.complex128), n_fft)
            rows.append(f"  n_fft {n_fft:5d}: rfft {err:.2e} (numpy float32 rfft: {own:.2e}), irfft {np.abs(back - wi).max() / np.abs(wi).max():.2e} (gates 3e-6), fused Griffin-Lim frame "
                        f"{np.abs(o - want).max() / np.abs(want).max():.2e} (gate 5e-6)")
        return rows


assert not factorable(fft_len(RATE)), f"{RATE} Hz plans on the generic engine: nothing to compare"
near = min((r for r in range(RATE - 2000, RATE + 2000) if factorable(fft_len(r))), key=lambda r: (abs(r - RATE), r))
lines = [f"chirp-z engine vs generic engine, {B} tiles of {T} frames, best of three (tools/probe_chirpz.py)"]
if torch.cuda.is_available():
    cz, cz_dec, cz_fwd = measure(RATE, "chirp-z")
    ge, ge_dec, ge_fwd = measure(near, "auto")
    lines += [cz, ge, f"ratio chirp-z / generic: decode {cz_dec / ge_dec:.3f}, forward {cz_fwd / ge_fwd:.3f}"]
else:  # the host half alone
    lines += [f"throughput at {RATE} Hz against {near} Hz (generic engine) and the device's STFT error: NOT MEASURED - this run had no GPU"]
lines += ["host emulator (rfx_czt_core.h on the CPU) against numpy float64, of the largest value:"] + emulator_errors()
text = "\n".join(lines) + "\n"
print(text, end="")
with open(os.path.join(ROOT, "profiles", "chirpz.txt"), "w") as fh:
    fh.write(text)
