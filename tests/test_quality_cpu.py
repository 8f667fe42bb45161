"""
CPU checks of the spectral-error reduction (csrc/rfx_quality.hip): the arithmetic header csrc/rfx_quality_core.h is compiled for
the host together with tests/emu/rfx_quality_emu.cpp, which walks the logical threads of both kernels, and checked

* against numpy float64 on random slot tensors at magnitudes 1e-6, 30e6 and 1e20.  Bound: relative n * 2^-52, n the number of
  elements summed.  Every term is non-negative, so any order of n - 1 additions (one rounding each, 2^-53; the emulator's fma
  rounds the square and the addition once) is within (n - 1) 2^-53 of the exact sum, and numpy's own pairwise sum of rounded
  squares within (2 + log2 n) 2^-53: together below n * 2^-52 for every n >= 4;
* for batch invariance: a row's 16 bytes placed first, last and alone;
* for the mask: exactly the n_stft bins of a frame are counted, each once, on the specialised slot layout (against the slot
  maps of tests/emu/rfx_emu.cpp) and on the plain frames of a row-family and a generic-engine geometry (frame strides from
  rfx_debug_plan_bank: no GPU);
* under -fsanitize=address,undefined (a stand-alone build of the same emulator) for the same bytes.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emu_build

EMU_SRC = "rfx_quality_emu.cpp"
SCALES = [1e-6, 30e6, 1e20]
SPEC = dict(fs=9408, n_stft=8821, plain=0)  # the default geometry's slot layout (rfx_core.h)


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    lib.emu_qual_mask.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.emu_spectral_error.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return lib


def aligned(shape, dtype=np.float32) -> np.ndarray:
    """a zeroed array whose data starts on a 16-byte boundary (the kernels and the emulator load 16-byte vectors)"""
    n = int(np.prod(shape))
    raw = np.zeros(n * np.dtype(dtype).itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype).reshape(shape)


def mask_of(emu, fs, n_stft, plain, vector=0) -> np.ndarray:
    m = np.zeros(fs, np.uint8)
    emu.emu_qual_mask(fs, n_stft, plain, vector, m.ctypes.data)
    return m.astype(bool)


def emu_sums(emu, a, m, B, T, fs, n_stft, plain) -> np.ndarray:
    assert a.shape == m.shape == (B * T, fs) and a.ctypes.data % 16 == 0 and m.ctypes.data % 16 == 0
    out = np.full((B, 2), np.nan)
    emu.emu_spectral_error(a.ctypes.data, m.ctypes.data, B, T, fs, n_stft, plain, out.ctypes.data)
    return out


def slot_pair(rng, B, T, fs, scale):
    """two slot tensors of magnitude `scale`; what the padding holds must not matter: it holds NaN in one and a huge value in the other"""
    a, m = aligned((B * T, fs)), aligned((B * T, fs))
    a[:] = (rng.random((B * T, fs)) * scale).astype(np.float32)
    m[:] = (rng.random((B * T, fs)) * scale).astype(np.float32)
    return a, m


def poison(emu, a, m, fs, n_stft, plain):
    dead = ~mask_of(emu, fs, n_stft, plain)
    a[:, dead] = np.nan
    m[:, dead] = 3e38


def numpy_sums(a, m, B, T, mask) -> np.ndarray:
    a64 = a.reshape(B, T, -1)[:, :, mask].astype(np.float64)
    m64 = m.reshape(B, T, -1)[:, :, mask].astype(np.float64)
    return np.stack([((a64 - m64) ** 2).sum(axis=(1, 2)), (m64 ** 2).sum(axis=(1, 2))], axis=1)


def geometry(rate=None, **kw):
    """(frame stride, n_stft, plain, engine) as plan creation decides them, without a GPU"""
    import riffusion_oracle as O
    from helpers import plan_bank_report
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams(**({"sample_rate": rate} if rate else {}), **kw)
    op = O.params_from(p)
    rep = plan_bank_report(op)
    return rep.frame_stride, op.n_stft, int(rep.engine != 0), rep.engine


# ---- the mask ------------------------------------------------------------------------------------------------------------------
def test_mask_counts_every_bin_once_on_the_slot_layout(emu):
    fs, n_stft, plain, engine = geometry()
    assert (fs, n_stft, plain, engine) == (SPEC["fs"], SPEC["n_stft"], 0, 0)
    core = ctypes.CDLL(emu_build.shared("rfx_emu.cpp"))
    maps = [np.zeros(9261, np.int32) for _ in range(4)]
    core.emu_slot_maps(*[x.ctypes.data_as(ctypes.c_void_p) for x in maps])
    slot_bin, _, _, pos_f = maps
    pos_bin = np.full(fs, -1)
    pos_bin[pos_f] = slot_bin
    assert int((pos_bin >= 0).sum()) == 9261  # the positions of the 21 x 441 slots are distinct
    mask = mask_of(emu, fs, n_stft, plain)
    assert np.array_equal(mask, mask_of(emu, fs, n_stft, plain, vector=1)), "the four-at-a-time form differs from the definition"
    assert int(mask.sum()) == n_stft and not mask[pos_bin < 0].any()
    assert np.array_equal(np.sort(pos_bin[mask]), np.arange(n_stft)), "a bin is counted twice or not at all"
    # the counted copy of a bin stored twice is the one the unpack reads: the direct slot, bin = k1 + 40 k'
    twice = [b for b in range(n_stft) if (pos_bin == b).sum() == 2]
    assert len(twice) == 440 and all(b % 40 in (0, 20) for b in twice)


@pytest.mark.parametrize("rate,kw,engine", [(48000, {}, 2), (8000, {"max_frequency": 4000}, 2), (11025, {"max_frequency": 5000}, 1),
                                            (34650, dict(padded_duration_ms=100, window_duration_ms=100, max_frequency=8000), 1)])
def test_mask_counts_n_stft_bins_on_plain_frames(emu, rate, kw, engine):
    fs, n_stft, plain, eng = geometry(rate, **kw)
    assert plain == 1 and eng == engine and fs % 64 == 0 and n_stft <= fs < n_stft + 64
    mask = mask_of(emu, fs, n_stft, plain)
    assert np.array_equal(mask, np.arange(fs) < n_stft) and np.array_equal(mask, mask_of(emu, fs, n_stft, plain, vector=1))
    for T in (1, 5):
        a, m = aligned((T, fs)), aligned((T, fs))
        m[:] = 1.0
        got = emu_sums(emu, a, m, 1, T, fs, n_stft, plain)
        assert got[0, 0] == got[0, 1] == float(n_stft * T)  # a = 0, m = 1: both sums count the elements


def test_mask_counts_n_stft_times_T_elements_default_geometry(emu):
    for T in (1, 4, 5, 33):
        a, m = aligned((T, SPEC["fs"])), aligned((T, SPEC["fs"]))
        m[:] = 1.0
        got = emu_sums(emu, a, m, 1, T, **SPEC)
        assert got[0, 0] == got[0, 1] == float(SPEC["n_stft"] * T)


# ---- the sums --------------------------------------------------------------------------------------------------------------------
# T = 1: one partial chunk of one frame; T = 5: a full chunk and a one-frame tail, 9408 / 4 = 2352 vectors per frame are no
# multiple of the 256 threads; the plain geometry: fewer vectors per frame (80) than threads
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("T,geom", [(1, SPEC), (5, SPEC), (7, dict(fs=320, n_stft=257, plain=1)), (1, dict(fs=2240, n_stft=2206, plain=1))])
def test_sums_against_numpy_float64(emu, scale, T, geom):
    rng = np.random.default_rng(T * 1000 + geom["fs"])
    B = 2
    a, m = slot_pair(rng, B, T, geom["fs"], scale)
    poison(emu, a, m, **geom)
    got = emu_sums(emu, a, m, B, T, **geom)
    want = numpy_sums(a, m, B, T, mask_of(emu, **geom))
    n = geom["n_stft"] * T
    rel = np.abs(got - want) / want
    print(f"scale {scale:g}, T {T}, fs {geom['fs']}: relative distance to numpy {rel.max():.2e}, bound {n * 2.0 ** -52:.2e}")
    assert np.isfinite(got).all() and (want > 0).all()
    assert (rel <= n * 2.0 ** -52).all()


def test_exact_known_answers(emu):
    rng = np.random.default_rng(3)
    T = 5
    a, m = slot_pair(rng, 1, T, SPEC["fs"], 30e6)
    assert emu_sums(emu, m, m, 1, T, **SPEC)[0, 0] == 0.0
    zero = aligned((T, SPEC["fs"]))
    z = emu_sums(emu, zero, m, 1, T, **SPEC)
    assert z[0, 0] == z[0, 1]
    base = emu_sums(emu, a, m, 1, T, **SPEC)
    for k in (-40, 7, 60):  # powers of two: every product and sum scales exactly
        a2, m2 = aligned(a.shape), aligned(m.shape)
        a2[:], m2[:] = a * np.float32(2.0 ** k), m * np.float32(2.0 ** k)
        assert np.array_equal(emu_sums(emu, a2, m2, 1, T, **SPEC), base * 4.0 ** k)


@pytest.mark.parametrize("T,geom", [(5, SPEC), (3, dict(fs=320, n_stft=257, plain=1))])
def test_a_rows_bytes_do_not_depend_on_the_batch(emu, T, geom):
    rng = np.random.default_rng(11)
    fs = geom["fs"]
    a, m = slot_pair(rng, 3, T, fs, 30e6)
    alone = emu_sums(emu, a[:T], m[:T], 1, T, **geom)
    for place in (0, 2):
        a3, m3 = slot_pair(rng, 3, T, fs, 1e3)
        a3[place * T:(place + 1) * T], m3[place * T:(place + 1) * T] = a[:T], m[:T]
        got = emu_sums(emu, a3, m3, 3, T, **geom)
        assert got[place].tobytes() == alone[0].tobytes(), place


# ---- the same emulator under the sanitizers ------------------------------------------------------------------------------------
SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rfx_quality_emu.cpp"
// argv: file B T fs n_stft plain; the file holds a then m, [B * T][fs] float32 each; B * 2 doubles go to stdout
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int B = atoi(argv[2]), T = atoi(argv[3]), fs = atoi(argv[4]), n_stft = atoi(argv[5]), plain = atoi(argv[6]);
  const size_t n = (size_t)B * T * fs;
  std::vector<QualVec> a(n / 4), m(n / 4);  // exactly the tensors: a read past their end is the sanitizer's to find
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(a.data(), 4, n, f) != n || fread(m.data(), 4, n, f) != n) return 3;
  fclose(f);
  std::vector<double> sums(2 * (size_t)B);
  emu_spectral_error(a[0].v, m[0].v, B, T, fs, n_stft, plain, sums.data());
  return fwrite(sums.data(), 8, sums.size(), stdout) == sums.size() ? 0 : 4;
}
"""


def test_emulator_under_address_and_undefined_sanitizers(emu, tmp_path):
    main = tmp_path / "quality_san.cpp"
    main.write_text(SAN_MAIN)
    exe = emu_build.sanitized_program(str(main), "-ffp-contract=off", "-static-libasan", "-I", emu_build.EMU_DIR, static=False)
    rng = np.random.default_rng(5)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0")
    for B, T, geom in ((2, 1, SPEC), (1, 5, SPEC), (3, 7, dict(fs=320, n_stft=257, plain=1))):
        a, m = slot_pair(rng, B, T, geom["fs"], 30e6)
        path = tmp_path / f"in_{B}_{T}.bin"
        path.write_bytes(a.tobytes() + m.tobytes())
        run = subprocess.run([exe, str(path), str(B), str(T), str(geom["fs"]), str(geom["n_stft"]), str(geom["plain"])], capture_output=True, env=env)
        assert run.returncode == 0, run.stderr.decode()[-2000:]
        assert run.stdout == emu_sums(emu, a, m, B, T, **geom).tobytes()
