// Host emulator of a loop FORWARD call's read positions (csrc/rfx_stft_kernels.hip.h: stft_loop_kernel, stft_mel_loop_kernel,
// stft_mel2_loop_kernel; csrc/rfx_fam_fwd_kernel.hip.h: fam_fwd_loop_kernel; csrc/rfx_gen_stft_kernel.hip.h: gen_stft_loop_kernel;
// csrc/rfx_czt.hip: czt_load_frame<true>) and of its length rule.  TEST INFRASTRUCTURE ONLY (built by tests/test_loop_encode_cpu.py
// with g++, and with tests/emu/rfx_loop_fwd_emu_main.cpp as a stand-alone program under the sanitizers): it walks loop_read_index of
// rfx_loop_core.h the way each engine's forward kernel forms a frame's sample positions - the expressions below are the kernels'
// own.  Every walk returns how many unwrapped positions it handed to loop_read_index outside [-P, 2 P), the range loop_wrap serves:
// it must be 0.
#include <cstddef>
#include <cstdint>
#include "../../riffusion-hobby_amd/csrc/rfx_loop_core.h"

using namespace rfx;

namespace {
struct Reader {
  int P;
  int bad = 0;
  int at(int p) {
    if (p < -P || p >= 2 * P) ++bad;
    return loop_read_index(p, P);
  }
};
}  // namespace

extern "C" {

int emu_loop_samples_valid(int hop, int n_fft, long long Lw) { return loop_samples_valid(hop, n_fft, Lw) ? 1 : 0; }
int emu_loop_samples_frames(int hop, int n_fft, long long Lw) { return loop_samples_frames(hop, n_fft, Lw); }
long long emu_loop_samples_below(int hop, int n_fft, long long Lw) { return loop_samples_below(hop, n_fft, Lw); }
long long emu_loop_samples_above(int hop, int n_fft, long long Lw) { return loop_samples_above(hop, n_fft, Lw); }

// generic engine (one thread per element i of the padded frame; only the window's elements read) and chirp-z engine (the same
// position, czt_load_frame): window position j = i - left at hop t + i - n_fft / 2.  idx[win]
int emu_fwd_gather_gen(int n_fft, int win, int hop, int T, int t, int32_t* idx) {
  Reader r{hop * T};
  const int half = n_fft / 2, left = (n_fft - win) / 2;
  for (int i = 0; i < n_fft; ++i) {
    const int j = i - left;
    if (j >= 0 && j < win) idx[j] = r.at(hop * t + i - half);
  }
  return r.bad;
}

// row family (n_fft == 40 H, win == 10 H): thread n' < H reads window positions j H + n', j < 10, at hop fr + off + j H + n',
// off = left - n_fft / 2 (FamGeom::off).  idx[win]
int emu_fwd_gather_fam(int n_fft, int win, int hop, int T, int fr, int32_t* idx) {
  Reader r{hop * T};
  const int H = win / 10, off = (n_fft - win) / 2 - n_fft / 2;
  for (int npr = 0; npr < H; ++npr)
    for (int j = 0; j < 10; ++j) idx[j * H + npr] = r.at(hop * fr + off + j * H + npr);
  return r.bad;
}

// specialised engine, stft_loop_kernel and stft_mel_loop_kernel (win == 10 hop, n_fft / 2 - left == 5 hop): thread n' < hop reads hop
// blocks fr - 5 .. fr + 4 of every frame afresh.  idx[win]
int emu_fwd_gather_blocks(int hop, int T, int fr, int32_t* idx) {
  Reader r{hop * T};
  for (int npr = 0; npr < hop; ++npr)
    for (int j = 0; j < 10; ++j) idx[j * hop + npr] = r.at((fr + j - 5) * hop + npr);
  return r.bad;
}

// specialised engine, stft_mel2_loop_kernel: a workgroup walks the run [f0, f1) with a sliding window - load_frame(f0) fetches the ten
// blocks, and during frame fr's mel phase next_frame(fr + 1) shifts them down and fetches block fr + 1 + 4 alone, after the run's last
// frame too (a look-ahead that is read and dropped: at f1 == T it reaches block T + 4).  slide == 0: next_frame re-fetches all ten
// (the 21-slot form).  idx[(f1 - f0)][win]: what frame fr's transform is given
int emu_fwd_gather_run(int hop, int T, int f0, int f1, int slide, int32_t* idx) {
  Reader r{hop * T};
  const int win = 10 * hop;
  for (int npr = 0; npr < hop; ++npr) {
    int d[10];
    auto load_x = [&](int blk) { return r.at(blk * hop + npr); };
    for (int j = 0; j < 10; ++j) d[j] = load_x(f0 + j - 5);
    for (int fr = f0; fr < f1; ++fr) {
      for (int j = 0; j < 10; ++j) idx[(size_t)(fr - f0) * win + j * hop + npr] = d[j];
      if (slide) {
        for (int j = 0; j < 9; ++j) d[j] = d[j + 1];
        d[9] = load_x(fr + 1 + 9 - 5);
      } else {
        for (int j = 0; j < 10; ++j) d[j] = load_x(fr + 1 + j - 5);
      }
    }
  }
  return r.bad;
}

}  // extern "C"
