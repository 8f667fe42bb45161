// Stand-alone driver of tests/emu/rfx_loop_fwd_emu.cpp for a sanitizer run (tests/test_loop_encode_cpu.py builds the two files with
// -fsanitize=address,undefined and runs the program): every walk of the emulator at the four test geometries, T = the smallest frame
// count and one more, into heap buffers of exactly the size the walk is documented to write, checked against the definition
// (hop t + i - n_fft / 2) mod P computed here with a 64-bit modulo.  Exit status 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int emu_loop_samples_valid(int hop, int n_fft, long long Lw);
int emu_loop_samples_frames(int hop, int n_fft, long long Lw);
long long emu_loop_samples_below(int hop, int n_fft, long long Lw);
long long emu_loop_samples_above(int hop, int n_fft, long long Lw);
int emu_fwd_gather_gen(int n_fft, int win, int hop, int T, int t, int32_t* idx);
int emu_fwd_gather_fam(int n_fft, int win, int hop, int T, int fr, int32_t* idx);
int emu_fwd_gather_blocks(int hop, int T, int fr, int32_t* idx);
int emu_fwd_gather_run(int hop, int T, int f0, int f1, int slide, int32_t* idx);
}

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      ++failures;                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
    }                                                            \
  } while (0)

static int want(int n_fft, int win, int hop, int T, int t, int j) {
  const long long P = (long long)hop * T, p = (long long)hop * t + (n_fft - win) / 2 + j - n_fft / 2;
  return (int)(((p % P) + P) % P);
}

int main() {
  const int geo[4][3] = {{17640, 4410, 441}, {19200, 4800, 480}, {4410, 1102, 110}, {1001, 251, 26}};
  for (const auto& g : geo) {
    const int n_fft = g[0], win = g[1], hop = g[2], tmin = (n_fft + hop - 1) / hop;
    for (int T = tmin; T <= tmin + 1; ++T) {
      const long long P = (long long)hop * T;
      CHECK(emu_loop_samples_valid(hop, n_fft, P) == 1 && emu_loop_samples_frames(hop, n_fft, P) == T);
      CHECK(emu_loop_samples_valid(hop, n_fft, P - 1) == 0 && emu_loop_samples_frames(hop, n_fft, P + 1) == 0);
      CHECK(emu_loop_samples_below(hop, n_fft, P + 1) == P && emu_loop_samples_above(hop, n_fft, P + 1) == P + hop);
      CHECK(emu_loop_samples_below(hop, n_fft, (long long)hop * tmin - 1) == 0 && emu_loop_samples_above(hop, n_fft, -7) == (long long)hop * tmin);
      const bool fam = n_fft == 4 * win && win % 10 == 0, blocks = fam && win == 10 * hop;
      for (int t = 0; t < T; ++t) {
        std::vector<int32_t> a(win), b(win);
        CHECK(emu_fwd_gather_gen(n_fft, win, hop, T, t, a.data()) == 0);
        for (int j = 0; j < win; ++j) CHECK(a[j] == want(n_fft, win, hop, T, t, j));
        if (fam) {
          CHECK(emu_fwd_gather_fam(n_fft, win, hop, T, t, b.data()) == 0);
          CHECK(a == b);
        }
        if (blocks) {
          CHECK(emu_fwd_gather_blocks(hop, T, t, b.data()) == 0);
          CHECK(a == b);
        }
      }
      if (blocks)
        for (int slide = 0; slide < 2; ++slide)
          for (int per = 1; per <= T; per += 6) {  // runs of `per` frames, the last one short
            for (int f0 = 0; f0 < T; f0 += per) {
              const int f1 = f0 + per < T ? f0 + per : T;
              std::vector<int32_t> run((size_t)(f1 - f0) * win);
              CHECK(emu_fwd_gather_run(hop, T, f0, f1, slide, run.data()) == 0);
              for (int fr = f0; fr < f1; ++fr)
                for (int j = 0; j < win; ++j) CHECK(run[(size_t)(fr - f0) * win + j] == want(n_fft, win, hop, T, fr, j));
            }
          }
    }
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
