// Stand-alone driver of tests/emu/rfx_mel_bwd_emu.cpp for a sanitizer run (tests/test_mel_backward_cpu.py builds the two files with
// -fsanitize=address,undefined and runs the program).  At the four test geometries and the three row lengths of the test it prints
// the emulator's adjoint defect - Re <STFT x, G> against <x, backward G>, the STFT written out from its definition - one figure per
// line, into heap buffers of exactly the documented sizes; then the zero rule and the three taps of the fold at their edges.
// Exit status 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_mel_bwd_core.h"

extern "C" {
int emu_mel_bwd_frames(int n_fft, int win, int hop, int Lw);
int emu_mel_from_waveform_backward(int n_fft, int win, int hop, int Lw, int M, const double* window, const double* Xre, const double* Xim,
                                   const int32_t* first, const int32_t* count, const float* wt, int width, const double* g_mel, double* grad);
double emu_stft_adjoint_defect(int n_fft, int win, int hop, int Lw, unsigned seed, double* figures);
}

static int failures = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      ++failures;                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                       \
  } while (0)

int main() {
  const int geo[4][3] = {{17640, 4410, 441}, {19200, 4800, 480}, {4410, 1102, 110}, {1001, 251, 26}};
  for (const auto& g : geo) {
    const int n_fft = g[0], win = g[1], hop = g[2], h = n_fft / 2;
    const int lengths[3] = {h + 1, h + hop + 3, hop * 40 + 17};
    for (int Lw : lengths) {
      double fig[2];
      const double defect = emu_stft_adjoint_defect(n_fft, win, hop, Lw, 7u, fig);
      std::printf("defect %d %d %d %d %.17g\n", n_fft, win, hop, Lw, defect);
      CHECK(defect <= 1e-10);
      // the taps: every padded position 0 .. Lw + 2 h - 1 is collected by exactly one sample
      std::vector<int> hits((size_t)Lw + 2 * h, 0);
      for (int j = 0; j < Lw; ++j) {
        int q[3];
        const int n = rfx::mel_bwd_taps(j, h, Lw, q);
        for (int i = 0; i < n; ++i) {
          CHECK(q[i] >= 0 && q[i] < Lw + 2 * h);
          if (q[i] >= 0 && q[i] < Lw + 2 * h) ++hits[(size_t)q[i]];
        }
      }
      for (int v : hits) CHECK(v == 1);
    }
    // a silent row: X == 0 everywhere gives a gradient of exact zeros, whatever g_mel is
    const int Lw = h + 1, T = emu_mel_bwd_frames(n_fft, win, hop, Lw), F = h + 1, M = 3;
    std::vector<double> window((size_t)win, 0.5), X((size_t)F * T, 0.0), gm((size_t)M * T, 1.25), grad((size_t)Lw, 123.0);
    std::vector<int32_t> first((size_t)F, 0), count((size_t)F, 2);
    std::vector<float> wt((size_t)F * 2, 0.5f);
    CHECK(emu_mel_from_waveform_backward(n_fft, win, hop, Lw, M, window.data(), X.data(), X.data(), first.data(), count.data(), wt.data(), 2,
                                         gm.data(), grad.data()) == T);
    for (double v : grad) CHECK(v == 0.0);
  }
  CHECK(rfx::mel_bwd_unit_scale(3.0, 0.0, 0.0) == 0.0 && rfx::mel_bwd_unit_scale(3.0, 3.0, 4.0) == 0.6);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
