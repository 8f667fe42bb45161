// Host emulator of the closed-form InverseMelScale (csrc/rfx_imel_lstsq.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_imel_lstsq_cpu.py with g++): it runs the functions of rfx_imel_lstsq_core.h that the kernels inline - the two sweeps
// of the tridiagonal solve, one logical lane per frame, and the two-tap expansion - on the factor tables rfx_debug_lstsq_bank
// reports.  What the kernels have of their own is the mapping of frames to lanes, the staging of y in LDS and the slot order of
// the output: the emulator writes plain (B, n_stft, T) magnitudes, what rfx_unpack_magnitudes makes of the device's frames.
#include <cstddef>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_imel_lstsq_core.h"

using namespace rfx;

extern "C" {

int emu_lsq_batch() { return kLsqBatch; }

// fb: the dense bank [F][M]; nl, inv_d: [M]; mel (B, M, T) -> y (B, M, T) and out (B, F, T).  y may be null.
void emu_inverse_mel_lstsq(const float* fb, const float* nl, const float* inv_d, const float* mel, int B, int F, int M, int T, float* y_out,
                           float* out) {
  // per bin, as rfx_plan_core.h reads the bank: first filter and two weights; a bin without a filter aims at the zeros behind y
  std::vector<int> m0(F, M);
  std::vector<float> w0(F, 0.f), w1(F, 0.f);
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < M; ++m)
      if (fb[(size_t)f * M + m] != 0.f) {
        m0[f] = m;
        w0[f] = fb[(size_t)f * M + m];
        w1[f] = m + 1 < M ? fb[(size_t)f * M + m + 1] : 0.f;
        break;
      }
  std::vector<float> zy((size_t)M * T), col((size_t)lsq_y_stride(M));
  for (int b = 0; b < B; ++b) {
    const float* mel_row = mel + (size_t)b * M * T;
    for (int t = 0; t < T; ++t) {  // lsq_solve_kernel, lane t of row b
      lsq_forward_sweep(nl, mel_row + t, zy.data() + t, (size_t)T, M);
      lsq_backward_sweep(nl, inv_d, zy.data() + t, (size_t)T, M);
    }
    if (y_out)
      for (size_t i = 0; i < (size_t)M * T; ++i) y_out[(size_t)b * M * T + i] = zy[i];
    for (int t = 0; t < T; ++t) {  // lsq_expand_kernel: the frame's y, two zeros behind it
      for (int m = 0; m < M; ++m) col[m] = zy[(size_t)m * T + t];
      for (int m = M; m < lsq_y_stride(M); ++m) col[m] = 0.f;
      for (int f = 0; f < F; ++f) out[((size_t)b * F + f) * T + t] = lsq_expand_value(w0[f], w1[f], col[m0[f]], col[m0[f] + 1]);
    }
  }
}

}  // extern "C"
