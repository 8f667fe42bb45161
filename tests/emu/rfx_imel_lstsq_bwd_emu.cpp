// Host emulator of the backward of the closed-form InverseMelScale (csrc/rfx_imel_lstsq.hip: lsq_collect_kernel between two
// lsq_solve_kernel launches).  TEST INFRASTRUCTURE ONLY (built by tests/test_imel_lstsq_bwd_cpu.py with g++): it runs the functions of
// rfx_imel_lstsq_core.h that the kernels inline - the two sweeps, the mask and the per-filter sum - on the factor tables
// rfx_debug_lstsq_bank reports and the lists rfx_debug_lstsq_collect reports.  What the kernel has of its own is the mapping of
// frames and filters to lanes and the staging of the masked frame in LDS; the emulator reads every entry's gradient straight from
// the position the list names, so a wrong position, a bin counted twice or a padding position read shows as a difference.
#include <cstddef>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_imel_lstsq_core.h"

using namespace rfx;

extern "C" {

// fb: the dense bank [F][M]; nl, inv_d: [M]; ptr [M + 1], bin / pos / w [ptr[M]]: the collect's lists; mel (B, M, T);
// gx [B * T][stride]: the gradient in slot layout -> c_out (B, M, T), optional, and g_mel (B, M, T)
void emu_inverse_mel_lstsq_backward(const float* fb, const float* nl, const float* inv_d, const int* ptr, const int* bin, const int* pos,
                                    const float* w, const float* mel, const float* gx, int B, int F, int M, int T, int stride, float* c_out,
                                    float* g_mel) {
  // per bin, as rfx_plan_core.h reads the bank: first filter and two weights
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
  int longest = 0;
  for (int m = 0; m < M; ++m) longest = ptr[m + 1] - ptr[m] > longest ? ptr[m + 1] - ptr[m] : longest;
  std::vector<float> y((size_t)M * T), c((size_t)M * T), col((size_t)lsq_y_stride(M)), run((size_t)longest + 1);
  for (int b = 0; b < B; ++b) {
    const float* mel_row = mel + (size_t)b * M * T;
    float* out_row = g_mel + (size_t)b * M * T;
    for (int t = 0; t < T; ++t) {  // lsq_solve_kernel on mel: the forward's y
      lsq_forward_sweep(nl, mel_row + t, y.data() + t, (size_t)T, M);
      lsq_backward_sweep(nl, inv_d, y.data() + t, (size_t)T, M);
    }
    for (int t = 0; t < T; ++t) {  // lsq_collect_kernel: the frame's y, two zeros behind it
      for (int m = 0; m < M; ++m) col[m] = y[(size_t)m * T + t];
      for (int m = M; m < lsq_y_stride(M); ++m) col[m] = 0.f;
      const float* frame = gx + ((size_t)b * T + t) * (size_t)stride;
      for (int m = 0; m < M; ++m) {
        const int n = ptr[m + 1] - ptr[m];
        for (int i = 0; i < n; ++i) {
          const int f = bin[ptr[m] + i];
          run[i] = lsq_collect_masked(w0[f], w1[f], col[m0[f]], col[m0[f] + 1], frame[pos[ptr[m] + i]]);
        }
        c[(size_t)m * T + t] = lsq_collect_sum(w + ptr[m], 1, run.data(), n);
      }
    }
    if (c_out)
      for (size_t i = 0; i < (size_t)M * T; ++i) c_out[(size_t)b * M * T + i] = c[i];
    for (int t = 0; t < T; ++t) {  // lsq_solve_kernel on c
      lsq_forward_sweep(nl, c.data() + t, out_row + t, (size_t)T, M);
      lsq_backward_sweep(nl, inv_d, out_row + t, (size_t)T, M);
    }
  }
}

}  // extern "C"
