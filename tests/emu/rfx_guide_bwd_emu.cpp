// Host emulator of the guided decode's backward (csrc/rfx_guide.hip: guide_stage_rows_kernel; csrc/rfx_guide_bwd.hip:
// guide_project_kernel).  TEST INFRASTRUCTURE ONLY (built by tests/test_guided_backward_cpu.py with g++): it runs the functions of
// rfx_guide_core.h that the kernels inline - the fit, the peak step, the powers of two, guide_project - over the same tables.  What the
// kernels have of their own is the 16-byte access, the exchange of the maximum and the LDS round trip between the two layouts.
#include <cstddef>
#include <cstdint>
#include "../../riffusion-hobby_amd/csrc/rfx_guide_core.h"

using namespace rfx;

extern "C" {

// guide: B rows of guide_samples floats, contiguous; dst: (B, L): the fitted row times the power of two of its peak, no kernel factor
void emu_guide_stage_rows(const float* guide, int guide_samples, int B, int L, float* dst) {
  const int n_valid = guide_samples < L ? guide_samples : L;
  for (int row = 0; row < B; ++row) {
    const float* src = guide + (size_t)row * guide_samples;
    float peak = 0.f;  // (max is exact in any order: the kernels' chunks give this value)
    for (int p = 0; p < n_valid; ++p) peak = guide_peak_step(peak, src[p]);
    const GuideScale s = guide_scale(peak, 0.f);
    for (int p = 0; p < L; ++p) dst[(size_t)row * L + p] = p < n_valid ? guide_apply(guide_fit(src, n_valid, p), s) : 0.f;
  }
}

// G, A: nframes frames of xstride complex slots (re, im interleaved); out: nframes frames of sstride floats
void emu_guide_project(const float* G, const float* A, const int32_t* xpos_bin, const int32_t* s2x, long long nframes, int xstride, int sstride,
                       float* out) {
  for (long long fr = 0; fr < nframes; ++fr) {
    const float* g = G + 2 * (size_t)fr * xstride;
    const float* a = A + 2 * (size_t)fr * xstride;
    for (int p = 0; p < sstride; ++p) {
      const int x = s2x[p];
      out[(size_t)fr * sstride + p] = x < 0 || xpos_bin[x] < 0 ? 0.f : guide_project(cf{a[2 * x], a[2 * x + 1]}, cf{g[2 * x], g[2 * x + 1]});
    }
  }
}

}  // extern "C"
