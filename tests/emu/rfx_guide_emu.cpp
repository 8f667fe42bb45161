// Host emulator of the guide staging (csrc/rfx_guide.hip).  TEST INFRASTRUCTURE ONLY (built by tests/test_guided_start_cpu.py
// with g++): it runs the functions of rfx_guide_core.h that the kernels inline - the fit, the peak step, the powers of two, the
// product - the way the two kernels walk them: per (row, chunk) one workgroup of kGuideThreads logical threads, each taking the
// vectors tid, tid + kGuideThreads, ... of its chunk; the second pass takes the largest of the row's chunk peaks.  What the
// kernels have of their own is the 16-byte load and the shuffle / LDS exchange of the maximum.
#include <cstdint>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_guide_core.h"

using namespace rfx;

static int vec_at(int chunk, int i, int tid) { return chunk * kGuideChunk + (i * kGuideThreads + tid) * 4; }

extern "C" {

int emu_guide_chunk() { return kGuideChunk; }
int emu_guide_peak_exp() { return kGuidePeakExp; }

// guide: B rows of guide_samples floats, `stride` elements apart; row_scale: [B][2] or null; dst, zero (nullable): (B, Lpad)
void emu_guide_stage(const float* guide, long long stride, int guide_samples, int B, int L, int Lpad, const float* row_scale, float* dst,
                     float* zero) {
  const int n_valid = guide_samples < L ? guide_samples : L, chunks = guide_chunks(Lpad);
  std::vector<float> peaks((size_t)B * chunks);
  for (int row = 0; row < B; ++row) {  // guide_peak_kernel, workgroup (chunk, row)
    const float* src = guide + (long long)row * stride;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      float wg = 0.f;
      for (int tid = 0; tid < kGuideThreads; ++tid) {
        float peak = 0.f;
        for (int i = 0; i < kGuideVecsPerThread; ++i) {
          const int p = vec_at(chunk, i, tid);
          if (p < n_valid)
            for (int e = 0; e < 4; ++e) peak = guide_peak_step(peak, guide_fit(src, n_valid, p + e));
        }
        wg = fmaxf(wg, peak);
      }
      peaks[(size_t)row * chunks + chunk] = wg;
    }
  }
  for (int row = 0; row < B; ++row) {  // guide_stage_kernel, workgroup (chunk, row)
    const float* src = guide + (long long)row * stride;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      float peak = 0.f;
      for (int c = 0; c < chunks; ++c) peak = fmaxf(peak, peaks[(size_t)row * chunks + c]);
      const GuideScale s = guide_scale(peak, row_scale ? row_scale[2 * (size_t)row] : 0.f);
      for (int tid = 0; tid < kGuideThreads; ++tid)
        for (int i = 0; i < kGuideVecsPerThread; ++i) {
          const int p = vec_at(chunk, i, tid);
          if (p >= Lpad) continue;
          for (int e = 0; e < 4; ++e) {
            dst[(size_t)row * Lpad + p + e] = p < n_valid ? guide_apply(guide_fit(src, n_valid, p + e), s) : 0.f;
            if (zero) zero[(size_t)row * Lpad + p + e] = 0.f;
          }
        }
    }
  }
}

}  // extern "C"
