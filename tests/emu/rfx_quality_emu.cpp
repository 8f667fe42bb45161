// Host emulator of the spectral-error reduction (csrc/rfx_quality.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_quality_cpu.py with g++): it runs the functions of rfx_quality_core.h that the kernels inline - the mask of counted
// positions, a thread's partial sums, the halving tree, the combine - the way the kernels walk them: one workgroup of
// kQualThreads logical threads per chunk of kQualFrames frames of a row, then one per row over the row's partials.  What the
// kernels have of their own is the barrier between two levels of the tree.
#include <cstdint>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_quality_core.h"

using namespace rfx;

static QualSums tree(std::vector<QualSums>& s) {
  for (int stride = kQualThreads / 2; stride > 0; stride >>= 1)
    for (int tid = 0; tid < stride; ++tid) qual_tree_step(s.data(), tid, stride);
  return s[0];
}

extern "C" {

int emu_qual_threads() { return kQualThreads; }
int emu_qual_frames() { return kQualFrames; }

// mask[p] = 1 when position p of a frame of fs floats counts; by the scalar definition (vector == 0) or the kernels' four at a time
void emu_qual_mask(int fs, int n_stft, int plain, int vector, uint8_t* mask) {
  for (int p = 0; p < fs; ++p) {
    if (vector) mask[p] = ((plain ? qual_plain_counts4(p >> 2, n_stft) : qual_slot_counts4(p >> 2)) >> (p & 3)) & 1u;
    else mask[p] = plain ? p < n_stft : qual_pos_counts(p);
  }
}

// a, m: [B * T][fs] float32, 16-byte aligned -> sums (B, 2)
void emu_spectral_error(const float* a, const float* m, int B, int T, int fs, int n_stft, int plain, double* sums) {
  const int chunks = qual_chunks(T);
  std::vector<QualSums> partials((size_t)chunks), s(kQualThreads);
  for (int row = 0; row < B; ++row) {
    const size_t row_at = (size_t)row * T * fs;
    for (int chunk = 0; chunk < chunks; ++chunk) {  // qual_partial_kernel, workgroup (row, chunk)
      const int f0 = chunk * kQualFrames, f1 = f0 + kQualFrames < T ? f0 + kQualFrames : T;
      for (int tid = 0; tid < kQualThreads; ++tid)
        s[tid] = plain ? qual_thread_partial<true>(a + row_at, m + row_at, f0, f1, fs, n_stft, tid)
                       : qual_thread_partial<false>(a + row_at, m + row_at, f0, f1, fs, n_stft, tid);
      partials[chunk] = tree(s);
    }
    for (int tid = 0; tid < kQualThreads; ++tid) s[tid] = qual_combine_partial(partials.data(), chunks, tid);  // qual_combine_kernel
    const QualSums r = tree(s);
    sums[2 * row] = r.num;
    sums[2 * row + 1] = r.den;
  }
}

}  // extern "C"
