// Host emulator of the int16 post-processing kernels (csrc/rfx_pcm.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_pcm_filters_cpu.py with g++): it runs the per-sample and per-clip functions of rfx_pcm_core.h that the kernels
// inline - statistics, factors, apply, and the stitch of the planner's pieces - so that they are pinned against audioop and
// PcmSegment on the CPU.
#include <cstdint>
#include "../../riffusion-hobby_amd/csrc/rfx_pcm_core.h"

using namespace rfx;

extern "C" {

int emu_mul(int x, double f) { return pcm_mul(x, f); }
int emu_add(int a, int b) { return pcm_add(a, b); }

// audioop.rms / audioop.max of n interleaved samples, through the kernels' statistics
unsigned emu_rms(const int16_t* x, int64_t n) {
  int64_t s = 0;
  for (int64_t i = 0; i < n; ++i) s += (int64_t)x[i] * x[i];
  return n > 0 ? pcm_rms(s, n) : 0u;
}
unsigned emu_max(const int16_t* x, int64_t n) {
  unsigned m = 0;
  for (int64_t i = 0; i < n; ++i) {
    const unsigned a = x[i] < 0 ? (unsigned)(-(int)x[i]) : (unsigned)x[i];
    m = a > m ? a : m;
  }
  return m;
}

// apply_filters(compression=False) on every clip of an (N, L, C) batch; factors (N x 2 doubles) optional
void emu_apply_filters(const int16_t* in, int N, int64_t L, int C, const double* gain_by_rms, const double* boost_by_peak,
                       int16_t* out, double* factors) {
  const int64_t count = L * C;
  for (int n = 0; n < N; ++n) {
    const int16_t* x = in + n * count;
    int64_t s = 0;
    int mx = -32768, mn = 32767;
    for (int64_t i = 0; i < count; ++i) {
      s += (int64_t)x[i] * x[i];
      mx = x[i] > mx ? x[i] : mx;
      mn = x[i] < mn ? x[i] : mn;
    }
    const PcmFactors f = pcm_filter_factors(s, count, mx, mn, gain_by_rms, boost_by_peak);
    if (factors) {
      factors[2 * n] = f.f1;
      factors[2 * n + 1] = f.f2;
    }
    for (int64_t i = 0; i < count; ++i) out[n * count + i] = pcm_filter_sample(x[i], f);
  }
}

// the stitch kernel: every output sample from its piece
void emu_stitch(const int16_t* pcm, int64_t L, int C, const PcmPiece* pieces, int n_pieces, int64_t frames, int16_t* out) {
  for (int64_t f = 0; f < frames; ++f) {
    const PcmPiece& p = pieces[pcm_find_piece(pieces, n_pieces, f)];
    for (int c = 0; c < C; ++c) out[f * C + c] = pcm_stitch_sample(p, f, c, pcm, L, C);
  }
}

int emu_piece_bytes() { return (int)sizeof(PcmPiece); }

}  // extern "C"
