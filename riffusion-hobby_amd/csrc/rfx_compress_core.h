// rfx_compress_core.h - per-step arithmetic of apply_filters(compression=True)'s compressor (pydub 0.25.1
// effects.compress_dynamic_range, riffusion/util/audio_util.py PcmSegment.compress_dynamic_range), written once for both the
// gfx950 kernels (rfx_compress.hip, hipcc) and the host emulator of the CPU tests (tests/emu/rfx_compress_emu.cpp, g++).
//
// The compressor's window rms values read its INPUT, so they are all known before the loop; only the attenuation is a
// recurrence.  Its step is pydub's, on values the host tabulated by rms with pydub's own expressions (audio_util.compress_tables):
//   if above[r] and att <= max_att[r]:  att = min(att + inc[r], max_att[r])     (Python's min: att unless max_att < att)
//   else:                               att = max(att - dec[r], 0)              (Python's max: att unless 0 > att)
// one IEEE add or subtract, compares and selects - no multiply, nothing to contract - so every form that takes the same steps
// from the same state computes the same bits.  A frame is QUIET when its step is the identity for every reachable state
// (att >= 0): not above, and dec == +0.0.  That holds for every frame at or below the threshold, where max_att is 0, so pydub
// holds the attenuation through quiet passages.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rfx_pcm_core.h"

#if defined(__HIPCC__)
#define RFX_CMP_HD __host__ __device__ __forceinline__
#else
#define RFX_CMP_HD inline __attribute__((always_inline))
#endif

namespace rfx {

// the four tables of audio_util.compress_tables, 32769 entries each (indexed by audioop.rms of a window)
struct CmpTables {
  const uint8_t* above;
  const double* max_att;
  const double* inc;
  const double* dec;
};

RFX_CMP_HD uint64_t cmp_bits(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}

// the parameters of one frame's step, looked up from its window rms (independent of the state: loaded ahead of the steps)
struct CmpFrame {
  double m, inc, dec;
  bool above;
};

RFX_CMP_HD CmpFrame cmp_frame(const CmpTables& t, unsigned r) { return CmpFrame{t.max_att[r], t.inc[r], t.dec[r], t.above[r] != 0}; }

RFX_CMP_HD bool cmp_quiet(const CmpFrame& f) { return !f.above && cmp_bits(f.dec) == 0; }

RFX_CMP_HD double cmp_step(double att, const CmpFrame& f) {
  if (f.above && att <= f.m) {
    const double a = att + f.inc;
    return f.m < a ? f.m : a;
  }
  const double a = att - f.dec;
  return 0.0 > a ? 0.0 : a;
}

// audioop.rms of the window [max(0, i - look), i) of one clip from its exact int64 prefix sums of frame energies
// (prefix[j] = sum of x^2 over frames < j, all channels); 0 for an empty window.  Below 2^53 the double division and square
// root see the exact sum, as audioop's double accumulator does.
RFX_CMP_HD unsigned cmp_window_rms(const int64_t* prefix, int64_t i, int64_t look, int C) {
  const int64_t lo = i - look > 0 ? i - look : 0;
  const int64_t n = (i - lo) * C;
  if (n <= 0) return 0u;
  const double s = (double)(prefix[i] - prefix[lo]);
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)__dsqrt_rn(__ddiv_rn(s, (double)n));
#else
  return (unsigned)sqrt(s / (double)n);
#endif
}

constexpr int kCmpBatch = 8;  // frames whose parameters are loaded before their steps run

// Run the recurrence over frames [b, e) of one clip from state `att` (rms: the clip's per-frame window rms).  Each state
// after a step goes to traj[i].  With `stop_on_match`, the run ends at the first frame whose new state equals the stored
// traj[i] bitwise: from there on the stored trajectory is the one this start produces.  Returns the state after the last
// frame stepped (after frame e - 1 when it ran through), and sets *matched / *any_above.
RFX_CMP_HD double cmp_run(double att, const uint16_t* rms, const CmpTables& t, double* traj, int64_t b, int64_t e,
                          bool stop_on_match, bool* matched, bool* any_above) {
  bool hit = false, loud = false;
  for (int64_t i0 = b; i0 < e && !hit; i0 += kCmpBatch) {
    CmpFrame f[kCmpBatch];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < kCmpBatch; ++k)
      if (i0 + k < e) f[k] = cmp_frame(t, rms[i0 + k]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < kCmpBatch; ++k) {
      if (i0 + k < e && !hit) {
        loud = loud || !cmp_quiet(f[k]);
        att = cmp_step(att, f[k]);
        if (stop_on_match && cmp_bits(att) == cmp_bits(traj[i0 + k])) hit = true;
        else traj[i0 + k] = att;
      }
    }
  }
  if (matched) *matched = hit;
  if (any_above) *any_above = loud;
  return att;
}

// Chunk length of the chunked form: the requested length (0 = the default, one chunk per lane of a 1024-lane workgroup,
// at least 64 frames), raised until a clip holds at most kCmpMaxChunks chunks.
constexpr int kCmpLanes = 1024;
constexpr int kCmpMaxChunks = 2048;
RFX_CMP_HD int64_t cmp_chunk_frames(int64_t L, int64_t requested) {
  int64_t c = requested > 0 ? requested : (L + kCmpLanes - 1) / kCmpLanes;
  if (requested <= 0 && c < 64) c = 64;
  const int64_t least = (L + kCmpMaxChunks - 1) / kCmpMaxChunks;
  return c < least ? least : (c < 1 ? 1 : c);
}

// ---- the apply: x3 = attenuation != 0 ? audioop.mul(x2, 10 ** (-attenuation / 20)) : x2 ------------------------------------
// x2 is the compressor's input sample: normalize, then gain to -10 dBFS (two audioop.mul by the clip's factors).
struct CmpFactors {
  double f_norm, f_gain;
};
RFX_CMP_HD int cmp_x2(int x, const CmpFactors& f) { return pcm_mul(pcm_mul(x, f.f_norm), f.f_gain); }

// The factor as the DEVICE computes it.  It may differ from Python's 10 ** y (glibc pow) in the last bits, so the apply flags
// every product within `margin` of an integer - where a different last bit of the factor could move floor() - and the host
// recomputes those with pow (cmp_gain_host).  The emulator uses exp(y * ln 10), a formula with a different rounding, so that
// its flag-and-patch path is exercised on the CPU as well.
RFX_CMP_HD double cmp_gain_dev(double att) {
#if defined(__HIP_DEVICE_COMPILE__)
  return exp10(-att / 20.0);
#else
  return exp(-att / 20.0 * 2.302585092994045684);
#endif
}

// CPython's float ** is libm pow for a finite base and exponent: Python's 10 ** (float(-att) / 20), bit for bit (host only)
#if defined(__HIPCC__)
__host__
#endif
inline double cmp_gain_host(double att) { return pow(10.0, -att / 20.0); }

// the product x2 * g lies within `margin` of an integer (margin >= 0.5 takes every sample)
RFX_CMP_HD bool cmp_near_integer(double v, double margin) {
  const double d = v - floor(v);
  return d <= margin || 1.0 - d <= margin;
}

// one flagged sample: its index in the (N, L, C) batch, the exact attenuation of its frame, its x2; the host fills `value`
struct CmpFlag {
  int64_t index;
  double att;
  int32_t x2;
  int32_t value;
};

}  // namespace rfx
