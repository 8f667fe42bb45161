// rfx_pcm_core.h - per-sample and per-clip arithmetic of the int16 PCM post-processing (riffusion/util/audio_util.py:
// apply_filters without compression, stitch_segments), written once for both the gfx950 kernels (rfx_pcm.hip, hipcc) and
// the host emulator of the CPU tests (tests/emu/rfx_pcm_emu.cpp, g++).
//
// Every step is CPython's `audioop` on 16-bit samples, which is what pydub.AudioSegment and PcmSegment call:
//   mul(x, f)   floor(clip((double)x * f, -32768, 32767)); NaN (0 * inf) gives 0, as CPython's (int) cast of NaN
//               (INT_MIN on x86-64) stored into 16 bits does
//   add(a, b)   a + b saturated to [-32768, 32767]
//   rms         (unsigned)sqrt((double)sum(x^2) / n): the double sum is exact while it stays <= 2^53, i.e. for n < 2^23
//   max         largest |x|, with |-32768| = 32768
// The transcendentals of the filters (10 ** (dB / 20), 20 * log10(r)) are never evaluated here: the host tabulates them
// with Python's own expressions (gain by rms, boost by peak, 32769 doubles each) and the device only indexes the tables.
// No expression below has the shape a * b + c, and the products go through pcm_dmul, so nothing can be contracted into an
// FMA; the division and the square root are the correctly rounded ones on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RFX_PCM_HD __host__ __device__ __forceinline__
#else
#define RFX_PCM_HD inline __attribute__((always_inline))
#endif

namespace rfx {

constexpr int kPcmTableSize = 32769;  // gain_by_rms / boost_by_peak are indexed 0..32768

// one piece of a stitched output (riffusion/util/audio_util.py:stitch_plan): frames [out_start, next piece's out_start)
// kind 0: copy of source a; kind 1: add(mul(a, a_gain), mul(b, b_gain)).  A source is frame a_off + t of clip a_clip, or
// silence when the clip index is negative.  56 bytes, the layout of audio_util.STITCH_PIECE_DTYPE.
struct PcmPiece {
  int64_t out_start;
  int64_t a_off;
  int64_t b_off;
  double a_gain;
  double b_gain;
  int32_t a_clip;
  int32_t b_clip;
  int32_t kind;
  int32_t pad;
};

RFX_PCM_HD double pcm_dmul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}

// audioop.mul on one 16-bit sample
RFX_PCM_HD int pcm_mul(int x, double f) {
  double v = pcm_dmul((double)x, f);
  if (v != v) return 0;
  if (v > 32767.0) v = 32767.0;
  else if (v < -32768.0) v = -32768.0;
  return (int)floor(v);
}

// audioop.add on one 16-bit sample
RFX_PCM_HD int pcm_add(int a, int b) {
  const int v = a + b;
  return v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
}

// audioop.rms from the exact sum of squares of n samples (n > 0)
RFX_PCM_HD unsigned pcm_rms(int64_t sumsq, int64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)__dsqrt_rn(__ddiv_rn((double)sumsq, (double)n));
#else
  return (unsigned)sqrt((double)sumsq / (double)n);
#endif
}

// The two factors of apply_filters(compression=False) = apply_gain(-12 - dBFS).normalize(0.1) for a clip whose samples have the
// given sum of squares, count, maximum and minimum.  mul(., f1) is monotone in the sample, so the peak after the first gain is
// reached at the clip's maximum or minimum.
struct PcmFactors {
  double f1, f2;
};
RFX_PCM_HD PcmFactors pcm_filter_factors(int64_t sumsq, int64_t n, int xmax, int xmin, const double* gain_by_rms,
                                         const double* boost_by_peak) {
  const unsigned rms = n > 0 ? pcm_rms(sumsq, n) : 0u;
  const double f1 = gain_by_rms[rms];
  const int a = pcm_mul(xmax, f1), b = pcm_mul(xmin, f1);
  const int pa = a < 0 ? -a : a, pb = b < 0 ? -b : b;
  const int peak = pa > pb ? pa : pb;
  return PcmFactors{f1, boost_by_peak[peak]};
}

RFX_PCM_HD int16_t pcm_filter_sample(int x, PcmFactors f) { return (int16_t)pcm_mul(pcm_mul(x, f.f1), f.f2); }

// index of the piece that holds output frame `frame`: the last one with out_start <= frame (pieces[0].out_start == 0)
RFX_PCM_HD int pcm_find_piece(const PcmPiece* pieces, int n_pieces, int64_t frame) {
  int lo = 0, hi = n_pieces - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pieces[mid].out_start <= frame) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// channel ch of output frame `frame` of a stitch of N clips of L frames, C channels ((N, L, C) int16)
RFX_PCM_HD int16_t pcm_stitch_sample(const PcmPiece& p, int64_t frame, int ch, const int16_t* pcm, int64_t L, int C) {
  const int64_t t = frame - p.out_start;
  const int a = p.a_clip >= 0 ? (int)pcm[((int64_t)p.a_clip * L + p.a_off + t) * C + ch] : 0;
  if (p.kind == 0) return (int16_t)a;
  const int b = p.b_clip >= 0 ? (int)pcm[((int64_t)p.b_clip * L + p.b_off + t) * C + ch] : 0;
  return (int16_t)pcm_add(pcm_mul(a, p.a_gain), pcm_mul(b, p.b_gain));
}

}  // namespace rfx
