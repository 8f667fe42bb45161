// rfx_pcm_in_core.h - arithmetic of the int16 PCM front end of the encode (riffusion/util/audio_util.py: set_frame_rate,
// set_channels, the int16 -> float32 planar conversion), written once for both the gfx950 kernels (rfx_pcm_in.hip, hipcc) and
// the host emulator of the CPU tests (tests/emu/rfx_pcm_in_emu.cpp, g++).
//
// set_frame_rate is audioop.ratecv(data, 2, C, inrate, outrate, None): weightA = 1, weightB = 0, a fresh state.  With
// a = inrate / g, b = outrate / g, g = gcd(inrate, outrate), x[-1] = 0 and samples widened as x << 16, audioop's loop
//     d = -b;  for (;;) { while (d < 0) { take the next input frame or stop; d += b; }
//                         while (d >= 0) { emit (prev * d + cur * (b - d)) / b; d -= a; } }
// has the closed form
//     K    = floor((L - 1) * b / a) + 1             output frames of L input frames
//     n_k  = 1 + ceil(k * a / b)                    input frames consumed when output k is emitted
//     d_k  = (n_k - 1) * b - k * a                  in [0, b)
//     out  = trunc((x[n_k - 2] << 16) * d_k + (x[n_k - 1] << 16) * (b - d_k)) / b) >> 16
// audioop forms the numerator and the quotient in double and truncates with an (int) cast.  While b < 2^21 the numerator stays
// below 2^15 * 2^16 * 2^21 = 2^52: it is exact in double, and a correctly rounded quotient of an exact numerator cannot reach the
// next integer (the nearest multiple of 1/b is further away than half an ulp of a value below 2^31): the double quotient,
// truncated, IS the integer truncating quotient (audio_util.ratecv_np computes that one; the tests hold the two together).
// The entry points refuse reduced rates of kRatecvRateLimit = 2^20 or more.
// Consecutive outputs follow audioop's own recurrence (ratecv_advance): one 64-bit division for a thread's first output, none
// after it.
//
// set_channels is audioop.tomono(data, 2, 0.5, 0.5) = floor(clip(l * 0.5 + r * 0.5)) in double (both products and their sum are
// exact: no rounding to contract) and audioop.tostereo(data, 2, 1, 1), which writes every sample twice.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RFX_PCM_IN_HD __host__ __device__ __forceinline__
#else
#define RFX_PCM_IN_HD inline __attribute__((always_inline))
#endif

namespace rfx {

constexpr int64_t kRatecvRateLimit = (int64_t)1 << 20;  // reduced rates must stay below this
constexpr int kRatecvRun = 8;                           // consecutive output frames one thread of the resample kernel produces

RFX_PCM_IN_HD int64_t pcm_in_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the reduced rates of a conversion
struct RatecvRates {
  int64_t a, b;  // inrate / g, outrate / g
};
RFX_PCM_IN_HD RatecvRates ratecv_rates(int64_t in_rate, int64_t out_rate) {
  const int64_t g = pcm_in_gcd(in_rate, out_rate);
  return RatecvRates{in_rate / g, out_rate / g};
}

// output frames of L >= 1 input frames
RFX_PCM_IN_HD int64_t ratecv_out_frames(int64_t L, RatecvRates r) { return (L - 1) * r.b / r.a + 1; }

// where output k stands: n input frames consumed (cur = x[n - 1], prev = x[n - 2], x[-1] = 0), d = audioop's counter
struct RatecvState {
  int64_t n, d;
};
RFX_PCM_IN_HD RatecvState ratecv_state(int64_t k, RatecvRates r) {
  const int64_t ka = k * r.a;
  const int64_t n = 1 + (ka + r.b - 1) / r.b;
  return RatecvState{n, (n - 1) * r.b - ka};
}
// from output k to output k + 1: audioop's loop; where a frame of output skips many of input (a > 4 b) its steps are counted
// by one division instead
RFX_PCM_IN_HD void ratecv_advance(RatecvState& s, RatecvRates r) {
  s.d -= r.a;
  if (s.d >= 0) return;
  if (r.a <= 4 * r.b) {
    while (s.d < 0) {
      s.d += r.b;
      ++s.n;
    }
  } else {
    const int64_t steps = (r.b - 1 - s.d) / r.b;
    s.d += steps * r.b;
    s.n += steps;
  }
}

// one output sample of one channel from the two input samples around it: audioop's own expression - the exact numerator
// (below 2^52, see above) divided in double, truncated by the cast - then SETSAMPLE32's arithmetic shift
RFX_PCM_IN_HD int ratecv_interp(int prev, int cur, int64_t d, int64_t b) {
  const int64_t num = ((int64_t)prev * 65536) * d + ((int64_t)cur * 65536) * (b - d);
#if defined(__HIP_DEVICE_COMPILE__)
  const int q = (int)__ddiv_rn((double)num, (double)b);
#else
  const int q = (int)((double)num / (double)b);
#endif
  return q >> 16;
}

// audioop.tomono(., 0.5, 0.5) of one frame
RFX_PCM_IN_HD int pcm_tomono(int l, int r) {
  double v = (double)l * 0.5 + (double)r * 0.5;
  if (v > 32767.0) v = 32767.0;
  else if (v < -32768.0) v = -32768.0;
  return (int)floor(v);
}

// channel c (of C_out) of stored frame `frame` of an (L, C_in) recording after the mix (C_in, C_out in {1, 2}); frame -1 is
// ratecv's zero state
RFX_PCM_IN_HD int pcm_mixed_sample(const int16_t* pcm, int64_t frame, int c, int C_in, int C_out) {
  if (frame < 0) return 0;
  if (C_in == C_out) return pcm[frame * C_in + c];
  if (C_out == 1) return pcm_tomono(pcm[2 * frame], pcm[2 * frame + 1]);
  return pcm[frame];
}

// One thread's run of the resample: `count` (1 .. kRatecvRun) consecutive output frames from k0, C_OUT channels each, into
// res[j * C_OUT + c] (entries past the run are zeroed).  load(frame, v) fetches the mixed frame `frame` (-1: zero) as
// CC = min(C_in, C_OUT) channel values - the kernel's dword loads, the emulator's pcm_mixed_sample.  The first frame's state
// comes from the closed form, the others from the recurrence; an advance by one input frame shifts cur into prev and loads
// one frame, a longer one reloads both, none keeps both.  The kernel and the emulator both run exactly this function.
template <int C_OUT, int CC, class Load>
RFX_PCM_IN_HD void ratecv_run(int64_t k0, int count, RatecvRates r, Load load, int16_t* res) {
  RatecvState s = ratecv_state(k0, r);
  int prev[2], cur[2];
  load(s.n - 2, prev);
  load(s.n - 1, cur);
#pragma unroll
  for (int j = 0; j < kRatecvRun; ++j) {
    if (j < count) {
#pragma unroll
      for (int c = 0; c < C_OUT; ++c) res[j * C_OUT + c] = (int16_t)ratecv_interp(prev[c < CC ? c : 0], cur[c < CC ? c : 0], s.d, r.b);
      if (j + 1 < count) {
        const int64_t n_before = s.n;
        ratecv_advance(s, r);
        if (s.n == n_before + 1) {
          prev[0] = cur[0], prev[1] = cur[1];
          load(s.n - 1, cur);
        } else if (s.n != n_before) {
          load(s.n - 2, prev);
          load(s.n - 1, cur);
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < C_OUT; ++c) res[j * C_OUT + c] = 0;
    }
  }
}

}  // namespace rfx
