// rfx_resample_core.h - the windowed-sinc resampler (include/rfx.h "SINC RESAMPLE": rfx_resample_sinc_frames, rfx_resample_sinc_table,
// rfx_resample_sinc), written once for the kernel of rfx_resample.hip, the host entries of rfx_api_resample.hip and the host emulator
// of the CPU tests (tests/emu/rfx_resample_emu.cpp).  It states
//   - the reduced pair, the filter's width and the output length;
//   - the weight of a tap, in double, as torchaudio writes it, and which taps are dropped;
//   - the polyphase table: per phase the first input offset, then the weights tap-major;
//   - one output sample: the taps in ascending order, one fmaf each.
//
// Definition (torchaudio.functional.resample, resampling_method = "sinc_interp_hann"): o = orig / g, n = new / g, g = gcd(orig, new),
// base = min(o, n) rolloff, width = ceil(lpw o / base).  L input samples give K = ceil(n L / o) output samples; output j = q n + p,
// 0 <= p < n, is
//     sum over i in [0, 2 width + o) of x[q o + i - width] k_p[i],    x zero outside [0, L)
//     k_p[i] = sin(pi t) / (pi t)  cos^2(pi t / (2 lpw))  base / o,   t = clamp((-p / n + (i - width) / o) base, -lpw, lpw)
// the dense (n, 2 width + o) kernel torchaudio hands to conv1d with stride o.
// DROPPED TAPS.  Where |t| reaches lpw the clamp makes the weight cos^2(pi / 2) sin(pi lpw) / (pi lpw) base / o: not zero in floating
// point, but its window factor alone is 4e-33 in float64.  Those taps are dropped here: a phase keeps the taps with |t| < lpw, a run of
// about 2 lpw o / base + 1 consecutive i, 13 to 25 of the 2 width + o.  tests/test_resample_cpu.py holds every dropped tap of the dense
// transcription below 1e-30.
// The weights are computed in double and rounded once to float32 - the kernel torchaudio.transforms.Resample holds - and a sample is
// accumulated in float32 in ascending tap order with one fmaf per tap, on the device and in the emulator alike.  A tap whose sample
// lies outside the row, and a zero-filled tap of a phase shorter than ntaps, still takes its fmaf (with a zero factor), so what a
// row gives does not depend on how the zeros came about: rows padded with zeros and rows that end give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rfx_core.h"

namespace rfx {

// the table of a pair may take this many bytes (n ntaps floats): every integer semitone shift within +-12 at sample rates of 8 to
// 96 kHz stays below 8.5 MiB (n up to 96000 phases, 13 to 25 taps; tests/test_resample_cpu.py walks them all)
constexpr int64_t kRsMaxTableBytes = (int64_t)16 << 20;

struct RsGeom {
  int64_t o, n;  // the reduced pair
  double base;   // min(o, n) rolloff
  int64_t width;
  double lpw;
};
inline int64_t rs_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// false: a frequency or the width is not positive, or rolloff is not in (0, 1]
inline bool rs_geom(int orig, int neu, int lpw, double rolloff, RsGeom* g) {
  if (orig < 1 || neu < 1 || lpw < 1 || !(rolloff > 0.0) || !(rolloff <= 1.0)) return false;
  const int64_t d = rs_gcd(orig, neu);
  g->o = orig / d;
  g->n = neu / d;
  g->base = (double)(g->o < g->n ? g->o : g->n) * rolloff;
  g->width = (int64_t)ceil((double)lpw * (double)g->o / g->base);
  g->lpw = (double)lpw;
  return true;
}
// K = ceil(n L / o), exact in integers (n L < 2^62); -1: past 2^31 - 1
inline int64_t rs_frames(int64_t L, int64_t o, int64_t n) {
  const int64_t K = (n * L + o - 1) / o;
  return K <= 2147483647LL ? K : -1;
}
// t of tap i of phase p before the clamp, operation for operation what torchaudio computes in float64
inline double rs_t(const RsGeom& g, int64_t p, int64_t i) {
  return ((double)(-p) / (double)g.n + (double)(i - g.width) / (double)g.o) * g.base;
}
inline bool rs_kept(const RsGeom& g, double t) { return t > -g.lpw && t < g.lpw; }
// the weight at t (after the clamp), in double
inline double rs_weight(const RsGeom& g, double t) {
  const double pi = 3.14159265358979323846;
  if (t < -g.lpw) t = -g.lpw;
  if (t > g.lpw) t = g.lpw;
  const double c = cos(t * pi / g.lpw / 2.0), window = c * c;
  t *= pi;
  const double s = t == 0.0 ? 1.0 : sin(t) / t;
  return s * (window * (g.base / (double)g.o));
}
// the kept taps of phase p: [*i0, *i0 + count) of the dense kernel's [0, 2 width + o).  The candidates are the integers around
// width + o p / n -+ o lpw / base; each is decided by rs_t itself, so the run is exactly the dense kernel's taps with |t| < lpw.
inline int rs_support(const RsGeom& g, int64_t p, int64_t* i0) {
  const double centre = (double)g.width + (double)g.o * (double)p / (double)g.n, half = (double)g.o * g.lpw / g.base;
  int64_t lo = (int64_t)floor(centre - half) - 2, hi = (int64_t)ceil(centre + half) + 2;
  if (lo < 0) lo = 0;
  if (hi > 2 * g.width + g.o - 1) hi = 2 * g.width + g.o - 1;
  while (lo <= hi && !rs_kept(g, rs_t(g, p, lo))) ++lo;
  while (hi >= lo && !rs_kept(g, rs_t(g, p, hi))) --hi;
  *i0 = lo;
  return (int)(hi - lo + 1);
}
// ntaps: the longest run over the phases
inline int rs_ntaps(const RsGeom& g) {
  int most = 0;
  for (int64_t p = 0; p < g.n; ++p) {
    int64_t i0;
    const int c = rs_support(g, p, &i0);
    most = c > most ? c : most;
  }
  return most;
}
// the table: first[p] = i0 - width, the offset of tap 0 from q o (negative at a row's start); taps[k n + p] the weight of tap
// i0 + k rounded to float32, 0 past the phase's run
inline void rs_table(const RsGeom& g, int ntaps, int32_t* first, float* taps) {
  for (int64_t p = 0; p < g.n; ++p) {
    int64_t i0;
    const int c = rs_support(g, p, &i0);
    first[p] = (int32_t)(i0 - g.width);
    for (int k = 0; k < ntaps; ++k) taps[(int64_t)k * g.n + p] = k < c ? (float)rs_weight(g, rs_t(g, p, i0 + k)) : 0.f;
  }
}

// ---- one output sample ------------------------------------------------------------------------------------------------------------------
// where output j of a row starts reading: phase p = j mod n, input index q o + first[p] with q = j / n (64-bit: q o can pass 2^31)
struct RsStart {
  int p;
  int64_t at;
};
RFX_HD RsStart rs_start(int64_t j, int o, int n, const int32_t* __restrict__ first) {
  const int64_t q = j / n;
  const int p = (int)(j - q * n);
  return RsStart{p, q * (int64_t)o + (int64_t)first[p]};
}
// a row's sample at index i, zero outside [0, valid)
RFX_HD float rs_sample(const float* __restrict__ row, int64_t i, int64_t valid) { return i >= 0 && i < valid ? row[i] : 0.f; }
// One output sample of each of R rows that share j: acc[r] = sum over k, ascending, of rows[r][at + k] taps[k n] by fmaf - the weight
// is read once for the R rows.  A run that lies inside [0, valid) skips the per-sample bounds test; the arithmetic is the same.
template <int R>
RFX_HD void rs_accumulate(const float* const* rows, int64_t valid, int64_t at, const float* __restrict__ taps, int64_t n, int ntaps, float* acc) {
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  if (at >= 0 && at + ntaps <= valid) {
    for (int k = 0; k < ntaps; ++k) {
      const float w = taps[(int64_t)k * n];
      for (int r = 0; r < R; ++r) acc[r] = fmaf(rows[r][at + k], w, acc[r]);
    }
  } else {
    for (int k = 0; k < ntaps; ++k) {
      const float w = taps[(int64_t)k * n];
      for (int r = 0; r < R; ++r) acc[r] = fmaf(rs_sample(rows[r], at + k, valid), w, acc[r]);
    }
  }
}

}  // namespace rfx
