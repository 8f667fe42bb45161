// rfx_resize_core.h - PIL.Image.resize of RGB uint8 images (Pillow's libImaging/Resample.c, 8 bits per channel), written
// once for the gfx950 kernels (rfx_resize.hip, hipcc) and the host emulator of the CPU tests (tests/emu/rfx_resize_emu.cpp,
// g++).
//
// Pillow resamples with a separable convolution in fixed point:
//   * per output column (row), in double: scale = in / out, filterscale = max(scale, 1), support = filter support *
//     filterscale, center = (x + 0.5) * scale, taps [xmin, xmin + xmax) with xmin = max(int(center - support + 0.5), 0),
//     xmax = min(int(center + support + 0.5), in) - xmin, weights filter((i + xmin - center + 0.5) / filterscale) divided by
//     their sum (summed in order), then rounded half away from zero to PRECISION_BITS = 22 fractional bits;
//   * per output byte: ss = 2^21 + sum in[xmin + i] * k[i] in int32, clamp(ss >> 22, 0, 255);
//   * the horizontal pass first, its result stored as uint8, then the vertical pass over it; a pass whose size does not
//     change is skipped.
// The coefficients are planned on the host (rsz_coefficients) with the same double operations and libm's sin, contraction
// off, so the tables are Pillow's bit for bit; the device only runs the integer part (rsz_pixel_taps / rsz_clip8).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RFX_RSZ_HD __host__ __device__ __forceinline__
#else
#define RFX_RSZ_HD inline __attribute__((always_inline))
#endif

namespace rfx {

// PIL.Image.Resampling values
constexpr int kRszLanczos = 1;
constexpr int kRszBilinear = 2;
constexpr int kRszBicubic = 3;
constexpr int kRszPrecisionBits = 22;
constexpr int kRszMaxSize = 16384;  // per axis, in and out (a staged input row is at most 48 KiB of LDS)

// Pillow's filter supports; 0 for a filter this library does not implement
inline double rsz_support(int filter) {
  return filter == kRszBilinear ? 1.0 : filter == kRszBicubic ? 2.0 : filter == kRszLanczos ? 3.0 : 0.0;
}

// ---- Pillow's filter functions (Resample.c bilinear_filter, bicubic_filter with a = -0.5, sinc_filter, lanczos_filter) ----
inline double rsz_filter(int filter, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (filter == kRszBilinear) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
  }
  if (filter == kRszBicubic) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  // lanczos: sinc(x) * sinc(x / 3) on [-3, 3)
  if (-3.0 <= x && x < 3.0) {
    double s0 = 1.0, s1 = 1.0;
    if (x != 0.0) {
      const double t = x * M_PI;
      s0 = sin(t) / t;
    }
    const double y = x / 3;
    if (y != 0.0) {
      const double t = y * M_PI;
      s1 = sin(t) / t;
    }
    return s0 * s1;
  }
  return 0.0;
}

inline int rsz_ksize(int in_size, int out_size, int filter) {
  double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(rsz_support(filter) * filterscale) * 2 + 1;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc: bounds[2 x] = xmin, bounds[2 x + 1] = xmax (the tap count), kk[x *
// ksize + i] the fixed-point weights (0 past xmax).  `wbuf` holds ksize doubles.  Returns ksize.  Host only.
inline int rsz_coefficients(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, double* wbuf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = rsz_support(filter) * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double w = rsz_filter(filter, (x + xmin - center + 0.5) * ss);
      wbuf[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) wbuf[x] /= ww;
    int32_t* k = kk + (int64_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      const double w = x < xmax ? wbuf[x] : 0.0;
      k[x] = w < 0 ? (int32_t)(-0.5 + w * (1 << kRszPrecisionBits)) : (int32_t)(0.5 + w * (1 << kRszPrecisionBits));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

// ---- the integer part, per output byte (host and device) ------------------------------------------------------------------
RFX_RSZ_HD int rsz_clip8(int ss) {
  ss >>= kRszPrecisionBits;  // arithmetic shift: Resample.c clip8
  return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// the taps of output column (row) o, clamped to the input: a table that is not rsz_coefficients' cannot make a read leave it
RFX_RSZ_HD void rsz_span(const int32_t* bounds, int o, int in_size, int ksize, int* lo, int* n) {
  int a = bounds[2 * o], c = bounds[2 * o + 1];
  a = a < 0 ? 0 : (a > in_size - 1 ? in_size - 1 : a);
  c = c > in_size - a ? in_size - a : c;
  c = c > ksize ? ksize : c;
  *lo = a;
  *n = c < 0 ? 0 : c;
}

// one output pixel's three channels: src points at input pixel xmin's first byte, consecutive taps `stride` bytes apart
template <typename Src>
RFX_RSZ_HD void rsz_pixel_taps(Src src, int stride, const int32_t* k, int n, int* r, int* g, int* b) {
  int s0 = 1 << (kRszPrecisionBits - 1), s1 = s0, s2 = s0;
  for (int i = 0; i < n; ++i) {
    const int w = k[i];
    s0 += (int)src[i * stride + 0] * w;
    s1 += (int)src[i * stride + 1] * w;
    s2 += (int)src[i * stride + 2] * w;
  }
  *r = rsz_clip8(s0);
  *g = rsz_clip8(s1);
  *b = rsz_clip8(s2);
}

// one output byte of a column pass: taps `stride` bytes apart
template <typename Src>
RFX_RSZ_HD int rsz_byte_taps(Src src, int64_t stride, const int32_t* k, int n) {
  int s = 1 << (kRszPrecisionBits - 1);
  for (int i = 0; i < n; ++i) s += (int)src[i * stride] * k[i];
  return rsz_clip8(s);
}

}  // namespace rfx
