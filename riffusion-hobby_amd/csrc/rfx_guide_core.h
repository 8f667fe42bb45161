// rfx_guide_core.h - arithmetic of the guide staging (rfx_guide.hip), written once for the gfx950 kernels (hipcc) and the host
// emulator of the CPU tests (tests/emu/rfx_guide_emu.cpp, g++).
//
// A guided Griffin-Lim call (include/rfx.h: rfx_guided_call_options) starts from the phase of a caller's waveform instead of random
// phases: its first launch is MODE 1 - a = STFT(x), normalise, ISTFT(|S| a / |a|) - with x the guide.  Staging brings row r of the
// caller's (B, guide_samples) tensor into the buffer that launch reads:
//   fit    the row is cut to L samples or zero-padded at its end to L (its STFT then has exactly T frames); the buffer's row is
//          Lpad >= L floats and the padding behind L is zeroed as well;
//   range  only the direction of STFT(guide) matters, so the row is multiplied by the power of two 2^n that brings its peak
//          (largest |sample| of the fitted row) into [2^(kGuidePeakExp - 1), 2^kGuidePeakExp): re^2 + im^2 of the analysis can then
//          neither overflow (|a| <= window length x peak) nor come near the projection's eps^2, whatever units the guide is in;
//   units  the specialised engine's kernels multiply what they load by row_scale[2 r] = 2^-j (GlArgs::row_scale), so the value
//          stored for them is the ranged sample divided by that factor; the generic, row-family and chirp-z kernels analyse their
//          buffer as it is (their fold applies the factor) and get the ranged sample itself.
// Every factor is a power of two: the products are exact unless a sample lies so far below the row's peak that it leaves float32's
// normal range (2^140 below it at j = 0, 2^40 at the extreme j = -100), and guide x 2^m stages the same bytes as guide.
//
// The shape of the peak reduction is a function of Lpad alone: the row is cut into chunks of kGuideChunk samples, one workgroup of
// kGuideThreads each takes its chunk's peak (guide_chunk_peak: thread t the vectors t, t + kGuideThreads, ...; max is exact in any
// order), and every workgroup of the second launch takes the largest of the row's chunk peaks.  No atomics, nothing depends on B,
// on the grid or on the row's place in the call.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rfx_core.h"

namespace rfx {

constexpr int kGuideThreads = 256;
constexpr int kGuideVecsPerThread = 4;
constexpr int kGuideChunk = kGuideThreads * kGuideVecsPerThread * 4;  // samples per workgroup: 16 KiB
constexpr int kGuidePeakExp = 15;  // the ranged peak lies in [2^14, 2^15): the amplitude of 16-bit audio

RFX_HD int guide_chunks(int Lpad) { return (Lpad + kGuideChunk - 1) / kGuideChunk; }

// sample p of the fitted row: the guide's where it has one (n_valid = min(guide_samples, L)), zero behind it
RFX_HD float guide_fit(const float* row, int n_valid, int p) { return p < n_valid ? row[p] : 0.f; }

// |sample| into a running peak; NaN is skipped, as fmaxf does (a NaN sample stays NaN in what is staged: garbage in, garbage out)
RFX_HD float guide_peak_step(float peak, float x) { return fmaxf(peak, fabsf(x)); }

// the two halves of 2^n for a row's peak (n = kGuidePeakExp - k, peak in [2^(k-1), 2^k); n reaches 164 for a denormal peak, so it
// is applied as two factors of at most 2^82), and the reciprocal of the kernels' own factor (1 when they apply none).
// A silent row (peak 0) keeps factors of 1 and stages zeros.
struct GuideScale {
  float a, b, c;
};
RFX_HD GuideScale guide_scale(float peak, float ks) {
  GuideScale s{1.f, 1.f, 1.f};
  if (peak > 0.f) {
    int k = 129;
    if (peak < __builtin_inff()) (void)frexpf(peak, &k);
    const int n = kGuidePeakExp - k, n1 = n / 2;
    s.a = ldexpf(1.f, n1);
    s.b = ldexpf(1.f, n - n1);
  }
  if (ks > 0.f) s.c = 1.f / ks;  // ks = 2^-j, |j| <= 100 (range_exponents): exact
  return s;
}
RFX_HD float guide_apply(float x, const GuideScale& s) { return ((x * s.a) * s.b) * s.c; }

}  // namespace rfx
