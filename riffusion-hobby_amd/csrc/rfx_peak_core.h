// rfx_peak_core.h - arithmetic of the spectral-peak start of Griffin-Lim (include/rfx.h: rfx_peak_start, rfx_start_call_options;
// kernels in rfx_peak.hip), written once for the gfx950 kernels (hipcc) and the host emulator of the CPU tests
// (tests/emu/rfx_peak_emu.cpp, g++).
//
// The start builds phases from the magnitudes alone (single-pass spectrogram inversion with phase-vocoder peak tracking): in every
// frame the local maxima of |S| are the partials, a parabola through a maximum and its neighbours gives the partial's frequency in
// fractional bins, and a partial's phase advances from frame to frame by the mean of its old and new frequency times the hop.  Every
// bin of a frame takes the phase of the peak that owns it, times (-1)^bin: frames are referenced to their first sample, n_fft / 2
// before the centre, so a centred sinusoid alternates in sign from bin to bin.
//
// Decisions (which bin is a peak, which peak owns a bin) are float32 compares on the float32 inputs: exact, the same on every
// machine.  Arithmetic (position, phase chain) is double from the float32 inputs; phase is counted in turns; cosine and sine are
// formed in float32 from the fraction.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rfx_core.h"

namespace rfx {

constexpr int kPeakThreads = 1024;        // frame kernels (owners, angles): a workgroup per frame
constexpr int kPeakBins = 10;             // ... bins per thread at most: n_stft <= 10240 (the chain keeps two doubles per bin in 160 KiB)
constexpr int kPeakChainThreads = 512;    // chain kernel: a workgroup per row
constexpr int kPeakChainBins = 20;        // ... bins per thread at most
constexpr uint16_t kPeakNone = 0xFFFF;    // owner of a bin of a frame without peaks (peaks are bins 1 .. n_stft - 2 <= 65534)
constexpr int kPeakMaxBins = kPeakThreads * kPeakBins;
static_assert(kPeakChainThreads * kPeakChainBins == kPeakMaxBins, "both splits cover the same frame");

// largest non-NaN magnitude so far (-inf before the first); a NaN is skipped: every compare with it is false
RFX_HD float peak_max(float acc, float v) { return v > acc ? v : acc; }
RFX_HD float peak_threshold(float frame_max) { return 1e-5f * frame_max; }

// is bin k of a frame of F bins a peak?  a, b, c: the magnitudes of bins k - 1, k, k + 1 (a and c are not looked at for the two end bins)
RFX_HD bool peak_is3(float a, float b, float c, int k, int F, float thr) { return k >= 1 && k <= F - 2 && b > a && b >= c && b > thr; }
RFX_HD bool peak_is(const float* m, int k, int F, float thr) {
  return k >= 1 && k <= F - 2 && peak_is3(m[k - 1], m[k], m[k + 1], k, F, thr);
}

// owner of bin j: prev = the largest peak <= j (-1: none), next = the smallest peak > j (-1: none).  With the peaks p_0 < p_1 < ...
// bin j belongs to p_i for the smallest i with j <= (p_i + p_{i+1}) / 2 (integer division), to the last peak if there is none.
RFX_HD int peak_owner(int j, int prev, int next) {
  if (prev < 0) return next;  // (-1 when the frame has no peak at all)
  if (next < 0) return prev;
  return j <= ((prev + next) >> 1) ? prev : next;
}

// fractional position of peak p from its three magnitudes: the vertex of the parabola through them, at most half a bin away
RFX_HD double peak_pos(int p, float a, float b, float c) {
  const double da = a, db = b, dc = c;
  double delta = 0.5 * (da - dc) / (da - 2.0 * db + dc);  // (the denominator is negative for every peak)
  if (delta < -0.5) delta = -0.5;
  if (delta > 0.5) delta = 0.5;
  return (double)p + delta;
}

// turns per bin of frequency and frame: hop / n_fft, formed once per call (the chain multiplies by it: no division per peak)
RFX_HD double peak_turns_per_bin(int hop, int n_fft) { return (double)hop / (double)n_fft; }
// phase (turns, in [0, 1)) of peak p of this frame from the peak q of the previous frame that owns bin p
RFX_HD double peak_advance(double phi_q, double pos_q, double pos_p, double turns_per_bin) {
  const double x = phi_q + 0.5 * (pos_q + pos_p) * turns_per_bin;
  return x - floor(x);
}

// angles0 of bin k from its owner's phase
RFX_HD cf peak_angle(double phi, int k) {
  const float f = (float)phi;
  float s, c;
  sincosf(6.28318530717958647692f * f, &s, &c);
  return (k & 1) ? cf{-c, -s} : cf{c, s};
}

// ---- one frame, as the kernels walk it: m[F] the magnitudes in bin order -> own[F] the owning peak of every bin (kPeakNone
// everywhere for a frame without peaks).  The kernel does the same with a workgroup-wide scan; this is the definition.
RFX_HD void peak_frame_owners(const float* m, int F, uint16_t* own) {
  float mx = -INFINITY;
  for (int k = 0; k < F; ++k) mx = peak_max(mx, m[k]);
  const float thr = peak_threshold(mx);
  int prev = -1;
  for (int k = 0; k < F; ++k) {  // forward: the largest peak <= k, for now
    if (peak_is(m, k, F, thr)) prev = k;
    own[k] = prev < 0 ? kPeakNone : (uint16_t)prev;
  }
  int next = -1;
  for (int k = F - 1; k >= 0; --k) {  // backward: the smallest peak > k decides
    const int pv = own[k] == kPeakNone ? -1 : (int)own[k];
    const int o = peak_owner(k, pv, next);
    if (pv == k) next = k;
    own[k] = o < 0 ? kPeakNone : (uint16_t)o;
  }
}

}  // namespace rfx
