// rfx_guide_core.h - arithmetic of the guide staging (rfx_guide.hip), written once for the gfx950 kernels (hipcc) and the host
// emulators of the CPU tests (tests/emu/rfx_guide_emu.cpp, tests/emu/rfx_guide_bwd_emu.cpp, tests/emu/rfx_hold_emu.cpp, g++).  Below the
// staging: the projection of the guided decode's backward; the held frames of a guided call and the list of the frames that are not held.
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

// ---- the guided decode's backward (include/rfx.h: rfx_griffinlim_guided_backward) -------------------------------------------------
// At zero iterations a guided call returns w = ISTFT(S u), u = a / (|a| + 1e-16) the unit phase of a = STFT(staged guide): linear
// in S.  For an incoming g_w, with G the gradient of the synthesis with respect to its complex input (rfx_istft_backward), the
// gradient with respect to a magnitude is g_S = Re(conj(u) G) = u_re G_re + u_im G_im, per position of the slot cube: a conjugate
// slot holds conj(a) and conj(G) and gives the same number.  u is the forward's projection rule at S = 1 (rfx_core.h: gl_project)
// in its IEEE form, on the device too, so that tests/emu/rfx_guide_bwd_emu.cpp gives the kernel's bits; the forward's launch forms
// the same factor with one v_rsq_f32 (1 ulp).  a == 0 gives u = 0 in both: a silent bin, and every bin of a silent guide row,
// passes no gradient.  The guide is staged as the forward stages it - fit and range above - with no kernel factor (c = 1): the
// forward's own factor row_scale[2 r] = 2^-j is a power of two that its analysis multiplies back in, so a is the forward's a whatever
// the magnitudes' range is; its eps is the same 1e-16 times 2^-j (row_scale[2 r + 1]) and matters only for 0 < |a| within a few
// orders of it, far below what a ranged guide's bins hold.  The backward takes 1e-16 itself and needs no range table.  g_S is linear
// in g_w with power-of-two-exact roundings.
RFX_HD cf guide_unit(cf a) { return gl_project_ieee(a, 1.f); }
RFX_HD float guide_project(cf a, cf G) {
  const cf u = guide_unit(a);
  return fmaf(u.re, G.re, u.im * G.im);
}

// ---- held frames (include/rfx.h: rfx_held_call_options) -----------------------------------------------------------------------------
// A guided call may hold the first `head` and the last `tail` frames of a row at the guide's phase: after every projection the
// angles of a held frame are set back to a0, so its synthesis frame IFFT(|S_t| a0_t) is what launch 0 wrote, at every iteration.
// Launches 1 .. n_iter therefore walk a list of the FREE frames only and leave the held frames' entries of the frame buffer alone.
// Any int32 pair is legal: h = clamp(head, 0, T), l = clamp(tail, 0, T - h); the free frames of a row are t in [h, T - l).
struct HoldSpan {
  int first, count;  // the free frames of a row: first <= t < first + count
};
RFX_HD HoldSpan hold_free_span(int head, int tail, int T) {
  const int h = head < 0 ? 0 : head > T ? T : head;
  const int rest = T - h;
  const int l = tail < 0 ? 0 : tail > rest ? rest : tail;
  return HoldSpan{h, rest - l};
}
RFX_HD bool hold_is_held(int t, int head, int tail, int T) {
  const HoldSpan s = hold_free_span(head, tail, T);
  return t < s.first || t >= s.first + s.count;
}

// The free-frame list: the global indices row T + t of the free frames, increasing, in list[0 .. count), and the count itself at
// list[B T] (a fixed place: the frame kernels read it without knowing it).  Built by three launches over CHUNKS of kHoldChunkRows
// rows (rfx_guide.hip): the chunks' free counts, one workgroup's exclusive scan over them, the fill.  Thread `tid` of a chunk's
// workgroup owns the kHoldRowsPerThread consecutive rows from hold_thread_row; the chunks' offsets live behind the count.
// B T < 2^31 (the entry points check it), so every count and offset fits an int; products with T are formed in 64 bits.
constexpr int kHoldThreads = 256;
constexpr int kHoldRowsPerThread = 4;
constexpr int kHoldChunkRows = kHoldThreads * kHoldRowsPerThread;
RFX_HD long long hold_chunks(long long B) { return (B + kHoldChunkRows - 1) / kHoldChunkRows; }
RFX_HD long long hold_thread_row(long long chunk, int tid, int e) { return chunk * kHoldChunkRows + (long long)tid * kHoldRowsPerThread + e; }
RFX_HD long long hold_count_at(long long B, int T) { return B * T; }
RFX_HD long long hold_chunk_offsets_at(long long B, int T) { return B * T + 1; }
// int32 words of the list, its count and the chunk offsets, rounded up to whole 16 bytes
RFX_HD size_t hold_list_words(long long B, int T) { return (size_t)((B * T + 1 + hold_chunks(B) + 3) / 4 * 4); }
// the free frames of row `row`, or none behind the batch
RFX_HD HoldSpan hold_row_span(const int32_t* hold, long long row, long long B, int T) {
  return row < B ? hold_free_span(hold[2 * row], hold[2 * row + 1], T) : HoldSpan{0, 0};
}
// entry i of a row's part of the list
RFX_HD int hold_list_entry(long long row, int T, const HoldSpan& s, int i) { return (int)(row * T + s.first + i); }

}  // namespace rfx
