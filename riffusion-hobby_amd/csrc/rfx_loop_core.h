// rfx_loop_core.h - index rules and envelope of a LOOP decode (include/rfx.h: rfx_loop_call_options) and the read position and length
// rule of a LOOP ENCODE (rfx_stft_loop and the other *_loop forward entries), written once for the gfx950 kernels (hipcc) and the host
// emulators of the CPU tests (tests/emu/rfx_loop_emu.cpp, tests/emu/rfx_loop_fwd_emu.cpp, g++).
//
// A loop call treats a row of T frames as the STFT of a signal with period P = hop T.  With h = n_fft / 2, left = (n_fft - win) / 2
// and the window w zero-padded to n_fft:
//   analysis   frame t, element i reads x[(hop t + i - h) mod P]
//   synthesis  y[m] = (sum of w[i] frame_t[i] over hop t + i - h = m mod P) / env[m],   env[m] the same sum of w[i]^2
// Valid when P >= n_fft: a frame then covers the period at most once, every position a frame reads lies in [-P, 2 P), and the wrap
// is one conditional add or subtract.
//
// The fold, per output sample m: with q = m + h - left, window sample j = q - hop t of frame t covers m for the UNWRAPPED frame
// indices t in [tlo, thi] = [ceil((q - win + 1) / hop), floor(q / hop)] - tlo may be negative, thi may pass T - 1 - and the frame
// read is t mod T.  The chain runs from tlo (the oldest covering frame) to thi: its length and the window samples it meets depend
// on m mod hop alone, so rolling the frames by k rolls the audio by k hop bit for bit.  env is a table of hop entries for the same
// reason, summed in the same order.
#pragma once
#include <stddef.h>
#include "rfx_core.h"

namespace rfx {

RFX_HD bool loop_valid(int hop, int T, int n_fft) { return T > 0 && (long long)hop * T >= n_fft; }
RFX_HD int loop_min_frames(int hop, int n_fft) { return (n_fft + hop - 1) / hop; }

// p mod P for p in [-P, 2 P)
RFX_HD int loop_wrap(int p, int P) {
  if (p < 0) p += P;
  if (p >= P) p -= P;
  return p;
}

// ---- LOOP ENCODE: the analysis above as the forward entries run it (include/rfx.h: rfx_stft_loop).  A forward frame kernel forms
// the unwrapped position p = hop t + i - h of what it reads in its own way - the specialised engine as hop blocks t - 5 .. t + 4,
// the others as window sample j at hop t + left + j - h - and reads the row at loop_read_index(p, P) where its plain twin reads
// reflect_index(p, Lw).  That is the whole difference between the two.  With P >= n_fft and t in [0, T] (a run's prefetch looks one
// frame past the row's end) every p lies in [-P, 2 P).
RFX_HD int loop_read_index(int p, int P) { return loop_wrap(p, P); }

// a loop forward call takes rows of exactly P samples: a positive multiple of hop, at least n_fft (the loop decode's rule:
// P = hop T, loop_valid(hop, T, n_fft)); it makes P / hop frames
RFX_HD bool loop_samples_valid(int hop, int n_fft, long long P) { return P > 0 && P % hop == 0 && P >= n_fft; }
RFX_HD int loop_samples_frames(int hop, int n_fft, long long P) { return loop_samples_valid(hop, n_fft, P) ? (int)(P / hop) : 0; }
// the nearest legal lengths: the largest one <= P (0: there is none) and the smallest one >= P
RFX_HD long long loop_samples_below(int hop, int n_fft, long long P) {
  const long long lo = (long long)hop * loop_min_frames(hop, n_fft);
  return P < lo ? 0 : P / hop * hop;
}
RFX_HD long long loop_samples_above(int hop, int n_fft, long long P) {
  const long long lo = (long long)hop * loop_min_frames(hop, n_fft);
  return P <= lo ? lo : (P + hop - 1) / hop * hop;
}

// floor(a / b), b > 0
RFX_HD int loop_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the unwrapped covering frames of q = m + h - left
RFX_HD void loop_fold_range(int q, int win, int hop, int& tlo, int& thi) {
  tlo = -loop_floor_div(win - 1 - q, hop);  // ceil((q - win + 1) / hop)
  thi = loop_floor_div(q, hop);
}
// frame index of the unwrapped t in [-T, 2 T)
RFX_HD int loop_frame(int t, int T) { return loop_wrap(t, T); }

// env[r], r = m mod hop: sum of w[j]^2 over the window samples the chain of m meets, in chain order (j decreasing), one fma chain
RFX_HD float loop_env(const float* win, int r, int h, int left, int win_len, int hop) {
  int tlo, thi;
  const int q = r + h - left;
  loop_fold_range(q, win_len, hop, tlo, thi);
  float e = 0.f;
  for (int t = tlo; t <= thi; ++t) {
    const float w = win[q - hop * t];
    e = fmaf(w, w, e);
  }
  return e;
}

// one output sample of the circular fold, before the envelope.  rows: the row's T synthesis frames, `pitch` floats apart, window
// sample j of a frame at shift + j.
// ... of frames that are windowed already (generic engine, row family): a chain of sums
RFX_HD float loop_fold_sum(const float* rows, size_t pitch, int shift, int q, int win_len, int hop, int T) {
  int tlo, thi;
  loop_fold_range(q, win_len, hop, tlo, thi);
  float acc = 0.f;
  for (int t = tlo; t <= thi; ++t) acc += rows[(size_t)loop_frame(t, T) * pitch + shift + (q - hop * t)];
  return acc;
}
// ... of un-windowed frames (specialised engine): an fma chain y w + acc
RFX_HD float loop_fold_fma(const float* rows, size_t pitch, const float* win, int q, int win_len, int hop, int T) {
  int tlo, thi;
  loop_fold_range(q, win_len, hop, tlo, thi);
  float acc = 0.f;
  for (int t = tlo; t <= thi; ++t) {
    const int j = q - hop * t;
    acc = fmaf(rows[(size_t)loop_frame(t, T) * pitch + j], win[j], acc);
  }
  return acc;
}

}  // namespace rfx
