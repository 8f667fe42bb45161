// rfx_mel_bwd_core.h - the backward of the forward path (include/rfx.h: rfx_stft_backward, rfx_mel_scale_backward,
// rfx_mel_from_waveform_backward), written once for the kernels of rfx_mel_bwd.hip, the host half of plan creation and the host
// emulator of the CPU tests (tests/emu/rfx_mel_bwd_emu.cpp, in double).  It states
//   - the per-bin adjoint table of the filterbank: first band, count and weights of every linear bin;
//   - the zero rule of the magnitude adjoint: gS X / |X|, exactly 0 where |X| == 0 (torch's abs backward);
//   - the weights that turn a one-sided gradient into what a MODE 0 frame launch synthesises;
//   - the three-chain index rule of the adjoint fold: centre, left reflect partner, right reflect partner.
//
// Definition.  h = n_fft / 2, left = (n_fft - win_length) / 2, w the window zero-padded to n_fft, T the frames of a row of Lw > h
// samples, X the row's complex STFT, g_mel (n_mels, T) the incoming gradient:
//   1  gS[k][t] = sum_m fb[k][m] g_mel[m][t] over the bands first[k] .. first[k] + count[k] - 1, in increasing m
//   2  G[k][t] = gS[k][t] X[k][t] / |X[k][t]|, 0 where |X| == 0       (rfx_stft_backward: G is the caller's complex gradient)
//   3  f_t[i] = sum_k Re G[k][t] cos(2 pi k i / n_fft) - Im G[k][t] sin(2 pi k i / n_fft), every one-sided bin with weight 1:
//      n_fft irfft of G with the interior bins halved; the imaginary parts of bin 0 and of the Nyquist bin drop out
//   4  gp[q] = sum_t w[q - hop t] f_t[q - hop t], one chain from the oldest covering frame on; sample j of the result is
//      gp[h + j], plus gp[h - j] when 1 <= j <= h, plus gp[h + 2 (Lw - 1) - j] when Lw - 1 - h <= j <= Lw - 2, added in that order
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

#include "rfx_core.h"

namespace rfx {

// ---- 1: the adjoint table ---------------------------------------------------------------------------------------------------------
// For every bin the first band with a non-zero weight, the number of bands up to the last non-zero one (0: no band reaches the bin)
// and their weights, `width` = the largest count (at least 1) per bin.  The count comes from the bank: 2 for a triangular bank, but
// any bank is served - a zero weight inside a bin's run stays in the table as a zero.
struct MelAdjoint {
  int F = 0, M = 0, width = 1;
  std::vector<int> first, count;
  std::vector<float> wt;  // [F][width], zero past a bin's count
};
inline MelAdjoint mel_adjoint_table(int F, int M, const float* fb /* [F][M] */) {
  MelAdjoint a;
  a.F = F;
  a.M = M;
  a.first.assign((size_t)F, 0);
  a.count.assign((size_t)F, 0);
  for (int k = 0; k < F; ++k) {
    int lo = -1, hi = -1;
    for (int m = 0; m < M; ++m)
      if (fb[(size_t)k * M + m] != 0.f) {
        if (lo < 0) lo = m;
        hi = m;
      }
    if (lo < 0) continue;
    a.first[k] = lo;
    a.count[k] = hi - lo + 1;
    if (a.count[k] > a.width) a.width = a.count[k];
  }
  a.wt.assign((size_t)F * a.width, 0.f);
  for (int k = 0; k < F; ++k)
    for (int i = 0; i < a.count[k]; ++i) a.wt[(size_t)k * a.width + i] = fb[(size_t)k * M + a.first[k] + i];
  return a;
}
// gS of one bin: `g(m)` is the gradient of band m at the frame.  One chain in increasing m.
template <class R, class G>
RFX_HD R mel_adjoint_bin(int first, int count, const float* wt, G g) {
  R s = (R)0;
  for (int i = 0; i < count; ++i) s += (R)wt[i] * g(first + i);
  return s;
}

// ---- 2: the zero rule -------------------------------------------------------------------------------------------------------------
RFX_HD float mel_bwd_abs(float re, float im) { return hypotf(re, im); }
RFX_HD double mel_bwd_abs(double re, double im) { return hypot(re, im); }
// gS / |X|: what multiplies X (the magnitude slot of a MODE 0 launch that takes X itself as its angles); 0 where |X| == 0
template <class R>
RFX_HD R mel_bwd_unit_scale(R gs, R re, R im) {
  const R a = mel_bwd_abs(re, im);
  return a == (R)0 ? (R)0 : gs / a;
}

// ---- 3: one-sided weights -----------------------------------------------------------------------------------------------------------
// A MODE 0 frame launch synthesises kappa irfft(Z) of a one-sided spectrum Z (kappa = n_fft / 2 on the specialised engine, whose
// fold applies 2 / n_fft; 1 on the generic, chirp-z and row-family engines).  Step 3 is n_fft irfft(G'), G' = G with the interior
// bins halved: Z[k] = unit * (2 for bin 0 and the Nyquist bin of an even n_fft, else 1) * G[k], unit = n_fft / (2 kappa).
RFX_HD float mel_bwd_unit(int n_fft, bool specialised) { return specialised ? 1.f : 0.5f * (float)n_fft; }
RFX_HD float mel_bwd_bin_weight(int k, int n_fft, float unit) {
  return (k == 0 || (n_fft % 2 == 0 && k == n_fft / 2)) ? 2.f * unit : unit;
}

// ---- 4: the adjoint fold ------------------------------------------------------------------------------------------------------------
// frames t whose WINDOW covers position q of the padded signal: its window sample is i = q - left - hop t in [0, win)
// (outside the window w is zero: the terms the definition's wider range adds are exact zeros).  Empty: tlo > thi.
RFX_HD void mel_bwd_frame_range(int q, int left, int win, int hop, int T, int& tlo, int& thi) {
  const int qw = q - left;
  if (qw < 0) {
    tlo = 0;
    thi = -1;
    return;
  }
  tlo = qw - (win - 1) <= 0 ? 0 : (qw - (win - 1) + hop - 1) / hop;
  thi = qw / hop;
  if (thi > T - 1) thi = T - 1;
}
// the padded positions sample j of a row of Lw samples collects, in the order they are added: centre, left partner, right partner
RFX_HD int mel_bwd_taps(int j, int h, int Lw, int (&q)[3]) {
  int n = 0;
  q[n++] = h + j;
  if (j >= 1 && j <= h) q[n++] = h - j;
  if (j >= Lw - 1 - h && j <= Lw - 2) q[n++] = h + 2 * (Lw - 1) - j;
  return n;
}
// does any of the samples j .. j + 3 have a reflect partner?  (the 4-wide fold serves the groups that have none)
RFX_HD bool mel_bwd_group_has_partner(int j, int h, int Lw) { return j <= h || j + 3 >= Lw - 1 - h; }
// sample j: `gp(q)` is the chain of padded position q
template <class R, class GP>
RFX_HD R mel_bwd_sample(int j, int h, int Lw, GP gp) {
  int q[3];
  const int n = mel_bwd_taps(j, h, Lw, q);
  R x = gp(q[0]);
  for (int i = 1; i < n; ++i) x += gp(q[i]);
  return x;
}

// ---- the position table of the magnitude slots a plan's MODE 0 launch reads: bin held by position p, -1 for padding -------------------
// specialised: slot_pos_f order with its doubled 440 bins; generic / chirp-z: position = bin; row family: its bin_of table (passed in)
inline std::vector<int> mel_bwd_pos_bin_spec() {
  std::vector<int> t((size_t)kFrameStride, -1);
  for (int q = 0; q < 441; ++q)
    for (int kb = 0; kb < 21; ++kb) t[(size_t)slot_pos_f(q, kb)] = slot_bin(q / 21, q % 21, kb, nullptr);
  return t;
}
// ... and of the complex slots the specialised forward transform writes (slot_pos_c order), both slots of a doubled bin included
inline std::vector<int> mel_bwd_xpos_bin_spec() {
  std::vector<int> t((size_t)kFrameStride, -1);
  for (int q = 0; q < 441; ++q)
    for (int kb = 0; kb < 21; ++kb) t[(size_t)slot_pos_c(q, kb)] = slot_bin(q / 21, q % 21, kb, nullptr);
  return t;
}
// The position of the spectrum a magnitude slot goes with: the frame launch multiplies magnitude slot p by the complex value it
// reads at s2x[p] (-1: padding).  Specialised: the SAME slot (q, kb) in the other order - a doubled bin's two slots hold two separately
// rounded values of X, and each magnitude slot is gS / |the value it will multiply|, so that the product has the modulus gS whatever
// the forward transform's rounding was (on a bin with |X| near zero the two values differ by far more than an ulp).
inline std::vector<int> mel_bwd_s2x_spec() {
  std::vector<int> t((size_t)kFrameStride, -1);
  for (int q = 0; q < 441; ++q)
    for (int kb = 0; kb < 21; ++kb) t[(size_t)slot_pos_f(q, kb)] = slot_pos_c(q, kb);
  return t;
}
inline std::vector<int> mel_bwd_pos_bin_plain(int n_stft, int stride) {
  std::vector<int> t((size_t)stride, -1);
  for (int k = 0; k < n_stft && k < stride; ++k) t[(size_t)k] = k;
  return t;
}

}  // namespace rfx
