// rfx_istft_core.h - the inverse spectrogram (include/rfx.h: rfx_istft, rfx_istft_loop, rfx_istft_backward, rfx_istft_backward_loop),
// written once for the kernels of rfx_istft.hip, the host drivers of rfx_api_istft.hip and the host emulator of the CPU tests
// (tests/emu/rfx_istft_emu.cpp, in double).  It states
//   - the zero-extension index rule of the backward's frame kernels, and the zero-padded period whose circular analysis is its exact test;
//   - the staging g -> u: the envelope-scaled gradient, laid out as the forward transform reads it;
//   - the weights c_k * unit and the zero-imaginary rule of the gradient slots.
//
// Definition.  h = n_fft / 2, N = n_fft, w the window zero-padded to N, X (n_stft, T) a row's complex spectrum, L the row's samples.
//   forward   y[q] = (sum_t w[q + h - hop t] f_t[q + h - hop t]) / env[q + h],  f_t = irfft_N(X[:, t]),  env[p] = sum_t w^2[p - hop t]
//             (loop: positions and frames modulo the period hop T, env the circular envelope - rfx_loop_core.h)
//   backward  G[k][t] = (c_k / N) sum_i w[i] u[hop t + i - h] e^{-2 pi i k i / N},  u[q] = g[q] / env[q + h] inside [0, L), 0 outside;
//             c_k = 1 for bin 0 and the Nyquist bin of an even N, else 2; Im G = 0 exactly where c_k = 1
//             (loop: u[q] = g[q] renv[q mod hop], the sample index modulo hop T: the circular analysis as it is)
#pragma once
#include <stddef.h>

#include "rfx_core.h"

namespace rfx {

// ---- the index rule ---------------------------------------------------------------------------------------------------------------
// position p of a row of L samples, zero-extended: the sample to read, or -1 for an exact 0 (neither reflected nor wrapped)
RFX_HD int zero_outside(int p, int L) { return p >= 0 && p < L ? p : -1; }
// ... as the zero-extension twins of the forward frame kernels read a row (the third index rule, beside reflect_index and
// loop_read_index): one unsigned compare, an exact 0.0f outside whatever the neighbours hold
RFX_HD float zero_outside_read(const float* x, int p, int L) { return (unsigned)p < (unsigned)L ? x[p] : 0.f; }
// The twin's exact test: the circular analysis (loop_read_index) of a row padded with zeros to the period P' = hop ceil((L + n_fft) / hop)
// reads, in its frames t < T, exactly what zero_outside gives - frame t reaches from hop t - h (at least -h: it wraps into the last h
// samples of the period, zeros) to hop (T - 1) + N - 1 - h < L + N <= P' - and the arithmetic per frame is the same kernel text.
RFX_HD int istft_pad_frames(int hop, int n_fft, int L) { return (int)(((long long)L + n_fft + hop - 1) / hop); }

// ---- the staging ------------------------------------------------------------------------------------------------------------------
// u = g * tab (the specialised engine's table (2 / N) / env and every loop table: reciprocals) or g / tab (the generic fold's env)
template <class R>
RFX_HD R istft_stage_value(R g, R tab, bool divide) {
  return divide ? g / tab : g * tab;
}
// Element `col` of a staged row of `pitch` elements whose first `valid` hold samples: the table entry it takes (col, or col mod
// period for a hop-entry table), or -1 for the zero padding
RFX_HD int istft_stage_entry(int col, int valid, int period) { return col >= valid ? -1 : period > 0 ? col % period : col; }

// ---- the gradient slots -----------------------------------------------------------------------------------------------------------
// unit: what is left of 1 / N once the staging table's own factor is counted - 1 / 2 where the table carries 2 / N (specialised
// engine), 1 / N where it is the bare envelope
RFX_HD bool istft_bin_is_real(int k, int n_fft) { return k == 0 || (n_fft % 2 == 0 && k == n_fft / 2); }
RFX_HD float istft_unit(int n_fft, bool specialised) { return specialised ? 0.5f : 1.f / (float)n_fft; }
RFX_HD double istft_unit_exact(int n_fft) { return 1.0 / (double)n_fft; }
template <class R>
RFX_HD R istft_bin_weight(int k, int n_fft, R unit) {
  return istft_bin_is_real(k, n_fft) ? unit : (R)2 * unit;
}
// one slot: the analysis value (re, im) of the slot as the forward transform wrote it - a conjugate slot holds the conjugate, and
// stays one under a real factor
template <class R>
RFX_HD void istft_grad_slot(int k, int n_fft, R unit, R re, R im, R& out_re, R& out_im) {
  const R c = istft_bin_weight(k, n_fft, unit);
  out_re = c * re;
  out_im = istft_bin_is_real(k, n_fft) ? (R)0 : c * im;
}

}  // namespace rfx
