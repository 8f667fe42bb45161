// rfx_spec_loss_core.h - arithmetic of the fused spectral losses (include/rfx.h: rfx_spectral_loss, rfx_spectral_loss_backward and their
// loop forms), written once for the gfx950 kernels (rfx_quality.hip: the sums; rfx_mel_bwd.hip: the magnitude slots and the circular
// adjoint fold) and the host emulator of the CPU tests (tests/emu/rfx_spec_loss_emu.cpp, g++).
//
// Per row, with a = |X| the magnitudes the plan's forward transform writes, m the target in the same slot layout, f the log floor and
// n = n_stft T bins, each counted once by the counting rule of rfx_quality_core.h:
//   forward    num = sum (a - m)^2     den = sum m^2     lsum = sum | ln max(a, f) - ln max(m, f) |       three double sums
//   backward   dL/da = c_sc (a - m) + c_lg sgn(ln max(a, f) - ln max(m, f)) [a >= f] / a                  c_sc, c_lg per row
// and then steps 2 to 4 of rfx_mel_bwd_core.h: the zero rule of torch.abs's backward, the frame adjoint (the engines' MODE 0 frame
// launch) and the adjoint fold - for a loop row the circular chain of rfx_loop_core.h.
//
// THE SUMS are rfx_quality_core.h's reduction at N = 3: num and den are rfx_spectral_error's bits, lsum rides the same walk.  The
// names below are that instantiation as the loss's emulator calls it; they hold no arithmetic.
//
// THE SLOT RULE.  A magnitude slot of the MODE 0 launch multiplies one complex value X = (re, im) of the re-analysed spectrum.  From
// that very value
//   a = sqrtf(fmaf(re, re, im * im))
// - the expression the forward entries form their magnitudes with (the specialised, generic and chirp-z kernels to the letter; the
// row family's forward kernel takes v_sqrt_f32 of the same argument, within 1 ulp of it) - so that a >= f and the sign are decided
// on the value the sums saw.  The sign is that of max(a, f) - max(m, f), compared as float32: the logarithm is increasing, and a
// double logarithm tells two different float32 values apart.  sgn(0) = 0; a == f passes the gradient (torch.clamp).  The slot is
//   S' = weight[k] ( fma(c_sc, a - m, sgn c_lg / a) ) / a,     0 where a == 0
// where the second term is there only when f > 0 and a >= f: with f >= 1e-18 its 1 / a^2 <= 1e36 fits float32.  Every operation is
// linear in (c_sc, c_lg): scaling both by a power of two scales S' by it exactly.
#pragma once
#include <math.h>
#include <stddef.h>

#include "rfx_core.h"
#include "rfx_loop_core.h"
#include "rfx_quality_core.h"

namespace rfx {

// the floors an entry takes: 0 (no log term) or a finite f >= 1e-18
RFX_HD bool spec_loss_floor_ok(float f) { return f == 0.f || (f >= 1e-18f && f <= 3.402823466e38f); }

// ---- the sums: rfx_quality_core.h at N = 3 -----------------------------------------------------------------------------------------
using SpecLossSums = SpecSums<3>;
template <bool PLAIN, bool LOG>
RFX_HD SpecLossSums spec_loss_thread_partial(const float* a_row, const float* m_row, int f0, int f1, int fs, int n_stft, float f, int tid) {
  return qual_walk<3, PLAIN, LOG>(a_row, m_row, f0, f1, fs, n_stft, f, tid);
}
RFX_HD void spec_loss_tree_step(SpecLossSums* s, int tid, int stride) { qual_tree_step(s, tid, stride); }
RFX_HD SpecLossSums spec_loss_combine_partial(const SpecLossSums* partials, int chunks, int tid) { return qual_combine_partial(partials, chunks, tid); }

// ---- the slot rule ---------------------------------------------------------------------------------------------------------------
RFX_HD float spec_loss_abs(float re, float im) { return sqrtf(fmaf(re, re, im * im)); }
RFX_HD double spec_loss_abs(double re, double im) { return sqrt(fma(re, re, im * im)); }
RFX_HD float spec_loss_fma(float x, float y, float z) { return fmaf(x, y, z); }
RFX_HD double spec_loss_fma(double x, double y, double z) { return fma(x, y, z); }
// (dL/da) / a from the magnitude a of the slot's own complex value and the target m of the slot: what multiplies X, before the
// one-sided weight.  0 where a == 0.
template <class R>
RFX_HD R spec_loss_unit_scale(R a, R m, R c_sc, R c_lg, R f) {
  if (a == (R)0) return (R)0;
  R l = (R)0;
  if (f > (R)0 && a >= f) {
    const R mf = m > f ? m : f;  // (a >= f: max(a, f) is a)
    const R sgn = a > mf ? (R)1 : a < mf ? (R)-1 : (R)0;
    l = sgn * c_lg / a;
  }
  return spec_loss_fma(c_sc, a - m, l) / a;
}

// ---- the circular adjoint fold -----------------------------------------------------------------------------------------------------
// Sample m of a loop row's gradient, P = hop T: with q = m + h - left the chain over the unwrapped covering frames loop_fold_range
// gives, oldest first, frame loop_frame(t, T) each - loop_fold_fma over un-windowed frames (specialised engine), loop_fold_sum over
// frames the launch has windowed - as it stands: no envelope, no reflect partners.  Rolling the frames by k rolls the result by k hop.
RFX_HD float spec_loss_loop_sample(const float* rows, size_t pitch, int shift, const float* win, int m, int h, int left, int win_len, int hop, int T) {
  const int q = m + h - left;
  return win ? loop_fold_fma(rows, pitch, win, q, win_len, hop, T) : loop_fold_sum(rows, pitch, shift, q, win_len, hop, T);
}

}  // namespace rfx
