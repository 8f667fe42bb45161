// rfx_quality_core.h - arithmetic of the per-row spectral sums (rfx_quality.hip), written once for the gfx950 kernels (hipcc) and
// the host emulators of the CPU tests (tests/emu/rfx_quality_emu.cpp, tests/emu/rfx_spec_loss_emu.cpp, g++).
//
// For every row (clip-channel) of T frames N double sums over the n_stft bins of every frame, each bin once:
//   num = sum (a - m)^2      den = sum m^2      N == 3: lsum = sum | ln max(a, f) - ln max(m, f) |
// a: the magnitudes the plan's forward transform gives for the row's waveform, m: the target, both float32 in the plan's slot
// layout, f the log floor.  N == 2 is rfx_spectral_error, N == 3 rfx_spectral_loss; the sums type (SpecSums<N>), the walk, the tree and the
// combine are templates of N, so the two-sum instantiation carries two doubles and nothing else through registers, LDS and the
// partials, and the first two sums of either are the same bits.  a - m is formed in double (exact for two float32 values);
// squares and sums are double as well: the supported magnitudes reach 1e33 (include/rfx.h, "Numeric range"), whose square
// float32 cannot hold.  Each term of lsum is formed in double from the two float32 values, max taken in float32 (exact), one
// double logarithm each, their difference, its absolute value, one addition.  LOG == false (f == 0) evaluates no logarithm and
// leaves lsum 0.
//
// The shape of a row's reduction is a function of (T, the plan's layout) alone, so that a row's sums are the same alone and
// inside any batch (the rule of rfx_kernels.h: kGlGroup):
//   - the row is cut into chunks of kQualFrames consecutive frames (the last one shorter), one workgroup of kQualThreads each;
//   - thread t of a chunk walks the chunk's frames in order and, within a frame, the 16-byte vectors t, t + kQualThreads, ...,
//     adding the counted elements of a vector in order: one fma per element and sum, one addition for lsum (qual_walk);
//   - the workgroup's kQualThreads sums are folded by the halving tree (qual_tree_step, strides 128 .. 1) into one partial;
//   - a second workgroup per row adds the row's partials, thread t taking partials t, t + kQualThreads, ... in order, and folds
//     them with the same tree (qual_combine_partial).
// No atomics, no dependence on the grid, on B or on the row's place in the call.
#pragma once
#include <math.h>
#include <stddef.h>
#include "rfx_core.h"

namespace rfx {

constexpr int kQualThreads = 256;  // a power of two: the tree halves it
constexpr int kQualFrames = 4;     // frames per chunk: 147 KiB of each tensor per workgroup on the specialised layout

template <int N>
struct SpecSums;
template <>
struct SpecSums<2> {
  double num, den;
};
template <>
struct SpecSums<3> {
  double num, den, lsum;
};
using QualSums = SpecSums<2>;  // rfx_spectral_error's
struct alignas(16) QualVec {
  float v[4];
};

RFX_HD int qual_chunks(int T) { return (T + kQualFrames - 1) / kQualFrames; }

// ---- which positions of a frame count --------------------------------------------------------------------------------------
// Specialised layout (rfx_core.h): 21 x 441 slots + padding; slot (k1, ka, kb) holds bin k = k1 + 40 (ka + 21 kb) when
// k <= 8820, else the conjugate of bin 17640 - k.  Bins with k mod 40 in 21 .. 39 exist ONLY as such a mirrored slot (of residue
// 40 - k mod 40 = 1 .. 19); bins with k mod 40 in {0, 20} exist twice: their mirrored copy (k1 = 0 or 20) is the one left out.
// 21 x 221 direct slots + (9261 - 4641 - 440) mirrored ones = 8821.
RFX_HD bool qual_slot_counts(int k1, int ka, int kb) { return k1 + 40 * (ka + 21 * kb) <= kNfft / 2 || (k1 != 0 && k1 != 20); }
// position p of a frame of magnitudes (slot_pos_f order)
RFX_HD bool qual_pos_counts(int p) {
  int q, kb;
  if (!pos_f_to_slot(p, q, kb)) return false;
  return qual_slot_counts(q / 21, q % 21, kb);
}
// the same for the four positions 4 i .. 4 i + 3 at once: bit e set when position 4 i + e counts.  Below 20 * kQPad a vector is
// one owner thread's four consecutive kb, above it four consecutive owner threads' kb = 20.
RFX_HD unsigned qual_slot_counts4(int i) {
  unsigned bits = 0;
  if (4 * i < 20 * kQPad) {
    const int g = i / kQPad, qp = i - g * kQPad;
    if ((qp & 63) == 63) return 0;
    const int q = (qp >> 6) * 63 + (qp & 63), k1 = q / 21, ka = q - 21 * k1;
#pragma unroll
    for (int e = 0; e < 4; ++e) bits |= qual_slot_counts(k1, ka, 4 * g + e) ? 1u << e : 0u;
    return bits;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int qp = 4 * i + e - 20 * kQPad;
    const int q = (qp >> 6) * 63 + (qp & 63), k1 = q / 21;
    bits |= ((qp & 63) != 63 && qual_slot_counts(k1, q - 21 * k1, 20)) ? 1u << e : 0u;
  }
  return bits;
}
// plain bin-ordered frames (generic plans): the first n_stft positions
RFX_HD unsigned qual_plain_counts4(int i, int n_stft) {
  const int left = n_stft - 4 * i;
  return left >= 4 ? 0xFu : left <= 0 ? 0u : (1u << left) - 1u;
}

// ---- the sums ------------------------------------------------------------------------------------------------------------------
template <int N, bool LOG>
RFX_HD void qual_accumulate(SpecSums<N>& s, float a, float m, float f, bool counts) {
  const double d = (double)a - (double)m, mm = (double)m;
  const double num = fma(d, d, s.num), den = fma(mm, mm, s.den);
  s.num = counts ? num : s.num;
  s.den = counts ? den : s.den;
  if constexpr (N == 3 && LOG) {
    const double l = s.lsum + fabs(log((double)fmaxf(a, f)) - log((double)fmaxf(m, f)));
    s.lsum = counts ? l : s.lsum;
  }
}
template <int N>
RFX_HD void qual_add(SpecSums<N>& s, const SpecSums<N>& o) {
  s.num += o.num;
  s.den += o.den;
  if constexpr (N == 3) s.lsum += o.lsum;
}

// thread `tid` of the workgroup that owns frames [f0, f1) of a row; a_row / m_row: the row's first frame, fs floats per frame
// (a multiple of four, frames 16-byte aligned).  A vector without a counted element is not loaded.
template <int N, bool PLAIN, bool LOG>
RFX_HD SpecSums<N> qual_walk(const float* a_row, const float* m_row, int f0, int f1, int fs, int n_stft, float floor, int tid) {
  SpecSums<N> s{};
  const int nv = fs >> 2;
  for (int f = f0; f < f1; ++f) {
    const QualVec* A = reinterpret_cast<const QualVec*>(a_row + (size_t)f * fs);
    const QualVec* M = reinterpret_cast<const QualVec*>(m_row + (size_t)f * fs);
    for (int i = tid; i < nv; i += kQualThreads) {
      const unsigned bits = PLAIN ? qual_plain_counts4(i, n_stft) : qual_slot_counts4(i);
      if (!bits) continue;
      const QualVec va = A[i], vm = M[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) qual_accumulate<N, LOG>(s, va.v[e], vm.v[e], floor, (bits >> e) & 1u);
    }
  }
  return s;
}
// the two-sum walk under the name rfx_spectral_error's emulator calls it by
template <bool PLAIN>
RFX_HD QualSums qual_thread_partial(const float* a_row, const float* m_row, int f0, int f1, int fs, int n_stft, int tid) {
  return qual_walk<2, PLAIN, false>(a_row, m_row, f0, f1, fs, n_stft, 0.f, tid);
}

// one level of the halving tree over kQualThreads sums: the threads tid < stride run it, a barrier follows
template <int N>
RFX_HD void qual_tree_step(SpecSums<N>* s, int tid, int stride) {
  qual_add(s[tid], s[tid + stride]);
}

// thread `tid` of the workgroup that combines a row's `chunks` partials
template <int N>
RFX_HD SpecSums<N> qual_combine_partial(const SpecSums<N>* partials, int chunks, int tid) {
  SpecSums<N> s{};
  for (int c = tid; c < chunks; c += kQualThreads) qual_add(s, partials[c]);
  return s;
}

}  // namespace rfx
