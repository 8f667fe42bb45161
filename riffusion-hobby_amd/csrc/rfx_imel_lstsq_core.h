// rfx_imel_lstsq_core.h - arithmetic of the closed-form InverseMelScale (rfx_imel_lstsq.hip), written once for the gfx950
// kernels (hipcc) and the host emulator of the CPU tests (tests/emu/rfx_imel_lstsq_emu.cpp, g++).
//
// torchaudio >= 2.1's InverseMelScale is relu(lstsq(fb^T, mel)): the minimum-norm least-squares solution, clamped at zero.  For a
// bank whose bins touch at most two adjacent filters, G = fb^T fb (M x M) is symmetric tridiagonal and, where it is regular, the
// answer is x = relu(fb G^-1 mel).  rfx_plan_core.h factors G = L D L^T once in double (L unit lower bidiagonal) and rounds two
// tables to float32: nl[m] = -L[m + 1][m] (nl[M - 1] = 0) and inv_d[m] = 1 / D[m].  Per frame, in float32, every step one fmaf
// (and one product) so that host and device round alike:
//   forward    z[0] = mel[0],                 z[m] = fmaf(nl[m - 1], z[m - 1], mel[m])        m = 1 .. M - 1
//   backward   y[M - 1] = z[M - 1] inv_d[M - 1],  y[m] = fmaf(nl[m], y[m + 1], z[m] inv_d[m])  m = M - 2 .. 0
//   expand     x[f] = max(0, fmaf(w1[f], y[m0[f] + 1], w0[f] y[m0[f]]))                         every position of a frame
// The order is a function of M alone: a frame's result depends on its mel column and the plan's tables, never on the batch, the
// frame's place in it or the launch grid.  Every step is linear with power-of-two-exact roundings: an input times 2^n gives the
// output times 2^n bit for bit as long as no intermediate leaves float32's normal range.
//
// The sweeps walk the column in batches of kLsqBatch steps and load the next batch's inputs before they run the current one:
// the loads do not depend on the chain, and the device needs them in flight ahead of it.
#pragma once
#include <math.h>
#include <stddef.h>
#include "rfx_core.h"

namespace rfx {

constexpr int kLsqBatch = 16;     // steps whose inputs are loaded together, one batch ahead of the chain
constexpr int kLsqThreads = 256;  // expand workgroup

// frames one expand workgroup stages in LDS: 16 x (M + 3) floats up to 512 filters (33 KB), 8 above (1024: 33 KB)
RFX_HD int lsq_expand_frames(int M) { return M <= 512 ? 16 : 8; }
// floats between two staged frames: y[0 .. M - 1], then at least two zeros (the entries M and M + 1 a position without a filter
// and the last filter's absent neighbour read); odd, so that frames fall on different banks
RFX_HD int lsq_y_stride(int M) { return (M + 2) | 1; }

RFX_HD float lsq_forward_step(float nl_prev, float z_prev, float mel) { return fmaf(nl_prev, z_prev, mel); }
RFX_HD float lsq_backward_step(float nl, float y_next, float z, float inv_d) { return fmaf(nl, y_next, z * inv_d); }
RFX_HD float lsq_expand_value(float w0, float w1, float y0, float y1) {
  const float v = fmaf(w1, y1, w0 * y0);
  return v > 0.f ? v : 0.f;
}

// Forward sweep of one frame.  mel, z: the frame's column, `stride` floats between consecutive filters (the column of a
// (M, T) matrix with T contiguous).
RFX_HD void lsq_forward_sweep(const float* __restrict__ nl, const float* __restrict__ mel, float* __restrict__ z, size_t stride, int M) {
  float cur[kLsqBatch], nxt[kLsqBatch];
#pragma unroll
  for (int i = 0; i < kLsqBatch; ++i) cur[i] = i < M ? mel[(size_t)i * stride] : 0.f;
  float carry = 0.f;  // z[m - 1]; nl[-1] is taken as 0
  for (int m0 = 0; m0 < M; m0 += kLsqBatch) {
#pragma unroll
    for (int i = 0; i < kLsqBatch; ++i) {
      const int m = m0 + kLsqBatch + i;
      nxt[i] = m < M ? mel[(size_t)m * stride] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kLsqBatch; ++i) {
      const int m = m0 + i;
      if (m < M) {
        carry = m == 0 ? cur[i] : lsq_forward_step(nl[m - 1], carry, cur[i]);
        z[(size_t)m * stride] = carry;
      }
    }
#pragma unroll
    for (int i = 0; i < kLsqBatch; ++i) cur[i] = nxt[i];
  }
}

// Backward sweep of one frame, in place: zy holds z on entry and y on return.
RFX_HD void lsq_backward_sweep(const float* __restrict__ nl, const float* __restrict__ inv_d, float* zy, size_t stride, int M) {
  float cur[kLsqBatch], nxt[kLsqBatch];
#pragma unroll
  for (int i = 0; i < kLsqBatch; ++i) {
    const int m = M - 1 - i;
    cur[i] = m >= 0 ? zy[(size_t)m * stride] : 0.f;
  }
  float carry = 0.f;  // y[m + 1]; there is no filter M
  for (int m0 = M - 1; m0 >= 0; m0 -= kLsqBatch) {
#pragma unroll
    for (int i = 0; i < kLsqBatch; ++i) {
      const int m = m0 - kLsqBatch - i;
      nxt[i] = m >= 0 ? zy[(size_t)m * stride] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kLsqBatch; ++i) {
      const int m = m0 - i;
      if (m >= 0) {
        carry = lsq_backward_step(nl[m], carry, cur[i], inv_d[m]);  // (m == M - 1: nl = 0, carry = 0)
        zy[(size_t)m * stride] = carry;
      }
    }
#pragma unroll
    for (int i = 0; i < kLsqBatch; ++i) cur[i] = nxt[i];
  }
}

// ---- backward: g_mel = G^-1 c, c = fb^T (gx where the relu is open) -------------------------------------------------------------------
// G is symmetric, so the backward's solve is the two sweeps above on another right-hand side.  What is new is the collect:
//   open[f] = fmaf(w1[f], y[m0[f] + 1], w0[f] y[m0[f]]) > 0     lsq_expand_value's own expression on the forward's y: the mask is
//                                                               the forward's x > 0 bit for bit, and 0 where v <= 0 as torch.relu
//   c[m]    = sum over the bins f of filter m, ASCENDING f, acc = fmaf(w(f, m), open[f] ? gx[f] : 0, acc), acc = 0 before the first
// A filter's bins are one run (rfx_plan_core.h: bank_lstsq_collect), so the order is the plan's alone: first the bins whose first
// filter is m - 1 (weight w1), then those whose first filter is m (weight w0).  A closed bin enters as +0.0 whatever gx holds there
// (a NaN included); every bin is read from ONE position of the frame, its first slot.  No atomics: a c[m] is one lane's chain.
// Linear in gx with power-of-two-exact roundings, as the sweeps are.
constexpr int kLsqCollectThreads = 512;  // collect workgroup
constexpr int kLsqCollectVecs = 5;       // 16-byte vectors of a frame one thread masks: bank_lstsq_collect admits at most 5 * 512

RFX_HD float lsq_collect_masked(float w0, float w1, float y0, float y1, float gx) {
  const float v = fmaf(w1, y1, w0 * y0);
  return v > 0.f ? gx : 0.f;
}
// w: the n weights of a filter's run, `wstride` floats apart (1: the host lists; n_mels: the device's table, transposed so that the
// lanes of a wave - consecutive filters - read one line per step); g: the masked gradient of its bins; both in ascending bin order.
// Eight terms' inputs are loaded before their chain runs; the chain itself is one fmaf per term in that order.
constexpr int kLsqCollectBatch = 8;
RFX_HD float lsq_collect_sum(const float* __restrict__ w, size_t wstride, const float* g, int n) {
  float acc = 0.f;
  for (int i0 = 0; i0 < n; i0 += kLsqCollectBatch) {
    float wv[kLsqCollectBatch], gv[kLsqCollectBatch];
#pragma unroll
    for (int k = 0; k < kLsqCollectBatch; ++k) {
      const int i = i0 + k;
      wv[k] = i < n ? w[(size_t)i * wstride] : 0.f;
      gv[k] = i < n ? g[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kLsqCollectBatch; ++k)
      if (i0 + k < n) acc = fmaf(wv[k], gv[k], acc);
  }
  return acc;
}

}  // namespace rfx
