// rfx_imel_lstsq.hip - closed-form InverseMelScale (rfx_inverse_mel_lstsq, include/rfx.h): x = relu(fb G^-1 mel) with
// G = fb^T fb symmetric tridiagonal, factored on the host (rfx_plan_core.h: bank_lstsq).  The arithmetic is
// rfx_imel_lstsq_core.h (shared with tests/emu/rfx_imel_lstsq_emu.cpp); the kernels add the mapping of frames to lanes and the
// staging of a frame's y in LDS.
//
// lsq_solve_kernel: one lane per frame.  mel is (B, M, T) with T contiguous, so the 64 lanes of a wave - 64 consecutive frames of
// a row - load one coalesced line per step; the factor tables are wave-uniform.  The forward sweep's z goes to the workspace
// (B, M, T), the backward sweep turns it into y in place.
// lsq_expand_kernel: one workgroup per lsq_expand_frames(M) consecutive frames of a row.  It stages their y columns in LDS
// (frame-major, two zeros behind each), then every thread takes four consecutive positions of the output frame - their first
// filter and two weights from the plan's per-position tables, loaded once for all the staged frames - and writes one 16-byte
// vector per frame: a wave stores 1 KiB of consecutive bytes.  Every position of the frame stride is written (padding and bins
// without a filter: 0.0).
// lsq_collect_kernel (the backward, rfx_inverse_mel_lstsq_backward): c = fb^T (gx where the relu is open), (B, M, T).  One workgroup
// per lsq_expand_frames(M) consecutive frames of a row, y staged as in the expansion.  Per frame: every thread reads its share of
// the frame's gx in whole 16-byte vectors - only the vectors that hold a counted position, their tables in registers for all the
// staged frames, the next frame's loads in flight under this frame's sums - and puts the masked values in LDS in bin order; then
// one lane per filter sums its run of bins there in ascending order (lsq_collect_sum; the weights transposed, [entry][filter], so
// that a wave's 64 filters read one line per step).  c[m] of frame j takes the place of
// y[m] of frame j in LDS, which the frame's mask was the last to read; at the end the block leaves as it was staged, a wave writing
// runs of consecutive t.  HBM traffic: one read of the counted vectors of gx, y and c.  LDS: 33 KB of y and at most 36 KB of frame.
#include <hip/hip_runtime.h>
#include "rfx_kernels.h"
#include "rfx_imel_lstsq_core.h"

namespace rfx {
namespace {

__global__ __launch_bounds__(64) void lsq_solve_kernel(const float* __restrict__ nl, const float* __restrict__ inv_d, const float* __restrict__ mel,
                                                        float* __restrict__ zy, int M, int T, int chunks) {
  const size_t row = blockIdx.x / (unsigned)chunks;
  const int t = (int)(blockIdx.x - row * (unsigned)chunks) * 64 + (int)threadIdx.x;
  if (t >= T) return;
  const size_t at = row * (size_t)M * (size_t)T + (size_t)t;
  lsq_forward_sweep(nl, mel + at, zy + at, (size_t)T, M);
  lsq_backward_sweep(nl, inv_d, zy + at, (size_t)T, M);
}

struct alignas(16) LsqVecF { float v[4]; };
struct alignas(16) LsqVecI { int v[4]; };

__global__ __launch_bounds__(kLsqThreads) void lsq_expand_kernel(const float* __restrict__ y, const int* __restrict__ pos_m0,
                                                                  const float* __restrict__ pos_w0, const float* __restrict__ pos_w1,
                                                                  float* __restrict__ out, int M, int T, int stride, int chunks, int FR) {
  extern __shared__ __attribute__((aligned(16))) float ys[];  // [FR][lsq_y_stride(M)]
  const int tid = threadIdx.x, Ms = lsq_y_stride(M);
  const size_t row = blockIdx.x / (unsigned)chunks;
  const int t0 = (int)(blockIdx.x - row * (unsigned)chunks) * FR;
  const int nfr = T - t0 < FR ? T - t0 : FR;
  const float* yrow = y + row * (size_t)M * (size_t)T + (size_t)t0;
  for (int i = tid; i < M * FR; i += kLsqThreads) {
    const int m = i / FR, j = i - m * FR;
    if (j < nfr) ys[j * Ms + m] = yrow[(size_t)m * (size_t)T + j];
  }
  for (int i = tid; i < FR * (Ms - M); i += kLsqThreads) {
    const int j = i / (Ms - M), k = i - j * (Ms - M);
    ys[j * Ms + M + k] = 0.f;
  }
  __syncthreads();
  float* orow = out + (row * (size_t)T + (size_t)t0) * (size_t)stride;
  for (int v = tid; v < (stride >> 2); v += kLsqThreads) {
    const LsqVecI m0 = reinterpret_cast<const LsqVecI*>(pos_m0)[v];
    const LsqVecF w0 = reinterpret_cast<const LsqVecF*>(pos_w0)[v], w1 = reinterpret_cast<const LsqVecF*>(pos_w1)[v];
    for (int j = 0; j < nfr; ++j) {
      const float* yj = ys + j * Ms;
      LsqVecF o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o.v[e] = lsq_expand_value(w0.v[e], w1.v[e], yj[m0.v[e]], yj[m0.v[e] + 1]);
      reinterpret_cast<LsqVecF*>(orow + (size_t)j * (size_t)stride)[v] = o;
    }
  }
}

// NV: 16-byte vectors of a frame per thread, ceil(n_vecs / kLsqCollectThreads) - 3 for the default bank, whose 4000 bins with a
// filter sit in 1273 vectors; at most kLsqCollectVecs
template <int NV>
__global__ __launch_bounds__(kLsqCollectThreads) void lsq_collect_kernel(const float* __restrict__ y, const float* __restrict__ gx,
                                                                          const LsqCollectTables tb, float* __restrict__ c, int M, int T,
                                                                          int stride, int chunks, int FR) {
  extern __shared__ __attribute__((aligned(16))) float ys[];  // [FR][lsq_y_stride(M)], then the frame: [n_bins]
  const int tid = threadIdx.x, Ms = lsq_y_stride(M);
  float* gs = ys + ((FR * Ms + 3) & ~3);
  const size_t row = blockIdx.x / (unsigned)chunks;
  const int t0 = (int)(blockIdx.x - row * (unsigned)chunks) * FR;
  const int nfr = T - t0 < FR ? T - t0 : FR;
  const float* yrow = y + row * (size_t)M * (size_t)T + (size_t)t0;
  for (int i = tid; i < M * FR; i += kLsqCollectThreads) {
    const int m = i / FR, j = i - m * FR;
    if (j < nfr) ys[j * Ms + m] = yrow[(size_t)m * (size_t)T + j];
  }
  for (int i = tid; i < FR * (Ms - M); i += kLsqCollectThreads) {
    const int j = i / (Ms - M), k = i - j * (Ms - M);
    ys[j * Ms + M + k] = 0.f;
  }
  // this thread's vectors of a frame, and what their four positions need
  int vec[NV];
  LsqVecI at[NV];
  LsqVecF w0[NV], w1[NV], g[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = k * kLsqCollectThreads + tid;
    vec[k] = i < tb.n_vecs ? tb.vec[i] : -1;
    if (vec[k] >= 0) {
      at[k] = reinterpret_cast<const LsqVecI*>(tb.vec_at)[i];
      w0[k] = reinterpret_cast<const LsqVecF*>(tb.vec_w0)[i];
      w1[k] = reinterpret_cast<const LsqVecF*>(tb.vec_w1)[i];
    }
  }
  // ... and its filters (a bank has at most 2 * kLsqCollectThreads): where the run starts in the staged frame, and its length
  int first[2], run[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int m = tid + r * kLsqCollectThreads;
    first[r] = m < M ? tb.first[m] : 0;
    run[r] = m < M ? tb.run[m] : 0;
  }
  const float* grow = gx + (row * (size_t)T + (size_t)t0) * (size_t)stride;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (vec[k] >= 0) g[k] = reinterpret_cast<const LsqVecF*>(grow)[vec[k]];
  __syncthreads();
  for (int j = 0; j < nfr; ++j) {
    float* yj = ys + j * Ms;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (vec[k] >= 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int dst = at[k].v[e] & 0xffff, m0 = at[k].v[e] >> 16;
          if (dst != 0xffff) gs[dst] = lsq_collect_masked(w0[k].v[e], w1[k].v[e], yj[m0], yj[m0 + 1], g[k].v[e]);
        }
      }
    if (j + 1 < nfr) {
#pragma unroll
      for (int k = 0; k < NV; ++k)
        if (vec[k] >= 0) g[k] = reinterpret_cast<const LsqVecF*>(grow + (size_t)(j + 1) * (size_t)stride)[vec[k]];
    }
    __syncthreads();  // the frame is whole, and nobody reads y of frame j any more
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int m = tid + r * kLsqCollectThreads;
      if (m < M) yj[m] = lsq_collect_sum(tb.wt + m, (size_t)M, gs + first[r], run[r]);
    }
    __syncthreads();  // the next frame overwrites gs
  }
  float* crow = c + row * (size_t)M * (size_t)T + (size_t)t0;
  for (int i = tid; i < M * FR; i += kLsqCollectThreads) {
    const int m = i / FR, j = i - m * FR;
    if (j < nfr) crow[(size_t)m * (size_t)T + j] = ys[j * Ms + m];
  }
}

}  // namespace

size_t lsq_collect_lds_bytes(int M, int n_bins) {
  return ((size_t)((lsq_expand_frames(M) * lsq_y_stride(M) + 3) & ~3) + (size_t)n_bins) * sizeof(float);
}

template <int NV>
static hipError_t launch_lsq_collect_nv(const LsqCollectTables& tb, const float* y, const float* gx, float* c, int B, int M, int T, int stride,
                                        int chunks, int FR, size_t lds, hipStream_t s) {
  const hipError_t e = hipFuncSetAttribute((const void*)lsq_collect_kernel<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lsq_collect_kernel<NV>, dim3((unsigned)((size_t)B * chunks)), dim3(kLsqCollectThreads), lds, s, y, gx, tb, c, M, T, stride,
                     chunks, FR);
  return hipGetLastError();
}

// nrows * ceil(T / lsq_expand_frames(M)) must stay below 2^31 (the caller has checked B * T)
hipError_t launch_lsq_collect(const LsqCollectTables& tb, const float* y, const float* gx, float* c, int B, int M, int T, int stride, hipStream_t s) {
  const int FR = lsq_expand_frames(M), chunks = (T + FR - 1) / FR;
  const size_t lds = lsq_collect_lds_bytes(M, tb.n_bins);  // above the 64 KB a kernel gets unasked
  const int nv = (tb.n_vecs + kLsqCollectThreads - 1) / kLsqCollectThreads;
  return nv <= 1   ? launch_lsq_collect_nv<1>(tb, y, gx, c, B, M, T, stride, chunks, FR, lds, s)
         : nv == 2 ? launch_lsq_collect_nv<2>(tb, y, gx, c, B, M, T, stride, chunks, FR, lds, s)
         : nv == 3 ? launch_lsq_collect_nv<3>(tb, y, gx, c, B, M, T, stride, chunks, FR, lds, s)
         : nv == 4 ? launch_lsq_collect_nv<4>(tb, y, gx, c, B, M, T, stride, chunks, FR, lds, s)
         : nv == 5 ? launch_lsq_collect_nv<kLsqCollectVecs>(tb, y, gx, c, B, M, T, stride, chunks, FR, lds, s)
                   : hipErrorInvalidValue;
}

size_t lsq_expand_lds_bytes(int M) { return (size_t)lsq_expand_frames(M) * lsq_y_stride(M) * sizeof(float); }

// nrows * ceil(T / 64) and nrows * ceil(T / lsq_expand_frames(M)) must stay below 2^31 (the caller has checked B * T)
hipError_t launch_lsq_solve(const LsqTables& tb, const float* mel, float* zy, int B, int M, int T, hipStream_t s) {
  const int chunks = (T + 63) / 64;
  hipLaunchKernelGGL(lsq_solve_kernel, dim3((unsigned)((size_t)B * chunks)), dim3(64), 0, s, tb.nl, tb.inv_d, mel, zy, M, T, chunks);
  return hipGetLastError();
}

hipError_t launch_lsq_expand(const LsqTables& tb, const float* y, float* out, int B, int M, int T, int stride, hipStream_t s) {
  const int FR = lsq_expand_frames(M), chunks = (T + FR - 1) / FR;
  hipLaunchKernelGGL(lsq_expand_kernel, dim3((unsigned)((size_t)B * chunks)), dim3(kLsqThreads), lsq_expand_lds_bytes(M), s, y, tb.pos_m0,
                     tb.pos_w0, tb.pos_w1, out, M, T, stride, chunks, FR);
  return hipGetLastError();
}

}  // namespace rfx
