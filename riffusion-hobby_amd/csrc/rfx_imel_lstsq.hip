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

}  // namespace

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
