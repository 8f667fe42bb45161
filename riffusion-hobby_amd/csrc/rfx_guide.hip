// rfx_guide.hip - staging of a guided Griffin-Lim call's guide waveforms (include/rfx.h: rfx_guided_call_options): the caller's
// (B, guide_samples) rows, fitted to the call's L samples and brought into the kernels' numeric range by exact powers of two, into
// the audio buffer the call's first launch analyses.  Arithmetic and the shape of the peak reduction: rfx_guide_core.h.
// Two launches over (chunk, row): the chunks' peaks, then the scaled copy.
// Below them: the compaction of a held call's free frames into the list its launches 1 .. n_iter walk (rfx_held_call_options).
#include <hip/hip_runtime.h>

#include "rfx_guide_core.h"
#include "rfx_kernels.h"

namespace rfx {

namespace {
using v4 = float __attribute__((ext_vector_type(4)));

// samples p .. p + 3 of the fitted row (p a multiple of four): one 16-byte load where the source allows it
template <bool VEC>
__device__ __forceinline__ v4 guide_load4(const float* __restrict__ row, int n_valid, int p) {
  if (VEC && p + 3 < n_valid) return *reinterpret_cast<const v4*>(row + p);
  return v4{guide_fit(row, n_valid, p), guide_fit(row, n_valid, p + 1), guide_fit(row, n_valid, p + 2), guide_fit(row, n_valid, p + 3)};
}

// the largest of the workgroup's values, in every thread
__device__ __forceinline__ float block_max(float x, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  float m = lds[0];
#pragma unroll
  for (int w = 1; w < kGuideThreads / 64; ++w) m = fmaxf(m, lds[w]);
  return m;
}

// first sample of thread `tid`'s i-th vector of chunk `chunk`
__device__ __forceinline__ int guide_vec_at(int chunk, int i, int tid) { return chunk * kGuideChunk + (i * kGuideThreads + tid) * 4; }
}  // namespace

// peaks[row * chunks + chunk] = max |sample| of the chunk's part of the fitted row
template <bool VEC>
__global__ void __launch_bounds__(kGuideThreads) guide_peak_kernel(const float* __restrict__ guide, long long stride, int n_valid, int row0,
                                                                   float* __restrict__ peaks) {
  __shared__ float lds[kGuideThreads / 64];
  const int chunk = blockIdx.x, row = row0 + (int)blockIdx.y;
  const float* __restrict__ src = guide + (long long)row * stride;
  float peak = 0.f;
#pragma unroll
  for (int i = 0; i < kGuideVecsPerThread; ++i) {
    const int p = guide_vec_at(chunk, i, threadIdx.x);
    if (p < n_valid) {  // (behind it the fitted row is zero)
      const v4 v = guide_load4<VEC>(src, n_valid, p);
      peak = guide_peak_step(guide_peak_step(guide_peak_step(guide_peak_step(peak, v.x), v.y), v.z), v.w);
    }
  }
  peak = block_max(peak, lds);
  if (threadIdx.x == 0) peaks[(size_t)row * gridDim.x + chunk] = peak;
}

// dst[row][p] = fitted sample x 2^n / row_scale[2 row] for p < Lpad; zero[row][p] = 0 (the buffer the first launch adds to dst)
template <bool VEC>
__global__ void __launch_bounds__(kGuideThreads) guide_stage_kernel(const float* __restrict__ guide, long long stride, int n_valid, int Lpad,
                                                                    int row0, const float* __restrict__ peaks, const float* __restrict__ row_scale,
                                                                    float* __restrict__ dst, float* __restrict__ zero) {
  __shared__ float lds[kGuideThreads / 64];
  const int chunk = blockIdx.x, chunks = gridDim.x, row = row0 + (int)blockIdx.y;
  float peak = 0.f;
  for (int c = threadIdx.x; c < chunks; c += kGuideThreads) peak = fmaxf(peak, peaks[(size_t)row * chunks + c]);
  peak = block_max(peak, lds);
  const GuideScale s = guide_scale(peak, row_scale ? row_scale[2 * (size_t)row] : 0.f);
  const float* __restrict__ src = guide + (long long)row * stride;
  const size_t out_at = (size_t)row * Lpad;
#pragma unroll
  for (int i = 0; i < kGuideVecsPerThread; ++i) {
    const int p = guide_vec_at(chunk, i, threadIdx.x);
    if (p >= Lpad) continue;  // (Lpad is a multiple of 64: a vector is inside the row or outside it)
    v4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < n_valid) {
      v = guide_load4<VEC>(src, n_valid, p);
      v = v4{guide_apply(v.x, s), guide_apply(v.y, s), guide_apply(v.z, s), guide_apply(v.w, s)};
    }
    *reinterpret_cast<v4*>(dst + out_at + p) = v;
    if (zero) *reinterpret_cast<v4*>(zero + out_at + p) = v4{0.f, 0.f, 0.f, 0.f};
  }
}

hipError_t launch_guide_stage(const float* guide, long long stride, int guide_samples, int B, int L, int Lpad, const float* row_scale,
                              float* peaks, float* dst, float* zero, hipStream_t stream) {
  const int n_valid = guide_samples < L ? guide_samples : L;
  const int chunks = guide_chunks(Lpad);
  const bool vec = ((uintptr_t)guide & 15) == 0 && (stride & 3) == 0;
  for (int r0 = 0; r0 < B; r0 += 65535) {  // (grid y is 16 bits wide)
    const int n = B - r0 < 65535 ? B - r0 : 65535;
    const dim3 grid((unsigned)chunks, (unsigned)n);
    if (vec) hipLaunchKernelGGL(guide_peak_kernel<true>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, r0, peaks);
    else hipLaunchKernelGGL(guide_peak_kernel<false>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, r0, peaks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (vec) hipLaunchKernelGGL(guide_stage_kernel<true>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, Lpad, r0, peaks, row_scale, dst, zero);
    else hipLaunchKernelGGL(guide_stage_kernel<false>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, Lpad, r0, peaks, row_scale, dst, zero);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// The same staging for the guided decode's backward (rfx_api_guided.hip): rows of exactly L samples, L floats apart, as the plan's
// forward transform takes them (rfx_stft, rfx_stft_loop) - such a row need not start on 16 bytes, so the stores are scalar.  No
// kernel factor (c = 1).  The chunks here cover L samples; max is exact in any order, so the peak is the forward's.
template <bool VEC>
__global__ void __launch_bounds__(kGuideThreads) guide_stage_rows_kernel(const float* __restrict__ guide, long long stride, int n_valid, int L, int row0,
                                                                         const float* __restrict__ peaks, float* __restrict__ dst) {
  __shared__ float lds[kGuideThreads / 64];
  const int chunk = blockIdx.x, chunks = gridDim.x, row = row0 + (int)blockIdx.y;
  float peak = 0.f;
  for (int c = threadIdx.x; c < chunks; c += kGuideThreads) peak = fmaxf(peak, peaks[(size_t)row * chunks + c]);
  peak = block_max(peak, lds);
  const GuideScale s = guide_scale(peak, 0.f);
  const float* __restrict__ src = guide + (long long)row * stride;
  float* __restrict__ out = dst + (size_t)row * L;
#pragma unroll
  for (int i = 0; i < kGuideVecsPerThread; ++i) {
    const int p = guide_vec_at(chunk, i, threadIdx.x);
    if (p >= L) continue;
    v4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < n_valid) {
      v = guide_load4<VEC>(src, n_valid, p);
      v = v4{guide_apply(v.x, s), guide_apply(v.y, s), guide_apply(v.z, s), guide_apply(v.w, s)};
    }
    out[p] = v.x;
    if (p + 1 < L) out[p + 1] = v.y;
    if (p + 2 < L) out[p + 2] = v.z;
    if (p + 3 < L) out[p + 3] = v.w;
  }
}

hipError_t launch_guide_stage_rows(const float* guide, long long stride, int guide_samples, int B, int L, float* peaks, float* dst, hipStream_t stream) {
  const int n_valid = guide_samples < L ? guide_samples : L;
  const int chunks = guide_chunks(L);
  const bool vec = ((uintptr_t)guide & 15) == 0 && (stride & 3) == 0;
  for (int r0 = 0; r0 < B; r0 += 65535) {  // (grid y is 16 bits wide)
    const int n = B - r0 < 65535 ? B - r0 : 65535;
    const dim3 grid((unsigned)chunks, (unsigned)n);
    if (vec) hipLaunchKernelGGL(guide_peak_kernel<true>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, r0, peaks);
    else hipLaunchKernelGGL(guide_peak_kernel<false>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, r0, peaks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (vec) hipLaunchKernelGGL(guide_stage_rows_kernel<true>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, L, r0, peaks, dst);
    else hipLaunchKernelGGL(guide_stage_rows_kernel<false>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, L, r0, peaks, dst);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- the free-frame list of a held call (rfx_guide_core.h): counts per chunk of rows, a scan over the chunks, the fill ----------------
namespace {
// exclusive prefix sum of one value per thread of a kHoldThreads workgroup; *total: the workgroup's sum.  lds: kHoldThreads / 64 ints
__device__ __forceinline__ int hold_block_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  __syncthreads();  // (a previous call's readers are done with lds)
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kHoldThreads / 64; ++w) {
    if (w < wave) before += lds[w];
    all += lds[w];
  }
  *total = all;
  return before + incl - v;
}
}  // namespace

// list[chunk_offsets_at + chunk] = free frames of the chunk's rows
__global__ void __launch_bounds__(kHoldThreads) hold_count_kernel(const int32_t* __restrict__ hold, long long B, int T, int* __restrict__ list) {
  __shared__ int lds[kHoldThreads / 64];
  const long long chunk = blockIdx.x;
  int n = 0;
#pragma unroll
  for (int e = 0; e < kHoldRowsPerThread; ++e) n += hold_row_span(hold, hold_thread_row(chunk, threadIdx.x, e), B, T).count;
  int total;
  (void)hold_block_scan(n, lds, &total);
  if (threadIdx.x == 0) list[hold_chunk_offsets_at(B, T) + chunk] = total;
}

// one workgroup: the chunks' counts become their exclusive offsets, in place; the count of all free frames to its place
__global__ void __launch_bounds__(kHoldThreads) hold_scan_kernel(long long B, int T, int* __restrict__ list) {
  __shared__ int lds[kHoldThreads / 64];
  int* __restrict__ offs = list + hold_chunk_offsets_at(B, T);
  const long long chunks = hold_chunks(B);
  int carry = 0;
  for (long long c0 = 0; c0 < chunks; c0 += kHoldThreads) {
    const long long c = c0 + threadIdx.x;
    const int v = c < chunks ? offs[c] : 0;
    int total;
    const int before = hold_block_scan(v, lds, &total);
    if (c < chunks) offs[c] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) list[hold_count_at(B, T)] = carry;
}

// the chunk's rows write their free frames' indices from the chunk's offset on: a wave per row, lanes along the row's span
__global__ void __launch_bounds__(kHoldThreads) hold_fill_kernel(const int32_t* __restrict__ hold, long long B, int T, int* __restrict__ list) {
  __shared__ int lds[kHoldThreads / 64];
  __shared__ int row_first[kHoldChunkRows], row_count[kHoldChunkRows], row_at[kHoldChunkRows];
  const long long chunk = blockIdx.x;
  HoldSpan s[kHoldRowsPerThread];
  int n = 0;
#pragma unroll
  for (int e = 0; e < kHoldRowsPerThread; ++e) {
    s[e] = hold_row_span(hold, hold_thread_row(chunk, threadIdx.x, e), B, T);
    n += s[e].count;
  }
  int total;
  int at = list[hold_chunk_offsets_at(B, T) + chunk] + hold_block_scan(n, lds, &total);
#pragma unroll
  for (int e = 0; e < kHoldRowsPerThread; ++e) {
    const int r = threadIdx.x * kHoldRowsPerThread + e;
    row_first[r] = s[e].first;
    row_count[r] = s[e].count;
    row_at[r] = at;
    at += s[e].count;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < kHoldChunkRows; r += kHoldThreads / 64) {
    const long long row = chunk * kHoldChunkRows + r;
    const HoldSpan sp{row_first[r], row_count[r]};  // (count 0 behind the batch)
    for (int i = lane; i < sp.count; i += 64) list[(size_t)row_at[r] + i] = hold_list_entry(row, T, sp, i);
  }
}

hipError_t launch_hold_list(const int32_t* hold, int B, int T, int* list, hipStream_t stream) {
  const unsigned chunks = (unsigned)hold_chunks(B);
  hipLaunchKernelGGL(hold_count_kernel, dim3(chunks), dim3(kHoldThreads), 0, stream, hold, (long long)B, T, list);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hold_scan_kernel, dim3(1), dim3(kHoldThreads), 0, stream, (long long)B, T, list);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(hold_fill_kernel, dim3(chunks), dim3(kHoldThreads), 0, stream, hold, (long long)B, T, list);
  return hipGetLastError();
}

}  // namespace rfx
