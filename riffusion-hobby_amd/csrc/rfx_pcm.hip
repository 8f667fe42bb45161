// rfx_pcm.hip - the int16 PCM post-processing of the decode on the device (riffusion/util/audio_util.py):
//   * apply_filters(compression=False): gain to -12 dBFS, then peak normalisation with 0.1 dB headroom, per clip of a
//     (N, L, C) batch; three launches - statistics (clip x split workgroups, partials to the workspace: no atomics, no
//     memset), finish (one wave per clip: the two factors), apply (elementwise, may run in place)
//   * stitch_segments of N equal-length clips: one launch over the output frames, driven by the host planner's pieces
// The arithmetic (audioop's mul / add / rms / max) is rfx_pcm_core.h, shared with the CPU emulator of the tests.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_kernels.h"
#include "rfx_pcm_core.h"

namespace rfx {

namespace {

constexpr int kPcmThreads = 256;
constexpr int64_t kPcmSplitSamples = 32768;  // samples of one clip per statistics workgroup (64 KB of int16)
constexpr int kPcmMaxSplits = 64;

}  // namespace

int pcm_splits(int64_t count) {
  int64_t s = (count + kPcmSplitSamples - 1) / kPcmSplitSamples;
  return (int)(s < 1 ? 1 : (s > kPcmMaxSplits ? kPcmMaxSplits : s));
}

// ---- statistics: workgroup (clip, part) reduces samples [begin, end) of the clip; 16-byte loads over the aligned middle
__global__ void __launch_bounds__(kPcmThreads) pcm_stats_kernel(const int16_t* __restrict__ pcm, int64_t count, int splits,
                                                                PcmPartial* __restrict__ partials) {
  __shared__ long long red_s[kPcmThreads / 64];
  __shared__ int max_s[kPcmThreads / 64], min_s[kPcmThreads / 64];
  const int clip = blockIdx.x / splits, part = blockIdx.x - clip * splits;
  const int64_t chunk = (count + splits - 1) / splits;
  const int64_t begin = (int64_t)part * chunk, end = begin + chunk < count ? begin + chunk : count;
  const int16_t* p = pcm + (int64_t)clip * count;
  long long s = 0;  // |x| <= 2^15: each square <= 2^30, a thread's sum stays far below 2^63
  int mx = -32768, mn = 32767;
  auto take = [&](int v) {
    s += (long long)(v * v);
    mx = v > mx ? v : mx;
    mn = v < mn ? v : mn;
  };
  // [begin, ab) and [ae, end) one sample at a time, [ab, ae) as whole 16-byte groups of eight samples
  int64_t ab = begin;
  while (ab < end && (reinterpret_cast<uintptr_t>(p + ab) & 15)) ++ab;
  const int64_t ae = ab + ((end - ab) & ~(int64_t)7);
  for (int64_t i = begin + threadIdx.x; i < ab; i += kPcmThreads) take(p[i]);
  for (int64_t i = ab + 8 * (int64_t)threadIdx.x; i < ae; i += 8 * kPcmThreads) {
    const int4 v = *reinterpret_cast<const int4*>(p + i);
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      take((int)(int16_t)(w[k] & 0xFFFF));
      take(w[k] >> 16);
    }
  }
  for (int64_t i = ae + threadIdx.x; i < end; i += kPcmThreads) take(p[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    mx = max(mx, __shfl_xor(mx, o));
    mn = min(mn, __shfl_xor(mn, o));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red_s[wave] = s;
    max_s[wave] = mx;
    min_s[wave] = mn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    PcmPartial r{0, -32768, 32767};
    for (int w = 0; w < kPcmThreads / 64; ++w) {
      r.sumsq += red_s[w];
      r.xmax = max(r.xmax, max_s[w]);
      r.xmin = min(r.xmin, min_s[w]);
    }
    partials[blockIdx.x] = r;
  }
}

// ---- finish: one wave per clip combines its partials (integer sums: the order cannot change them) and writes (f1, f2)
__global__ void __launch_bounds__(64) pcm_finish_kernel(const PcmPartial* __restrict__ partials, int splits, int64_t count,
                                                        const double* __restrict__ gain_by_rms, const double* __restrict__ boost_by_peak,
                                                        PcmFactors* __restrict__ factors) {
  const int clip = blockIdx.x;
  long long s = 0;
  int mx = -32768, mn = 32767;
  for (int j = threadIdx.x; j < splits; j += 64) {
    const PcmPartial q = partials[(int64_t)clip * splits + j];
    s += q.sumsq;
    mx = max(mx, q.xmax);
    mn = min(mn, q.xmin);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    mx = max(mx, __shfl_xor(mx, o));
    mn = min(mn, __shfl_xor(mn, o));
  }
  if (threadIdx.x == 0) factors[clip] = pcm_filter_factors(s, count, mx, mn, gain_by_rms, boost_by_peak);
}

// ---- apply: out = mul(mul(x, f1), f2) over the whole batch; eight samples per thread and step.  A group of eight may straddle
// clips: then each sample looks up its own clip's factors.  In place when out == in (each thread reads its samples before it
// writes them, and no two threads share a sample).
__global__ void __launch_bounds__(kPcmThreads) pcm_apply_kernel(const int16_t* in, int16_t* out, int64_t total, int64_t count,
                                                                const PcmFactors* __restrict__ factors, int64_t head) {
  const int64_t stride = 8 * (int64_t)gridDim.x * kPcmThreads;
  // [0, head): samples before the first 16-byte boundary of both pointers (the launcher checks that in and out share it)
  for (int64_t i = (int64_t)blockIdx.x * kPcmThreads + threadIdx.x; i < head; i += (int64_t)gridDim.x * kPcmThreads)
    out[i] = pcm_filter_sample(in[i], factors[i / count]);
  const int64_t body = head + ((total - head) & ~(int64_t)7);
  for (int64_t i = head + 8 * ((int64_t)blockIdx.x * kPcmThreads + threadIdx.x); i < body; i += stride) {
    const int4 v = *reinterpret_cast<const int4*>(in + i);
    const int64_t clip = i / count;
    const bool split = i + 7 >= (clip + 1) * count;  // the group reaches into the next clip (or several: clips shorter than 8)
    const PcmFactors f0 = factors[clip];
    auto fac = [&](int64_t j) { return split ? factors[j / count] : f0; };
    const int w[4] = {v.x, v.y, v.z, v.w};
    int r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int lo = pcm_filter_sample((int)(int16_t)(w[k] & 0xFFFF), fac(i + 2 * k));
      const int hi = pcm_filter_sample(w[k] >> 16, fac(i + 2 * k + 1));
      r[k] = (int)(((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16));
    }
    *reinterpret_cast<int4*>(out + i) = int4{r[0], r[1], r[2], r[3]};
  }
  for (int64_t i = body + (int64_t)blockIdx.x * kPcmThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kPcmThreads)
    out[i] = pcm_filter_sample(in[i], factors[i / count]);
}

// ---- stitch: one thread per output sample (frame, channel); the piece comes from a binary search over the piece starts
__global__ void __launch_bounds__(kPcmThreads) pcm_stitch_kernel(const int16_t* __restrict__ pcm, int64_t L, int C,
                                                                 const PcmPiece* __restrict__ pieces, int n_pieces, int64_t total,
                                                                 int16_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kPcmThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kPcmThreads) {
    const int64_t frame = i / C;
    const int ch = (int)(i - frame * C);
    out[i] = pcm_stitch_sample(pieces[pcm_find_piece(pieces, n_pieces, frame)], frame, ch, pcm, L, C);
  }
}

static unsigned pcm_grid(int64_t items) {
  const int64_t b = (items + kPcmThreads - 1) / kPcmThreads;
  return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

size_t pcm_filters_workspace_bytes(int N, int L, int C) {
  const int splits = pcm_splits((int64_t)L * C);
  return ((size_t)N * splits * sizeof(PcmPartial) + 255) / 256 * 256 + (size_t)N * sizeof(PcmFactors);
}

hipError_t launch_pcm_filters(const int16_t* in, int N, int L, int C, const double* gain_by_rms, const double* boost_by_peak,
                              int16_t* out, void* workspace, hipStream_t s) {
  const int64_t count = (int64_t)L * C, total = count * N;
  const int splits = pcm_splits(count);
  PcmPartial* partials = reinterpret_cast<PcmPartial*>(workspace);
  PcmFactors* factors = reinterpret_cast<PcmFactors*>((char*)workspace + ((size_t)N * splits * sizeof(PcmPartial) + 255) / 256 * 256);
  hipLaunchKernelGGL(pcm_stats_kernel, dim3((unsigned)N * splits), dim3(kPcmThreads), 0, s, in, count, splits, partials);
  hipLaunchKernelGGL(pcm_finish_kernel, dim3((unsigned)N), dim3(64), 0, s, partials, splits, count, gain_by_rms, boost_by_peak, factors);
  // both pointers must reach a 16-byte boundary after the same number of samples (the caller's tensors: both 0 mod 16)
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(in) & 15)) & 15) / 2;
  if ((reinterpret_cast<uintptr_t>(in) & 1) || ((reinterpret_cast<uintptr_t>(in) ^ reinterpret_cast<uintptr_t>(out)) & 15)) head = total;
  if (head > total) head = total;
  hipLaunchKernelGGL(pcm_apply_kernel, dim3(pcm_grid((total - head + 7) / 8)), dim3(kPcmThreads), 0, s, in, out, total, count, factors, head);
  return hipGetLastError();
}

hipError_t launch_pcm_stats(const int16_t* in, int N, int64_t count, PcmPartial* partials, hipStream_t s) {
  const int splits = pcm_splits(count);
  hipLaunchKernelGGL(pcm_stats_kernel, dim3((unsigned)N * splits), dim3(kPcmThreads), 0, s, in, count, splits, partials);
  return hipGetLastError();
}

hipError_t launch_pcm_stitch(const int16_t* pcm, int64_t L, int C, const void* pieces, int n_pieces, int64_t frames, int16_t* out,
                             hipStream_t s) {
  const int64_t total = frames * C;
  hipLaunchKernelGGL(pcm_stitch_kernel, dim3(pcm_grid(total)), dim3(kPcmThreads), 0, s, pcm, L, C,
                     reinterpret_cast<const PcmPiece*>(pieces), n_pieces, total, out);
  return hipGetLastError();
}

}  // namespace rfx
