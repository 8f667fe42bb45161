// rfx_compress.hip - apply_filters(compression=True) on the device, up to the compressor's output (riffusion/util/audio_util.py:
// normalize(0.1), apply_gain(-10 - dBFS), compress_dynamic_range(-20, 4, 5, 50)); the rest is the compression=False pipeline
// of rfx_pcm.hip, run by the caller on this output.  Per (N, L, C) batch:
//   * statistics of rfx_pcm.hip (the peak of each clip)
//   * prepare: one workgroup per clip - the normalisation factor, the sum of squares after it (the -10 dBFS factor), the
//     exact int64 prefix sums of the frame energies of x2 (one contiguous run of frames per thread, a block scan between
//     runs: no atomics), and from them every frame's window rms (uint16, 0..32768)
//   * the attenuation recurrence, sequential (one lane per clip: the definition) or chunked (one workgroup per clip, one
//     lane per chunk, repair rounds until every chunk starts from its predecessor's end - DESIGN.md 4.4)
//   * apply: x3 = mul(x2, 10^(-att/20)) where att != 0, into the workspace, flagging every product within `margin` of an
//     integer for the host
// The arithmetic is rfx_compress_core.h / rfx_pcm_core.h, shared with the CPU emulator of the tests.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_compress_core.h"
#include "rfx_kernels.h"

namespace rfx {

namespace {

constexpr int kCmpWaves = kCmpLanes / 64;
constexpr int kCmpPerLane = kCmpMaxChunks / kCmpLanes;  // chunks one lane of the chunked form owns (contiguous)
constexpr int kCmpApplyThreads = 256;

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

// ---- prepare: one workgroup of kCmpLanes threads per clip
__global__ void __launch_bounds__(kCmpLanes) cmp_prepare_kernel(const int16_t* __restrict__ in, int64_t L, int C, int splits,
                                                                const PcmPartial* __restrict__ partials,
                                                                const double* __restrict__ boost_by_peak,
                                                                const double* __restrict__ gain10_by_rms, int64_t look,
                                                                CmpFactors* __restrict__ factors, int64_t* __restrict__ prefix_all,
                                                                uint16_t* __restrict__ rms_all) {
  __shared__ long long red_s[kCmpWaves];
  __shared__ int max_s[kCmpWaves], min_s[kCmpWaves];
  const int clip = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t count = L * C;
  const int16_t* x = in + (int64_t)clip * count;

  // the peak of the clip from the statistics partials -> normalize's factor
  int mx = -32768, mn = 32767;
  for (int j = tid; j < splits; j += kCmpLanes) {
    const PcmPartial q = partials[(int64_t)clip * splits + j];
    mx = max(mx, q.xmax);
    mn = min(mn, q.xmin);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, __shfl_xor(mx, o));
    mn = min(mn, __shfl_xor(mn, o));
  }
  if (lane == 0) {
    max_s[wave] = mx;
    min_s[wave] = mn;
  }
  __syncthreads();
  for (int w = 0; w < kCmpWaves; ++w) {
    mx = max(mx, max_s[w]);
    mn = min(mn, min_s[w]);
  }
  const double f_norm = boost_by_peak[max(mx, -mn)];

  // sum of squares of x1 = mul(x, f_norm) -> the factor of apply_gain(-10 - dBFS)
  long long s = 0;
  for (int64_t i = tid; i < count; i += kCmpLanes) {
    const int v = pcm_mul(x[i], f_norm);
    s += (long long)(v * v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) red_s[wave] = s;
  __syncthreads();
  s = 0;
  for (int w = 0; w < kCmpWaves; ++w) s += red_s[w];
  const CmpFactors f{f_norm, gain10_by_rms[pcm_rms(s, count)]};
  if (tid == 0) factors[clip] = f;
  __syncthreads();  // red_s is reused below

  // prefix[j] = sum of the energies of x2 over frames < j: thread t owns frames [t R, t R + R)
  const int64_t R = (L + kCmpLanes - 1) / kCmpLanes;
  const int64_t b = tid * R < L ? tid * R : L, e = b + R < L ? b + R : L;
  long long run = 0;
  for (int64_t j = b; j < e; ++j)
    for (int c = 0; c < C; ++c) {
      const int v = cmp_x2(x[j * C + c], f);
      run += (long long)(v * v);
    }
  long long incl = run;  // inclusive scan over the wave, then over the waves before this one
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) red_s[wave] = incl;
  __syncthreads();
  long long acc = incl - run;
  for (int w = 0; w < wave; ++w) acc += red_s[w];
  int64_t* prefix = prefix_all + (int64_t)clip * (L + 1);
  if (tid == 0) prefix[0] = 0;
  for (int64_t j = b; j < e; ++j) {
    for (int c = 0; c < C; ++c) {
      const int v = cmp_x2(x[j * C + c], f);
      acc += (long long)(v * v);
    }
    prefix[j + 1] = acc;
  }
  __syncthreads();  // the prefix sums of the whole clip are visible to the workgroup

  uint16_t* rms = rms_all + (int64_t)clip * L;
  for (int64_t i = tid; i < L; i += kCmpLanes) rms[i] = (uint16_t)cmp_window_rms(prefix, i, look, C);
}

// ---- the recurrence, sequential: one lane per clip, all L steps from 0.0
__global__ void __launch_bounds__(64) cmp_sequential_kernel(const uint16_t* __restrict__ rms_all, int N, int64_t L, CmpTables t,
                                                            double* __restrict__ traj_all) {
  const int clip = blockIdx.x * 64 + threadIdx.x;
  if (clip >= N) return;
  cmp_run(0.0, rms_all + (int64_t)clip * L, t, traj_all + (int64_t)clip * L, 0, L, false, nullptr, nullptr);
}

// ---- the recurrence, chunked: one workgroup per clip, K <= kCmpMaxChunks chunks of CH frames, lane t owns chunks
// [t q, t q + q).  Round 0 runs every chunk from 0.0 and finds the quiet ones (every frame the identity).  Each chunk's start
// is the end of the last non-quiet chunk before it (src), or 0.0.  Each repair round re-runs, from that end, every non-quiet
// chunk whose stored start differs from it bitwise, stopping at the first frame where the new state meets the stored
// trajectory; the loop ends after a round that re-ran nothing.  Quiet chunks hold their start: they are filled at the end.
__global__ void __launch_bounds__(kCmpLanes) cmp_chunked_kernel(const uint16_t* __restrict__ rms_all, int64_t L, int64_t CH, int K,
                                                                CmpTables t, double* __restrict__ traj_all, int32_t* __restrict__ rounds_out) {
  __shared__ double st[kCmpMaxChunks], en[kCmpMaxChunks];
  __shared__ int src[kCmpMaxChunks];
  __shared__ unsigned char quiet[kCmpMaxChunks];
  __shared__ int wmax_s[kCmpWaves];
  const int clip = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint16_t* rms = rms_all + (int64_t)clip * L;
  double* traj = traj_all + (int64_t)clip * L;
  const int q = (K + kCmpLanes - 1) / kCmpLanes;
  auto begin_of = [&](int k) { return (int64_t)k * CH; };
  auto end_of = [&](int k) { return (int64_t)k * CH + CH < L ? (int64_t)k * CH + CH : L; };

  for (int j = 0; j < kCmpPerLane; ++j) {
    const int k = tid * q + j;
    if (j < q && k < K) {
      bool loud = false;
      en[k] = cmp_run(0.0, rms, t, traj, begin_of(k), end_of(k), false, nullptr, &loud);
      st[k] = 0.0;
      quiet[k] = loud ? 0 : 1;
    }
  }
  __syncthreads();

  // src[k] = the last non-quiet chunk before k (-1: none): an exclusive max-scan over the lanes' runs of chunks
  int last = -1;
  for (int j = 0; j < kCmpPerLane; ++j) {
    const int k = tid * q + j;
    if (j < q && k < K && !quiet[k]) last = k;
  }
  int incl = last;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o);
    if (lane >= o) incl = max(incl, y);
  }
  if (lane == 63) wmax_s[wave] = incl;
  int excl = __shfl_up(incl, 1);
  if (lane == 0) excl = -1;
  __syncthreads();
  for (int w = 0; w < wave; ++w) excl = max(excl, wmax_s[w]);
  for (int j = 0; j < kCmpPerLane; ++j) {
    const int k = tid * q + j;
    if (j < q && k < K) {
      src[k] = excl;
      if (!quiet[k]) excl = k;
    }
  }
  __syncthreads();

  int rounds = 0;
  for (;;) {
    double want[kCmpPerLane];
    for (int j = 0; j < kCmpPerLane; ++j) {
      const int k = tid * q + j;
      want[j] = (j < q && k < K && src[k] >= 0) ? en[src[k]] : 0.0;
    }
    __syncthreads();  // every lane has read the ends of this round before any lane writes one
    int any = 0;
    for (int j = 0; j < kCmpPerLane; ++j) {
      const int k = tid * q + j;
      if (j < q && k < K && !quiet[k] && cmp_bits(want[j]) != cmp_bits(st[k])) {
        bool hit = false;
        const double z = cmp_run(want[j], rms, t, traj, begin_of(k), end_of(k), true, &hit, nullptr);
        if (!hit) en[k] = z;
        st[k] = want[j];
        any = 1;
      }
    }
    if (!__syncthreads_or(any)) break;
    ++rounds;
  }

  for (int j = 0; j < kCmpPerLane; ++j) {
    const int k = tid * q + j;
    if (j < q && k < K && quiet[k] && src[k] >= 0) {
      const double v = en[src[k]];
      if (cmp_bits(v) != 0)
        for (int64_t i = begin_of(k); i < end_of(k); ++i) traj[i] = v;
    }
  }
  if (tid == 0 && rounds_out) rounds_out[clip] = rounds;
}

// ---- apply: one thread per sample, into the workspace (the input stays intact until the filters' last pass)
__global__ void __launch_bounds__(kCmpApplyThreads) cmp_apply_kernel(const int16_t* in, int16_t* out, int64_t total, int64_t count,
                                                                     int64_t L, int C, const CmpFactors* __restrict__ factors,
                                                                     const double* __restrict__ traj_all, double margin,
                                                                     CmpFlag* __restrict__ flags, int64_t capacity,
                                                                     unsigned long long* __restrict__ n_flags) {
  for (int64_t i = (int64_t)blockIdx.x * kCmpApplyThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCmpApplyThreads) {
    const int64_t clip = i / count, frame = (i - clip * count) / C;
    const int x2 = cmp_x2(in[i], factors[clip]);
    const double att = traj_all[clip * L + frame];
    int y = x2;
    if (att != 0.0) {
      const double g = cmp_gain_dev(att);
      y = pcm_mul(x2, g);
      if (x2 != 0 && cmp_near_integer(pcm_dmul((double)x2, g), margin)) {
        const unsigned long long slot = atomicAdd(n_flags, 1ull);
        if ((int64_t)slot < capacity) flags[slot] = CmpFlag{i, att, x2, 0};
      }
    }
    out[i] = (int16_t)y;
  }
}

// ---- the host's values of the flagged samples back into the output
__global__ void __launch_bounds__(kCmpApplyThreads) cmp_scatter_kernel(const CmpFlag* __restrict__ flags, int64_t n, int16_t* out) {
  for (int64_t j = (int64_t)blockIdx.x * kCmpApplyThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kCmpApplyThreads)
    out[flags[j].index] = (int16_t)flags[j].value;
}

static unsigned cmp_grid(int64_t items) {
  const int64_t b = (items + kCmpApplyThreads - 1) / kCmpApplyThreads;
  return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

CmpLayout cmp_workspace_layout(int N, int L, int C) {
  CmpLayout w{};
  size_t at = 0;
  w.partials = at;
  at += align256((size_t)N * pcm_splits((int64_t)L * C) * sizeof(PcmPartial));
  w.factors = at;
  at += align256((size_t)N * sizeof(CmpFactors));
  w.traj = at;  // the prefix sums (N x (L + 1) int64) first, then the trajectories (N x L doubles)
  at += align256((size_t)N * ((size_t)L + 1) * sizeof(int64_t));
  w.rms = at;
  at += align256((size_t)N * L * sizeof(uint16_t));
  w.x3 = at;
  at += align256((size_t)N * L * C * sizeof(int16_t));
  w.count = at;
  at += 256;
  w.filters = at;
  at += pcm_filters_workspace_bytes(N, L, C);
  w.total = at;
  return w;
}

hipError_t launch_cmp_compress(const int16_t* in, int N, int L, int C, const double* boost_by_peak, const double* gain10_by_rms,
                               const uint8_t* above, const double* max_att, const double* inc, const double* dec, int look_frames,
                               int form, int chunk_frames, double margin, void* flags, int64_t flag_capacity, int32_t* rounds,
                               void* workspace, hipStream_t s) {
  const CmpLayout w = cmp_workspace_layout(N, L, C);
  char* ws = reinterpret_cast<char*>(workspace);
  PcmPartial* partials = reinterpret_cast<PcmPartial*>(ws + w.partials);
  CmpFactors* factors = reinterpret_cast<CmpFactors*>(ws + w.factors);
  double* traj = reinterpret_cast<double*>(ws + w.traj);
  uint16_t* rms = reinterpret_cast<uint16_t*>(ws + w.rms);
  int16_t* x3 = reinterpret_cast<int16_t*>(ws + w.x3);
  unsigned long long* n_flags = reinterpret_cast<unsigned long long*>(ws + w.count);
  const int64_t count = (int64_t)L * C;
  const CmpTables t{above, max_att, inc, dec};
  hipError_t e = hipMemsetAsync(n_flags, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  if ((e = launch_pcm_stats(in, N, count, partials, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(cmp_prepare_kernel, dim3((unsigned)N), dim3(kCmpLanes), 0, s, in, (int64_t)L, C, pcm_splits(count), partials,
                     boost_by_peak, gain10_by_rms, (int64_t)look_frames, factors, reinterpret_cast<int64_t*>(traj), rms);
  if (form == 0) {
    if (rounds && (e = hipMemsetAsync(rounds, 0, (size_t)N * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(cmp_sequential_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, rms, N, (int64_t)L, t, traj);
  } else {
    const int64_t CH = cmp_chunk_frames(L, chunk_frames);
    const int K = (int)((L + CH - 1) / CH);
    hipLaunchKernelGGL(cmp_chunked_kernel, dim3((unsigned)N), dim3(kCmpLanes), 0, s, rms, (int64_t)L, CH, K, t, traj, rounds);
  }
  const int64_t total = count * N;
  hipLaunchKernelGGL(cmp_apply_kernel, dim3(cmp_grid(total)), dim3(kCmpApplyThreads), 0, s, in, x3, total, count, (int64_t)L, C,
                     factors, traj, margin, reinterpret_cast<CmpFlag*>(flags), flag_capacity, n_flags);
  return hipGetLastError();
}

hipError_t launch_cmp_scatter(const void* flags, int64_t n, int16_t* out, hipStream_t s) {
  hipLaunchKernelGGL(cmp_scatter_kernel, dim3(cmp_grid(n)), dim3(kCmpApplyThreads), 0, s, reinterpret_cast<const CmpFlag*>(flags), n, out);
  return hipGetLastError();
}

}  // namespace rfx
