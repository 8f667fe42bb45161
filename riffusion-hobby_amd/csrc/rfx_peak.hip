// rfx_peak.hip - the spectral-peak start of Griffin-Lim (include/rfx.h: rfx_peak_start; arithmetic in rfx_peak_core.h): initial
// angles built from the magnitudes alone.  Three launches; the frame kernels run 1024-thread workgroups (16 wave64):
//   1. owners: one workgroup per frame, the frame in LDS in bin order (8821 floats = 35 KB at the default geometry, 53 KB with the
//      owners: two workgroups, the 32 waves a CU takes).  The frame's maximum (wave shuffles, one value per wave through LDS), then
//      every thread takes one contiguous chunk of at most 10 bins into registers and finds its last and first peak.  What crosses
//      chunks is the nearest peak on either side: a scan over the 64 lanes of a wave by shuffles (6 steps), over the 16 waves by
//      reading their totals from LDS - one barrier, where a workgroup-wide Hillis-Steele scan in LDS takes 10 steps of two barriers,
//      each of them a wait of all 16 waves.  Writes the owning peak of every bin (uint16) and, at the peaks, the interpolated
//      position (double).
//   2. chain: one workgroup of 512 threads per row (20 bins a thread: its state fits the registers of 8 waves, and a barrier waits for
//      8 waves, not 16) walks the row's T frames; phase and position of the previous frame's peaks stay in LDS (two
//      doubles per bin: 141 KB at the default geometry - one workgroup per CU, which is all a batch of rows asks for).  Sequential
//      over frames and latency-bound: two barriers per frame; what a frame reads from memory (its owners, its peaks' positions) is
//      requested one and two frames ahead, under the arithmetic of the frames before.  Overwrites the peaks' positions with their
//      phases.
//   3. angles: one workgroup per frame stages the frame's owners and its peaks' phases in LDS (independent loads, no dependent
//      gather from memory), then a thread per output position: the owner's phase, cos / sin in float32, (-1)^bin, conjugated in
//      the conjugate slots of the specialised layout, 0 in the padding.
// Frames go on grid x (up to 2^31 - 1); every offset is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "rfx_holdmask_core.h"
#include "rfx_kernels.h"
#include "rfx_peak_core.h"

namespace rfx {

constexpr int kPeakWaves = kPeakThreads / 64;
constexpr int kPeakFar = 0x7fffffff;  // "no peak above"

template <int LAYOUT>
__global__ void __launch_bounds__(kPeakThreads) peak_owner_kernel(const float* __restrict__ S, const int* __restrict__ bin_of,
                                                                  uint16_t* __restrict__ own, double* __restrict__ val, int stride, int F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* m = reinterpret_cast<float*>(smem);                       // [F] the frame in bin order
  uint16_t* ow = reinterpret_cast<uint16_t*>(m + ((F + 1) & ~1));  // [F] the owner of every bin
  __shared__ float wave_max[kPeakWaves];
  __shared__ int wave_last[kPeakWaves], wave_first[kPeakWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t fr = blockIdx.x;
  // a bin the layout stores twice holds the same value in both places (rfx_pack_magnitudes, InverseMelScale): either store serves
#pragma unroll 4
  for (int p = tid; p < stride; p += kPeakThreads) {
    const int bin = holdmask_slot_bin(LAYOUT, p, F, bin_of);
    if (bin >= 0) m[bin] = S[fr * (size_t)stride + p];
  }
  __syncthreads();
  // this thread's chunk of bins [c0, c0 + per), with one neighbour on either side, in registers
  const int per = (F + kPeakThreads - 1) / kPeakThreads;  // <= kPeakBins
  const int c0 = tid * per;
  float v[kPeakBins + 2];
#pragma unroll
  for (int j = 0; j < kPeakBins + 2; ++j) {
    const int k = c0 - 1 + j;
    v[j] = j < per + 2 && k >= 0 && k < F ? m[k] : -INFINITY;  // (what lies outside the frame is never compared: peak_is3)
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 1; j <= kPeakBins; ++j)
    if (j <= per) mx = peak_max(mx, v[j]);
  for (int d = 32; d > 0; d >>= 1) mx = peak_max(mx, __shfl_xor(mx, d));
  if (lane == 0) wave_max[wave] = mx;
  __syncthreads();
  mx = wave_max[0];
  for (int w = 1; w < kPeakWaves; ++w) mx = peak_max(mx, wave_max[w]);
  const float thr = peak_threshold(mx);
  unsigned flags = 0;  // bit j: bin c0 + j is a peak
  int last = -1, first = kPeakFar;
#pragma unroll
  for (int j = 0; j < kPeakBins; ++j) {
    const int k = c0 + j;
    if (j < per && k < F && peak_is3(v[j], v[j + 1], v[j + 2], k, F, thr)) {
      flags |= 1u << j;
      last = k;
      if (first == kPeakFar) first = k;
    }
  }
  // the largest peak at or below this chunk's end and the smallest at or above its start, over the wave, then over the waves
  int incl_last = last, incl_first = first;
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_up(incl_last, d), b = __shfl_down(incl_first, d);
    if (lane >= d) incl_last = max(incl_last, a);
    if (lane + d < 64) incl_first = min(incl_first, b);
  }
  if (lane == 63) wave_last[wave] = incl_last;
  if (lane == 0) wave_first[wave] = incl_first;
  int prev = __shfl_up(incl_last, 1), next = __shfl_down(incl_first, 1);
  if (lane == 0) prev = -1;
  if (lane == 63) next = kPeakFar;
  __syncthreads();
  for (int w = 0; w < wave; ++w) prev = max(prev, wave_last[w]);
  for (int w = wave + 1; w < kPeakWaves; ++w) next = min(next, wave_first[w]);
  if (next == kPeakFar) next = -1;
  // owners: forward for the largest peak at or below every bin, backward for the smallest above it
  int pv[kPeakBins];
#pragma unroll
  for (int j = 0; j < kPeakBins; ++j) {
    if ((flags >> j) & 1u) prev = c0 + j;
    pv[j] = prev;
  }
#pragma unroll
  for (int j = kPeakBins - 1; j >= 0; --j) {
    const int k = c0 + j;
    if (j < per && k < F) {
      const int o = peak_owner(k, pv[j], next);
      ow[k] = o < 0 ? kPeakNone : (uint16_t)o;
    }
    if ((flags >> j) & 1u) next = k;
  }
  __syncthreads();
  for (int k = tid; k < F; k += kPeakThreads) {
    const uint16_t o = ow[k];
    own[fr * (size_t)F + k] = o;
    if ((int)o == k) val[fr * (size_t)F + k] = peak_pos(k, m[k - 1], m[k], m[k + 1]);  // (a peak is never bin 0 or F - 1)
  }
}

__global__ void __launch_bounds__(kPeakChainThreads) peak_chain_kernel(const uint16_t* __restrict__ own, double* __restrict__ val, int T, int F, int hop,
                                                                  int n_fft) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* phi_s = reinterpret_cast<double*>(smem);  // [F] phase of the previous frame's peaks, by bin
  double* pos_s = phi_s + F;                        // [F] their positions
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * (size_t)T * (size_t)F;
  const double turns = peak_turns_per_bin(hop, n_fft);
  // bins tid + 512 i; a bin past F never equals its owner entry.  o0: owners of frame t - 1, o1: of t, o2: of t + 1; p1: positions of t
  uint16_t o0[kPeakChainBins], o1[kPeakChainBins], o2[kPeakChainBins];
  double p1[kPeakChainBins];
#pragma unroll
  for (int i = 0; i < kPeakChainBins; ++i) {
    const int k = tid + i * kPeakChainThreads;
    o0[i] = kPeakNone;  // frame 0 starts every chain
    o1[i] = k < F ? own[base + k] : kPeakNone;
    o2[i] = k < F && T > 1 ? own[base + F + k] : kPeakNone;
  }
#pragma unroll
  for (int i = 0; i < kPeakChainBins; ++i) {
    const int k = tid + i * kPeakChainThreads;
    p1[i] = (int)o1[i] == k ? val[base + k] : 0.0;
  }
  for (int t = 0; t < T; ++t) {
    const size_t at = base + (size_t)t * (size_t)F;
    // requested now, used in the next trip: the positions of frame t + 1 (its owners came a trip ago) and the owners of frame t + 2
    uint16_t o3[kPeakChainBins];
    double p2[kPeakChainBins];
#pragma unroll
    for (int i = 0; i < kPeakChainBins; ++i) {
      const int k = tid + i * kPeakChainThreads;
      p2[i] = (int)o2[i] == k ? val[at + F + k] : 0.0;
      o3[i] = t + 2 < T && k < F ? own[at + 2 * (size_t)F + k] : kPeakNone;
    }
    // q: the previous frame's peak that owns this bin; none: the previous frame was empty, a chain starts.  Branch-free - a wave has
    // a peak in nearly every one of its 20 trips, so all lanes read (entry 0 where there is nothing to read) and the reads overlap
    double phi[kPeakChainBins];
#pragma unroll
    for (int i = 0; i < kPeakChainBins; ++i) {
      const int k = tid + i * kPeakChainThreads;
      const bool chained = (int)o1[i] == k && o0[i] != kPeakNone;
      const int q = chained ? (int)o0[i] : 0;
      const double a = peak_advance(phi_s[q], pos_s[q], p1[i], turns);
      phi[i] = chained ? a : 0.0;
    }
    __syncthreads();  // every read of the previous frame's state is done
#pragma unroll
    for (int i = 0; i < kPeakChainBins; ++i) {
      const int k = tid + i * kPeakChainThreads;
      if ((int)o1[i] == k) {
        phi_s[k] = phi[i];
        pos_s[k] = p1[i];
        val[at + k] = phi[i];
      }
      o0[i] = o1[i];
      o1[i] = o2[i];
      o2[i] = o3[i];
      p1[i] = p2[i];
    }
    __syncthreads();
  }
}

template <bool SPEC>
__global__ void __launch_bounds__(kPeakThreads) peak_angles_kernel(const uint16_t* __restrict__ own, const double* __restrict__ val,
                                                                   cf* __restrict__ out, int stride, int F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* phi_s = reinterpret_cast<float*>(smem);                       // [F] the peaks' phases, by bin
  uint16_t* ow = reinterpret_cast<uint16_t*>(phi_s + ((F + 1) & ~1));  // [F] the owner of every bin
  const int tid = threadIdx.x;
  const size_t fr = blockIdx.x;
  const uint16_t* o_fr = own + fr * (size_t)F;
  const double* v_fr = val + fr * (size_t)F;
  uint16_t o[kPeakBins];
#pragma unroll
  for (int i = 0; i < kPeakBins; ++i) {
    const int k = tid + i * kPeakThreads;
    o[i] = k < F ? o_fr[k] : kPeakNone;
  }
#pragma unroll
  for (int i = 0; i < kPeakBins; ++i) {
    const int k = tid + i * kPeakThreads;
    if (k < F) {
      ow[k] = o[i];
      if ((int)o[i] == k) phi_s[k] = (float)v_fr[k];
    }
  }
  __syncthreads();
#pragma unroll 2
  for (int p = tid; p < stride; p += kPeakThreads) {
    int bin = -1;
    bool cj = false;
    if (SPEC) {
      int q, kb;
      if (pos_c_to_slot(p, q, kb)) bin = slot_bin(q / 21, q % 21, kb, &cj);
    } else if (p < F) {
      bin = p;
    }
    cf v{0.f, 0.f};
    if (bin >= 0) {
      const uint16_t w = ow[bin];
      v = peak_angle(w == kPeakNone ? 0.f : phi_s[w], bin);
      if (cj) v.im = -v.im;
    }
    out[fr * (size_t)stride + p] = v;
  }
}

// the owner kernel's frame and owners; the angles kernel's phases and owners take the same
size_t peak_owner_lds_bytes(int F) { return (size_t)((F + 1) & ~1) * sizeof(float) + (size_t)F * sizeof(uint16_t); }
size_t peak_chain_lds_bytes(int F) { return 2 * (size_t)F * sizeof(double); }

hipError_t launch_peak_start(int layout, const float* S, const int* bin_of, int B, int T, int stride_in, int n_stft, int hop, int n_fft,
                             uint16_t* own, double* val, cf* angles, int stride_out, hipStream_t stream) {
  const unsigned nframes = (unsigned)((long long)B * T);
  const size_t lds1 = peak_owner_lds_bytes(n_stft), lds2 = peak_chain_lds_bytes(n_stft);
  const void* fn = layout == kHoldMaskSpec    ? (const void*)peak_owner_kernel<kHoldMaskSpec>
                   : layout == kHoldMaskTable ? (const void*)peak_owner_kernel<kHoldMaskTable>
                                              : (const void*)peak_owner_kernel<kHoldMaskPlain>;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
  if (e != hipSuccess) return e;
  if (layout == kHoldMaskSpec)
    hipLaunchKernelGGL(peak_owner_kernel<kHoldMaskSpec>, dim3(nframes), dim3(kPeakThreads), lds1, stream, S, bin_of, own, val, stride_in, n_stft);
  else if (layout == kHoldMaskTable)
    hipLaunchKernelGGL(peak_owner_kernel<kHoldMaskTable>, dim3(nframes), dim3(kPeakThreads), lds1, stream, S, bin_of, own, val, stride_in, n_stft);
  else
    hipLaunchKernelGGL(peak_owner_kernel<kHoldMaskPlain>, dim3(nframes), dim3(kPeakThreads), lds1, stream, S, bin_of, own, val, stride_in, n_stft);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipFuncSetAttribute((const void*)peak_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2)) != hipSuccess) return e;
  hipLaunchKernelGGL(peak_chain_kernel, dim3((unsigned)B), dim3(kPeakChainThreads), lds2, stream, own, val, T, n_stft, hop, n_fft);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const void* afn = layout == kHoldMaskSpec ? (const void*)peak_angles_kernel<true> : (const void*)peak_angles_kernel<false>;
  if ((e = hipFuncSetAttribute(afn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1)) != hipSuccess) return e;
  if (layout == kHoldMaskSpec)
    hipLaunchKernelGGL(peak_angles_kernel<true>, dim3(nframes), dim3(kPeakThreads), lds1, stream, own, val, angles, stride_out, n_stft);
  else
    hipLaunchKernelGGL(peak_angles_kernel<false>, dim3(nframes), dim3(kPeakThreads), lds1, stream, own, val, angles, stride_out, n_stft);
  return hipGetLastError();
}

}  // namespace rfx
