// rfx_guide_bwd.hip - the guide projection of the guided decode's backward (include/rfx.h: rfx_griffinlim_guided_backward;
// arithmetic: rfx_guide_core.h, guide_project).  It reads the gradient slots G the synthesis adjoint wrote (rfx_istft_backward) and
// the spectrum slots a the plan's forward transform wrote from the staged guide - two complex cubes in the same layout - and writes
// g_S = Re(conj(u) G), u = a / (|a| + 1e-16), in the magnitude slot layout rfx_inverse_mel_lstsq_backward reads.
//
// One frame per trip, the structure of the slot kernels of rfx_mel_bwd.hip.  Phase 1: both cubes 16 bytes (two complex values) per
// lane in the order they lie in memory; the value of position x goes to v[x] in LDS (every position has one writer; padding: 0,
// whatever the cubes hold there).  Phase 2: the magnitude slots, 16 bytes (four floats) per lane: slot p takes v[s2x[p]] - a bin
// the layout holds twice gets, in each slot, the value made from the complex pair that slot multiplied in the forward - and the
// padding 0: every float of the output is written and finite where G and a are.  No atomics; a frame's bytes are a function of
// that frame's slots alone, not of B or the grid.  Memory-bound: 16 + 4 bytes per position against one fused multiply-add, a square
// root and a divide.
#include <hip/hip_runtime.h>

#include "rfx_guide_core.h"
#include "rfx_kernels.h"

namespace rfx {

constexpr int kGuideProjectThreads = 512;

__global__ void __launch_bounds__(kGuideProjectThreads) guide_project_kernel(GuideProjectArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gp_lds[];
  float2* __restrict__ v2 = reinterpret_cast<float2*>(gp_lds);  // [xstride] floats
  const long long nframes = (long long)a.B * a.T;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const int2* __restrict__ xb2 = reinterpret_cast<const int2*>(a.xpos_bin);
  const int4* __restrict__ sx4 = reinterpret_cast<const int4*>(a.s2x);
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    const float4* __restrict__ G4 = reinterpret_cast<const float4*>(a.G + (size_t)fr * a.xstride);
    const float4* __restrict__ A4 = reinterpret_cast<const float4*>(a.A + (size_t)fr * a.xstride);
    for (int i = tid; i < a.xstride / 2; i += nthr) {
      const float4 g = G4[i], x = A4[i];
      const int2 k = xb2[i];
      // (both values are formed whatever the position holds and the padding's is dropped: the two cubes are read 16 bytes at a time)
      const float p0 = guide_project(cf{x.x, x.y}, cf{g.x, g.y}), p1 = guide_project(cf{x.z, x.w}, cf{g.z, g.w});
      v2[i] = float2{k.x >= 0 ? p0 : 0.f, k.y >= 0 ? p1 : 0.f};
    }
    __syncthreads();
    float4* __restrict__ S4 = reinterpret_cast<float4*>(a.out + (size_t)fr * a.sstride);
    auto slot = [&](int x) { return x < 0 ? 0.f : gp_lds[x]; };
    for (int i = tid; i < a.sstride / 4; i += nthr) {
      const int4 x = sx4[i];
      S4[i] = float4{slot(x.x), slot(x.y), slot(x.z), slot(x.w)};
    }
    __syncthreads();  // the next trip rewrites the values
  }
}

// xstride even, sstride a multiple of four, every s2x entry below xstride; G, A and out 16-byte aligned (the host has checked)
hipError_t launch_guide_project(const GuideProjectArgs& a, hipStream_t stream) {
  const long long nframes = (long long)a.B * a.T;
  if (nframes <= 0) return hipSuccess;
  const size_t lds = sizeof(float) * (size_t)a.xstride;
  if (lds > 48u * 1024u) {
    const hipError_t e = hipFuncSetAttribute((const void*)guide_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long long cap = 1 << 16;
  hipLaunchKernelGGL(guide_project_kernel, dim3((unsigned)(nframes < cap ? nframes : cap)), dim3(kGuideProjectThreads), lds, stream, a);
  return hipGetLastError();
}

}  // namespace rfx
