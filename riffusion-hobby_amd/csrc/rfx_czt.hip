// rfx_czt.hip - the framed transform and Griffin-Lim for STFT geometries whose FFT length has a prime factor above 13: the
// chirp-z engine (rfx_plan_options.frame_engine = RFX_ENGINE_CHIRPZ; rfx_czt_core.h has the arithmetic).  Same structure, same
// argument blocks, same frame layouts and the same companion kernels (fold, envelope, pack, unpack, mel: rfx_generic.hip) as the
// generic engine; the nc-point FFT of a frame is replaced by a circular convolution of length g.np >= 2 nc - 1 in LDS - chirp,
// forward passes, pointwise H, inverse passes, chirp - whose result is in natural order.  One workgroup per frame.
//     czt_stft_kernel  windowed frame x chirp -> convolution -> chirp x real split -> |X| or X
//     czt_gl_kernel    per frame: analysis of x_k - m x_{k-1}, convolution, [chirp, projection, conj chirp] pairwise in place,
//                      convolution, conj chirp x window -> synthesis frame -> HBM (gen_fold_kernel overlap-adds)
// The chirp c [nc] and H [buffer layout] are read from global memory (L2-resident: 8 (nc + np) bytes), in batches ahead of the
// LDS traffic that depends on them.  Bit-reproducible (no atomics).
// This file is compiled twice: as itself, and as rfx_czt_list.hip (`#define RFX_CZT_LIST_TU 1`, then this file), which holds only
// the Griffin-Lim kernels that walk a held call's free-frame list (rfx_guide_core.h) and their launcher.
#ifndef RFX_CZT_LIST_TU
#define RFX_CZT_LIST_TU 0
#endif
// ... and a third time as rfx_czt_loop.hip (`#define RFX_CZT_LOOP_TU 1`, then this file), which holds only the forward kernels of a loop
// call - czt_stft_loop_kernel, the row read modulo its length (include/rfx.h: rfx_stft_loop) - and their launcher; and a fourth time
// as rfx_czt_zero.hip (`#define RFX_CZT_LOOP_TU 2`): the same unit over czt_stft_zero_kernel, the zero-extended row of rfx_istft_backward.
#ifndef RFX_CZT_LOOP_TU
#define RFX_CZT_LOOP_TU 0
#endif
#include <hip/hip_runtime.h>

#include "rfx_czt_core.h"
#include "rfx_kernels.h"
#include "rfx_loop_core.h"
#include "rfx_istft_core.h"

namespace rfx {

constexpr int kCztThreads = 512;
#ifndef RFX_CZT_BATCH
#define RFX_CZT_BATCH 4
#endif

struct CztLds {
  cf* a;    // [gen_ibuf_elems(np, pad_shift)]
  cf* lo;   // [128]  exp(-2 pi i t / np)
  cf* hi;   // [nhi]  exp(-2 pi i 128 t / np)
  cf* lo2;  // [128]  exp(-2 pi i t / n_fft)
  cf* hi2;  // [nhi2] exp(-2 pi i 128 t / n_fft)
};

__device__ __forceinline__ CztLds czt_lds(char* smem, const GenGeom& g, const GenTables& tb) {
  CztLds l;
  l.a = reinterpret_cast<cf*>(smem);
  l.lo = l.a + gen_ibuf_elems(g.np, g.pad_shift);
  l.hi = l.lo + kGenTwLo;
  l.lo2 = l.hi + g.nhi;
  l.hi2 = l.lo2 + kGenTwLo;
  for (int i = threadIdx.x; i < kGenTwLo; i += blockDim.x) {
    l.lo[i] = tb.lo[i];
    l.lo2[i] = tb.lo2[i];
  }
  for (int i = threadIdx.x; i < g.nhi; i += blockDim.x) l.hi[i] = tb.hi[i];
  for (int i = threadIdx.x; i < g.nhi2; i += blockDim.x) l.hi2[i] = tb.hi2[i];
  return l;
}

// all passes of the np-point FFT in l.a (forward: digit-reversed out; inverse: digit-reversed in).  A barrier before every pass and
// one at the end.
template <bool INV, int MAXR>
__device__ __forceinline__ void czt_passes(const GenGeom& g, const CztLds& l, const cf* __restrict__ tw) {
  int L = INV ? 1 : g.np;
  int off = 0;  // this pass's slice of the exact twiddle tables
  if (INV) {
    int len = g.np;
    for (int s = 0; s < g.nstages; ++s) {
      const int m = len / g.radix[s];
      off += m * (g.radix[s] - 1);
      len = m;
    }
  }
  for (int i = 0; i < g.nstages; ++i) {
    const int R = g.radix[INV ? g.nstages - 1 - i : i];
    if (INV) {
      L *= R;
      off -= (L / R) * (R - 1);
    }
    __syncthreads();
    gen_ip_stage<INV, MAXR>(l.a, g.np, L, R, l.lo, l.hi, (int)threadIdx.x, (int)blockDim.x, g.pad_shift, tw + off);
    if (!INV) {
      off += (L / R) * (R - 1);
      L /= R;
    }
  }
  __syncthreads();
}
// steps 2 - 4: the circular convolution with the chirp.  Chirped data (zero tail included) in l.a, result in natural order in l.a
template <int MAXR>
__device__ __forceinline__ void czt_conv(const GenGeom& g, const CztLds& l, const cf* __restrict__ tw, const cf* __restrict__ H) {
  czt_passes<false, MAXR>(g, l, tw);
  czt_mul_h(l.a, H, g, (int)threadIdx.x, (int)blockDim.x);
  czt_passes<true, MAXR>(g, l, tw);
}

// step 1 on the analysis frame t of x (- mom xp): windowed, zero-padded (reflect-padded signal like torch.stft center=True), packed
// two reals per complex when n_fft is even, times the chirp.  Only the elements the window covers need loads; global loads of a
// batch first, then its LDS stores.  RULE 1 (czt_stft_loop_kernel): the row is one period of L samples, read modulo L (rfx_loop_core.h);
// RULE 2 (czt_stft_zero_kernel): the row is zero-extended (rfx_istft_core.h: zero_outside), an exact 0.0f outside [0, L).
template <int RULE = 0>
__device__ __forceinline__ void czt_load_frame(const GenGeom& g, cf* buf, const float* __restrict__ x, const float* __restrict__ xp, float mom, int L,
                                               int t, const float* __restrict__ win, const cf* __restrict__ c) {
  const int nthr = (int)blockDim.x, half = g.n_fft / 2;
  const int per = g.even ? 2 : 1;
  const int n_lo = g.left / per, n_hi = (g.left + g.win + per - 1) / per;
  for (int n = threadIdx.x; n < g.np; n += nthr)
    if (n < n_lo || n >= n_hi) buf[gen_ipad(n, g.pad_shift)] = cf{0.f, 0.f};  // the zero tail [nc, np) included
  constexpr int UL = RFX_CZT_BATCH;
  for (int n0 = n_lo + (int)threadIdx.x; n0 < n_hi; n0 += UL * nthr) {
    float xs[UL][2], ps[UL][2], ws[UL][2];
    cf cs[UL];
#pragma unroll
    for (int u = 0; u < UL; ++u) {
      const int n = n0 + u * nthr;
      cs[u] = c[n < n_hi ? n : n_lo];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        xs[u][e] = ps[u][e] = ws[u][e] = 0.f;
        if (e < per && n < n_hi) {
          const int i = per * n + e;  // position inside the padded frame
          const int j = i - g.left;   // position inside the window
          if (j >= 0 && j < g.win) {
            if (RULE == 2) {
              xs[u][e] = zero_outside_read(x, g.hop * t + i - half, L);
            } else {
              const int p = RULE == 1 ? loop_read_index(g.hop * t + i - half, L) : reflect_index(g.hop * t + i - half, L);
              xs[u][e] = x[p];
              if (xp) ps[u][e] = xp[p];
            }
            ws[u][e] = win[j];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UL; ++u) {
      const int n = n0 + u * nthr;
      if (n < n_hi) {
        const cf v{fmaf(-mom, ps[u][0], xs[u][0]) * ws[u][0], fmaf(-mom, ps[u][1], xs[u][1]) * ws[u][1]};
        buf[gen_ipad(n, g.pad_shift)] = czt_chirp(v, cs[u]);
      }
    }
  }
}

struct CztTab {
  const cf* c;  // [nc] chirp
  const cf* h;  // [gen_ibuf_elems(np, pad_shift)] spectrum of the wrapped conjugate chirp / np, in the buffer's layout
};

#if !RFX_CZT_LIST_TU
// ---- forward: frame fr of clip b is centred on sample hop*fr of the reflect-padded waveform (torch.stft center=True)
enum CztStftMode { kCztMag = 0, kCztSpec = 1 };

#define RFX_FWDK_LOOP RFX_CZT_LOOP_TU  // this unit: czt_stft_kernel; rfx_czt_loop.hip: czt_stft_loop_kernel
#include "rfx_czt_stft_kernel.hip.h"
#undef RFX_FWDK_LOOP

#endif  // !RFX_CZT_LIST_TU

#if !RFX_CZT_LOOP_TU
// ---- Griffin-Lim, one iteration for one frame per trip.  MODE 0: Z = S * angles0 (injected or drawn) -> synthesis;
// MODE 1: analysis of x_cur (the fold forms d = x_k - m x_{k-1}); MODE 2: analysis of x_cur - m x_prev
// RFX_CZT_LIST_TU (a held call's launches 1 .. n_iter): trip i of the loop takes frame list[i], list[B T] trips in all
template <int MODE, int MAXR>
__global__ void __launch_bounds__(kCztThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
#if RFX_CZT_LIST_TU
czt_gl_list_kernel(GenGlArgs a, CztTab ct, const int* __restrict__ list) {
#else
czt_gl_kernel(GenGlArgs a, CztTab ct) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GenGeom& g = a.g;
  const CztLds l = czt_lds(smem, g, a.tb);
  const long long nframes = (long long)a.B * a.T;
  const float scale = 1.0f / (float)g.nc;  // even: z = IFFT_nc(Z) ; odd: x = Re IFFT_n(Z)
  const int npairs = gen_pair_count(g);
  const int nthr = (int)blockDim.x;
#if RFX_CZT_LIST_TU
  const long long ntrips = list[nframes];
  for (long long trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
    const long long fr = list[trip];
#else
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
#endif
    const int clip = (int)(fr / a.T), t = (int)(fr - (long long)clip * a.T);
    const float eps2 = a.row_scale ? a.row_scale[2 * clip + 1] : 1e-32f;
    (void)eps2;
    const size_t base = (size_t)fr * g.fs;
    const float* __restrict__ S = a.S + base;
    __syncthreads();  // the previous frame's output loop is done with the buffer
    if (MODE == 0) {
      auto X = [&](int k) {
        cf ang;
        if (a.angles0) ang = a.angles0[base + k];
        else ang = rand_unit_pair(rand_frame_key(a.seed, a.frame_base + (unsigned long long)fr), k);
        const float s = S[k];
        return cf{s * ang.re, s * ang.im};
      };
      // batches: the chirp and the two one-sided bins (|S|, angle) of every element first, then the merge and the LDS stores
      constexpr int UI = RFX_CZT_BATCH;
      for (int k0 = threadIdx.x; k0 < g.nc; k0 += UI * nthr) {
        cf cv[UI], xa[UI], xb[UI];
#pragma unroll
        for (int u = 0; u < UI; ++u) {
          const int k = k0 + u * nthr;
          const int kk = k < g.nc ? k : 0;
          cv[u] = ct.c[kk];
          xa[u] = X(gen_split_bin_a(g, kk));
          xb[u] = X(gen_split_bin_b(g, kk));
        }
#pragma unroll
        for (int u = 0; u < UI; ++u) {
          const int k = k0 + u * nthr;
          if (k < g.nc) l.a[gen_ipad(k, g.pad_shift)] = czt_chirp_conj(gen_split_inverse_vals(g, xa[u], xb[u], l.lo2, l.hi2, k), cv[u]);
        }
      }
    } else {
      czt_load_frame(g, l.a, a.x_cur + (size_t)clip * a.audio_stride, MODE == 2 ? a.x_prev + (size_t)clip * a.audio_stride : nullptr,
                     MODE == 2 ? a.mom : 0.f, a.L, t, a.tb.win, ct.c);
      czt_conv<MAXR>(g, l, a.tb.tw, ct.h);  // ends with a barrier; the convolution's output in natural order in l.a
      // chirp / projection / conj chirp, pairwise in place (czt_pair_compute).  Batches of UP pairs per thread: every global load of
      // the batch (chirp, |S|), then the LDS reads, the arithmetic, the stores
      constexpr int UP = RFX_CZT_BATCH;
      for (int k0 = threadIdx.x; k0 < npairs; k0 += UP * nthr) {
        GenPair pr[UP];
        cf ck[UP], cc[UP];
        int pk[UP], pc[UP];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const int k = k0 + u * nthr;
          const int kk = k < npairs ? k : 0;
          const int kc = czt_pair_partner(g, kk);
          pr[u].k = kk;
          pk[u] = gen_ipad(kk, g.pad_shift);
          pc[u] = gen_ipad(kc, g.pad_shift);
          ck[u] = ct.c[kk];
          cc[u] = ct.c[kc];
          pr[u].sk = S[kk];
          pr[u].sc = g.even ? S[g.nc - kk] : 0.f;  // even, k == 0: bin nc
        }
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          pr[u].zk = l.a[pk[u]];
          pr[u].zc = l.a[pc[u]];
        }
#pragma unroll
        for (int u = 0; u < UP; ++u) czt_pair_compute(pr[u], g, ck[u], cc[u], l.lo2, l.hi2, eps2);
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const int k = k0 + u * nthr;
          if (k < npairs) {
            l.a[pk[u]] = pr[u].zk;
            if (czt_pair_has_partner(g, k)) l.a[pc[u]] = pr[u].zc;
          }
        }
      }
    }
    czt_zero_tail(l.a, g, (int)threadIdx.x, nthr);
    czt_conv<MAXR>(g, l, a.tb.tw, ct.h);  // starts and ends with a barrier
    float* __restrict__ out = a.frames + (size_t)fr * g.fpitch + g.fshift;
    constexpr int UO = RFX_CZT_BATCH;  // window and chirp samples fetched per batch before the stores
    for (int j0 = threadIdx.x; j0 < g.win; j0 += UO * nthr) {
      float wv[UO];
      cf cv[UO], zv[UO];
      int iv[UO];
#pragma unroll
      for (int u = 0; u < UO; ++u) {
        const int j = j0 + u * nthr;
        const int jj = j < g.win ? j : 0;
        iv[u] = jj + g.left;
        wv[u] = a.tb.win[jj];
        cv[u] = ct.c[g.even ? iv[u] >> 1 : iv[u]];
      }
#pragma unroll
      for (int u = 0; u < UO; ++u) zv[u] = l.a[gen_ipad(g.even ? iv[u] >> 1 : iv[u], g.pad_shift)];
#pragma unroll
      for (int u = 0; u < UO; ++u) {
        const int j = j0 + u * nthr;
        if (j < g.win) out[j] = czt_out_sample(g, zv[u], cv[u], iv[u]) * scale * wv[u];
      }
    }
  }
}
#endif  // !RFX_CZT_LOOP_TU

// --------------------------------------------------------------------------------------------------------------------
static int czt_grid(const GenGeom& g, int num_cus, long long nframes) {
  // resident workgroups: LDS bound (160 KiB per CU) and register bound (256 VGPRs: 8 waves per CU)
  int per_cu = (int)(kCztLdsLimit / (czt_lds_bytes(g) + 512));
  if (per_cu < 1) per_cu = 1;
  const int by_waves = 512 / g.nthr;
  if (per_cu > by_waves) per_cu = by_waves < 1 ? 1 : by_waves;
  const long long n = (long long)num_cus * per_cu;
  return (int)(n < nframes ? n : nframes);
}

#if RFX_CZT_LIST_TU
using CztGlListFn = void (*)(GenGlArgs, CztTab, const int*);
static CztGlListFn czt_gl_list_fn(const GenGeom& g) {
  const int c = gen_radix_class(g.radix, g.nstages);
  return c == 5 ? czt_gl_list_kernel<1, 5> : c == 7 ? czt_gl_list_kernel<1, 7> : czt_gl_list_kernel<1, 13>;
}
hipError_t prepare_czt_list_kernels(const GenGeom& g) {
  return hipFuncSetAttribute((const void*)czt_gl_list_fn(g), hipFuncAttributeMaxDynamicSharedMemorySize, (int)czt_lds_bytes(g));
}
hipError_t launch_czt_gl_list(const GenGlArgs& a, const int* list, const cf* chirp, const cf* h, int num_cus, hipStream_t stream) {
  const int grid = czt_grid(a.g, num_cus, (long long)a.B * a.T);
  hipLaunchKernelGGL(czt_gl_list_fn(a.g), dim3(grid), dim3(a.g.nthr), czt_lds_bytes(a.g), stream, a, CztTab{chirp, h}, list);
  return hipGetLastError();
}
#elif RFX_CZT_LOOP_TU
#if RFX_CZT_LOOP_TU == 2  // rfx_czt_zero.hip: the dispatch below over the zero-extension twins, under their own names
#define czt_stft_loop_kernel czt_stft_zero_kernel
#define czt_stft_loop_fn czt_stft_zero_fn
#define prepare_czt_loop_kernels prepare_czt_zero_kernels
#define launch_czt_stft_loop launch_czt_stft_zero
#endif
// the forward kernels of a loop call by (mode, radix class of the pass length)
using CztStftFn = void (*)(GenStftArgs, CztTab);
template <int MAXR>
static CztStftFn czt_stft_loop_fn(int mode) {
  return mode == kCztMag ? czt_stft_loop_kernel<kCztMag, MAXR> : czt_stft_loop_kernel<kCztSpec, MAXR>;
}
static CztStftFn czt_stft_loop_fn(const GenGeom& g, int mode) {
#ifdef RFX_CZT_CLASS
  return czt_stft_loop_fn<RFX_CZT_CLASS>(mode);
#else
  const int c = gen_radix_class(g.radix, g.nstages);
  return c == 5 ? czt_stft_loop_fn<5>(mode) : c == 7 ? czt_stft_loop_fn<7>(mode) : czt_stft_loop_fn<13>(mode);
#endif
}
hipError_t prepare_czt_loop_kernels(const GenGeom& g) {
  hipError_t e;
  for (int mode = 0; mode < 2; ++mode)
    if ((e = hipFuncSetAttribute((const void*)czt_stft_loop_fn(g, mode), hipFuncAttributeMaxDynamicSharedMemorySize, (int)czt_lds_bytes(g))) != hipSuccess) return e;
  return hipSuccess;
}
hipError_t launch_czt_stft_loop(int mode, const GenStftArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream) {
  const int grid = czt_grid(a.g, num_cus, (long long)a.B * a.T);
  hipLaunchKernelGGL(czt_stft_loop_fn(a.g, mode), dim3(grid), dim3(a.g.nthr), czt_lds_bytes(a.g), stream, a, CztTab{chirp, h});
  return hipGetLastError();
}
#else
// kernels by (mode, radix class of the pass length)
using CztStftFn = void (*)(GenStftArgs, CztTab);
using CztGlFn = void (*)(GenGlArgs, CztTab);
template <int MAXR>
static CztStftFn czt_stft_fn(int mode) {
  return mode == kCztMag ? czt_stft_kernel<kCztMag, MAXR> : czt_stft_kernel<kCztSpec, MAXR>;
}
// (RFX_CZT_CLASS: instantiate ONE radix class - tests/test_czt_isa.py reads the three classes' ISA from three parallel compiles)
static CztStftFn czt_stft_fn(const GenGeom& g, int mode) {
#ifdef RFX_CZT_CLASS
  return czt_stft_fn<RFX_CZT_CLASS>(mode);
#else
  const int c = gen_radix_class(g.radix, g.nstages);
  return c == 5 ? czt_stft_fn<5>(mode) : c == 7 ? czt_stft_fn<7>(mode) : czt_stft_fn<13>(mode);
#endif
}
template <int MAXR>
static CztGlFn czt_gl_fn(int mode) {
  return mode == 0 ? czt_gl_kernel<0, MAXR> : mode == 1 ? czt_gl_kernel<1, MAXR> : czt_gl_kernel<2, MAXR>;
}
static CztGlFn czt_gl_fn(const GenGeom& g, int mode) {
#ifdef RFX_CZT_CLASS
  return czt_gl_fn<RFX_CZT_CLASS>(mode);
#else
  const int c = gen_radix_class(g.radix, g.nstages);
  return c == 5 ? czt_gl_fn<5>(mode) : c == 7 ? czt_gl_fn<7>(mode) : czt_gl_fn<13>(mode);
#endif
}

hipError_t prepare_czt_kernels(const GenGeom& g) {
  const int lds = (int)czt_lds_bytes(g);
  hipError_t e;
  for (int mode = 0; mode < 2; ++mode)
    if ((e = hipFuncSetAttribute((const void*)czt_stft_fn(g, mode), hipFuncAttributeMaxDynamicSharedMemorySize, lds)) != hipSuccess) return e;
  for (int mode = 0; mode < 3; ++mode)
    if ((e = hipFuncSetAttribute((const void*)czt_gl_fn(g, mode), hipFuncAttributeMaxDynamicSharedMemorySize, lds)) != hipSuccess) return e;
  return hipSuccess;
}

hipError_t launch_czt_stft(int mode, const GenStftArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream) {
  const int grid = czt_grid(a.g, num_cus, (long long)a.B * a.T);
  hipLaunchKernelGGL(czt_stft_fn(a.g, mode), dim3(grid), dim3(a.g.nthr), czt_lds_bytes(a.g), stream, a, CztTab{chirp, h});
  return hipGetLastError();
}

hipError_t launch_czt_gl(int mode, const GenGlArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream) {
  const int grid = czt_grid(a.g, num_cus, (long long)a.B * a.T);
  hipLaunchKernelGGL(czt_gl_fn(a.g, mode), dim3(grid), dim3(a.g.nthr), czt_lds_bytes(a.g), stream, a, CztTab{chirp, h});
  return hipGetLastError();
}
#endif  // RFX_CZT_LIST_TU

}  // namespace rfx
