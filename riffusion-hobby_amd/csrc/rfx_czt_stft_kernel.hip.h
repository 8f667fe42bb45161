// rfx_czt_stft_kernel.hip.h - the forward frame kernel of the chirp-z engine, included once by each of two units of rfx_czt.hip:
//   RFX_FWDK_LOOP 0  czt_stft_kernel<MODE, MAXR>       (rfx_czt.hip itself) the row is reflect-padded (torch.stft center=True): the text this kernel
//                                                      always had
//   RFX_FWDK_LOOP 1  czt_stft_loop_kernel<MODE, MAXR>  (rfx_czt_loop.hip) a loop forward call (include/rfx.h: rfx_stft_loop): the row of a.Lw = hop a.T
//                                                      samples is one period and is read modulo a.Lw (czt_load_frame<1>; rfx_loop_core.h)
// One text, chosen at compile time.  (The engine's Griffin-Lim kernels have no circular variant: it still refuses a loop DECODE.)
// (two waves per SIMD = 256 VGPRs for every radix class: a kernel holds the forward AND the inverse passes - the Griffin-Lim kernel
// two of each - and under the generic engine's 128-register bound of the 2 / 3 / 5 / 7 classes the compiler spilled 180 - 370 bytes per
// thread inside the frame loop, whatever the batch sizes below.  One 512-thread workgroup per CU then; the buffer of the lengths this
// engine is for - 137 KB at n_fft 17028 - leaves no room for a second one anyway)
template <int MODE, int MAXR>
__global__ void __launch_bounds__(kCztThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
#if RFX_FWDK_LOOP == 2
czt_stft_zero_kernel(GenStftArgs a, CztTab ct) {  // (rfx_czt_zero.hip) the row is zero-extended: rfx_istft_backward's analysis
#elif RFX_FWDK_LOOP
czt_stft_loop_kernel(GenStftArgs a, CztTab ct) {
#else
czt_stft_kernel(GenStftArgs a, CztTab ct) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GenGeom& g = a.g;
  const CztLds l = czt_lds(smem, g, a.tb);
  const long long nframes = (long long)a.B * a.T;
  const int nthr = (int)blockDim.x;
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    const int clip = (int)(fr / a.T), t = (int)(fr - (long long)clip * a.T);
    __syncthreads();  // previous frame's epilogue is done with the buffer
    czt_load_frame<RFX_FWDK_LOOP>(g, l.a, a.wave + (size_t)clip * a.wave_stride, nullptr, 0.f, a.Lw, t, a.tb.win, ct.c);
    czt_conv<MAXR>(g, l, a.tb.tw, ct.h);
    const size_t base = (size_t)fr * g.fs;
    constexpr int UB = RFX_CZT_BATCH;
    for (int k0 = threadIdx.x; k0 < g.fs; k0 += UB * nthr) {
      int ea[UB], eb[UB];
      cf ca[UB], cb[UB], za[UB], zb[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int k = k0 + u * nthr;
        const int kk = k < g.n_stft ? k : 0;
        ea[u] = czt_bin_elem_a(g, kk);
        eb[u] = czt_bin_elem_b(g, kk);
        ca[u] = ct.c[ea[u]];
        cb[u] = ct.c[eb[u]];
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        za[u] = l.a[gen_ipad(ea[u], g.pad_shift)];
        zb[u] = l.a[gen_ipad(eb[u], g.pad_shift)];
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int k = k0 + u * nthr;
        if (k >= g.fs) continue;
        cf X{0.f, 0.f};  // padding of the frame stride: keep it zero
        if (k < g.n_stft) X = czt_bin_vals(g, za[u], ca[u], zb[u], cb[u], l.lo2, l.hi2, k);
        if (MODE == kCztMag) a.mag[base + k] = sqrtf(fmaf(X.re, X.re, X.im * X.im));
        if (MODE == kCztSpec) a.spec[base + k] = X;
      }
    }
  }
}
