// rfx_gen_stft_kernel.hip.h - the forward frame kernel of the generic engine, included by rfx_generic.hip twice:
//   RFX_FWDK_LOOP 0  gen_stft_kernel<MODE, MAXR>       the row is reflect-padded (torch.stft center=True): the text this kernel always had
//   RFX_FWDK_LOOP 1  gen_stft_loop_kernel<MODE, MAXR>  a loop forward call (include/rfx.h: rfx_stft_loop): the row of a.Lw = hop a.T samples is one period
//                                                      and is read modulo a.Lw (rfx_loop_core.h)
// One text, chosen at compile time: the two differ in how a sample position is formed and in nothing else.
//   RFX_FWDK_LOOP 2  gen_stft_zero_kernel<MODE, MAXR>  the row of a.Lw samples is ZERO-EXTENDED (rfx_istft_core.h: zero_outside): the analysis of
//                                                      rfx_istft_backward, a.T frames whatever a.Lw is; outside [0, a.Lw) an exact 0.0f
#if RFX_FWDK_LOOP == 2
#define RFX_FWDK_READ(x, p, L) zero_outside_read(x, p, L)
#elif RFX_FWDK_LOOP
#define RFX_FWDK_READ(x, p, L) x[loop_read_index(p, L)]
#else
#define RFX_FWDK_READ(x, p, L) x[reflect_index(p, L)]
#endif
// (Prefetching the next frame's samples and the epilogue's |S| / tprev into register slots across the passes was tried:
// 229 -> 245-257 ms per 64 tiles at 48 kHz - the slot arrays spill.  The simple loops below stay.)
// (four waves per SIMD = 128 VGPRs, so that two 512-thread workgroups share a CU: without the bound the compiler took 169
// registers for the batched butterflies and the second workgroup no longer fitted - 121 -> 182 ms per 64 tiles at 48 kHz;
// the O(R^2) radix-11 / 13 class keeps its larger budget)
template <int MODE, int MAXR>
__global__ void __launch_bounds__(kGenThreads) __attribute__((amdgpu_waves_per_eu(MAXR <= 7 ? 4 : 2)))
#if RFX_FWDK_LOOP == 2
gen_stft_zero_kernel(GenStftArgs a) {
#elif RFX_FWDK_LOOP
gen_stft_loop_kernel(GenStftArgs a) {
#else
gen_stft_kernel(GenStftArgs a) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GenGeom& g = a.g;
  const GenLds l = gen_lds(smem, g, a.tb);
  const long long nframes = (long long)a.B * a.T;
  const int half = g.n_fft / 2;
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    const int clip = (int)(fr / a.T), t = (int)(fr - (long long)clip * a.T);
    const float* __restrict__ x = a.wave + (size_t)clip * a.wave_stride;
    __syncthreads();  // previous frame's epilogue is done with the buffers
    // windowed, zero-padded frame, packed two reals per complex when n_fft is even
    for (int n = threadIdx.x; n < g.nc; n += blockDim.x) {
      float v[2] = {0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (!g.even && e == 1) break;
        const int i = g.even ? 2 * n + e : n;  // position inside the padded frame
        const int j = i - g.left;              // position inside the window
        if (j >= 0 && j < g.win) v[e] = RFX_FWDK_READ(x, g.hop * t + i - half, a.Lw) * a.tb.win[j];
      }
      l.a[RFX_GEN_INPLACE ? gen_ipad(n, g.pad_shift) : gen_pad(n)] = cf{v[0], v[1]};
    }
    const cf* Z = gen_fft<false, MAXR>(g, l, a.tb.tw);
    const size_t base = (size_t)fr * g.fs;
    for (int k = threadIdx.x; k < g.fs; k += blockDim.x) {
      if (k >= g.n_stft) {  // padding of the frame stride: keep it zero
        if (MODE == kGenMag) a.mag[base + k] = 0.f;
        if (MODE == kGenSpec) a.spec[base + k] = cf{0.f, 0.f};
        continue;
      }
      const cf X = gen_split_forward(g, Z, l.lo2, l.hi2, k, RFX_GEN_INPLACE ? a.tb.rev : nullptr);
      if (MODE == kGenMag) a.mag[base + k] = sqrtf(fmaf(X.re, X.re, X.im * X.im));
      if (MODE == kGenSpec) a.spec[base + k] = X;
    }
  }
}
#undef RFX_FWDK_READ
