// rfx_fam_fwd_kernel.hip.h - the forward frame kernel of the row family, included by rfx_fam.hip (translation unit 0) twice:
//   RFX_FWDK_LOOP 0  fam_fwd_kernel<MODE, RA, RB, NR>       the row is reflect-padded (torch.stft center=True): the text this kernel always had
//   RFX_FWDK_LOOP 1  fam_fwd_loop_kernel<MODE, RA, RB, NR>  a loop forward call (include/rfx.h: rfx_stft_loop): the row of a.Lw = hop a.T samples is one
//                                                           period and is read modulo a.Lw (rfx_loop_core.h)
// One text, chosen at compile time: the two differ in how a sample position is formed and in nothing else.
//   RFX_FWDK_LOOP 2  fam_fwd_zero_kernel<MODE, RA, RB, NR>  the row of a.Lw samples is ZERO-EXTENDED (rfx_istft_core.h: zero_outside): the analysis of
//                                                           rfx_istft_backward, a.T frames whatever a.Lw is; outside [0, a.Lw) an exact 0.0f
#if RFX_FWDK_LOOP == 2
#define RFX_FWDK_LD(x, p, L) ((unsigned)(p) < (unsigned)(L) ? ld1(x, (unsigned)(p) * 4u, 0) : 0.f)
#elif RFX_FWDK_LOOP
#define RFX_FWDK_LD(x, p, L) ld1(x, (unsigned)loop_read_index(p, L) * 4u, 0)
#else
#define RFX_FWDK_LD(x, p, L) ld1(x, (unsigned)reflect_index(p, L) * 4u, 0)
#endif
// ---- forward: Spectrogram(power=None) [+ abs] of the family geometries (spectrogram_converter.py:47-59, :179-182).  Same P1 /
// A / B as above; the frame then changes places through LDS - once every row has been read the cube's memory becomes the
// bin-ordered frame, each bin written by its primary slot (the direct one where a bin has two) - and leaves in whole lines, in
// the plan's plain layout [B*T][fs] (what rfx_stft hands out and gen_mel_kernel reads).  MODE 0: |X|, MODE 1: X.
template <int MODE, int RA, int RB, int NR = 40>
#if RFX_FWDK_LOOP == 2
__global__ void __launch_bounds__(fam_threads(RA, RB, NR)) __attribute__((amdgpu_waves_per_eu(4))) fam_fwd_zero_kernel(FamFwdArgs a) {
#elif RFX_FWDK_LOOP
__global__ void __launch_bounds__(fam_threads(RA, RB, NR)) __attribute__((amdgpu_waves_per_eu(4))) fam_fwd_loop_kernel(FamFwdArgs a) {
#else
__global__ void __launch_bounds__(fam_threads(RA, RB, NR)) __attribute__((amdgpu_waves_per_eu(4))) fam_fwd_kernel(FamFwdArgs a) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* cube = reinterpret_cast<cf*>(smem);
  float* magl = reinterpret_cast<float*>(smem);
  constexpr int H = RA * RB;
  constexpr int NT = fam_threads(RA, RB, NR);
  constexpr int ROWS = NR / 2 + 1, WH = NR / 4;
  constexpr bool VEC = RFX_FAM_VEC && RB % 2 == 0;
  constexpr bool TWL = fam_twiddles_in_lds(RA, RB);
  const int tid = threadIdx.x;
  const int rs = a.g.rs;
  const bool act1 = tid < H;
  const int npr = act1 ? tid : H - 1;
  const int col = NR == 40 ? npr : (npr + a.g.left) % H;
  const bool actA = tid < ROWS * RB;
  const int tA = actA ? tid : ROWS * RB - 1;
  const int rowA = tA / RB, iA = tA - rowA * RB;
  const bool actB = tid < ROWS * RA;
  const int tB = actB ? tid : ROWS * RA - 1;
  const int rowB = tB / RA, pB = tB - rowB * RA;
  cf* const rowa = cube + rowA * rs + iA;
  cf* const rowb = cube + rowB * rs + pB * RB;
  const rsrc_t tw1 = make_rsrc(a.tw1, (size_t)ROWS * H * sizeof(cf));
  const rsrc_t win = make_rsrc(a.win, (size_t)WH * H * sizeof(float));
  const unsigned npr4 = (unsigned)npr * 4u, npr8 = (unsigned)npr * 8u;
  const long long nframes = (long long)a.B * a.T;
  const int fs = a.fs_plain, n_stft = a.g.n_stft;

  __shared__ __attribute__((aligned(16))) cf twa_lds[TWL ? RB * (RA - 1) : 1];
  if (TWL)
    for (int i = tid; i < RB * (RA - 1); i += NT) twa_lds[i] = a.twa[i];
  __syncthreads();  // as in fam_gl_kernel: the table must be complete before the first pass A
  FamTwA<RA, RB, TWL> wa;
  wa.src = make_rsrc(a.twa, (size_t)RB * (RA - 1) * sizeof(cf));
  wa.voff = (unsigned)iA * 8u;
  wa.tab = twa_lds + iA;
  cf w1[12];
  float wv[WH], u[WH];
  auto g1 = [&w1](int k) { return fam_g_pow(w1, k); };
  auto load_frame_inputs = [&](long long gf) {  // tables and the frame's samples (reflect-padded like torch.stft center=True)
#pragma unroll
    for (int k = 1; k <= (NR == 40 ? 11 : 10); ++k) {
      const v2f t = ld2(tw1, npr8, (unsigned)(k <= 10 ? k : 20) * (H * 8u));
      w1[k] = cf{t.x, t.y};
    }
    const int clip = (int)(gf / a.T), fr = (int)(gf - (long long)clip * a.T);
    const rsrc_t x = make_rsrc(a.wave + (size_t)clip * a.wave_stride, (size_t)a.Lw * sizeof(float));
#pragma unroll
    for (int j = 0; j < WH; ++j) {
      wv[j] = ld1(win, npr4, (unsigned)j * (H * 4u));
      u[j] = RFX_FWDK_LD(x, a.g.hop * fr + a.g.off + j * H + npr, a.Lw);
    }
  };
  if ((long long)blockIdx.x < nframes) load_frame_inputs(blockIdx.x);
  for (long long gf = blockIdx.x; gf < nframes; gf += gridDim.x) {
#pragma unroll
    for (int j = 0; j < WH; ++j) u[j] *= wv[j];
    if (act1) fam_p1_forward_store<NR>(u, g1, cube, col, rs);
    RFX_SCHED_FENCE();
    wa.template load<false, 0, true>();
    __syncthreads();
    RFX_SCHED_FENCE();
    if (actA)
      fam_pass_a_forward<RA, RB, true>(rowa, 0, [&wa](int p) { return wa.w[p]; }, [&wa](int batch) {
        wa.template load_batch<false, true>(batch);
        RFX_SCHED_FENCE();
      });
    RFX_SCHED_FENCE();
    __syncthreads();
    RFX_SCHED_FENCE();
    cf R[RB];
    fam_pass_b_forward<RA, RB, VEC>(rowb, 0, R);
    RFX_SCHED_FENCE();
    __syncthreads();  // every row has been read: the memory is now the bin-ordered frame
    if (actB) {
      // slot s of this thread holds k = k0 + 40 RA s.  k0 is frame-invariant, and the compiler would hoist all RB bin positions
      // and conjugate flags out of the frame loop - into scratch at the 128-register bound (68 spilled registers in round 3):
      // the empty asm makes k0 opaque per frame, two integer instructions per slot instead
      int k0 = rowB + NR * pB;
      asm volatile("" : "+v"(k0));
#pragma unroll
      for (int s = 0; s < RB; ++s) {
        const int k = k0 + NR * RA * s;
        const bool cj = k > a.g.n_fft / 2;
        const int bin = cj ? a.g.n_fft - k : k;
        // rows 0 and nrad / 2 hold their bins twice: the direct slot writes, the other one stores into a dump entry past the
        // frame (a select instead of a branch per slot: twenty s_and_saveexec / s_cbranch pairs per frame in round 3)
        const int at = fam_slot_is_primary(NR, rowB, cj) ? bin : n_stft + (tid & 31);
        if (MODE == 1) cube[at] = cf{R[s].re, cj ? -R[s].im : R[s].im};
        // v_sqrt_f32 (1 ulp) instead of the IEEE expansion: |X| carries ~1e-7 relative error from the transform anyway
        else magl[at] = __builtin_amdgcn_sqrtf(fmaf(R[s].re, R[s].re, R[s].im * R[s].im));
      }
    }
    RFX_SCHED_FENCE();
    __syncthreads();
    if (gf + gridDim.x < nframes) load_frame_inputs(gf + gridDim.x);  // in flight underneath the output loop
    if (MODE == 2) {
      // banded mel projection straight from the frame in LDS (the reference multiplies the dense filterbank,
      // spectrogram_converter.py:76-84, :185): a filter's weights come eight at a time from the L2-resident table, summed in
      // increasing bin order like gen_mel_kernel
      // (buffer-descriptor addressing: SRD + one 32-bit lane offset - the 64-bit per-lane pointers of the first version were what the
      // 48 kHz kernel spilled inside its frame loop)
      const rsrc_t bw = make_rsrc(a.band_wt, 0xFFFFFFFFull), blo = make_rsrc(a.band_lo, (size_t)a.Mpad * 4), bln = make_rsrc(a.band_len, (size_t)a.Mpad * 4);
      const rsrc_t mrow = make_rsrc(a.mel_tm + (size_t)gf * a.Mpad, (size_t)a.Mpad * 4);
      const unsigned mstride = (unsigned)a.Mpad * 4u;
      for (int m = tid; m < a.Mpad; m += NT) {
        float acc = 0.f;
#ifndef RFX_ABL_FAM_NOMEL  // (ablation: what the sum phase costs)
        if (m < a.M) {
          const int lo = (int)ld1u(blo, (unsigned)m * 4u, 0), n = (int)ld1u(bln, (unsigned)m * 4u, 0);
          for (int i = 0; i < n; i += 8) {
            float w[8], v[8];
            const unsigned woff = (unsigned)m * 4u + (unsigned)i * mstride;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              w[e] = ld1(bw, woff + (unsigned)e * mstride, 0);
              const int q = lo + i + e;
              v[e] = magl[q < n_stft ? q : n_stft - 1];  // (rows past the filter's end carry zero weights)
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(w[e], v[e], acc);
          }
        }
#else
        acc = magl[m];
#endif
        st1(acc, mrow, (unsigned)m * 4u, 0);
      }
    } else if (MODE == 1) {
      cf* __restrict__ out = a.spec + (size_t)gf * fs;
      for (int k = tid; k < fs; k += NT) out[k] = k < n_stft ? cube[k] : cf{0.f, 0.f};
    } else {
      float* __restrict__ out = a.mag + (size_t)gf * fs;
      for (int k = tid; k < fs; k += NT) out[k] = k < n_stft ? magl[k] : 0.f;  // (the padding of the frame stride stays zero)
    }
    RFX_SCHED_FENCE();
    __syncthreads();  // the next frame's P1 overwrites the frame
  }
}
#undef RFX_FWDK_LD
