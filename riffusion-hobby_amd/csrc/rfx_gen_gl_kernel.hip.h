// rfx_gen_gl_kernel.hip.h - the Griffin-Lim frame kernel of the generic engine, included by rfx_generic.hip twice:
//   RFX_GLK_LIST 0  gen_gl_kernel<MODE, MAXR>       the grid-stride loop walks the call's B T frames (this instantiation compiles to the code it
//                                                    always compiled to)
//   RFX_GLK_LIST 1  gen_gl_list_kernel<MODE, MAXR>  trip i of the loop takes frame list[i], list[B T] trips in all: launches 1 .. n_iter of a
//                                                    held call (include/rfx.h: rfx_held_call_options; the list: rfx_guide_core.h)
//   RFX_GLK_LOOP 1  gen_gl_loop_kernel<MODE, MAXR>  (with RFX_GLK_LIST 0) a loop call's launches 1 .. n_iter (include/rfx.h: rfx_loop_call_options):
//                                                    the analysis input is read modulo the period a.L = hop T (rfx_loop_core.h) instead of reflected
// One text, chosen at compile time: no branch on the form inside any of the kernels.
#if RFX_GLK_LOOP
#define RFX_GLK_POS(p, L) loop_wrap(p, L)
#else
#define RFX_GLK_POS(p, L) reflect_index(p, L)
#endif
template <int MODE, int MAXR>
__global__ void __launch_bounds__(kGenThreads) __attribute__((amdgpu_waves_per_eu(MAXR <= 7 ? 4 : 2)))
#if RFX_GLK_LOOP
gen_gl_loop_kernel(GenGlArgs a) {
#elif RFX_GLK_LIST
gen_gl_list_kernel(GenGlArgs a, const int* __restrict__ list) {
#else
gen_gl_kernel(GenGlArgs a) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GenGeom& g = a.g;
  const GenLds l = gen_lds(smem, g, a.tb);
  const long long nframes = (long long)a.B * a.T;
  const int half = g.n_fft / 2;
  const float scale = 1.0f / (float)g.nc;  // even: z = IFFT_nc(Z) ; odd: x = Re IFFT_n(Z)
  const int npairs = gen_pair_count(g);
#ifdef RFX_GEN_TIMING
  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0}, tlast = wall_clock64();
  int nfr = 0;
#define GSTAMP(i) do { unsigned long long now_ = wall_clock64(); tacc[i] += now_ - tlast; tlast = now_; } while (0)
#else
#define GSTAMP(i) ((void)0)
#endif
#if RFX_GLK_LIST
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
    GSTAMP(0);
    if (MODE == 0) {
      auto X = [&](int k) {
        cf ang;
        if (a.angles0) ang = a.angles0[base + k];
        else ang = rand_unit_pair(rand_frame_key(a.seed, a.frame_base + (unsigned long long)fr), k);
        const float s = S[k];
        return cf{s * ang.re, s * ang.im};
      };
      for (int k = threadIdx.x; k < g.nc; k += blockDim.x) l.a[a.tb.rev[k]] = gen_split_inverse(g, X, l.lo2, l.hi2, k);
    } else {
      // windowed, zero-padded frame of x_k - m x_{k-1} (reflect-padded like torch.stft center=True), packed two reals per
      // complex when n_fft is even.  Only the elements the window covers need loads ([n_lo, n_hi): a quarter of the frame at
      // the reference's 100 / 400 ms); the rest is zeroed.  Loads are batched - all of a batch's global loads, then its LDS
      // stores - so that a thread waits for HBM / L2 once per batch, not once per element.
      const float* __restrict__ xc = a.x_cur + (size_t)clip * a.audio_stride;
      const float* __restrict__ xp = a.x_prev + (size_t)clip * a.audio_stride;
      const int nthr = (int)blockDim.x;
      const int per = g.even ? 2 : 1;
      const int n_lo = g.left / per, n_hi = (g.left + g.win + per - 1) / per;
      for (int n = threadIdx.x; n < g.nc; n += nthr)
        if (n < n_lo || n >= n_hi) l.a[gen_ipad(n, g.pad_shift)] = cf{0.f, 0.f};
      constexpr int UL = 5;
      for (int n0 = n_lo + (int)threadIdx.x; n0 < n_hi; n0 += UL * nthr) {
        float xs[UL][2], ps[UL][2], ws[UL][2];
#pragma unroll
        for (int u = 0; u < UL; ++u)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            xs[u][e] = ps[u][e] = ws[u][e] = 0.f;
            const int n = n0 + u * nthr;
            if (e < per && n < n_hi) {
              const int i = per * n + e;  // position inside the padded frame
              const int j = i - g.left;   // position inside the window
              if (j >= 0 && j < g.win) {
                const int p = RFX_GLK_POS(g.hop * t + i - half, a.L);
                xs[u][e] = xc[p];
                if (MODE == 2) ps[u][e] = xp[p];
                ws[u][e] = a.tb.win[j];
              }
            }
          }
#pragma unroll
        for (int u = 0; u < UL; ++u) {
          const int n = n0 + u * nthr;
          if (n < n_hi)
            l.a[gen_ipad(n, g.pad_shift)] = cf{fmaf(-a.mom, ps[u][0], xs[u][0]) * ws[u][0], fmaf(-a.mom, ps[u][1], xs[u][1]) * ws[u][1]};
        }
      }
      __syncthreads();
      GSTAMP(1);
      gen_fft<false, MAXR>(g, l, a.tb.tw);  // ends with a barrier; spectrum digit-reversed in l.a
      GSTAMP(2);
      {
        // split / projection / merge, pairwise in place (gen_pair_compute).  Batches of UP pairs per thread: first every
        // global load of the batch (LDS positions from the digit-reversal table, |S| from HBM), then the LDS reads that depend
        // on them, the arithmetic, the stores - one global round trip and one LDS round trip per batch.
        constexpr int UP = 5;
        const int kc_of0 = g.even ? g.nc : 0;
        for (int k0 = threadIdx.x; k0 < npairs; k0 += UP * nthr) {
          GenPair pr[UP];
          int pk[UP], pc[UP];
#pragma unroll
          for (int u = 0; u < UP; ++u) {
            const int k = k0 + u * nthr;
            const bool ok = k < npairs;
            const int kk = ok ? k : 0;
            const int kc = g.even ? g.nc - kk : (kk == 0 ? 0 : g.n_fft - kk);  // partner ELEMENT (odd n_fft: the mirror element)
            pr[u].k = kk;
            pk[u] = a.tb.rev[kk];
            pc[u] = a.tb.rev[kc == kc_of0 && g.even ? 0 : kc];
            pr[u].sk = S[kk];
            pr[u].sc = g.even ? S[kc] : 0.f;  // even, k == 0: bin nc
          }
#pragma unroll
          for (int u = 0; u < UP; ++u) {
            pr[u].zk = l.a[pk[u]];
            pr[u].zc = g.even ? l.a[pc[u]] : pr[u].zk;
          }
#pragma unroll
          for (int u = 0; u < UP; ++u) gen_pair_compute(pr[u], g, l.lo2, l.hi2, eps2);
#pragma unroll
          for (int u = 0; u < UP; ++u) {
            const int k = k0 + u * nthr;
            if (k < npairs) {
              l.a[pk[u]] = pr[u].zk;
              const bool partner = g.even ? (k != 0 && k != g.nc - k) : k != 0;
              if (partner) l.a[pc[u]] = pr[u].zc;
            }
          }
        }
      }
    }
#ifdef RFX_GEN_TIMING
    __syncthreads();
#endif
    GSTAMP(3);
    const cf* z = gen_fft<true, MAXR>(g, l, a.tb.tw);  // starts with a barrier
    GSTAMP(4);
    float* __restrict__ out = a.frames + (size_t)fr * g.fpitch + g.fshift;
    {
      constexpr int UO = 5;  // window samples fetched per batch before the stores
      const int nthr = (int)blockDim.x;
      for (int j0 = threadIdx.x; j0 < g.win; j0 += UO * nthr) {
        float wv[UO], zv[UO];
#pragma unroll
        for (int u = 0; u < UO; ++u) {
          const int j = j0 + u * nthr;
          const int jj = j < g.win ? j : 0;
          const int i = jj + g.left;
          wv[u] = a.tb.win[jj];
          const cf zz = z[gen_ipad(g.even ? i >> 1 : i, g.pad_shift)];
          zv[u] = (g.even && (i & 1)) ? zz.im : zz.re;
        }
#pragma unroll
        for (int u = 0; u < UO; ++u) {
          const int j = j0 + u * nthr;
          if (j < g.win) out[j] = zv[u] * scale * wv[u];
        }
      }
    }
    GSTAMP(5);
#ifdef RFX_GEN_TIMING
    ++nfr;
#endif
  }
#ifdef RFX_GEN_TIMING
  if (MODE == 2 && blockIdx.x == 7 && threadIdx.x == 0)
    printf("gen_gl timing (100 MHz ticks per frame, %d frames): barrier-wait %.1f load %.1f fwd %.1f pair %.1f inv %.1f out %.1f\n", nfr,
           (double)tacc[0] / nfr, (double)tacc[1] / nfr, (double)tacc[2] / nfr, (double)tacc[3] / nfr, (double)tacc[4] / nfr, (double)tacc[5] / nfr);
#endif
}
#undef RFX_GLK_POS
