// rfx_fam_gl_kernel.hip.h - the Griffin-Lim frame kernel of the row family, included by rfx_fam.hip (in both of its translation units) twice:
//   RFX_GLK_LIST 0  fam_gl_kernel<MODE, RA, RB, NR, TU>       the grid-stride loop walks the call's B T frames (this instantiation compiles
//                                                              to the code it always compiled to)
//   RFX_GLK_LIST 1  fam_gl_list_kernel<MODE, RA, RB, NR, TU>  trip i of the loop takes frame list[i], list[B T] trips in all, and the next
//                                                              frame's prefetch follows the list: launches 1 .. n_iter of a held call
//                                                              (include/rfx.h: rfx_held_call_options; the list: rfx_guide_core.h)
//   RFX_GLK_LOOP 1  fam_gl_loop_kernel<MODE, RA, RB, NR, TU>  (with RFX_GLK_LIST 0) a loop call's launches 1 .. n_iter (include/rfx.h:
//                                                              rfx_loop_call_options): the analysis input is read modulo the period
//                                                              a.L = hop T (rfx_loop_core.h) instead of reflected
// One text, chosen at compile time: no branch on the form inside any of the kernels.
#if RFX_GLK_LOOP
#define RFX_GLK_POS(p, L) loop_wrap(p, L)
#else
#define RFX_GLK_POS(p, L) reflect_index(p, L)
#endif
template <int MODE, int RA, int RB, int NR = 40, int TU = RFX_FAM_TU>
#if RFX_GLK_LOOP
__global__ void __launch_bounds__(fam_threads(RA, RB, NR)) __attribute__((amdgpu_waves_per_eu(4))) fam_gl_loop_kernel(FamGlArgs a) {
#elif RFX_GLK_LIST
__global__ void __launch_bounds__(fam_threads(RA, RB, NR)) __attribute__((amdgpu_waves_per_eu(4))) fam_gl_list_kernel(FamGlArgs a, const int* __restrict__ list) {
#else
__global__ void __launch_bounds__(fam_threads(RA, RB, NR)) __attribute__((amdgpu_waves_per_eu(4))) fam_gl_kernel(FamGlArgs a) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* cube = reinterpret_cast<cf*>(smem);
  constexpr int H = RA * RB;
  constexpr int NT = fam_threads(RA, RB, NR);
  constexpr int ROWS = NR / 2 + 1, WH = NR / 4;  // rows of the cube, window blocks of h samples (rfx_fam_core.h)
  const int tid = threadIdx.x;
  const int rs = a.g.rs;
  const bool act1 = tid < H;
  const int npr = act1 ? tid : H - 1;  // idle lanes shadow the last active one (loads only, never stores)
  const int col = NR == 40 ? npr : (npr + a.g.left) % H;  // cube column of this thread's window samples
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
  const unsigned npr4 = (unsigned)npr * 4u, npr8 = (unsigned)npr * 8u, tB4 = (unsigned)tB * 4u;
  const float oscale = 2.0f / (float)a.g.n_fft;
  const long long nframes = (long long)a.B * a.T;

  constexpr bool VEC = RFX_FAM_VEC && RB % 2 == 0;  // the host picks an even row stride then (fam_row_stride_even)
  constexpr bool TWL = fam_twiddles_in_lds(RA, RB);
  __shared__ __attribute__((aligned(16))) cf twa_lds[TWL ? RB * (RA - 1) : 1];
  if (TWL)
    for (int i = tid; i < RB * (RA - 1); i += NT) twa_lds[i] = a.twa[i];
  __syncthreads();  // the first pass-A read of the frame loop may precede the loop's first barrier, and reads other waves' entries
  FamTwA<RA, RB, TWL> wa;
  wa.src = make_rsrc(a.twa, (size_t)RB * (RA - 1) * sizeof(cf));
  wa.voff = (unsigned)iA * 8u;
  wa.tab = twa_lds + iA;
  // g(n')^k1 for k1 = 1..10 and 20 only (fam_g_pow)
  cf w1[12];
  float wv[WH], u[WH];
  auto load_tables = [&] {
#if defined(RFX_FAM_ABL) && RFX_FAM_ABL >= 2  // timing ablation (wrong results): no g^k1 / Hann fetches either
#pragma unroll
    for (int k = 1; k <= (NR == 40 ? 11 : 10); ++k) w1[k] = cf{1.f, (float)k};
#pragma unroll
    for (int j = 0; j < WH; ++j) wv[j] = (float)j;
    return;
#endif
#pragma unroll
    for (int k = 1; k <= (NR == 40 ? 11 : 10); ++k) {
      const v2f t = ld2(tw1, npr8, (unsigned)(k <= 10 ? k : 20) * (H * 8u));
      w1[k] = cf{t.x, t.y};
    }
#pragma unroll
    for (int j = 0; j < WH; ++j) wv[j] = ld1(win, npr4, (unsigned)j * (H * 4u));
  };
  auto g1 = [&w1](int k) { return fam_g_pow(w1, k); };
  // frame fr is centred on sample hop * fr of the reflect-padded estimate (torch.stft center=True): the window covers
  // positions hop * fr + off .. hop * fr + off + win - 1, off = left - n_fft / 2 (-5 h in the 40 h family)
  // (x_cur holds d = x_k - m x_{k-1} since round 4: the fold of the previous iteration forms it, one load per window sample
  // here instead of two and ten registers less across P1')
  auto load_samples = [&](long long gf) {
    const int clip = (int)(gf / a.T), fr = (int)(gf - (long long)clip * a.T);
    const rsrc_t xc = make_rsrc(a.x_cur + (size_t)clip * a.audio_stride, (size_t)a.L * sizeof(float));
#pragma unroll
    for (int j = 0; j < WH; ++j) u[j] = ld1(xc, (unsigned)RFX_GLK_POS(a.g.hop * fr + a.g.off + j * H + npr, a.L) * 4u, 0);
  };
  auto window_samples = [&] {
#pragma unroll
    for (int j = 0; j < WH; ++j) u[j] *= wv[j];
  };
#if RFX_GLK_LIST
  const long long ntrips = list[nframes];
  if (MODE != 0 && (long long)blockIdx.x < ntrips) {
    load_tables();
    load_samples(list[blockIdx.x]);
    window_samples();
  }
#else
  if (MODE != 0 && (long long)blockIdx.x < nframes) {
    load_tables();
    load_samples(blockIdx.x);
    window_samples();
  }
#endif

#ifdef RFX_FAM_TIMING
  unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = wall_clock64();
  int nfr = 0;
#define FSTAMP(i) do { unsigned long long now_ = wall_clock64(); tacc[i] += now_ - tlast; tlast = now_; } while (0)
#else
#define FSTAMP(i) ((void)0)
#endif
#if RFX_GLK_LIST
  for (long long trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
    const long long gf = list[trip];
#else
  for (long long gf = blockIdx.x; gf < nframes; gf += gridDim.x) {
#endif
    const rsrc_t S = make_rsrc(a.S + (size_t)gf * a.g.fsf, (size_t)a.g.fsf * sizeof(float));
    cf R[RB];
    FSTAMP(0);
    if (MODE != 0) {
      if (act1) fam_p1_forward_store<NR>(u, g1, cube, col, rs);
      RFX_SCHED_FENCE();
      wa.template load<false, 0, RFX_FAM_GL_STREAM_FWD>();
#if RFX_FAM_TW_EARLY
      for (int b = 1; b < fam_tw_batches(RA, false, RFX_FAM_GL_STREAM_FWD); ++b) wa.template load_batch<false, RFX_FAM_GL_STREAM_FWD>(b);
#endif
      FSTAMP(1);
      __syncthreads();
      FSTAMP(2);
      RFX_SCHED_FENCE();
      if (actA)
        fam_pass_a_forward<RA, RB, RFX_FAM_GL_STREAM_FWD>(rowa, 0, [&wa](int p) { return wa.w[p]; }, [&wa](int batch) {
          if (!RFX_FAM_TW_EARLY) wa.template load_batch<false, RFX_FAM_GL_STREAM_FWD>(batch);
          RFX_SCHED_FENCE();
        });
      RFX_SCHED_FENCE();
      float Sv[RB];
#pragma unroll
      for (int s = 0; s < RB; ++s) Sv[s] = ld1<RFX_FAM_STREAM_AUX>(S, tB4, (unsigned)s * (NT * 4u));
      FSTAMP(3);
      __syncthreads();
      FSTAMP(2);
      RFX_SCHED_FENCE();
#if RFX_FAM_PRIO
      __builtin_amdgcn_s_setprio(2);
#endif
      fam_pass_b_forward<RA, RB, VEC>(rowb, 0, R);
      const float eps2 = a.row_scale ? a.row_scale[2 * (gf / a.T) + 1] : 1e-32f;  // (the fold has applied row_scale[2 row] to x_cur)
#pragma unroll
      for (int s = 0; s < RB; ++s) R[s] = gl_project(R[s], Sv[s], eps2);
    } else {
      const unsigned rng_key = rand_frame_key(a.seed, a.frame_base + (unsigned long long)gf);  // the generic engine's stream
#pragma unroll
      for (int s = 0; s < RB; ++s) {
        bool cj;
        const int bin = fam_slot_bin(a.g, rowB, pB, s, &cj);
        cf ang;
        if (a.angles0) ang = a.angles0[(size_t)gf * a.fs_plain + bin];
        else ang = rand_unit_pair(rng_key, bin);
        const float sv = ld1<RFX_FAM_STREAM_AUX>(S, tB4, (unsigned)s * (NT * 4u));
        R[s] = cf{sv * ang.re, cj ? -(sv * ang.im) : sv * ang.im};
      }
    }
    if (actB) fam_pass_b_inverse<RA, RB, VEC>(rowb, 0, R);
#if RFX_FAM_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    RFX_SCHED_FENCE();
    wa.template load<true, 0, RFX_FAM_GL_STREAM_INV>();
    FSTAMP(4);
    __syncthreads();
    FSTAMP(2);
    RFX_SCHED_FENCE();
    if (actA)
      fam_pass_a_inverse<RA, RB, RFX_FAM_GL_STREAM_INV>(rowa, 0, [&wa](int p) { return wa.w[p]; }, [&wa](int batch) {
        wa.template load_batch<true, RFX_FAM_GL_STREAM_INV>(batch);
        RFX_SCHED_FENCE();
      });
    RFX_SCHED_FENCE();
    load_tables();
    FSTAMP(5);
    __syncthreads();
    FSTAMP(2);
    RFX_SCHED_FENCE();
    // the next frame's samples are requested here and arrive underneath P1' (requested before the barrier, together with the
    // tables, the 61 loads of this phase queue up behind each other: 4 us of issue time per frame, measured)
#if RFX_GLK_LIST
    const bool more = MODE != 0 && trip + gridDim.x < ntrips;
    if (more) load_samples(list[trip + gridDim.x]);  // (the prefetch follows the list)
#else
    const bool more = MODE != 0 && gf + gridDim.x < nframes;
    if (more) load_samples(gf + gridDim.x);
#endif
    RFX_SCHED_FENCE();
    {
      float y[WH];
      fam_p1_load_inverse<NR>(cube, g1, y, col, rs);
      if (act1) {
        const rsrc_t out = make_rsrc(a.frames + (size_t)gf * a.fpitch + a.fshift, (size_t)WH * H * sizeof(float));
#pragma unroll
        for (int j = 0; j < WH; ++j) st1<RFX_FAM_STORE_AUX>(y[j] * (wv[j] * oscale), out, npr4, (unsigned)j * (H * 4u));
      }
    }
    RFX_SCHED_FENCE();
    if (more) window_samples();
    RFX_SCHED_FENCE();
    FSTAMP(6);
    // no barrier here when a P1 follows: its stores go to column n' of the rows - exactly the elements this thread has just
    // read in P1' - and nobody else touches a column between these two phases (a wave's LDS operations execute in order)
    if (MODE == 0) __syncthreads();  // (mode 0 goes straight to the next frame's B', which writes whole rows)
#ifdef RFX_FAM_TIMING
    ++nfr;
#endif
  }
#ifdef RFX_FAM_TIMING
  if (MODE == 1 && (blockIdx.x == 7 || blockIdx.x == 300) && (threadIdx.x == 0 || threadIdx.x == 256 || threadIdx.x == 448))
    printf("fam_gl timing, block %d of %d, thread %d (100 MHz ticks per frame, %d frames): P1 %.1f | barriers %.1f | A %.1f | B+proj+B' %.1f | A' %.1f | P1' %.1f | loop top %.1f\n",
           (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, nfr, (double)tacc[1] / nfr, (double)tacc[2] / nfr, (double)tacc[3] / nfr, (double)tacc[4] / nfr, (double)tacc[5] / nfr,
           (double)tacc[6] / nfr, (double)tacc[0] / nfr);
#endif
}
#undef RFX_GLK_POS
