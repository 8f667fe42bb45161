// rfx_gl_frame_kernel.hip.h - the per-frame Griffin-Lim kernel of the specialised engine, included by rfx_gl.hip twice:
//   RFX_GLK_LIST 0  gl_frame_kernel<MODE>       the grid-stride loop walks the call's B T frames (the text every call ran before held frames existed:
//                                                this instantiation compiles to the code it always compiled to)
//   RFX_GLK_LIST 1  gl_frame_list_kernel<MODE>  trip i of the loop takes frame list[i], list[B T] trips in all: launches 1 .. n_iter of a
//                                                held call (include/rfx.h: rfx_held_call_options; the list: rfx_guide_core.h)
//   RFX_GLK_LOOP 1  gl_frame_loop_kernel<MODE>  (with RFX_GLK_LIST 0) a loop call's launches 1 .. n_iter (include/rfx.h: rfx_loop_call_options): the
//                                                analysis input is read modulo the period g.L = hop T (rfx_loop_core.h) instead of reflected
// One text, chosen at compile time: no branch on the form inside any of the kernels.
#if RFX_GLK_LOOP
#define RFX_GLK_POS(p, L) loop_wrap(p, L)
#else
#define RFX_GLK_POS(p, L) reflect_index(p, L)
#endif
template <int MODE>
#if RFX_GLK_LOOP
__global__ void __launch_bounds__(kThreads, RFX_MIN_WAVES) gl_frame_loop_kernel(GlFrameArgs g) {
#elif RFX_GLK_LIST
__global__ void __launch_bounds__(kThreads, RFX_MIN_WAVES) gl_frame_list_kernel(GlFrameArgs g, const int* __restrict__ list) {
#else
__global__ void __launch_bounds__(kThreads, RFX_MIN_WAVES) gl_frame_kernel(GlFrameArgs g) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ThreadId t = thread_id();
  const FrameCtx f = frame_ctx(smem, t, g.tw1, g.tw2);
  const rsrc_t win = make_rsrc(g.win, kWin * 4);
  const unsigned npr4 = (unsigned)t.npr * 4u;
  const unsigned q16 = (unsigned)slot_qp(t.npr) * 16u;
  float wv[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) wv[j] = ld1(win, npr4, (unsigned)j * (kHop * 4u));
  Tw1 tw1;
  if (MODE != 0) load_tw1(tw1, f);
  __syncthreads();  // tw2 table in LDS

  const long long nframes = (long long)g.B * g.T;
#if RFX_GLK_LIST
  const long long ntrips = list[nframes];
  for (long long trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
    const long long gf = list[trip];
#else
  for (long long gf = blockIdx.x; gf < nframes; gf += gridDim.x) {
#endif
    const int clip = (int)(gf / g.T), fr = (int)(gf - (long long)clip * g.T);
    const size_t clip_slots = (size_t)g.T * kFrameStride;
    const rsrc_t Ssrc = make_rsrc(g.S + clip * clip_slots, clip_slots * sizeof(float));
    const unsigned foff = (unsigned)fr * (kFrameStride * 4u);
    cf R[21];
    MagRegs mag;
    if (MODE != 0) {
      const rsrc_t in = make_rsrc(g.audio_in + (size_t)clip * g.Lpad, (size_t)g.L * 4);
      const rsrc_t pv = make_rsrc(g.audio_prev + (size_t)clip * g.Lpad, (size_t)g.L * 4);
      const float ks = g.row_scale ? g.row_scale[2 * clip] : 1.f, eps2 = g.row_scale ? g.row_scale[2 * clip + 1] : 1e-32f;
      float u[10];
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        const unsigned p4 = (unsigned)RFX_GLK_POS((fr + j - kHalfHops) * kHop + t.npr, g.L) * 4u;
        float x = ld1(in, p4, 0);
        if (MODE == 2) x = fmaf(-g.mom, ld1(pv, p4, 0), x);
        u[j] = (x * ks) * wv[j];  // (the run kernel scales when the sample enters its sliding window: same two products)
      }
      frame_forward_tw(u, R, f, t, tw1, [&] { mag_issue(mag, Ssrc, foff, q16); });
#pragma unroll
      for (int kb = 0; kb < 21; ++kb) R[kb] = gl_project(R[kb], mag_at(mag, kb), eps2);
    } else {
      mag_issue(mag, Ssrc, foff, q16);
      if (g.angles0) {
        const rsrc_t init = make_rsrc(g.angles0 + clip * clip_slots, clip_slots * sizeof(cf));
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          const v4f v = ld4<RFX_STREAM_AUX>(init, q16, 2u * foff + (unsigned)i * (kQPad * 16u));
          R[2 * i] = cf{v.x, v.y};
          R[2 * i + 1] = cf{v.z, v.w};
        }
        const v2f w = ld2<RFX_STREAM_AUX>(init, q16 >> 1, 2u * foff + 20u * kQPad * 8u);
        R[20] = cf{w.x, w.y};
      } else {
        const unsigned rng_key = rand_frame_key(g.seed, g.frame_base + (unsigned long long)clip * g.T + fr);  // same stream as gl_iter_kernel
#pragma unroll
        for (int kb = 0; kb < 21; ++kb) {
          bool cj;
          const int bin = slot_bin(t.k1, t.idx, kb, &cj);
          const cf r = rand_unit_pair(rng_key, bin);
          R[kb] = cf{r.re, cj ? -r.im : r.im};
        }
      }
#pragma unroll
      for (int kb = 0; kb < 21; ++kb) {
        const float s = mag_at(mag, kb);
        R[kb] = cf{s * R[kb].re, s * R[kb].im};
      }
    }
    float y[10];
    frame_inverse_tw(R, y, f, t, tw1);
    if (t.active) {
      float* __restrict__ out = g.frames + (size_t)gf * kFramePitch + t.npr;
#pragma unroll
      for (int j = 0; j < 10; ++j) out[j * kHop] = y[j];  // un-windowed: the fold forms the run kernel's fma chains
    }
    __syncthreads();  // the next frame's first LDS stores overwrite rows other waves are still gathering in P1'
  }
}
#undef RFX_GLK_POS
