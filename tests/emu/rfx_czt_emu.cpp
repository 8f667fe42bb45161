// Host-side emulator of the CHIRP-Z frame transform (csrc/rfx_czt_core.h).  TEST INFRASTRUCTURE ONLY, built with g++ by
// tests/test_czt_core.py: it runs the same per-thread functions the gfx950 kernels of rfx_czt.hip inline - the chirp products, the
// in-place passes of rfx_gen_core.h at the convolution length, the pointwise H, the real split and the pairwise projection - looping
// over the logical threads of a workgroup phase by phase (a loop boundary stands where the kernel has a barrier), with the tables
// czt_tables builds for the plan.
#include <cmath>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_czt_core.h"

using namespace rfx;

namespace {
struct Tables {
  std::vector<cf> lo, hi, lo2, hi2, tw, c, h;
};
// the geometry as plan_geometry fills it for the chirp-z engine (ps: LDS padding shift, the plan's choice left to the caller)
bool make_geom(int n_fft, int ps, GenGeom& g, Tables& t) {
  g = GenGeom{};
  g.n_fft = n_fft; g.win = n_fft; g.hop = 1; g.n_stft = n_fft / 2 + 1;
  g.even = n_fft % 2 == 0;
  g.nc = g.even ? n_fft / 2 : n_fft;
  g.left = 0;
  g.fs = (g.n_stft + 63) / 64 * 64;
  g.pad_shift = ps;
  if (!czt_fits(g.nc)) return false;
  g.np = czt_pass_len(g.nc, g.radix, &g.nstages);
  g.nhi = czt_nhi(g.np);
  g.nhi2 = czt_nhi2(g.nc);
  const double PI2 = 6.283185307179586476925286766559;
  auto root = [&](long long num, long long den) {
    const double a = -PI2 * (double)(num % den) / (double)den;
    return cf{(float)cos(a), (float)sin(a)};
  };
  t.lo.resize(kGenTwLo); t.lo2.resize(kGenTwLo); t.hi.resize(g.nhi); t.hi2.resize(g.nhi2);
  for (int i = 0; i < kGenTwLo; ++i) { t.lo[i] = root(i, g.np); t.lo2[i] = root(i, g.n_fft); }
  for (int i = 0; i < g.nhi; ++i) t.hi[i] = root((long long)i * kGenTwLo, g.np);
  for (int i = 0; i < g.nhi2; ++i) t.hi2[i] = root((long long)i * kGenTwLo, g.n_fft);
  // exact per-pass twiddles at the convolution length, as plan creation builds them (double precision, rounded once)
  const GenGeom pg = czt_pass_geom(g);
  t.tw.assign(gen_tw_table_elems(pg) + 1, cf{0.f, 0.f});
  int L = g.np;
  for (int s = 0; s < g.nstages; ++s) {
    const int R = g.radix[s], m = L / R, off = gen_tw_table_offset(pg, s);
    for (int i = 0; i < m; ++i)
      for (int p = 1; p < R; ++p) {
        const double a = -PI2 * (double)(((long long)i * p) % L) / (double)L;
        t.tw[off + i * (R - 1) + p - 1] = cf{(float)cos(a), (float)sin(a)};
      }
    L = m;
  }
  CztTables ct = czt_tables(g);
  t.c = ct.c;
  t.h = ct.h;
  return true;
}
template <bool INV>
void run_passes(const GenGeom& g, const Tables& t, cf* buf, int nthr) {
  const GenGeom pg = czt_pass_geom(g);
  int Ls[kGenMaxStages];
  int L = g.np;
  for (int s = 0; s < g.nstages; ++s) { Ls[s] = L; L /= g.radix[s]; }
  for (int i = 0; i < g.nstages; ++i) {
    const int s = INV ? g.nstages - 1 - i : i;
    for (int tid = 0; tid < nthr; ++tid)
      gen_ip_stage<INV>(buf, g.np, Ls[s], g.radix[s], t.lo.data(), t.hi.data(), tid, nthr, g.pad_shift, t.tw.data() + gen_tw_table_offset(pg, s));
  }
}
// steps 2 - 4
void run_conv(const GenGeom& g, const Tables& t, cf* buf, int nthr) {
  run_passes<false>(g, t, buf, nthr);
  for (int tid = 0; tid < nthr; ++tid) czt_mul_h(buf, t.h.data(), g, tid, nthr);
  run_passes<true>(g, t, buf, nthr);
}
void load_frame(const GenGeom& g, const Tables& t, const float* frame, cf* buf, int nthr) {
  for (int tid = 0; tid < nthr; ++tid) {
    for (int n = tid; n < g.nc; n += nthr)
      buf[gen_ipad(n, g.pad_shift)] = czt_chirp(g.even ? cf{frame[2 * n], frame[2 * n + 1]} : cf{frame[n], 0.f}, t.c[n]);
    czt_zero_tail(buf, g, tid, nthr);
  }
}
void store_frame(const GenGeom& g, const Tables& t, const cf* buf, float* out) {
  const float scale = 1.0f / (float)g.nc;
  for (int i = 0; i < g.n_fft; ++i) {
    const int e = g.even ? i >> 1 : i;
    out[i] = czt_out_sample(g, buf[gen_ipad(e, g.pad_shift)], t.c[e], i) * scale;
  }
}
}  // namespace

extern "C" {

// number of passes at the convolution length (0: the length does not fit); *np_out = that length, radices to radix_out[16]
int emu_czt_plan(int n_fft, int* np_out, int* radix_out) {
  GenGeom g; Tables t;
  if (!make_geom(n_fft, 0, g, t)) return 0;
  *np_out = g.np;
  for (int i = 0; i < g.nstages; ++i) radix_out[i] = g.radix[i];
  return g.nstages;
}
int emu_czt_max_nc(void) { return czt_max_nc(); }

// the tables in natural order: c [nc] and H [np] (interleaved re, im)
int emu_czt_tables(int n_fft, int ps, float* c_out, float* h_out) {
  GenGeom g; Tables t;
  if (!make_geom(n_fft, ps, g, t)) return -1;
  const GenGeom pg = czt_pass_geom(g);
  for (int n = 0; n < g.nc; ++n) { c_out[2 * n] = t.c[n].re; c_out[2 * n + 1] = t.c[n].im; }
  for (int k = 0; k < g.np; ++k) {
    const cf v = t.h[gen_ipad(gen_digit_reverse(pg, k), ps)];
    h_out[2 * k] = v.re; h_out[2 * k + 1] = v.im;
  }
  return 0;
}

// frame: n_fft reals -> n_stft complex bins (interleaved re, im)
int emu_czt_rfft(int n_fft, const float* frame, float* out, int nthr, int ps) {
  GenGeom g; Tables t;
  if (!make_geom(n_fft, ps, g, t)) return -1;
  std::vector<cf> a(gen_ibuf_elems(g.np, ps));
  load_frame(g, t, frame, a.data(), nthr);
  run_conv(g, t, a.data(), nthr);
  for (int k = 0; k < g.n_stft; ++k) {
    const int ea = czt_bin_elem_a(g, k), eb = czt_bin_elem_b(g, k);
    const cf X = czt_bin_vals(g, a[gen_ipad(ea, ps)], t.c[ea], a[gen_ipad(eb, ps)], t.c[eb], t.lo2.data(), t.hi2.data(), k);
    out[2 * k] = X.re; out[2 * k + 1] = X.im;
  }
  return 0;
}

// n_stft complex bins -> n_fft reals, scaled like numpy / torch irfft (1/n_fft)
int emu_czt_irfft(int n_fft, const float* spec, float* out, int nthr, int ps) {
  GenGeom g; Tables t;
  if (!make_geom(n_fft, ps, g, t)) return -1;
  std::vector<cf> a(gen_ibuf_elems(g.np, ps));
  auto X = [&](int k) { return cf{spec[2 * k], spec[2 * k + 1]}; };
  for (int tid = 0; tid < nthr; ++tid) {
    for (int k = tid; k < g.nc; k += nthr)
      a[gen_ipad(k, ps)] = czt_chirp_conj(gen_split_inverse(g, X, t.lo2.data(), t.hi2.data(), k), t.c[k]);
    czt_zero_tail(a.data(), g, tid, nthr);
  }
  run_conv(g, t, a.data(), nthr);
  store_frame(g, t, a.data(), out);
  return 0;
}

// One frame of the fused Griffin-Lim kernel (czt_gl_kernel, modes 1 / 2): chirp, convolution, the pairwise in-place
// [chirp, projection, conj chirp], convolution, conj chirp.  frame: n_fft reals; S: n_stft magnitudes; out: n_fft reals =
// irfft(S * X / (|X| + 1e-16)), X = rfft(frame)
int emu_czt_gl_frame(int n_fft, const float* frame, const float* S, float* out, int nthr, int ps) {
  GenGeom g; Tables t;
  if (!make_geom(n_fft, ps, g, t)) return -1;
  std::vector<cf> a(gen_ibuf_elems(g.np, ps));
  load_frame(g, t, frame, a.data(), nthr);
  run_conv(g, t, a.data(), nthr);
  const int npairs = gen_pair_count(g);
  for (int tid = 0; tid < nthr; ++tid) {
    for (int k = tid; k < npairs; k += nthr) {
      const int kc = czt_pair_partner(g, k);
      GenPair p;
      p.k = k;
      p.zk = a[gen_ipad(k, ps)];
      p.zc = a[gen_ipad(kc, ps)];
      p.sk = S[k];
      p.sc = g.even ? S[g.nc - k] : 0.f;
      czt_pair_compute(p, g, t.c[k], t.c[kc], t.lo2.data(), t.hi2.data());
      a[gen_ipad(k, ps)] = p.zk;
      if (czt_pair_has_partner(g, k)) a[gen_ipad(kc, ps)] = p.zc;
    }
    czt_zero_tail(a.data(), g, tid, nthr);
  }
  run_conv(g, t, a.data(), nthr);
  store_frame(g, t, a.data(), out);
  return 0;
}
}
