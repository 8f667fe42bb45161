// rfx_czt_core.h - the CHIRP-Z frame transform: the generic engine's framed real FFT (rfx_gen_core.h) for lengths the mixed-radix
// passes cannot factor (a prime factor above 13 in nc = n_fft / 2, or in n_fft when it is odd).  Bluestein's identity
// n k = (n^2 + k^2 - (k - n)^2) / 2 turns the nc-point DFT into a circular convolution of any length np >= 2 nc - 1 with a chirp:
//     c[n] = exp(-i pi n^2 / nc)
//     1. y[n] = x[n] c[n] (n < nc), 0 (nc <= n < np)
//     2. forward in-place passes of length np (gen_ip_stage): Y, digit-reversed
//     3. Y *= H, H = FFT_np(wrapped conj c) / np stored at the same digit-reversed, padded positions
//     4. inverse in-place passes of length np: z, natural order
//     5. X[k] = c[k] z[k] (k < nc)
// np = the smallest length >= 2 nc - 1 that gen_factor accepts (GenGeom::np; radix list, per-pass twiddles, lo / hi tables, LDS
// padding and LDS size follow np, everything else of the geometry follows nc and n_fft).  The result is in NATURAL order, so the
// real <-> packed split and the pairwise Griffin-Lim projection of rfx_gen_core.h run on top of it with gen_ipad as their
// position map.  The unscaled inverse DFT is conj(DFT(conj Z)): the same tables.  c and H are built in double precision and
// rounded once (czt_tables); they live in global memory (they do not fit LDS next to the buffer).
// Written once for the gfx950 kernels (rfx_czt.hip) and for the host emulator of the CPU tests (tests/emu/rfx_czt_emu.cpp).
#pragma once
#include "rfx_gen_core.h"

#include <math.h>

#include <complex>
#include <vector>

namespace rfx {

constexpr size_t kCztLdsLimit = 160u * 1024u;  // LDS of a CU

// smallest pass length >= 2 nc - 1 the radix passes factor (0: none up to kGenMaxNc); its radix list
RFX_HD int czt_pass_len(int nc, int* radix, int* nstages) {
  for (int m = 2 * nc - 1; m <= kGenMaxNc; ++m)
    if (gen_factor(m, radix, nstages)) return m;
  return 0;
}
// the geometry as the PASSES see it: helpers of rfx_gen_core.h that walk the radix list by g.nc (gen_tw_table_offset,
// gen_digit_reverse, gen_pick_pad) and the table builders of plan creation take this copy
RFX_HD GenGeom czt_pass_geom(const GenGeom& g) {
  GenGeom p = g;
  p.nc = g.np;
  return p;
}
// LDS: the np-point buffer (padded), lo / hi of the passes (base np), lo2 / hi2 of the split (base n_fft).  One formula for the plan's
// check, the kernels' launch size and the stated limits
RFX_HD int czt_nhi(int np) { return np / kGenTwLo + 1; }   // GenGeom::nhi of a chirp-z plan
RFX_HD int czt_nhi2(int nc) { return nc / kGenTwLo + 2; }  // GenGeom::nhi2, as the generic plan's
RFX_HD size_t czt_lds_bytes_of(int np, int pad_shift, int nhi, int nhi2) {
  return sizeof(cf) * ((size_t)gen_ibuf_elems(np, pad_shift) + 2 * kGenTwLo + nhi + nhi2);
}
RFX_HD size_t czt_lds_bytes(const GenGeom& g) { return czt_lds_bytes_of(g.np, g.pad_shift, g.nhi, g.nhi2); }
// does a frame FFT of nc points fit (unpadded buffer)?  The limit the plan states is the largest nc that does.
RFX_HD bool czt_fits(int nc) {
  int radix[kGenMaxStages], ns;
  const int np = czt_pass_len(nc, radix, &ns);
  if (!np) return false;
  return czt_lds_bytes_of(np, 0, czt_nhi(np), czt_nhi2(nc)) <= kCztLdsLimit;
}
RFX_HD int czt_max_nc() {  // pass length and LDS need grow with nc: the first fit from above is the limit
  int nc = kGenMaxNc / 2 + 1;
  while (nc > 1 && !czt_fits(nc)) --nc;
  return nc;
}

// ---- per-thread arithmetic ---------------------------------------------------------------------------------------------------
RFX_HD cf czt_conj(cf a) { return cf{a.re, -a.im}; }
// step 1 / step 5: x c
RFX_HD cf czt_chirp(cf x, cf c) { return cmul(x, c); }
// step 1 of the inverse: conj(Z) c
RFX_HD cf czt_chirp_conj(cf x, cf c) { return cmul(czt_conj(x), c); }

// zeros behind the nc chirped samples
RFX_HD void czt_zero_tail(cf* buf, const GenGeom& g, int tid, int nthr) {
  for (int n = g.nc + tid; n < g.np; n += nthr) buf[gen_ipad(n, g.pad_shift)] = cf{0.f, 0.f};
}
// step 3 over the buffer as it lies in LDS (H has the buffer's layout, padding included).  Batches: the global loads of H first,
// then the LDS round trip
RFX_HD void czt_mul_h(cf* buf, const cf* __restrict__ H, const GenGeom& g, int tid, int nthr) {
  constexpr int U = 4;
  const int n = gen_ibuf_elems(g.np, g.pad_shift);
  for (int i0 = tid; i0 < n; i0 += U * nthr) {
    cf h[U], v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * nthr;
      h[u] = H[i < n ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * nthr;
      v[u] = buf[i < n ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * nthr;
      if (i < n) buf[i] = cmul(v[u], h[u]);
    }
  }
}
// bin k (0 <= k <= n_fft / 2) of the real FFT from the convolution's output z (step 5 and the real split in one):
// za = z[k] (z[0] for k == nc), zb = z[nc - k] (z[0] for k == 0), ca / cb the chirp at the same elements
RFX_HD cf czt_bin_vals(const GenGeom& g, cf za, cf ca, cf zb, cf cb, const cf* lo2, const cf* hi2, int k) {
  if (!g.even) return czt_chirp(za, ca);
  return gen_split_forward_vals(g, czt_chirp(za, ca), czt_chirp(zb, cb), lo2, hi2, k);
}
RFX_HD int czt_bin_elem_a(const GenGeom& g, int k) { return (g.even && k == g.nc) ? 0 : k; }
RFX_HD int czt_bin_elem_b(const GenGeom& g, int k) { return (!g.even || k == 0) ? 0 : g.nc - k; }

// Griffin-Lim between the two convolutions, one call per pair of elements (gen_pair_*): step 5 of the forward transform, the
// projection, and step 1 of the inverse transform.  ck / cc: the chirp at element k and at the partner element
// (nc - k when n_fft is even, n_fft - k when odd)
RFX_HD int czt_pair_partner(const GenGeom& g, int k) { return g.even ? (k == 0 ? 0 : g.nc - k) : (k == 0 ? 0 : g.n_fft - k); }
RFX_HD bool czt_pair_has_partner(const GenGeom& g, int k) { return g.even ? (k != 0 && k != g.nc - k) : k != 0; }
RFX_HD void czt_pair_compute(GenPair& p, const GenGeom& g, cf ck, cf cc, const cf* lo2, const cf* hi2, float eps2 = 1e-32f) {
  p.zk = czt_chirp(p.zk, ck);
  p.zc = g.even ? czt_chirp(p.zc, cc) : p.zk;
  gen_pair_compute(p, g, lo2, hi2, eps2);
  p.zk = czt_chirp_conj(p.zk, ck);
  p.zc = czt_chirp_conj(p.zc, cc);
}
// sample i of the padded frame from element zz = z[i >> 1] (even n_fft) or z[i] (odd) of the second convolution's output,
// c the chirp at that element: the packed signal is conj(c z)
RFX_HD float czt_out_sample(const GenGeom& g, cf zz, cf c, int i) {
  const cf w = czt_chirp(zz, c);
  return (g.even && (i & 1)) ? -w.im : w.re;
}

// ---- tables (host, double precision, rounded once) -----------------------------------------------------------------------------
constexpr double kCztPi = 3.14159265358979323846264338327950288;

inline std::complex<double> czt_chirp_double(long long n, long long nc) {  // exp(-i pi n^2 / nc), exponent reduced as an integer
  const long long e = (n * n) % (2 * nc);
  const double a = -kCztPi * (double)e / (double)nc;
  return {cos(a), sin(a)};
}
// double-precision DFT of any length (decimation in time over the smallest prime factor; O(n sum of prime factors)):
// w[t] = exp(-2 pi i t / n_root), the sub-transform of length n reads it with stride n_root / n
inline void czt_dft_double(const std::complex<double>* in, int stride, std::complex<double>* out, int n, const std::complex<double>* w, int n_root) {
  if (n == 1) {
    out[0] = in[0];
    return;
  }
  int p = 2;
  while (n % p) ++p;
  const int m = n / p, ws = n_root / n;
  for (int q = 0; q < p; ++q) czt_dft_double(in + (size_t)q * stride, stride * p, out + (size_t)q * m, m, w, n_root);
  std::vector<std::complex<double>> t(p), y(p);
  for (int k = 0; k < m; ++k) {
    for (int q = 0; q < p; ++q) t[q] = out[(size_t)q * m + k] * w[(size_t)q * k * ws];
    for (int r = 0; r < p; ++r) {
      std::complex<double> acc = t[0];
      for (int q = 1; q < p; ++q) acc += t[q] * w[(size_t)((q * r) % p) * (n_root / p)];
      y[r] = acc;
    }
    for (int r = 0; r < p; ++r) out[(size_t)k + (size_t)m * r] = y[r];
  }
}
// c [nc] in natural order; H [gen_ibuf_elems(np, pad_shift)]: H[k] = FFT_np(b)[k] / np at gen_ipad(digit-reversed k), zero in the
// padding, b[n] = b[np - n] = conj c[n] for n < nc and zero between
struct CztTables {
  std::vector<cf> c, h;
};
inline CztTables czt_tables(const GenGeom& g) {
  CztTables t;
  const int nc = g.nc, np = g.np;
  t.c.resize(nc);
  std::vector<std::complex<double>> b(np), w(np), Hd(np);
  for (int n = 0; n < nc; ++n) {
    const std::complex<double> c = czt_chirp_double(n, nc);
    t.c[n] = cf{(float)c.real(), (float)c.imag()};
    b[n] = std::conj(c);
    if (n) b[np - n] = std::conj(c);
  }
  for (int i = 0; i < np; ++i) {
    const double a = -2.0 * kCztPi * (double)i / (double)np;
    w[i] = {cos(a), sin(a)};
  }
  czt_dft_double(b.data(), 1, Hd.data(), np, w.data(), np);
  const GenGeom pg = czt_pass_geom(g);
  t.h.assign((size_t)gen_ibuf_elems(np, g.pad_shift), cf{0.f, 0.f});
  for (int k = 0; k < np; ++k) {
    const std::complex<double> v = Hd[k] / (double)np;
    t.h[gen_ipad(gen_digit_reverse(pg, k), g.pad_shift)] = cf{(float)v.real(), (float)v.imag()};
  }
  return t;
}

}  // namespace rfx
