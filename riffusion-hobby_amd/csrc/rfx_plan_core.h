// rfx_plan_core.h - the host half of plan creation: every decision that later picks a kernel (frame engine, InverseMelScale
// kernel, unit form, forward path) and every table the plan uploads, as plain functions of rfx_params, rfx_plan_options and the
// dense filterbank.  No device call and no environment read: rfx_plan_create_ex uploads what these functions return, and
// rfx_debug_plan_bank runs the same functions without a GPU (tests/test_plan_selection.py).
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rfx.h"
#include "rfx_czt_core.h"
#include "rfx_kernels.h"
#include "rfx_mel_bwd_core.h"
#include "rfx_vocoder_core.h"

namespace rfx {

// Experiment overrides of an ablation build, read from the environment by the caller; a release build passes the defaults
struct PlanOverrides {
  int gen_threads = 0;           // RFX_GEN_THREADS: threads per workgroup of the generic engine (a multiple of 64 in 64 .. 512)
  int gen_pad = -1;              // RFX_GEN_PAD: LDS padding shift of the generic engine (0, 3 .. 8; -1 = not given)
  bool fwd_table_form = false;   // RFX_FWD_V1: the forward path keeps the table form (stft_mel_kernel)
};

// ---- geometry: which frame engine a parameter set runs on ----------------------------------------------------------------
struct PlanGeometry {
  bool generic = false;  // every geometry but 17640 / 4410 / 441, or RFX_LAYOUT_GENERIC
  GenGeom gg{};          // valid when generic
  bool fam_ok = false;   // row family (n_fft = 40 h, win_length = 10 h) on top of the generic plan
  FamGeom fam{};
  int n_stft = 0;
  int frame_stride = kFrameStride;
  bool czt = false;      // chirp-z engine on top of the generic plan: gg.np > gg.nc (RFX_ENGINE_CHIRPZ and an unfactorable length)
  int engine() const { return !generic ? 0 : fam_ok ? 2 : czt ? 3 : 1; }  // as rfx_plan_griffinlim_engine answers
};

inline int plan_geometry(const rfx_params& p, const rfx_plan_options& opt, const PlanOverrides& ov, PlanGeometry* out, std::string* err) {
  PlanGeometry g;
  g.n_stft = p.n_fft / 2 + 1;
  g.generic = p.n_fft != kNfft || p.win_length != kWin || p.hop_length != kHop || opt.plan_layout == RFX_LAYOUT_GENERIC;
  GenGeom& gg = g.gg;
  if (g.generic) {
    // any geometry torch.stft accepts (0 < hop, 0 < win <= n_fft) whose FFT length factors into the implemented radices
    if (p.n_fft < 2 || p.hop_length < 1 || p.win_length < 1 || p.win_length > p.n_fft) {
      *err = "rfx_plan_create: need 0 < hop_length, 0 < win_length <= n_fft";
      return RFX_ERR_INVALID;
    }
    gg.n_fft = p.n_fft;
    gg.win = p.win_length;
    gg.hop = p.hop_length;
    gg.n_stft = g.n_stft;
    gg.even = p.n_fft % 2 == 0;
    gg.nc = gg.even ? p.n_fft / 2 : p.n_fft;
    gg.left = (p.n_fft - p.win_length) / 2;
    gen_frame_layout(gg);
    gg.fs = (gg.n_stft + 63) / 64 * 64;
    gg.nhi = gg.nc / kGenTwLo + 1;
    gg.nhi2 = gg.nc / kGenTwLo + 2;
    if (gg.nc > kGenMaxNc) {
      *err = "rfx_plan_create: n_fft = " + std::to_string(p.n_fft) + ": the frame's FFT buffer (" + std::to_string(gg.nc) +
             " complex numbers) does not fit the 160 KiB of LDS of a CU";
      return RFX_ERR_UNSUPPORTED;
    }
    gg.np = gg.nc;
    if (!gen_factor(gg.nc, gg.radix, &gg.nstages)) {
      if (opt.frame_engine != RFX_ENGINE_CHIRPZ) {
        *err = "rfx_plan_create: FFT length " + std::to_string(gg.nc) + " (from n_fft = " + std::to_string(p.n_fft) +
               ") has a prime factor above 13; implemented radices: 2, 3, 4, 5, 7, 11, 13 (rfx_plan_options.frame_engine = RFX_ENGINE_CHIRPZ "
               "runs such lengths on the chirp-z engine)";
        return RFX_ERR_UNSUPPORTED;
      }
      // chirp-z engine: the passes run at the convolution length np >= 2 nc - 1; the buffer of np complex numbers and the tables must
      // fit the LDS of a CU
      if (!czt_fits(gg.nc)) {
        const int lim = czt_max_nc();
        *err = "rfx_plan_create: n_fft = " + std::to_string(p.n_fft) + ": the chirp-z engine's convolution buffer (at least " +
               std::to_string(2 * gg.nc - 1) + " complex numbers for an FFT length of " + std::to_string(gg.nc) +
               ") and its twiddle tables do not fit the 160 KiB of LDS of a CU (largest supported: n_fft " + std::to_string(2 * lim) +
               " when even, " + std::to_string(lim % 2 ? lim : lim - 1) + " when odd)";
        return RFX_ERR_UNSUPPORTED;
      }
      gg.np = czt_pass_len(gg.nc, gg.radix, &gg.nstages);
      gg.nhi = czt_nhi(gg.np);
      gg.nhi2 = czt_nhi2(gg.nc);
      g.czt = true;
    }
    // threads per workgroup: measured on MI355X, the engine is latency bound and more waves win over fuller rounds
    // (48 kHz, 64 tiles x 32 iterations: 512 threads 121 ms, 384: 134, 320 - the count gen_pick_threads prefers: 155, 256: 163)
    gg.nthr = 512;
    if (ov.gen_threads >= 64 && ov.gen_threads <= 512 && ov.gen_threads % 64 == 0) gg.nthr = ov.gen_threads;
    // LDS padding: keep as many workgroups per CU as the unpadded buffer allows
    const size_t tables = sizeof(cf) * (2 * (size_t)kGenTwLo + gg.nhi + gg.nhi2);
    const size_t plain = sizeof(cf) * (size_t)gg.np + tables + 512;
    int per_cu = (int)((160u * 1024u) / plain);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 1024 / gg.nthr) per_cu = 1024 / gg.nthr;
    const size_t plain_room = (160u * 1024u) / per_cu;
    const size_t room = plain_room > tables + 512 ? plain_room - tables - 512 : 0;
    gg.pad_shift = gen_pick_pad(g.czt ? czt_pass_geom(gg) : gg, (int)(room / sizeof(cf)));
    if (ov.gen_pad == 0 || (ov.gen_pad >= 3 && ov.gen_pad <= 8)) gg.pad_shift = ov.gen_pad;
    if (g.czt) {
      if (czt_lds_bytes(gg) > kCztLdsLimit) gg.pad_shift = 0;
      if (czt_lds_bytes(gg) > kCztLdsLimit) {  // (czt_fits said otherwise: the two must share czt_lds_bytes_of)
        *err = "rfx_plan_create: n_fft = " + std::to_string(p.n_fft) + ": the chirp-z engine's buffer and tables (" + std::to_string(czt_lds_bytes(gg)) +
               " bytes) do not fit the 160 KiB of LDS of a CU";
        return RFX_ERR_UNSUPPORTED;
      }
    } else if (gen_lds_bytes(gg) > 160u * 1024u) gg.pad_shift = 0;
    if (!g.czt && gen_lds_bytes(gg) > 160u * 1024u) {
      *err = "rfx_plan_create: n_fft = " + std::to_string(p.n_fft) + ": the frame's FFT buffer and twiddle tables (" +
             std::to_string(gen_lds_bytes(gg)) + " bytes) do not fit the 160 KiB of LDS of a CU (largest supported: n_fft about 39000 when "
             "even, 19500 when odd)";
      return RFX_ERR_UNSUPPORTED;
    }
    g.frame_stride = gg.fs;
  }
  // Griffin-Lim of the geometries with n_fft = 40 h, win_length = 10 h (the default 400 / 100 ms at 48 / 32 / 24 / 16 / 8 kHz)
  // runs on the row-family kernels; the generic engine keeps everything else of the plan (layouts, forward path)
  FamGeom& fam = g.fam;
  g.fam_ok = g.generic && !g.czt && opt.frame_engine != RFX_ENGINE_GENERIC && fam_make_geom(p.n_fft, p.win_length, p.hop_length, &fam);
  if (g.fam_ok) {
    // pad the rows by up to seven elements (bank spread of the row-to-row accesses) as long as that costs no resident workgroup
    const size_t plain = fam_lds_bytes(fam) + fam_static_lds_bytes(fam);
    int per_cu = (int)((160u * 1024u) / plain);
    if (per_cu > 1024 / fam.nthr) per_cu = 1024 / fam.nthr;
    if (per_cu < 1) g.fam_ok = false;
    for (int pad = 7; g.fam_ok && pad > 0; --pad) {
      FamGeom t = fam;
      t.rs = fam.h + pad;
      if (fam_row_stride_even(fam) && t.rs % 2) continue;
      if ((fam_lds_bytes(t) + fam_static_lds_bytes(t)) * per_cu <= 160u * 1024u) { fam = t; break; }
    }
  }
  *out = g;
  return RFX_OK;
}

// ---- twiddle tables of the three frame engines (double precision, rounded once) --------------------------------------------
constexpr double kPi2 = 6.283185307179586476925286766559;

inline std::vector<cf> spec_twiddles1() {  // [21][441] g(n)^k1 of the specialised engine
  std::vector<cf> tw(21 * kHop);
  for (int k1 = 0; k1 < 21; ++k1)
    for (int n = 0; n < kHop; ++n) {
      const long long e = ((long long)k1 * (n + 6615)) % kNfft;
      tw[k1 * kHop + n] = cf{(float)cos(kPi2 * (double)e / kNfft), (float)(-sin(kPi2 * (double)e / kNfft))};
    }
  return tw;
}
inline std::vector<cf> spec_twiddles2() {  // [21][21] W_441^{i j}
  std::vector<cf> tw(21 * 21);
  for (int i = 0; i < 21; ++i)
    for (int j = 0; j < 21; ++j) {
      const int e = (i * j) % kHop;
      tw[i * 21 + j] = cf{(float)cos(kPi2 * e / (double)kHop), (float)(-sin(kPi2 * e / (double)kHop))};
    }
  return tw;
}
// generic engine: two-level twiddle tables of the Stockham passes (base nc) and of the real <-> packed split (base n_fft),
// lo [kGenTwLo] | hi [nhi] | lo2 [kGenTwLo] | hi2 [nhi2]
inline std::vector<cf> gen_two_level_twiddles(const GenGeom& gg) {
  std::vector<cf> t(2 * kGenTwLo + gg.nhi + gg.nhi2);
  cf* lo = t.data();
  cf* hi = lo + kGenTwLo;
  cf* lo2 = hi + gg.nhi;
  cf* hi2 = lo2 + kGenTwLo;
  auto root = [](long long num, long long den) {
    const double a = -kPi2 * (double)(num % den) / (double)den;
    return cf{(float)cos(a), (float)sin(a)};
  };
  for (int i = 0; i < kGenTwLo; ++i) { lo[i] = root(i, gg.nc); lo2[i] = root(i, gg.n_fft); }
  for (int i = 0; i < gg.nhi; ++i) hi[i] = root((long long)i * kGenTwLo, gg.nc);
  for (int i = 0; i < gg.nhi2; ++i) hi2[i] = root((long long)i * kGenTwLo, gg.n_fft);
  return t;
}
inline std::vector<int> gen_rev_table(const GenGeom& gg) {  // LDS position incl. padding of element k after the forward passes
  std::vector<int> rev(gg.nc);
  for (int k = 0; k < gg.nc; ++k) rev[k] = gen_ipad(gen_digit_reverse(gg, k), gg.pad_shift);
  return rev;
}
inline std::vector<cf> gen_pass_twiddles(const GenGeom& gg) {  // exact twiddles of every pass
  std::vector<cf> twt((size_t)gen_tw_table_elems(gg) + 1);
  for (int s2 = 0, L = gg.nc; s2 < gg.nstages; ++s2) {
    const int R = gg.radix[s2], m = L / R, off = gen_tw_table_offset(gg, s2);
    for (int i = 0; i < m; ++i)
      for (int q = 1; q < R; ++q) {
        const double ang = -kPi2 * (double)(((long long)i * q) % L) / (double)L;
        twt[(size_t)off + (size_t)i * (R - 1) + q - 1] = cf{(float)cos(ang), (float)sin(ang)};
      }
    L = m;
  }
  return twt;
}
inline std::vector<cf> fam_twiddles(const FamGeom& f) {  // [rows][h] g(n')^k1, then [ra-1][rb] W_h^{i p}
  std::vector<cf> tw((size_t)f.rows * f.h + (size_t)f.rb * (f.ra - 1));
  for (int k1 = 0; k1 < f.rows; ++k1)
    for (int n = 0; n < f.h; ++n) {  // g(n)^k1 = exp(-2 pi i k1 (n + left) / n_fft); left = 15 h in the 40 h family
      const long long e = ((long long)k1 * (n + f.left)) % f.n_fft;
      tw[(size_t)k1 * f.h + n] = cf{(float)cos(kPi2 * (double)e / f.n_fft), (float)(-sin(kPi2 * (double)e / f.n_fft))};
    }
  cf* twa = tw.data() + (size_t)f.rows * f.h;
  for (int i = 0; i < f.rb; ++i)
    for (int q = 1; q < f.ra; ++q) {
      const int e = (i * q) % f.h;
      twa[(size_t)(q - 1) * f.rb + i] = cf{(float)cos(kPi2 * e / (double)f.h), (float)(-sin(kPi2 * e / (double)f.h))};
    }
  return tw;
}
// chirp-z engine: the chirp and H (czt_tables), the passes' tables at the convolution length
struct CztPlanTables {
  std::vector<cf> two_level, pass_tw, c, h;
};
inline CztPlanTables czt_plan_tables(const GenGeom& gg) {
  const GenGeom pg = czt_pass_geom(gg);  // lo / hi base np [nhi], lo2 / hi2 base n_fft [nhi2]
  CztTables t = czt_tables(gg);
  return CztPlanTables{gen_two_level_twiddles(pg), gen_pass_twiddles(pg), std::move(t.c), std::move(t.h)};
}
inline std::vector<int> fam_bin_of(const FamGeom& f) {  // [fsf] bin held by each position of the slot-ordered magnitudes (-1: padding)
  std::vector<int> binof((size_t)f.fsf, -1);
  for (int k1 = 0; k1 < f.rows; ++k1)
    for (int q = 0; q < f.ra; ++q)
      for (int s2 = 0; s2 < f.rb; ++s2) binof[(size_t)s2 * f.nthr + k1 * f.ra + q] = fam_slot_bin(f, k1, q, s2, nullptr);
  return binof;
}

// ---- filterbank analysis ---------------------------------------------------------------------------------------------------
// [2 F]: for every bin the first band with a nonzero weight (lo, [0, F)) and the last (hi, [F, 2 F)); -1 / -1 for a bin no filter
// reaches.  What rfx_hold_bins_from_bands expands a per-band mask by (rfx_holdmask_core.h); n_mels < 2^15.
inline std::vector<int16_t> bin_bands(int F, int M, const float* fb) {
  std::vector<int16_t> v((size_t)2 * F, (int16_t)-1);
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < M; ++m)
      if (fb[(size_t)f * M + m] != 0.f) {
        if (v[f] < 0) v[f] = (int16_t)m;
        v[(size_t)F + f] = (int16_t)m;
      }
  return v;
}

struct SlotEntry { float w0, w1; };
constexpr double kImelLineTol = 4e-7;  // of a group's largest weight: see bank_groups

struct PlanBank {
  int F = 0, M = 0;
  bool generic = false;
  int frame_stride = kFrameStride;
  // banded view (InverseMelScale): every bin feeds at most two ADJACENT mel filters, every filter's support is one run of bins
  bool ok = true;
  std::string why;
  std::vector<int> bin_m0, band_lo, band_hi, csr_ptr;
  std::vector<float> bin_w0, bin_w1, csr_w;
  int f_lo = 0, f_hi = 0;  // bins with a non-zero filterbank row: [f_lo, f_hi)
  // where a bin lives in a frame: primary slot, duplicate slot (-1), the inverse map, and the primary slot's (q, kb)
  std::vector<int> bin_pos, bin_pos2, pos_bin, slot_q, slot_kb;
  // dense bank in slot order and its non-zero 32-position K blocks (specialised engine, MelScale GEMM)
  int melfb_cols = 0;
  std::vector<float> fbs;
  std::vector<int> kblocks;
  // groups (bins whose first filter is g), shared by the SGD admission and the forward product form
  bool grouped = false;
  std::vector<int> cnt, grp_start;
  std::vector<float> lin;  // [4][M] a0 | s0 | a1 | s1
  int line_from = 0;
  double line_dev = -1.0;  // largest |line - weight| over the group's largest weight, all non-empty groups (-1: no groups)
  // the scalars of ImelTables (pointers null): fast_ok, unit_form, wave_ok, line_from, f_lo, f_hi, nnz
  ImelTables imel{};
  // forward path: band tables, then the product form's tables
  bool fwd_ok = false;
  int band_rows = 0, Mpad = 0;
  std::vector<float> wt;
  std::vector<int> addr, lo_len;
  bool prod_ok = false, packed = false;
  std::vector<SlotEntry> tab;
  std::vector<int> tab_at, padtab, seg;
  std::vector<unsigned> pk;
  unsigned mask = 0;
  int arr = 0;
  // backward of the forward path: first band, count and weights of every bin (rfx_mel_bwd_core.h; any bank, banded or not)
  MelAdjoint adj;
};

// banded tables for InverseMelScale: every bin feeds at most two ADJACENT mel filters and every filter's support is one
// contiguous run of bins (true for torchaudio's triangular banks)
inline void bank_banded_view(PlanBank& b, const float* fb) {
  const int F = b.F, M = b.M;
  b.bin_m0.assign(F, -1);
  b.band_lo.assign(M, 0);
  b.band_hi.assign(M, 0);
  b.csr_ptr.assign(M + 1, 0);
  b.bin_w0.assign(F, 0.f);
  b.bin_w1.assign(F, 0.f);
  bool& ok = b.ok;
  int f_lo = F, f_hi = 0;
  for (int f = 0; f < F && ok; ++f) {
    int first = -1, cnt = 0, last = -1;
    for (int m = 0; m < M; ++m)
      if (fb[(size_t)f * M + m] != 0.f) { if (first < 0) first = m; last = m; ++cnt; }
    if (cnt == 0) continue;
    if (cnt > 2 || last - first != cnt - 1) { ok = false; b.why = "a linear bin feeds more than two adjacent mel filters"; break; }
    b.bin_m0[f] = first;
    b.bin_w0[f] = fb[(size_t)f * M + first];
    b.bin_w1[f] = cnt == 2 ? fb[(size_t)f * M + first + 1] : 0.f;
    f_lo = f < f_lo ? f : f_lo;
    f_hi = f + 1;
  }
  for (int m = 0; m < M && ok; ++m) {
    int lo = -1, hi = -1;
    for (int f = 0; f < F; ++f)
      if (fb[(size_t)f * M + m] != 0.f) { if (lo < 0) lo = f; hi = f + 1; }
    if (lo < 0) { lo = hi = (f_lo < F ? f_lo : 0); }
    for (int f = lo; f < hi; ++f)
      if (fb[(size_t)f * M + m] == 0.f) { ok = false; b.why = "a mel filter's support is not contiguous"; break; }
    b.band_lo[m] = lo;
    b.band_hi[m] = hi;
    b.csr_ptr[m] = (int)b.csr_w.size();
    for (int f = lo; f < hi; ++f) b.csr_w.push_back(fb[(size_t)f * M + m]);
  }
  b.csr_ptr[M] = (int)b.csr_w.size();
  if (ok && (f_hi <= f_lo)) { ok = false; b.why = "empty filterbank"; }
  if (ok && (f_hi - f_lo > 36 * 256)) { ok = false; b.why = "more than 9216 active bins"; }
  if (ok && M > 1024) { ok = false; b.why = "more than 1024 mel filters"; }
  b.f_lo = f_lo;
  b.f_hi = f_hi;
}

// The one walk of the 21 x 21 x 21 slot cube: the first slot that holds a bin is its primary slot, the second (440 bins have
// one) its duplicate.  A generic plan stores plain bin-ordered frames.  Then the dense bank in slot order - row of position p =
// filterbank row of its bin for PRIMARY slots, zero for the duplicates and the padding, so a GEMM over slot order equals the
// reference's GEMM over bins up to summation order - with columns padded to the GEMM's 128-row tile.
inline void bank_slots(PlanBank& b, const float* fb) {
  const int F = b.F, M = b.M;
  b.bin_pos.assign(F, -1);
  b.bin_pos2.assign(F, -1);
  b.slot_q.assign(F, -1);
  b.slot_kb.assign(F, -1);
  if (b.generic)
    for (int f = 0; f < F; ++f) b.bin_pos[f] = f;
  else
    for (int k1 = 0; k1 < 21; ++k1)
      for (int ka = 0; ka < 21; ++ka)
        for (int kb = 0; kb < 21; ++kb) {
          const int bin = slot_bin(k1, ka, kb, nullptr), pos = slot_pos_f(k1 * 21 + ka, kb);
          if (b.bin_pos[bin] < 0) { b.bin_pos[bin] = pos; b.slot_q[bin] = k1 * 21 + ka; b.slot_kb[bin] = kb; }
          else b.bin_pos2[bin] = pos;
        }
  b.pos_bin.assign((size_t)b.frame_stride, -1);  // a bin with two slots appears at both; padding positions hold -1
  for (int f = 0; f < F; ++f) {
    if (b.bin_pos[f] >= 0) b.pos_bin[b.bin_pos[f]] = f;
    if (b.bin_pos2[f] >= 0) b.pos_bin[b.bin_pos2[f]] = f;
  }
  const int Mp = b.melfb_cols = (M + 127) / 128 * 128;
  if (b.generic) return;
  b.fbs.assign((size_t)kFrameStride * Mp, 0.f);
  for (int f = 0; f < F; ++f)
    if (b.bin_pos[f] >= 0) memcpy(&b.fbs[(size_t)b.bin_pos[f] * Mp], &fb[(size_t)f * M], M * sizeof(float));
  for (int blk = 0; blk < kFrameStride / 32; ++blk) {
    bool nz = false;
    for (int r = blk * 32; r < blk * 32 + 32 && !nz; ++r)
      for (int m = 0; m < M; ++m)
        if (b.fbs[(size_t)r * Mp + m] != 0.f) { nz = true; break; }
    if (nz) b.kblocks.push_back(blk);
  }
}

// Group structure: active bins contiguous with no zero row inside, first-filter index non-decreasing, at most 512 filters.
// Then the weights as a LINE per group: on a uniform bin grid a triangular filter's weight is linear in the bin index between two
// centres, w0 = a0 + s0 i, w1 = a1 + s1 i for the group's i-th bin (least-squares line in double, checked per bin).  The
// tolerance is RELATIVE to the group's largest weight (an area-normalised bank has weights ~1e-2: an absolute 1e-6 would
// admit 1e-4 relative there).  Measured on the reference's banks (tests/test_round5_cpu.py): 0.72e-7 of the group maximum
// for htk / no norm, 1.16e-7 for slaney - one ulp of the largest weight; 4e-7 leaves a factor of three.
// line_from = the lowest group from which every group is a line (group 0 of a bank whose first filter rises over several
// bins holds that rising edge AND its own falling one: a kink)
inline void bank_groups(PlanBank& b) {
  const int M = b.M;
  b.grp_start.assign(M + 1, 0);
  b.grouped = b.ok && M <= 512;
  for (int f = b.f_lo, prev = 0; f < b.f_hi && b.grouped; ++f) {
    if (b.bin_m0[f] < prev) b.grouped = false;  // (a zero row has bin_m0 == -1)
    else prev = b.bin_m0[f];
  }
  if (!b.grouped) return;
  b.cnt.assign(M, 0);
  for (int f = b.f_lo; f < b.f_hi; ++f) b.cnt[b.bin_m0[f]]++;
  int acc = b.f_lo;
  for (int g = 0; g < M; ++g) { b.grp_start[g] = acc; acc += b.cnt[g]; }
  b.grp_start[M] = acc;
  b.lin.assign(4 * (size_t)M, 0.f);
  b.line_dev = 0.0;
  for (int g = 0; g < M; ++g) {
    const int n = b.cnt[g], f0 = b.grp_start[g];
    if (n == 0) continue;
    for (int which = 0; which < 2; ++which) {
      const std::vector<float>& w = which ? b.bin_w1 : b.bin_w0;
      double sx = 0, sy = 0, sxx = 0, sxy = 0;
      for (int i = 0; i < n; ++i) { sx += i; sy += w[f0 + i]; sxx += (double)i * i; sxy += (double)i * w[f0 + i]; }
      const double den = n * sxx - sx * sx;
      const double slope = n > 1 ? (n * sxy - sx * sy) / den : 0.0, icpt = (sy - slope * sx) / n;
      const float af = (float)icpt, sf = (float)slope;
      double wmax = 0, dev = 0;
      for (int i = 0; i < n; ++i) wmax = fmax(wmax, fabs((double)w[f0 + i]));
      for (int i = 0; i < n; ++i) dev = fmax(dev, fabs((double)af + (double)sf * i - (double)w[f0 + i]));
      if (dev > kImelLineTol * wmax) b.line_from = g + 1;
      b.line_dev = fmax(b.line_dev, dev / fmax(wmax, 1e-30));
      b.lin[(size_t)(2 * which) * M + g] = af;
      b.lin[(size_t)(2 * which + 1) * M + g] = sf;
    }
  }
}

// which register budgets the bank's groups fit: thread role t owns the long group M-1-t and the short group t
inline bool groups_fit(const PlanBank& b, const int* lo_cap, const int* hi_cap) {
  for (int t = 0; t < 256; ++t) {
    const int gH = b.M - 1 - t, gL = t < b.M - 256 ? t : -1;
    if (gH >= 0 && b.cnt[gH] > hi_cap[t >> 6]) return false;
    if (gL >= 0 && b.cnt[gL] > lo_cap[t >> 6]) return false;
    if (gL >= 0 && gH >= 0 && gL >= gH) return false;
  }
  return true;
}
// the line-form group kernel's set: a long group that is NOT a line - group 0 of a bank with at most 256 filters - moves into its
// thread's free table-form slot
inline bool groups_fit_line(const PlanBank& b) {
  for (int t = 0; t < 256; ++t) {
    const int gH = b.M - 1 - t, gL = t < b.M - 256 ? t : -1, c = t >> 6;
    if (gH >= 0 && gH < b.line_from) {
      if (gL >= 0 || b.cnt[gH] > kImelLoCapLine[c]) return false;
    } else if (gH >= 0 && b.cnt[gH] > kImelHiCapLine[c]) return false;
    if (gL >= 0 && b.cnt[gL] > kImelLoCapLine[c]) return false;
    if (gL >= 0 && gH >= 0 && gL >= gH) return false;
  }
  return true;
}

// Which SGD kernel family the bank admits (ImelTables::fast_ok), the gradient's unit form and the wave kernel.
// Per-wave budgets of imel_group_kernel_perwave (rfx_kernels.h): the default bank's exact set (kImelKernelPerWave), then the wide
// set (kImelKernelPerWaveWide); banks whose groups are too long for either (max_frequency above ~11 kHz at 512 filters - the
// reference's own round-trip test uses 20 Hz .. 20 kHz, test/spectrogram_converter_test.py:46-53 - or fewer filters) take the
// line-form group kernel (round 5: imel_line_kernel_perwave, kImelKernelLine) when their LONG groups M-256 .. M-1 are lines; they
// ran on the general LDS kernel until then: 169 ms per 64 tiles against 4.5 for the default bank.  Then the uniform budget
// (kImelKernelUniform), else the general kernel.
inline void bank_sgd_admission(PlanBank& b, int imel_form) {
  if (!b.ok) return;
  const int M = b.M;
  ImelKernel fast_code = kImelKernelGeneral;
  bool unit_form = false, wave_ok = false;
  if (b.grouped) {
    const int uni_lo[4] = {8, 8, 8, 8}, uni_hi[4] = {24, 24, 24, 24};
    fast_code = groups_fit(b, kImelLoCap, kImelHiCap)           ? kImelKernelPerWave
                : groups_fit(b, kImelLoCapWide, kImelHiCapWide) ? kImelKernelPerWaveWide
                : groups_fit_line(b)                            ? kImelKernelLine
                : groups_fit(b, uni_lo, uni_hi)                 ? kImelKernelUniform
                                                                : kImelKernelGeneral;
    // unit form of the gradient: the long groups M-256 .. M-1 must have w0 + w1 == 1 per bin (triangular
    // filters, no area normalisation), the last one w1 == 0 throughout (there is no filter M)
    unit_form = fast_code != kImelKernelGeneral && fast_code != kImelKernelUniform;
    for (int f = b.f_lo; f < b.f_hi && unit_form; ++f) {
      const int g = b.bin_m0[f];
      if (g < M - 256) continue;
      if (g == M - 1) unit_form = b.bin_w1[f] == 0.f;
      else unit_form = fabsf(b.bin_w0[f] + b.bin_w1[f] - 1.f) <= 1e-6f;
    }
    // wave kernel (imel_wave_kernel): 512 groups dealt to 64 lanes in eight chunks whose budgets must hold every
    // group, every group a line; with the unit form (no area normalisation) the upper four chunks need one weight only
    wave_ok = imel_form == RFX_IMEL_FORM_AUTO && fast_code == kImelKernelPerWave && M == 64 * kImelWaveChunks && b.line_from == 0;
    for (int c = 0; c < kImelWaveChunks && wave_ok; ++c)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = b.cnt[imel_wave_group(c, lane)];
        if (n > 2 * kImelWavePairs[c] || n < 2 * kImelWaveFullPairs[c]) wave_ok = false;
      }
  }
  b.imel.fast_ok = fast_code;
  b.imel.unit_form = unit_form ? 1 : 0;
  b.imel.wave_ok = wave_ok ? 1 : 0;
  b.imel.line_from = b.line_from;
  b.imel.f_lo = b.f_lo;
  b.imel.f_hi = b.f_hi;
  b.imel.nnz = (int)b.csr_w.size();
}

// fused forward path: per-filter band tables, weights transposed so that lane m reads row i coalesced
inline void bank_forward_bands(PlanBank& b, const float* fb) {
  const int M = b.M;
  if (!b.ok || !(b.generic || M <= 2 * kThreads)) return;
  const int Mpad = b.Mpad = (M + 63) / 64 * 64;
  int rows = 1;
  for (int m = 0; m < M; ++m) rows = b.band_hi[m] - b.band_lo[m] > rows ? b.band_hi[m] - b.band_lo[m] : rows;
  rows = b.band_rows = (rows + 7) / 8 * 8;  // the kernel reads eight rows per step
  b.wt.assign((size_t)rows * Mpad, 0.f);
  b.lo_len.assign(2 * (size_t)Mpad, 0);  // [Mpad] first bin, [Mpad] bins of filter m's band
  for (int m = 0; m < M; ++m) {
    b.lo_len[m] = b.band_lo[m];
    b.lo_len[Mpad + m] = b.band_hi[m] - b.band_lo[m];
    for (int f = b.band_lo[m]; f < b.band_hi[m]; ++f) b.wt[(size_t)(f - b.band_lo[m]) * Mpad + m] = fb[(size_t)f * M + m];
  }
  if (!b.generic) {  // where the fused kernel finds bin f in LDS: float view of the cube, primary slot of the bin
    b.addr.assign((size_t)rows * Mpad, 0);
    for (int m = 0; m < M; ++m)
      for (int f = b.band_lo[m]; f < b.band_hi[m]; ++f) {
        const int k = (f % 40 > 20) ? kNfft - f : f;  // bins with residue 21..39 live in conjugate slots
        const int k1 = k % 40, kp = k / 40;
        b.addr[(size_t)(f - b.band_lo[m]) * Mpad + m] = 2 * cube_at(k1, kp % 21, 0) + kp / 21;
      }
  }
  b.fwd_ok = true;
}

// Product form of the fused kernel (stft_mel2_kernel).  Needs the group structure of the bank, so that filter m = (w1 products of
// group m-1) + (w0 products of group m).  Its sum phase gives every thread one filter and the first wave a second one:
// Mpad <= kThreads + 64 (banks of up to 512 filters); wider banks keep the table form (stft_mel_kernel), which handles two
// filters per thread up to 2 * kThreads.
// LDS layout in floats: [0, kQPad) one dump float per lane, [kQPad, G[M]) the w0 products group by group, then at the distance
// `arr` the same again for w1 - its dump floats [arr, arr + kQPad) sit behind the w0 array, its products at arr + G[g].
// (Rounds 3-4 put the dump floats behind both arrays: the w1 dump stores of a non-contributing slot then aimed past the cube
// for banks beyond 6000 padded bins and relied on the LDS range check dropping them.)
inline void bank_forward_products(PlanBank& b, const float* fb, bool table_form) {
  const int M = b.M, Mpad = b.Mpad;
  if (!b.fwd_ok || b.generic || Mpad > kThreads + 64 || table_form || !b.grouped) return;
  const std::vector<int>& cnt = b.cnt;
  std::vector<int> G(M + 1, kQPad);  // padded position of group g
  for (int g = 0; g < M; ++g) G[g + 1] = G[g] + (cnt[g] + 3) / 4 * 4;
  // the packed tables of the default-bank kernel want the second array at a compile-time distance: the gap behind G[M] is never read
  const bool packed_ok = G[M] <= kMelProdArr;
  const int arr = packed_ok ? kMelProdArr : G[M];
  if (arr + G[M] + 16 > 2 * kCubeElems) return;  // (a short segment's four unconditional 16-byte reads may run 12 floats past the last group)
  // every filter must equal its two group sums exactly: check weights against the dense bank
  for (int m = 0; m < M; ++m)
    for (int f = b.band_lo[m]; f < b.band_hi[m]; ++f) {
      const float want = fb[(size_t)f * M + m];
      if (!((b.bin_m0[f] == m && b.bin_w0[f] == want) || (b.bin_m0[f] == m - 1 && b.bin_w1[f] == want))) return;
    }
  std::vector<int> pads;
  for (int g = 0; g < M; ++g)
    for (int p = G[g] + cnt[g]; p < G[g + 1]; ++p) pads.push_back(p);
  if ((int)pads.size() > kMelPadsPerThread * kHop) return;
  for (int m = 0; m < M; ++m)
    if (cnt[m] > 60) return;  // a segment is (first float << 4) | 16-byte reads: groups hold at most 60 bins here
  // a slot that contributes nothing and a padding entry a thread does not need aim at the lane's dump float
  b.tab.assign(21 * (size_t)kQPad, SlotEntry{0.f, 0.f});
  b.tab_at.resize(21 * (size_t)kQPad);
  for (int kb = 0; kb < 21; ++kb)
    for (int qp = 0; qp < kQPad; ++qp) b.tab_at[(size_t)kb * kQPad + qp] = qp;
  for (int bin = b.f_lo; bin < b.f_hi; ++bin) {  // the duplicate slot of a bin contributes nothing
    const int g = b.bin_m0[bin], at = b.slot_kb[bin] * kQPad + slot_qp(b.slot_q[bin]);
    b.tab[at] = SlotEntry{b.bin_w0[bin], b.bin_w1[bin]};
    b.tab_at[at] = G[g] + (bin - b.grp_start[g]);
    b.mask |= 1u << b.slot_kb[bin];
  }
  b.padtab.resize((size_t)kMelPadsPerThread * kQPad);
  for (int i = 0; i < kMelPadsPerThread; ++i)
    for (int qp = 0; qp < kQPad; ++qp) b.padtab[(size_t)i * kQPad + qp] = qp;
  for (size_t i = 0; i < pads.size(); ++i) b.padtab[(i / kHop) * kQPad + slot_qp((int)(i % kHop))] = pads[i];
  b.seg.assign(2 * (size_t)Mpad, 0);
  for (int m = 0; m < M; ++m) {
    if (m > 0) b.seg[m] = ((arr + G[m - 1]) << 4) | ((cnt[m - 1] + 3) / 4);  // rising: w1 products of group m-1
    b.seg[(size_t)Mpad + m] = (G[m] << 4) | ((cnt[m] + 3) / 4);              // falling: w0 products of group m
  }
  b.arr = arr;
  b.prod_ok = true;
  // packed copies for the default-bank kernel (rfx_kernels.h: pk_at / pk_pad / pk_seg)
  b.packed = packed_ok && (b.mask & ~kKbMaskLow) == 0 && G[M] * 4 <= 65536;  // (16-bit byte addresses of the first array)
  if (!b.packed) return;
  b.pk.assign(5 * (size_t)kQPad + 2 * (size_t)kQPad + 2 * (size_t)Mpad, 0u);
  int kbs[10], n = 0;
  for (int kb = 0; kb < 21; ++kb)
    if ((kKbMaskLow >> kb) & 1u) kbs[n++] = kb;
  for (int i = 0; i < 5; ++i)
    for (int qp = 0; qp < kQPad; ++qp)
      b.pk[(size_t)i * kQPad + qp] = (unsigned)(4 * b.tab_at[(size_t)kbs[2 * i] * kQPad + qp]) | ((unsigned)(4 * b.tab_at[(size_t)kbs[2 * i + 1] * kQPad + qp]) << 16);
  unsigned* pkpad = b.pk.data() + 5 * (size_t)kQPad;
  for (int qp = 0; qp < kQPad; ++qp)
    for (int w = 0; w < 2; ++w)
      pkpad[2 * qp + w] = (unsigned)(4 * b.padtab[(size_t)(2 * w) * kQPad + qp]) | ((unsigned)(4 * b.padtab[(size_t)(2 * w + 1) * kQPad + qp]) << 16);
  unsigned* pkseg = pkpad + 2 * (size_t)kQPad;
  for (int m = 0; m < Mpad; ++m) {
    pkseg[2 * m] = (unsigned)b.seg[m];
    pkseg[2 * m + 1] = (unsigned)b.seg[(size_t)Mpad + m];
  }
}

// ---- closed-form InverseMelScale (rfx_imel_lstsq.hip): the factor tables of G = fb^T fb -----------------------------------------
// In a banded bank every bin touches at most two ADJACENT filters, so G is symmetric tridiagonal: diagonal d[m] = sum w(f, m)^2,
// off-diagonal e[m] = sum w(f, m) w(f, m + 1), both in double from the float32 weights.  G = L D L^T with L unit lower bidiagonal:
// D[0] = d[0], l[m] = e[m] / D[m], D[m + 1] = d[m + 1] - l[m] e[m].  The kernels read nl[m] = -l[m] (nl[M - 1] = 0) and
// inv_d[m] = 1 / D[m], rounded once to float32.  A pivot D[m] <= 2^-20 d[m] refuses the bank: G is singular or nearly so (an
// empty filter, or filters that cannot be told apart on this bin grid), which torch.linalg.lstsq's "gels" does not support either.
constexpr double kLsqPivotFloor = 1.0 / 1048576.0;  // 2^-20
struct LstsqBank {
  bool ok = false;
  std::string why;
  double min_pivot_ratio = 0.0;  // smallest D[m] / d[m] seen (up to and including a refused pivot); 0 when no factorisation was tried
  int min_pivot = -1;            // its index
  std::vector<float> nl, inv_d;  // [M]
  // per position of an output frame (PlanBank::pos_bin order): first filter and weights of the bin it holds; a position without
  // a bin and a bin without a filter point at the zero the kernel keeps behind y: (M, 0, 0)
  std::vector<int> pos_m0;
  std::vector<float> pos_w0, pos_w1;
};
inline LstsqBank bank_lstsq(const PlanBank& b) {
  LstsqBank q;
  const int F = b.F, M = b.M;
  if (!b.ok) {
    q.why = "the filterbank is not banded: " + b.why;
    return q;
  }
  std::vector<double> d(M, 0.0), e(M, 0.0);
  for (int f = 0; f < F; ++f) {
    const int m = b.bin_m0[f];
    if (m < 0) continue;
    const double w0 = b.bin_w0[f], w1 = b.bin_w1[f];
    d[m] += w0 * w0;
    if (m + 1 < M) {
      d[m + 1] += w1 * w1;
      e[m] += w0 * w1;
    }
  }
  q.nl.assign(M, 0.f);
  q.inv_d.assign(M, 0.f);
  q.min_pivot_ratio = INFINITY;
  double D = d[0];
  for (int m = 0; m < M; ++m) {
    const double ratio = d[m] > 0.0 ? D / d[m] : 0.0;
    if (ratio < q.min_pivot_ratio) { q.min_pivot_ratio = ratio; q.min_pivot = m; }
    if (!(D > kLsqPivotFloor * d[m])) {
      char msg[160];
      snprintf(msg, sizeof(msg), "pivot %d of the LDL^T factorisation of fb^T fb is %.3g times its diagonal entry %.3g: singular or nearly so",
               m, ratio, d[m]);
      q.why = msg;
      q.nl.clear();
      q.inv_d.clear();
      return q;
    }
    q.inv_d[m] = (float)(1.0 / D);
    if (m + 1 < M) {
      const double l = e[m] / D;
      q.nl[m] = (float)(-l);
      D = d[m + 1] - l * e[m];
    }
  }
  const size_t P = b.pos_bin.size();
  q.pos_m0.assign(P, M);
  q.pos_w0.assign(P, 0.f);
  q.pos_w1.assign(P, 0.f);
  for (size_t p = 0; p < P; ++p) {
    const int f = b.pos_bin[p];
    if (f < 0 || b.bin_m0[f] < 0) continue;
    q.pos_m0[p] = b.bin_m0[f];
    q.pos_w0[p] = b.bin_w0[f];
    q.pos_w1[p] = b.bin_w1[f];
  }
  q.ok = true;
  return q;
}

// Backward of the closed form (rfx_imel_lstsq.hip: lsq_collect_kernel; the order is rfx_imel_lstsq_core.h's): what the collect
// c = fb^T (gx where the relu is open) walks.  A filter's bins are one run [band_lo, band_hi) of ascending bins, so the lists are
// CSR over filters: ptr [M + 1], and per entry the bin, the weight fb[bin][m] (= bin_w0 of a bin whose first filter is m, bin_w1 of
// one whose first filter is m - 1) and the position of the frame the bin is read from.  A bin counts ONCE: from its FIRST slot
// (PlanBank::bin_pos; the specialised layout holds 440 bins a second time at bin_pos2, which the collect never reads, as it never
// reads padding or a bin without a filter).
// The kernel stages a frame's masked gradient in bin order, bins [f_lo, f_hi) at index bin - f_lo: `first` is a filter's run there,
// and the frame's 16-byte vectors that hold at least one counted position are listed with, per element, where it goes and what the
// mask needs: at = index | first filter << 16 (index 0xffff: not counted), and the bin's two weights.
struct LstsqCollect {
  std::vector<int> ptr, bin, pos;  // [M + 1], [nnz], [nnz]
  std::vector<float> w;            // [nnz]
  int n_bins = 0;                  // f_hi - f_lo: floats of the staged frame
  std::vector<int> first, run;     // [M] where a filter's run starts in the staged frame, and its length
  std::vector<float> wt;           // [longest run][M]: w transposed, entry i of filter m at i * M + m (0 behind a run's end)
  std::vector<int> vec;            // [n_vecs] index of the 16-byte vector in a frame
  std::vector<int> vec_at;         // [n_vecs][4]
  std::vector<float> vec_w0, vec_w1;  // [n_vecs][4]
};
inline LstsqCollect bank_lstsq_collect(const PlanBank& b) {
  LstsqCollect q;
  const int M = b.M;
  q.ptr.assign(M + 1, 0);
  q.first.assign(M, 0);
  for (int m = 0; m < M; ++m) {
    q.ptr[m] = (int)q.w.size();
    q.first[m] = b.band_lo[m] - b.f_lo;
    for (int f = b.band_lo[m]; f < b.band_hi[m]; ++f) {
      q.bin.push_back(f);
      q.pos.push_back(b.bin_pos[f]);
      q.w.push_back(b.csr_w[(size_t)b.csr_ptr[m] + (f - b.band_lo[m])]);
    }
  }
  q.ptr[M] = (int)q.w.size();
  q.n_bins = b.f_hi - b.f_lo;
  q.run.assign(M, 0);
  int longest = 0;
  for (int m = 0; m < M; ++m) {
    q.run[m] = q.ptr[m + 1] - q.ptr[m];
    longest = q.run[m] > longest ? q.run[m] : longest;
  }
  q.wt.assign((size_t)longest * M, 0.f);
  for (int m = 0; m < M; ++m)
    for (int i = 0; i < q.run[m]; ++i) q.wt[(size_t)i * M + m] = q.w[(size_t)q.ptr[m] + i];
  for (int v = 0; v < b.frame_stride / 4; ++v) {
    int at[4];
    float w0[4], w1[4];
    bool any = false;
    for (int e = 0; e < 4; ++e) {
      const int p = 4 * v + e, f = b.pos_bin[p];
      at[e] = 0xffff | (M << 16);
      w0[e] = w1[e] = 0.f;
      if (f < 0 || b.bin_m0[f] < 0 || b.bin_pos[f] != p) continue;
      at[e] = (f - b.f_lo) | (b.bin_m0[f] << 16);
      w0[e] = b.bin_w0[f];
      w1[e] = b.bin_w1[f];
      any = true;
    }
    if (!any) continue;
    q.vec.push_back(v);
    q.vec_at.insert(q.vec_at.end(), at, at + 4);
    q.vec_w0.insert(q.vec_w0.end(), w0, w0 + 4);
    q.vec_w1.insert(q.vec_w1.end(), w1, w1 + 4);
  }
  return q;
}

// everything plan creation derives from a dense filterbank fb [n_stft][n_mels] (n_mels > 0)
inline PlanBank plan_bank(const PlanGeometry& g, int n_mels, const float* fb, const rfx_plan_options& opt, const PlanOverrides& ov) {
  PlanBank b;
  b.F = g.n_stft;
  b.M = n_mels;
  b.generic = g.generic;
  b.frame_stride = g.frame_stride;
  bank_banded_view(b, fb);
  bank_slots(b, fb);
  bank_groups(b);
  bank_sgd_admission(b, opt.imel_form);
  bank_forward_bands(b, fb);
  bank_forward_products(b, fb, ov.fwd_table_form);
  b.adj = mel_adjoint_table(b.F, b.M, fb);
  return b;
}

// ---- backward of the forward path: the position tables of a geometry (no filterbank needed) ----------------------------------------
struct MelBwdTables {
  int sstride = 0;                  // floats per frame of the magnitude slots the MODE 0 frame launch reads
  std::vector<int> pos_bin;         // [sstride]
  std::vector<int> xpos_bin;        // [frame_stride]: the spectrum the forward transform writes
  std::vector<int> s2x;             // [sstride]: position of the spectrum the frame launch multiplies magnitude slot p by
};
inline MelBwdTables mel_bwd_tables(const PlanGeometry& g) {
  MelBwdTables t;
  if (!g.generic) {
    t.sstride = kFrameStride;
    t.pos_bin = mel_bwd_pos_bin_spec();
    t.xpos_bin = mel_bwd_xpos_bin_spec();
    t.s2x = mel_bwd_s2x_spec();
    return t;
  }
  t.xpos_bin = mel_bwd_pos_bin_plain(g.n_stft, g.frame_stride);
  if (g.fam_ok) {
    t.sstride = g.fam.fsf;
    t.pos_bin = fam_bin_of(g.fam);
  } else {
    t.sstride = g.frame_stride;
    t.pos_bin = t.xpos_bin;
  }
  t.s2x = t.pos_bin;  // plain spectrum: position = bin (the row family's launch reads its angles by bin)
  return t;
}

// ---- time stretch (rfx_vocoder.hip): the per-position table of the complex slots, beside MelBwdTables::xpos_bin ---------------------------
// For every position of a frame as rfx_pack_complex lays it out: the bin it holds (-1: padding - the marker), whether it holds the
// bin's conjugate, the PRIMARY position of that bin - the one rfx_unpack_complex reads, so that both slots of a doubled bin are
// computed from the same input and leave as one trajectory - and the bin's advance in turns, frac(hop k / D) with D = 2 (n_stft - 1),
// negated where the position holds the conjugate.  Specialised engine: slot_pos_c order, 440 bins twice; every other engine (row
// family, generic, chirp-z): plain frames, position = bin, no conjugates.
struct VocoderTable {
  std::vector<int> bin, src;        // [frame_stride]; src -1 for padding
  std::vector<float> adv;           // [frame_stride]
  std::vector<unsigned char> conj;  // [frame_stride]
  // the entries the kernel reads (rfx_vocoder_core.h: kVocFlip)
  std::vector<int2> device() const {
    std::vector<int2> t(src.size());
    for (size_t p = 0; p < src.size(); ++p) {
      int32_t bits;
      memcpy(&bits, &adv[p], sizeof(bits));
      t[p] = int2{src[p] < 0 ? -1 : src[p] | (conj[p] != conj[(size_t)src[p]] ? kVocFlip : 0), bits};
    }
    return t;
  }
};
inline VocoderTable vocoder_table(const PlanGeometry& g, int hop) {
  VocoderTable t;
  t.bin = g.generic ? mel_bwd_pos_bin_plain(g.n_stft, g.frame_stride) : mel_bwd_xpos_bin_spec();
  const size_t P = t.bin.size();
  t.src.assign(P, -1);
  t.adv.assign(P, 0.f);
  t.conj.assign(P, 0);
  if (!g.generic)
    for (int q = 0; q < 441; ++q)
      for (int kb = 0; kb < 21; ++kb) {
        bool cj;
        slot_bin(q / 21, q % 21, kb, &cj);
        t.conj[(size_t)slot_pos_c(q, kb)] = cj;
      }
  for (size_t p = 0; p < P; ++p) {
    const int k = t.bin[p];
    if (k < 0) continue;
    t.src[p] = g.generic ? k : voc_spec_primary(k, nullptr);
    const float a = voc_advance_turns(hop, k, g.n_stft);
    t.adv[p] = t.conj[p] ? -a : a;
  }
  return t;
}

}  // namespace rfx
