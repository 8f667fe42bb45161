// rfx_api_plan.hip - the C ABI of librfx.so (include/rfx.h), plan half: the last-error text, plan creation from the host analysis
// of rfx_plan_core.h, destruction and the plan's queries.  No torch types, no exceptions across the boundary.
#include "rfx_api.h"
#include "rfx_plan_core.h"

using namespace rfx;

namespace {
thread_local std::string g_err;

// device copy of a host array, owned by the plan (rfx_plan_destroy frees plan->owned)
template <class D, class T>
hipError_t upload(rfx_plan* plan, D** d_out, const T* src, size_t n) {
  const size_t bytes = n * sizeof(T);
  hipError_t e = hipMalloc((void**)d_out, bytes ? bytes : sizeof(T));
  if (e != hipSuccess) return e;
  plan->owned.push_back(*d_out);
  return bytes ? hipMemcpy(*d_out, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
}
template <class D, class T>
hipError_t upload(rfx_plan* plan, D** d_out, const std::vector<T>& v) {
  return upload(plan, d_out, v.data(), v.size());
}

struct PlanRelease {  // releases the half-built plan if a step of rfx_plan_create_ex fails
  void operator()(rfx_plan* p) const { rfx_plan_destroy(p); }
};
}  // namespace

int rfx::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

const char* rfx_last_error(void) { return g_err.c_str(); }
int rfx_version(void) { return 2; }  // 2: rfx_guided_call_options; rfx_call_options.reserved is checked
int rfx_frame_stride(void) { return kFrameStride; }
int rfx_num_bins(void) { return kBins; }
int rfx_plan_frame_stride(const rfx_plan* plan) { return plan ? plan->frame_stride : 0; }
int rfx_plan_is_generic(const rfx_plan* plan) { return plan && plan->generic ? 1 : 0; }
int rfx_plan_griffinlim_engine(const rfx_plan* plan) { return !plan ? -1 : !plan->generic ? 0 : plan->fam_ok ? 2 : plan->czt ? 3 : 1; }
int rfx_plan_imel_unit_form(const rfx_plan* plan) {
  if (!plan || !plan->d_melfb || !plan->imel_ok || plan->imel_variant != rfx::kImelVariantBest) return 0;
  return plan->imel.unit_form;  // (set for the per-wave and line-form families only: bank_sgd_admission)
}

int rfx_plan_imel_kernel(const rfx_plan* plan) {
  if (!plan || !plan->d_melfb || !plan->imel_ok) return -1;
  return rfx::imel_kernel_choice(plan->imel, plan->p.n_mels, plan->p.max_mel_iters, plan->imel_variant);
}
int rfx_stft_frames(const rfx_plan* plan, int Lw) {
  if (!plan || Lw <= plan->p.n_fft / 2) return 0;
  return stft_frames(plan, Lw);
}
int rfx_griffinlim_output_samples(const rfx_plan* plan, int T) {
  if (!plan || T < 1) return 0;
  return plan->p.hop_length * (T - 1) + (plan->p.n_fft & 1);
}

int rfx_plan_create(const rfx_params* params, const float* h_window, const float* h_melfb, int device,
                    rfx_plan** out_plan) {
  return rfx_plan_create_ex(params, h_window, h_melfb, device, nullptr, out_plan);
}

// Experiment switches (RFX_* environment variables) exist only in builds made with -DRFX_ABLATION (tools/build_variants.sh):
// a release build of librfx.so reads no environment variable at all, rfx_plan_options is its only configuration surface.
static inline const char* abl_env(const char* name) {
#ifdef RFX_ABLATION
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
static int abl_int(const char* name, int unset) {
  const char* e = abl_env(name);
  return e ? atoi(e) : unset;
}
// an override that must be positive: `fallback` for anything else that was given, 0 when the variable is not set
static int abl_positive(const char* name, int fallback) {
  const char* e = abl_env(name);
  return !e ? 0 : atoi(e) > 0 ? atoi(e) : fallback;
}

// rfx_plan_options as the library reads them: defaults, then the caller's (possibly shorter) struct, validated
static int resolve_options(const rfx_plan_options* options, rfx_plan_options* out) {
  rfx_plan_options opt{};
  opt.struct_size = sizeof(rfx_plan_options);
  if (options) {
    if (options->struct_size < 2 * sizeof(uint32_t) || options->struct_size > sizeof(rfx_plan_options))
      return fail(RFX_ERR_INVALID, "rfx_plan_create_ex: options->struct_size does not describe an rfx_plan_options this library knows");
    memcpy(&opt, options, options->struct_size);
    if (opt.gl_form < RFX_GL_FORM_AUTO || opt.gl_form > RFX_GL_FORM_FRAMES || opt.gl_frames_per_slot < 0)
      return fail(RFX_ERR_INVALID, "rfx_plan_create_ex: gl_form must be RFX_GL_FORM_AUTO / _RUNS / _FRAMES, gl_frames_per_slot >= 0");
    if (opt.frame_engine < RFX_ENGINE_AUTO || opt.frame_engine > RFX_ENGINE_CHIRPZ)
      return fail(RFX_ERR_INVALID, "rfx_plan_create_ex: frame_engine must be RFX_ENGINE_AUTO, RFX_ENGINE_GENERIC or RFX_ENGINE_CHIRPZ");
    if (opt.plan_layout < RFX_LAYOUT_AUTO || opt.plan_layout > RFX_LAYOUT_GENERIC)
      return fail(RFX_ERR_INVALID, "rfx_plan_create_ex: plan_layout must be RFX_LAYOUT_AUTO or RFX_LAYOUT_GENERIC");
    if (opt.imel_form < RFX_IMEL_FORM_AUTO || opt.imel_form > RFX_IMEL_FORM_GROUPS)
      return fail(RFX_ERR_INVALID, "rfx_plan_create_ex: imel_form must be RFX_IMEL_FORM_AUTO or RFX_IMEL_FORM_GROUPS");
  }
  *out = opt;
  return RFX_OK;
}

// the overrides that change a decision of rfx_plan_core.h, passed to it as values
static PlanOverrides plan_overrides() {
  PlanOverrides ov;
  ov.gen_threads = abl_int("RFX_GEN_THREADS", 0);
  ov.gen_pad = abl_int("RFX_GEN_PAD", -1);
  ov.fwd_table_form = abl_env("RFX_FWD_V1") != nullptr;
  return ov;
}

int rfx_plan_create_ex(const rfx_params* params, const float* h_window, const float* h_melfb, int device,
                       const rfx_plan_options* options, rfx_plan** out_plan) {
  if (!params || !out_plan || !h_window) return fail(RFX_ERR_INVALID, "rfx_plan_create: null argument");
  // 1, 2: the options, then the geometry and its frame engine (host only)
  rfx_plan_options opt;
  if (const int rc = resolve_options(options, &opt)) return rc;
  const PlanOverrides ov = plan_overrides();
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, ov, &geo, &err)) return fail(rc, err);
  const GenGeom& gg = geo.gg;
  // 3, 4: the device - CU count, per-device kernel attributes (dynamic LDS above 64 KB), occupancy
  RFX_ON_DEVICE(device);
  std::unique_ptr<rfx_plan, PlanRelease> pl(new rfx_plan());
  pl->p = *params;
  pl->device = device;
  pl->n_stft = geo.n_stft;
  pl->generic = geo.generic;
  pl->gg = gg;
  pl->frame_stride = geo.frame_stride;
  pl->gl_form = opt.gl_form;
  hipDeviceProp_t prop;
  RFX_HIP(hipGetDeviceProperties(&prop, device));
  pl->num_cus = prop.multiProcessorCount;
  RFX_HIP(prepare_frame_kernels());
  if (geo.generic && !geo.czt) RFX_HIP(prepare_generic_kernels(gg));
  if (geo.czt) RFX_HIP(prepare_czt_kernels(gg));
  if (geo.czt) RFX_HIP(prepare_czt_list_kernels(gg));
  if (geo.czt) RFX_HIP(prepare_czt_loop_kernels(gg));
  if (geo.czt) RFX_HIP(prepare_czt_zero_kernels(gg));
  if (geo.fam_ok) {
    RFX_HIP(prepare_fam_kernels(geo.fam));
    pl->fam = geo.fam;
    pl->fam_wgs_per_cu = fam_blocks_per_cu(geo.fam);
  }
  pl->gl_wgs_per_cu = gl_blocks_per_cu();
  // 5: the remaining ablation overrides, read here, once, never on the hot calls.  The Griffin-Lim form a call takes is decided by
  // the options; the environment only changes what RFX_GL_FORM_AUTO / the default threshold mean
  if (const int v = abl_positive("RFX_FAM_WGS_PER_CU", 1)) pl->fam_wgs_per_cu = v;
  if (const int v = abl_positive("RFX_GL_WGS_PER_CU", 1)) pl->gl_wgs_per_cu = v;
  pl->imel_variant = abl_env("RFX_IMEL_GENERAL") ? rfx::kImelVariantGeneral : abl_env("RFX_IMEL_UNIFORM") ? rfx::kImelVariantUniform : rfx::kImelVariantBest;
  pl->gl_latency_mode = abl_int("RFX_GL_LATENCY_MODE", 1) != 0;
  if (const int v = abl_positive("RFX_GL_LATENCY_FRAMES", 6)) pl->gl_latency_frames_per_slot = v;
  if (opt.gl_frames_per_slot > 0) pl->gl_latency_frames_per_slot = opt.gl_frames_per_slot;
  const bool fwd_unfused = abl_env("RFX_FWD_UNFUSED") != nullptr;
  const int fwd_run_cap = abl_positive("RFX_FWD_RUN", 64), fwd_run_skew = abl_int("RFX_FWD_SKEW", pl->fwd_run_skew);
#if defined(RFX_TIMING) || defined(RFX_WGCLOCK)
  if (const char* e = getenv("RFX_TIMING_PTR")) pl->timing = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
  // 6: window and twiddles of the engines this plan runs on
  RFX_HIP(upload(pl.get(), &pl->d_tw1, spec_twiddles1()));
  RFX_HIP(upload(pl.get(), &pl->d_tw2, spec_twiddles2()));
  RFX_HIP(upload(pl.get(), &pl->d_win, h_window, (size_t)params->win_length));
  if (geo.czt) {  // the passes' tables at the convolution length, the chirp and H; no digit-reversal table: the result is in natural order
    const CztPlanTables ct = czt_plan_tables(gg);
    RFX_HIP(upload(pl.get(), &pl->d_gen_tables, ct.two_level));
    RFX_HIP(upload(pl.get(), &pl->d_gen_tw, ct.pass_tw));
    RFX_HIP(upload(pl.get(), &pl->d_czt_c, ct.c));
    RFX_HIP(upload(pl.get(), &pl->d_czt_h, ct.h));
    pl->czt = true;
  } else if (geo.generic) {
    RFX_HIP(upload(pl.get(), &pl->d_gen_tables, gen_two_level_twiddles(gg)));
    RFX_HIP(upload(pl.get(), &pl->d_gen_rev, gen_rev_table(gg)));
    RFX_HIP(upload(pl.get(), &pl->d_gen_tw, gen_pass_twiddles(gg)));
  }
  if (geo.generic) {
    cf* d = (cf*)pl->d_gen_tables;
    pl->gt.lo = d;
    pl->gt.hi = d + kGenTwLo;
    pl->gt.lo2 = d + kGenTwLo + gg.nhi;
    pl->gt.hi2 = d + 2 * kGenTwLo + gg.nhi;
    pl->gt.win = pl->d_win;
    pl->gt.rev = pl->d_gen_rev;
    pl->gt.tw = pl->d_gen_tw;
  }
  if (geo.fam_ok) {
    RFX_HIP(upload(pl.get(), &pl->d_fam_tw, fam_twiddles(geo.fam)));
    RFX_HIP(upload(pl.get(), &pl->d_fam_binof, fam_bin_of(geo.fam)));
    pl->fam_ok = true;
  }
  {  // the position tables of the backward entries (rfx_mel_bwd.hip)
    const MelBwdTables mb = mel_bwd_tables(geo);
    pl->mb_sstride = mb.sstride;
    RFX_HIP(upload(pl.get(), &pl->d_mb_pos_bin, mb.pos_bin));
    RFX_HIP(upload(pl.get(), &pl->d_mb_xpos_bin, mb.xpos_bin));
    RFX_HIP(upload(pl.get(), &pl->d_mb_s2x, mb.s2x));
    RFX_HIP(upload(pl.get(), &pl->d_voc_table, vocoder_table(geo, params->hop_length).device()));
  }
  if (h_melfb) {
    const int F = geo.n_stft, M = params->n_mels;
    if (M <= 0) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive");
    // 7: everything the filterbank decides (host only)
    const PlanBank bank = plan_bank(geo, M, h_melfb, opt, ov);
    // 8: upload
    if (M > 32767) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be below 32768");
    RFX_HIP(upload(pl.get(), &pl->d_melfb, h_melfb, (size_t)F * M));
    RFX_HIP(upload(pl.get(), &pl->d_bin_bands, bin_bands(F, M, h_melfb)));
    RFX_HIP(upload(pl.get(), &pl->d_mb_first, bank.adj.first));
    RFX_HIP(upload(pl.get(), &pl->d_mb_count, bank.adj.count));
    RFX_HIP(upload(pl.get(), &pl->d_mb_wt, bank.adj.wt));
    pl->mb_width = bank.adj.width;
    if (!geo.generic) {
      RFX_HIP(upload(pl.get(), &pl->d_melfb_slots, bank.fbs));
      RFX_HIP(upload(pl.get(), &pl->d_kblocks, bank.kblocks));
    }
    if (bank.fwd_ok) {
      RFX_HIP(upload(pl.get(), &pl->d_band_wt, bank.wt));
      if (!geo.generic) RFX_HIP(upload(pl.get(), &pl->d_band_addr, bank.addr));
      RFX_HIP(upload(pl.get(), &pl->d_band_lo, bank.lo_len));
    }
    if (bank.prod_ok) {  // d_slot_idx: padtab | seg | tab_at | packed tables
      std::vector<int> idx(bank.padtab);
      idx.insert(idx.end(), bank.seg.begin(), bank.seg.end());
      idx.insert(idx.end(), bank.tab_at.begin(), bank.tab_at.end());
      if (bank.packed) pl->fwd_packed_off = (int)idx.size();
      idx.insert(idx.end(), bank.pk.begin(), bank.pk.end());
      RFX_HIP(upload(pl.get(), &pl->d_slot_tab, bank.tab));
      RFX_HIP(upload(pl.get(), &pl->d_slot_idx, idx));
    }
    // 9: the plan's fields
    pl->melfb_cols = bank.melfb_cols;
    pl->n_kblocks = (int)bank.kblocks.size();
    pl->imel_ok = bank.ok;
    pl->imel_why = bank.why;
    pl->fwd_ok = bank.fwd_ok;
    pl->band_rows = bank.band_rows;
    pl->Mpad = bank.Mpad;
    if (bank.prod_ok) {
      pl->fwd_kb_mask = bank.mask;
      pl->fwd_prod_arr = bank.arr;
    }
    if (bank.fwd_ok) {
      pl->fwd_unfused = fwd_unfused;
      if (fwd_run_cap) pl->fwd_run_cap = fwd_run_cap;
      pl->fwd_run_skew = fwd_run_skew;
    }
    if (bank.ok) {
      // one device blob, every table on a 256-byte boundary: csr_w | csr_ptr | band_lo | bin_m0 | bin_w0 | bin_w1 | bin_pos | bin_pos2 |
      // grp_start | lin (zeros unless a group kernel reads it) | pos_bin
      std::vector<char> blob;
      auto put = [&](const void* src, size_t bytes, size_t copy) {
        const size_t o = blob.size();
        blob.resize(o + align_up(bytes, 256), 0);
        if (copy) memcpy(&blob[o], src, copy);
        return o;
      };
      auto ints = [&](const std::vector<int>& v, size_t n) { return put(v.data(), n * 4, n * 4); };
      auto floats = [&](const std::vector<float>& v, size_t n) { return put(v.data(), n * 4, n * 4); };
      const size_t o_w = floats(bank.csr_w, bank.csr_w.size()), o_ptr = ints(bank.csr_ptr, M + 1), o_lo = ints(bank.band_lo, M),
                   o_m0 = ints(bank.bin_m0, F), o_w0 = floats(bank.bin_w0, F), o_w1 = floats(bank.bin_w1, F), o_p = ints(bank.bin_pos, F),
                   o_p2 = ints(bank.bin_pos2, F), o_gs = ints(bank.grp_start, M + 1),
                   o_lin = put(bank.lin.data(), 4 * (size_t)M * 4, bank.imel.fast_ok ? 4 * (size_t)M * 4 : 0),
                   o_pb = ints(bank.pos_bin, bank.pos_bin.size());
      RFX_HIP(upload(pl.get(), &pl->d_imel_blob, blob));
      const char* d = (const char*)pl->d_imel_blob;
      pl->imel = bank.imel;
      pl->imel.csr_w = (const float*)(d + o_w);
      pl->imel.csr_ptr = (const int*)(d + o_ptr);
      pl->imel.band_lo = (const int*)(d + o_lo);
      pl->imel.bin_m0 = (const int*)(d + o_m0);
      pl->imel.bin_w0 = (const float*)(d + o_w0);
      pl->imel.bin_w1 = (const float*)(d + o_w1);
      pl->imel.bin_pos = (const int*)(d + o_p);
      pl->imel.bin_pos2 = (const int*)(d + o_p2);
      pl->imel.pos_bin = (const int*)(d + o_pb);
      pl->imel.grp_start = (const int*)(d + o_gs);
      pl->imel.lin = (const float*)(d + o_lin);
    }
    // closed-form InverseMelScale: the factor tables, only for a bank that admits them (rfx_plan_lstsq_ok)
    const LstsqBank lsq = bank_lstsq(bank);
    pl->lstsq_ok = lsq.ok;
    pl->lstsq_why = lsq.why;
    if (lsq.ok) {
      float *d_nl, *d_inv_d, *d_w0, *d_w1;
      int* d_m0;
      RFX_HIP(upload(pl.get(), &d_nl, lsq.nl));
      RFX_HIP(upload(pl.get(), &d_inv_d, lsq.inv_d));
      RFX_HIP(upload(pl.get(), &d_m0, lsq.pos_m0));
      RFX_HIP(upload(pl.get(), &d_w0, lsq.pos_w0));
      RFX_HIP(upload(pl.get(), &d_w1, lsq.pos_w1));
      pl->lstsq = LsqTables{d_nl, d_inv_d, d_m0, d_w0, d_w1};
      // ... and the lists its backward's collect walks
      const LstsqCollect col = bank_lstsq_collect(bank);
      int *d_run, *d_first, *d_vec, *d_at;
      float *d_wt, *d_vw0, *d_vw1;
      RFX_HIP(upload(pl.get(), &d_wt, col.wt));
      RFX_HIP(upload(pl.get(), &d_first, col.first));
      RFX_HIP(upload(pl.get(), &d_run, col.run));
      RFX_HIP(upload(pl.get(), &d_vec, col.vec));
      RFX_HIP(upload(pl.get(), &d_at, col.vec_at));
      RFX_HIP(upload(pl.get(), &d_vw0, col.vec_w0));
      RFX_HIP(upload(pl.get(), &d_vw1, col.vec_w1));
      pl->lstsq_collect = LsqCollectTables{d_wt, d_first, d_run, d_vec, d_at, d_vw0, d_vw1, (int)col.vec.size(), col.n_bins};
    }
  } else {
    pl->lstsq_why = "plan was created without a mel filterbank";
  }
  *out_plan = pl.release();
  return RFX_OK;
}

int rfx_plan_lstsq_ok(const rfx_plan* plan) { return plan && plan->lstsq_ok ? 1 : 0; }

int rfx_debug_lstsq_bank(const rfx_params* params, const float* h_melfb, rfx_lstsq_bank_report* report) {
  if (!params || !h_melfb || !report) return fail(RFX_ERR_INVALID, "rfx_debug_lstsq_bank: null argument");
  if (report->struct_size < 2 * sizeof(uint32_t) || report->struct_size > sizeof(rfx_lstsq_bank_report))
    return fail(RFX_ERR_INVALID, "rfx_debug_lstsq_bank: report->struct_size does not describe an rfx_lstsq_bank_report this library knows");
  if (params->n_mels <= 0) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive");
  rfx_plan_options opt;
  if (const int rc = resolve_options(nullptr, &opt)) return rc;
  const PlanOverrides ov = plan_overrides();
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, ov, &geo, &err)) return fail(rc, err);
  const LstsqBank lsq = bank_lstsq(plan_bank(geo, params->n_mels, h_melfb, opt, ov));
  rfx_lstsq_bank_report r{};
  memcpy(&r, report, report->struct_size);  // (the caller's table pointers)
  r.ok = lsq.ok;
  r.min_pivot = lsq.min_pivot;
  r.min_pivot_ratio = lsq.min_pivot_ratio;
  snprintf(r.why, sizeof(r.why), "%s", lsq.why.c_str());
  if (lsq.ok && r.h_neg_l) memcpy(r.h_neg_l, lsq.nl.data(), lsq.nl.size() * sizeof(float));
  if (lsq.ok && r.h_inv_d) memcpy(r.h_inv_d, lsq.inv_d.data(), lsq.inv_d.size() * sizeof(float));
  memcpy(report, &r, r.struct_size);
  return RFX_OK;
}

int rfx_debug_lstsq_collect(const rfx_params* params, const float* h_melfb, int32_t* h_ptr, int32_t* h_bin, int32_t* h_pos, float* h_weight,
                            int capacity, int32_t* entries_out) {
  if (!params || !h_melfb || !entries_out) return fail(RFX_ERR_INVALID, "rfx_debug_lstsq_collect: null argument");
  if (params->n_mels <= 0) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive");
  rfx_plan_options opt;
  if (const int rc = resolve_options(nullptr, &opt)) return rc;
  const PlanOverrides ov = plan_overrides();
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, ov, &geo, &err)) return fail(rc, err);
  const PlanBank bank = plan_bank(geo, params->n_mels, h_melfb, opt, ov);
  const LstsqBank lsq = bank_lstsq(bank);
  if (!lsq.ok) return fail(RFX_ERR_INVALID, "rfx_debug_lstsq_collect: the closed-form InverseMelScale does not serve this filterbank: " + lsq.why);
  const LstsqCollect col = bank_lstsq_collect(bank);  // what plan creation uploads
  const int n = (int)col.w.size();
  *entries_out = n;
  if (h_ptr) memcpy(h_ptr, col.ptr.data(), col.ptr.size() * sizeof(int32_t));
  if (h_bin || h_pos || h_weight) {
    if (capacity < n)
      return fail(RFX_ERR_INVALID, "rfx_debug_lstsq_collect: the lists have " + std::to_string(n) + " entries, capacity is " + std::to_string(capacity));
    if (h_bin) memcpy(h_bin, col.bin.data(), (size_t)n * sizeof(int32_t));
    if (h_pos) memcpy(h_pos, col.pos.data(), (size_t)n * sizeof(int32_t));
    if (h_weight) memcpy(h_weight, col.w.data(), (size_t)n * sizeof(float));
  }
  return RFX_OK;
}

int rfx_debug_guide_project_tables(const rfx_params* params, int32_t* h_xpos_bin, int32_t* h_s2x, int capacity, int32_t* stride_out) {
  if (!params || !stride_out) return fail(RFX_ERR_INVALID, "rfx_debug_guide_project_tables: null argument");
  rfx_plan_options opt;
  if (const int rc = resolve_options(nullptr, &opt)) return rc;
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, plan_overrides(), &geo, &err)) return fail(rc, err);
  const MelBwdTables mb = mel_bwd_tables(geo);
  const std::vector<int>& s2x = geo.generic ? mb.xpos_bin : mb.s2x;  // (plain frames: a magnitude position is its bin's spectrum position)
  const int n = (int)mb.xpos_bin.size();
  *stride_out = n;
  if (h_xpos_bin || h_s2x) {
    if (capacity < n)
      return fail(RFX_ERR_INVALID, "rfx_debug_guide_project_tables: a frame has " + std::to_string(n) + " positions, capacity is " + std::to_string(capacity));
    if (h_xpos_bin) memcpy(h_xpos_bin, mb.xpos_bin.data(), (size_t)n * sizeof(int32_t));
    if (h_s2x) memcpy(h_s2x, s2x.data(), (size_t)n * sizeof(int32_t));
  }
  return RFX_OK;
}

int rfx_debug_vocoder_table(const rfx_params* params, const rfx_plan_options* options, int32_t* h_bin, int32_t* h_src, float* h_advance,
                            uint8_t* h_conj, int capacity, int32_t* stride_out) {
  if (!params || !stride_out) return fail(RFX_ERR_INVALID, "rfx_debug_vocoder_table: null argument");
  rfx_plan_options opt;
  if (const int rc = resolve_options(options, &opt)) return rc;
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, plan_overrides(), &geo, &err)) return fail(rc, err);
  const VocoderTable t = vocoder_table(geo, params->hop_length);  // what plan creation uploads
  const int n = (int)t.src.size();
  *stride_out = n;
  if (h_bin || h_src || h_advance || h_conj) {
    if (capacity < n)
      return fail(RFX_ERR_INVALID, "rfx_debug_vocoder_table: a frame has " + std::to_string(n) + " positions, capacity is " + std::to_string(capacity));
    if (h_bin) memcpy(h_bin, t.bin.data(), (size_t)n * sizeof(int32_t));
    if (h_src) memcpy(h_src, t.src.data(), (size_t)n * sizeof(int32_t));
    if (h_advance) memcpy(h_advance, t.adv.data(), (size_t)n * sizeof(float));
    if (h_conj) memcpy(h_conj, t.conj.data(), (size_t)n);
  }
  return RFX_OK;
}

int rfx_hold_mask_words(const rfx_plan* plan) { return plan ? (plan->n_stft + 31) / 32 : 0; }

int rfx_debug_bin_bands(const rfx_params* params, const float* h_melfb, int16_t* lo, int16_t* hi) {
  if (!params || !h_melfb || !lo || !hi) return fail(RFX_ERR_INVALID, "rfx_debug_bin_bands: null argument");
  if (params->n_mels <= 0 || params->n_mels > 32767) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive and below 32768");
  rfx_plan_options opt;
  if (const int rc = resolve_options(nullptr, &opt)) return rc;
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, plan_overrides(), &geo, &err)) return fail(rc, err);
  const std::vector<int16_t> v = bin_bands(geo.n_stft, params->n_mels, h_melfb);
  memcpy(lo, v.data(), (size_t)geo.n_stft * sizeof(int16_t));
  memcpy(hi, v.data() + geo.n_stft, (size_t)geo.n_stft * sizeof(int16_t));
  return RFX_OK;
}

int rfx_debug_mel_adjoint(const rfx_params* params, const float* h_melfb, int32_t* h_first, int32_t* h_count, float* h_weights, int capacity,
                           int32_t* width_out) {
  if (!params || !h_melfb || !width_out) return fail(RFX_ERR_INVALID, "rfx_debug_mel_adjoint: null argument");
  if (params->n_mels <= 0 || params->n_fft < 2) return fail(RFX_ERR_INVALID, "rfx_debug_mel_adjoint: n_mels and n_fft must be positive");
  const int F = params->n_fft / 2 + 1;
  const MelAdjoint adj = mel_adjoint_table(F, params->n_mels, h_melfb);  // what plan_bank keeps as PlanBank::adj
  *width_out = adj.width;
  if (h_first) memcpy(h_first, adj.first.data(), (size_t)F * sizeof(int32_t));
  if (h_count) memcpy(h_count, adj.count.data(), (size_t)F * sizeof(int32_t));
  if (h_weights) {
    if (capacity < adj.width)
      return fail(RFX_ERR_INVALID, "rfx_debug_mel_adjoint: the table has " + std::to_string(adj.width) + " weights per bin, capacity is " + std::to_string(capacity));
    for (int k = 0; k < F; ++k)
      for (int i = 0; i < capacity; ++i) h_weights[(size_t)k * capacity + i] = i < adj.width ? adj.wt[(size_t)k * adj.width + i] : 0.f;
  }
  return RFX_OK;
}

int rfx_debug_plan_bank(const rfx_params* params, const float* h_melfb, const rfx_plan_options* options, rfx_plan_bank_report* report) {
  if (!params || !report) return fail(RFX_ERR_INVALID, "rfx_debug_plan_bank: null argument");
  if (report->struct_size < 2 * sizeof(uint32_t) || report->struct_size > sizeof(rfx_plan_bank_report))
    return fail(RFX_ERR_INVALID, "rfx_debug_plan_bank: report->struct_size does not describe an rfx_plan_bank_report this library knows");
  rfx_plan_options opt;
  if (const int rc = resolve_options(options, &opt)) return rc;
  const PlanOverrides ov = plan_overrides();
  PlanGeometry geo;
  std::string err;
  if (const int rc = plan_geometry(*params, opt, ov, &geo, &err)) return fail(rc, err);
  rfx_plan_bank_report r{};
  r.struct_size = report->struct_size;
  r.engine = geo.engine();
  r.frame_stride = geo.frame_stride;
  r.imel_kernel = -1;
  r.line_tolerance = kImelLineTol;
  r.line_deviation = -1.0;
  if (geo.generic) {
    r.fft_length = geo.gg.nc;
    r.pass_length = geo.gg.np;
  }
  if (geo.czt) {
    const CztPlanTables ct = czt_plan_tables(geo.gg);
    r.czt_chirp_elems = (int32_t)ct.c.size();
    r.czt_h_elems = (int32_t)ct.h.size();
  }
  if (h_melfb) {
    if (params->n_mels <= 0) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive");
    const PlanBank bank = plan_bank(geo, params->n_mels, h_melfb, opt, ov);
    r.imel_ok = bank.ok;
    snprintf(r.imel_why, sizeof(r.imel_why), "%s", bank.why.c_str());
    if (bank.ok) r.imel_kernel = rfx::imel_kernel_choice(bank.imel, params->n_mels, params->max_mel_iters, rfx::kImelVariantBest);
    r.fast_ok = bank.imel.fast_ok;
    r.unit_form = bank.imel.unit_form;
    r.wave_ok = bank.imel.wave_ok;
    r.line_from = bank.imel.line_from;
    r.f_lo = bank.imel.f_lo;
    r.f_hi = bank.imel.f_hi;
    r.nnz = bank.imel.nnz;
    r.fwd_ok = bank.fwd_ok;
    r.fwd_product = bank.prod_ok;
    r.fwd_packed = bank.packed;
    r.fwd_kb_mask = bank.mask;
    r.fwd_prod_arr = bank.arr;
    r.band_rows = bank.band_rows;
    r.Mpad = bank.Mpad;
    r.n_kblocks = (int32_t)bank.kblocks.size();
    r.line_deviation = bank.line_dev;
  }
  memcpy(report, &r, r.struct_size);
  return RFX_OK;
}

int rfx_plan_destroy(rfx_plan* plan) {
  if (!plan) return RFX_OK;
  {
    DeviceGuard guard(plan->device);
    for (void* d : plan->owned) (void)hipFree(d);
  }
  delete plan;
  return RFX_OK;
}
