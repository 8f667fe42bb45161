// rfx_api.hip - the C ABI of librfx.so (include/rfx.h): plan construction and the host-side drivers
// that sequence the gfx950 kernels.  No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/rfx.h"
#include "rfx_kernels.h"
#include "rfx_compress_core.h"
#include "rfx_pcm_core.h"
#include "rfx_plan_core.h"
#include "rfx_resize_core.h"

using namespace rfx;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define RFX_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return fail(RFX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// device copy of a host array: every allocation of plan creation (the plan's destructor frees them)
template <class D, class T>
hipError_t upload(D** d_out, const T* src, size_t n) {
  const size_t bytes = n * sizeof(T);
  hipError_t e = hipMalloc((void**)d_out, bytes ? bytes : sizeof(T));
  if (e == hipSuccess && bytes) e = hipMemcpy(*d_out, src, bytes, hipMemcpyHostToDevice);
  return e;
}
template <class D, class T>
hipError_t upload(D** d_out, const std::vector<T>& v) {
  return upload(d_out, v.data(), v.size());
}

struct PlanRelease {  // releases the half-built plan if a step of rfx_plan_create_ex fails
  void operator()(rfx_plan* p) const { rfx_plan_destroy(p); }
};

// Every entry point runs on the device that owns its plan (or its buffers) and leaves the calling thread's
// current device as it found it: torch tracks the current device per thread, and one process may hold plans
// on several GPUs.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) {
      err = hipSetDevice(device);
      switched = err == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define RFX_ON_DEVICE(dev)   \
  DeviceGuard guard_((dev)); \
  if (guard_.err != hipSuccess) return fail(RFX_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// device that owns a caller buffer (the codec entry points take no plan)
int device_of(const void* d_ptr, int* device) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, d_ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(RFX_ERR_INVALID, std::string("not a device pointer: ") + hipGetErrorString(e));
  }
  *device = attr.device;
  return RFX_OK;
}

// HIP events of the timed Griffin-Lim entry point; released on every exit path
struct EventList {
  std::vector<hipEvent_t> ev;
  ~EventList() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  hipError_t create(size_t n) {
    ev.reserve(n);
    for (size_t i = 0; i < n; ++i) {
      hipEvent_t e;
      const hipError_t rc = hipEventCreate(&e);
      if (rc != hipSuccess) return rc;
      ev.push_back(e);
    }
    return hipSuccess;
  }
};
}  // namespace

#ifndef RFX_FWD_RUN_SKEW
#define RFX_FWD_RUN_SKEW 170  // per mille: 74 / 54 frames instead of 64 / 64; -4.3 % on the forward kernel (profiles/r06_forward_skew.txt)
#endif

struct rfx_plan {
  rfx_params p;
  int device;
  int num_cus;
  int n_stft;
  int gl_wgs_per_cu = 1;    // resident Griffin-Lim workgroups per CU on this device (occupancy query at creation)
  int imel_variant = 0;     // debugging override read once at creation: 0 = best, 1 = uniform groups, 2 = general, 3 = best one-frame kernel
  unsigned long long* timing = nullptr;  // RFX_TIMING builds only
  cf* d_tw1 = nullptr;      // [21][441]
  cf* d_tw2 = nullptr;      // [21][21]
  float* d_win = nullptr;   // [4410]
  float* d_melfb_slots = nullptr;  // [kFrameStride][n_mels]: filterbank rows permuted to slot order
  float* d_melfb = nullptr;        // [n_stft][n_mels] as given
  int* d_kblocks = nullptr;        // non-zero 32-position K blocks of d_melfb_slots
  int n_kblocks = 0;
  int melfb_cols = 0;              // columns of d_melfb_slots (n_mels rounded up to 128)
  // banded view of the filterbank for InverseMelScale (valid when imel_ok)
  bool imel_ok = false;
  std::string imel_why;
  ImelTables imel{};
  void* d_imel_blob = nullptr;
  // fused forward path (banded mel projection inside the STFT kernel), valid when fwd_ok
  bool fwd_ok = false;
  float* d_band_wt = nullptr;      // [band_rows][Mpad]
  int* d_band_addr = nullptr;      // [band_rows][Mpad] LDS position of each band bin (specialised engine)
  int* d_band_lo = nullptr;        // [Mpad] followed by band_len [Mpad]
  int band_rows = 0, Mpad = 0;
  bool fwd_unfused = false;        // debugging override (RFX_FWD_UNFUSED), read once at creation
  void* d_slot_tab = nullptr;      // product form of the fused kernel: [21][kQPad] {w0, w1} per slot ...
  int* d_slot_idx = nullptr;       // ... [kMelPadsPerThread][kQPad] padding positions, [2][Mpad] filter segments, [21][kQPad] product positions; null: table form
  unsigned fwd_kb_mask = 0;
  int fwd_prod_arr = 0;
  int fwd_packed_off = 0;          // ints into d_slot_idx where the packed tables start (0: none)
  int fwd_run_skew = RFX_FWD_RUN_SKEW;  // per mille of the run length the first-dispatched workgroups of the forward kernel take on top (RFX_FWD_SKEW in ablation builds)
  int fwd_run_cap = 64;            // longest run of frames one workgroup of the product-form kernel walks (RFX_FWD_RUN, read at creation)
  // generic-geometry path (rfx_generic.hip): everything but n_fft = 17640 / win = 4410 / hop = 441
  bool gl_latency_mode = true;     // small batches use the per-frame Griffin-Lim kernels (RFX_GL_LATENCY_MODE=0 disables, in ablation builds)
  int gl_latency_frames_per_slot = 6;  // ... up to this many frames per resident workgroup slot (RFX_GL_LATENCY_FRAMES).  4 until round 6;
                                       // runs are whole groups of 16 frames now, so the run form costs a batch below nine tiles what it costs
                                       // eight (3.4 - 3.7 ms per Griffin-Lim 32) and the per-frame form, linear in the batch, wins up to six
                                       // tiles (3.2 ms): profiles/r06_griffinlim_forms_by_batch.txt
  int gl_form = RFX_GL_FORM_AUTO;      // rfx_plan_options.gl_form
  bool generic = false;
  GenGeom gg{};
  GenTables gt{};
  void* d_gen_tables = nullptr;
  int* d_gen_rev = nullptr;
  cf* d_gen_tw = nullptr;
  int frame_stride = kFrameStride;
  // row-family Griffin-Lim (rfx_fam.hip) on top of a generic plan: n_fft = 40 h, win_length = 10 h
  bool fam_ok = false;
  FamGeom fam{};
  cf* d_fam_tw = nullptr;      // [21][h] g(n')^k1, then [rb][ra-1] W_h^{i p}
  int* d_fam_binof = nullptr;  // [fsf] bin held by each position of the slot-ordered magnitudes (-1: padding)
  int fam_wgs_per_cu = 1;
};

namespace rfx {
__global__ void out_scale_kernel(const float* __restrict__ win, float* __restrict__ out, int T, int L) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= L) return;
  // frames t with 0 <= p - 441 t + 2205 < 4410
  int tlo = (p + 2205 - (kWin - 1) + kHop - 1) / kHop;  // ceil, numerator may be negative
  if (p + 2205 - (kWin - 1) < 0) tlo = 0;
  int thi = (p + 2205) / kHop;
  if (thi > T - 1) thi = T - 1;
  float env = 0.f;
  for (int t = tlo; t <= thi; ++t) {
    const float w = win[p - kHop * t + 2205];
    env = fmaf(w, w, env);
  }
  out[p] = (2.0f / (float)kNfft) / env;
}
}  // namespace rfx

extern "C" {

const char* rfx_last_error(void) { return g_err.c_str(); }
int rfx_version(void) { return 1; }
int rfx_frame_stride(void) { return kFrameStride; }
int rfx_num_bins(void) { return kBins; }
int rfx_plan_frame_stride(const rfx_plan* plan) { return plan ? plan->frame_stride : 0; }
int rfx_plan_is_generic(const rfx_plan* plan) { return plan && plan->generic ? 1 : 0; }
int rfx_plan_griffinlim_engine(const rfx_plan* plan) { return !plan ? -1 : !plan->generic ? 0 : plan->fam_ok ? 2 : 1; }
int rfx_griffinlim_form(const rfx_plan* plan, int B, int T);
int rfx_plan_imel_unit_form(const rfx_plan* plan) {
  if (!plan || !plan->d_melfb || !plan->imel_ok || (plan->imel_variant != 0 && plan->imel_variant != 3)) return 0;
  return plan->imel.fast_ok >= 2 ? plan->imel.unit_form : 0;
}

int rfx_plan_imel_kernel(const rfx_plan* plan) {
  if (!plan || !plan->d_melfb || !plan->imel_ok) return -1;
  return rfx::imel_kernel_choice(plan->imel, plan->p.n_mels, plan->p.max_mel_iters, plan->imel_variant);
}
// torch.stft(center=True): the signal is reflect-padded by n_fft/2 on both sides, so a waveform of Lw samples gives
// 1 + (Lw + 2*(n_fft/2) - n_fft) / hop frames: 1 + Lw/hop for even n_fft, 1 + (Lw - 1)/hop for odd n_fft
static int stft_frames(const rfx_plan* plan, int Lw) {
  return 1 + (Lw + 2 * (plan->p.n_fft / 2) - plan->p.n_fft) / plan->p.hop_length;
}
int rfx_stft_frames(const rfx_plan* plan, int Lw) {
  if (!plan || Lw <= plan->p.n_fft / 2) return 0;
  return stft_frames(plan, Lw);
}
int rfx_griffinlim_output_samples(const rfx_plan* plan, int T) {
  if (!plan || T < 1) return 0;
  return plan->p.hop_length * (T - 1) + (plan->p.n_fft & 1);
}

int rfx_plan_destroy(rfx_plan* plan);

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
    if (opt.frame_engine < RFX_ENGINE_AUTO || opt.frame_engine > RFX_ENGINE_GENERIC)
      return fail(RFX_ERR_INVALID, "rfx_plan_create_ex: frame_engine must be RFX_ENGINE_AUTO or RFX_ENGINE_GENERIC");
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
  if (geo.generic) RFX_HIP(prepare_generic_kernels(gg));
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
  pl->imel_variant = abl_env("RFX_IMEL_GENERAL") ? 2 : abl_env("RFX_IMEL_UNIFORM") ? 1 : abl_env("RFX_IMEL_NO_PAIR") ? 3 : 0;  // 3: best one-frame kernel
  pl->gl_latency_mode = abl_int("RFX_GL_LATENCY_MODE", 1) != 0;
  if (const int v = abl_positive("RFX_GL_LATENCY_FRAMES", 6)) pl->gl_latency_frames_per_slot = v;
  if (opt.gl_frames_per_slot > 0) pl->gl_latency_frames_per_slot = opt.gl_frames_per_slot;
  const bool fwd_unfused = abl_env("RFX_FWD_UNFUSED") != nullptr;
  const int fwd_run_cap = abl_positive("RFX_FWD_RUN", 64), fwd_run_skew = abl_int("RFX_FWD_SKEW", pl->fwd_run_skew);
#if defined(RFX_TIMING) || defined(RFX_WGCLOCK)
  if (const char* e = getenv("RFX_TIMING_PTR")) pl->timing = (unsigned long long*)strtoull(e, nullptr, 0);
#endif
  // 6: window and twiddles of the engines this plan runs on
  RFX_HIP(upload(&pl->d_tw1, spec_twiddles1()));
  RFX_HIP(upload(&pl->d_tw2, spec_twiddles2()));
  RFX_HIP(upload(&pl->d_win, h_window, (size_t)params->win_length));
  if (geo.generic) {
    RFX_HIP(upload(&pl->d_gen_tables, gen_two_level_twiddles(gg)));
    RFX_HIP(upload(&pl->d_gen_rev, gen_rev_table(gg)));
    RFX_HIP(upload(&pl->d_gen_tw, gen_pass_twiddles(gg)));
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
    RFX_HIP(upload(&pl->d_fam_tw, fam_twiddles(geo.fam)));
    RFX_HIP(upload(&pl->d_fam_binof, fam_bin_of(geo.fam)));
    pl->fam_ok = true;
  }
  if (h_melfb) {
    const int F = geo.n_stft, M = params->n_mels;
    if (M <= 0) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive");
    // 7: everything the filterbank decides (host only)
    const PlanBank bank = plan_bank(geo, M, h_melfb, opt, ov);
    // 8: upload
    RFX_HIP(upload(&pl->d_melfb, h_melfb, (size_t)F * M));
    if (!geo.generic) {
      RFX_HIP(upload(&pl->d_melfb_slots, bank.fbs));
      RFX_HIP(upload(&pl->d_kblocks, bank.kblocks));
    }
    if (bank.fwd_ok) {
      RFX_HIP(upload(&pl->d_band_wt, bank.wt));
      if (!geo.generic) RFX_HIP(upload(&pl->d_band_addr, bank.addr));
      RFX_HIP(upload(&pl->d_band_lo, bank.lo_len));
    }
    if (bank.prod_ok) {  // d_slot_idx: padtab | seg | tab_at | packed tables
      std::vector<int> idx(bank.padtab);
      idx.insert(idx.end(), bank.seg.begin(), bank.seg.end());
      idx.insert(idx.end(), bank.tab_at.begin(), bank.tab_at.end());
      if (bank.packed) pl->fwd_packed_off = (int)idx.size();
      idx.insert(idx.end(), bank.pk.begin(), bank.pk.end());
      RFX_HIP(upload(&pl->d_slot_tab, bank.tab));
      RFX_HIP(upload(&pl->d_slot_idx, idx));
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
      RFX_HIP(upload(&pl->d_imel_blob, blob));
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
  }
  *out_plan = pl.release();
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
  if (h_melfb) {
    if (params->n_mels <= 0) return fail(RFX_ERR_INVALID, "rfx_plan_create: n_mels must be positive");
    const PlanBank bank = plan_bank(geo, params->n_mels, h_melfb, opt, ov);
    r.imel_ok = bank.ok;
    snprintf(r.imel_why, sizeof(r.imel_why), "%s", bank.why.c_str());
    if (bank.ok) r.imel_kernel = rfx::imel_kernel_choice(bank.imel, params->n_mels, params->max_mel_iters, 0);
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
    (void)hipFree(plan->d_tw1);
    (void)hipFree(plan->d_tw2);
    (void)hipFree(plan->d_win);
    (void)hipFree(plan->d_melfb);
    (void)hipFree(plan->d_melfb_slots);
    (void)hipFree(plan->d_kblocks);
    (void)hipFree(plan->d_imel_blob);
    (void)hipFree(plan->d_fam_tw);
    (void)hipFree(plan->d_fam_binof);
    (void)hipFree(plan->d_band_wt);
    (void)hipFree(plan->d_band_lo);
    (void)hipFree(plan->d_band_addr);
    (void)hipFree(plan->d_slot_tab);
    (void)hipFree(plan->d_slot_idx);
    (void)hipFree(plan->d_gen_tables);
    (void)hipFree(plan->d_gen_rev);
    (void)hipFree(plan->d_gen_tw);
  }
  delete plan;
  return RFX_OK;
}

int rfx_pack_magnitudes(const rfx_plan* plan, const float* d_lin_bft, int B, int T, float* d_slots, void* stream) {
  if (!plan || !d_lin_bft || !d_slots || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_pack_magnitudes: bad argument");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) RFX_HIP(launch_gen_pack(d_lin_bft, d_slots, false, B, plan->n_stft, T, plan->gg.fs, (hipStream_t)stream));
  else RFX_HIP(launch_pack_mag(d_lin_bft, d_slots, B, T, (hipStream_t)stream));
  return RFX_OK;
}
int rfx_pack_complex(const rfx_plan* plan, const void* d_bft, int B, int T, void* d_slots, void* stream) {
  if (!plan || !d_bft || !d_slots || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_pack_complex: bad argument");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) RFX_HIP(launch_gen_pack(d_bft, d_slots, true, B, plan->n_stft, T, plan->gg.fs, (hipStream_t)stream));
  else RFX_HIP(launch_pack_angles((const cf*)d_bft, (cf*)d_slots, B, T, (hipStream_t)stream));
  return RFX_OK;
}
int rfx_unpack_complex(const rfx_plan* plan, const void* d_slots, int B, int T, void* d_bft, void* stream) {
  if (!plan || !d_bft || !d_slots || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_unpack_complex: bad argument");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) RFX_HIP(launch_gen_unpack(d_slots, d_bft, true, B, plan->n_stft, T, plan->gg.fs, (hipStream_t)stream));
  else RFX_HIP(launch_unpack_complex((const cf*)d_slots, (cf*)d_bft, B, T, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_stft(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mag_slots, void* d_spec_slots,
             void* stream) {
  if (!plan || !d_wave || B <= 0) return fail(RFX_ERR_INVALID, "rfx_stft: bad argument");
  // torch.stft(center=True, pad_mode="reflect") raises when the pad n_fft/2 is not smaller than the input
  if (Lw <= plan->p.n_fft / 2)
    return fail(RFX_ERR_INVALID, "rfx_stft: reflect padding needs more than n_fft/2 = " + std::to_string(plan->p.n_fft / 2) + " samples");
  RFX_ON_DEVICE(plan->device);
  if (plan->fam_ok) {  // row-family kernels (rfx_fam.hip), same plain layout as the generic engine's
    const FamGeom& f = plan->fam;
    FamFwdArgs fa{};
    fa.g = f;
    fa.wave = d_wave;
    fa.wave_stride = (size_t)Lw;
    fa.Lw = Lw;
    fa.mag = d_mag_slots;
    fa.spec = (cf*)d_spec_slots;
    fa.fs_plain = plan->gg.fs;
    fa.tw1 = plan->d_fam_tw;
    fa.twa = plan->d_fam_tw + (size_t)f.rows * f.h;
    fa.win = plan->d_win;
    fa.B = B;
    fa.T = stft_frames(plan, Lw);
    const long long nframes = (long long)B * fa.T, slots = (long long)plan->num_cus * plan->fam_wgs_per_cu;
    const int nblocks = (int)(nframes < slots ? nframes : slots);
    if (d_mag_slots) RFX_HIP(launch_fam_fwd(0, fa, nblocks, (hipStream_t)stream));
    if (d_spec_slots) RFX_HIP(launch_fam_fwd(1, fa, nblocks, (hipStream_t)stream));
    return RFX_OK;
  }
  if (plan->generic) {
    GenStftArgs g{};
    g.g = plan->gg;
    g.tb = plan->gt;
    g.wave = d_wave;
    g.wave_stride = (size_t)Lw;
    g.mag = d_mag_slots;
    g.spec = (cf*)d_spec_slots;
    g.B = B;
    g.T = stft_frames(plan, Lw);
    g.Lw = Lw;
    if (d_mag_slots) RFX_HIP(launch_gen_stft(0, g, plan->num_cus, (hipStream_t)stream));
    if (d_spec_slots) RFX_HIP(launch_gen_stft(1, g, plan->num_cus, (hipStream_t)stream));
    return RFX_OK;
  }
  StftArgs a;
  a.wave = d_wave;
  a.mag = d_mag_slots;
  a.spec = (cf*)d_spec_slots;
  a.tw1 = plan->d_tw1;
  a.tw2 = plan->d_tw2;
  a.win = plan->d_win;
  a.B = B;
  a.Lw = Lw;
  a.T = 1 + Lw / kHop;
  const long long frames = (long long)B * a.T;
  int fpb = (int)((frames + 2LL * plan->num_cus - 1) / (2LL * plan->num_cus));
  if (fpb < 1) fpb = 1;
  if (fpb > 16) fpb = 16;
  a.frames_per_block = fpb;
  RFX_HIP(launch_stft(a, (hipStream_t)stream));
  return RFX_OK;
}

// Griffin-Lim workspace: three generations (x_{k-1}, x_k, x_{k+1}) of the two parity audio buffers, and the
// istft normalisation table.  No spectral state is kept between iterations (see rfx_gl.hip).
// Small batches take the per-frame kernels (rfx_gl.hip: gl_frame_kernel + gl_fold_kernel): at most four frames per resident
// workgroup slot, where the run-based kernel (>= 10 frames per workgroup) would leave most of the chip idle.
static bool gl_use_latency_mode(const rfx_plan* plan, int B, int T) {
  if (plan->gl_form == RFX_GL_FORM_RUNS) return false;
  if (plan->gl_form == RFX_GL_FORM_FRAMES) return true;
  if (!plan->gl_latency_mode) return false;
  const long long nframes = (long long)B * T, slots = (long long)plan->num_cus * plan->gl_wgs_per_cu;
  if (nframes <= (long long)plan->gl_latency_frames_per_slot * slots) return true;
  // one stair further (round 6): as soon as the batch has more groups than the chip has CUs some CU walks two 16-frame runs and the
  // launch lasts as long as if all did (5.6 ms per Griffin-Lim 32 for nine tiles, 3.7 for eight); the per-frame form still beats
  // that up to ten frames per slot (5.0 / 5.2 ms for nine / ten tiles: profiles/r06_griffinlim_forms_by_batch.txt)
  const long long groups = (long long)B * rfx::gl_groups_per_row(T);
  return groups > plan->num_cus && groups <= slots && 3 * nframes <= 5LL * plan->gl_latency_frames_per_slot * slots;
}

// The runs of one launch of the run-based Griffin-Lim kernel: at most one run per resident workgroup slot of the chip (a launch of
// 520 workgroups on 512 slots runs eight of them alone in a second wave: the ceil(slots / B) runs per clip of rounds 1-4 did that
// for every B that does not divide the slot count).
// Round 6: the unit of the partition is the GROUP (kGlGroup = 16 consecutive frames of a row, rfx_kernels.h): runs are whole groups,
// at most one run per slot and never more runs than groups.  A clip's bits no longer depend on the partition at all (every group
// boundary splits the overlap-add chains, inside a run as between runs), so the partition is free to follow the chip and the batch.
struct GlPartition { int runs, h, w1, w2; };
static GlPartition gl_partition_for(long long slots, int B, int T) {
  const long long N = (long long)B * rfx::gl_groups_per_row(T);
  long long nruns = N;
  if (nruns > slots) nruns = slots;
  if (nruns < 1) nruns = 1;
  // N = q runs + r: the FIRST r runs take q + 1 groups, the others q (gl_run_start with weights q + 1 / q is exact: W_total = N).
  // First, because blocks 0 .. num_cus - 1 are the workgroups the dispatcher places first, one per CU, and the earlier workgroup
  // of a CU wins its issue arbitration: it runs ~12 % faster than the partner that joins it (profiles/r05_wgclock_dispatch_order.txt:
  // 659 against 746 us for 64 frames each), so the extra group of a batch that is not a whole number of groups per slot (B = 65:
  // 32 runs of 80 frames among 480 of 64) lands where there is slack.  (The per-mille skew of round 5 is gone with it: it never
  // moved the step, same file.)
  const long long q = N / nruns, r = N - q * nruns;
  return GlPartition{(int)nruns, (int)r, (int)(q + 1), (int)q};
}
static GlPartition gl_partition(const rfx_plan* plan, int B, int T, int which) {
  (void)which;
  return gl_partition_for((long long)plan->num_cus * plan->gl_wgs_per_cu, B, T);
}

int rfx_griffinlim_runs(const rfx_plan* plan, int B, int T, int which, int64_t* run_starts, int capacity) {
  if (!plan || B <= 0 || T < 2 || plan->generic) return 0;
  const GlPartition p = gl_partition(plan, B, T, which);
  if (run_starts)
    for (int b = 0; b <= p.runs && b < capacity; ++b) run_starts[b] = rfx::gl_run_start_frame(b, p.runs, B, T, p.h, p.w1, p.w2);
  return p.runs;
}

int64_t rfx_debug_run_start(int64_t b, int64_t runs, int64_t n_frames, int64_t h, int64_t w1, int64_t w2) {
  return rfx::gl_run_start(b, runs, n_frames, h, w1, w2);
}

int rfx_debug_gl_partition(int slots, int B, int T, int64_t* run_starts, int capacity) {
  if (slots <= 0 || B <= 0 || T < 2) return 0;
  const GlPartition p = gl_partition_for(slots, B, T);
  if (run_starts)
    for (int b = 0; b <= p.runs && b < capacity; ++b) run_starts[b] = rfx::gl_run_start_frame(b, p.runs, B, T, p.h, p.w1, p.w2);
  return p.runs;
}

int rfx_debug_range_exponents(float max_abs, int mel_units, int* sgd_exponent, int* gl_exponent) {
  if (!sgd_exponent || !gl_exponent) return fail(RFX_ERR_INVALID, "rfx_debug_range_exponents: null argument");
  int k = 0;
  if (max_abs > 0.f) {
    if (max_abs < __builtin_inff()) (void)frexpf(max_abs, &k);
    else k = 129;
  }
  rfx::range_exponents(k, mel_units, sgd_exponent, gl_exponent);
  return RFX_OK;
}

int rfx_griffinlim_form(const rfx_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T < 2) return RFX_GL_FORM_AUTO;
  if (plan->generic) return RFX_GL_FORM_FRAMES;  // the generic engine has one form: frame kernels + fold
  return gl_use_latency_mode(plan, B, T) ? RFX_GL_FORM_FRAMES : RFX_GL_FORM_RUNS;
}

// [B][2] floats of scales + [B] key words (launch_range_scale)
static size_t range_table_bytes(int B) { return align_up((size_t)B * 3 * sizeof(float), 256); }

static void gl_layout(const rfx_plan* plan, int B, int T, size_t& off_audio, size_t& off_scale, size_t& off_frames, size_t& total, int& Lpad) {
  const int L = kHop * (T - 1);
  Lpad = (int)align_up((size_t)L, 64);
  size_t o = 0;
  off_audio = o;
  o += align_up(6 * (size_t)B * Lpad * sizeof(float), 256);
  off_scale = o;
  o += align_up((size_t)Lpad * sizeof(float), 256);
  off_frames = o;
  if (gl_use_latency_mode(plan, B, T)) o += align_up(gl_frame_buffer_bytes(B, T), 256);
  o += range_table_bytes(B);  // the call's own row-scale table (GlArgs::row_scale), at total - range_table_bytes(B)
  total = o;
}

// torch.istft(center=True, length=None) returns n_fft + hop*(T-1) - 2*(n_fft/2) samples: hop*(T-1), plus one when n_fft is odd
static int gen_out_len(const GenGeom& g, int T) { return g.hop * (T - 1) + (g.n_fft & 1); }

// generic path: the windowed synthesis frames and three generations of the audio estimate (x_{k-1}, x_k read; x_{k+1} written)
// (row family: plus the magnitudes re-ordered into slot order, at the end)
static void gen_gl_layout(const rfx_plan* plan, int B, int T, size_t& off_frames, size_t& off_audio, size_t& total, int& Lpad) {
  const GenGeom& g = plan->gg;
  const size_t nf = (size_t)B * T;
  Lpad = (int)align_up((size_t)gen_out_len(g, T), 64);
  size_t o = 0;
  off_frames = o;
  o += align_up(nf * g.fpitch * sizeof(float), 256);
  off_audio = o;
  o += align_up((3 * (size_t)B + 1) * Lpad * sizeof(float), 256);  // + the window envelope of the fold, [Lpad]
  if (plan->fam_ok) o += align_up(nf * plan->fam.fsf * sizeof(float), 256);
  o += range_table_bytes(B);  // as in gl_layout
  total = o;
}

// rfx_call_options as the entry points below see them (NULL / short struct = defaults)
struct CallOpt {
  uint64_t row_base = 0;
  float magnitude_hint = 0.f;
};
static int read_call_options(const rfx_call_options* o, CallOpt* out, const char* who) {
  *out = CallOpt{};
  if (!o) return RFX_OK;
  if (o->struct_size < offsetof(rfx_call_options, row_base) + sizeof(uint64_t))
    return fail(RFX_ERR_INVALID, std::string(who) + ": rfx_call_options.struct_size is not set");
  if (o->flags != 0) return fail(RFX_ERR_INVALID, std::string(who) + ": rfx_call_options.flags must be 0");
  out->row_base = o->row_base;
  if (o->struct_size >= offsetof(rfx_call_options, magnitude_hint) + sizeof(float)) out->magnitude_hint = o->magnitude_hint;
  if (!(out->magnitude_hint >= 0.f) || out->magnitude_hint > 3.0e38f)
    return fail(RFX_ERR_INVALID, std::string(who) + ": rfx_call_options.magnitude_hint must be a finite value >= 0");
  return RFX_OK;
}

// mag_in_fam_slots (rfx_waveform_from_mel on a row-family plan): d_mag already holds the family kernels' slot order [B*T][fsf] -
// InverseMelScale wrote it that way - so the once-per-call re-ordering of the plain frames is left out
static int gen_griffinlim(const rfx_plan* plan, const float* d_mag, const void* d_angles0, uint64_t seed, int B, int T, int n_iter,
                          float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, hipStream_t stream,
                          float* h_launch_ms, const CallOpt& opt, bool mag_in_fam_slots = false, const float* d_row_scale = nullptr) {
  const GenGeom& g = plan->gg;
  const int L = gen_out_len(g, T);
  if (n_iter > 0 && L <= g.n_fft / 2)
    return fail(RFX_ERR_INVALID, "rfx_griffinlim: Padding size should be less than the corresponding input dimension (reflect padding " +
                                 std::to_string(g.n_fft / 2) + " needs more than that many samples)");
  size_t ofr, oa, total;
  int Lpad;
  gen_gl_layout(plan, B, T, ofr, oa, total, Lpad);
  if (workspace_bytes < total) return fail(RFX_ERR_WORKSPACE, "rfx_griffinlim: workspace too small");
  char* ws = (char*)d_workspace;
  float* frames = (float*)(ws + ofr);
  float* gen[3];
  for (int i = 0; i < 3; ++i) gen[i] = (float*)(ws + oa) + (size_t)i * B * Lpad;  // x_k lives in gen[k % 3]
  float* env = (float*)(ws + oa) + (size_t)3 * B * Lpad;
  if (!d_row_scale) {  // numeric range: from the caller's hint, else from the magnitudes themselves (one pass over them)
    float* tab = (float*)(ws + total - range_table_bytes(B));
    const size_t per_row = (size_t)T * ((plan->fam_ok && mag_in_fam_slots) ? (size_t)plan->fam.fsf : (size_t)g.fs);
    RFX_HIP(launch_range_scale(d_mag, per_row, B, opt.magnitude_hint, (unsigned*)(tab + 2 * (size_t)B), nullptr, tab, 1, 0, stream));
    d_row_scale = tab;
  }
  RFX_HIP(launch_gen_env(plan->d_win, env, g, T, L, stream));
  // padded frame rows (gen_frame_layout): the kernels write the window samples only, the fold reads the padding as zeros
  if (g.fshift > 0) RFX_HIP(hipMemsetAsync(frames, 0, (size_t)B * T * g.fpitch * sizeof(float), stream));
  EventList events;
  if (h_launch_ms) {
    RFX_HIP(events.create(n_iter + 2));
    RFX_HIP(hipEventRecord(events.ev[0], stream));
  }
  if (plan->fam_ok) {
    const FamGeom& f = plan->fam;
    const float* S_slots = d_mag;
    if (!mag_in_fam_slots) {
      float* repacked = (float*)(ws + oa + align_up((3 * (size_t)B + 1) * Lpad * sizeof(float), 256));
      RFX_HIP(launch_fam_repack(d_mag, repacked, plan->d_fam_binof, (long long)B * T, g.fs, f.fsf, f.n_stft, stream));
      S_slots = repacked;
    }
    FamGlArgs fa{};
    fa.g = f;
    fa.S = S_slots;
    fa.angles0 = (const cf*)d_angles0;
    fa.fs_plain = g.fs;
    fa.audio_stride = (size_t)Lpad;
    fa.frames = frames;
    fa.row_scale = d_row_scale;
    fa.fpitch = g.fpitch;
    fa.fshift = g.fshift;
    fa.tw1 = plan->d_fam_tw;
    fa.twa = plan->d_fam_tw + (size_t)f.rows * f.h;
    fa.win = plan->d_win;
    fa.mom = momentum / (1.f + momentum);
    fa.seed = seed;
    fa.frame_base = opt.row_base * (uint64_t)T;
    fa.B = B;
    fa.T = T;
    fa.L = L;
    const long long nframes = (long long)B * T, slots = (long long)plan->num_cus * plan->fam_wgs_per_cu;
    const int nblocks = (int)(nframes < slots ? nframes : slots);
    // x_it lives in gen[it % 2]; gen[2] holds d_it = x_it - m x_{it-1} (d_0 = x_0), which the fold writes next to x_it and the
    // next launch analyses (the kernel used to form it from two generations itself)
    for (int it = 0; it <= n_iter; ++it) {
      fa.x_cur = gen[2];
      fa.x_prev = nullptr;
      RFX_HIP(launch_fam_gl(it == 0 ? 0 : 1, fa, nblocks, stream));
      const bool last = it == n_iter;
      RFX_HIP(launch_gen_fold(frames, env, last ? d_wave_out : gen[it % 2], g, B, T, L, last ? (size_t)L : (size_t)Lpad, stream,
                              it == 0 ? nullptr : gen[(it + 1) % 2], last ? nullptr : gen[2], fa.mom, d_row_scale));
      if (h_launch_ms) RFX_HIP(hipEventRecord(events.ev[it + 1], stream));
    }
    if (h_launch_ms) {
      RFX_HIP(hipEventSynchronize(events.ev[n_iter + 1]));
      for (int i = 0; i <= n_iter; ++i) RFX_HIP(hipEventElapsedTime(&h_launch_ms[i], events.ev[i], events.ev[i + 1]));
    }
    return RFX_OK;
  }
  GenGlArgs a{};
  a.g = g;
  a.tb = plan->gt;
  a.S = d_mag;
  a.angles0 = (const cf*)d_angles0;
  a.audio_stride = (size_t)Lpad;
  a.frames = frames;
  a.row_scale = d_row_scale;
  a.mom = momentum / (1.f + momentum);
  a.seed = seed;
  a.frame_base = opt.row_base * (uint64_t)T;
  a.B = B;
  a.T = T;
  a.L = L;
  for (int it = 0; it <= n_iter; ++it) {
    // iteration `it` analyses d = x_{it-1} - m * x_{it-2} (the momentum term of the reference's `rebuilt - m * tprev`, applied in
    // the time domain; d = x_0 for it == 1) and writes the frames of x_it; it == 0 synthesises the initial estimate from
    // S * angles0.  As on the row family, the fold of iteration it - 1 forms d next to x_{it-1} (x_it lives in gen[it % 2], d in
    // gen[2]), so the kernel runs its one-signal mode for every iteration: half the audio loads, same bits.
    a.x_cur = gen[2];
    a.x_prev = nullptr;
    RFX_HIP(launch_gen_gl(it == 0 ? 0 : 1, a, plan->num_cus, stream));
    const bool last = it == n_iter;
    RFX_HIP(launch_gen_fold(frames, env, last ? d_wave_out : gen[it % 2], g, B, T, L, last ? (size_t)L : (size_t)Lpad, stream,
                            it == 0 ? nullptr : gen[(it + 1) % 2], last ? nullptr : gen[2], a.mom, d_row_scale));
    if (h_launch_ms) RFX_HIP(hipEventRecord(events.ev[it + 1], stream));
  }
  if (h_launch_ms) {
    RFX_HIP(hipEventSynchronize(events.ev[n_iter + 1]));
    for (int i = 0; i <= n_iter; ++i) RFX_HIP(hipEventElapsedTime(&h_launch_ms[i], events.ev[i], events.ev[i + 1]));
  }
  return RFX_OK;
}

size_t rfx_griffinlim_workspace_bytes(const rfx_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T < 2) return 0;
  if (plan->generic) {
    size_t a, b, total;
    int Lpad;
    gen_gl_layout(plan, B, T, a, b, total, Lpad);
    return total;
  }
  size_t a, c, fr, total;
  int Lpad;
  gl_layout(plan, B, T, a, c, fr, total, Lpad);
  return total;
}

static int griffinlim_impl(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                           int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                           void* stream_, float* h_launch_ms, const CallOpt& opt, const float* d_row_scale = nullptr) {
  if (!plan || !d_mag_slots || !d_wave_out || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_griffinlim: null argument");
  if (B <= 0 || T < 2 || n_iter < 0) return fail(RFX_ERR_INVALID, "rfx_griffinlim: bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, "rfx_griffinlim: more than 2^31 - 1 frames in one call");
  if (!(momentum >= 0.f && momentum < 1.f)) return fail(RFX_ERR_INVALID, "rfx_griffinlim: momentum must be in [0, 1)");
  if (plan->generic) {
    RFX_ON_DEVICE(plan->device);
    return gen_griffinlim(plan, d_mag_slots, d_angles0_slots, seed, B, T, n_iter, momentum, d_wave_out, d_workspace, workspace_bytes,
                          (hipStream_t)stream_, h_launch_ms, opt, false, d_row_scale);
  }
  // every iteration re-analyses the hop*(T-1)-sample estimate with torch.stft(center=True, reflect):
  // the reference raises there unless the signal is longer than the n_fft/2 padding
  if (n_iter > 0 && kHop * (T - 1) <= kNfft / 2)
    return fail(RFX_ERR_INVALID, "rfx_griffinlim: Padding size should be less than the corresponding input dimension "
                                 "(reflect padding 8820 needs more than 8820 samples, i.e. at least 22 frames)");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  size_t off_audio, off_scale, off_frames, total;
  int Lpad;
  gl_layout(plan, B, T, off_audio, off_scale, off_frames, total, Lpad);
  if (workspace_bytes < total) return fail(RFX_ERR_WORKSPACE, "rfx_griffinlim: workspace too small");
  const int L = kHop * (T - 1);
  char* ws = (char*)d_workspace;
  float* audio = (float*)(ws + off_audio);
  float* gen[3][2];
  for (int i = 0; i < 3; ++i)
    for (int p = 0; p < 2; ++p) gen[i][p] = audio + (size_t)(2 * i + p) * B * Lpad;
  float* scale = (float*)(ws + off_scale);

  hipLaunchKernelGGL(out_scale_kernel, dim3((L + 255) / 256), dim3(256), 0, stream, plan->d_win, scale, T, L);
  RFX_HIP(hipGetLastError());
  if (!d_row_scale) {  // numeric range: from the caller's hint, else from the magnitudes themselves (one pass over them)
    float* tab = (float*)(ws + total - range_table_bytes(B));
    RFX_HIP(launch_range_scale(d_mag_slots, (size_t)T * kFrameStride, B, opt.magnitude_hint, (unsigned*)(tab + 2 * (size_t)B), nullptr, tab, 1, 0, stream));
    d_row_scale = tab;
  }

  if (gl_use_latency_mode(plan, B, T)) {
    // x_k lives in generation k % 3 (one folded buffer each: gen[k][0]); frame kernel + fold per iteration
    GlFrameArgs fa;
    fa.S = d_mag_slots;
    fa.angles0 = (const cf*)d_angles0_slots;
    fa.frames = (float*)(ws + off_frames);
    fa.row_scale = d_row_scale;
    fa.tw1 = plan->d_tw1;
    fa.tw2 = plan->d_tw2;
    fa.win = plan->d_win;
    fa.B = B;
    fa.T = T;
    fa.L = L;
    fa.Lpad = Lpad;
    fa.mom = momentum / (1.f + momentum);
    fa.seed = seed;
    fa.frame_base = opt.row_base * (uint64_t)T;
    const long long nframes = (long long)B * T;
    const long long slots = (long long)plan->num_cus * plan->gl_wgs_per_cu;
    const int nblocks = (int)(nframes < slots ? nframes : slots);
    EventList events;
    if (h_launch_ms) {
      RFX_HIP(events.create(n_iter + 2));
      RFX_HIP(hipEventRecord(events.ev[0], stream));
    }
    for (int it = 0; it <= n_iter; ++it) {
      fa.audio_in = gen[(it + 2) % 3][0];    // x_{it-1}
      fa.audio_prev = gen[(it + 1) % 3][0];  // x_{it-2}
      RFX_HIP(launch_gl_frame(it == 0 ? 0 : it == 1 ? 1 : 2, fa, nblocks, stream));
      const bool last = it == n_iter;
      RFX_HIP(launch_gl_fold(fa.frames, plan->d_win, scale, last ? d_wave_out : gen[it % 3][0], B, T, L, last ? (size_t)L : (size_t)Lpad, stream));
      if (h_launch_ms) RFX_HIP(hipEventRecord(events.ev[it + 1], stream));
    }
    if (h_launch_ms) {
      RFX_HIP(hipEventSynchronize(events.ev[n_iter + 1]));
      for (int i = 0; i <= n_iter; ++i) RFX_HIP(hipEventElapsedTime(&h_launch_ms[i], events.ev[i], events.ev[i + 1]));
    }
    return RFX_OK;
  }

  GlArgs g;
  g.S = d_mag_slots;
  g.angles0 = (const cf*)d_angles0_slots;
  g.out_scale = scale;
  g.row_scale = d_row_scale;
  g.tw1 = plan->d_tw1;
  g.tw2 = plan->d_tw2;
  g.win = plan->d_win;
  g.B = B;
  g.T = T;
  g.L = L;
  g.Lpad = Lpad;
  g.mom = momentum / (1.f + momentum);
  g.seed = seed;
  g.frame_base = opt.row_base * (uint64_t)T;
  g.timing = plan->timing;
  // runs: the batch's B*T frames, counted clip after clip, are cut into one run per resident workgroup slot (gl_partition)
  GlPartition part = gl_partition(plan, B, T, 0);
  const int nblocks = part.runs;
  auto set_partition = [&](int which) {
    part = gl_partition(plan, B, T, which);
    g.run_h = part.h;
    g.run_w1 = part.w1;
    g.run_w2 = part.w2;
  };
  set_partition(0);

  // optional per-launch timing with HIP events recorded on the launch stream (bench.py's roofline leg)
  EventList events;
  std::vector<hipEvent_t>& ev = events.ev;
  if (h_launch_ms) {
    RFX_HIP(events.create(n_iter + 2));
    RFX_HIP(hipEventRecord(ev[0], stream));
  }
  // generation indices: x_k lives in gen[k % 3]
  auto set_io = [&](int k_in, int k_prev, int k_out) {
    for (int p = 0; p < 2; ++p) {
      g.audio_in[p] = gen[k_in][p];
      g.audio_prev[p] = gen[k_prev][p];
      g.audio_out[p] = gen[k_out][p];
    }
  };
  set_io(1, 2, 0);  // MODE 0 reads nothing; writes x_0
#ifdef RFX_WGCLOCK
  g.launch = 0;
#endif
  RFX_HIP(launch_gl_iter(0, g, nblocks, stream));
  if (h_launch_ms) RFX_HIP(hipEventRecord(ev[1], stream));
  set_partition(1);
  for (int it = 1; it <= n_iter; ++it) {
    // iteration `it` analyses x_{it-1} - m*x_{it-2} and writes x_it
    set_io((it - 1) % 3, (it + 1) % 3 /* == (it-2) mod 3 */, it % 3);
#ifdef RFX_WGCLOCK
    g.launch = it;
#endif
    RFX_HIP(launch_gl_iter(it == 1 ? 1 : 2, g, nblocks, stream));
    if (h_launch_ms) RFX_HIP(hipEventRecord(ev[it + 1], stream));
  }
  const int last = n_iter % 3;
  RFX_HIP(launch_gl_combine(gen[last][0], gen[last][1], d_wave_out, B, L, Lpad, stream));
  if (h_launch_ms) {
    RFX_HIP(hipEventSynchronize(ev[n_iter + 1]));
    for (int i = 0; i <= n_iter; ++i) RFX_HIP(hipEventElapsedTime(&h_launch_ms[i], ev[i], ev[i + 1]));
  }
  return RFX_OK;
}

int rfx_griffinlim(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                   int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                   void* stream) {
  return griffinlim_impl(plan, d_mag_slots, d_angles0_slots, seed, B, T, n_iter, momentum, d_wave_out, d_workspace,
                         workspace_bytes, stream, nullptr, CallOpt{});
}

int rfx_griffinlim_ex(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                      int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                      void* stream, const rfx_call_options* options, float* h_launch_ms) {
  CallOpt opt;
  if (int rc = read_call_options(options, &opt, "rfx_griffinlim_ex")) return rc;
  return griffinlim_impl(plan, d_mag_slots, d_angles0_slots, seed, B, T, n_iter, momentum, d_wave_out, d_workspace,
                         workspace_bytes, stream, h_launch_ms, opt);
}

int rfx_griffinlim_timed(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                         int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                         void* stream, float* h_launch_ms) {
  if (!h_launch_ms) return fail(RFX_ERR_INVALID, "rfx_griffinlim_timed: null timing array");
  return griffinlim_impl(plan, d_mag_slots, d_angles0_slots, seed, B, T, n_iter, momentum, d_wave_out, d_workspace,
                         workspace_bytes, stream, h_launch_ms, CallOpt{});
}

int rfx_unpack_magnitudes(const rfx_plan* plan, const float* d_slots, int B, int T, float* d_bft, void* stream) {
  if (!plan || !d_bft || !d_slots || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_unpack_magnitudes: bad argument");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) RFX_HIP(launch_gen_unpack(d_slots, d_bft, false, B, plan->n_stft, T, plan->gg.fs, (hipStream_t)stream));
  else RFX_HIP(launch_unpack_mag(d_slots, d_bft, B, T, (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_mel_workspace_bytes(const rfx_plan* plan, int B, int Lw) {
  if (!plan || B <= 0 || Lw <= plan->p.n_fft / 2) return 0;
  const size_t T = (size_t)stft_frames(plan, Lw);
  if (plan->generic)  // magnitudes [B*T][fs] + frame-major mel amplitudes [B*T][Mpad]
    return align_up((size_t)B * T * plan->gg.fs * sizeof(float), 256) + align_up((size_t)B * T * plan->Mpad * sizeof(float), 256);
  // the fused kernel keeps the magnitudes on chip: its scratch is the frame-major copy of the mel amplitudes
  if (plan->fwd_ok && !plan->fwd_unfused) return align_up((size_t)B * T * plan->Mpad * sizeof(float), 256);
  return align_up((size_t)B * T * kFrameStride * sizeof(float), 256);
}

// does the plan's forward path leave the mel amplitudes frame-major ([B*T][Mpad]) in the workspace before transposing them?
static bool forward_has_frame_major(const rfx_plan* plan) { return plan->generic ? plan->fwd_ok : (plan->fwd_ok && !plan->fwd_unfused); }

// rfx_mel_from_waveform, and the front half of rfx_image_from_waveform: there d_mel_out is null (no (B, M, T) copy is made),
// *mel_tm_out receives the frame-major amplitudes and - where the kernel can take it on the fly - max_keys the keys of the maxima its
// workgroups formed, *keys_per_row of them for every row, rows in order (0: it did not; up to T per row: image_keys_bytes)
static int mel_forward(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace, size_t workspace_bytes,
                       void* stream, float** mel_tm_out, unsigned* max_keys, int max_group, int* keys_per_row) {
  if (!plan || !d_wave || !d_workspace || (!d_mel_out && !mel_tm_out)) return fail(RFX_ERR_INVALID, "rfx_mel_from_waveform: null argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, "rfx_mel_from_waveform: plan was created without a mel filterbank");
  if (workspace_bytes < rfx_mel_workspace_bytes(plan, B, Lw) || Lw <= plan->p.n_fft / 2)
    return fail(Lw <= plan->p.n_fft / 2 ? RFX_ERR_INVALID : RFX_ERR_WORKSPACE, "rfx_mel_from_waveform: input too short or workspace too small");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) {
    if (!plan->fwd_ok) return fail(RFX_ERR_UNSUPPORTED, "rfx_mel_from_waveform: filterbank is not banded: " + plan->imel_why);
    const int T = stft_frames(plan, Lw);
    float* mag = (float*)d_workspace;
    float* mel_tm = (float*)((char*)d_workspace + align_up((size_t)B * T * plan->gg.fs * sizeof(float), 256));
    if (plan->fam_ok && !plan->fwd_unfused) {  // row family: transform and banded projection in one kernel, |X| stays on chip
      const FamGeom& f = plan->fam;
      FamFwdArgs fa{};
      fa.g = f;
      fa.wave = d_wave;
      fa.wave_stride = (size_t)Lw;
      fa.Lw = Lw;
      fa.fs_plain = plan->gg.fs;
      fa.tw1 = plan->d_fam_tw;
      fa.twa = plan->d_fam_tw + (size_t)f.rows * f.h;
      fa.win = plan->d_win;
      fa.B = B;
      fa.T = T;
      fa.mel_tm = mel_tm;
      fa.band_wt = plan->d_band_wt;
      fa.band_lo = plan->d_band_lo;
      fa.band_len = plan->d_band_lo + plan->Mpad;
      fa.M = plan->p.n_mels;
      fa.Mpad = plan->Mpad;
      const long long nframes = (long long)B * T, slots = (long long)plan->num_cus * plan->fam_wgs_per_cu;
      RFX_HIP(launch_fam_fwd(2, fa, (int)(nframes < slots ? nframes : slots), (hipStream_t)stream));
      if (mel_tm_out) *mel_tm_out = mel_tm;
      if (d_mel_out) RFX_HIP(launch_mel_transpose(mel_tm, d_mel_out, B, T, plan->p.n_mels, plan->Mpad, (hipStream_t)stream));
      return RFX_OK;
    }
    int rc = rfx_stft(plan, d_wave, B, Lw, mag, nullptr, stream);
    if (rc) return rc;
    RFX_HIP(launch_gen_mel(mag, mel_tm, plan->d_band_wt, plan->d_band_lo, plan->d_band_lo + plan->Mpad, (long long)B * T, plan->gg.fs,
                           plan->p.n_mels, plan->Mpad, plan->imel.f_lo, plan->imel.f_hi, (hipStream_t)stream));
    if (mel_tm_out) *mel_tm_out = mel_tm;
    if (d_mel_out) RFX_HIP(launch_mel_transpose(mel_tm, d_mel_out, B, T, plan->p.n_mels, plan->Mpad, (hipStream_t)stream));
    return RFX_OK;
  }
  if (plan->fwd_ok && !plan->fwd_unfused) {
    StftMelArgs f;
    f.wave = d_wave;
    f.mel = d_mel_out;
    f.mel_tm = (float*)d_workspace;
    f.tw1 = plan->d_tw1;
    f.tw2 = plan->d_tw2;
    f.win = plan->d_win;
    f.band_wt = plan->d_band_wt;
    f.band_addr = plan->d_band_addr;
    f.band_lo = plan->d_band_lo;
    f.band_len = plan->d_band_lo + plan->Mpad;
    f.B = B;
    f.Lw = Lw;
    f.T = 1 + Lw / kHop;
    f.M = plan->p.n_mels;
    f.Mpad = plan->Mpad;
    f.f_lo = plan->imel.f_lo;
    f.f_hi = plan->imel.f_hi;
    f.slot_tab = plan->d_slot_tab;
    f.pad_tab = plan->d_slot_idx;
    f.filt_seg = plan->d_slot_idx ? plan->d_slot_idx + (size_t)kMelPadsPerThread * kQPad : nullptr;
    f.slot_at = plan->d_slot_idx ? f.filt_seg + 2 * (size_t)plan->Mpad : nullptr;
    f.prod_arr = plan->fwd_prod_arr;
    f.kb_mask = plan->fwd_kb_mask;
    f.pk_at = plan->fwd_packed_off ? reinterpret_cast<const unsigned*>(plan->d_slot_idx + plan->fwd_packed_off) : nullptr;
    f.pk_pad = f.pk_at ? f.pk_at + 5 * (size_t)kQPad : nullptr;
    f.pk_seg = f.pk_at ? f.pk_pad + 2 * (size_t)kQPad : nullptr;
    f.max_keys = plan->d_slot_tab ? max_keys : nullptr;  // (the product-form kernel takes the maximum on the fly)
    f.max_group = max_group > 0 ? max_group : 1;
    if (mel_tm_out) *mel_tm_out = f.mel_tm;
    // runs of consecutive frames: every resident workgroup slot of the chip gets one run when the batch allows it (the
    // product-form kernel carries a sliding input window along a run), at most 64 frames, at least 1
    const long long frames = (long long)B * f.T;
    const int cap = plan->d_slot_tab ? plan->fwd_run_cap : 16;
    int fpb = (int)((frames + 2LL * plan->num_cus - 1) / (2LL * plan->num_cus));
    f.frames_per_block = fpb < 1 ? 1 : fpb > cap ? cap : fpb;
    {  // unequal runs by dispatch order (StftMelArgs::run_skew), only in the shape it was measured in: one wave of workgroups, two per CU
      const int chunks = (f.T + f.frames_per_block - 1) / f.frames_per_block;
      const bool shape_ok = plan->d_slot_tab && chunks % 2 == 0 && chunks * f.frames_per_block == f.T && (long long)B * chunks == 2LL * plan->num_cus;
      const int d = (int)((long long)f.frames_per_block * plan->fwd_run_skew / 1000);
      f.run_skew = shape_ok && d > 0 && d < f.frames_per_block ? d : 0;
      if (keys_per_row) *keys_per_row = f.max_keys ? chunks : 0;
    }
    RFX_HIP(launch_stft_mel(f, (hipStream_t)stream));
    return RFX_OK;
  }
  if (!d_mel_out) return fail(RFX_ERR_INVALID, "rfx_mel_from_waveform: this plan's forward path has no frame-major stage");
  float* mag = (float*)d_workspace;
  int rc = rfx_stft(plan, d_wave, B, Lw, mag, nullptr, stream);
  if (rc) return rc;
  MelArgs a;
  a.mag = mag;
  a.fbs = plan->d_melfb_slots;
  a.kblocks = plan->d_kblocks;
  a.n_kblocks = plan->n_kblocks;
  a.out = d_mel_out;
  a.M = plan->p.n_mels;
  a.Mp = plan->melfb_cols;
  a.T = 1 + Lw / kHop;
  a.N = B * a.T;
  RFX_HIP(launch_mel_gemm(a, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_mel_from_waveform(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  if (!d_mel_out) return fail(RFX_ERR_INVALID, "rfx_mel_from_waveform: null argument");
  return mel_forward(plan, d_wave, B, Lw, d_mel_out, d_workspace, workspace_bytes, stream, nullptr, nullptr, 1, nullptr);
}

// ---- spectrogram_image_from_audio's device half (spectrogram_image_converter.py:30-51: spectrogram_from_audio, then
// image_util.image_from_spectrogram): waveforms -> mel amplitudes -> uint8 image without the (B, M, T) tensor in between
// the forward kernel leaves one key per workgroup: at most one workgroup per frame
static size_t image_keys_bytes(const rfx_plan* plan, int rows, int Lw) { return align_up((size_t)rows * stft_frames(plan, Lw) * sizeof(unsigned), 256); }

size_t rfx_image_from_waveform_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw) {
  if (!plan || N <= 0) return 0;
  const int C = stereo ? 2 : 1;
  const size_t mel_ws = rfx_mel_workspace_bytes(plan, N * C, Lw);
  if (!mel_ws) return 0;
  size_t total = mel_ws + image_keys_bytes(plan, N * C, Lw);
  if (!forward_has_frame_major(plan)) total += align_up((size_t)N * C * plan->p.n_mels * stft_frames(plan, Lw) * sizeof(float), 256);
  return total;
}

int rfx_image_from_waveform(const rfx_plan* plan, const float* d_wave, int N, int stereo, int Lw, const float* d_thresholds255,
                            float* d_clip_max, uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!plan || !d_wave || !d_thresholds255 || !d_clip_max || !d_img_out || !d_workspace || N <= 0)
    return fail(RFX_ERR_INVALID, "rfx_image_from_waveform: bad argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, "rfx_image_from_waveform: plan was created without a mel filterbank");
  if (Lw <= plan->p.n_fft / 2) return fail(RFX_ERR_INVALID, "rfx_image_from_waveform: input too short");
  if (workspace_bytes < rfx_image_from_waveform_workspace_bytes(plan, N, stereo, Lw)) return fail(RFX_ERR_WORKSPACE, "rfx_image_from_waveform: workspace too small");
  RFX_ON_DEVICE(plan->device);
  const int C = stereo ? 2 : 1, B = N * C, T = stft_frames(plan, Lw), M = plan->p.n_mels;
  const size_t mel_ws = rfx_mel_workspace_bytes(plan, B, Lw);
  unsigned* keys = reinterpret_cast<unsigned*>((char*)d_workspace + mel_ws);
  if (!forward_has_frame_major(plan)) {  // (dense-GEMM fall-back of a non-banded bank: the two calls, the tensor in the workspace)
    float* mel = reinterpret_cast<float*>((char*)keys + image_keys_bytes(plan, B, Lw));
    if (int rc = rfx_mel_from_waveform(plan, d_wave, B, Lw, mel, d_workspace, mel_ws, stream)) return rc;
    return rfx_image_encode_u8(mel, N, M, T, stereo, d_thresholds255, d_clip_max, d_img_out, stream);
  }
  float* mel_tm = nullptr;
  int keys_per_row = 0;  // (round 6: one key per workgroup of the forward kernel, every one written by the launch: nothing to zero)
  if (int rc = mel_forward(plan, d_wave, B, Lw, nullptr, d_workspace, mel_ws, stream, &mel_tm, keys, C, &keys_per_row)) return rc;
  // (a kernel that does not take the maximum on the fly: one pass over the frame-major amplitudes; their padding columns are zero
  // and mel amplitudes are not negative)
  if (!keys_per_row) RFX_HIP(launch_clip_max(mel_tm, reinterpret_cast<float*>(keys), N, (size_t)C * T * plan->Mpad, false, (hipStream_t)stream));
  RFX_HIP(launch_image_encode_tm(mel_tm, keys_per_row ? keys : nullptr, C * keys_per_row, keys_per_row ? nullptr : reinterpret_cast<const float*>(keys),
                                 d_thresholds255, d_img_out, d_clip_max, N, M, plan->Mpad, T, C, (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_mel_scale_workspace_bytes(const rfx_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T <= 0) return 0;
  if (plan->generic)
    return align_up((size_t)B * T * plan->gg.fs * sizeof(float), 256) + align_up((size_t)B * T * plan->Mpad * sizeof(float), 256);
  return align_up((size_t)B * T * kFrameStride * sizeof(float), 256);
}

int rfx_mel_scale(const rfx_plan* plan, const float* d_lin_bft, int B, int T, float* d_mel_out, void* d_workspace,
                  size_t workspace_bytes, void* stream) {
  if (!plan || !d_lin_bft || !d_mel_out || !d_workspace || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_mel_scale: bad argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, "rfx_mel_scale: plan was created without a mel filterbank");
  if (workspace_bytes < rfx_mel_scale_workspace_bytes(plan, B, T)) return fail(RFX_ERR_WORKSPACE, "rfx_mel_scale: workspace too small");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) {
    if (!plan->fwd_ok) return fail(RFX_ERR_UNSUPPORTED, "rfx_mel_scale: filterbank is not banded: " + plan->imel_why);
    float* mag = (float*)d_workspace;
    float* mel_tm = (float*)((char*)d_workspace + align_up((size_t)B * T * plan->gg.fs * sizeof(float), 256));
    RFX_HIP(launch_gen_pack(d_lin_bft, mag, false, B, plan->n_stft, T, plan->gg.fs, (hipStream_t)stream));
    RFX_HIP(launch_gen_mel(mag, mel_tm, plan->d_band_wt, plan->d_band_lo, plan->d_band_lo + plan->Mpad, (long long)B * T, plan->gg.fs,
                           plan->p.n_mels, plan->Mpad, plan->imel.f_lo, plan->imel.f_hi, (hipStream_t)stream));
    RFX_HIP(launch_mel_transpose(mel_tm, d_mel_out, B, T, plan->p.n_mels, plan->Mpad, (hipStream_t)stream));
    return RFX_OK;
  }
  float* mag = (float*)d_workspace;
  RFX_HIP(launch_pack_mag(d_lin_bft, mag, B, T, (hipStream_t)stream));
  MelArgs a;
  a.mag = mag;
  a.fbs = plan->d_melfb_slots;
  a.kblocks = plan->d_kblocks;
  a.n_kblocks = plan->n_kblocks;
  a.out = d_mel_out;
  a.M = plan->p.n_mels;
  a.Mp = plan->melfb_cols;
  a.T = T;
  a.N = B * T;
  RFX_HIP(launch_mel_gemm(a, (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_inverse_mel_workspace_bytes(const rfx_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T <= 0) return 0;
  return align_up((size_t)B * T * plan->p.max_mel_iters * sizeof(float), 256) + align_up((size_t)(B + 1) * sizeof(int), 256) + range_table_bytes(B);
}

// can InverseMelScale write a row-family plan's frames straight in the family kernels' slot order?  (Every kernel that leaves
// through imel_emit_frame can: the output order is just its pos_bin table.  The general LDS kernel stores bin by bin.)
static bool imel_can_emit_fam_slots(const rfx_plan* plan) {
  return plan->generic && plan->fam_ok && plan->imel_ok && plan->d_fam_binof &&
         rfx::imel_kernel_choice(plan->imel, plan->p.n_mels, plan->p.max_mel_iters, plan->imel_variant) != 0;
}

static int inverse_mel_impl(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                            uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream_, bool fam_slots,
                            const CallOpt& opt, float* d_gl_row_scale = nullptr);

int rfx_inverse_mel(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                    uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream_) {
  return inverse_mel_impl(plan, d_mel, B, T, channels_per_clip, d_spec0, seed, d_mag_slots, d_workspace, workspace_bytes, stream_, false, CallOpt{});
}

int rfx_inverse_mel_ex(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                       uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream_,
                       const rfx_call_options* options) {
  CallOpt opt;
  if (int rc = read_call_options(options, &opt, "rfx_inverse_mel_ex")) return rc;
  return inverse_mel_impl(plan, d_mel, B, T, channels_per_clip, d_spec0, seed, d_mag_slots, d_workspace, workspace_bytes, stream_, false, opt);
}

static int inverse_mel_impl(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                            uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream_, bool fam_slots,
                            const CallOpt& opt, float* d_gl_row_scale) {
  if (!plan || !d_mel || !d_mag_slots || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_inverse_mel: null argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, "rfx_inverse_mel: plan was created without a mel filterbank");
  if (!plan->imel_ok) return fail(RFX_ERR_UNSUPPORTED, "rfx_inverse_mel: filterbank is not banded: " + plan->imel_why);
  if (B <= 0 || T <= 0 || channels_per_clip <= 0 || B % channels_per_clip)
    return fail(RFX_ERR_INVALID, "rfx_inverse_mel: batch must be a multiple of channels_per_clip");
  if (opt.row_base % (uint64_t)channels_per_clip)
    return fail(RFX_ERR_INVALID, "rfx_inverse_mel: rfx_call_options.row_base must be a multiple of channels_per_clip (clips are not split)");
  if (workspace_bytes < rfx_inverse_mel_workspace_bytes(plan, B, T)) return fail(RFX_ERR_WORKSPACE, "rfx_inverse_mel: workspace too small");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int nclips = B / channels_per_clip;
  char* ws = (char*)d_workspace;
  float* hist = (float*)ws;
  int* it_stop = (int*)(ws + align_up((size_t)B * T * plan->p.max_mel_iters * sizeof(float), 256));
  int* any_early = it_stop + nclips;
  RFX_HIP(hipMemsetAsync(any_early, 0, sizeof(int), stream));
  // numeric range: the power of two each clip's SGD state is held in (and, for the fused call, the Griffin-Lim rows' factors),
  // from the caller's hint or the clip's largest mel amplitude
  float* clip_scale = (float*)(ws + align_up((size_t)B * T * plan->p.max_mel_iters * sizeof(float), 256) + align_up((size_t)(B + 1) * sizeof(int), 256));
  RFX_HIP(launch_range_scale(d_mel, (size_t)channels_per_clip * plan->p.n_mels * T, nclips, opt.magnitude_hint, (unsigned*)(clip_scale + 2 * (size_t)nclips),
                             clip_scale, d_gl_row_scale, channels_per_clip, 1, stream));
  ImelArgs a;
  a.clip_scale = clip_scale;
  a.sc = a.un = 0.f;
  a.tb = plan->imel;
  a.mel = d_mel;
  a.spec0 = d_spec0;
  a.out_slots = d_mag_slots;
  a.loss_hist = hist;
  a.it_limit = nullptr;
  a.B = B;
  a.M = plan->p.n_mels;
  a.T = T;
  a.C = channels_per_clip;
  a.n_stft = plan->n_stft;
  a.out_stride = plan->frame_stride;
  a.plain = plan->generic ? 1 : 0;
  if (fam_slots) {  // (imel_can_emit_fam_slots: the frame's positions are the family kernels' slots)
    a.tb.pos_bin = plan->d_fam_binof;
    a.out_stride = plan->fam.fsf;
  }
  a.max_iter = plan->p.max_mel_iters;
  a.lr = 0.1f;        // sgdargs=None -> {"lr": 0.1, "momentum": 0.9} (torchaudio 0.13 InverseMelScale)
  a.momentum = 0.9f;
  a.seed = seed;
  a.frame_base = opt.row_base * (uint64_t)T;
  if (a.max_iter <= 0) return fail(RFX_ERR_INVALID, "rfx_inverse_mel: max_mel_iters must be positive");
  RFX_HIP(launch_imel(a, plan->imel_variant, stream));
  // reproduce the reference's early exit (tolerance_loss 1e-5, tolerance_change 1e-8,
  // spectrogram_converter.py:94-95): scan the clip losses, then re-run stopped clips for it_stop steps
  RFX_HIP(launch_imel_scan(hist, it_stop, any_early, nclips, channels_per_clip, T, a.max_iter, 1e-5f, 1e-8f, stream));
  a.it_limit = it_stop;
  RFX_HIP(launch_imel(a, plan->imel_variant, stream));
  return RFX_OK;
}

// ---- SpectrogramConverter.waveform_from_mel_amplitudes in one call (spectrogram_converter.py:187-204: inverse_mel_scaler, then
// inverse_spectrogram_func).  rfx_inverse_mel into the head of the workspace, rfx_griffinlim from there: the same two launches
// sequences, the same seeds (seed for the SGD start, seed + 1 for the phases, as the Python layer always called them), the linear
// magnitudes never leave the library.
size_t rfx_waveform_from_mel_workspace_bytes(const rfx_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T <= 0) return 0;
  const size_t imel = rfx_inverse_mel_workspace_bytes(plan, B, T), gl = rfx_griffinlim_workspace_bytes(plan, B, T);
  if (!imel || !gl) return 0;
  const size_t stride = imel_can_emit_fam_slots(plan) ? (size_t)plan->fam.fsf : (size_t)plan->frame_stride;
  return align_up((size_t)B * T * stride * sizeof(float), 256) + range_table_bytes(B) + (imel > gl ? imel : gl);
}

static int waveform_from_mel_impl(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                                 float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream, const CallOpt& opt);

int rfx_waveform_from_mel(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                          float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  return waveform_from_mel_impl(plan, d_mel, B, T, channels_per_clip, seed, n_iter, momentum, d_wave_out, d_workspace, workspace_bytes, stream, CallOpt{});
}

int rfx_waveform_from_mel_ex(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                             float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream,
                             const rfx_call_options* options) {
  CallOpt opt;
  if (int rc = read_call_options(options, &opt, "rfx_waveform_from_mel_ex")) return rc;
  return waveform_from_mel_impl(plan, d_mel, B, T, channels_per_clip, seed, n_iter, momentum, d_wave_out, d_workspace, workspace_bytes, stream, opt);
}

static int waveform_from_mel_impl(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                                 float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream, const CallOpt& opt) {
  if (!plan || !d_mel || !d_wave_out || !d_workspace || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_waveform_from_mel: bad argument");
  const size_t need = rfx_waveform_from_mel_workspace_bytes(plan, B, T);
  if (!need) return fail(RFX_ERR_UNSUPPORTED, "rfx_waveform_from_mel: this plan cannot invert (see rfx_inverse_mel / rfx_griffinlim)");
  if (workspace_bytes < need) return fail(RFX_ERR_WORKSPACE, "rfx_waveform_from_mel: workspace too small");
  float* lin = reinterpret_cast<float*>(d_workspace);
  // a row-family plan's magnitudes go from the SGD kernel to the Griffin-Lim kernels in THEIR slot order: the once-per-call
  // re-ordering of plain frames (0.75 ms and 2.5 GB of traffic per 64 tiles at 48 kHz) exists only for callers of the two entry points
  const bool fam_slots = imel_can_emit_fam_slots(plan);
  const size_t lin_bytes = align_up((size_t)B * T * (fam_slots ? (size_t)plan->fam.fsf : (size_t)plan->frame_stride) * sizeof(float), 256);
  float* row_scale = reinterpret_cast<float*>((char*)d_workspace + lin_bytes);  // written by the SGD stage's range pass, read by Griffin-Lim
  const size_t head = lin_bytes + range_table_bytes(B);
  void* rest = (char*)d_workspace + head;
  if (int rc = inverse_mel_impl(plan, d_mel, B, T, channels_per_clip, nullptr, seed, lin, rest, workspace_bytes - head, stream, fam_slots, opt, row_scale)) return rc;
  if (!fam_slots) return griffinlim_impl(plan, lin, nullptr, seed + 1, B, T, n_iter, momentum, d_wave_out, rest, workspace_bytes - head, stream, nullptr, opt, row_scale);
  if (T < 2 || n_iter < 0 || (long long)B * T > 0x7fffffffLL || !(momentum >= 0.f && momentum < 1.f)) return fail(RFX_ERR_INVALID, "rfx_waveform_from_mel: bad shape");
  RFX_ON_DEVICE(plan->device);
  return gen_griffinlim(plan, lin, nullptr, seed + 1, B, T, n_iter, momentum, d_wave_out, rest, workspace_bytes - head, (hipStream_t)stream, nullptr, opt, true, row_scale);
}

int rfx_image_decode_u8(const uint8_t* d_img, int N, int H, int W, int stereo, const float* d_lut256, float* d_mel_out,
                        void* stream) {
  if (!d_img || !d_lut256 || !d_mel_out || N <= 0 || H <= 0 || W <= 0) return fail(RFX_ERR_INVALID, "rfx_image_decode_u8: bad argument");
  int dev;
  if (int rc = device_of(d_mel_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_image_decode(d_img, d_lut256, d_mel_out, N, H, W, stereo ? 2 : 1, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_image_encode_u8(const float* d_mel, int N, int M, int T, int stereo, const float* d_thresholds255, float* d_clip_max,
                        uint8_t* d_img_out, void* stream) {
  if (!d_mel || !d_thresholds255 || !d_clip_max || !d_img_out || N <= 0 || M <= 0 || T <= 0)
    return fail(RFX_ERR_INVALID, "rfx_image_encode_u8: bad argument");
  int dev;
  if (int rc = device_of(d_img_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  const int C = stereo ? 2 : 1;
  RFX_HIP(launch_clip_max(d_mel, d_clip_max, N, (size_t)C * M * T, false, (hipStream_t)stream));
  RFX_HIP(launch_image_encode(d_mel, d_clip_max, d_thresholds255, d_img_out, N, M, T, C, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_pcm16(const float* d_wave, int N, int C, int L, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* stream) {
  if (!d_wave || !d_clip_peak || !d_pcm_out || N <= 0 || C <= 0 || L <= 0) return fail(RFX_ERR_INVALID, "rfx_pcm16: bad argument");
  int dev;
  if (int rc = device_of(d_pcm_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  if (normalize) RFX_HIP(launch_clip_max(d_wave, d_clip_peak, N, (size_t)C * L, true, (hipStream_t)stream));
  RFX_HIP(launch_pcm16(d_wave, d_clip_peak, d_pcm_out, N, L, C, normalize, (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_pcm16_filters_workspace_bytes(int N, int L, int C) {
  if (N <= 0 || L <= 0 || C <= 0) return 0;
  return pcm_filters_workspace_bytes(N, L, C);
}

int rfx_pcm16_apply_filters(const int16_t* d_pcm_in, int N, int L, int C, const double* d_gain_by_rms, const double* d_boost_by_peak,
                            int16_t* d_pcm_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_pcm_in || !d_gain_by_rms || !d_boost_by_peak || !d_pcm_out || !d_workspace || N <= 0 || L <= 0 || C <= 0)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters: bad argument");
  if ((int64_t)L * C >= ((int64_t)1 << 23))
    return fail(RFX_ERR_UNSUPPORTED, "rfx_pcm16_apply_filters: L * C >= 2^23 (audioop.rms is exact only below that)");
  if (workspace_bytes < pcm_filters_workspace_bytes(N, L, C)) return fail(RFX_ERR_WORKSPACE, "rfx_pcm16_apply_filters: workspace too small");
  int dev;
  if (int rc = device_of(d_pcm_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_pcm_filters(d_pcm_in, N, L, C, d_gain_by_rms, d_boost_by_peak, d_pcm_out, d_workspace, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_pcm16_stitch(const int16_t* d_pcm, int N, int L, int C, const rfx_stitch_piece* h_pieces, const rfx_stitch_piece* d_pieces,
                     int n_pieces, int64_t out_frames, int16_t* d_out, void* stream) {
  static_assert(sizeof(rfx_stitch_piece) == sizeof(PcmPiece), "rfx_stitch_piece is PcmPiece (rfx_pcm_core.h)");
  if (!d_pcm || !h_pieces || !d_pieces || !d_out || N <= 0 || L <= 0 || C <= 0 || n_pieces <= 0 || out_frames <= 0)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_stitch: bad argument");
  // every read the kernel will make stays inside the batch: checked here, on the host table
  if (h_pieces[0].out_start != 0) return fail(RFX_ERR_INVALID, "rfx_pcm16_stitch: the first piece must start at frame 0");
  for (int k = 0; k < n_pieces; ++k) {
    const rfx_stitch_piece& p = h_pieces[k];
    const int64_t next = k + 1 < n_pieces ? h_pieces[k + 1].out_start : out_frames;
    const int64_t count = next - p.out_start;
    bool ok = count > 0 && (p.kind == 0 || p.kind == 1);
    ok = ok && (p.a_clip < 0 || (p.a_clip < N && p.a_off >= 0 && p.a_off + count <= L));
    ok = ok && (p.kind == 0 || p.b_clip < 0 || (p.b_clip < N && p.b_off >= 0 && p.b_off + count <= L));
    if (!ok) return fail(RFX_ERR_INVALID, "rfx_pcm16_stitch: piece " + std::to_string(k) + " is empty or reads outside the batch");
  }
  int dev;
  if (int rc = device_of(d_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_pcm_stitch(d_pcm, L, C, d_pieces, n_pieces, out_frames, d_out, (hipStream_t)stream));
  return RFX_OK;
}

static bool resize_args_ok(int N, int H, int W, int out_h, int out_w, int filter) {
  const auto in_range = [](int v) { return v >= 1 && v <= kRszMaxSize; };
  return N >= 1 && in_range(H) && in_range(W) && in_range(out_h) && in_range(out_w) && rsz_support(filter) > 0.0;
}

int rfx_image_resize_coefficients(int in_size, int out_size, int filter, int32_t* h_bounds, int32_t* h_kk, int capacity) {
  if (in_size < 1 || in_size > kRszMaxSize || out_size < 1 || out_size > kRszMaxSize || rsz_support(filter) == 0.0)
    return fail(RFX_ERR_INVALID, "rfx_image_resize_coefficients: sizes must be in [1, 16384] and the filter RFX_RESIZE_LANCZOS, "
                                 "_BILINEAR or _BICUBIC");
  const int ksize = rsz_ksize(in_size, out_size, filter);
  if (!h_bounds && !h_kk) return ksize;
  if (!h_bounds || !h_kk) return fail(RFX_ERR_INVALID, "rfx_image_resize_coefficients: h_bounds and h_kk go together");
  if ((int64_t)capacity < (int64_t)out_size * ksize)
    return fail(RFX_ERR_WORKSPACE, "rfx_image_resize_coefficients: h_kk holds fewer than out_size * ksize entries");
  std::vector<double> w(ksize);
  return rsz_coefficients(in_size, out_size, filter, h_bounds, h_kk, w.data());
}

size_t rfx_image_resize_workspace_bytes(int N, int H, int W, int out_h, int out_w, int filter) {
  if (!resize_args_ok(N, H, W, out_h, out_w, filter)) return 0;
  return resize_workspace_bytes(N, H, W, out_h, out_w);
}

int rfx_image_resize_u8(const uint8_t* d_in, int N, int H, int W, int out_h, int out_w, int filter, const int32_t* d_bounds_x,
                        const int32_t* d_kk_x, const int32_t* d_bounds_y, const int32_t* d_kk_y, uint8_t* d_out, void* d_workspace,
                        size_t workspace_bytes, void* stream) {
  if (!d_in || !d_out || !resize_args_ok(N, H, W, out_h, out_w, filter))
    return fail(RFX_ERR_INVALID, "rfx_image_resize_u8: bad argument (N >= 1, sizes in [1, 16384], filter RFX_RESIZE_LANCZOS, "
                                 "_BILINEAR or _BICUBIC)");
  if (out_w != W && (!d_bounds_x || !d_kk_x)) return fail(RFX_ERR_INVALID, "rfx_image_resize_u8: the width changes: need d_bounds_x, d_kk_x");
  if (out_h != H && (!d_bounds_y || !d_kk_y)) return fail(RFX_ERR_INVALID, "rfx_image_resize_u8: the height changes: need d_bounds_y, d_kk_y");
  const size_t need = resize_workspace_bytes(N, H, W, out_h, out_w);
  if (need && (!d_workspace || workspace_bytes < need)) return fail(RFX_ERR_WORKSPACE, "rfx_image_resize_u8: workspace too small");
  int dev;
  if (int rc = device_of(d_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_resize(d_in, N, H, W, out_h, out_w, d_bounds_x, d_kk_x, rsz_ksize(W, out_w, filter), d_bounds_y, d_kk_y,
                        rsz_ksize(H, out_h, filter), d_out, d_workspace, (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_pcm16_compress_filters_workspace_bytes(int N, int L, int C) {
  if (N <= 0 || L <= 0 || C <= 0) return 0;
  return cmp_workspace_layout(N, L, C).total;
}

int rfx_pcm16_apply_filters_compressed(const int16_t* d_pcm_in, int N, int L, int C, rfx_compress_options* o, int16_t* d_pcm_out,
                                       void* d_workspace, size_t workspace_bytes, void* stream) {
  static_assert(sizeof(CmpFlag) == 24, "rfx_compress_options.d_flags entries are CmpFlag (rfx_compress_core.h)");
  if (!d_pcm_in || !o || !d_pcm_out || !d_workspace || N <= 0 || L <= 0 || C <= 0)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: bad argument");
  if (o->struct_size != sizeof(rfx_compress_options))
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: options->struct_size is not sizeof(rfx_compress_options)");
  if (!o->d_gain10_by_rms || !o->d_gain12_by_rms || !o->d_boost_by_peak || !o->d_above || !o->d_max_att || !o->d_inc || !o->d_dec)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: a table is missing");
  if ((o->form != RFX_COMPRESS_SEQUENTIAL && o->form != RFX_COMPRESS_CHUNKED) || o->look_frames < 0 || o->chunk_frames < 0 ||
      !(o->margin >= 0.0) || o->flag_capacity < 0 || (o->flag_capacity > 0 && !o->d_flags))
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: bad option");
  if ((int64_t)L * C >= ((int64_t)1 << 23))
    return fail(RFX_ERR_UNSUPPORTED, "rfx_pcm16_apply_filters_compressed: L * C >= 2^23 (audioop.rms is exact only below that)");
  const CmpLayout w = cmp_workspace_layout(N, L, C);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_pcm16_apply_filters_compressed: workspace too small");
  int dev;
  if (int rc = device_of(d_pcm_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  const hipStream_t s = (hipStream_t)stream;
  RFX_HIP(launch_cmp_compress(d_pcm_in, N, L, C, o->d_boost_by_peak, o->d_gain10_by_rms, o->d_above, o->d_max_att, o->d_inc, o->d_dec,
                              o->look_frames, o->form, o->chunk_frames, o->margin, o->d_flags, o->flag_capacity, o->d_rounds, d_workspace, s));
  // the one synchronisation of this path: how many products need the host's pow
  unsigned long long n = 0;
  RFX_HIP(hipMemcpyAsync(&n, (char*)d_workspace + w.count, sizeof n, hipMemcpyDeviceToHost, s));
  RFX_HIP(hipStreamSynchronize(s));
  o->n_flagged = (int64_t)n;
  if ((int64_t)n > o->flag_capacity) return RFX_OK;  // documented: d_pcm_out is not written, the caller redoes the batch on the host
  int16_t* x3 = reinterpret_cast<int16_t*>((char*)d_workspace + w.x3);
  if (n > 0) {
    std::vector<CmpFlag> h(n);
    RFX_HIP(hipMemcpyAsync(h.data(), o->d_flags, n * sizeof(CmpFlag), hipMemcpyDeviceToHost, s));
    RFX_HIP(hipStreamSynchronize(s));
    const int64_t total = (int64_t)N * L * C;
    for (CmpFlag& f : h) {
      if (f.index < 0 || f.index >= total) return fail(RFX_ERR_HIP, "rfx_pcm16_apply_filters_compressed: corrupt flag list");
      f.value = pcm_mul(f.x2, cmp_gain_host(f.att));
    }
    RFX_HIP(hipMemcpyAsync(o->d_flags, h.data(), n * sizeof(CmpFlag), hipMemcpyHostToDevice, s));
    RFX_HIP(launch_cmp_scatter(o->d_flags, (int64_t)n, x3, s));
    RFX_HIP(hipStreamSynchronize(s));  // h is released on return
  }
  RFX_HIP(launch_pcm_filters(x3, N, L, C, o->d_gain12_by_rms, o->d_boost_by_peak, d_pcm_out, (char*)d_workspace + w.filters, s));
  return RFX_OK;
}

// ---- SpectrogramImageConverter.audio_from_spectrogram_image's device half in one call (spectrogram_image_converter.py:54-91:
// image_util.spectrogram_from_image, SpectrogramConverter.audio_from_spectrogram -> waveform_from_mel_amplitudes on the image's
// (C, n_mels, T) tensor, audio_util.audio_from_waveform): uint8 tiles in, int16 PCM out.  The three entry points it is made of,
// in their order, with the same seeds: same bytes.
size_t rfx_audio_from_image_workspace_bytes(const rfx_plan* plan, int N, int stereo, int T) {
  if (!plan || N <= 0 || T <= 0) return 0;
  const int C = stereo ? 2 : 1, B = N * C;
  const size_t inner = rfx_waveform_from_mel_workspace_bytes(plan, B, T);
  if (!inner) return 0;
  return align_up((size_t)B * plan->p.n_mels * T * sizeof(float), 256) + align_up((size_t)B * rfx_griffinlim_output_samples(plan, T) * sizeof(float), 256) + inner;
}

static int audio_from_image_impl(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                                int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                                size_t workspace_bytes, void* stream, const CallOpt& opt);

int rfx_audio_from_image_u8(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                            int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  return audio_from_image_impl(plan, d_img, N, T, stereo, d_lut256, seed, n_iter, momentum, normalize, d_clip_peak, d_pcm_out, d_workspace,
                               workspace_bytes, stream, CallOpt{});
}

int rfx_audio_from_image_u8_ex(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                               int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                               size_t workspace_bytes, void* stream, const rfx_call_options* options) {
  CallOpt opt;
  if (int rc = read_call_options(options, &opt, "rfx_audio_from_image_u8_ex")) return rc;
  return audio_from_image_impl(plan, d_img, N, T, stereo, d_lut256, seed, n_iter, momentum, normalize, d_clip_peak, d_pcm_out, d_workspace,
                               workspace_bytes, stream, opt);
}

static int audio_from_image_impl(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                                int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                                size_t workspace_bytes, void* stream, const CallOpt& opt) {
  if (!plan || !d_img || !d_lut256 || !d_clip_peak || !d_pcm_out || !d_workspace || N <= 0 || T <= 0)
    return fail(RFX_ERR_INVALID, "rfx_audio_from_image_u8: bad argument");
  const size_t need = rfx_audio_from_image_workspace_bytes(plan, N, stereo, T);
  if (!need) return fail(RFX_ERR_UNSUPPORTED, "rfx_audio_from_image_u8: this plan cannot invert (see rfx_inverse_mel / rfx_griffinlim)");
  if (workspace_bytes < need) return fail(RFX_ERR_WORKSPACE, "rfx_audio_from_image_u8: workspace too small");
  const int C = stereo ? 2 : 1, B = N * C, M = plan->p.n_mels, L = rfx_griffinlim_output_samples(plan, T);
  float* mel = reinterpret_cast<float*>(d_workspace);
  const size_t mel_bytes = align_up((size_t)B * M * T * sizeof(float), 256), wave_bytes = align_up((size_t)B * L * sizeof(float), 256);
  float* wave = reinterpret_cast<float*>((char*)d_workspace + mel_bytes);
  void* rest = (char*)d_workspace + mel_bytes + wave_bytes;
  if (int rc = rfx_image_decode_u8(d_img, N, M, T, stereo, d_lut256, mel, stream)) return rc;
  // (a clip is one image: its channels share the SGD loss mean and the peak normalisation)
  if (int rc = waveform_from_mel_impl(plan, mel, B, T, C, seed, n_iter, momentum, wave, rest, workspace_bytes - mel_bytes - wave_bytes, stream, opt)) return rc;
  return rfx_pcm16(wave, N, C, L, normalize, d_clip_peak, d_pcm_out, stream);
}

}  // extern "C"
