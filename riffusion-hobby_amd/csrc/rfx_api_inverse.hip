// rfx_api_inverse.hip - the C ABI of librfx.so (include/rfx.h), inverse half: Griffin-Lim on the three frame engines,
// InverseMelScale, and the fused calls made of them.  Host code only: the drivers that sequence the kernels.
#include <algorithm>

#include "rfx_api.h"
#include "rfx_guide_core.h"
#include "rfx_holdmask_core.h"
#include "rfx_imel_lstsq_core.h"
#include "rfx_loop_core.h"
#include "rfx_peak_core.h"

using namespace rfx;

namespace {
// Per-launch times of a Griffin-Lim call, from HIP events recorded on the launch stream (bench.py's roofline leg).  Without an
// array to fill every member does nothing and nothing is allocated; the events are released on every exit path.
class LaunchTimer {
  float* h_ms_;
  int n_;  // launches: n_ + 1 events
  bool begun_ = false;
  std::vector<hipEvent_t> ev_;

 public:
  LaunchTimer(float* h_launch_ms, int n_launches) : h_ms_(h_launch_ms), n_(n_launches) {}
  ~LaunchTimer() {
    for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
  }
  LaunchTimer(const LaunchTimer&) = delete;
  LaunchTimer& operator=(const LaunchTimer&) = delete;
  hipError_t begin(hipStream_t stream) {
    if (!h_ms_ || begun_) return hipSuccess;  // (a call with the spectral-peak start begins before its start; the engine's begin then does nothing)
    begun_ = true;
    ev_.reserve((size_t)n_ + 1);
    for (int i = 0; i <= n_; ++i) {
      hipEvent_t e;
      const hipError_t rc = hipEventCreate(&e);
      if (rc != hipSuccess) return rc;
      ev_.push_back(e);
    }
    return hipEventRecord(ev_[0], stream);
  }
  hipError_t mark(int launch, hipStream_t stream) { return h_ms_ ? hipEventRecord(ev_[launch + 1], stream) : hipSuccess; }
  hipError_t finish() {  // waits for the last marked launch
    if (!h_ms_) return hipSuccess;
    hipError_t rc = hipEventSynchronize(ev_[n_]);
    for (int i = 0; i < n_ && rc == hipSuccess; ++i) rc = hipEventElapsedTime(&h_ms_[i], ev_[i], ev_[i + 1]);
    return rc;
  }
};
}  // namespace

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
hipError_t launch_gl_out_scale(const float* win, float* out, int T, int L, hipStream_t stream) {
  hipLaunchKernelGGL(out_scale_kernel, dim3((L + 255) / 256), dim3(256), 0, stream, win, out, T, L);
  return hipGetLastError();
}
}  // namespace rfx

static long long gl_slot_count(const rfx_plan* plan) { return (long long)plan->num_cus * plan->gl_wgs_per_cu; }
// [B][2] floats of scales + [B] key words (launch_range_scale)
static size_t range_table_bytes(int B) { return (size_t)B * 3 * sizeof(float); }

// ---- Griffin-Lim ----------------------------------------------------------------------------------------------------------------
// Small batches take the per-frame kernels (rfx_gl.hip: gl_frame_kernel + gl_fold_kernel): up to gl_latency_frames_per_slot (six)
// frames per resident workgroup slot, and one stair further (below), where the run-based kernel (whole groups of 16 frames per
// workgroup) would leave most of the chip idle.
static bool gl_use_latency_mode(const rfx_plan* plan, int B, int T) {
  if (plan->gl_form == RFX_GL_FORM_RUNS) return false;
  if (plan->gl_form == RFX_GL_FORM_FRAMES) return true;
  if (!plan->gl_latency_mode) return false;
  const long long nframes = (long long)B * T, slots = gl_slot_count(plan);
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
static GlPartition gl_partition(const rfx_plan* plan, int B, int T) { return gl_partition_for(gl_slot_count(plan), B, T); }
static int report_run_starts(const GlPartition& p, int B, int T, int64_t* run_starts, int capacity) {
  if (run_starts)
    for (int b = 0; b <= p.runs && b < capacity; ++b) run_starts[b] = rfx::gl_run_start_frame(b, p.runs, B, T, p.h, p.w1, p.w2);
  return p.runs;
}

// (`which` selected a per-launch skew until round 6; every launch of a call has the same partition now)
int rfx_griffinlim_runs(const rfx_plan* plan, int B, int T, int which, int64_t* run_starts, int capacity) {
  (void)which;
  if (!plan || B <= 0 || T < 2 || plan->generic) return 0;
  return report_run_starts(gl_partition(plan, B, T), B, T, run_starts, capacity);
}

int64_t rfx_debug_run_start(int64_t b, int64_t runs, int64_t n_frames, int64_t h, int64_t w1, int64_t w2) {
  return rfx::gl_run_start(b, runs, n_frames, h, w1, w2);
}

int rfx_debug_gl_partition(int slots, int B, int T, int64_t* run_starts, int capacity) {
  if (slots <= 0 || B <= 0 || T < 2) return 0;
  return report_run_starts(gl_partition_for(slots, B, T), B, T, run_starts, capacity);
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

// Specialised engine: three generations (x_{k-1}, x_k, x_{k+1}) of the run form's two audio buffers (rfx_gl.hip), the istft normalisation table,
// the synthesis frames of the per-frame form, and the call's own row-scale table (GlArgs::row_scale).  No spectral state is kept
// between iterations (see rfx_gl.hip).  held (a call with rfx_held_call_options.d_hold_frames): always the per-frame form and its frame
// buffer, and the free-frame list behind everything an unheld call has.  masked (rfx_masked_call_options.d_hold_bins): the
// per-frame form as well, and behind everything else the second magnitude array X and the constant audio c (rfx_holdmask_core.h).
// loop (rfx_loop_call_options.loop): the per-frame form, audio rows of the period's hop T samples, and the hop-entry reciprocal envelope
// where the unlooped call keeps its normalisation table; no layout (total 0) for a T the call refuses.
enum GlKind { kGlPlain = 0, kGlHeld = 1, kGlMasked = 2, kGlLoop = 3 };
// One struct for both engines (`scale`: the specialised engine only; `repacked`: the generic one only).  peak (a call with
// rfx_start_call_options.start): behind everything the call has without it, the start's angles and scratch (rfx_api_peak.hip).
struct GlLayout {
  size_t audio, scale, frames, repacked, row_scale, list, xmag, cadd, angles, peak_scratch, total;
  int Lpad;
};
static size_t hold_list_bytes(int B, int T) { return hold_list_words(B, T) * sizeof(int32_t); }
// the fields every kind has at its end, in both engines
static void carve_gl_tail(Carve& c, GlLayout& l, const rfx_plan* plan, int B, int T, GlKind kind, bool peak, size_t xmag_stride) {
  l.row_scale = c.take(range_table_bytes(B));
  l.list = c.take(kind == kGlHeld ? hold_list_bytes(B, T) : 0);
  l.xmag = c.take(kind == kGlMasked ? (size_t)B * T * xmag_stride * sizeof(float) : 0);
  l.cadd = c.take(kind == kGlMasked ? (size_t)B * l.Lpad * sizeof(float) : 0);
  l.angles = c.take(peak ? peak_angles_bytes(plan, B, T) : 0);
  l.peak_scratch = c.take(peak ? peak_scratch_bytes(plan, B, T) : 0);
  l.total = c.at;
}
static GlLayout gl_layout(const rfx_plan* plan, int B, int T, GlKind kind, bool peak) {
  const bool loop = kind == kGlLoop;
  GlLayout l{};
  if (B <= 0 || T < 2) return l;
  if (loop && !loop_valid(kHop, T, kNfft)) return l;
  l.Lpad = (int)align_up((size_t)kHop * (loop ? T : T - 1), 64);
  Carve c;
  l.audio = c.take(6 * (size_t)B * l.Lpad * sizeof(float));
  l.scale = c.take((size_t)l.Lpad * sizeof(float));
  l.frames = c.take(kind != kGlPlain || gl_use_latency_mode(plan, B, T) ? gl_frame_buffer_bytes(B, T) : 0);
  carve_gl_tail(c, l, plan, B, T, kind, peak, kFrameStride);
  return l;
}

// torch.istft(center=True, length=None) returns n_fft + hop*(T-1) - 2*(n_fft/2) samples: hop*(T-1), plus one when n_fft is odd
static int gen_out_len(const GenGeom& g, int T) { return g.hop * (T - 1) + (g.n_fft & 1); }

// Generic engine: the windowed synthesis frames, three generations of the audio estimate (x_{k-1}, x_k read; x_{k+1} written) and
// the window envelope of the fold, [Lpad]; on a row family the magnitudes re-ordered into slot order; the row-scale table; held: the
// free-frame list; masked: X (in the order the frame kernels read: the family's slot order on a row family) and c
static GlLayout gen_gl_layout(const rfx_plan* plan, int B, int T, GlKind kind, bool peak) {
  const bool loop = kind == kGlLoop;
  GlLayout l{};
  if (B <= 0 || T < 2) return l;
  const GenGeom& g = plan->gg;
  if (loop && (plan->czt || !loop_valid(g.hop, T, g.n_fft))) return l;
  const size_t nf = (size_t)B * T;
  l.Lpad = (int)align_up(loop ? (size_t)g.hop * T : (size_t)gen_out_len(g, T), 64);
  Carve c;
  l.frames = c.take(nf * g.fpitch * sizeof(float));
  l.audio = c.take((3 * (size_t)B + 1) * l.Lpad * sizeof(float));
  l.repacked = c.take(plan->fam_ok ? nf * plan->fam.fsf * sizeof(float) : 0);
  carve_gl_tail(c, l, plan, B, T, kind, peak, plan->fam_ok ? (size_t)plan->fam.fsf : (size_t)g.fs);
  return l;
}
static GlLayout griffinlim_layout(const rfx_plan* plan, int B, int T, GlKind kind, bool peak) {
  return plan->generic ? gen_gl_layout(plan, B, T, kind, peak) : gl_layout(plan, B, T, kind, peak);
}
int rfx_griffinlim_loop_output_samples(const rfx_plan* plan, int T) {
  if (!plan || T <= 0 || (long long)plan->p.hop_length * T > 0x7fffffffLL) return 0;
  return plan->p.hop_length * T;
}
// samples per row of a call
static int gl_out_samples(const rfx_plan* plan, int T, bool loop) {
  return loop ? rfx_griffinlim_loop_output_samples(plan, T) : rfx_griffinlim_output_samples(plan, T);
}

// rfx_call_options as the entry points below see them (NULL / short struct = defaults)
struct CallOpt {
  uint64_t row_base = 0;
  float magnitude_hint = 0.f;
  bool lstsq = false;  // RFX_CALL_INVERSE_MEL_LSTSQ (the fused calls)
  // rfx_guided_call_options: the guide waveforms of a guided Griffin-Lim start (null: the start is drawn or injected)
  const float* guide = nullptr;
  int64_t guide_stride = 0;
  int guide_samples = 0;
  // rfx_held_call_options: (B, 2) {head, tail} of the frames held at the guide's phase (null: a guided call holds nothing)
  const int32_t* hold = nullptr;
  // rfx_masked_call_options: (B, T, mask_words) bit mask of the bins held at the guide's phase (null: no bins held)
  const uint32_t* mask = nullptr;
  int mask_words = 0;
  // rfx_loop_call_options: the row's T columns are one period of a loop (rfx_loop_core.h)
  bool loop = false;
  // rfx_start_call_options: Griffin-Lim starts from the spectral-peak phases of the call's magnitudes (rfx_peak_core.h)
  bool peak = false;
  GlKind kind() const { return loop ? kGlLoop : mask ? kGlMasked : hold ? kGlHeld : kGlPlain; }
};
// The grown tails of rfx_call_options, in the order they were added (each is the same struct, grown; a caller that passes a
// shorter size has none of the later ones)
enum { kTailGuide, kTailHold, kTailMask, kTailLoop, kTailStart, kTails };
struct TailRead {
  const char* bad = nullptr;      // a reserved field or a range: refused whether or not the option is set
  bool set = false;
  const char* bad_set = nullptr;  // of an option that is set: its pointer's alignment, the guide's geometry
};
// why an entry point that runs no Griffin-Lim refuses a tail that is set
static const char* const kNoGriffinLim[kTails] = {
    "takes no guide (d_guide must be NULL)", "holds no frames (d_hold_frames must be NULL)", "holds no bins (d_hold_bins must be NULL)",
    "decodes no loop (loop must be 0)", "takes no start (start must be 0)"};
// The combination rules: what the option of `tail` does not go with, among the options read before it
static const char* rule_refusal(int tail, const CallOpt& o) {
  switch (tail) {
    case kTailHold:
      if (!o.guide) return "d_hold_frames needs a guide to hold the frames at (d_guide is NULL)";
      break;
    case kTailMask:
      if (!o.guide) return "d_hold_bins needs a guide to hold the bins at (d_guide is NULL)";
      if (o.hold) return "d_hold_bins together with d_hold_frames is not served: set the held frames' bits in the mask";
      break;
    case kTailLoop:
      if (o.hold || o.mask) return "loop together with d_hold_frames or d_hold_bins is not served";
      break;
    case kTailStart:
      if (o.mask) return "start == 1 together with d_hold_bins is not served (bins are held at a guide's phase)";
      if (o.hold) return "start == 1 together with d_hold_frames is not served (frames are held at a guide's phase)";
      if (o.guide) return "start == 1 and d_guide are two starts: give one";
      break;
  }
  return nullptr;
}
template <class Tail, class Field>
static const Tail* tail_of(const rfx_call_options* o, Field Tail::*last) {  // null: the caller's struct ends before `last`
  const Tail* t = reinterpret_cast<const Tail*>(o);
  return o->struct_size >= (size_t)((const char*)&(t->*last) - (const char*)t) + sizeof(Field) ? t : nullptr;
}
// allowed_flags: the RFX_CALL_* bits this entry point reads (0 for the two stages themselves); runs_gl: it runs Griffin-Lim
static int read_call_options(const rfx_call_options* o, CallOpt* out, const char* who, uint32_t allowed_flags = 0, bool runs_gl = false) {
  *out = CallOpt{};
  if (!o) return RFX_OK;
  if (o->struct_size < offsetof(rfx_call_options, row_base) + sizeof(uint64_t))
    return fail(RFX_ERR_INVALID, std::string(who) + ": rfx_call_options.struct_size is not set");
  if (o->flags & ~allowed_flags)
    return fail(RFX_ERR_INVALID, std::string(who) + (allowed_flags ? ": rfx_call_options.flags has a bit this entry point does not know"
                                                                   : ": rfx_call_options.flags must be 0"));
  out->lstsq = (o->flags & RFX_CALL_INVERSE_MEL_LSTSQ) != 0;
  out->row_base = o->row_base;
  if (o->struct_size >= offsetof(rfx_call_options, magnitude_hint) + sizeof(float)) out->magnitude_hint = o->magnitude_hint;
  if (!(out->magnitude_hint >= 0.f) || out->magnitude_hint > 3.0e38f)
    return fail(RFX_ERR_INVALID, std::string(who) + ": rfx_call_options.magnitude_hint must be a finite value >= 0");
  if (o->struct_size >= offsetof(rfx_call_options, reserved) + sizeof(float) && !(o->reserved == 0.f))
    return fail(RFX_ERR_INVALID, std::string(who) + ": rfx_call_options.reserved must be 0");
  TailRead tails[kTails];
  if (const auto* g = tail_of(o, &rfx_guided_call_options::reserved2)) {
    TailRead& t = tails[kTailGuide];
    if (g->reserved2 != 0) t.bad = "rfx_guided_call_options.reserved2 must be 0";
    if ((t.set = g->d_guide != nullptr)) {
      t.bad_set = g->guide_samples <= 0                           ? "guide_samples must be positive when d_guide is given"
                  : g->guide_stride < (int64_t)g->guide_samples   ? "guide_stride (elements between rows) must be at least guide_samples"
                  : (uintptr_t)g->d_guide & (sizeof(float) - 1)   ? "d_guide must be aligned to 4 bytes"
                                                                  : nullptr;
      out->guide = g->d_guide;
      out->guide_stride = g->guide_stride;
      out->guide_samples = g->guide_samples;
    }
  }
  if (const auto* h = tail_of(o, &rfx_held_call_options::reserved3)) {
    TailRead& t = tails[kTailHold];
    if (h->reserved3 != 0) t.bad = "rfx_held_call_options.reserved3 must be 0";
    if ((t.set = h->d_hold_frames != nullptr)) {
      if ((uintptr_t)h->d_hold_frames & (sizeof(int32_t) - 1)) t.bad_set = "d_hold_frames must be aligned to 4 bytes";
      out->hold = h->d_hold_frames;
    }
  }
  if (const auto* m = tail_of(o, &rfx_masked_call_options::reserved4)) {
    TailRead& t = tails[kTailMask];
    if (m->reserved4 != 0) t.bad = "rfx_masked_call_options.reserved4 must be 0";
    if ((t.set = m->d_hold_bins != nullptr)) {
      if ((uintptr_t)m->d_hold_bins & (sizeof(uint32_t) - 1)) t.bad_set = "d_hold_bins must be aligned to 4 bytes";
      out->mask = m->d_hold_bins;
      out->mask_words = m->hold_words;
    }
  }
  if (const auto* l = tail_of(o, &rfx_loop_call_options::reserved5)) {
    TailRead& t = tails[kTailLoop];
    t.bad = l->reserved5 != 0 ? "rfx_loop_call_options.reserved5 must be 0" : l->loop > 1 ? "rfx_loop_call_options.loop must be 0 or 1" : nullptr;
    t.set = out->loop = l->loop != 0;
  }
  if (const auto* st = tail_of(o, &rfx_start_call_options::reserved6)) {
    TailRead& t = tails[kTailStart];
    t.bad = st->reserved6 != 0 ? "rfx_start_call_options.reserved6 must be 0" : st->start > 1 ? "rfx_start_call_options.start must be 0 or 1" : nullptr;
    t.set = out->peak = st->start != 0;
  }
  // the refusals, tail after tail: a reserved field or a range; then, of an option that is set, an entry point that runs no
  // Griffin-Lim, the combination rules, the option's own pointer
  for (int i = 0; i < kTails; ++i) {
    const TailRead& t = tails[i];
    if (t.bad) return fail(RFX_ERR_INVALID, std::string(who) + ": " + t.bad);
    if (!t.set) continue;
    if (!runs_gl) return fail(RFX_ERR_INVALID, std::string(who) + ": this entry point runs no Griffin-Lim and " + kNoGriffinLim[i]);
    const char* why = rule_refusal(i, *out);
    if (!why) why = t.bad_set;
    if (why) return fail(RFX_ERR_INVALID, std::string(who) + ": " + why);
  }
  return RFX_OK;
}

// One checked Griffin-Lim call, as every engine and form is given it
struct GlCall {
  const float* S;
  const cf* angles0;
  const float* row_scale;  // null: the driver fills the table of its own workspace (gl_row_scale)
  float mom;
  uint64_t seed;
  int B, T, L, n_iter;
  float* out;
  char* ws;
  hipStream_t stream;
  // the call's extras.  guide: launch 0 is MODE 1 on the staged guide (rfx_guide.hip).  hold: launches 1 .. n_iter walk the
  // free-frame list (rfx_guide_core.h) and leave the held frames' synthesis frames as launch 0 wrote them.  mask: launches
  // 1 .. n_iter read S_free and every fold adds c = ISTFT(S_held a0).  loop: L = hop T is the row's period: launches that read
  // audio read it modulo L, every fold is circular (rfx_loop_core.h)
  CallOpt x;
};
// ... and the fields that all four argument blocks have
template <class Args>
static void set_gl_args(Args& a, const GlCall& c) {
  a.S = c.S;
  a.angles0 = c.angles0;
  a.row_scale = c.row_scale;
  a.mom = c.mom;
  a.seed = c.seed;
  a.frame_base = c.x.row_base * (uint64_t)c.T;
  a.B = c.B;
  a.T = c.T;
  a.L = c.L;
}
// numeric range of the rows: from the caller's hint, else from the magnitudes themselves (one pass over them).  A fused call
// brings the table its SGD stage wrote.
static int gl_row_scale(GlCall& c, size_t per_row, float* table) {
  if (c.row_scale) return RFX_OK;
  RFX_HIP(launch_range_scale(c.S, per_row, c.B, c.x.magnitude_hint, (unsigned*)(table + 2 * (size_t)c.B), nullptr, table, 1, 0, c.stream));
  c.row_scale = table;
  return RFX_OK;
}

// A guided call's staging, after the row-scale table is written and before launch 0: the fitted, ranged guide into `dst`, the
// buffer launch 0 analyses (Lpad floats per row), zeros into `zero` (the run form's other parity buffer; else null).  `peaks`: any
// audio buffer of the call that launch 0 neither reads nor writes.  pre_scaled: the engine's kernels analyse their buffer as it is
// (the fold applies row_scale[2 r]); the specialised engine's multiply by it, and the staged values are divided by it.
static int gl_stage_guide(const GlCall& c, int Lpad, bool pre_scaled, float* peaks, float* dst, float* zero) {
  RFX_HIP(launch_guide_stage(c.x.guide, c.x.guide_stride, c.x.guide_samples, c.B, c.L, Lpad, pre_scaled ? nullptr : c.row_scale, peaks, dst, zero, c.stream));
  return RFX_OK;
}

// Generic engine and row family: a frame kernel, then the fold, per iteration.
// mag_in_fam_slots (rfx_waveform_from_mel on a row-family plan): c.S already holds the family kernels' slot order [B*T][fsf] -
// InverseMelScale wrote it that way - so the once-per-call re-ordering of the plain frames is left out
static int gen_griffinlim(const rfx_plan* plan, GlCall& c, const GlLayout& w, bool mag_in_fam_slots, LaunchTimer& timer) {
  const GenGeom& g = plan->gg;
  const int B = c.B, T = c.T, L = c.L;
  const bool fam = plan->fam_ok;
  float* frames = (float*)(c.ws + w.frames);
  float* gen[3];
  for (int i = 0; i < 3; ++i) gen[i] = (float*)(c.ws + w.audio) + (size_t)i * B * w.Lpad;
  float* env = (float*)(c.ws + w.audio) + (size_t)3 * B * w.Lpad;
  const size_t per_row = (size_t)T * ((fam && mag_in_fam_slots) ? (size_t)plan->fam.fsf : (size_t)g.fs);
  if (int rc = gl_row_scale(c, per_row, (float*)(c.ws + w.row_scale))) return rc;
  // (a loop call keeps the hop-entry reciprocal circular envelope there)
  if (c.x.loop) RFX_HIP(launch_loop_renv(plan->d_win, env, g.n_fft, g.win, g.hop, 1.f, c.stream));
  else RFX_HIP(launch_gen_env(plan->d_win, env, g, T, L, c.stream));
  // padded frame rows (gen_frame_layout): the kernels write the window samples only, the fold reads the padding as zeros
  if (g.fshift > 0) RFX_HIP(hipMemsetAsync(frames, 0, (size_t)B * T * g.fpitch * sizeof(float), c.stream));
  RFX_HIP(timer.begin(c.stream));
  // x_it lives in gen[it % 2]; gen[2] holds d_it = x_it - m x_{it-1} (d_0 = x_0), the momentum term of the reference's
  // `rebuilt - m * tprev` applied in the time domain: the fold of iteration it forms it next to x_it and launch it + 1 analyses it,
  // so the kernels run their one-signal mode for every iteration (half the audio loads, same bits); it == 0 synthesises the
  // initial estimate from S * angles0 - or, guided, analyses the staged guide in gen[2] like any later launch (gen[1] is free until
  // the fold of launch 1: the staging's scratch)
  if (c.x.guide)
    if (int rc = gl_stage_guide(c, w.Lpad, true, gen[1], gen[2], nullptr)) return rc;
  // held: nothing but the frame kernels writes `frames` from here on (the fold reads them), so what launch 0 writes for a held frame
  // is what every later fold reads
  int* list = (int*)(c.ws + w.list);
  if (c.x.hold) RFX_HIP(launch_hold_list(c.x.hold, B, T, list, c.stream));
  FamGlArgs fa{};
  GenGlArgs ga{};
  int nblocks = 0;
  if (fam) {
    const FamGeom& f = plan->fam;
    if (!mag_in_fam_slots) {
      float* repacked = (float*)(c.ws + w.repacked);
      RFX_HIP(launch_fam_repack(c.S, repacked, plan->d_fam_binof, (long long)B * T, g.fs, f.fsf, f.n_stft, c.stream));
      c.S = repacked;
    }
    set_gl_args(fa, c);
    fa.g = f;
    fa.fs_plain = g.fs;
    fa.x_cur = gen[2];
    fa.audio_stride = (size_t)w.Lpad;
    fa.frames = frames;
    fa.fpitch = g.fpitch;
    fa.fshift = g.fshift;
    fa.tw1 = plan->d_fam_tw;
    fa.twa = plan->d_fam_tw + (size_t)f.rows * f.h;
    fa.win = plan->d_win;
    nblocks = frame_blocks(fam_slot_count(plan), B, T);
  } else {
    set_gl_args(ga, c);
    ga.g = g;
    ga.tb = plan->gt;
    ga.x_cur = gen[2];
    ga.audio_stride = (size_t)w.Lpad;
    ga.frames = frames;
  }
  // masked (rfx_holdmask_core.h): X = S_held, one more MODE 1 launch on the staged guide and its fold give c = ISTFT(S_held a0) in the
  // generations' units; launch 0 then runs on the full S as a guided call's does (the same bytes), and launches 1 .. n_iter on
  // X = S_free, every fold adding c before it stores x and forms d.  The split acts on the order the frame kernels read.
  const bool masked = c.x.mask && c.n_iter > 0;
  float* X = (float*)(c.ws + w.xmag);
  float* cadd = (float*)(c.ws + w.cadd);
  const int x_layout = fam ? kHoldMaskTable : kHoldMaskPlain, x_stride = fam ? plan->fam.fsf : g.fs;
  auto set_S = [&](const float* S) { fa.S = ga.S = S; };
  if (masked) {
    RFX_HIP(launch_holdmask_split(x_layout, c.S, X, c.x.mask, plan->d_fam_binof, B, T, x_stride, plan->n_stft, true, c.stream));
    set_S(X);
    RFX_HIP(fam         ? launch_fam_gl(1, fa, nblocks, c.stream)
            : plan->czt ? launch_czt_gl(1, ga, plan->d_czt_c, plan->d_czt_h, plan->num_cus, c.stream)
                        : launch_gen_gl(1, ga, plan->num_cus, c.stream));
    RFX_HIP(launch_gen_fold(frames, env, cadd, g, B, T, L, (size_t)w.Lpad, c.stream));
    set_S(c.S);
  }
  for (int it = 0; it <= c.n_iter; ++it) {
    const int mode = it == 0 && !c.x.guide ? 0 : 1;
    if (masked && it == 1) {
      RFX_HIP(launch_holdmask_split(x_layout, c.S, X, c.x.mask, plan->d_fam_binof, B, T, x_stride, plan->n_stft, false, c.stream));
      set_S(X);
    }
    if (c.x.hold && it > 0)
      RFX_HIP(fam         ? launch_fam_gl_list(fa, list, nblocks, c.stream)
              : plan->czt ? launch_czt_gl_list(ga, list, plan->d_czt_c, plan->d_czt_h, plan->num_cus, c.stream)
                          : launch_gen_gl_list(ga, list, plan->num_cus, c.stream));
    else if (c.x.loop && mode == 1)  // (never a chirp-z plan: refused before the driver)
      RFX_HIP(fam ? launch_fam_gl_loop(fa, nblocks, c.stream) : launch_gen_gl_loop(ga, plan->num_cus, c.stream));
    else
      RFX_HIP(fam         ? launch_fam_gl(mode, fa, nblocks, c.stream)
              : plan->czt ? launch_czt_gl(mode, ga, plan->d_czt_c, plan->d_czt_h, plan->num_cus, c.stream)
                          : launch_gen_gl(mode, ga, plan->num_cus, c.stream));
    const bool last = it == c.n_iter;
    if (c.x.loop)
      RFX_HIP(launch_gen_loop_fold(frames, env, last ? c.out : gen[it % 2], g, B, T, last ? (size_t)L : (size_t)w.Lpad, c.stream,
                                   it == 0 ? nullptr : gen[(it + 1) % 2], last ? nullptr : gen[2], c.mom, c.row_scale));
    else
      RFX_HIP(launch_gen_fold(frames, env, last ? c.out : gen[it % 2], g, B, T, L, last ? (size_t)L : (size_t)w.Lpad, c.stream,
                              it == 0 ? nullptr : gen[(it + 1) % 2], last ? nullptr : gen[2], c.mom, c.row_scale,
                              masked && it > 0 ? cadd : nullptr, (size_t)w.Lpad));
    RFX_HIP(timer.mark(it, c.stream));
  }
  RFX_HIP(timer.finish());
  return RFX_OK;
}

// Specialised engine: the per-frame form (frame kernel + fold per iteration) or the run form (one kernel per iteration)
static int spec_griffinlim(const rfx_plan* plan, GlCall& c, const GlLayout& w, LaunchTimer& timer) {
  const int B = c.B, T = c.T, L = c.L;
  float* gen[3][2];  // x_k lives in generation k % 3
  for (int i = 0; i < 3; ++i)
    for (int p = 0; p < 2; ++p) gen[i][p] = (float*)(c.ws + w.audio) + (size_t)(2 * i + p) * B * w.Lpad;
  float* scale = (float*)(c.ws + w.scale);
  // (a loop call keeps the hop-entry table (2 / N) / env of the circular envelope there)
  if (c.x.loop) RFX_HIP(launch_loop_renv(plan->d_win, scale, kNfft, kWin, kHop, 2.0f / (float)kNfft, c.stream));
  else {
    hipLaunchKernelGGL(out_scale_kernel, dim3((L + 255) / 256), dim3(256), 0, c.stream, plan->d_win, scale, T, L);
    RFX_HIP(hipGetLastError());
  }
  if (int rc = gl_row_scale(c, (size_t)T * kFrameStride, (float*)(c.ws + w.row_scale))) return rc;

  if (c.x.kind() != kGlPlain || gl_use_latency_mode(plan, B, T)) {  // one folded buffer per generation: gen[k][0]
    GlFrameArgs fa;
    set_gl_args(fa, c);
    fa.frames = (float*)(c.ws + w.frames);
    fa.tw1 = plan->d_tw1;
    fa.tw2 = plan->d_tw2;
    fa.win = plan->d_win;
    fa.Lpad = w.Lpad;
    const int nblocks = frame_blocks(gl_slot_count(plan), B, T);
    RFX_HIP(timer.begin(c.stream));
    // guided: launch 0 is MODE 1 on the guide, staged where it reads its input (gen[2][0]; gen[1][0] is free until launch 1's fold)
    if (c.x.guide)
      if (int rc = gl_stage_guide(c, w.Lpad, false, gen[1][0], gen[2][0], nullptr)) return rc;
    // held: only the frame kernel writes fa.frames; launches 1 .. n_iter skip the held frames, whose entries stay launch 0's
    int* list = (int*)(c.ws + w.list);
    if (c.x.hold) RFX_HIP(launch_hold_list(c.x.hold, B, T, list, c.stream));
    // masked: as in gen_griffinlim - c from X = S_held and the staged guide, launch 0 on S, launches 1 .. n_iter on X = S_free, + c in every fold
    const bool masked = c.x.mask && c.n_iter > 0;
    float* X = (float*)(c.ws + w.xmag);
    float* cadd = (float*)(c.ws + w.cadd);
    if (masked) {
      RFX_HIP(launch_holdmask_split(kHoldMaskSpec, c.S, X, c.x.mask, nullptr, B, T, kFrameStride, kBins, true, c.stream));
      fa.S = X;
      fa.audio_in = gen[2][0];
      fa.audio_prev = gen[1][0];
      RFX_HIP(launch_gl_frame(1, fa, nblocks, c.stream));
      RFX_HIP(launch_gl_fold(fa.frames, plan->d_win, scale, cadd, B, T, L, (size_t)w.Lpad, c.stream));
      fa.S = c.S;
    }
    for (int it = 0; it <= c.n_iter; ++it) {
      if (masked && it == 1) {
        RFX_HIP(launch_holdmask_split(kHoldMaskSpec, c.S, X, c.x.mask, nullptr, B, T, kFrameStride, kBins, false, c.stream));
        fa.S = X;
      }
      fa.audio_in = gen[(it + 2) % 3][0];    // x_{it-1}
      fa.audio_prev = gen[(it + 1) % 3][0];  // x_{it-2}
      const int mode = it == 0 ? (c.x.guide ? 1 : 0) : it == 1 ? 1 : 2;
      if (c.x.hold && it > 0) RFX_HIP(launch_gl_frame_list(it == 1 ? 1 : 2, fa, list, nblocks, c.stream));
      else if (c.x.loop && mode != 0) RFX_HIP(launch_gl_frame_loop(mode, fa, nblocks, c.stream));
      else RFX_HIP(launch_gl_frame(mode, fa, nblocks, c.stream));
      const bool last = it == c.n_iter;
      if (c.x.loop)
        RFX_HIP(launch_gl_loop_fold(fa.frames, plan->d_win, scale, last ? c.out : gen[it % 3][0], B, T, last ? (size_t)L : (size_t)w.Lpad, c.stream));
      else
        RFX_HIP(launch_gl_fold(fa.frames, plan->d_win, scale, last ? c.out : gen[it % 3][0], B, T, L, last ? (size_t)L : (size_t)w.Lpad, c.stream,
                               masked && it > 0 ? cadd : nullptr, (size_t)w.Lpad));
      RFX_HIP(timer.mark(it, c.stream));
    }
    RFX_HIP(timer.finish());
    return RFX_OK;
  }

  GlArgs g;
  set_gl_args(g, c);
  g.out_scale = scale;
  g.tw1 = plan->d_tw1;
  g.tw2 = plan->d_tw2;
  g.win = plan->d_win;
  g.Lpad = w.Lpad;
  g.timing = plan->timing;
  // runs: the batch's B*T frames, counted clip after clip, are cut into one run per resident workgroup slot (gl_partition)
  const GlPartition part = gl_partition(plan, B, T);
  g.run_h = part.h;
  g.run_w1 = part.w1;
  g.run_w2 = part.w2;
  auto set_io = [&](int k_in, int k_prev, int k_out) {
    for (int p = 0; p < 2; ++p) {
      g.audio_in[p] = gen[k_in][p];
      g.audio_prev[p] = gen[k_prev][p];
      g.audio_out[p] = gen[k_out][p];
    }
  };
  RFX_HIP(timer.begin(c.stream));
  // guided: launch 0 is MODE 1 on the guide, staged as the generation it reads (buffer 0 the guide, buffer 1 zeros: the kernel adds
  // the two around its run boundaries); generation 2 is free until launch 2 writes it
  if (c.x.guide)
    if (int rc = gl_stage_guide(c, w.Lpad, false, gen[2][0], gen[1][0], gen[1][1])) return rc;
  for (int it = 0; it <= c.n_iter; ++it) {
    // iteration `it` analyses x_{it-1} - m*x_{it-2} and writes x_it; MODE 0 reads nothing and writes x_0
    if (it == 0) set_io(1, 2, 0);
    else set_io((it - 1) % 3, (it + 1) % 3 /* == (it-2) mod 3 */, it % 3);
#ifdef RFX_WGCLOCK
    g.launch = it;
#endif
    RFX_HIP(launch_gl_iter(it == 0 ? (c.x.guide ? 1 : 0) : it == 1 ? 1 : 2, g, part.runs, c.stream));
    RFX_HIP(timer.mark(it, c.stream));
  }
  const int last = c.n_iter % 3;
  RFX_HIP(launch_gl_combine(gen[last][0], gen[last][1], c.out, g, part.runs, c.stream));
  RFX_HIP(timer.finish());
  return RFX_OK;
}

// every iteration re-analyses the estimate with torch.stft(center=True, reflect): the reference raises there unless the signal is
// longer than the n_fft/2 padding.  A guided call analyses its guide that way even with no iteration.
static int reflect_refusal(const rfx_plan* plan) {
  return fail(RFX_ERR_INVALID,
              plan->generic ? "rfx_griffinlim: Padding size should be less than the corresponding input dimension (reflect padding " +
                                  std::to_string(plan->p.n_fft / 2) + " needs more than that many samples)"
                            : "rfx_griffinlim: Padding size should be less than the corresponding input dimension "
                              "(reflect padding 8820 needs more than 8820 samples, i.e. at least 22 frames)");
}
// what every entry that takes a guide checks before it launches anything
static int guide_refusal(const rfx_plan* plan, const CallOpt& opt, int T, bool has_angles0, const char* who) {
  if (!opt.guide) return RFX_OK;
  if (has_angles0) return fail(RFX_ERR_INVALID, std::string(who) + ": a guide and d_angles0_slots are two starts: give one");
  if (opt.mask && opt.mask_words != rfx_hold_mask_words(plan))
    return fail(RFX_ERR_INVALID, std::string(who) + ": hold_words must be rfx_hold_mask_words(plan) = " + std::to_string(rfx_hold_mask_words(plan)));
  if (!opt.loop && T >= 2 && rfx_griffinlim_output_samples(plan, T) <= plan->p.n_fft / 2) return reflect_refusal(plan);
  return RFX_OK;
}
// ... and every entry that decodes a loop
static int loop_frames_refusal(int hop, int n_fft, int T, const char* who) {
  if (loop_valid(hop, T, n_fft)) return RFX_OK;
  return fail(RFX_ERR_INVALID, std::string(who) + ": a loop call needs hop_length * T >= n_fft (a frame covers the period at most once): at least " +
                                   std::to_string(loop_min_frames(hop, n_fft)) + " frames, got " + std::to_string(T));
}
static int loop_refusal(const rfx_plan* plan, const CallOpt& opt, int T, const char* who) {
  if (!opt.loop) return RFX_OK;
  if (plan->czt)
    return fail(RFX_ERR_UNSUPPORTED, std::string(who) + ": a loop call is not served on the chirp-z engine (its frame kernels have no circular variant)");
  return loop_frames_refusal(plan->p.hop_length, plan->p.n_fft, T, who);
}
int rfx_debug_loop_frames(const rfx_params* params, int T) {
  if (!params || params->hop_length <= 0 || params->n_fft <= 0) return fail(RFX_ERR_INVALID, "rfx_debug_loop_frames: bad argument");
  return loop_frames_refusal(params->hop_length, params->n_fft, T, "rfx_debug_loop_frames");
}

static int griffinlim_impl(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                           int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                           void* stream, float* h_launch_ms, const CallOpt& opt, bool mag_in_fam_slots = false,
                           const float* d_row_scale = nullptr) {
  // (a loop call this plan or this T cannot serve has no workspace to bring: its refusal comes first)
  if (plan)
    if (int rc = loop_refusal(plan, opt, T, "rfx_griffinlim")) return rc;
  if (!plan || !d_mag_slots || !d_wave_out || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_griffinlim: null argument");
  if (B <= 0 || T < 2 || n_iter < 0) return fail(RFX_ERR_INVALID, "rfx_griffinlim: bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, "rfx_griffinlim: more than 2^31 - 1 frames in one call");
  if (!(momentum >= 0.f && momentum < 1.f)) return fail(RFX_ERR_INVALID, "rfx_griffinlim: momentum must be in [0, 1)");
  const int L = gl_out_samples(plan, T, opt.loop);
  if (!opt.loop && n_iter > 0 && L <= plan->p.n_fft / 2) return reflect_refusal(plan);
  if (int rc = guide_refusal(plan, opt, T, d_angles0_slots != nullptr, "rfx_griffinlim")) return rc;
  if (opt.peak)
    if (int rc = peak_refusal(plan, "rfx_griffinlim")) return rc;
  const GlLayout w = griffinlim_layout(plan, B, T, opt.kind(), opt.peak);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_griffinlim: workspace too small");
  RFX_ON_DEVICE(plan->device);
  GlCall c{d_mag_slots, (const cf*)d_angles0_slots, d_row_scale, momentum / (1.f + momentum), seed, B, T, L, n_iter, d_wave_out,
           (char*)d_workspace, (hipStream_t)stream, opt};
  LaunchTimer timer(h_launch_ms, n_iter + 1);
  if (opt.peak) {  // rfx_peak_start into the angles of the call's workspace, then the call with those angles injected
    RFX_HIP(timer.begin(c.stream));
    const int layout = !plan->generic ? kHoldMaskSpec : plan->fam_ok && mag_in_fam_slots ? kHoldMaskTable : kHoldMaskPlain;
    if (int rc = peak_start_run(plan, layout, c.S, B, T, c.ws + w.angles, c.ws + w.peak_scratch, c.stream)) return rc;
    c.angles0 = (const cf*)(c.ws + w.angles);
  }
  return plan->generic ? gen_griffinlim(plan, c, w, mag_in_fam_slots, timer) : spec_griffinlim(plan, c, w, timer);
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
  if (int rc = read_call_options(options, &opt, "rfx_griffinlim_ex", 0, true)) return rc;
  if (opt.peak && d_angles0_slots) return fail(RFX_ERR_INVALID, "rfx_griffinlim_ex: start == 1 and d_angles0_slots are two starts: give one");
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

// a per-mel-band mask to the bin mask of a masked call (rfx_holdmask_core.h), by the bins' band ranges uploaded with the plan
int rfx_hold_bins_from_bands(const rfx_plan* plan, const uint8_t* d_bands, int B, int T, uint32_t* d_hold_bins_out, void* stream) {
  if (!plan || !d_bands || !d_hold_bins_out) return fail(RFX_ERR_INVALID, "rfx_hold_bins_from_bands: null argument");
  if (!plan->d_bin_bands) return fail(RFX_ERR_INVALID, "rfx_hold_bins_from_bands: plan was created without a mel filterbank");
  if (B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_hold_bins_from_bands: bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, "rfx_hold_bins_from_bands: more than 2^31 - 1 frames in one call");
  if ((uintptr_t)d_hold_bins_out & (sizeof(uint32_t) - 1)) return fail(RFX_ERR_INVALID, "rfx_hold_bins_from_bands: d_hold_bins_out must be aligned to 4 bytes");
  RFX_ON_DEVICE(plan->device);
  RFX_HIP(launch_holdmask_bands(d_bands, plan->d_bin_bands, plan->d_bin_bands + plan->n_stft, d_hold_bins_out, B, plan->p.n_mels, T, plan->n_stft,
                                (hipStream_t)stream));
  return RFX_OK;
}

// ---- InverseMelScale ------------------------------------------------------------------------------------------------------------
// the loss history [B*T][max_mel_iters], the clips' stopping steps and the any-early word behind them, the clips' range table
struct ImelLayout {
  size_t hist, it_stop, clip_scale, total;
};
static ImelLayout inverse_mel_layout(const rfx_plan* plan, int B, int T) {
  ImelLayout l{};
  if (B <= 0 || T <= 0) return l;
  Carve c;
  l.hist = c.take((size_t)B * T * plan->p.max_mel_iters * sizeof(float));
  l.it_stop = c.take((size_t)(B + 1) * sizeof(int));
  l.clip_scale = c.take(range_table_bytes(B));
  l.total = c.at;
  return l;
}
size_t rfx_inverse_mel_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? inverse_mel_layout(plan, B, T).total : 0; }

// can InverseMelScale write a row-family plan's frames straight in the family kernels' slot order?  (Every kernel that leaves
// through imel_emit_frame can: the output order is just its pos_bin table.  The general LDS kernel stores bin by bin.)
static bool imel_can_emit_fam_slots(const rfx_plan* plan) {
  return plan->generic && plan->fam_ok && plan->imel_ok && plan->d_fam_binof &&
         rfx::imel_kernel_choice(plan->imel, plan->p.n_mels, plan->p.max_mel_iters, plan->imel_variant) != rfx::kImelKernelGeneral;
}

static int inverse_mel_impl(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                            uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream_, bool fam_slots,
                            const CallOpt& opt, float* d_gl_row_scale = nullptr) {
  if (!plan || !d_mel || !d_mag_slots || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_inverse_mel: null argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, "rfx_inverse_mel: plan was created without a mel filterbank");
  if (!plan->imel_ok) return fail(RFX_ERR_UNSUPPORTED, "rfx_inverse_mel: filterbank is not banded: " + plan->imel_why);
  if (B <= 0 || T <= 0 || channels_per_clip <= 0 || B % channels_per_clip)
    return fail(RFX_ERR_INVALID, "rfx_inverse_mel: batch must be a multiple of channels_per_clip");
  if (opt.row_base % (uint64_t)channels_per_clip)
    return fail(RFX_ERR_INVALID, "rfx_inverse_mel: rfx_call_options.row_base must be a multiple of channels_per_clip (clips are not split)");
  const ImelLayout w = inverse_mel_layout(plan, B, T);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_inverse_mel: workspace too small");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int nclips = B / channels_per_clip;
  char* ws = (char*)d_workspace;
  float* hist = (float*)(ws + w.hist);
  int* it_stop = (int*)(ws + w.it_stop);
  int* any_early = it_stop + nclips;
  RFX_HIP(hipMemsetAsync(any_early, 0, sizeof(int), stream));
  // numeric range: the power of two each clip's SGD state is held in (and, for the fused call, the Griffin-Lim rows' factors),
  // from the caller's hint or the clip's largest mel amplitude
  float* clip_scale = (float*)(ws + w.clip_scale);
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

// ---- InverseMelScale, closed form (rfx_imel_lstsq.hip): the tridiagonal solve into the workspace, then the expansion -----------------
struct LstsqLayout {
  size_t zy, total;  // (B, n_mels, T) floats: the forward sweep's z, then y in place
};
static LstsqLayout inverse_mel_lstsq_layout(const rfx_plan* plan, int B, int T) {
  LstsqLayout l{};
  if (!plan->lstsq_ok || B <= 0 || T <= 0) return l;
  Carve c;
  l.zy = c.take((size_t)B * plan->p.n_mels * T * sizeof(float));
  l.total = c.at;
  return l;
}
size_t rfx_inverse_mel_lstsq_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? inverse_mel_lstsq_layout(plan, B, T).total : 0; }

// what every entry that takes the closed form checks before it launches anything
static int lstsq_refusal(const rfx_plan* plan, const char* who) {
  if (plan->lstsq_ok) return RFX_OK;
  return fail(RFX_ERR_INVALID, std::string(who) + ": the closed-form InverseMelScale does not serve this plan: " + plan->lstsq_why);
}

int rfx_inverse_mel_lstsq(const rfx_plan* plan, const float* d_mel, int B, int T, float* d_mag_slots, void* d_workspace,
                          size_t workspace_bytes, void* stream_) {
  if (!plan || !d_mel || !d_mag_slots || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_inverse_mel_lstsq: null argument");
  if (int rc = lstsq_refusal(plan, "rfx_inverse_mel_lstsq")) return rc;
  if (B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_inverse_mel_lstsq: bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, "rfx_inverse_mel_lstsq: more than 2^31 - 1 frames in one call");
  if (((uintptr_t)d_mag_slots & 15) || (plan->frame_stride & 3))
    return fail(RFX_ERR_INVALID, "rfx_inverse_mel_lstsq: d_mag_slots must be 16-byte aligned");
  const LstsqLayout w = inverse_mel_lstsq_layout(plan, B, T);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_inverse_mel_lstsq: workspace too small");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  float* zy = (float*)((char*)d_workspace + w.zy);
  RFX_HIP(launch_lsq_solve(plan->lstsq, d_mel, zy, B, plan->p.n_mels, T, stream));
  RFX_HIP(launch_lsq_expand(plan->lstsq, zy, d_mag_slots, B, plan->p.n_mels, T, plan->frame_stride, stream));
  return RFX_OK;
}

// ---- its backward: the forward's solve again (the mask is recomputed, not saved), the collect, and the same solve on c ---------------
struct LstsqBackwardLayout {
  size_t y, c, total;  // (B, n_mels, T) floats each: y = G^-1 mel, and c = fb^T (gx where the relu is open)
};
static LstsqBackwardLayout inverse_mel_lstsq_backward_layout(const rfx_plan* plan, int B, int T) {
  LstsqBackwardLayout l{};
  if (!plan->lstsq_ok || B <= 0 || T <= 0) return l;
  Carve c;
  l.y = c.take((size_t)B * plan->p.n_mels * T * sizeof(float));
  l.c = c.take((size_t)B * plan->p.n_mels * T * sizeof(float));
  l.total = c.at;
  return l;
}
size_t rfx_inverse_mel_lstsq_backward_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? inverse_mel_lstsq_backward_layout(plan, B, T).total : 0;
}

int rfx_inverse_mel_lstsq_backward(const rfx_plan* plan, const float* d_mel, const float* d_grad_slots, int B, int T, float* d_grad_mel,
                                   void* d_workspace, size_t workspace_bytes, void* stream_) {
  const char* who = "rfx_inverse_mel_lstsq_backward";
  if (!plan || !d_mel || !d_grad_slots || !d_grad_mel || !d_workspace) return fail(RFX_ERR_INVALID, std::string(who) + ": null argument");
  if (int rc = lstsq_refusal(plan, who)) return rc;
  if (B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, std::string(who) + ": bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, std::string(who) + ": more than 2^31 - 1 frames in one call");
  if (((uintptr_t)d_grad_slots & 15) || (plan->frame_stride & 3)) return fail(RFX_ERR_INVALID, std::string(who) + ": d_grad_slots must be 16-byte aligned");
  if (plan->lstsq_collect.n_vecs > kLsqCollectVecs * kLsqCollectThreads)
    return fail(RFX_ERR_INVALID, std::string(who) + ": more 16-byte vectors with a counted bin in a frame than the collect kernel holds");
  const LstsqBackwardLayout w = inverse_mel_lstsq_backward_layout(plan, B, T);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, std::string(who) + ": workspace too small");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  float *y = (float*)((char*)d_workspace + w.y), *c = (float*)((char*)d_workspace + w.c);
  const int M = plan->p.n_mels;
  RFX_HIP(launch_lsq_solve(plan->lstsq, d_mel, y, B, M, T, stream));
  RFX_HIP(launch_lsq_collect(plan->lstsq_collect, y, d_grad_slots, c, B, M, T, plan->frame_stride, stream));
  RFX_HIP(launch_lsq_solve(plan->lstsq, c, d_grad_mel, B, M, T, stream));
  return RFX_OK;
}

// ---- SpectrogramConverter.waveform_from_mel_amplitudes in one call (spectrogram_converter.py:187-204: inverse_mel_scaler, then
// inverse_spectrogram_func).  rfx_inverse_mel into the head of the workspace, rfx_griffinlim from there: the same two launches
// sequences, the same seeds (seed for the SGD start, seed + 1 for the phases, as the Python layer always called them), the linear
// magnitudes never leave the library.
// The linear magnitudes, the Griffin-Lim rows' range table (written by the SGD stage's range pass), then the two stages' own
// workspaces on top of each other.  A row-family plan's magnitudes go from the SGD kernel to the Griffin-Lim kernels in THEIR slot
// order (fam_slots): the once-per-call re-ordering of plain frames (0.75 ms and 2.5 GB of traffic per 64 tiles at 48 kHz) exists
// only for callers of the two entry points.
struct WaveFromMelLayout {
  size_t lin, row_scale, rest, total;
  bool fam_slots;
};
static WaveFromMelLayout waveform_from_mel_layout(const rfx_plan* plan, int B, int T, GlKind kind, bool peak) {
  WaveFromMelLayout l{};
  const size_t imel = rfx_inverse_mel_workspace_bytes(plan, B, T), gl = griffinlim_layout(plan, B, T, kind, false).total;
  if (!imel || !gl) return l;
  const size_t lstsq = inverse_mel_lstsq_layout(plan, B, T).total;
  l.fam_slots = imel_can_emit_fam_slots(plan);
  // one layout for both forms of InverseMelScale: the closed form writes plain frames also on a row-family plan
  const size_t per_frame = l.fam_slots && plan->fam.fsf > plan->frame_stride ? (size_t)plan->fam.fsf : (size_t)plan->frame_stride;
  Carve c;
  l.lin = c.take((size_t)B * T * per_frame * sizeof(float));
  l.row_scale = c.take(range_table_bytes(B));
  l.rest = c.at;
  // (the peak start's angles and scratch lie behind the Griffin-Lim stage's own bytes; the call brings them on top of the largest stage)
  l.total = l.rest + std::max(std::max(imel, gl), lstsq) + (peak ? peak_extra_bytes(plan, B, T) : 0);
  return l;
}
static int waveform_from_mel_impl(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                                 float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream, const CallOpt& opt) {
  if (plan)
    if (int rc = loop_refusal(plan, opt, T, "rfx_waveform_from_mel")) return rc;
  if (!plan || !d_mel || !d_wave_out || !d_workspace || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_waveform_from_mel: bad argument");
  if (opt.lstsq)
    if (int rc = lstsq_refusal(plan, "rfx_waveform_from_mel")) return rc;
  if (int rc = guide_refusal(plan, opt, T, false, "rfx_waveform_from_mel")) return rc;
  const WaveFromMelLayout w = waveform_from_mel_layout(plan, B, T, opt.kind(), opt.peak);
  if (!w.total) return fail(RFX_ERR_UNSUPPORTED, "rfx_waveform_from_mel: this plan cannot invert (see rfx_inverse_mel / rfx_griffinlim)");
  if (opt.peak)
    if (int rc = peak_refusal(plan, "rfx_waveform_from_mel")) return rc;
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_waveform_from_mel: workspace too small");
  char* ws = (char*)d_workspace;
  float* lin = reinterpret_cast<float*>(ws + w.lin);
  float* row_scale = reinterpret_cast<float*>(ws + w.row_scale);
  if (opt.lstsq) {  // rfx_inverse_mel_lstsq, then rfx_griffinlim_ex: plain frames, the rows' range from the hint or the magnitudes
    if (int rc = rfx_inverse_mel_lstsq(plan, d_mel, B, T, lin, ws + w.rest, workspace_bytes - w.rest, stream)) return rc;
    return griffinlim_impl(plan, lin, nullptr, seed + 1, B, T, n_iter, momentum, d_wave_out, ws + w.rest, workspace_bytes - w.rest, stream, nullptr, opt);
  }
  if (int rc = inverse_mel_impl(plan, d_mel, B, T, channels_per_clip, nullptr, seed, lin, ws + w.rest, workspace_bytes - w.rest, stream, w.fam_slots, opt, row_scale)) return rc;
  return griffinlim_impl(plan, lin, nullptr, seed + 1, B, T, n_iter, momentum, d_wave_out, ws + w.rest, workspace_bytes - w.rest, stream, nullptr, opt, w.fam_slots, row_scale);
}

int rfx_waveform_from_mel(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                          float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  return waveform_from_mel_impl(plan, d_mel, B, T, channels_per_clip, seed, n_iter, momentum, d_wave_out, d_workspace, workspace_bytes, stream, CallOpt{});
}

int rfx_waveform_from_mel_ex(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                             float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream,
                             const rfx_call_options* options) {
  CallOpt opt;
  if (int rc = read_call_options(options, &opt, "rfx_waveform_from_mel_ex", RFX_CALL_INVERSE_MEL_LSTSQ, true)) return rc;
  return waveform_from_mel_impl(plan, d_mel, B, T, channels_per_clip, seed, n_iter, momentum, d_wave_out, d_workspace, workspace_bytes, stream, opt);
}

// ---- SpectrogramImageConverter.audio_from_spectrogram_image's device half in one call (spectrogram_image_converter.py:54-91:
// image_util.spectrogram_from_image, SpectrogramConverter.audio_from_spectrogram -> waveform_from_mel_amplitudes on the image's
// (C, n_mels, T) tensor, audio_util.audio_from_waveform): uint8 tiles in, int16 PCM out.  The three entry points it is made of,
// in their order, with the same seeds: same bytes.
// The decoded mel amplitudes, the waveform, then rfx_waveform_from_mel's workspace.
struct AudioFromImageLayout {
  size_t mel, wave, rest, total;
};
static AudioFromImageLayout audio_from_image_layout(const rfx_plan* plan, int N, int stereo, int T, GlKind kind, bool peak) {
  AudioFromImageLayout l{};
  if (N <= 0 || T <= 0) return l;
  const int B = N * (stereo ? 2 : 1);
  const size_t inner = waveform_from_mel_layout(plan, B, T, kind, peak).total;
  if (!inner) return l;
  Carve c;
  l.mel = c.take((size_t)B * plan->p.n_mels * T * sizeof(float));
  l.wave = c.take((size_t)B * gl_out_samples(plan, T, kind == kGlLoop) * sizeof(float));
  l.rest = c.at;
  l.total = l.rest + inner;
  return l;
}
// The workspace queries of the three entries: one sizing function, asked by the plain names for a call without options and by the
// _ex names with the call's own options, read as the entry of the same name reads them (refused options: 0, and the refusal in
// rfx_last_error).  rows: B, or N images of 1 + stereo rows
enum Entry { kEntryGriffinLim, kEntryWaveformFromMel, kEntryAudioFromImage };
static size_t inverse_workspace(const rfx_plan* plan, Entry entry, int rows, int stereo, int T, GlKind kind, bool peak) {
  if (!plan) return 0;
  return entry == kEntryGriffinLim        ? griffinlim_layout(plan, rows, T, kind, peak).total
         : entry == kEntryWaveformFromMel ? waveform_from_mel_layout(plan, rows, T, kind, peak).total
                                          : audio_from_image_layout(plan, rows, stereo, T, kind, peak).total;
}
static size_t inverse_workspace_ex(const rfx_plan* plan, Entry entry, int rows, int stereo, int T, const rfx_call_options* options, const char* who) {
  CallOpt opt;
  if (read_call_options(options, &opt, who, entry == kEntryGriffinLim ? 0 : RFX_CALL_INVERSE_MEL_LSTSQ, true)) return 0;
  return inverse_workspace(plan, entry, rows, stereo, T, opt.kind(), opt.peak);
}
size_t rfx_griffinlim_workspace_bytes_ex(const rfx_plan* plan, int B, int T, const rfx_call_options* options) {
  return inverse_workspace_ex(plan, kEntryGriffinLim, B, 0, T, options, __func__);
}
size_t rfx_waveform_from_mel_workspace_bytes_ex(const rfx_plan* plan, int B, int T, const rfx_call_options* options) {
  return inverse_workspace_ex(plan, kEntryWaveformFromMel, B, 0, T, options, __func__);
}
size_t rfx_audio_from_image_workspace_bytes_ex(const rfx_plan* plan, int N, int stereo, int T, const rfx_call_options* options) {
  return inverse_workspace_ex(plan, kEntryAudioFromImage, N, stereo, T, options, __func__);
}
size_t rfx_griffinlim_workspace_bytes(const rfx_plan* plan, int B, int T) { return rfx_griffinlim_workspace_bytes_ex(plan, B, T, nullptr); }
size_t rfx_waveform_from_mel_workspace_bytes(const rfx_plan* plan, int B, int T) { return rfx_waveform_from_mel_workspace_bytes_ex(plan, B, T, nullptr); }
size_t rfx_audio_from_image_workspace_bytes(const rfx_plan* plan, int N, int stereo, int T) {
  return rfx_audio_from_image_workspace_bytes_ex(plan, N, stereo, T, nullptr);
}

static int audio_from_image_impl(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                                int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                                size_t workspace_bytes, void* stream, const CallOpt& opt) {
  if (plan)
    if (int rc = loop_refusal(plan, opt, T, "rfx_audio_from_image_u8")) return rc;
  if (!plan || !d_img || !d_lut256 || !d_clip_peak || !d_pcm_out || !d_workspace || N <= 0 || T <= 0)
    return fail(RFX_ERR_INVALID, "rfx_audio_from_image_u8: bad argument");
  if (opt.lstsq)
    if (int rc = lstsq_refusal(plan, "rfx_audio_from_image_u8")) return rc;
  if (int rc = guide_refusal(plan, opt, T, false, "rfx_audio_from_image_u8")) return rc;
  const AudioFromImageLayout w = audio_from_image_layout(plan, N, stereo, T, opt.kind(), opt.peak);
  if (!w.total) return fail(RFX_ERR_UNSUPPORTED, "rfx_audio_from_image_u8: this plan cannot invert (see rfx_inverse_mel / rfx_griffinlim)");
  const int C = stereo ? 2 : 1, B = N * C;
  if (opt.peak)
    if (int rc = peak_refusal(plan, "rfx_audio_from_image_u8")) return rc;
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_audio_from_image_u8: workspace too small");
  const int M = plan->p.n_mels, L = gl_out_samples(plan, T, opt.loop);
  char* ws = (char*)d_workspace;
  float* mel = reinterpret_cast<float*>(ws + w.mel);
  float* wave = reinterpret_cast<float*>(ws + w.wave);
  if (int rc = rfx_image_decode_u8(d_img, N, M, T, stereo, d_lut256, mel, stream)) return rc;
  // (a clip is one image: its channels share the SGD loss mean and the peak normalisation)
  if (int rc = waveform_from_mel_impl(plan, mel, B, T, C, seed, n_iter, momentum, wave, ws + w.rest, workspace_bytes - w.rest, stream, opt)) return rc;
  return rfx_pcm16(wave, N, C, L, normalize, d_clip_peak, d_pcm_out, stream);
}

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
  if (int rc = read_call_options(options, &opt, "rfx_audio_from_image_u8_ex", RFX_CALL_INVERSE_MEL_LSTSQ, true)) return rc;
  return audio_from_image_impl(plan, d_img, N, T, stereo, d_lut256, seed, n_iter, momentum, normalize, d_clip_peak, d_pcm_out, d_workspace,
                               workspace_bytes, stream, opt);
}
