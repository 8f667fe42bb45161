// rfx_api_guided.hip - the C ABI of librfx.so (include/rfx.h), "GUIDED DECODE, BACKWARD": rfx_griffinlim_guided_backward,
// rfx_waveform_from_mel_guided_backward and their loop forms.  Host code only: one layout and one driver per entry, the form (plain /
// loop) an argument.  The stage entry, per group of rows:
//     rfx_istft_backward / rfx_istft_backward_loop   G: the synthesis adjoint of the rows' g_w, gradient slots
//     guide_peak_kernel, guide_stage_rows_kernel     the guide fitted to L samples and ranged, rows of L floats (rfx_guide.hip)
//     rfx_stft / rfx_stft_loop                       a: the plan's forward frame transform of the staged guide, spectrum slots
//     guide_project_kernel                           g_S = Re(conj(u) G), u = a / (|a| + 1e-16), magnitude slots (rfx_guide_bwd.hip)
// The fused entry is the stage entry into the head of its workspace, then rfx_inverse_mel_lstsq_backward from there: the per-module
// calls themselves, hence their bytes.  Rows are walked in groups of whole rows: the stage's workspace is bounded whatever B is, and
// every kernel works frame by frame or sample by sample - a row's bytes depend on that row alone.
#include <algorithm>

#include "rfx_api.h"
#include "rfx_guide_core.h"

using namespace rfx;

constexpr size_t kGuidedBwdGroupBytes = (size_t)256 << 20;
constexpr size_t kGuidedBwdGroupRows = 65535;  // the staging carries the row in blockIdx.y
constexpr size_t kGuidedBwdMaxLds = (size_t)160 << 10;

// samples per row of T frames as the guided call of the form stages its guide; 0: the form does not serve T
static int guided_samples(const rfx_plan* plan, int T, bool loop) {
  if (T < 2) return 0;
  const int L = loop ? (plan->czt ? 0 : rfx_griffinlim_loop_output_samples(plan, T)) : rfx_griffinlim_output_samples(plan, T);
  return L > 0 && fwd_length_ok(plan, L, loop) && fwd_frames(plan, L, loop) == T ? L : 0;
}
static size_t istft_backward_bytes(const rfx_plan* plan, int rows, int T, bool loop) {
  return loop ? rfx_istft_backward_loop_workspace_bytes(plan, rows, T) : rfx_istft_backward_workspace_bytes(plan, rows, T);
}

// The group's gradient slots G, the staged guide rows, their chunk peaks, the guide's spectrum slots a, rfx_istft_backward's own bytes
struct GuidedBwdLayout {
  size_t grad, staged, peaks, spec, inner, inner_bytes, total;
  int group_rows, L;
};
static GuidedBwdLayout guided_backward_layout(const rfx_plan* plan, int B, int T, bool loop) {
  GuidedBwdLayout l{};
  if (B <= 0 || (long long)B * T > 0x7fffffffLL) return l;
  l.L = guided_samples(plan, T, loop);
  if (l.L <= 0) return GuidedBwdLayout{};
  const size_t spec_row = (size_t)T * plan->frame_stride * sizeof(cf), staged_row = (size_t)l.L * sizeof(float);
  l.group_rows = group_rows(kGuidedBwdGroupBytes, 2 * spec_row + staged_row, B, kGuidedBwdGroupRows);
  l.inner_bytes = istft_backward_bytes(plan, l.group_rows, T, loop);
  if (!l.inner_bytes) return GuidedBwdLayout{};
  Carve c;
  l.grad = c.take((size_t)l.group_rows * spec_row);
  l.staged = c.take((size_t)l.group_rows * staged_row);
  l.peaks = c.take((size_t)l.group_rows * guide_chunks(l.L) * sizeof(float));
  l.spec = c.take((size_t)l.group_rows * spec_row);
  l.inner = c.take(l.inner_bytes);
  l.total = c.at;
  return l;
}
size_t rfx_griffinlim_guided_backward_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? guided_backward_layout(plan, B, T, false).total : 0;
}
size_t rfx_griffinlim_guided_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? guided_backward_layout(plan, B, T, true).total : 0;
}

static std::string guided_name(const char* stem, bool loop) { return std::string(stem) + (loop ? "_loop" : ""); }

// what both entries check after their null checks and before anything is launched
static int guided_backward_refusal(const rfx_plan* plan, int guide_samples, int B, int T, bool loop, const std::string& w) {
  if (B <= 0 || T < 2) return fail(RFX_ERR_INVALID, w + ": bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, w + ": more than 2^31 - 1 frames in one call");
  if (guide_samples <= 0) return fail(RFX_ERR_INVALID, w + ": guide_samples must be positive");
  if (loop && plan->czt)
    return fail(RFX_ERR_UNSUPPORTED, w + ": a loop call is not served on the chirp-z engine (its frame kernels have no circular variant)");
  if (loop && !loop_valid(plan->p.hop_length, T, plan->p.n_fft))
    return fail(RFX_ERR_INVALID, w + ": a loop call needs hop_length * T >= n_fft (a frame covers the period at most once): at least " +
                                     std::to_string(loop_min_frames(plan->p.hop_length, plan->p.n_fft)) + " frames, got " + std::to_string(T));
  if (guided_samples(plan, T, loop) <= 0)
    return fail(RFX_ERR_INVALID, w + ": Padding size should be less than the corresponding input dimension (the guide of " + std::to_string(T) +
                                     " frames is analysed with reflect padding " + std::to_string(plan->p.n_fft / 2) + " and needs more than that many samples)");
  if ((plan->frame_stride & 3) || (plan->mb_sstride & 3)) return fail(RFX_ERR_UNSUPPORTED, w + ": the plan's frame strides are not multiples of four");
  if ((size_t)plan->frame_stride * sizeof(float) > kGuidedBwdMaxLds)
    return fail(RFX_ERR_UNSUPPORTED, w + ": a frame of " + std::to_string(plan->frame_stride) + " slots does not fit the projection kernel's LDS");
  return RFX_OK;
}

static int guided_backward_run(const rfx_plan* plan, const float* d_guide, int guide_samples, const float* d_grad_wave, int B, int T,
                               float* d_grad_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream_, bool loop) {
  const std::string w = guided_name("rfx_griffinlim_guided_backward", loop);
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_guide || !d_grad_wave || !d_grad_mag_slots || !d_workspace) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (int rc = guided_backward_refusal(plan, guide_samples, B, T, loop, w)) return rc;
  if (((uintptr_t)d_workspace | (uintptr_t)d_grad_mag_slots) & 15 || ((uintptr_t)d_guide | (uintptr_t)d_grad_wave) & 3)
    return fail(RFX_ERR_INVALID, w + ": d_workspace and d_grad_mag_slots must be 16-byte aligned, d_guide and d_grad_wave 4-byte aligned");
  const GuidedBwdLayout l = guided_backward_layout(plan, B, T, loop);
  if (!l.total) return fail(RFX_ERR_UNSUPPORTED, w + ": this plan's inverse spectrogram does not serve " + std::to_string(T) + " frames");
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)d_workspace;
  cf* G = reinterpret_cast<cf*>(ws + l.grad);
  cf* A = reinterpret_cast<cf*>(ws + l.spec);
  float* staged = reinterpret_cast<float*>(ws + l.staged);
  float* peaks = reinterpret_cast<float*>(ws + l.peaks);
  const int L = l.L;
  // the magnitude slots are rfx_pack_magnitudes': the specialised engine's slot order, a generic plan's plain frames (position = bin,
  // on a row family too: rfx_griffinlim re-orders them itself)
  const int sstride = plan->frame_stride;
  for (int r0 = 0; r0 < B; r0 += l.group_rows) {
    const int rows = B - r0 < l.group_rows ? B - r0 : l.group_rows;
    if (int rc = (loop ? rfx_istft_backward_loop : rfx_istft_backward)(plan, d_grad_wave + (size_t)r0 * L, rows, T, G, ws + l.inner, l.inner_bytes, stream_))
      return rc;
    RFX_HIP(launch_guide_stage_rows(d_guide + (size_t)r0 * guide_samples, guide_samples, guide_samples, rows, L, peaks, staged, stream));
    if (int rc = (loop ? rfx_stft_loop : rfx_stft)(plan, staged, rows, L, nullptr, A, stream_)) return rc;
    GuideProjectArgs a{};
    a.G = G;
    a.A = A;
    a.out = d_grad_mag_slots + (size_t)r0 * T * sstride;
    a.xpos_bin = plan->d_mb_xpos_bin;
    a.s2x = plan->generic ? plan->d_mb_xpos_bin : plan->d_mb_s2x;
    a.B = rows;
    a.T = T;
    a.xstride = plan->frame_stride;
    a.sstride = sstride;
    RFX_HIP(launch_guide_project(a, stream));
  }
  return RFX_OK;
}
int rfx_griffinlim_guided_backward(const rfx_plan* plan, const float* d_guide, int guide_samples, const float* d_grad_wave, int B, int T,
                                   float* d_grad_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream) {
  return guided_backward_run(plan, d_guide, guide_samples, d_grad_wave, B, T, d_grad_mag_slots, d_workspace, workspace_bytes, stream, false);
}
int rfx_griffinlim_guided_backward_loop(const rfx_plan* plan, const float* d_guide, int guide_samples, const float* d_grad_wave, int B, int T,
                                        float* d_grad_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream) {
  return guided_backward_run(plan, d_guide, guide_samples, d_grad_wave, B, T, d_grad_mag_slots, d_workspace, workspace_bytes, stream, true);
}

// ---- fused: the magnitude gradient of all B rows, then the two stages' own workspaces on top of each other ---------------------------
struct GuidedMelBwdLayout {
  size_t slots, rest, stage_bytes, lstsq_bytes, total;
};
static GuidedMelBwdLayout guided_mel_backward_layout(const rfx_plan* plan, int B, int T, bool loop) {
  GuidedMelBwdLayout l{};
  if (!plan->lstsq_ok) return l;
  l.stage_bytes = guided_backward_layout(plan, B, T, loop).total;
  l.lstsq_bytes = rfx_inverse_mel_lstsq_backward_workspace_bytes(plan, B, T);
  if (!l.stage_bytes || !l.lstsq_bytes) return GuidedMelBwdLayout{};
  Carve c;
  l.slots = c.take((size_t)B * T * plan->frame_stride * sizeof(float));
  l.rest = c.at;
  l.total = l.rest + std::max(l.stage_bytes, l.lstsq_bytes);
  return l;
}
size_t rfx_waveform_from_mel_guided_backward_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? guided_mel_backward_layout(plan, B, T, false).total : 0;
}
size_t rfx_waveform_from_mel_guided_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? guided_mel_backward_layout(plan, B, T, true).total : 0;
}

static int guided_mel_backward_run(const rfx_plan* plan, const float* d_mel, const float* d_guide, int guide_samples, const float* d_grad_wave, int B,
                                   int T, float* d_grad_mel, void* d_workspace, size_t workspace_bytes, void* stream, bool loop) {
  const std::string w = guided_name("rfx_waveform_from_mel_guided_backward", loop);
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_mel || !d_guide || !d_grad_wave || !d_grad_mel || !d_workspace) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (!plan->lstsq_ok) return fail(RFX_ERR_INVALID, w + ": the closed-form InverseMelScale does not serve this plan: " + plan->lstsq_why);
  if (int rc = guided_backward_refusal(plan, guide_samples, B, T, loop, w)) return rc;
  if (((uintptr_t)d_workspace & 15) || ((uintptr_t)d_mel | (uintptr_t)d_guide | (uintptr_t)d_grad_wave | (uintptr_t)d_grad_mel) & 3)
    return fail(RFX_ERR_INVALID, w + ": d_workspace must be 16-byte aligned, the float tensors 4-byte aligned");
  const GuidedMelBwdLayout l = guided_mel_backward_layout(plan, B, T, loop);
  if (!l.total) return fail(RFX_ERR_UNSUPPORTED, w + ": this plan's inverse spectrogram does not serve " + std::to_string(T) + " frames");
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  char* ws = (char*)d_workspace;
  float* slots = reinterpret_cast<float*>(ws + l.slots);
  if (int rc = guided_backward_run(plan, d_guide, guide_samples, d_grad_wave, B, T, slots, ws + l.rest, l.stage_bytes, stream, loop)) return rc;
  return rfx_inverse_mel_lstsq_backward(plan, d_mel, slots, B, T, d_grad_mel, ws + l.rest, l.lstsq_bytes, stream);
}
int rfx_waveform_from_mel_guided_backward(const rfx_plan* plan, const float* d_mel, const float* d_guide, int guide_samples, const float* d_grad_wave,
                                          int B, int T, float* d_grad_mel, void* d_workspace, size_t workspace_bytes, void* stream) {
  return guided_mel_backward_run(plan, d_mel, d_guide, guide_samples, d_grad_wave, B, T, d_grad_mel, d_workspace, workspace_bytes, stream, false);
}
int rfx_waveform_from_mel_guided_backward_loop(const rfx_plan* plan, const float* d_mel, const float* d_guide, int guide_samples,
                                               const float* d_grad_wave, int B, int T, float* d_grad_mel, void* d_workspace, size_t workspace_bytes,
                                               void* stream) {
  return guided_mel_backward_run(plan, d_mel, d_guide, guide_samples, d_grad_wave, B, T, d_grad_mel, d_workspace, workspace_bytes, stream, true);
}
