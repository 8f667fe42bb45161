// rfx_api_backward.hip - the C ABI of librfx.so (include/rfx.h), backward of the forward path: rfx_stft_backward,
// rfx_mel_scale_backward and rfx_mel_from_waveform_backward, and of the fused spectral losses: rfx_spectral_loss_backward and its loop
// form.  Host code only: one layout, one driver (mel_bwd_run).  Per group of rows the driver queues
//     [the forward transform of the rows, spectrum into the workspace]   rfx_stft / rfx_stft_loop; not for rfx_stft_backward
//     the entry's slot kernel: the magnitude slots S'                    mel_bwd_spec_kernel / spec_loss_slots_kernel (rfx_mel_bwd.hip)
//     the engine's MODE 0 per-frame launch on (S', angles)               launch_gl_frame / launch_fam_gl / launch_gen_gl / launch_czt_gl
//     the adjoint fold into the caller's rows                            mel_bwd_fold_kernel, loop: spec_loss_loop_fold_kernel
// An entry brings its own argument checks and the one step that differs, queueing its slot kernel for a group.  The rows are walked in
// groups of whole rows (as the spectral sums walk them), so the workspace is bounded whatever B is, and every kernel of the sequence
// works frame by frame or sample by sample: a row's bytes depend on that row alone.
#include "rfx_api.h"
#include "rfx_mel_bwd_core.h"
#include "rfx_spec_loss_core.h"

using namespace rfx;

constexpr size_t kMelBwdGroupBytes = (size_t)256 << 20;

// The spectrum of the group's rows (with_spec: the entries that transform d_wave), their magnitude slots, their synthesis frames
struct MelBwdLayout {
  size_t spec, smag, frames, total;
  int group_rows, T;
};
size_t mel_bwd_frame_pitch(const rfx_plan* plan) { return plan->generic ? (size_t)plan->gg.fpitch : gl_frame_buffer_bytes(1, 1) / sizeof(float); }
static MelBwdLayout mel_bwd_layout(const rfx_plan* plan, int B, int Lw, bool with_spec, bool loop) {
  MelBwdLayout l{};
  if (B <= 0 || !fwd_length_ok(plan, Lw, loop)) return l;
  l.T = fwd_frames(plan, Lw, loop);
  const size_t T = (size_t)l.T;
  const size_t spec_row = with_spec ? T * plan->frame_stride * sizeof(cf) : 0, smag_row = T * plan->mb_sstride * sizeof(float),
               frames_row = T * mel_bwd_frame_pitch(plan) * sizeof(float);
  l.group_rows = group_rows(kMelBwdGroupBytes, spec_row + smag_row + frames_row, B);
  Carve c;
  l.spec = c.take(l.group_rows * spec_row);
  l.smag = c.take(l.group_rows * smag_row);
  l.frames = c.take(l.group_rows * frames_row);
  l.total = c.at;
  return l;
}
size_t rfx_stft_backward_workspace_bytes(const rfx_plan* plan, int B, int Lw) { return plan ? mel_bwd_layout(plan, B, Lw, false, false).total : 0; }
size_t rfx_mel_from_waveform_backward_workspace_bytes(const rfx_plan* plan, int B, int Lw) {
  return plan && plan->d_mb_wt ? mel_bwd_layout(plan, B, Lw, true, false).total : 0;
}
size_t rfx_spectral_loss_backward_workspace_bytes(const rfx_plan* plan, int B, int Lw) {
  return plan ? mel_bwd_layout(plan, B, Lw, true, false).total : 0;
}
size_t rfx_spectral_loss_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int Lw) {
  return plan ? mel_bwd_layout(plan, B, Lw, true, true).total : 0;
}
size_t rfx_mel_scale_backward_workspace_bytes(const rfx_plan* plan, int B, int T) {
  (void)plan, (void)B, (void)T;
  return 0;  // step 1 alone needs no scratch
}

// the engine's MODE 0 per-frame launch: frames = synthesis of S * angles0, `rows` rows of T frames (rfx_api_istft.hip runs it too)
int mel_bwd_frames(const rfx_plan* plan, const float* S, const cf* angles0, float* frames, int rows, int T, hipStream_t stream) {
  if (!plan->generic) {
    GlFrameArgs fa{};
    fa.S = S;
    fa.angles0 = angles0;
    fa.frames = frames;
    fa.tw1 = plan->d_tw1;
    fa.tw2 = plan->d_tw2;
    fa.win = plan->d_win;
    fa.B = rows;
    fa.T = T;
    RFX_HIP(launch_gl_frame(0, fa, frame_blocks((long long)plan->num_cus * plan->gl_wgs_per_cu, rows, T), stream));
    return RFX_OK;
  }
  const GenGeom& g = plan->gg;
  // padded frame rows (gen_frame_layout): the kernels write the window samples only, the fold reads the padding as zeros
  if (g.fshift > 0) RFX_HIP(hipMemsetAsync(frames, 0, (size_t)rows * T * g.fpitch * sizeof(float), stream));
  if (plan->fam_ok) {
    const FamGeom& f = plan->fam;
    FamGlArgs fa{};
    fa.g = f;
    fa.S = S;
    fa.angles0 = angles0;
    fa.fs_plain = g.fs;
    fa.frames = frames;
    fa.fpitch = g.fpitch;
    fa.fshift = g.fshift;
    fa.tw1 = plan->d_fam_tw;
    fa.twa = plan->d_fam_tw + (size_t)f.rows * f.h;
    fa.win = plan->d_win;
    fa.B = rows;
    fa.T = T;
    RFX_HIP(launch_fam_gl(0, fa, frame_blocks(fam_slot_count(plan), rows, T), stream));
    return RFX_OK;
  }
  GenGlArgs ga{};
  ga.g = g;
  ga.tb = plan->gt;
  ga.S = S;
  ga.angles0 = angles0;
  ga.frames = frames;
  ga.B = rows;
  ga.T = T;
  RFX_HIP(plan->czt ? launch_czt_gl(0, ga, plan->d_czt_c, plan->d_czt_h, plan->num_cus, stream) : launch_gen_gl(0, ga, plan->num_cus, stream));
  return RFX_OK;
}

// the fold of a group: frames of `rows` rows of T frames -> out (rows, Lw)
static MelBwdFoldArgs mel_bwd_fold_args(const rfx_plan* plan, const float* frames, float* out, int rows, int T, int Lw) {
  MelBwdFoldArgs f{};
  f.frames = frames;
  f.win = plan->generic ? nullptr : plan->d_win;
  f.out = out;
  f.fpitch = (int)mel_bwd_frame_pitch(plan);
  f.fshift = plan->generic ? plan->gg.fshift : 0;
  f.left = (plan->p.n_fft - plan->p.win_length) / 2;
  f.win_len = plan->p.win_length;
  f.hop = plan->p.hop_length;
  f.h = plan->p.n_fft / 2;
  f.B = rows;
  f.T = T;
  f.Lw = Lw;
  return f;
}

// The grouped driver.  d_wave: the rows the forward transform (loop: the circular one) writes the group's spectrum from, which is then
// the frame launch's angles; null: no transform, the angles are the caller's d_angles.  ptrs_ok: the entry's own pointers are there.
// refusal(): the entry's remaining argument checks, RFX_OK or its fail().  slots(r0, rows, T, spec, smag, stream): queue the entry's
// slot kernel for the rows r0 .. r0 + rows - 1 - spec the group's spectrum (with d_wave), smag the slots to write.
template <class Refusal, class Slots>
static int mel_bwd_run(const std::string& w, const rfx_plan* plan, bool ptrs_ok, const float* d_wave, const cf* d_angles, int B, int Lw, bool loop,
                       float* d_grad_wave, void* d_workspace, size_t workspace_bytes, void* stream_, Refusal refusal, Slots slots) {
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_grad_wave || !d_workspace || !ptrs_ok) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (int rc = refusal()) return rc;
  const MelBwdLayout l = mel_bwd_layout(plan, B, Lw, d_wave != nullptr, loop);
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int T = l.T;
  cf* spec = reinterpret_cast<cf*>((char*)d_workspace + l.spec);
  float* smag = reinterpret_cast<float*>((char*)d_workspace + l.smag);
  float* frames = reinterpret_cast<float*>((char*)d_workspace + l.frames);
  const size_t row_slots = (size_t)T * plan->frame_stride;
  for (int r0 = 0; r0 < B; r0 += l.group_rows) {
    const int rows = B - r0 < l.group_rows ? B - r0 : l.group_rows;
    if (d_wave)
      if (int rc = (loop ? rfx_stft_loop : rfx_stft)(plan, d_wave + (size_t)r0 * Lw, rows, Lw, nullptr, spec, stream_)) return rc;
    RFX_HIP(slots(r0, rows, T, spec, smag, stream));
    if (int rc = mel_bwd_frames(plan, smag, d_wave ? spec : d_angles + (size_t)r0 * row_slots, frames, rows, T, stream)) return rc;
    RFX_HIP(launch_mel_bwd_fold(mel_bwd_fold_args(plan, frames, d_grad_wave + (size_t)r0 * Lw, rows, T, Lw), loop, stream));
  }
  return RFX_OK;
}

// rfx_mel_from_waveform_backward (d_wave and d_grad_mel) and rfx_stft_backward (d_grad_spec_slots): mel_bwd_spec_kernel's slots
static int mel_bwd_entry(const char* who, bool fused, const rfx_plan* plan, const float* d_wave, const float* d_grad_mel, const void* d_grad_spec_slots, int B, int Lw,
                         float* d_grad_wave, void* d_workspace, size_t workspace_bytes, void* stream) {
  const std::string w = who;
  auto refusal = [&] {
    if (fused && !plan->d_mb_wt) return fail(RFX_ERR_INVALID, w + ": plan was created without a mel filterbank");
    if (int rc = fwd_length_refusal(plan, Lw, false, who)) return rc;
    if (((uintptr_t)d_workspace | (uintptr_t)d_grad_spec_slots) & 15 || ((uintptr_t)d_grad_wave | (uintptr_t)d_wave | (uintptr_t)d_grad_mel) & 3)
      return fail(RFX_ERR_INVALID, w + ": d_workspace and d_grad_spec_slots must be 16-byte aligned, the float tensors 4-byte aligned");
    if ((plan->mb_sstride & 3) || (plan->frame_stride & 1)) return fail(RFX_ERR_UNSUPPORTED, w + ": the plan's frame strides are not multiples of four");
    return (int)RFX_OK;
  };
  auto slots = [&](int r0, int rows, int T, const cf* spec, float* smag, hipStream_t s) {
    const int M = plan->p.n_mels;
    MelBwdSpecArgs a{};
    a.g_mel = fused ? d_grad_mel + (size_t)r0 * M * T : nullptr;
    a.X = fused ? spec : nullptr;
    a.S = smag;
    a.pos_bin = plan->d_mb_pos_bin;
    a.xpos_bin = plan->d_mb_xpos_bin;
    a.s2x = plan->d_mb_s2x;
    a.first = plan->d_mb_first;
    a.count = plan->d_mb_count;
    a.wt = plan->d_mb_wt;
    a.width = plan->mb_width;
    a.B = rows;
    a.T = T;
    a.M = fused ? M : 0;
    a.n_stft = plan->n_stft;
    a.n_fft = plan->p.n_fft;
    a.xstride = plan->frame_stride;
    a.sstride = plan->mb_sstride;
    a.unit = mel_bwd_unit(plan->p.n_fft, !plan->generic);
    return launch_mel_bwd_spec(a, s);
  };
  return mel_bwd_run(w, plan, fused ? d_wave && d_grad_mel : d_grad_spec_slots != nullptr, fused ? d_wave : nullptr,
                     reinterpret_cast<const cf*>(d_grad_spec_slots), B, Lw, false, d_grad_wave, d_workspace, workspace_bytes, stream, refusal, slots);
}

int rfx_stft_backward(const rfx_plan* plan, const void* d_grad_spec_slots, int B, int Lw, float* d_grad_wave, void* d_workspace,
                      size_t workspace_bytes, void* stream) {
  return mel_bwd_entry("rfx_stft_backward", false, plan, nullptr, nullptr, d_grad_spec_slots, B, Lw, d_grad_wave, d_workspace, workspace_bytes, stream);
}

int rfx_mel_from_waveform_backward(const rfx_plan* plan, const float* d_wave, const float* d_grad_mel, int B, int Lw, float* d_grad_wave,
                                   void* d_workspace, size_t workspace_bytes, void* stream) {
  return mel_bwd_entry("rfx_mel_from_waveform_backward", true, plan, d_wave, d_grad_mel, nullptr, B, Lw, d_grad_wave, d_workspace, workspace_bytes, stream);
}

int rfx_mel_scale_backward(const rfx_plan* plan, const float* d_grad_mel, int B, int T, float* d_grad_lin_bft, void* d_workspace,
                           size_t workspace_bytes, void* stream) {
  (void)d_workspace, (void)workspace_bytes;
  if (B < 0) return fail(RFX_ERR_INVALID, "rfx_mel_scale_backward: B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_grad_mel || !d_grad_lin_bft || T <= 0) return fail(RFX_ERR_INVALID, "rfx_mel_scale_backward: bad argument");
  if (!plan->d_mb_wt) return fail(RFX_ERR_INVALID, "rfx_mel_scale_backward: plan was created without a mel filterbank");
  if (((uintptr_t)d_grad_mel | (uintptr_t)d_grad_lin_bft) & 3) return fail(RFX_ERR_INVALID, "rfx_mel_scale_backward: the tensors must be 4-byte aligned");
  if (plan->n_stft > 65535) return fail(RFX_ERR_UNSUPPORTED, "rfx_mel_scale_backward: more than 65535 linear bins");
  RFX_ON_DEVICE(plan->device);
  RFX_HIP(launch_mel_bwd_bank(d_grad_mel, d_grad_lin_bft, plan->d_mb_first, plan->d_mb_count, plan->d_mb_wt, plan->mb_width, B, plan->p.n_mels, T,
                              plan->n_stft, (hipStream_t)stream));
  return RFX_OK;
}

// ---- fused spectral losses, backward (rfx_spec_loss_core.h): the driver with spec_loss_slots_kernel's slots, which come from the
// spectrum, the target's slots and the rows' coefficients.  All four engines serve both forms - the chirp-z engine's too: it refuses a
// loop DECODE, its MODE 0 launch and its loop forward exist.
static int spectral_loss_backward_entry(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, const float* d_coef, int B, int Lw,
                                        float log_floor, float* d_grad_wave, void* d_workspace, size_t workspace_bytes, void* stream, bool loop) {
  const std::string w = loop ? "rfx_spectral_loss_backward_loop" : "rfx_spectral_loss_backward";
  auto refusal = [&] {
    if (int rc = fwd_length_refusal(plan, Lw, loop, w.c_str())) return rc;
    if (!spec_loss_floor_ok(log_floor))
      return fail(RFX_ERR_INVALID, w + ": log_floor must be 0 (no log term) or a finite value of at least 1e-18, got " + std::to_string(log_floor));
    if (((uintptr_t)d_workspace | (uintptr_t)d_mag_slots) & 15 || ((uintptr_t)d_grad_wave | (uintptr_t)d_wave | (uintptr_t)d_coef) & 3)
      return fail(RFX_ERR_INVALID, w + ": d_workspace and d_mag_slots must be 16-byte aligned, the other float tensors 4-byte aligned");
    if ((plan->mb_sstride & 3) || (plan->frame_stride & 3)) return fail(RFX_ERR_UNSUPPORTED, w + ": the plan's frame strides are not multiples of four");
    return (int)RFX_OK;
  };
  auto slots = [&](int r0, int rows, int T, const cf* spec, float* smag, hipStream_t s) {
    SpecLossSlotArgs a{};
    a.X = spec;
    a.target = d_mag_slots + (size_t)r0 * T * plan->frame_stride;
    a.coef = d_coef + 2 * (size_t)r0;
    a.S = smag;
    a.pos_bin = plan->d_mb_pos_bin;
    a.s2x = plan->d_mb_s2x;
    a.B = rows;
    a.T = T;
    a.n_fft = plan->p.n_fft;
    a.xstride = plan->frame_stride;
    a.sstride = plan->mb_sstride;
    a.target_by_bin = plan->generic;
    a.unit = mel_bwd_unit(plan->p.n_fft, !plan->generic);
    a.floor = log_floor;
    return launch_spec_loss_slots(a, s);
  };
  return mel_bwd_run(w, plan, d_wave && d_mag_slots && d_coef, d_wave, nullptr, B, Lw, loop, d_grad_wave, d_workspace, workspace_bytes, stream, refusal,
                     slots);
}
int rfx_spectral_loss_backward(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, const float* d_coef, int B, int Lw, float log_floor,
                               float* d_grad_wave, void* d_workspace, size_t workspace_bytes, void* stream) {
  return spectral_loss_backward_entry(plan, d_wave, d_mag_slots, d_coef, B, Lw, log_floor, d_grad_wave, d_workspace, workspace_bytes, stream, false);
}
int rfx_spectral_loss_backward_loop(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, const float* d_coef, int B, int Lw,
                                    float log_floor, float* d_grad_wave, void* d_workspace, size_t workspace_bytes, void* stream) {
  return spectral_loss_backward_entry(plan, d_wave, d_mag_slots, d_coef, B, Lw, log_floor, d_grad_wave, d_workspace, workspace_bytes, stream, true);
}
