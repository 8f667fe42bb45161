// rfx_api_istft.hip - the C ABI of librfx.so (include/rfx.h), "INVERSE SPECTROGRAM": rfx_istft, rfx_istft_loop, rfx_istft_backward,
// rfx_istft_backward_loop.  Host code only: one layout and one driver per direction, the form (plain / loop) an argument.
// Forward, per group of rows:
//     istft_unit_slots_kernel   the magnitude slots: 1 per bin slot (rfx_istft.hip)
//     the engine's MODE 0 per-frame launch on (1, X)              mel_bwd_frames: launch_gl_frame / launch_fam_gl / launch_gen_gl / launch_czt_gl
//     the engine's Griffin-Lim fold into the caller's rows         launch_gl_fold / launch_gen_fold, loop: launch_gl_loop_fold / launch_gen_loop_fold
// Backward, per group of rows:
//     istft_stage_kernel        u = g over the envelope, L samples per row
//     the engine's forward frame launch on u                       plain: its zero-extension twin (stft_zero_extended: launch_stft_zero /
//                                                                  launch_fam_fwd_zero / launch_gen_stft_zero / launch_czt_stft_zero);
//                                                                  loop: the circular one (rfx_stft_loop)
//     istft_grad_kernel         c_k unit and the zero-imaginary rule, into gradient slots
// rfx_debug_istft_backward_padded is the twin's exact test: the plain backward with u padded with zeros to the period
// P' = hop ceil((L + n_fft) / hop) and the circular transform in the twin's place - the same bits, about n_fft / hop frames per row more.
// The envelope tables come from the kernels the folds take them from, once per call.  Rows are walked in groups of whole rows: the
// workspace is bounded whatever B is, and every kernel works frame by frame or sample by sample - a row's bytes depend on that row alone.
#include "rfx_api.h"
#include "rfx_istft_core.h"
#include "rfx_loop_core.h"

using namespace rfx;

static bool istft_specialised(const rfx_plan* plan) { return !plan->generic; }
// samples per row of T frames; 0: the form does not serve T
static int istft_samples(const rfx_plan* plan, int T, bool loop) {
  if (T <= 0) return 0;
  if (loop) return loop_valid(plan->p.hop_length, T, plan->p.n_fft) && !plan->czt ? rfx_griffinlim_loop_output_samples(plan, T) : 0;
  const long long L = (long long)plan->p.hop_length * (T - 1) + (plan->p.n_fft & 1);
  return L > 0 && L + (long long)plan->p.n_fft + 4LL * plan->p.hop_length <= 0x7fffffffLL ? (int)L : 0;
}
// the table both directions take once per call: the fold's of the forward, the staging's of the backward - L floats of the envelope
// rule of the engine's own fold, loop: the hop floats of the period's
static hipError_t istft_table(const rfx_plan* plan, float* tab, int T, int L, bool loop, hipStream_t stream) {
  const bool spec = istft_specialised(plan);
  if (loop) return launch_loop_renv(plan->d_win, tab, plan->p.n_fft, plan->p.win_length, plan->p.hop_length, spec ? 2.0f / (float)plan->p.n_fft : 1.f, stream);
  return spec ? launch_gl_out_scale(plan->d_win, tab, T, L, stream) : launch_gen_env(plan->d_win, tab, plan->gg, T, L, stream);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// The fold's table (L floats, loop: hop), the group's magnitude slots, its synthesis frames
struct IstftLayout {
  size_t tab, smag, frames, total;
  int group_rows, L;
};
static IstftLayout istft_layout(const rfx_plan* plan, int B, int T, bool loop) {
  IstftLayout l{};
  if (B <= 0) return l;
  l.L = istft_samples(plan, T, loop);
  if (l.L <= 0) return IstftLayout{};
  const size_t smag_row = (size_t)T * plan->mb_sstride * sizeof(float), frames_row = (size_t)T * mel_bwd_frame_pitch(plan) * sizeof(float);
  l.group_rows = group_rows(kIstftGroupBytes, smag_row + frames_row, B, kIstftGroupRows);
  Carve c;
  l.tab = c.take((size_t)(loop ? plan->p.hop_length : l.L) * sizeof(float));
  l.smag = c.take((size_t)l.group_rows * smag_row);
  l.frames = c.take((size_t)l.group_rows * frames_row);
  l.total = c.at;
  return l;
}
size_t rfx_istft_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? istft_layout(plan, B, T, false).total : 0; }
size_t rfx_istft_loop_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? istft_layout(plan, B, T, true).total : 0; }

// the refusal of a frame count the form does not serve (after the null checks)
static int istft_frames_refusal(const rfx_plan* plan, int T, bool loop, const std::string& w) {
  if (loop && plan->czt) return fail(RFX_ERR_UNSUPPORTED, w + ": the chirp-z engine has no loop synthesis");
  if (istft_samples(plan, T, loop) > 0) return RFX_OK;
  if (loop)
    return fail(RFX_ERR_INVALID, w + ": a loop call needs hop_length * T >= n_fft (a frame covers the period at most once): at least " +
                                     std::to_string(loop_min_frames(plan->p.hop_length, plan->p.n_fft)) + " frames, got " + std::to_string(T));
  return fail(RFX_ERR_INVALID, w + ": " + std::to_string(T) + " frames give no sample (hop_length * (T - 1) + n_fft % 2 must be positive and fit 31 bits)");
}

static int istft_run(const rfx_plan* plan, const void* d_spec_slots, int B, int T, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                     void* stream_, bool loop) {
  const std::string w = loop ? "rfx_istft_loop" : "rfx_istft";
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_spec_slots || !d_wave_out || !d_workspace) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (int rc = istft_frames_refusal(plan, T, loop, w)) return rc;
  if (((uintptr_t)d_workspace | (uintptr_t)d_spec_slots) & 15 || ((uintptr_t)d_wave_out & 3))
    return fail(RFX_ERR_INVALID, w + ": d_workspace and d_spec_slots must be 16-byte aligned, d_wave_out 4-byte aligned");
  if (plan->mb_sstride & 3) return fail(RFX_ERR_UNSUPPORTED, w + ": the plan's slot stride is not a multiple of four");
  const IstftLayout l = istft_layout(plan, B, T, loop);
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int L = l.L;
  const bool spec = istft_specialised(plan);
  float* tab = reinterpret_cast<float*>((char*)d_workspace + l.tab);
  float* smag = reinterpret_cast<float*>((char*)d_workspace + l.smag);
  float* frames = reinterpret_cast<float*>((char*)d_workspace + l.frames);
  RFX_HIP(istft_table(plan, tab, T, L, loop, stream));
  const size_t row_slots = (size_t)T * plan->frame_stride;
  for (int r0 = 0; r0 < B; r0 += l.group_rows) {
    const int rows = B - r0 < l.group_rows ? B - r0 : l.group_rows;
    const cf* X = reinterpret_cast<const cf*>(d_spec_slots) + (size_t)r0 * row_slots;
    float* out = d_wave_out + (size_t)r0 * L;
    RFX_HIP(launch_istft_unit_slots(smag, plan->d_mb_pos_bin, (long long)rows * T, plan->mb_sstride, stream));
    if (int rc = mel_bwd_frames(plan, smag, X, frames, rows, T, stream)) return rc;
    if (spec) {
      if (loop) RFX_HIP(launch_gl_loop_fold(frames, plan->d_win, tab, out, rows, T, (size_t)L, stream));
      else RFX_HIP(launch_gl_fold(frames, plan->d_win, tab, out, rows, T, L, (size_t)L, stream));
    } else {
      if (loop) RFX_HIP(launch_gen_loop_fold(frames, tab, out, plan->gg, rows, T, (size_t)L, stream, nullptr, nullptr, 0.f, nullptr));
      else RFX_HIP(launch_gen_fold(frames, tab, out, plan->gg, rows, T, L, (size_t)L, stream));
    }
  }
  return RFX_OK;
}
int rfx_istft(const rfx_plan* plan, const void* d_spec_slots, int B, int T, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
              void* stream) {
  return istft_run(plan, d_spec_slots, B, T, d_wave_out, d_workspace, workspace_bytes, stream, false);
}
int rfx_istft_loop(const rfx_plan* plan, const void* d_spec_slots, int B, int T, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                   void* stream) {
  return istft_run(plan, d_spec_slots, B, T, d_wave_out, d_workspace, workspace_bytes, stream, true);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// The staging table (L floats, loop: hop), the group's staged rows u, their analysis frames (Tp per row: T, or the padded period's)
struct IstftBwdLayout {
  size_t tab, u, spec, total;
  int group_rows, L, Tp;
};
// (padded: the debug entry's - rows of Tp = istft_pad_frames hops and as many analysis frames; else L samples and T frames per row)
static IstftBwdLayout istft_backward_layout(const rfx_plan* plan, int B, int T, bool loop, bool padded = false) {
  IstftBwdLayout l{};
  if (B <= 0) return l;
  l.L = istft_samples(plan, T, loop);
  if (l.L <= 0) return IstftBwdLayout{};
  l.Tp = padded ? istft_pad_frames(plan->p.hop_length, plan->p.n_fft, l.L) : T;
  const size_t u_row = (padded ? (size_t)l.Tp * plan->p.hop_length : (size_t)l.L) * sizeof(float), spec_row = (size_t)l.Tp * plan->frame_stride * sizeof(cf);
  l.group_rows = group_rows(kIstftGroupBytes, u_row + spec_row, B, kIstftGroupRows);
  Carve c;
  l.tab = c.take((size_t)(loop ? plan->p.hop_length : l.L) * sizeof(float));
  l.u = c.take((size_t)l.group_rows * u_row + 16);  // the staging writes whole 16 bytes
  l.spec = c.take((size_t)l.group_rows * spec_row);
  l.total = c.at;
  return l;
}
size_t rfx_istft_backward_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? istft_backward_layout(plan, B, T, false).total : 0; }
size_t rfx_istft_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? istft_backward_layout(plan, B, T, true).total : 0;
}
size_t rfx_debug_istft_backward_padded_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan ? istft_backward_layout(plan, B, T, false, true).total : 0;
}

static int istft_backward_run(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots, void* d_workspace,
                              size_t workspace_bytes, void* stream_, bool loop, bool padded = false) {
  const std::string w = padded ? "rfx_debug_istft_backward_padded" : loop ? "rfx_istft_backward_loop" : "rfx_istft_backward";
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_grad_wave || !d_grad_spec_slots || !d_workspace) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (int rc = istft_frames_refusal(plan, T, loop, w)) return rc;
  if (((uintptr_t)d_workspace | (uintptr_t)d_grad_spec_slots) & 15 || ((uintptr_t)d_grad_wave & 3))
    return fail(RFX_ERR_INVALID, w + ": d_workspace and d_grad_spec_slots must be 16-byte aligned, d_grad_wave 4-byte aligned");
  if (plan->frame_stride & 1) return fail(RFX_ERR_UNSUPPORTED, w + ": the plan's frame stride is odd");
  const IstftBwdLayout l = istft_backward_layout(plan, B, T, loop, padded);
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  const int L = l.L, n_fft = plan->p.n_fft, hop = plan->p.hop_length;
  const int P = padded ? l.Tp * hop : L;  // samples per staged row; the circular forms: the period, a whole number of hops of at least n_fft
  // (the last refusal: nothing below this line answers anything but a HIP error - rfx_stft_loop's own length rule holds by the layout)
  if ((loop || padded) && !loop_samples_valid(hop, n_fft, P)) return fail(RFX_ERR_INVALID, w + ": the staged period is no whole loop");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  const bool spec = istft_specialised(plan);
  float* tab = reinterpret_cast<float*>((char*)d_workspace + l.tab);
  float* u = reinterpret_cast<float*>((char*)d_workspace + l.u);
  cf* X = reinterpret_cast<cf*>((char*)d_workspace + l.spec);
  RFX_HIP(istft_table(plan, tab, T, L, loop, stream));
  for (int r0 = 0; r0 < B; r0 += l.group_rows) {
    const int rows = B - r0 < l.group_rows ? B - r0 : l.group_rows;
    IstftStageArgs s{};
    s.g = d_grad_wave + (size_t)r0 * L;
    s.tab = tab;
    s.u = u;
    s.total = (long long)rows * P;
    s.pitch = P;
    s.valid = L;
    s.period = loop ? hop : 0;
    s.divide = !loop && !spec;
    RFX_HIP(launch_istft_stage(s, stream));
    if (loop || padded) {
      if (int rc = rfx_stft_loop(plan, u, rows, P, nullptr, X, stream_)) return rc;
    } else if (int rc = stft_zero_extended(plan, u, rows, L, T, X, stream_)) {
      return rc;
    }
    IstftGradArgs a{};
    a.spec = X;
    a.out = reinterpret_cast<cf*>(d_grad_spec_slots) + (size_t)r0 * T * plan->frame_stride;
    a.xpos_bin = plan->d_mb_xpos_bin;
    a.rows = rows;
    a.T = T;
    a.Tp = l.Tp;
    a.xstride = plan->frame_stride;
    a.n_fft = n_fft;
    a.unit = istft_unit(n_fft, spec);
    RFX_HIP(launch_istft_grad(a, stream));
  }
  return RFX_OK;
}
int rfx_istft_backward(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
  return istft_backward_run(plan, d_grad_wave, B, T, d_grad_spec_slots, d_workspace, workspace_bytes, stream, false);
}
int rfx_istft_backward_loop(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  return istft_backward_run(plan, d_grad_wave, B, T, d_grad_spec_slots, d_workspace, workspace_bytes, stream, true);
}
int rfx_debug_istft_backward_padded(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
  return istft_backward_run(plan, d_grad_wave, B, T, d_grad_spec_slots, d_workspace, workspace_bytes, stream, false, true);
}
