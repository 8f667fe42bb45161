// rfx_api_forward.hip - the C ABI of librfx.so (include/rfx.h), forward half: layout conversion, STFT, the mel projections and
// the image of a waveform or of int16 clips, and the per-row spectral sums (spectral error, spectral loss).  Host code only: the
// drivers that sequence the kernels.
#include "rfx_api.h"
#include "rfx_loop_core.h"
#include "rfx_spec_loss_core.h"

using namespace rfx;

// ---- the two forms of every forward entry.  Plain: the row is reflect-padded by n_fft / 2 on both sides (torch.stft center=True) and
// must be longer than that.  Loop (the *_loop entries; rfx_loop_core.h): the row is one period of exactly hop T samples and is read
// modulo its length.  Each driver below is written once and takes the form as `loop`; the two differ in the frame count, the length
// rule (fwd_frames, fwd_length_ok, fwd_length_refusal: rfx_api.h) and the launcher (the loop twin of the same kernel).
// the refusal of a row length a loop forward call does not take, with the nearest lengths it does
static int loop_samples_refusal(int hop, int n_fft, int Lw, const char* who) {
  if (loop_samples_valid(hop, n_fft, Lw)) return RFX_OK;
  const long long below = loop_samples_below(hop, n_fft, Lw), above = loop_samples_above(hop, n_fft, Lw);
  return fail(RFX_ERR_INVALID, std::string(who) + ": a loop call takes rows of one whole period, hop_length * T samples with hop_length * T >= n_fft (hop_length " +
                                   std::to_string(hop) + ", n_fft " + std::to_string(n_fft) + "), got " + std::to_string(Lw) + ": the nearest legal lengths are " +
                                   (below ? std::to_string(below) + " (" + std::to_string(below / hop) + " frames)" : std::string("none")) + " below and " +
                                   std::to_string(above) + " (" + std::to_string(above / hop) + " frames) above");
}
// the refusal of a row length a forward call of either form does not take; RFX_OK for a legal one
int rfx::fwd_length_refusal(const rfx_plan* plan, int Lw, bool loop, const char* who) {
  if (loop) return loop_samples_refusal(plan->p.hop_length, plan->p.n_fft, Lw, who);
  if (Lw > plan->p.n_fft / 2) return RFX_OK;
  // torch.stft(center=True, pad_mode="reflect") raises when the pad n_fft/2 is not smaller than the input
  return fail(RFX_ERR_INVALID, std::string(who) + ": reflect padding needs more than n_fft/2 = " + std::to_string(plan->p.n_fft / 2) + " samples");
}
int rfx_debug_loop_samples(const rfx_params* params, int Lw) {
  if (!params || params->hop_length <= 0 || params->n_fft <= 0) return fail(RFX_ERR_INVALID, "rfx_debug_loop_samples: bad argument");
  return loop_samples_refusal(params->hop_length, params->n_fft, Lw, "rfx_debug_loop_samples");
}
int rfx_debug_loop_nearest_samples(const rfx_params* params, int Lw, int64_t* below, int64_t* above) {
  if (!params || params->hop_length <= 0 || params->n_fft <= 0 || !below || !above)
    return fail(RFX_ERR_INVALID, "rfx_debug_loop_nearest_samples: bad argument");
  *below = loop_samples_below(params->hop_length, params->n_fft, Lw);
  *above = loop_samples_above(params->hop_length, params->n_fft, Lw);
  return RFX_OK;
}
int rfx_stft_loop_frames(const rfx_plan* plan, int Lw) { return plan ? fwd_frames(plan, Lw, true) : 0; }

// the forward transform of a row-family plan (rfx_fam.hip): everything but the outputs of the mode that is launched
static FamFwdArgs fam_fwd_args(const rfx_plan* plan, const float* d_wave, int B, int Lw, int T) {
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
  return fa;
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

int rfx_unpack_magnitudes(const rfx_plan* plan, const float* d_slots, int B, int T, float* d_bft, void* stream) {
  if (!plan || !d_bft || !d_slots || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_unpack_magnitudes: bad argument");
  RFX_ON_DEVICE(plan->device);
  if (plan->generic) RFX_HIP(launch_gen_unpack(d_slots, d_bft, false, B, plan->n_stft, T, plan->gg.fs, (hipStream_t)stream));
  else RFX_HIP(launch_unpack_mag(d_slots, d_bft, B, T, (hipStream_t)stream));
  return RFX_OK;
}

enum FwdRule { kFwdReflect = 0, kFwdLoop = 1, kFwdZero = 2 };
static int stft_launch(const rfx_plan* plan, const float* d_wave, int B, int Lw, int T, float* d_mag_slots, void* d_spec_slots, void* stream, int rule);
static int stft_run(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mag_slots, void* d_spec_slots, void* stream, bool loop) {
  if (!plan || !d_wave || B <= 0) return fail(RFX_ERR_INVALID, loop ? "rfx_stft_loop: bad argument" : "rfx_stft: bad argument");
  if (int rc = fwd_length_refusal(plan, Lw, loop, loop ? "rfx_stft_loop" : "rfx_stft")) return rc;
  RFX_ON_DEVICE(plan->device);
  return stft_launch(plan, d_wave, B, Lw, fwd_frames(plan, Lw, loop), d_mag_slots, d_spec_slots, stream, loop ? kFwdLoop : kFwdReflect);
}
// the engine's forward frame launch on checked arguments, by index rule.  kFwdZero (rfx::stft_zero_extended): the complex spectrum only
static int stft_launch(const rfx_plan* plan, const float* d_wave, int B, int Lw, int T, float* d_mag_slots, void* d_spec_slots, void* stream, int rule) {
  const bool loop = rule == kFwdLoop, zero = rule == kFwdZero;
  if (plan->fam_ok) {  // row-family kernels (rfx_fam.hip), same plain layout as the generic engine's
    FamFwdArgs fa = fam_fwd_args(plan, d_wave, B, Lw, T);
    fa.mag = d_mag_slots;
    fa.spec = (cf*)d_spec_slots;
    const int nblocks = frame_blocks(fam_slot_count(plan), B, fa.T);
    if (zero) {
      RFX_HIP(launch_fam_fwd_zero(fa, nblocks, (hipStream_t)stream));
      return RFX_OK;
    }
    const auto launch = loop ? launch_fam_fwd_loop : launch_fam_fwd;
    if (d_mag_slots) RFX_HIP(launch(0, fa, nblocks, (hipStream_t)stream));
    if (d_spec_slots) RFX_HIP(launch(1, fa, nblocks, (hipStream_t)stream));
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
    g.T = T;
    g.Lw = Lw;
    if (plan->czt) {
      const auto launch = zero ? launch_czt_stft_zero : loop ? launch_czt_stft_loop : launch_czt_stft;
      if (d_mag_slots) RFX_HIP(launch(0, g, plan->d_czt_c, plan->d_czt_h, plan->num_cus, (hipStream_t)stream));
      if (d_spec_slots) RFX_HIP(launch(1, g, plan->d_czt_c, plan->d_czt_h, plan->num_cus, (hipStream_t)stream));
      return RFX_OK;
    }
    if (zero) {
      RFX_HIP(launch_gen_stft_zero(g, plan->num_cus, (hipStream_t)stream));
      return RFX_OK;
    }
    const auto launch = loop ? launch_gen_stft_loop : launch_gen_stft;
    if (d_mag_slots) RFX_HIP(launch(0, g, plan->num_cus, (hipStream_t)stream));
    if (d_spec_slots) RFX_HIP(launch(1, g, plan->num_cus, (hipStream_t)stream));
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
  a.T = T;
  const long long frames = (long long)B * a.T;
  int fpb = (int)((frames + 2LL * plan->num_cus - 1) / (2LL * plan->num_cus));
  if (fpb < 1) fpb = 1;
  if (fpb > 16) fpb = 16;
  a.frames_per_block = fpb;
  RFX_HIP(zero ? launch_stft_zero(a, (hipStream_t)stream) : loop ? launch_stft_loop(a, (hipStream_t)stream) : launch_stft(a, (hipStream_t)stream));
  return RFX_OK;
}
// the zero-extended analysis of rfx_istft_backward (rfx_api_istft.hip): `B` rows of L samples, T frames each - frame t, element i reads
// sample hop t + i - n_fft / 2, an exact zero outside [0, L) - into d_spec_slots.  The caller has checked its arguments and set the device.
int rfx::stft_zero_extended(const rfx_plan* plan, const float* d_rows, int B, int L, int T, void* d_spec_slots, void* stream) {
  return stft_launch(plan, d_rows, B, L, T, nullptr, d_spec_slots, stream, kFwdZero);
}
int rfx_stft(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mag_slots, void* d_spec_slots, void* stream) {
  return stft_run(plan, d_wave, B, Lw, d_mag_slots, d_spec_slots, stream, false);
}
int rfx_stft_loop(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mag_slots, void* d_spec_slots, void* stream) {
  return stft_run(plan, d_wave, B, Lw, d_mag_slots, d_spec_slots, stream, true);
}

// ---- mel projection -------------------------------------------------------------------------------------------------------------
// Magnitudes [B*T][frame_stride], then - generic plans - the frame-major mel amplitudes [B*T][Mpad].  The fused kernel of the
// specialised engine keeps the magnitudes on chip: its scratch is the frame-major amplitudes alone.
struct MelLayout {
  size_t mag, mel_tm, total;
};
static MelLayout mel_layout(const rfx_plan* plan, int B, int T, bool mag_on_chip) {
  MelLayout l{};
  if (B <= 0 || T <= 0) return l;
  const size_t nf = (size_t)B * T;
  Carve c;
  l.mag = c.take(mag_on_chip ? 0 : nf * plan->frame_stride * sizeof(float));
  l.mel_tm = c.take(plan->generic || mag_on_chip ? nf * plan->Mpad * sizeof(float) : 0);
  l.total = c.at;
  return l;
}
static MelLayout mel_forward_layout(const rfx_plan* plan, int B, int Lw, bool loop) {
  if (!fwd_length_ok(plan, Lw, loop)) return MelLayout{};
  return mel_layout(plan, B, fwd_frames(plan, Lw, loop), !plan->generic && plan->fwd_ok && !plan->fwd_unfused);
}
size_t rfx_mel_workspace_bytes(const rfx_plan* plan, int B, int Lw) { return plan ? mel_forward_layout(plan, B, Lw, false).total : 0; }
size_t rfx_mel_loop_workspace_bytes(const rfx_plan* plan, int B, int Lw) { return plan ? mel_forward_layout(plan, B, Lw, true).total : 0; }
size_t rfx_mel_scale_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? mel_layout(plan, B, T, false).total : 0; }

// does the plan's forward path leave the mel amplitudes frame-major ([B*T][Mpad]) in the workspace before transposing them?
static bool forward_has_frame_major(const rfx_plan* plan) { return plan->generic ? plan->fwd_ok : (plan->fwd_ok && !plan->fwd_unfused); }

// specialised engine: the MFMA GEMM over slot-ordered magnitudes [B*T][kFrameStride] -> (B, M, T)
static int mel_gemm(const rfx_plan* plan, const float* mag, int B, int T, float* d_mel_out, hipStream_t stream) {
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
  RFX_HIP(launch_mel_gemm(a, stream));
  return RFX_OK;
}
// generic plans: the banded projection of plain magnitudes (mag null: mel_tm holds the amplitudes already) and, where the caller
// wants the tensor, the transpose to (B, M, T)
static int gen_mel(const rfx_plan* plan, const float* mag, float* mel_tm, int B, int T, float* d_mel_out, hipStream_t stream) {
  if (mag)
    RFX_HIP(launch_gen_mel(mag, mel_tm, plan->d_band_wt, plan->d_band_lo, plan->d_band_lo + plan->Mpad, (long long)B * T, plan->gg.fs,
                           plan->p.n_mels, plan->Mpad, plan->imel.f_lo, plan->imel.f_hi, stream));
  if (d_mel_out) RFX_HIP(launch_mel_transpose(mel_tm, d_mel_out, B, T, plan->p.n_mels, plan->Mpad, stream));
  return RFX_OK;
}

// rfx_mel_from_waveform, and the front half of rfx_image_from_waveform: there d_mel_out is null (no (B, M, T) copy is made),
// *mel_tm_out receives the frame-major amplitudes and - where the kernel can take it on the fly - max_keys the keys of the maxima its
// workgroups formed, *keys_per_row of them for every row, rows in order (0: it did not; up to T per row: image_keys_bytes)
// loop: the *_loop form of either (rows of one period, the loop twins of the same kernels)
static int mel_forward(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace, size_t workspace_bytes,
                       void* stream_, float** mel_tm_out, unsigned* max_keys, int max_group, int* keys_per_row, bool loop) {
  const std::string who = loop ? "rfx_mel_from_waveform_loop" : "rfx_mel_from_waveform";
  if (!plan || !d_wave || !d_workspace || (!d_mel_out && !mel_tm_out)) return fail(RFX_ERR_INVALID, who + ": null argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, who + ": plan was created without a mel filterbank");
  if (int rc = fwd_length_refusal(plan, Lw, loop, who.c_str())) return rc;
  const MelLayout w = mel_forward_layout(plan, B, Lw, loop);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, who + ": workspace too small");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  float* mag = (float*)((char*)d_workspace + w.mag);
  float* mel_tm = (float*)((char*)d_workspace + w.mel_tm);
  const int T = fwd_frames(plan, Lw, loop);
  if (plan->generic) {
    if (!plan->fwd_ok) return fail(RFX_ERR_UNSUPPORTED, who + ": filterbank is not banded: " + plan->imel_why);
    const bool fused = plan->fam_ok && !plan->fwd_unfused;
    if (fused) {  // row family: transform and banded projection in one kernel, |X| stays on chip
      FamFwdArgs fa = fam_fwd_args(plan, d_wave, B, Lw, T);
      fa.mel_tm = mel_tm;
      fa.band_wt = plan->d_band_wt;
      fa.band_lo = plan->d_band_lo;
      fa.band_len = plan->d_band_lo + plan->Mpad;
      fa.M = plan->p.n_mels;
      fa.Mpad = plan->Mpad;
      RFX_HIP((loop ? launch_fam_fwd_loop : launch_fam_fwd)(2, fa, frame_blocks(fam_slot_count(plan), B, T), stream));
    } else if (int rc = stft_run(plan, d_wave, B, Lw, mag, nullptr, stream, loop)) {
      return rc;
    }
    if (mel_tm_out) *mel_tm_out = mel_tm;
    return gen_mel(plan, fused ? nullptr : mag, mel_tm, B, T, d_mel_out, stream);
  }
  if (plan->fwd_ok && !plan->fwd_unfused) {
    StftMelArgs f;
    f.wave = d_wave;
    f.mel = d_mel_out;
    f.mel_tm = mel_tm;
    f.tw1 = plan->d_tw1;
    f.tw2 = plan->d_tw2;
    f.win = plan->d_win;
    f.band_wt = plan->d_band_wt;
    f.band_addr = plan->d_band_addr;
    f.band_lo = plan->d_band_lo;
    f.band_len = plan->d_band_lo + plan->Mpad;
    f.B = B;
    f.Lw = Lw;
    f.T = T;
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
    RFX_HIP(loop ? launch_stft_mel_loop(f, stream) : launch_stft_mel(f, stream));
    return RFX_OK;
  }
  if (!d_mel_out) return fail(RFX_ERR_INVALID, who + ": this plan's forward path has no frame-major stage");
  if (int rc = stft_run(plan, d_wave, B, Lw, mag, nullptr, stream, loop)) return rc;
  return mel_gemm(plan, mag, B, T, d_mel_out, stream);
}

int rfx_mel_from_waveform(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  if (!d_mel_out) return fail(RFX_ERR_INVALID, "rfx_mel_from_waveform: null argument");
  return mel_forward(plan, d_wave, B, Lw, d_mel_out, d_workspace, workspace_bytes, stream, nullptr, nullptr, 1, nullptr, false);
}
int rfx_mel_from_waveform_loop(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace,
                               size_t workspace_bytes, void* stream) {
  if (!d_mel_out) return fail(RFX_ERR_INVALID, "rfx_mel_from_waveform_loop: null argument");
  return mel_forward(plan, d_wave, B, Lw, d_mel_out, d_workspace, workspace_bytes, stream, nullptr, nullptr, 1, nullptr, true);
}

// ---- spectrogram_image_from_audio's device half (spectrogram_image_converter.py:30-51: spectrogram_from_audio, then
// image_util.image_from_spectrogram): waveforms -> mel amplitudes -> uint8 image without the (B, M, T) tensor in between.
// The forward path's workspace, then the keys of its maxima - the forward kernel leaves one per workgroup, at most one workgroup
// per frame - and, for a plan without a frame-major stage, the (B, M, T) tensor.
struct ImageFwdLayout {
  size_t keys, mel, total;  // keys is also the size of the forward path's part, which starts the workspace
};
static ImageFwdLayout image_from_waveform_layout(const rfx_plan* plan, int N, int stereo, int Lw, bool loop) {
  ImageFwdLayout l{};
  if (N <= 0) return l;
  const int B = N * (stereo ? 2 : 1);
  Carve c;
  c.at = mel_forward_layout(plan, B, Lw, loop).total;
  if (!c.at) return l;
  const size_t T = (size_t)fwd_frames(plan, Lw, loop);
  l.keys = c.take((size_t)B * T * sizeof(unsigned));
  l.mel = c.take(forward_has_frame_major(plan) ? 0 : (size_t)B * plan->p.n_mels * T * sizeof(float));
  l.total = c.at;
  return l;
}
size_t rfx_image_from_waveform_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw) {
  return plan ? image_from_waveform_layout(plan, N, stereo, Lw, false).total : 0;
}
size_t rfx_image_from_waveform_loop_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw) {
  return plan ? image_from_waveform_layout(plan, N, stereo, Lw, true).total : 0;
}

static int image_from_waveform_run(const rfx_plan* plan, const float* d_wave, int N, int stereo, int Lw, const float* d_thresholds255, float* d_clip_max,
                                   uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream, bool loop) {
  const std::string who = loop ? "rfx_image_from_waveform_loop" : "rfx_image_from_waveform";
  if (!plan || !d_wave || !d_thresholds255 || !d_clip_max || !d_img_out || !d_workspace || N <= 0)
    return fail(RFX_ERR_INVALID, who + ": bad argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, who + ": plan was created without a mel filterbank");
  if (int rc = fwd_length_refusal(plan, Lw, loop, who.c_str())) return rc;
  const ImageFwdLayout w = image_from_waveform_layout(plan, N, stereo, Lw, loop);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, who + ": workspace too small");
  RFX_ON_DEVICE(plan->device);
  const int C = stereo ? 2 : 1, B = N * C, T = fwd_frames(plan, Lw, loop), M = plan->p.n_mels;
  unsigned* keys = reinterpret_cast<unsigned*>((char*)d_workspace + w.keys);
  if (!forward_has_frame_major(plan)) {  // (dense-GEMM fall-back of a non-banded bank: the two calls, the tensor in the workspace)
    float* mel = reinterpret_cast<float*>((char*)d_workspace + w.mel);
    if (int rc = mel_forward(plan, d_wave, B, Lw, mel, d_workspace, w.keys, stream, nullptr, nullptr, 1, nullptr, loop)) return rc;
    return rfx_image_encode_u8(mel, N, M, T, stereo, d_thresholds255, d_clip_max, d_img_out, stream);
  }
  float* mel_tm = nullptr;
  int keys_per_row = 0;  // (round 6: one key per workgroup of the forward kernel, every one written by the launch: nothing to zero)
  if (int rc = mel_forward(plan, d_wave, B, Lw, nullptr, d_workspace, w.keys, stream, &mel_tm, keys, C, &keys_per_row, loop)) return rc;
  // (a kernel that does not take the maximum on the fly: one pass over the frame-major amplitudes; their padding columns are zero
  // and mel amplitudes are not negative)
  if (!keys_per_row) RFX_HIP(launch_clip_max(mel_tm, reinterpret_cast<float*>(keys), N, (size_t)C * T * plan->Mpad, false, (hipStream_t)stream));
  RFX_HIP(launch_image_encode_tm(mel_tm, keys_per_row ? keys : nullptr, C * keys_per_row, keys_per_row ? nullptr : reinterpret_cast<const float*>(keys),
                                 d_thresholds255, d_img_out, d_clip_max, N, M, plan->Mpad, T, C, (hipStream_t)stream));
  return RFX_OK;
}
int rfx_image_from_waveform(const rfx_plan* plan, const float* d_wave, int N, int stereo, int Lw, const float* d_thresholds255,
                            float* d_clip_max, uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  return image_from_waveform_run(plan, d_wave, N, stereo, Lw, d_thresholds255, d_clip_max, d_img_out, d_workspace, workspace_bytes, stream, false);
}
int rfx_image_from_waveform_loop(const rfx_plan* plan, const float* d_wave, int N, int stereo, int Lw, const float* d_thresholds255,
                                 float* d_clip_max, uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  return image_from_waveform_run(plan, d_wave, N, stereo, Lw, d_thresholds255, d_clip_max, d_img_out, d_workspace, workspace_bytes, stream, true);
}

// ---- the same from int16 clips of one recording (rfx_pcm_in.hip): the gathered (N*C, Lw) float32 rows, then the workspace of
// rfx_image_from_waveform
struct ImagePcmLayout {
  size_t wave, fwd, fwd_bytes, total;
};
static ImagePcmLayout image_from_pcm16_clips_layout(const rfx_plan* plan, int N, int stereo, int Lw, bool loop) {
  ImagePcmLayout l{};
  if (N <= 0 || Lw <= 0) return l;
  l.fwd_bytes = image_from_waveform_layout(plan, N, stereo, Lw, loop).total;
  if (!l.fwd_bytes) return l;
  Carve c;
  l.wave = c.take((size_t)N * (stereo ? 2 : 1) * Lw * sizeof(float));
  l.fwd = c.take(l.fwd_bytes);
  l.total = c.at;
  return l;
}
size_t rfx_image_from_pcm16_clips_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw) {
  return plan ? image_from_pcm16_clips_layout(plan, N, stereo, Lw, false).total : 0;
}
size_t rfx_image_from_pcm16_clips_loop_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw) {
  return plan ? image_from_pcm16_clips_layout(plan, N, stereo, Lw, true).total : 0;
}

static int image_from_pcm16_clips_run(const rfx_plan* plan, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts,
                                      const int64_t* d_starts, int N, int Lw, int stereo, const float* d_thresholds255, float* d_clip_max,
                                      uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream, bool loop) {
  const std::string who = loop ? "rfx_image_from_pcm16_clips_loop" : "rfx_image_from_pcm16_clips";
  if (N < 0) return fail(RFX_ERR_INVALID, who + ": N is negative");
  if (N == 0) return RFX_OK;
  const int C = stereo ? 2 : 1;
  if (int rc = check_pcm_clips(who.c_str(), d_pcm, frames, in_channels, h_starts, N, Lw, C)) return rc;
  if (!plan || !d_starts || !d_thresholds255 || !d_clip_max || !d_img_out || !d_workspace)
    return fail(RFX_ERR_INVALID, who + ": null pointer");
  if (int rc = fwd_length_refusal(plan, Lw, loop, who.c_str())) return rc;
  const ImagePcmLayout w = image_from_pcm16_clips_layout(plan, N, stereo, Lw, loop);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, who + ": workspace too small");
  float* wave = reinterpret_cast<float*>((char*)d_workspace + w.wave);
  {
    RFX_ON_DEVICE(plan->device);
    RFX_HIP(launch_pcm_clips(d_pcm, in_channels, d_starts, N, Lw, C, wave, (hipStream_t)stream));
  }
  return image_from_waveform_run(plan, wave, N, stereo, Lw, d_thresholds255, d_clip_max, d_img_out, (char*)d_workspace + w.fwd, w.fwd_bytes, stream, loop);
}
int rfx_image_from_pcm16_clips(const rfx_plan* plan, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts,
                               const int64_t* d_starts, int N, int Lw, int stereo, const float* d_thresholds255, float* d_clip_max,
                               uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  return image_from_pcm16_clips_run(plan, d_pcm, frames, in_channels, h_starts, d_starts, N, Lw, stereo, d_thresholds255, d_clip_max, d_img_out, d_workspace,
                                    workspace_bytes, stream, false);
}
int rfx_image_from_pcm16_clips_loop(const rfx_plan* plan, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts,
                                    const int64_t* d_starts, int N, int Lw, int stereo, const float* d_thresholds255, float* d_clip_max,
                                    uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  return image_from_pcm16_clips_run(plan, d_pcm, frames, in_channels, h_starts, d_starts, N, Lw, stereo, d_thresholds255, d_clip_max, d_img_out, d_workspace,
                                    workspace_bytes, stream, true);
}

int rfx_mel_scale(const rfx_plan* plan, const float* d_lin_bft, int B, int T, float* d_mel_out, void* d_workspace,
                  size_t workspace_bytes, void* stream_) {
  if (!plan || !d_lin_bft || !d_mel_out || !d_workspace || B <= 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_mel_scale: bad argument");
  if (!plan->d_melfb) return fail(RFX_ERR_INVALID, "rfx_mel_scale: plan was created without a mel filterbank");
  const MelLayout w = mel_layout(plan, B, T, false);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_mel_scale: workspace too small");
  RFX_ON_DEVICE(plan->device);
  hipStream_t stream = (hipStream_t)stream_;
  float* mag = (float*)((char*)d_workspace + w.mag);
  if (plan->generic) {
    if (!plan->fwd_ok) return fail(RFX_ERR_UNSUPPORTED, "rfx_mel_scale: filterbank is not banded: " + plan->imel_why);
    RFX_HIP(launch_gen_pack(d_lin_bft, mag, false, B, plan->n_stft, T, plan->gg.fs, stream));
    return gen_mel(plan, mag, (float*)((char*)d_workspace + w.mel_tm), B, T, d_mel_out, stream);
  }
  RFX_HIP(launch_pack_mag(d_lin_bft, mag, B, T, stream));
  return mel_gemm(plan, mag, B, T, d_mel_out, stream);
}

// ---- the per-row spectral sums: how far the magnitudes of a waveform are from target magnitudes -----------------------------------
// rfx_spectral_error[_loop] (two sums; the rows are a decode's, their length follows from T) and rfx_spectral_loss[_loop] (three sums
// of rfx_quality_core.h; rows of any legal length) are two fronts of one driver: the plan's own forward transform of the rows into
// the workspace (stft_run: any of the frame engines), then the reduction of rfx_quality.hip over that tensor and the target.  The
// rows are walked in groups of whole rows whose magnitudes fill at most kQualGroupBytes (at least one row), so the workspace does not
// grow with the batch: the transformed magnitudes of a group, then the group's partial sums.  A row's result does not depend on the
// group it falls in (rfx_quality_core.h).
constexpr size_t kQualGroupBytes = (size_t)128 << 20;
struct SumsLayout {
  size_t mag, partials, total;
  int group_rows;
};
static SumsLayout sums_layout(const rfx_plan* plan, int B, int T, int nsums) {
  SumsLayout l{};
  const size_t row_bytes = (size_t)T * plan->frame_stride * sizeof(float);
  l.group_rows = group_rows(kQualGroupBytes, row_bytes, B);
  Carve c;
  l.mag = c.take(l.group_rows * row_bytes);
  l.partials = c.take(qual_partials_bytes(l.group_rows, T, nsums));
  l.total = c.at;
  return l;
}
// B > 0 rows of Lw samples, T frames each, on checked arguments: the workspace check and the walk
static int sums_run(const std::string& who, const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int Lw, int T, int nsums,
                    float log_floor, double* d_sums_out, void* d_workspace, size_t workspace_bytes, void* stream, bool loop) {
  const SumsLayout w = sums_layout(plan, B, T, nsums);
  if (workspace_bytes < w.total)
    return fail(RFX_ERR_WORKSPACE, who + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(w.total) + " needed)");
  RFX_ON_DEVICE(plan->device);
  float* mag = reinterpret_cast<float*>((char*)d_workspace + w.mag);
  void* partials = (char*)d_workspace + w.partials;
  const size_t row_elems = (size_t)T * plan->frame_stride;
  for (int r0 = 0; r0 < B; r0 += w.group_rows) {
    const int rows = B - r0 < w.group_rows ? B - r0 : w.group_rows;
    if (int rc = stft_run(plan, d_wave + (size_t)r0 * Lw, rows, Lw, mag, nullptr, stream, loop)) return rc;
    RFX_HIP(launch_spectral_sums(mag, d_mag_slots + (size_t)r0 * row_elems, rows, T, plan->frame_stride, plan->n_stft, plan->generic, nsums, log_floor,
                                 partials, d_sums_out + (size_t)nsums * r0, (hipStream_t)stream));
  }
  return RFX_OK;
}

// rfx_spectral_error: T >= 2 frames, rows of the samples a decode of T frames gives
static bool spectral_error_shape_ok(const rfx_plan* plan, int B, int T, bool loop) {
  if (B <= 0 || T < 2) return false;
  return !loop || (loop_valid(plan->p.hop_length, T, plan->p.n_fft) && (long long)plan->p.hop_length * T <= 0x7fffffffLL);
}
size_t rfx_spectral_error_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan && spectral_error_shape_ok(plan, B, T, false) ? sums_layout(plan, B, T, 2).total : 0;
}
size_t rfx_spectral_error_loop_workspace_bytes(const rfx_plan* plan, int B, int T) {
  return plan && spectral_error_shape_ok(plan, B, T, true) ? sums_layout(plan, B, T, 2).total : 0;
}

// loop: d_wave rows are the hop T samples of a loop decode, transformed by the loop forward call (stft_run)
static int spectral_error_front(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int T, double* d_sums_out, void* d_workspace,
                                size_t workspace_bytes, void* stream, bool loop) {
  const std::string who = loop ? "rfx_spectral_error_loop" : "rfx_spectral_error";
  if (B < 0) return fail(RFX_ERR_INVALID, who + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_wave || !d_mag_slots || !d_sums_out || !d_workspace) return fail(RFX_ERR_INVALID, who + ": null argument");
  if (T < 2) return fail(RFX_ERR_INVALID, who + ": T must be at least 2");
  int L;
  if (loop) {
    const long long P = (long long)plan->p.hop_length * T;
    if (P > 0x7fffffffLL) return fail(RFX_ERR_INVALID, who + ": hop_length * T does not fit an int");
    if (int rc = fwd_length_refusal(plan, (int)P, true, who.c_str())) return rc;
    L = (int)P;
  } else {
    L = rfx_griffinlim_output_samples(plan, T);
    if (L <= plan->p.n_fft / 2 || stft_frames(plan, L) != T)
      return fail(RFX_ERR_INVALID, "rfx_spectral_error: the " + std::to_string(L) + " samples of " + std::to_string(T) +
                                       " frames are not more than the forward transform's reflect padding, n_fft/2 = " + std::to_string(plan->p.n_fft / 2));
  }
  if (((uintptr_t)d_mag_slots | (uintptr_t)d_workspace) & 15 || ((uintptr_t)d_sums_out & 7) || (plan->frame_stride & 3))
    return fail(RFX_ERR_INVALID, who + ": d_mag_slots and d_workspace must be 16-byte aligned, d_sums_out 8-byte aligned");
  return sums_run(who, plan, d_wave, d_mag_slots, B, L, T, 2, 0.f, d_sums_out, d_workspace, workspace_bytes, stream, loop);
}
int rfx_spectral_error(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int T, double* d_sums_out,
                       void* d_workspace, size_t workspace_bytes, void* stream) {
  return spectral_error_front(plan, d_wave, d_mag_slots, B, T, d_sums_out, d_workspace, workspace_bytes, stream, false);
}
int rfx_spectral_error_loop(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int T, double* d_sums_out,
                            void* d_workspace, size_t workspace_bytes, void* stream) {
  return spectral_error_front(plan, d_wave, d_mag_slots, B, T, d_sums_out, d_workspace, workspace_bytes, stream, true);
}

// rfx_spectral_loss: rows of any legal length Lw, the log floor
static size_t spectral_loss_bytes(const rfx_plan* plan, int B, int Lw, bool loop) {
  return plan && B > 0 && fwd_length_ok(plan, Lw, loop) ? sums_layout(plan, B, fwd_frames(plan, Lw, loop), 3).total : 0;
}
size_t rfx_spectral_loss_workspace_bytes(const rfx_plan* plan, int B, int Lw) { return spectral_loss_bytes(plan, B, Lw, false); }
size_t rfx_spectral_loss_loop_workspace_bytes(const rfx_plan* plan, int B, int Lw) { return spectral_loss_bytes(plan, B, Lw, true); }

static int spectral_loss_front(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int Lw, float log_floor, double* d_sums_out,
                               void* d_workspace, size_t workspace_bytes, void* stream, bool loop) {
  const std::string who = loop ? "rfx_spectral_loss_loop" : "rfx_spectral_loss";
  if (B < 0) return fail(RFX_ERR_INVALID, who + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_wave || !d_mag_slots || !d_sums_out || !d_workspace) return fail(RFX_ERR_INVALID, who + ": null argument");
  if (int rc = fwd_length_refusal(plan, Lw, loop, who.c_str())) return rc;
  if (!spec_loss_floor_ok(log_floor))
    return fail(RFX_ERR_INVALID, who + ": log_floor must be 0 (no log term) or a finite value of at least 1e-18, got " + std::to_string(log_floor));
  if (((uintptr_t)d_mag_slots | (uintptr_t)d_workspace) & 15 || ((uintptr_t)d_sums_out & 7) || ((uintptr_t)d_wave & 3) || (plan->frame_stride & 3))
    return fail(RFX_ERR_INVALID, who + ": d_mag_slots and d_workspace must be 16-byte aligned, d_sums_out 8-byte and d_wave 4-byte aligned");
  return sums_run(who, plan, d_wave, d_mag_slots, B, Lw, fwd_frames(plan, Lw, loop), 3, log_floor, d_sums_out, d_workspace, workspace_bytes, stream, loop);
}
int rfx_spectral_loss(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int Lw, float log_floor, double* d_sums_out,
                      void* d_workspace, size_t workspace_bytes, void* stream) {
  return spectral_loss_front(plan, d_wave, d_mag_slots, B, Lw, log_floor, d_sums_out, d_workspace, workspace_bytes, stream, false);
}
int rfx_spectral_loss_loop(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int Lw, float log_floor, double* d_sums_out,
                           void* d_workspace, size_t workspace_bytes, void* stream) {
  return spectral_loss_front(plan, d_wave, d_mag_slots, B, Lw, log_floor, d_sums_out, d_workspace, workspace_bytes, stream, true);
}
