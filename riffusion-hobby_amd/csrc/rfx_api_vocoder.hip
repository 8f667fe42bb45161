// rfx_api_vocoder.hip - the C ABI of librfx.so (include/rfx.h), "TIME STRETCH": rfx_phase_vocoder_frames, rfx_phase_vocoder,
// rfx_time_stretch.  Host code only.  The fused entry is, per group of rows, exactly the composition of three calls the library has:
//     rfx_stft             the group's complex spectrogram, T frames per row
//     launch_vocoder       T frames -> T_out frames per row (rfx_vocoder.hip)
//     rfx_istft            T_out frames -> hop (T_out - 1) (+ n_fft % 2) samples per row, into the caller's rows
// Every one of the three works row by row, so a row's bytes depend on that row alone and the grouping does not show.
#include <cmath>

#include "rfx_api.h"
#include "rfx_vocoder_core.h"

using namespace rfx;

// ---- the frame count ------------------------------------------------------------------------------------------------------------------
static int vocoder_frames(int T, double rate, int* T_out, const std::string& w) {
  if (!(rate > 0.0) || !std::isfinite(rate)) return fail(RFX_ERR_INVALID, w + ": rate must be finite and positive, got " + std::to_string(rate));
  if (T < 1) return fail(RFX_ERR_INVALID, w + ": T must be positive, got " + std::to_string(T));
  const long long n = voc_frames(T, rate);
  if (n < 1) return fail(RFX_ERR_INVALID, w + ": " + std::to_string(T) + " frames at rate " + std::to_string(rate) + " give more than 2^31 - 1 frames");
  *T_out = (int)n;
  return RFX_OK;
}
int rfx_phase_vocoder_frames(int T, double rate, int* T_out) {
  if (!T_out) return fail(RFX_ERR_INVALID, "rfx_phase_vocoder_frames: null argument");
  return vocoder_frames(T, rate, T_out, "rfx_phase_vocoder_frames");
}

// ---- the kernel alone -----------------------------------------------------------------------------------------------------------------
// on checked arguments: rate == 1 copies the rows, as torchaudio returns its input
static int vocoder_launch(const rfx_plan* plan, const cf* in, int rows, int T, int T_out, double rate, cf* out, hipStream_t stream) {
  if (rate == 1.0) {
    RFX_HIP(hipMemcpyAsync(out, in, (size_t)rows * T * plan->frame_stride * sizeof(cf), hipMemcpyDeviceToDevice, stream));
    return RFX_OK;
  }
  VocoderArgs a{};
  a.in = in;
  a.out = out;
  a.table = plan->d_voc_table;
  a.rows = rows;
  a.T = T;
  a.T_out = T_out;
  a.stride = plan->frame_stride;
  a.rate = rate;
  RFX_HIP(launch_vocoder(a, stream));
  return RFX_OK;
}

int rfx_phase_vocoder(const rfx_plan* plan, const void* d_spec_slots, int B, int T, double rate, void* d_out_slots, void* stream) {
  const std::string w = "rfx_phase_vocoder";
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_spec_slots || !d_out_slots) return fail(RFX_ERR_INVALID, w + ": null argument");
  int T_out = 0;
  if (int rc = vocoder_frames(T, rate, &T_out, w)) return rc;
  if (((uintptr_t)d_spec_slots | (uintptr_t)d_out_slots) & 7) return fail(RFX_ERR_INVALID, w + ": d_spec_slots and d_out_slots must be 8-byte aligned");
  if (d_spec_slots == d_out_slots) return fail(RFX_ERR_INVALID, w + ": the call does not work in place");
  RFX_ON_DEVICE(plan->device);
  return vocoder_launch(plan, (const cf*)d_spec_slots, B, T, T_out, rate, (cf*)d_out_slots, (hipStream_t)stream);
}

// ---- the fused entry ------------------------------------------------------------------------------------------------------------------
// The group's two spectrograms, then the workspace rfx_istft asks for a group
struct StretchLayout {
  size_t spec, out, istft, istft_bytes, total;
  int group_rows, T, T_out, L;
};
// (the all-zero layout: B <= 0, a bad rate, a row rfx_stft refuses, a frame count rfx_istft refuses)
static StretchLayout stretch_layout(const rfx_plan* plan, int B, int Lw, double rate) {
  StretchLayout l{};
  if (B <= 0 || !fwd_length_ok(plan, Lw, false)) return l;
  const int T = stft_frames(plan, Lw);
  const long long n = voc_frames(T, rate);
  if (n < 1 || rfx_istft_workspace_bytes(plan, 1, (int)n) == 0) return l;
  l.T = T;
  l.T_out = (int)n;
  l.L = rfx_griffinlim_output_samples(plan, l.T_out);
  const size_t frame = (size_t)plan->frame_stride * sizeof(cf);
  l.group_rows = group_rows(kIstftGroupBytes, ((size_t)l.T + (size_t)l.T_out) * frame, B, kIstftGroupRows);
  Carve c;
  l.spec = c.take((size_t)l.group_rows * l.T * frame);
  l.out = c.take((size_t)l.group_rows * l.T_out * frame);
  l.istft_bytes = rfx_istft_workspace_bytes(plan, l.group_rows, l.T_out);
  l.istft = c.take(l.istft_bytes);
  l.total = c.at;
  return l;
}
size_t rfx_time_stretch_workspace_bytes(const rfx_plan* plan, int B, int Lw, double rate) {
  return plan ? stretch_layout(plan, B, Lw, rate).total : 0;
}
int rfx_time_stretch_samples(const rfx_plan* plan, int Lw, double rate) { return plan ? stretch_layout(plan, 1, Lw, rate).L : 0; }

int rfx_time_stretch(const rfx_plan* plan, const float* d_wave, int B, int Lw, double rate, float* d_wave_out, void* d_workspace,
                     size_t workspace_bytes, void* stream) {
  const std::string w = "rfx_time_stretch";
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_wave || !d_wave_out || !d_workspace) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (int rc = fwd_length_refusal(plan, Lw, false, w.c_str())) return rc;
  int T_out = 0;
  if (int rc = vocoder_frames(stft_frames(plan, Lw), rate, &T_out, w)) return rc;
  const StretchLayout l = stretch_layout(plan, B, Lw, rate);
  if (!l.total)  // rfx_istft's own refusal of T_out, under this entry's name
    return fail(RFX_ERR_INVALID, w + ": " + std::to_string(T_out) + " output frames give no sample (hop_length * (T_out - 1) + n_fft % 2 must be positive and fit 31 bits)");
  if (((uintptr_t)d_workspace & 15) || (((uintptr_t)d_wave | (uintptr_t)d_wave_out) & 3))
    return fail(RFX_ERR_INVALID, w + ": d_workspace must be 16-byte aligned, d_wave and d_wave_out 4-byte aligned");
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  cf* spec = reinterpret_cast<cf*>((char*)d_workspace + l.spec);
  cf* out = reinterpret_cast<cf*>((char*)d_workspace + l.out);
  void* ws = (char*)d_workspace + l.istft;
  for (int r0 = 0; r0 < B; r0 += l.group_rows) {
    const int rows = B - r0 < l.group_rows ? B - r0 : l.group_rows;
    if (int rc = rfx_stft(plan, d_wave + (size_t)r0 * Lw, rows, Lw, nullptr, spec, stream)) return rc;
    {
      RFX_ON_DEVICE(plan->device);
      if (int rc = vocoder_launch(plan, spec, rows, l.T, l.T_out, rate, out, (hipStream_t)stream)) return rc;
    }
    if (int rc = rfx_istft(plan, out, rows, l.T_out, d_wave_out + (size_t)r0 * l.L, ws, l.istft_bytes, stream)) return rc;
  }
  return RFX_OK;
}
