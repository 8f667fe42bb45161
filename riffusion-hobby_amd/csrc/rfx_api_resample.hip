// rfx_api_resample.hip - the C ABI of librfx.so (include/rfx.h), "SINC RESAMPLE" and "PITCH SHIFT": rfx_resample_sinc_frames,
// rfx_resample_sinc_table (both host only), rfx_resample_sinc, rfx_pitch_shift.  Host code only.  The fused entry is, per group of
// rows, exactly the composition
//     rfx_time_stretch     the group's rows at rate 2^(-n_steps / bins_per_octave), Ls samples per row
//     cut or pad           to len_stretch = round(Lw / rate) samples: the resampler reads zeros past min(Ls, len_stretch)
//     launch_resample_sinc int(sample_rate / rate) -> sample_rate, K = ceil(n len_stretch / o) samples per row
//     cut or pad           to Lw: the kernel stores min(K, Lw) samples into the caller's rows, the rest is set to zero
// A tap on a zero takes its fmaf like any other (rfx_resample_core.h), so reading zeros past the row's valid part gives the bytes a
// padded copy would, and every stage works row by row: the grouping does not show.
#include <cmath>

#include "rfx_api.h"
#include "rfx_resample_core.h"
#include "rfx_vocoder_core.h"

using namespace rfx;

static_assert(kRsMaxTableBytes == RFX_RESAMPLE_MAX_TABLE_BYTES, "the cap include/rfx.h states");

// ---- the reduced pair and the output length -------------------------------------------------------------------------------------------
static int resample_frames(int L, int orig, int neu, RsGeom* g, int* K, const std::string& w) {
  if (orig < 1 || neu < 1) return fail(RFX_ERR_INVALID, w + ": frequencies must be positive, got " + std::to_string(orig) + " -> " + std::to_string(neu));
  if (L < 1) return fail(RFX_ERR_INVALID, w + ": L must be positive, got " + std::to_string(L));
  rs_geom(orig, neu, 1, 1.0, g);  // (the pair alone: the filter's width plays no part here)
  const int64_t k = rs_frames(L, g->o, g->n);
  if (k < 0) return fail(RFX_ERR_INVALID, w + ": " + std::to_string(L) + " samples at " + std::to_string(orig) + " -> " + std::to_string(neu) + " give more than 2^31 - 1 samples");
  *K = (int)k;
  return RFX_OK;
}
int rfx_resample_sinc_frames(int L, int orig, int neu, int* K) {
  if (!K) return fail(RFX_ERR_INVALID, "rfx_resample_sinc_frames: null argument");
  RsGeom g;
  return resample_frames(L, orig, neu, &g, K, "rfx_resample_sinc_frames");
}

static int refuse_table(const std::string& w, const RsGeom& g, int ntaps) {
  return fail(RFX_ERR_UNSUPPORTED, w + ": the table of " + std::to_string(g.n) + " phases of " + (ntaps ? std::to_string(ntaps) : std::string("at least one")) +
                                       " float32 taps passes the cap of " + std::to_string(kRsMaxTableBytes >> 20) + " MiB (RFX_RESAMPLE_MAX_TABLE_BYTES)");
}

int rfx_resample_sinc_table(int orig, int neu, int lowpass_filter_width, double rolloff, int32_t* h_first, float* h_taps, int64_t capacity,
                            int32_t* n_out, int32_t* ntaps_out) {
  const std::string w = "rfx_resample_sinc_table";
  if (!n_out || !ntaps_out) return fail(RFX_ERR_INVALID, w + ": null argument");
  RsGeom g;
  if (!rs_geom(orig, neu, lowpass_filter_width, rolloff, &g))
    return fail(RFX_ERR_INVALID, w + ": frequencies and lowpass_filter_width must be positive and rolloff in (0, 1]");
  if (g.n * 4 > kRsMaxTableBytes) return refuse_table(w, g, 0);  // before the walk over the phases
  const int ntaps = rs_ntaps(g);
  if (g.n * ntaps * 4 > kRsMaxTableBytes) return refuse_table(w, g, ntaps);
  if (h_first || h_taps) {
    if (!h_first || !h_taps) return fail(RFX_ERR_INVALID, w + ": h_first and h_taps go together");
    if (capacity < g.n * ntaps)
      return fail(RFX_ERR_INVALID, w + ": the table has " + std::to_string(g.n) + " phases of " + std::to_string(ntaps) + " taps, capacity is " + std::to_string(capacity));
    rs_table(g, ntaps, h_first, h_taps);
  }
  *n_out = (int32_t)g.n;
  *ntaps_out = ntaps;
  return RFX_OK;
}

// ---- the kernel alone -------------------------------------------------------------------------------------------------------------------
// what a caller's table must satisfy as far as the entry can tell
static int check_table(const std::string& w, const RsGeom& g, const int32_t* d_first, const float* d_taps, int ntaps) {
  if (!d_first || !d_taps) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (ntaps < 1) return fail(RFX_ERR_INVALID, w + ": ntaps must be positive, got " + std::to_string(ntaps));
  if (((uintptr_t)d_first | (uintptr_t)d_taps) & 3) return fail(RFX_ERR_INVALID, w + ": d_first and d_taps must be 4-byte aligned");
  if (g.n * ntaps * 4 > kRsMaxTableBytes) return refuse_table(w, g, ntaps);
  return RFX_OK;
}

int rfx_resample_sinc(const float* d_in, int B, int L, int orig, int neu, const int32_t* d_first, const float* d_taps, int ntaps, float* d_out,
                      void* stream) {
  const std::string w = "rfx_resample_sinc";
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!d_in || !d_out) return fail(RFX_ERR_INVALID, w + ": null argument");
  RsGeom g;
  int K = 0;
  if (int rc = resample_frames(L, orig, neu, &g, &K, w)) return rc;
  const bool copy = orig == neu;  // (the table is not read then)
  if (!copy)
    if (int rc = check_table(w, g, d_first, d_taps, ntaps)) return rc;
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 3) return fail(RFX_ERR_INVALID, w + ": d_in and d_out must be 4-byte aligned");
  const uintptr_t in0 = (uintptr_t)d_in, in1 = in0 + (size_t)B * L * sizeof(float), out0 = (uintptr_t)d_out, out1 = out0 + (size_t)B * K * sizeof(float);
  if (in0 < out1 && out0 < in1) return fail(RFX_ERR_INVALID, w + ": d_in and d_out overlap");
  int dev;
  if (int rc = device_of(d_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  if (copy) {  // torchaudio returns its input
    RFX_HIP(hipMemcpyAsync(d_out, d_in, (size_t)B * L * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RFX_OK;
  }
  ResampleArgs a{};
  a.in = d_in;
  a.out = d_out;
  a.first = d_first;
  a.taps = d_taps;
  a.in_stride = a.valid = L;
  a.out_stride = a.K = K;
  a.rows = B;
  a.o = (int)g.o;
  a.n = (int)g.n;
  a.ntaps = ntaps;
  RFX_HIP(launch_resample_sinc(a, (hipStream_t)stream));
  return RFX_OK;
}

// ---- the fused entry ------------------------------------------------------------------------------------------------------------------
// The group's stretched rows, then the workspace rfx_time_stretch asks for a group
struct PitchLayout {
  size_t wave, stretch, stretch_bytes, total;
  int group_rows, Ls, len_stretch, orig, K;
  double rate;
  const char* why;  // the refusal of the all-zero layout
};
static double pitch_rate(double n_steps, int bins_per_octave) { return pow(2.0, -n_steps / (double)bins_per_octave); }
// (the all-zero layout: B <= 0, steps that are not finite, a row rfx_time_stretch refuses, a length or a frequency past 31 bits)
static PitchLayout pitch_layout(const rfx_plan* plan, int B, int Lw, double n_steps, int bins_per_octave) {
  PitchLayout l{};
  l.why = "B must be positive";
  if (B <= 0) return l;
  l.why = "n_steps must be finite and bins_per_octave positive";
  if (!std::isfinite(n_steps) || bins_per_octave < 1) return l;
  const double rate = pitch_rate(n_steps, bins_per_octave);
  l.why = "the shift's rate 2^(-n_steps / bins_per_octave) is not a positive finite number";
  if (!(rate > 0.0) || !std::isfinite(rate)) return l;
  const int Ls = rfx_time_stretch_samples(plan, Lw, rate);
  l.why = "rfx_time_stretch refuses the row length at the shift's rate";
  if (Ls < 1) return l;
  const double len = nearbyint((double)Lw / rate), orig = floor((double)plan->p.sample_rate / rate);  // int(round(.)) and int(.) of torchaudio
  l.why = "the stretched length round(Lw / rate) and the frequency int(sample_rate / rate) must be positive and fit 31 bits";
  if (!(len >= 1.0 && len <= 2147483647.0 && orig >= 1.0 && orig <= 2147483647.0)) return l;
  RsGeom g;
  rs_geom((int)orig, plan->p.sample_rate, 1, 1.0, &g);
  const int64_t K = rs_frames((int64_t)len, g.o, g.n);
  l.why = "the resampled length passes 2^31 - 1";
  if (K < 0) return l;
  const int T = stft_frames(plan, Lw);
  const long long T_out = voc_frames(T, rate);  // (positive: rfx_time_stretch_samples answered)
  const size_t frame = (size_t)plan->frame_stride * sizeof(cf);
  const int rows = group_rows(kIstftGroupBytes, ((size_t)T + (size_t)T_out) * frame, B, kIstftGroupRows);  // rfx_time_stretch's own groups
  const size_t inner = rfx_time_stretch_workspace_bytes(plan, rows, Lw, rate);
  l.why = "rfx_time_stretch refuses the row length at the shift's rate";
  if (!inner) return l;
  l.why = nullptr;
  l.rate = rate;
  l.Ls = Ls;
  l.len_stretch = (int)len;
  l.orig = (int)orig;
  l.K = (int)K;
  l.group_rows = rows;
  Carve c;
  l.wave = c.take((size_t)rows * Ls * sizeof(float));
  l.stretch_bytes = inner;
  l.stretch = c.take(inner);
  l.total = c.at;
  return l;
}
size_t rfx_pitch_shift_workspace_bytes(const rfx_plan* plan, int B, int Lw, double n_steps, int bins_per_octave) {
  if (!plan || n_steps == 0.0) return 0;  // (n_steps == 0 copies: no workspace)
  return pitch_layout(plan, B, Lw, n_steps, bins_per_octave).total;
}
int rfx_pitch_shift_resample_freq(const rfx_plan* plan, int Lw, double n_steps, int bins_per_octave) {
  return plan ? pitch_layout(plan, 1, Lw, n_steps, bins_per_octave).orig : 0;
}

int rfx_pitch_shift(const rfx_plan* plan, const float* d_wave, int B, int Lw, double n_steps, int bins_per_octave, const int32_t* d_first,
                    const float* d_taps, int ntaps, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  const std::string w = "rfx_pitch_shift";
  if (B < 0) return fail(RFX_ERR_INVALID, w + ": B is negative");
  if (B == 0) return RFX_OK;
  if (!plan || !d_wave || !d_wave_out) return fail(RFX_ERR_INVALID, w + ": null argument");
  if (Lw < 1) return fail(RFX_ERR_INVALID, w + ": Lw must be positive, got " + std::to_string(Lw));
  if (((uintptr_t)d_wave | (uintptr_t)d_wave_out) & 3) return fail(RFX_ERR_INVALID, w + ": d_wave and d_wave_out must be 4-byte aligned");
  const size_t bytes = (size_t)B * Lw * sizeof(float);
  if ((uintptr_t)d_wave < (uintptr_t)d_wave_out + bytes && (uintptr_t)d_wave_out < (uintptr_t)d_wave + bytes)
    return fail(RFX_ERR_INVALID, w + ": d_wave and d_wave_out overlap");
  if (n_steps == 0.0) {
    RFX_ON_DEVICE(plan->device);
    RFX_HIP(hipMemcpyAsync(d_wave_out, d_wave, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RFX_OK;
  }
  if (int rc = fwd_length_refusal(plan, Lw, false, w.c_str())) return rc;
  const PitchLayout l = pitch_layout(plan, B, Lw, n_steps, bins_per_octave);
  if (!l.total) return fail(RFX_ERR_INVALID, w + ": " + l.why);
  const bool copy = l.orig == plan->p.sample_rate;  // a shift too small to move the frequency: the resampler returns its input
  RsGeom g;
  rs_geom(l.orig, plan->p.sample_rate, 1, 1.0, &g);
  if (!copy)
    if (int rc = check_table(w, g, d_first, d_taps, ntaps)) return rc;
  if (!d_workspace) return fail(RFX_ERR_INVALID, w + ": null argument");
  if ((uintptr_t)d_workspace & 15) return fail(RFX_ERR_INVALID, w + ": d_workspace must be 16-byte aligned");
  if (workspace_bytes < l.total)
    return fail(RFX_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed)");
  float* stretched = reinterpret_cast<float*>((char*)d_workspace + l.wave);
  void* ws = (char*)d_workspace + l.stretch;
  const int valid = l.Ls < l.len_stretch ? l.Ls : l.len_stretch;         // the stretched row cut to len_stretch; zeros past it
  const int keep = copy ? (valid < Lw ? valid : Lw) : (l.K < Lw ? l.K : Lw);  // samples of a row the resampler gives; zeros past them
  for (int r0 = 0; r0 < B; r0 += l.group_rows) {
    const int rows = B - r0 < l.group_rows ? B - r0 : l.group_rows;
    float* out = d_wave_out + (size_t)r0 * Lw;
    if (int rc = rfx_time_stretch(plan, d_wave + (size_t)r0 * Lw, rows, Lw, l.rate, stretched, ws, l.stretch_bytes, stream)) return rc;
    RFX_ON_DEVICE(plan->device);
    if (copy) {
      RFX_HIP(hipMemcpy2DAsync(out, (size_t)Lw * sizeof(float), stretched, (size_t)l.Ls * sizeof(float), (size_t)keep * sizeof(float), rows,
                               hipMemcpyDeviceToDevice, (hipStream_t)stream));
    } else {
      ResampleArgs a{};
      a.in = stretched;
      a.out = out;
      a.first = d_first;
      a.taps = d_taps;
      a.in_stride = l.Ls;
      a.valid = valid;
      a.out_stride = Lw;
      a.K = keep;
      a.rows = rows;
      a.o = (int)g.o;
      a.n = (int)g.n;
      a.ntaps = ntaps;
      RFX_HIP(launch_resample_sinc(a, (hipStream_t)stream));
    }
    if (keep < Lw)
      RFX_HIP(hipMemset2DAsync(out + keep, (size_t)Lw * sizeof(float), 0, (size_t)(Lw - keep) * sizeof(float), rows, (hipStream_t)stream));
  }
  return RFX_OK;
}
