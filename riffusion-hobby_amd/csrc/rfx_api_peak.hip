// rfx_api_peak.hip - the C ABI of librfx.so (include/rfx.h): the spectral-peak start of Griffin-Lim, standalone, and what the
// inverse entries (rfx_api_inverse.hip) take from it when a call asks for that start.  Host code only.
#include "rfx_api.h"
#include "rfx_holdmask_core.h"
#include "rfx_peak_core.h"

using namespace rfx;

namespace {
// the owner of every bin, then position / phase of every peak (by bin)
struct PeakLayout {
  size_t own, val, total;
};
PeakLayout peak_layout(const rfx_plan* plan, int B, int T) {
  PeakLayout l{};
  if (B <= 0 || T <= 0) return l;
  const size_t n = (size_t)B * T * plan->n_stft;
  Carve c;
  l.own = c.take(n * sizeof(uint16_t));
  l.val = c.take(n * sizeof(double));
  l.total = c.at;
  return l;
}
}  // namespace

namespace rfx {
int peak_refusal(const rfx_plan* plan, const char* who) {
  if (plan->n_stft > kPeakMaxBins || peak_chain_lds_bytes(plan->n_stft) > 160 * 1024 || peak_owner_lds_bytes(plan->n_stft) > 160 * 1024)
    return fail(RFX_ERR_UNSUPPORTED, std::string(who) + ": the spectral-peak start keeps two doubles per bin of a frame in LDS: n_stft = " +
                                         std::to_string(plan->n_stft) + " is above the " + std::to_string(kPeakMaxBins) + " that 160 KiB hold");
  return RFX_OK;
}
size_t peak_scratch_bytes(const rfx_plan* plan, int B, int T) { return peak_layout(plan, B, T).total; }
size_t peak_angles_bytes(const rfx_plan* plan, int B, int T) {
  return B <= 0 || T <= 0 ? 0 : align_up((size_t)B * T * plan->frame_stride * sizeof(cf), 256);
}
size_t peak_extra_bytes(const rfx_plan* plan, int B, int T) { return peak_angles_bytes(plan, B, T) + peak_scratch_bytes(plan, B, T); }

int peak_start_run(const rfx_plan* plan, int layout, const float* d_mag, int B, int T, void* d_angles, void* d_scratch, hipStream_t stream) {
  const PeakLayout w = peak_layout(plan, B, T);
  char* ws = (char*)d_scratch;
  const int stride_in = layout == kHoldMaskTable ? plan->fam.fsf : plan->frame_stride;
  RFX_HIP(launch_peak_start(layout, d_mag, layout == kHoldMaskTable ? plan->d_fam_binof : nullptr, B, T, stride_in, plan->n_stft, plan->p.hop_length,
                            plan->p.n_fft, (uint16_t*)(ws + w.own), (double*)(ws + w.val), (cf*)d_angles, plan->frame_stride, stream));
  return RFX_OK;
}
}  // namespace rfx

size_t rfx_peak_start_workspace_bytes(const rfx_plan* plan, int B, int T) { return plan ? peak_scratch_bytes(plan, B, T) : 0; }

int rfx_peak_start(const rfx_plan* plan, const float* d_mag_slots, int B, int T, void* d_angles0_slots_out, void* d_workspace,
                   size_t workspace_bytes, void* stream) {
  if (!plan) return fail(RFX_ERR_INVALID, "rfx_peak_start: null argument");
  if (B == 0) return RFX_OK;
  if (!d_mag_slots || !d_angles0_slots_out || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_peak_start: null argument");
  if (B < 0 || T <= 0) return fail(RFX_ERR_INVALID, "rfx_peak_start: bad shape");
  if ((long long)B * T > 0x7fffffffLL) return fail(RFX_ERR_INVALID, "rfx_peak_start: more than 2^31 - 1 frames in one call");
  if (int rc = peak_refusal(plan, "rfx_peak_start")) return rc;
  if (workspace_bytes < peak_scratch_bytes(plan, B, T)) return fail(RFX_ERR_WORKSPACE, "rfx_peak_start: workspace too small");
  if ((uintptr_t)d_workspace & 7) return fail(RFX_ERR_INVALID, "rfx_peak_start: d_workspace must be aligned to 8 bytes");
  RFX_ON_DEVICE(plan->device);
  return peak_start_run(plan, plan->generic ? kHoldMaskPlain : kHoldMaskSpec, d_mag_slots, B, T, d_angles0_slots_out, d_workspace, (hipStream_t)stream);
}
