// rfx_api.h - what the units of the C ABI (rfx_api_*.hip) share: the error helpers, the device guard, struct rfx_plan and the
// workspace-layout helper.  Private to librfx.so.
#pragma once
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
#include "rfx_loop_core.h"

namespace rfx {
int fail(int code, const std::string& msg);  // sets rfx_last_error's text (one thread-local string, rfx_api_plan.hip); returns code
#define RFX_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return fail(RFX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

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
// device that owns a caller buffer, for the entry points that take no plan (rfx_api_codec.hip); RFX_ERR_INVALID: not a device pointer
int device_of(const void* d_ptr, int* device);
// the argument checks the two clip-gather entries share (rfx_api_codec.hip)
int check_pcm_clips(const char* who, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts, int N, int Lw,
                    int out_channels);
}  // namespace rfx

#ifndef RFX_FWD_RUN_SKEW
#define RFX_FWD_RUN_SKEW 170  // per mille: 74 / 54 frames instead of 64 / 64; -4.3 % on the forward kernel (profiles/r06_forward_skew.txt)
#endif

struct rfx_plan {
  rfx_params p;
  int device;
  std::vector<void*> owned;  // every device allocation of plan creation (upload); the d_* fields below are views of them
  int num_cus;
  int n_stft;
  int gl_wgs_per_cu = 1;    // resident Griffin-Lim workgroups per CU on this device (occupancy query at creation)
  rfx::ImelVariant imel_variant = rfx::kImelVariantBest;  // debugging override read once at creation
  unsigned long long* timing = nullptr;  // RFX_TIMING builds only
  rfx::cf* d_tw1 = nullptr;      // [21][441]
  rfx::cf* d_tw2 = nullptr;      // [21][21]
  float* d_win = nullptr;   // [4410]
  float* d_melfb_slots = nullptr;  // [kFrameStride][n_mels]: filterbank rows permuted to slot order
  float* d_melfb = nullptr;        // [n_stft][n_mels] as given
  int16_t* d_bin_bands = nullptr;  // [2 n_stft] first / last band of each bin, -1: none (bin_bands; rfx_hold_bins_from_bands)
  int* d_kblocks = nullptr;        // non-zero 32-position K blocks of d_melfb_slots
  int n_kblocks = 0;
  int melfb_cols = 0;              // columns of d_melfb_slots (n_mels rounded up to 128)
  // banded view of the filterbank for InverseMelScale (valid when imel_ok)
  bool imel_ok = false;
  std::string imel_why;
  rfx::ImelTables imel{};
  void* d_imel_blob = nullptr;
  // closed-form InverseMelScale (rfx_imel_lstsq.hip): the factor tables of fb^T fb, uploaded when the bank admits them
  bool lstsq_ok = false;
  std::string lstsq_why;
  rfx::LsqTables lstsq{};
  rfx::LsqCollectTables lstsq_collect{};  // its backward's collect (rfx_inverse_mel_lstsq_backward), uploaded with them
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
  rfx::GenGeom gg{};
  rfx::GenTables gt{};
  void* d_gen_tables = nullptr;
  int* d_gen_rev = nullptr;
  rfx::cf* d_gen_tw = nullptr;
  int frame_stride = rfx::kFrameStride;
  // chirp-z engine (rfx_czt.hip) on top of a generic plan: FFT lengths with a prime factor above 13, opt-in (RFX_ENGINE_CHIRPZ)
  bool czt = false;
  rfx::cf* d_czt_c = nullptr;  // [gg.nc] chirp
  rfx::cf* d_czt_h = nullptr;  // [gen_ibuf_elems(gg.np, gg.pad_shift)] H in the buffer's LDS layout
  // row-family Griffin-Lim (rfx_fam.hip) on top of a generic plan: n_fft = 40 h, win_length = 10 h
  bool fam_ok = false;
  rfx::FamGeom fam{};
  rfx::cf* d_fam_tw = nullptr;      // [21][h] g(n')^k1, then [rb][ra-1] W_h^{i p}
  int* d_fam_binof = nullptr;  // [fsf] bin held by each position of the slot-ordered magnitudes (-1: padding)
  int fam_wgs_per_cu = 1;
  // backward of the forward path (rfx_mel_bwd.hip): the position tables of the magnitude slots the plan's MODE 0 frame launch reads
  // and of the spectrum its forward transform writes, and - with a filterbank - the per-bin adjoint table (rfx_mel_bwd_core.h)
  int* d_mb_pos_bin = nullptr;   // [mb_sstride]
  int* d_mb_xpos_bin = nullptr;  // [frame_stride]
  int* d_mb_s2x = nullptr;       // [mb_sstride] position of the spectrum each magnitude slot goes with
  int2* d_voc_table = nullptr;   // [frame_stride] the time stretch's position table (rfx_plan_core.h: VocoderTable::device)
  int mb_sstride = 0;
  int* d_mb_first = nullptr;     // [n_stft]
  int* d_mb_count = nullptr;     // [n_stft]
  float* d_mb_wt = nullptr;      // [n_stft][mb_width]
  int mb_width = 0;
};

// the engine's MODE 0 per-frame launch as the backward entries and the inverse spectrogram drive it (rfx_api_backward.hip): `rows`
// rows of T frames, frames = synthesis of S * angles0, mel_bwd_frame_pitch floats per frame
size_t mel_bwd_frame_pitch(const rfx_plan* plan);
int mel_bwd_frames(const rfx_plan* plan, const float* S, const rfx::cf* angles0, float* frames, int rows, int T, hipStream_t stream);

namespace rfx {
// the specialised engine's fold table out[p] = (2 / n_fft) / env[p + n_fft / 2], p < L (rfx_api_inverse.hip: out_scale_kernel)
hipError_t launch_gl_out_scale(const float* win, float* out, int T, int L, hipStream_t stream);
// torch.stft(center=True): the signal is reflect-padded by n_fft/2 on both sides, so a waveform of Lw samples gives
// 1 + (Lw + 2*(n_fft/2) - n_fft) / hop frames: 1 + Lw/hop for even n_fft, 1 + (Lw - 1)/hop for odd n_fft
inline int stft_frames(const rfx_plan* plan, int Lw) {
  return 1 + (Lw + 2 * (plan->p.n_fft / 2) - plan->p.n_fft) / plan->p.hop_length;
}
// the two forms of a forward call - plain: the row is reflect-padded, loop: the row is one period (rfx_loop_core.h) - in frames ...
inline int fwd_frames(const rfx_plan* plan, int Lw, bool loop) {
  return loop ? loop_samples_frames(plan->p.hop_length, plan->p.n_fft, Lw) : stft_frames(plan, Lw);
}
// ... and in the row lengths they take
inline bool fwd_length_ok(const rfx_plan* plan, int Lw, bool loop) {
  return loop ? loop_samples_valid(plan->p.hop_length, plan->p.n_fft, Lw) : Lw > plan->p.n_fft / 2;
}
// workgroups of a kernel that walks frames: one per frame, at most one per resident slot of the chip
inline int frame_blocks(long long slots, int B, int T) {
  const long long nframes = (long long)B * T;
  return (int)(nframes < slots ? nframes : slots);
}
// the refusal of a row length fwd_length_ok does not pass; RFX_OK for a legal one (rfx_api_forward.hip).  Plain: "reflect padding
// needs more than n_fft/2 = N samples".  Loop: the refusal names the nearest legal lengths.
int fwd_length_refusal(const rfx_plan* plan, int Lw, bool loop, const char* who);
// the zero-extension twin of the plan's forward frame launch (rfx_api_forward.hip): rows of L samples, T frames, the complex spectrum
int stft_zero_extended(const rfx_plan* plan, const float* d_rows, int B, int L, int T, void* d_spec_slots, void* stream);
inline long long fam_slot_count(const rfx_plan* plan) { return (long long)plan->num_cus * plan->fam_wgs_per_cu; }

// the spectral-peak start as the inverse entries use it (rfx_api_peak.hip): the refusal of a plan whose frame does not fit the LDS;
// the bytes a call with that start brings on top of its query (the angles, then the start's scratch); the three launches, reading
// magnitudes in `layout` (kHoldMaskSpec / kHoldMaskPlain / kHoldMaskTable) and writing angles as d_angles0_slots takes them
int peak_refusal(const rfx_plan* plan, const char* who);
size_t peak_scratch_bytes(const rfx_plan* plan, int B, int T);
size_t peak_angles_bytes(const rfx_plan* plan, int B, int T);
size_t peak_extra_bytes(const rfx_plan* plan, int B, int T);
int peak_start_run(const rfx_plan* plan, int layout, const float* d_mag, int B, int T, void* d_angles, void* d_scratch, hipStream_t stream);

// A workspace layout is a plain struct of byte offsets and `total`, returned by value from one function of (plan, shape): the
// rfx_*_workspace_bytes query answers its total, the driver takes every pointer from its fields.  A shape the query answers 0
// for gives the all-zero layout.  Carve deals the parts out: each starts on a 256-byte boundary.
// Rows walked in groups of whole rows that fill at most `bytes`: the rows of a group - at least one, at most B, at most `cap`.
inline int group_rows(size_t bytes, size_t row_bytes, int B, size_t cap = (size_t)-1) {
  size_t rows = bytes / row_bytes;
  rows = rows < 1 ? 1 : rows > cap ? cap : rows;
  return (int)(rows > (size_t)B ? (size_t)B : rows);
}
// the cap of the grouped drivers that hold whole spectrogram rows in their workspace (rfx_api_istft.hip, rfx_api_vocoder.hip, rfx_api_resample.hip)
constexpr size_t kIstftGroupBytes = (size_t)256 << 20;
constexpr size_t kIstftGroupRows = 65535;  // the folds carry the row in blockIdx.y
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += align_up(bytes, 256);
    return o;
  }
};
}  // namespace rfx
