// rfx_kernels.h - argument blocks and host launchers of the gfx950 kernels (internal to librfx.so)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "rfx_core.h"
#include "rfx_gen_core.h"
#include "rfx_fam_core.h"
#include "rfx_jpeg_dec_core.h"

namespace rfx {

// Per-row numeric range of Griffin-Lim (round 6): row r of a call analyses its signal times row_scale[2 r] (a power of two that
// brings the row's magnitudes to about 2^25) and projects with eps^2 = row_scale[2 r + 1] (rfx_core.h::gl_project); written by
// launch_range_scale (rfx_range.hip) from the data or the caller's magnitude_hint.  A null table means {1, 1e-32}.
struct GlArgs {
  const float* S;             // [B*T][kFrameStride] magnitudes, slot_pos_f order
  const float* row_scale;     // [B][2] or null
  const cf* angles0;          // optional injected initial angles, slot_pos_c order (MODE 0)
  const float* audio_in[2];   // x_k, the current estimate, [B][Lpad]: [0] every block, [1] what a run adds to the nine blocks it
                              // shares with the previous run of its row - written and read there only (rfx_gl.hip)
  const float* audio_prev[2]; // x_{k-1} (MODE 2)
  float* audio_out[2];        // x_{k+1}
  const float* out_scale;     // [L]  (2/N) / window-envelope  (torch.istft's division by sum w^2)
  const cf* tw1;              // [21][441]
  const cf* tw2;              // [21][21]
  const float* win;           // [4410]
  int B, T, L, Lpad;          // (the runs of a launch are its workgroups: gridDim.x)
  // Run lengths by dispatch order (round 5; gl_run_start below): the first `run_h` workgroups of a launch are the ones the
  // dispatcher places first - one per CU - and every later one joins a CU that already runs one.  The earlier workgroup's waves
  // are the older ones and win the CU's issue arbitration: measured (tools/probe_wgclock.py, 64 tiles) it finishes its 64 frames
  // in 656 us, its partner in 738 us, every launch, on every CU (spread 0.3 % / 0.1 %) - and for the last tenth of the launch
  // every CU runs one workgroup alone, at three quarters of its two-workgroup rate.  So the early workgroups get run_w1 / 1000
  // and the late ones run_w2 / 1000 of the mean run length, and the pair finishes together.
  int run_h, run_w1, run_w2;
  float mom;                  // momentum / (1 + momentum)
  unsigned long long seed;
  unsigned long long frame_base;  // rfx_call_options::row_base * T: frame (row, t) of this call draws its phases from key (seed, frame_base + row T + t)
  unsigned long long* timing;  // optional [nblocks][8] phase timers (RFX_TIMING builds only)
#ifdef RFX_WGCLOCK
  int launch;                  // diagnostic build: index of this launch inside one rfx_griffinlim call (tools/probe_wgclock.py)
#endif
};

// first frame of run b when the launch's N frames are cut into `runs` runs: the runs b < h weigh w1, the others w2 (integers,
// any common unit: round 6 passes q + 1 and q groups for N = q runs + r, h = r).  Exact integer arithmetic, the same on the host
// (checks) and in the kernel; N * (w1 h + w2 (runs - h)) must fit 63 bits (N < 2^27 groups and weights <= N do).
RFX_HD long long gl_run_start(long long b, long long runs, long long N, long long h, long long w1, long long w2) {
  const long long hb = b < h ? b : h, ht = runs < h ? runs : h;
  const long long Wb = w1 * hb + w2 * (b - hb), Wt = w1 * ht + w2 * (runs - ht);
  return N * Wb / Wt;
}
// Round 6: CANONICAL GROUPS.  torch.istft's overlap-add sums ten windowed frames per sample, and fp32 addition is not associative:
// where two runs share a hop block, the block is the sum of two partial chains instead of one - so until round 5 a clip's audio
// depended (in the last bit, then - Griffin-Lim amplifies it - in the last few PCM steps) on where the run boundaries of the
// launch fell, i.e. on the batch it was converted in.  Now every row (clip-channel) is cut into the same groups of kGlGroup frames
// whatever the batch is, EVERY group boundary splits the chains of the nine blocks across it (the run kernel flushes its partial
// sums there exactly as it does at the end of a run, the fold kernel of the per-frame form sums the two sides separately), and
// runs are whole groups.  A block's value is then s * chain(frames before the cut) + s * chain(frames from the cut on) for every
// partition and both forms: a clip's bits are a function of the clip, its seed and its row index alone.  (>= 10 frames per group:
// a block's ten frames span at most one cut.  16 divides the 64 frames per run of the headline shape, 64 tiles x 512 frames on 512
// resident workgroups; the price is the granularity - a launch lasts as long as its longest run, a whole number of groups.)
constexpr int kGlGroup = 16;
RFX_HD int gl_groups_per_row(int T) { return (T + kGlGroup - 1) / kGlGroup; }
// first frame (counted row after row) of run b of a launch over B rows of T frames: gl_run_start in units of groups
RFX_HD long long gl_run_start_frame(long long b, long long runs, int B, int T, long long h, long long w1, long long w2) {
  const long long ng = gl_groups_per_row(T);
  const long long u = gl_run_start(b, runs, (long long)B * ng, h, w1, w2);
  const long long row = u / ng;
  return row * T + (u - row * ng) * kGlGroup;
}

// is group u (counted row after row, as in gl_run_start_frame) the first one of a run?  Run b starts at group floor(N W_b / W_t),
// W_b increasing in b: the first run that starts at or behind u is the first one with N W_b >= u W_t, i.e. W_b >= ceil(u W_t / N)
RFX_HD bool gl_is_run_start(long long u, long long runs, long long N, long long h, long long w1, long long w2) {
  const long long ht = runs < h ? runs : h, Wt = w1 * ht + w2 * (runs - ht);
  const long long W = (u * Wt + N - 1) / N;
  const long long b = W <= w1 * ht ? (W + w1 - 1) / w1 : ht + (W - w1 * ht + w2 - 1) / w2;
  return b < runs && gl_run_start(b, runs, N, h, w1, w2) == u;
}

hipError_t launch_gl_iter(int mode, const GlArgs& g, int nblocks, hipStream_t stream);
// per-device set-up, called by rfx_plan_create with the plan's device current
hipError_t prepare_frame_kernels();  // dynamic-LDS attributes of the STFT and Griffin-Lim kernels
hipError_t prepare_gl_kernels();
int gl_blocks_per_cu();  // resident Griffin-Lim workgroups per CU on the current device (occupancy query)
// the two buffers of the last generation -> out (B, L); g and nblocks: the call's launch_gl_iter arguments (the partition)
hipError_t launch_gl_combine(const float* a0, const float* a1, float* out, const GlArgs& g, int nblocks, hipStream_t stream);

// small-batch (latency) form: one frame per unit of work, synthesis frames to a buffer, then a fold
struct GlFrameArgs {
  const float* S;           // [B*T][kFrameStride] magnitudes
  const cf* angles0;        // optional injected initial angles (MODE 0)
  const float* audio_in;    // x_k      [B][Lpad]
  const float* audio_prev;  // x_{k-1}  (MODE 2)
  float* frames;            // [B*T][4416] windowed synthesis frames
  const float* row_scale;   // [B][2] or null (see GlArgs)
  const cf* tw1;
  const cf* tw2;
  const float* win;
  int B, T, L, Lpad;
  float mom;
  unsigned long long seed;
  unsigned long long frame_base;  // as GlArgs::frame_base
};
hipError_t launch_gl_frame(int mode, const GlFrameArgs& g, int nblocks, hipStream_t stream);
// the same over the free-frame list of a held call (launch_hold_list): trip i of the grid-stride loop takes frame list[i], the trip
// count is list[B T].  Modes 1 and 2; the grid is the unlisted launch's (the host does not know the count)
hipError_t launch_gl_frame_list(int mode, const GlFrameArgs& g, const int* list, int nblocks, hipStream_t stream);
// addend (nullable; a masked call's constant audio, rows addend_stride apart): added to the folded sample before it is stored
hipError_t launch_gl_fold(const float* frames, const float* win, const float* scale, float* out, int B, int T, int L, size_t out_stride, hipStream_t stream,
                          const float* addend = nullptr, size_t addend_stride = 0);
size_t gl_frame_buffer_bytes(int B, int T);
// a loop call (rfx_loop_core.h; include/rfx.h: rfx_loop_call_options): the frame kernels of modes 1 / 2 with the analysis input read
// modulo the period g.L = hop T, the circular folds, and the hop-entry table out[r] = scale / env[r] they multiply by
hipError_t launch_gl_frame_loop(int mode, const GlFrameArgs& g, int nblocks, hipStream_t stream);
hipError_t launch_gl_loop_fold(const float* frames, const float* win, const float* renv, float* out, int B, int T, size_t out_stride, hipStream_t stream);
hipError_t launch_loop_renv(const float* win, float* out, int n_fft, int win_len, int hop, float scale, hipStream_t stream);

// layout conversion between the reference's (B, n_stft, T) tensors and slot-major frames
hipError_t launch_pack_mag(const float* lin_bft, float* S_slots, int B, int T, hipStream_t stream);
hipError_t launch_pack_angles(const cf* ang_bft, cf* slots, int B, int T, hipStream_t stream);
hipError_t launch_unpack_mag(const float* slots, float* out_bft, int B, int T, hipStream_t stream);
hipError_t launch_unpack_complex(const cf* slots, cf* out_bft, int B, int T, hipStream_t stream);

// forward STFT magnitude of arbitrary-length waveforms: wave [B][Lw] -> mag slots [B*T][kFrameStride]
struct StftArgs {
  const float* wave;   // [B][Lw]
  float* mag;          // [B*T][kFrameStride] |X| in slot_pos_f order (nullable)
  cf* spec;            // [B*T][kFrameStride] X in slot_pos_c order (nullable)
  const cf* tw1;
  const cf* tw2;
  const float* win;
  int B, T, Lw, frames_per_block;
};
hipError_t launch_stft(const StftArgs& a, hipStream_t stream);
// a loop forward call (include/rfx.h: rfx_stft_loop): Lw = hop T is the row's period, read modulo Lw (rfx_loop_core.h: loop_read_index)
hipError_t launch_stft_loop(const StftArgs& a, hipStream_t stream);
// the zero-extension twin (rfx_istft_backward): rows of Lw samples, T frames each, outside [0, Lw) an exact zero; spec only
hipError_t launch_stft_zero(const StftArgs& a, hipStream_t stream);

// fused forward path: waveform -> framed transform -> |X| -> banded mel projection, nothing but the (B, M, T) mel
// amplitudes leaves the chip.  Valid for banded filterbanks (every filter's support one contiguous run of bins).
struct StftMelArgs {
  const float* wave;     // [B][Lw]
  float* mel;            // [B][M][T] result (written by the transpose that follows the transform kernel)
  float* mel_tm;         // [B][T][Mpad] frame-major scratch the transform kernel writes
  const cf* tw1;
  const cf* tw2;
  const float* win;
  const float* band_wt;  // [band_rows][Mpad]: weight of filter m on its i-th bin (band_lo[m] + i), zero past its end
  const int* band_addr;  // [band_rows][Mpad]: LDS float index (2 * cube_at(k1, ka, 0) + kb) of that bin's primary slot
  const int* band_lo;    // [Mpad] first bin of filter m's band (padding filters: 0)
  const int* band_len;   // [Mpad] bins in filter m's band (padding filters: 0)
  int B, T, Lw, frames_per_block;
  int run_skew;          // stft_mel2_kernel: > 0 = the first-dispatched half of the grid walks runs this many frames longer, the other half as many shorter
  int M, Mpad;           // Mpad = M rounded up to 64
  int f_lo, f_hi;        // bins with a non-zero filterbank row: [f_lo, f_hi)
  // product form (stft_mel2_kernel; valid when slot_tab != nullptr): the thread that owns a bin's primary slot multiplies
  // |X| by the bin's two filterbank weights and scatters the products group by group; a filter is then two contiguous sums
  const void* slot_tab;  // [21][kQPad] x {w0, w1}: weights of the slot's bin on its first / second filter (zero for a slot that contributes nothing)
  const int* slot_at;    // [21][kQPad] LDS position of the slot's w0 product (the lane's dump position for a slot that contributes nothing)
  const int* pad_tab;    // [kMelPadsPerThread][kQPad] LDS positions of the zero padding this thread rewrites every frame (dump if none)
  const int* filt_seg;   // [2][Mpad]: rising segment, falling segment, each as (first float << 4) | number of 16-byte reads
  int prod_arr;          // floats between the w0 and the w1 product arrays (and between their dump floats)
  unsigned kb_mask;      // bit kb set when any thread's slot kb contributes
  // the same tables in the packed form the default-bank kernel reads (round 5; null when the bank needs kb outside kKbMaskLow or
  // more than kMelProdArr floats per array): LDS BYTE addresses as 16-bit halves, prod_arr == kMelProdArr
  const unsigned* pk_at;   // [5][kQPad]: word i = byte address of the w0 product of the thread's contributing slots 2 i (low half) and 2 i + 1 (high half), slots in increasing kb
  const unsigned* pk_pad;  // [kQPad][2]: the thread's kMelPadsPerThread zero-padding byte addresses, two per word
  const unsigned* pk_seg;  // [Mpad][2]: {rising, falling} segment of filter m, each (first float << 4) | number of 16-byte reads
  // image_util.image_from_spectrogram's maximum (image_util.py:41) taken on the fly (rfx_image_from_waveform): when not null,
  // max_keys[clip * chunks + chunk] receives the order-preserving key (rfx_codec.hip::max_key) of the largest mel amplitude the
  // workgroup walking run `chunk` of row `clip` forms (chunks = ceil(T / frames_per_block); every word written exactly once per
  // launch: no atomics, nothing to zero); the launcher then leaves out the transpose to (B, M, T)
  unsigned* max_keys;
  int max_group;           // (unused since round 6: an image's words are the C * chunks consecutive ones of its rows)
};
constexpr int kMelPadsPerThread = 4;
// the kb (of a thread's 21 slots) that can contribute, as a compile-time set: 0x1F001F (kb 0..4 and 16..20) covers every bank that
// ends at or below bin 4200 (the default 0-10 kHz bank: bins 1..4000), 0x1FFFFF any bank
constexpr unsigned kKbMaskLow = 0x1F001Fu, kKbMaskAll = 0x1FFFFFu;
constexpr int kMelProdArr = 8192;  // floats between the w0 and the w1 product arrays whenever the first one ends below it (a compile-time LDS offset for the packed form)
hipError_t launch_stft_mel(const StftMelArgs& a, hipStream_t stream);
hipError_t launch_stft_mel_loop(const StftMelArgs& a, hipStream_t stream);  // a loop forward call: Lw = hop T, the row read modulo Lw

// mel projection GEMM: out[b][m][t] = sum_p fbs[p][m] * mag[b*T+t][p]
struct MelArgs {
  const float* mag;     // [N][kFrameStride]
  const float* fbs;     // [kFrameStride][Mp] slot-ordered filterbank, columns zero-padded to Mp
  const int* kblocks;   // indices of the 32-position K blocks that contain a non-zero filterbank row
  int n_kblocks;
  float* out;           // [B][M][T]
  int M, Mp, N, T;      // N = B*T frames, Mp = M rounded up to the 128-row tile
};
hipError_t launch_mel_gemm(const MelArgs& a, hipStream_t stream);

// Per-wave register budgets (bins per thread) of the InverseMelScale fast path: wave w owns the short groups
// 64w .. 64w+63 and the long groups M-1-64w .. M-64-64w.  Sized exactly to the reference's default bank
// (0-10 kHz, 512 HTK filters over 8821 bins); plan creation falls back to the uniform kernel when a bank
// does not fit.
constexpr int kImelLoCap[4] = {2, 3, 5, 6};
constexpr int kImelHiCap[4] = {23, 16, 12, 9};
// a second set for banks whose edges sit elsewhere: mel_scale_type "slaney" (spectrogram_params.py:35; linear below 1 kHz,
// so its low groups are longer, and its top groups reach 26 bins)
constexpr int kImelLoCapWide[4] = {5, 3, 5, 6};
constexpr int kImelHiCapWide[4] = {26, 17, 12, 9};
// a third set (round 5) for the LINE-FORM group kernel (rfx_imel_groups.hip::imel_line_kernel_perwave): the long groups keep one register
// per bin (weights and momentum buffer are lines per group), so a thread can hold 62 of them - 512 filters up to the Nyquist
// frequency (group sizes 1.5 .. 61 bins), htk or slaney scale, or 256 / 384 filters over the default 0 - 10 kHz
constexpr int kImelLoCapLine[4] = {6, 5, 7, 11};
constexpr int kImelHiCapLine[4] = {62, 40, 26, 18};
// Wave kernel (round 4, rfx_imel_wave.hip::imel_wave_kernel): ONE wave per frame.  The 512 groups are dealt to the 64 lanes in eight
// chunks of 64 consecutive groups, even chunks in lane order and odd chunks reversed (group 64 c + lane / 64 c + 63 - lane), so a
// lane's bin count is within 4 % of the mean although group sizes grow 12-fold over the bank, and every group's neighbours sit
// in the adjacent lane (a DPP wave shift) or, at the chunk seams, in the lane itself.  Budget per chunk in register PAIRS:
constexpr int kImelWaveChunks = 8;
constexpr int kImelWavePairs[kImelWaveChunks] = {2, 2, 3, 3, 5, 6, 8, 12};
// leading pairs that EVERY lane of the chunk fills (plan creation checks n >= 2 full for each group); the pairs behind them carry a
// per-lane 0 / 1 mask for the slots a shorter group leaves empty
constexpr int kImelWaveFullPairs[kImelWaveChunks] = {0, 1, 1, 2, 3, 4, 5, 8};
RFX_HD int imel_wave_group(int chunk, int lane) { return (chunk & 1) ? 64 * chunk + 63 - lane : 64 * chunk + lane; }

// The SGD kernel families.  The values are public: rfx_plan_imel_kernel and rfx_bank_report::imel_kernel return them, and
// rfx_bank_report::fast_ok (include/rfx.h) is ImelTables::fast_ok.
enum ImelKernel : int {
  kImelKernelGeneral = 0,      // any banded filterbank: spec and weights in LDS (rfx_imel.hip)
  kImelKernelUniform = 1,      // group formulation, <8, 24> bins per thread in every wave (rfx_imel_groups.hip)
  kImelKernelPerWave = 2,      // group formulation, per-wave budgets kImelLoCap / kImelHiCap
  kImelKernelPerWaveWide = 3,  // ... kImelLoCapWide / kImelHiCapWide
  kImelKernelWave = 4,         // one wave per frame (rfx_imel_wave.hip); never a value of fast_ok: ImelTables::wave_ok admits it
  kImelKernelLine = 5,         // group formulation with the long groups as lines, kImelLoCapLine / kImelHiCapLine
};
// debugging override of the choice (-DRFX_ABLATION builds: RFX_IMEL_UNIFORM, RFX_IMEL_GENERAL)
enum ImelVariant : int {
  kImelVariantBest = 0,     // the best kernel the bank admits
  kImelVariantUniform = 1,  // the uniform group kernel where its budget holds the bank, else the general kernel
  kImelVariantGeneral = 2,  // the general kernel
};

// banded InverseMelScale SGD (torchaudio 0.13 semantics), one workgroup per frame
struct ImelTables {
  const float* csr_w;    // [nnz] filterbank weights, mel-major (column m = bins fs[m] .. fe[m]-1)
  const int* csr_ptr;    // [M+1]
  const int* band_lo;    // [M] first bin of mel m's band
  const int* bin_m0;     // [n_stft] first mel a bin feeds (-1: zero filterbank row)
  const float* bin_w0;   // [n_stft] weight into mel m0
  const float* bin_w1;   // [n_stft] weight into mel m0+1 (0 if none)
  const int* bin_pos;    // [n_stft] slot position of the bin's primary slot
  const int* bin_pos2;   // [n_stft] slot position of its duplicate slot, or -1
  const int* pos_bin;    // [frame stride] the inverse map: bin held by output position p, -1 for the padding (round 5: the wave kernel's staged epilogue)
  const int* grp_start;  // [M+1] first bin of group g (bins whose first filter is g), fast path only
  int f_lo, f_hi;        // bins with a non-zero filterbank row: [f_lo, f_hi)
  int nnz;
  int fast_ok;           // the group-kernel family the bank's groups admit, as an ImelKernel: kImelKernelPerWave where the default set
                         // fits, else ...PerWaveWide, else ...Line, else ...Uniform, else ...General (none)
  int unit_form;         // 1: in every long group (the top 256) a bin's two weights sum to one (to 1e-6) - the last group, whose second
                         // filter does not exist, carries w1 == 0: the per-wave kernels compute the gradient as d1 + (d0 - d1) w0
  const float* lin;      // [4][M] a0 | s0 | a1 | s1: within group g the weights are w0 = a0 + s0 i, w1 = a1 + s1 i for the group's i-th bin
                         // (triangular filters on a uniform bin grid; fitted and checked to 1e-6 per bin at plan creation)
  int line_from;         // groups below this index are NOT lines (group 0 of a bank whose first filter rises over several bins): the
                         // line-form group kernel keeps such a long group in its thread's table-form slot
  int wave_ok;           // 1: imel_wave_kernel serves this bank (M == 512, the chunk budgets fit, the weights are linear per group)
};
struct ImelArgs {
  ImelTables tb;
  const float* mel;      // [B][M][T]
  const float* spec0;    // optional [B][T][n_stft] injected init (reference layout), else seeded RNG
  float* out_slots;      // [B*T][kFrameStride]
  const float* clip_scale;  // [nclips][2] {2^-e, 2^e}: the power of two the clip's SGD state is held in (launch_range_scale), null = 2^-60
  float sc, un;             // the frame's pair, set inside the kernels (imel_set_scale)
  float* loss_hist;      // [B*T][max_iter] per-frame sum_m diff^2 before each step
  const int* it_limit;   // optional [nclips] number of steps to run (fix-up pass), NULL = max_iter
  int B, M, T, C;        // C = channels per clip (the loss mean couples them)
  int n_stft;            // linear bins per frame (8821 on the specialised geometry)
  int out_stride;        // elements between output frames (kFrameStride, or the generic path's fs)
  int plain;             // 1: output frames are plain bin-ordered rows (generic path), 0: slot layout
  int max_iter;
  float lr, momentum;
  unsigned long long seed;
  unsigned long long frame_base;  // rfx_call_options::row_base * T: frame f of this call draws its start from key (seed, frame_base + f)
};
hipError_t launch_imel(const ImelArgs& a, ImelVariant variant, hipStream_t stream);
// the families' own launchers (rfx_imel_groups.hip: every group kernel; rfx_imel_wave.hip), called by launch_imel
hipError_t launch_imel_groups(const ImelArgs& a, ImelKernel kernel, hipStream_t stream);
hipError_t launch_imel_wave(const ImelArgs& a, hipStream_t stream);
// the kernel launch_imel runs (every one but the general kernel leaves through imel_emit_frame: its output order is the pos_bin table)
ImelKernel imel_kernel_choice(const ImelTables& tb, int M, int max_iter, ImelVariant variant);
// Numeric range (round 6, include/rfx.h): one workgroup per group of `count` contiguous floats of x (a clip's mel amplitudes, or a
// row's magnitudes) takes max |x| - or `hint` when > 0, without reading x - and writes the powers of two the kernels work in:
//   imel_scale[g] = {2^-e, 2^e}, e = max(k + 35, 30) for max in [2^(k-1), 2^k)     (nullable)
//   gl_scale[g * rows + r] = {2^-j, eps^2}, j = ks - 26, ks = k, or max(k, 0) + 1 when `mel_units` (the SGD's untouched bins keep
//   their U[0,1) start: a row's magnitudes reach 1 whatever the mel amplitudes are)                         (nullable)
// the arithmetic of it, shared by the kernel and rfx_debug_range_exponents (tests without a GPU): k with mx in [2^(k-1), 2^k)
// (0 for mx == 0 or NaN, 129 for +Inf) -> the SGD exponent e and the Griffin-Lim exponent j
RFX_HD void range_exponents(int k, int mel_units, int* e, int* j) {
  int ee = k + 35;
  *e = ee < 30 ? 30 : (ee > 126 ? 126 : ee);
  const int ks = mel_units ? (k > 0 ? k : 0) + 1 : k;
  int jj = ks - 26;
  *j = jj < -100 ? -100 : (jj > 100 ? 100 : jj);
}
// keys: [groups] scratch words
hipError_t launch_range_scale(const float* x, size_t count, int groups, float hint, unsigned* keys, float* imel_scale, float* gl_scale, int rows,
                              int mel_units, hipStream_t stream);
// scans loss_hist for the early-stop condition; it_stop[clip] = steps the reference would have run
hipError_t launch_imel_scan(const float* loss_hist, int* it_stop, int* any_early, int nclips, int C, int T, int max_iter,
                            float tol_loss, float tol_change, hipStream_t stream);

// ---- generic-geometry path (rfx_generic.hip): any n_fft / win_length / hop_length, plain [B*T][fs] frame arrays
struct GenTables {
  const cf* lo;      // [128]   exp(-2 pi i t / nc)
  const cf* hi;      // [nhi]   exp(-2 pi i 128 t / nc)
  const cf* lo2;     // [128]   exp(-2 pi i t / n_fft)
  const cf* hi2;     // [nhi2]  exp(-2 pi i 128 t / n_fft)
  const float* win;  // [win]
  const int* rev;    // [nc] LDS position (padding included) of element k after the in-place forward passes (digit reversal)
  const cf* tw;      // exact per-pass twiddles W_L^{i p} (gen_tw_table_offset / gen_ip_compute), all passes back to back
};
struct GenStftArgs {
  GenGeom g;
  GenTables tb;
  const float* wave;   // [B][wave_stride], Lw valid samples each
  size_t wave_stride;
  float* mag;          // mode 0: [B*T][fs] |X|
  cf* spec;            // mode 1: [B*T][fs] X
  int B, T, Lw;
};
// one Griffin-Lim iteration of the generic engine, frame by frame: analysis of x_k - m x_{k-1}, projection, synthesis
struct GenGlArgs {
  GenGeom g;
  GenTables tb;
  const float* S;        // [B*T][fs] magnitudes
  const cf* angles0;     // mode 0: optional injected initial angles [B*T][fs] (drawn from `seed` when null)
  const float* x_cur;    // modes 1, 2: the signal to analyse, d = x_k - m x_{k-1} (x_0 in the first iteration), formed by the fold of
                         // the previous iteration (launch_gen_fold's `dout`): [B][audio_stride], L valid samples per clip
  const float* x_prev;   // unused since round 4 (the kernel used to form d itself from x_k and x_{k-1})
  size_t audio_stride;
  float* frames;         // [B*T][win] windowed, scaled synthesis frames (gen_fold_kernel overlap-adds them)
  const float* row_scale;  // [B][2] or null (see GlArgs): the fold applies the factor to d, the kernel takes eps^2 from it
  float mom;             // momentum / (1 + momentum)
  unsigned long long seed;
  unsigned long long frame_base;  // as GlArgs::frame_base
  int B, T, L;
};
hipError_t prepare_generic_kernels(const GenGeom& g);
size_t gen_lds_bytes(const GenGeom& g);
hipError_t launch_gen_stft(int mode, const GenStftArgs& a, int num_cus, hipStream_t stream);  // mode 0 mag, 1 spec
hipError_t launch_gen_stft_loop(int mode, const GenStftArgs& a, int num_cus, hipStream_t stream);  // a loop forward call: Lw = hop T, the row read modulo Lw
hipError_t launch_gen_stft_zero(const GenStftArgs& a, int num_cus, hipStream_t stream);  // the zero-extension twin: a.spec from zero-extended rows of a.Lw samples, a.T frames
hipError_t launch_gen_gl(int mode, const GenGlArgs& a, int num_cus, hipStream_t stream);      // mode 0 init, 1 first iteration, 2 iteration
hipError_t launch_gen_gl_list(const GenGlArgs& a, const int* list, int num_cus, hipStream_t stream);  // mode 1 over a free-frame list (launch_gl_frame_list)
hipError_t launch_gen_env(const float* win, float* env, const GenGeom& g, int T, int L, hipStream_t stream);  // env[p] = sum_t w[j]^2, once per call
hipError_t launch_gen_fold(const float* frames, const float* env, float* out, const GenGeom& g, int B, int T, int L, size_t out_stride,
                           hipStream_t stream, const float* prev = nullptr, float* dout = nullptr, float mom = 0.f,
                           const float* row_scale = nullptr,  // L output samples per clip; dout = (x - mom prev) * row_scale[2 b]
                           const float* addend = nullptr, size_t addend_stride = 0);  // masked call: x += addend[b][p] before out and dout
// loop call: mode 1 with the input read modulo a.L = hop T, and the circular fold (x, and d as launch_gen_fold forms it)
hipError_t launch_gen_gl_loop(const GenGlArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_gen_loop_fold(const float* frames, const float* renv, float* out, const GenGeom& g, int B, int T, size_t out_stride, hipStream_t stream,
                                const float* prev, float* dout, float mom, const float* row_scale);
hipError_t launch_gen_pack(const void* bft, void* frames, bool complex_, int B, int F, int T, int fs, hipStream_t stream);
hipError_t launch_gen_unpack(const void* frames, void* bft, bool complex_, int B, int F, int T, int fs, hipStream_t stream);
hipError_t launch_gen_mel(const float* mag, float* mel_tm, const float* band_wt, const int* band_lo, const int* band_len, long long nframes,
                          int fs, int M, int Mpad, int f_lo, int f_hi, hipStream_t stream);  // [f_lo, f_hi): bins with a non-zero filterbank row
// ---- chirp-z engine (rfx_czt.hip, rfx_czt_core.h): the generic engine's frame kernels for FFT lengths with a prime factor above 13.
// Same argument blocks (g.np = the convolution length, tb.lo / hi / tw / g.radix of that length), plus the chirp [g.nc] and H [LDS layout
// of the g.np-point buffer]; fold, envelope, pack, unpack and mel are the generic engine's
hipError_t prepare_czt_kernels(const GenGeom& g);
hipError_t launch_czt_stft(int mode, const GenStftArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream);  // mode 0 mag, 1 spec
hipError_t launch_czt_gl(int mode, const GenGlArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream);      // modes as launch_gen_gl
// mode 1 over a free-frame list (launch_gl_frame_list); a translation unit of their own (rfx_czt_list.hip)
hipError_t prepare_czt_list_kernels(const GenGeom& g);
hipError_t launch_czt_gl_list(const GenGlArgs& a, const int* list, const cf* chirp, const cf* h, int num_cus, hipStream_t stream);
// the forward kernels of a loop call (Lw = hop T, the row read modulo Lw); a translation unit of their own as well (rfx_czt_loop.hip)
hipError_t prepare_czt_loop_kernels(const GenGeom& g);
hipError_t launch_czt_stft_loop(int mode, const GenStftArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream);  // mode 0 mag, 1 spec
// the forward kernels of the zero-extended analysis (rfx_istft_backward); a translation unit of their own too (rfx_czt_zero.hip)
hipError_t prepare_czt_zero_kernels(const GenGeom& g);
hipError_t launch_czt_stft_zero(int mode, const GenStftArgs& a, const cf* chirp, const cf* h, int num_cus, hipStream_t stream);  // mode 1 spec
hipError_t launch_mel_transpose(const float* mel_tm, float* mel, int B, int T, int M, int Mpad, hipStream_t stream);

// ---- row-family Griffin-Lim (rfx_fam.hip): n_fft = 40 h, win_length = 10 h; frames are folded by launch_gen_fold
struct FamGlArgs {
  FamGeom g;
  const float* S;        // [B*T][g.fsf] magnitudes in slot order (launch_fam_repack)
  const cf* angles0;     // mode 0: optional injected initial angles in the plan's PLAIN layout [B*T][fs_plain] (drawn from `seed` when null)
  int fs_plain;
  const float* x_cur;    // modes 1, 2: x_k      [B][audio_stride], L valid samples per clip
  const float* x_prev;   // mode 2:     x_{k-1}
  size_t audio_stride;
  float* frames;         // [B*T][fpitch] windowed, scaled synthesis frames, window sample j at fshift + j (GenGeom::fpitch / fshift)
  const float* row_scale;  // [B][2] or null (see GlArgs)
  int fpitch, fshift;
  const cf* tw1;         // [21][h]      g(n')^k1
  const cf* twa;         // [ra-1][rb]   W_h^{i p} at [p - 1][i]: the lanes of a wave (consecutive i) read consecutive entries (round 5; [rb][ra-1] until
                         // then: 29 cache lines per wave-wide load, which cost the 48 kHz kernels a fifth of their time)
  const float* win;      // [win]
  float mom;             // momentum / (1 + momentum)
  unsigned long long seed;
  unsigned long long frame_base;  // as GlArgs::frame_base
  int B, T, L;
};
// forward STFT of the family geometries into the plan's plain layout (mode 0: |X| floats, mode 1: X complex), or (mode 2) fused
// with the banded mel projection: |X| never leaves the chip, the frame-major mel amplitudes do (spectrogram_converter.py:165-185)
struct FamFwdArgs {
  FamGeom g;
  const float* wave;     // [B][wave_stride], Lw valid samples each
  size_t wave_stride;
  int Lw;
  float* mag;            // mode 0: [B*T][fs_plain]
  cf* spec;              // mode 1: [B*T][fs_plain]
  int fs_plain;
  const cf* tw1;
  const cf* twa;
  const float* win;
  int B, T;
  // mode 2: the band tables of gen_mel_kernel (weights transposed [rows][Mpad], rows a multiple of eight, zero past a filter's end)
  float* mel_tm;         // [B*T][Mpad] frame-major mel amplitudes (mel_transpose_kernel turns them into (B, M, T))
  const float* band_wt;
  const int* band_lo;
  const int* band_len;
  int M, Mpad;
};
hipError_t launch_fam_fwd(int mode, const FamFwdArgs& a, int nblocks, hipStream_t stream);
hipError_t launch_fam_fwd_loop(int mode, const FamFwdArgs& a, int nblocks, hipStream_t stream);  // a loop forward call: Lw = hop T, the row read modulo Lw
hipError_t launch_fam_fwd_zero(const FamFwdArgs& a, int nblocks, hipStream_t stream);  // the zero-extension twin, mode 1: a.spec from zero-extended rows of a.Lw samples
hipError_t prepare_fam_kernels(const FamGeom& g);
size_t fam_lds_bytes(const FamGeom& g);         // dynamic: the cube
size_t fam_static_lds_bytes(const FamGeom& g);  // static: the pass-A twiddles where they fit
int fam_blocks_per_cu(const FamGeom& g);
bool fam_row_stride_even(const FamGeom& g);     // the kernels use 16-byte LDS accesses in pass B: rows must start 16-byte aligned
hipError_t launch_fam_gl(int mode, const FamGlArgs& a, int nblocks, hipStream_t stream);  // mode 0 init, 1 first iteration, 2 iteration
hipError_t launch_fam_gl_list(const FamGlArgs& a, const int* list, int nblocks, hipStream_t stream);  // modes 1 / 2 over a free-frame list (launch_gl_frame_list)
hipError_t launch_fam_gl_loop(const FamGlArgs& a, int nblocks, hipStream_t stream);  // mode 1 of a loop call (launch_gl_frame_loop)
hipError_t launch_fam_repack(const float* plain, float* slots, const int* bin_of, long long nframes, int fs_plain, int fsf, int n_stft,
                             hipStream_t stream);

// image / PCM codecs
hipError_t launch_image_decode(const uint8_t* img, const float* lut, float* out, int N, int H, int W, int C, hipStream_t s);
// order-preserving integer key of a float for atomicMax: positive NaN is the largest key (np.max's NaN propagation comes for free),
// key 0 is below every value
__device__ __forceinline__ unsigned max_key(float v) {
  unsigned b = __float_as_uint(v);
  if (v != v) b = 0x7FC00000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
hipError_t launch_clip_max(const float* x, float* out, int nclips, size_t count, bool abs_value, hipStream_t s);
hipError_t launch_image_encode(const float* mel, const float* clip_max, const float* thr, uint8_t* img, int N, int M, int T,
                               int C, hipStream_t s);
// encode straight from the forward kernels' frame-major mel amplitudes [N*C][T][Mpad] (rfx_image_from_waveform): the transpose to the
// image's (mel, time) order happens in LDS; the maximum comes as a key (max_keys, from the forward kernel) or as a float (clip_max)
hipError_t launch_image_encode_tm(const float* mel_tm, const unsigned* max_keys, int keys_per_image, const float* clip_max_in, const float* thr,
                                  uint8_t* img, float* clip_max_out, int N, int M, int Mpad, int T, int C, hipStream_t s);
hipError_t launch_pcm16(const float* wave, const float* clip_peak, int16_t* pcm, int N, int L, int C, int normalize, hipStream_t s);
// int16 post-processing (rfx_pcm.hip, arithmetic in rfx_pcm_core.h): apply_filters(compression=False) per clip of an (N, L, C)
// batch (in place when out == in), and the stitch of N clips of L frames from the host planner's pieces (PcmPiece[n_pieces])
size_t pcm_filters_workspace_bytes(int N, int L, int C);
hipError_t launch_pcm_filters(const int16_t* in, int N, int L, int C, const double* gain_by_rms, const double* boost_by_peak,
                              int16_t* out, void* workspace, hipStream_t s);
hipError_t launch_pcm_stitch(const int16_t* pcm, int64_t L, int C, const void* pieces, int n_pieces, int64_t frames, int16_t* out,
                             hipStream_t s);
// the filters' statistics pass on its own: partials[clip * pcm_splits(count) + part] over clips of `count` samples
struct PcmPartial {  // one statistics workgroup's share of a clip
  int64_t sumsq;
  int32_t xmax, xmin;
};
int pcm_splits(int64_t count);
hipError_t launch_pcm_stats(const int16_t* in, int N, int64_t count, PcmPartial* partials, hipStream_t s);
// apply_filters(compression=True) up to the compressor's output (rfx_compress.hip, arithmetic in rfx_compress_core.h):
// normalize, gain to -10 dBFS, window rms, the attenuation recurrence (form 0 sequential, 1 chunked), and the apply with its
// flags, into the workspace's x3 (the input is not written); the caller patches the flagged samples and runs
// launch_pcm_filters from x3 to its output.  Layout of the workspace: cmp_workspace_layout.
struct CmpLayout {
  size_t partials, factors, traj, rms, x3, count, filters, total;  // byte offsets, and the size
};
CmpLayout cmp_workspace_layout(int N, int L, int C);
hipError_t launch_cmp_compress(const int16_t* in, int N, int L, int C, const double* boost_by_peak, const double* gain10_by_rms,
                               const uint8_t* above, const double* max_att, const double* inc, const double* dec, int look_frames,
                               int form, int chunk_frames, double margin, void* flags, int64_t flag_capacity, int32_t* rounds,
                               void* workspace, hipStream_t s);
hipError_t launch_cmp_scatter(const void* flags, int64_t n, int16_t* out, hipStream_t s);

// PIL.Image.resize of (N, H, W, 3) uint8 tiles (rfx_resize.hip, arithmetic in rfx_resize_core.h): the horizontal pass when
// OW != W, into the workspace when the vertical pass follows (OH != H), then the vertical pass; a copy when neither size changes.
size_t resize_workspace_bytes(int N, int H, int W, int OH, int OW);
hipError_t launch_resize(const uint8_t* in, int N, int H, int W, int OH, int OW, const int32_t* bounds_x, const int32_t* kk_x,
                         int ksize_x, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y, uint8_t* out, void* workspace,
                         hipStream_t s);

// baseline JPEG scans of (N, H, W, 3) uint8 tiles (rfx_jpeg.hip, arithmetic in rfx_jpeg_core.h): image n's entropy-coded scan
// and EOI at scan + n * capacity, its length in scan_bytes[n].  qtables: (2, 64) uint16, natural order.  The caller has checked
// the sizes (1 .. 65535, N * blocks and N * chunks within one launch).
struct JpgLayout {
  size_t coef, acbits, bitoff, bit_total, unstuffed, ffpre, total;  // byte offsets, and the size
  size_t unstuffed_per_image, chunks_per_image;                    // bytes (a multiple of 16) and 16-byte chunks of one image's stream
};
JpgLayout jpeg_workspace_layout(int N, int H, int W);
hipError_t launch_jpeg_encode(const uint8_t* rgb, int N, int H, int W, const uint16_t* qtables, uint8_t* scan, size_t capacity,
                              int32_t* scan_bytes, void* workspace, hipStream_t s);

// the zlib stream of a PNG's IDAT chunk for (N, H, W, 3) uint8 tiles (rfx_png.hip, the stream in rfx_png_core.h): tile n's stream
// at stream + n * capacity, its length in stream_bytes[n], the CRC-32 of b"IDAT" + stream in crc[n], and in channels[n] what it was
// written with: 3 (RGB), 1 (grey) or 0 (mode 1 met a colour tile: no stream).  mode: 0 RGB, 1 grey, 2 grey where R = G = B.  The
// caller has checked the sizes (1 .. 65535, capacity within int32, N * H and N * pieces within one launch).
struct PngLayout {
  size_t colour, row_a, row_b, hist, table, hdr, hdr_bits, block_bits, filt, words, total;  // byte offsets, and the size
  size_t words_per_tile, filt_per_tile;  // 32-bit words of one tile's stream (a multiple of 64), bytes of its filtered rows
};
PngLayout png_workspace_layout(int N, int H, int W);
hipError_t launch_png_encode(const uint8_t* rgb, int N, int H, int W, int mode, uint8_t* stream, size_t capacity, int32_t* stream_bytes,
                             uint32_t* crc, int32_t* channels, void* workspace, hipStream_t s);

// baseline JPEG scans to (N, H, W, 3) uint8 tiles (rfx_jpeg_dec.hip, arithmetic in rfx_jpeg_dec_core.h): image n's entropy-coded
// bytes are scans[offsets[n] .. offsets[n + 1]) (offsets: N + 1 int64 in device memory; scans 16-byte aligned), its tables
// qtables[n] (2, 64) uint16 in natural order and huff[n] (4, 272) uint8; status[n] receives 0 or a kJpd* code.  The caller has
// checked the sizes (1 .. 65535, N * blocks and N * H * W within one launch, every scan at most kJpdMaxScanBytes);
// max_scan_bytes is the longest scan, total_scan_bytes = offsets[N] - offsets[0].
// JpdLayout and jpeg_decode_workspace_layout: rfx_jpeg_dec_core.h (host inline, shared with the host emulator).
hipError_t launch_jpeg_decode(const uint8_t* scans, const int64_t* offsets, int64_t max_scan_bytes, size_t total_scan_bytes, int N, int H, int W,
                              const uint16_t* qtables, const uint8_t* huff, uint8_t* rgb, int32_t* status, void* workspace, hipStream_t s);

// zlib streams of PNG tiles to (N, H, W, 3) uint8 tiles (rfx_png_dec.hip, the decoder in rfx_png_dec_core.h): image n's
// concatenated IDAT payloads are streams[offsets[n] .. offsets[n + 1]) (offsets: N + 1 int64 in device memory; streams 16-byte
// aligned); colour type 0, 2, 3 or 6, for 3 with palettes (N, 256, 3) and palette_entries (N); status[n] receives 0 or a kPngd*
// code.  The caller has checked the sizes (1 .. 65535, every stream at most kPngdMaxStreamBytes).  workspace: 256-byte aligned,
// png_decode_workspace_layout (rfx_png_dec_core.h, host inline, shared with the host emulator).
hipError_t launch_png_decode(const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int color_type, const uint8_t* palettes,
                             const int32_t* palette_entries, uint8_t* rgb, int32_t* status, void* workspace, hipStream_t s);

// int16 front end of the encode (rfx_pcm_in.hip, arithmetic in rfx_pcm_in_core.h).  launch_pcm_ratecv: the (L, C_in) recording
// `in`, mixed to C_out channels, then audioop.ratecv to the K = ratecv_out_frames(L, ...) frames of `out`; both pointers are
// frame-aligned.  launch_pcm_clips: N clips of Lw frames at the frame offsets `starts` (device memory) of `pcm`, mixed to C_out
// channels after the slice -> wave (N * C_out, Lw) float32.  Channel counts are 1 or 2; the callers have checked every bound.
hipError_t launch_pcm_ratecv(const int16_t* in, int C_in, int64_t in_rate, int C_out, int64_t out_rate, int16_t* out, int64_t K,
                             hipStream_t s);
hipError_t launch_pcm_clips(const int16_t* pcm, int C_in, const int64_t* starts, int N, int64_t Lw, int C_out, float* wave, hipStream_t s);

// the per-row spectral sums (rfx_quality.hip, arithmetic and reduction shape in rfx_quality_core.h): `rows` rows of T frames of `a`
// and `m`, fs floats per frame (a multiple of four; both tensors 16-byte aligned) -> sums[nsums r ..]: sum (a - m)^2, sum m^2 and,
// with nsums == 3, sum | ln max(a, floor) - ln max(m, floor) | (floor == 0: no logarithm, 0), in double over the n_stft bins of every
// frame, each once (plain: bin-ordered frames, else the specialised slot layout).  nsums is 2 (floor not read) or 3; the first two
// sums are the same bits for either.  Two launches: one workgroup per four frames into `partials` (qual_partials_bytes), then one
// per row.  rows * ceil(T / 4) < 2^31.
size_t qual_partials_bytes(int rows, int T, int nsums);
hipError_t launch_spectral_sums(const float* a, const float* m, int rows, int T, int fs, int n_stft, bool plain, int nsums, float floor, void* partials,
                                double* sums, hipStream_t s);

// guide staging of a guided Griffin-Lim call (rfx_guide.hip, arithmetic in rfx_guide_core.h): row r of guide (B rows of
// guide_samples floats, `stride` elements apart), cut or zero-padded to L samples and times the power of two that brings its peak
// to 2^15, divided by row_scale[2 r] when a table is given (the specialised engine's kernels multiply by it), into dst[r][Lpad];
// zero[r][Lpad] (nullable) is zeroed.  peaks: scratch of B * guide_chunks(Lpad) floats (rfx_guide_core.h; fewer than B * Lpad).
// Lpad a multiple of 64, dst and zero 16-byte aligned; the guide needs float alignment only.
hipError_t launch_guide_stage(const float* guide, long long stride, int guide_samples, int B, int L, int Lpad, const float* row_scale,
                              float* peaks, float* dst, float* zero, hipStream_t stream);
// the guided decode's backward (include/rfx.h: rfx_griffinlim_guided_backward).  The same fit and range, no kernel factor, into rows
// of exactly L floats (dst[r][L], any float alignment: what rfx_stft and rfx_stft_loop read); peaks: B * guide_chunks(L) floats
hipError_t launch_guide_stage_rows(const float* guide, long long stride, int guide_samples, int B, int L, float* peaks, float* dst, hipStream_t stream);
// ... and the guide projection (rfx_guide_bwd.hip; guide_project of rfx_guide_core.h): G and A are B * T frames of xstride complex
// slots (rfx_pack_complex's layout), out B * T frames of sstride floats (rfx_pack_magnitudes' layout).  xpos_bin [xstride]: the bin
// a complex position holds, -1 for padding; s2x [sstride]: the complex position a magnitude slot goes with, -1 for padding
struct GuideProjectArgs {
  const cf* G;
  const cf* A;
  float* out;
  const int* xpos_bin;
  const int* s2x;
  int B, T, xstride, sstride;
};
hipError_t launch_guide_project(const GuideProjectArgs& a, hipStream_t stream);
// the free-frame list of a held call (rfx_guide_core.h): hold = (B, 2) {head, tail} per row, any values (clamped); list =
// hold_list_words(B, T) ints: the indices row T + t of the frames that are not held, increasing, their count at list[B T], the
// compaction's chunk offsets behind it.  Three launches, no atomics, nothing read back.
hipError_t launch_hold_list(const int32_t* hold, int B, int T, int* list, hipStream_t stream);
// a masked Griffin-Lim call (rfx_holdmask.hip, arithmetic in rfx_holdmask_core.h): X = S where the position's bin is held
// (want_held) or free, 0 elsewhere and in the padding.  layout: kHoldMaskSpec / kHoldMaskPlain / kHoldMaskTable (bin_of: the table
// of the last, [stride]); S and X: [B*T][stride]; mask: (B, T, ceil(n_stft / 32)) uint32
hipError_t launch_holdmask_split(int layout, const float* S, float* X, const uint32_t* mask, const int* bin_of, int B, int T, int stride,
                                 int n_stft, bool want_held, hipStream_t stream);
// bands (B, M, T) uint8, nonzero = held -> the bin mask; lo / hi [n_stft]: first and last band of each bin (-1: none)
hipError_t launch_holdmask_bands(const uint8_t* bands, const int16_t* lo, const int16_t* hi, uint32_t* out, int B, int M, int T, int n_stft,
                                 hipStream_t stream);
// the spectral-peak start (rfx_peak.hip, arithmetic in rfx_peak_core.h): S [B*T][stride_in] magnitudes in `layout` (kHoldMaskSpec /
// kHoldMaskPlain / kHoldMaskTable with bin_of) -> angles [B*T][stride_out] in the layout injected angles take (slot_pos_c order for
// kHoldMaskSpec, plain otherwise).  own [B*T][n_stft] uint16 and val [B*T][n_stft] double are scratch.  The LDS a frame needs:
size_t peak_owner_lds_bytes(int n_stft);
size_t peak_chain_lds_bytes(int n_stft);
hipError_t launch_peak_start(int layout, const float* S, const int* bin_of, int B, int T, int stride_in, int n_stft, int hop, int n_fft,
                             uint16_t* own, double* val, cf* angles, int stride_out, hipStream_t stream);

// closed-form InverseMelScale (rfx_imel_lstsq.hip, arithmetic in rfx_imel_lstsq_core.h).  The plan's tables: the float32
// L D L^T factors of fb^T fb - nl[m] = -L[m + 1][m] (nl[M - 1] = 0), inv_d[m] = 1 / D[m] - and, for every position of an output
// frame, its bin's first filter and two weights (a position that holds no bin, or a bin no filter reaches: M, 0, 0).
struct LsqTables {
  const float* nl;      // [M]
  const float* inv_d;   // [M]
  const int* pos_m0;    // [frame stride]
  const float* pos_w0;  // [frame stride]
  const float* pos_w1;  // [frame stride]
};
// mel (B, M, T) -> zy (B, M, T): y = G^-1 mel, one lane per frame (the forward sweep's z is held in zy on the way)
hipError_t launch_lsq_solve(const LsqTables& tb, const float* mel, float* zy, int B, int M, int T, hipStream_t s);
// y (B, M, T) -> out [B * T][stride] (stride a multiple of four, out 16-byte aligned): max(0, w0 y[m0] + w1 y[m0 + 1]) per position
hipError_t launch_lsq_expand(const LsqTables& tb, const float* y, float* out, int B, int M, int T, int stride, hipStream_t s);
// backward of the closed form: the collect's tables (rfx_plan_core.h: bank_lstsq_collect)
struct LsqCollectTables {
  const float* wt;      // [longest run][M]: entry i of filter m's run at i * M + m
  const int* first;     // [M]
  const int* run;       // [M]
  const int* vec;       // [n_vecs]
  const int* vec_at;    // [n_vecs][4]
  const float* vec_w0;  // [n_vecs][4]
  const float* vec_w1;  // [n_vecs][4]
  int n_vecs, n_bins;
};
size_t lsq_collect_lds_bytes(int M, int n_bins);
// y (B, M, T), gx [B * T][stride] (stride a multiple of four, gx 16-byte aligned) -> c (B, M, T): the transposed filterbank of gx
// where the forward's relu is open, every bin read once from its first slot.  n_vecs <= kLsqCollectVecs * kLsqCollectThreads.
hipError_t launch_lsq_collect(const LsqCollectTables& tb, const float* y, const float* gx, float* c, int B, int M, int T, int stride, hipStream_t s);

// backward of the forward path (rfx_mel_bwd.hip, arithmetic in rfx_mel_bwd_core.h).  launch_mel_bwd_spec: the magnitude slots
// S [B*T][sstride] a MODE 0 frame launch reads - weight[k] gS[k] / |X[k]| with gS from g_mel (B, M, T) through the adjoint table
// (first / count [n_stft], wt [n_stft][width]) and X [B*T][xstride] the forward transform's spectrum, or, with g_mel and X null, the
// one-sided weights alone.  pos_bin [sstride] / xpos_bin [xstride]: bin of each position of S / X, -1 for padding.  sstride a
// multiple of four, xstride even; S and X 16-byte aligned.
struct MelBwdSpecArgs {
  const float* g_mel;
  const cf* X;
  float* S;
  const int* pos_bin;
  const int* xpos_bin;
  const int* s2x;  // [sstride] position of X whose value magnitude slot p goes with (the frame launch multiplies the two), -1 for padding
  const int* first;
  const int* count;
  const float* wt;
  int width;
  int B, T, M, n_stft, n_fft, xstride, sstride;
  float unit;  // mel_bwd_unit
};
hipError_t launch_mel_bwd_spec(const MelBwdSpecArgs& a, hipStream_t stream);
// step 1 alone: g_mel (B, M, T) -> out (B, n_stft, T)
hipError_t launch_mel_bwd_bank(const float* g_mel, float* out_bft, const int* first, const int* count, const float* wt, int width, int B, int M,
                               int T, int n_stft, hipStream_t stream);
// the adjoint fold: frames [B*T][fpitch], window sample i of a frame at fshift + i -> out (B, Lw).  win: the plan's window where the
// frames come un-windowed (specialised engine), null where the frame launch has applied it.  circular: the fold of a loop row,
// Lw = hop T - no reflect partners, the chain of rfx_loop_core.h
struct MelBwdFoldArgs {
  const float* frames;
  const float* win;
  float* out;
  int fpitch, fshift, left, win_len, hop, h, B, T, Lw;
};
hipError_t launch_mel_bwd_fold(const MelBwdFoldArgs& a, bool circular, hipStream_t stream);

// fused spectral losses (arithmetic in rfx_spec_loss_core.h; the sums are launch_spectral_sums with nsums == 3).
// launch_spec_loss_slots (rfx_mel_bwd.hip): the magnitude slots S [B*T][sstride] of a MODE 0 frame launch that takes the spectrum
// X [B*T][xstride] itself as its angles - weight[k] (dL/da) / a per slot, from a = |the complex value the slot will multiply|, the
// target's slot and the row's coefficients coef[2 b] = c_sc, coef[2 b + 1] = c_lg.  target: [B*T][xstride] in the plan's magnitude
// layout (what rfx_pack_magnitudes writes): read at the slot's own position on the specialised engine, at the slot's bin
// (target_by_bin) on the plain layouts.  sstride a multiple of four, xstride even; S, X and target 16-byte aligned.
struct SpecLossSlotArgs {
  const cf* X;
  const float* target;
  const float* coef;
  float* S;
  const int* pos_bin;  // [sstride] bin of each magnitude slot, -1 for padding
  const int* s2x;      // [sstride] position of X the slot goes with
  int B, T, n_fft, xstride, sstride;
  bool target_by_bin;
  float unit;   // mel_bwd_unit
  float floor;  // 0: no log term
};
hipError_t launch_spec_loss_slots(const SpecLossSlotArgs& a, hipStream_t stream);

// inverse spectrogram (rfx_istft.hip, arithmetic in rfx_istft_core.h).  launch_istft_unit_slots: the magnitude slots S
// [nframes][sstride] of a MODE 0 frame launch that synthesises the caller's spectrum as it is - 1 where pos_bin holds a bin, 0 in the
// padding.  sstride a multiple of four, S 16-byte aligned.
hipError_t launch_istft_unit_slots(float* S, const int* pos_bin, long long nframes, int sstride, hipStream_t stream);
// the staging of the backward: g (rows, valid) -> u, `total` = rows * pitch floats: element col < valid of a row is g times (divide:
// over) tab[col] (period == 0) or tab[col mod period]; the elements from valid to pitch are zeros.  u is 16-byte aligned and holds a
// whole number of 16 bytes (up to three floats behind `total` are written as zeros)
struct IstftStageArgs {
  const float* g;
  const float* tab;
  float* u;
  long long total;
  int pitch, valid, period, divide;
};
hipError_t launch_istft_stage(const IstftStageArgs& a, hipStream_t stream);
// the epilogue of the backward: frames t < T of `rows` rows of Tp analysis frames, spec [rows*Tp][xstride] -> out [rows*T][xstride]
// times c_k unit, imaginary part 0 where c_k = 1, padding 0 (xpos_bin [xstride]: the bin of a position, -1 for padding).  xstride even,
// spec and out 16-byte aligned.
struct IstftGradArgs {
  const cf* spec;
  cf* out;
  const int* xpos_bin;
  int rows, T, Tp, xstride, n_fft;
  float unit;  // istft_unit
};
hipError_t launch_istft_grad(const IstftGradArgs& a, hipStream_t stream);

// time stretch (rfx_vocoder.hip, arithmetic in rfx_vocoder_core.h): in [rows*T][stride] -> out [rows*T_out][stride], complex slots;
// table [stride]: per position the primary position of its bin (| kVocFlip; -1: padding) and the bits of its signed advance in turns
// (rfx_plan_core.h: vocoder_table).  in and out 8-byte aligned and distinct; any number of rows.
struct VocoderArgs {
  const cf* in;
  cf* out;
  const int2* table;
  int rows, T, T_out, stride;
  double rate;
};
hipError_t launch_vocoder(const VocoderArgs& a, hipStream_t stream);

// windowed-sinc resample (rfx_resample.hip, arithmetic in rfx_resample_core.h): `rows` rows of in, in_stride floats apart, read as
// zero outside [0, valid) -> the first K outputs of each row, out_stride floats apart.  first [n] int32 and taps [ntaps][n] float32:
// the polyphase table of the reduced pair o / n (rs_table).  valid <= in_stride, K <= out_stride; any number of rows.  Every index
// the kernel forms from the table is tested against [0, valid), whatever the table holds.
constexpr int kRsRows = 4;  // rows a thread carries for one output index
struct ResampleArgs {
  const float* in;
  float* out;
  const int32_t* first;
  const float* taps;
  int64_t in_stride, out_stride, valid, K;
  int rows, o, n, ntaps;
};
hipError_t launch_resample_sinc(const ResampleArgs& a, hipStream_t stream);

}  // namespace rfx
