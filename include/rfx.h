/*
 * rfx.h - C ABI of librfx.so: the gfx950 (MI355X) implementation of riffusion's
 * spectrogram <-> audio hot path.
 *
 * The reference (riffusion-hobby @ v0.3.1, pure Python) has no FFI for this path: its boundary is
 * the Python class riffusion/spectrogram_converter.py:12-204 whose arithmetic members are four
 * torchaudio modules.  Each entry point below replaces the torchaudio call named in its comment;
 * INTEGRATION.md shows the ctypes binding a maintainer adds under that class.
 *
 * Conventions: every function returns 0 on success and a negative rfx_status on failure;
 * rfx_last_error() returns a thread-local message.  All pointers named d_* are DEVICE pointers
 * (e.g. torch.Tensor.data_ptr()) owned by the caller; `stream` is a hipStream_t passed as void*
 * (torch.cuda.current_stream().cuda_stream).  No entry point allocates device memory except
 * rfx_plan_create; scratch space is a caller-provided workspace sized by the *_workspace_bytes
 * queries.  Plans are immutable after creation and may be shared between threads.
 *
 * Layouts: "BFT" is the reference's (batch, n_stft, frames) tensor layout; "slots" is this
 * library's frame-major stream layout: [batch*frames][rfx_frame_stride()] with every one-sided
 * bin stored at the position its owning thread streams it from (440 bins are stored twice).
 */
#ifndef RFX_H_
#define RFX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rfx_plan rfx_plan;

typedef enum {
  RFX_OK = 0,
  RFX_ERR_INVALID = -1,     /* bad argument / unsupported geometry */
  RFX_ERR_HIP = -2,         /* a HIP runtime call failed */
  RFX_ERR_WORKSPACE = -3,   /* workspace too small */
  RFX_ERR_UNSUPPORTED = -4  /* FFT length with a prime factor above 13 without RFX_ENGINE_CHIRPZ, or whose frame buffer exceeds the 160 KiB
                               of LDS (n_fft above about 39 000; on the chirp-z engine, whose buffer is twice as long, above 19 968
                               when even and 9 983 when odd - the refusal states them); non-banded filterbank */
} rfx_status;

/* Mirrors the fields of riffusion/spectrogram_params.py:21-42 that the arithmetic depends on,
 * already resolved to samples (spectrogram_params.py:62-81). */
typedef struct {
  int32_t sample_rate;
  int32_t n_fft;        /* 17640 at 44.1 kHz: that geometry (win 4410, hop 441) runs on the specialised engine;        */
  int32_t win_length;   /* 4410     n_fft = 40 h, win = 10 h with h in {80 .. 480} (48 kHz: 19200 / 4800 / 480; 32, 24, 16, 8 kHz) and     */
  int32_t hop_length;   /* 441      n_fft = 20 h', win = 5 h' (22.05 kHz: 8820 / 2205 / 220) on the row-family kernels;    */
                        /*          every other geometry (11.025 kHz, 96 kHz, custom durations) on the generic engine      */
  int32_t n_mels;       /* num_frequencies */
  int32_t max_mel_iters;
} rfx_params;

const char* rfx_last_error(void);
int rfx_version(void);
/* number of elements (complex or float) between consecutive frames of a slot-major array */
int rfx_frame_stride(void);   /* of the default 44.1 kHz geometry; per plan: rfx_plan_frame_stride */
int rfx_num_bins(void);
/* frame stride of THIS plan's slot arrays (generic-geometry plans store plain bin-ordered frames, n_stft rounded up to 64) */
int rfx_plan_frame_stride(const rfx_plan* plan);
/* 1 when the plan is a generic-geometry plan (any geometry but 17640 / 4410 / 441): plain bin-ordered frames, and either the
 * row-family kernels (n_fft = 40 h, win = 10 h: the specialised engine's factorisation, 1.7x its per-tile time at 48 kHz) or the
 * generic engine - an in-place mixed-radix FFT (digits up to 16, exact per-pass twiddles) in LDS - for Griffin-Lim and the
 * forward STFT (rfx_plan_griffinlim_engine says which); Griffin-Lim is fused per frame with the momentum applied in the time
 * domain, two launches per iteration, on both */
int rfx_plan_is_generic(const rfx_plan* plan);

/* Builds the device constants that spectrogram_converter.py:47-99 builds as torchaudio module
 * buffers: the periodic Hann window (h_window: win_length floats, as torch.hann_window gives it)
 * and the mel filterbank (h_melfb: n_stft x n_mels floats, torchaudio functional.melscale_fbanks;
 * may be NULL when no mel entry point will be used). */
int rfx_plan_create(const rfx_params* params, const float* h_window, const float* h_melfb, int device,
                    rfx_plan** out_plan);
int rfx_plan_destroy(rfx_plan* plan);

/* Which of the two Griffin-Lim device forms of the specialised engine a call takes (see rfx_griffinlim below). */
typedef enum {
  RFX_GL_FORM_AUTO = 0,   /* per call, from B*T: frames for the few-tiles-per-request case, runs for batches */
  RFX_GL_FORM_RUNS = 1,   /* always the run-based fused kernel (one launch per iteration) */
  RFX_GL_FORM_FRAMES = 2  /* always the per-frame kernel + fold (two launches per iteration) */
} rfx_gl_form;

/* Which frame engine Griffin-Lim runs on for geometries other than 17640 / 4410 / 441 */
typedef enum {
  RFX_ENGINE_AUTO = 0,    /* the row-family kernels where n_fft = 40 h and win_length = 10 h with h in {80, 160, 240, 320, 441, 480}
                             (the default 400 / 100 ms at 8, 16, 24, 32, 44.1, 48 kHz; any hop), the generic FFT engine otherwise */
  RFX_ENGINE_GENERIC = 1, /* always the generic FFT engine (cross-checks) */
  RFX_ENGINE_CHIRPZ = 2   /* as RFX_ENGINE_AUTO, and a geometry AUTO refuses because its FFT length (n_fft / 2 when n_fft is even, n_fft
                             when odd) has a prime factor above 13 runs on the chirp-z engine: Bluestein's algorithm, two mixed-radix
                             FFTs of the smallest factorable length >= 2 x FFT length - 1 per transform, in LDS.  Every
                             entry point serves such a plan.  A geometry AUTO accepts is planned exactly as under AUTO. */
} rfx_frame_engine;

/* Which plan (layouts + kernels) a parameter set gets */
typedef enum {
  RFX_LAYOUT_AUTO = 0,    /* 17640 / 4410 / 441 (the reference's geometry at 44.1 kHz): the specialised engine and its slot-major
                             frames; every other geometry: the generic plan (plain bin-ordered frames) */
  RFX_LAYOUT_GENERIC = 1  /* the generic plan also for 17640 / 4410 / 441: a second, independent implementation of the same
                             transform (row family with h = 441, or the generic FFT engine with RFX_ENGINE_GENERIC) - cross-checks */
} rfx_plan_layout;

/* Which InverseMelScale kernel family a plan may select (rfx_plan_imel_kernel reports the choice) */
typedef enum {
  RFX_IMEL_FORM_AUTO = 0,   /* the wave kernel (one wave per frame) where the bank admits it, else the group kernels */
  RFX_IMEL_FORM_GROUPS = 1  /* never the wave kernel: the group kernels (one workgroup of four waves per frame) - cross-checks */
} rfx_imel_form;

/* Plan-creation options.  Set struct_size = sizeof(rfx_plan_options); zero in every other field means "default".
 * This struct is the library's ONLY configuration surface: a release build reads no environment variable (the RFX_*
 * experiment switches of the source exist only in builds made with -DRFX_ABLATION, tools/build_variants.sh). */
typedef struct {
  uint32_t struct_size;
  int32_t gl_form;             /* rfx_gl_form */
  int32_t gl_frames_per_slot;  /* RFX_GL_FORM_AUTO takes the per-frame form up to this many frames per resident
                                  workgroup slot of the chip (0 = default, 6: the measured crossover - six 512-frame tiles per call;
                                  4 until round 6) */
  int32_t frame_engine;        /* rfx_frame_engine */
  int32_t plan_layout;         /* rfx_plan_layout; added in round 4 - a caller built against the shorter struct gets AUTO */
  int32_t imel_form;           /* rfx_imel_form; added in round 4 after plan_layout, same rule */
} rfx_plan_options;

/* rfx_plan_create with options (NULL = defaults = rfx_plan_create). */
int rfx_plan_create_ex(const rfx_params* params, const float* h_window, const float* h_melfb, int device,
                       const rfx_plan_options* options, rfx_plan** out_plan);
/* the engine rfx_griffinlim runs on for this plan: 0 = specialised (17640 / 4410 / 441), 1 = generic FFT engine, 2 = row family,
 * 3 = chirp-z (the forward STFT of such a plan runs on it as well) */
int rfx_plan_griffinlim_engine(const rfx_plan* plan);
/* the form (RFX_GL_FORM_RUNS / _FRAMES) an rfx_griffinlim call of B x T frames takes on this plan */
int rfx_griffinlim_form(const rfx_plan* plan, int B, int T);
/* (A call with held frames - rfx_held_call_options.d_hold_frames - always takes RFX_GL_FORM_FRAMES on the specialised engine, whatever
 * the plan's gl_form or this rule says: the run form keeps no frame buffer to hold frames in.  Both forms give a clip the same bits.) */
/* (A masked call - rfx_masked_call_options.d_hold_bins - always takes RFX_GL_FORM_FRAMES on the specialised engine as well, whatever
 * the plan's gl_form or this rule says: the run form keeps two parity buffers per generation and sums them at run seams.) */
/* (A loop call - rfx_loop_call_options.loop - always takes RFX_GL_FORM_FRAMES on the specialised engine too: the run form's
 * sliding window and run seams are not looped.) */
/* How one launch of the run-based form cuts the call's B*T frames (counted clip after clip) into runs, one per workgroup: returns
 * the number of runs and, if run_starts != NULL, writes min(runs + 1, capacity) run boundaries (run b = frames
 * [run_starts[b], run_starts[b + 1])).  which = 0: the first (synthesis-only) launch, 1: the iterations.  0 for a generic plan.
 * No device work: the partition is a function of (chip, B, T) alone - results are bit-reproducible call to call.  (tests) */
int rfx_griffinlim_runs(const rfx_plan* plan, int B, int T, int which, int64_t* run_starts, int capacity);
/* the arithmetic behind it, callable without a plan or a GPU (tests): first frame of run b of `runs` over n_frames frames when
 * the first h runs weigh w1 and the others w2 (per mille of the mean run length) */
int64_t rfx_debug_run_start(int64_t b, int64_t runs, int64_t n_frames, int64_t h, int64_t w1, int64_t w2);
/* the partition rfx_griffinlim_runs reports, for a chip with `slots` resident workgroup slots, without a plan or a GPU (tests):
 * runs are whole groups of 16 frames of a row (round 6), the first N mod runs of them one group longer */
int rfx_debug_gl_partition(int slots, int B, int T, int64_t* run_starts, int capacity);
/* the two internal exponents of "Numeric range" above for a largest magnitude max_abs (mel_units != 0: max_abs is a mel amplitude,
 * the Griffin-Lim exponent is then taken for max(max_abs, 1) x 2), without a GPU (tests) */
int rfx_debug_range_exponents(float max_abs, int mel_units, int* sgd_exponent, int* gl_exponent);
/* What rfx_plan_create_ex would decide for these parameters, this filterbank (h_melfb: n_stft x n_mels floats on the host, may be
 * NULL) and these options (NULL = defaults), without a plan or a GPU (tests): the same host code fills the plan's tables.  Set
 * report->struct_size = sizeof(rfx_plan_bank_report).  A geometry the library refuses returns the error of rfx_plan_create_ex. */
typedef struct {
  uint32_t struct_size;
  int32_t engine;          /* as rfx_plan_griffinlim_engine answers */
  int32_t frame_stride;    /* as rfx_plan_frame_stride answers */
  int32_t imel_ok;         /* the bank is banded: rfx_inverse_mel serves it (imel_why says why not) */
  int32_t imel_kernel;     /* as rfx_plan_imel_kernel answers at params->max_mel_iters (-1: no bank, or not banded) */
  int32_t fast_ok;         /* kernel family the bank's groups admit: 2 / 3 per-wave budgets, 5 line form, 1 uniform, 0 none */
  int32_t unit_form;       /* as rfx_plan_imel_unit_form answers */
  int32_t wave_ok;         /* the wave kernel serves the bank */
  int32_t line_from;       /* groups below this index are not lines */
  int32_t f_lo, f_hi;      /* bins with a non-zero filterbank row: [f_lo, f_hi) */
  int32_t nnz;             /* non-zero band entries */
  int32_t fwd_ok;          /* the fused forward path serves the bank */
  int32_t fwd_product;     /* ... in its product form (0: table form) */
  int32_t fwd_packed;      /* ... with the packed tables of the default-bank kernel */
  uint32_t fwd_kb_mask;    /* product form: bit kb set when a thread's slot kb contributes */
  int32_t fwd_prod_arr;    /* product form: floats between the two product arrays */
  int32_t band_rows, Mpad; /* band tables: rows (longest band, rounded up to 8) and columns (n_mels rounded up to 64) */
  int32_t n_kblocks;       /* non-zero 32-position K blocks of the slot-ordered bank (specialised engine) */
  double line_tolerance;   /* a group is a line when no bin leaves its fitted line by more than this fraction of the group's largest weight */
  double line_deviation;   /* the largest such fraction over all non-empty groups (-1: the bank has no group structure) */
  char imel_why[96];
  int32_t fft_length;      /* generic plans: complex FFT length of a frame (n_fft / 2 when n_fft is even, n_fft when odd), else 0 */
  int32_t pass_length;     /* ... and the length the radix passes run at: the same, or the chirp-z engine's convolution length */
  int32_t czt_chirp_elems; /* chirp-z engine: entries of the chirp table and ... */
  int32_t czt_h_elems;     /* ... of H in the LDS layout of the pass_length buffer (padding included), as plan creation builds them; else 0 */
} rfx_plan_bank_report;
int rfx_debug_plan_bank(const rfx_params* params, const float* h_melfb, const rfx_plan_options* options, rfx_plan_bank_report* report);
/* Whether the closed-form InverseMelScale (rfx_inverse_mel_lstsq below) serves this filterbank, and the factor tables its kernels
 * read, without a plan or a GPU (tests): the same host code fills the plan's tables.  Set report->struct_size =
 * sizeof(rfx_lstsq_bank_report) and the two table pointers (NULL, or n_mels floats each on the host; written when ok).
 * Not ok, with the reason in `why`: the bank is not banded (a bin feeds more than two filters, or two that are not adjacent), or a
 * pivot of the L D L^T factorisation of fb^T fb (double) is <= 2^-20 times its diagonal entry - singular or nearly so, e.g. an
 * all-zero filter or the reference's bank at num_frequencies = 1024. */
typedef struct {
  uint32_t struct_size;
  int32_t ok;
  double min_pivot_ratio;  /* smallest pivot / diagonal entry seen, up to and including a refused pivot */
  int32_t min_pivot;       /* its index (-1: the bank is not banded, nothing was factored) */
  int32_t reserved;
  float* h_neg_l;          /* out, optional: -L[m + 1][m] for m = 0 .. n_mels - 2, then 0 */
  float* h_inv_d;          /* out, optional: 1 / D[m] */
  char why[160];
} rfx_lstsq_bank_report;
int rfx_debug_lstsq_bank(const rfx_params* params, const float* h_melfb, rfx_lstsq_bank_report* report);
/* The lists rfx_inverse_mel_lstsq_backward's collect walks, without a plan or a GPU (tests): CSR over the filters.  h_ptr
 * [n_mels + 1]; entries h_ptr[m] .. h_ptr[m + 1] - 1 are filter m's bins in the order they are summed, ascending: the bin, the
 * position of a frame (slot layout) it is read from - its FIRST slot where the layout holds it twice - and the weight
 * melfb[bin][m].  *entries_out: the number of entries; every array is optional, and the three entry arrays need capacity >=
 * *entries_out (call once with NULL arrays to learn it).  A bank rfx_debug_lstsq_bank refuses is refused here with its reason. */
int rfx_debug_lstsq_collect(const rfx_params* params, const float* h_melfb, int32_t* h_ptr, int32_t* h_bin, int32_t* h_pos, float* h_weight,
                            int capacity, int32_t* entries_out);
/* frames torch.stft(center=True, pad_mode="reflect") makes of Lw samples: 1 + (Lw + 2*(n_fft/2) - n_fft) / hop, i.e.
 * 1 + Lw/hop for even n_fft and 1 + (Lw-1)/hop for odd n_fft; 0 when Lw <= n_fft/2 (the reference raises there).
 * Every forward entry point below produces exactly this many frames. */
int rfx_stft_frames(const rfx_plan* plan, int Lw);

/* Per-call options of the inverse entry points (round 6; the *_ex forms below; NULL = defaults = the plain forms).
 * Set struct_size = sizeof(rfx_call_options) and zero everything you do not use.
 *
 * row_base: index, in the caller's WHOLE batch, of the first row (clip-channel) this call converts.  The random starts the
 *   reference draws from torch's global generator (spectrogram_converter.py:72 rand_init=True; torchaudio InverseMelScale's
 *   torch.rand) are drawn here from (seed, row_base + r, frame, bin) for row r of the call.  With the same seed, a batch converted
 *   in one call, in chunks (row_base = rows before the chunk) or sharded over the GPUs of a node gives the same audio for every clip,
 *   bit for bit: nothing else in a clip's arithmetic depends on the batch it travels in (csrc/rfx_kernels.h: kGlGroup).
 *   Must be a multiple of channels_per_clip where the entry point has one.
 * magnitude_hint: see "Numeric range" below; 0 = not given.
 *
 * Numeric range of the inverse entry points (rfx_inverse_mel, rfx_griffinlim, rfx_waveform_from_mel, rfx_audio_from_image_u8
 * and their *_ex forms).  The reference scales a decoded image by a caller-chosen `max_value` (image_util.py:59-108, default 30e6
 * at spectrogram_image_converter.py:69) and runs torchaudio in plain float32; so does this library, with two internal powers of
 * two that keep its fast paths inside float32 whatever the units are:
 *   - InverseMelScale holds the SGD state of a clip times 2^-e, e = max(k + 35, 30) for a largest mel amplitude in [2^(k-1), 2^k)
 *     (e = 60 at max_value 30e6): the `clamp(min=0)` of every step is then the output clamp of the FMA that makes it;
 *   - Griffin-Lim analyses a row's signal times 2^-j, j = k' - 26 for a largest magnitude in [2^(k'-1), 2^k') (j = 0 at 30e6),
 *     so that |a|^2 in a / (|a| + 1e-16) can neither overflow nor vanish.
 * Both commute with every float32 rounding of the linear steps: the results are those of the unscaled arithmetic, and an input
 * times 2^n gives the output times 2^n bit for bit (tests/test_gpu_round6_range.py).  The exponents are taken PER CLIP / PER ROW from
 * the data by one small reduction launch - or from magnitude_hint > 0, an upper bound of the call's magnitudes in the input's
 * units (the image path passes max_value), without reading the data.  A hint below the data is the caller's error: magnitudes
 * above 2^35 x hint saturate the SGD state.
 * Supported, and held against the oracle at 1e-6, 1, 30e6, 1e12, 1e20 (Griffin-Lim also 1e30): magnitudes from 0 up to 2^91 = 2.5e27
 * (InverseMelScale; above it the headroom of the clamp shrinks, at 2^126 it is gone) and 1e33 (Griffin-Lim: float32 itself ends
 * where 8821 bins of that size add up).  Not supported: NaN / Inf magnitudes (garbage in, garbage out, as in the reference).
 * Where the reference itself stops being scale-free, this library follows the reference, not the scale: its stopping rule is
 * absolute (loss < 1e-5, |change| < 1e-8: tiny spectrograms stop after one step - reproduced), the bins no filter reaches keep
 * their U[0,1) start whatever max_value is (reproduced), and below |a| = 1e-8 in the input's units the `+ 1e-16` guard becomes
 * visible: there this library's guard, rsq(|a|^2 + 1e-32), differs from the reference's 1 / (|a| + 1e-16) by up to 41 %
 * (at |a| = 1e-16) in the LENGTH of the phase factor - never in its direction, and it is exactly 0 for a = 0 in both.
 * A guide (rfx_guided_call_options below) is brought into that range by an exact power of two of its own, taken from each row's
 * peak: only the direction of its STFT matters, guide x 2^n gives the same output bytes, and the guard stays invisible for it. */
/* rfx_call_options.flags.  RFX_CALL_INVERSE_MEL_LSTSQ: the fused calls rfx_waveform_from_mel_ex and rfx_audio_from_image_u8_ex run
 * rfx_inverse_mel_lstsq in place of the SGD.  rfx_inverse_mel_ex and rfx_griffinlim_ex refuse any non-zero flag. */
#define RFX_CALL_INVERSE_MEL_LSTSQ 1u
typedef struct {
  uint32_t struct_size;
  uint32_t flags;           /* 0 or RFX_CALL_* bits */
  uint64_t row_base;
  float magnitude_hint;
  float reserved;           /* must be 0 (checked) */
} rfx_call_options;

/* rfx_call_options grown at its tail: the guide of a phase-guided Griffin-Lim start.  The same struct on the wire - every *_ex
 * entry point takes either through its `const rfx_call_options*` and tells them apart by struct_size - under a second name, so that
 * a caller built against the 24-byte struct keeps its type and, passing that size, exactly its behaviour.  Set struct_size =
 * sizeof(rfx_guided_call_options); the first five fields are rfx_call_options' own.
 *
 * d_guide != NULL: Griffin-Lim starts every row of the call from the phase of a waveform the caller already has (in an audio-to-audio
 * workflow: the source clip) instead of random phases.  d_guide: (B, guide_samples) float32 on the plan's device, row r at
 * d_guide + r * guide_stride (elements; >= guide_samples), any units, 4-byte aligned (16-byte aligned rows are read 16 bytes a lane).
 * For row r of a call with T frames, L = rfx_griffinlim_output_samples(plan, T):
 *   fit    g_r = the guide row cut to L samples, or zero-padded at its end to L; its STFT then has exactly T frames;
 *   start  angles0 = G / |G| with G the plan's STFT of g_r (what rfx_stft computes), 0 where G == 0; the rest is the reference's
 *          Griffin-Lim unchanged: n_iter iterations, tprev = 0 in the first, then the final ISTFT - what the oracle's
 *          griffinlim(S, p, angles0=G / (G.abs() + 1e-16), n_iter) computes.  On the device the first launch of the call analyses the
 *          staged guide (a = STFT(g_r); ISTFT(|S| a / |a|)) in place of synthesising from drawn phases: the same number of launches,
 *          rfx_griffinlim_ex's h_launch_ms keeps its n_iter + 1 entries ([0] includes the staging).
 * No randomness: a guided row's result does not depend on seed, on row_base or on the batch it travels in.  Scale: see "Numeric
 * range" above.  Digital silence stays what the mathematics makes of it: a wholly silent guide row gives a silent output row (a zero
 * start is a fixed point of the iteration, in the reference as here), and a zero-padded tail starts silent and is filled by the
 * iterations from the leakage of the neighbouring frames; no noise is injected and nothing falls back to a random start.  NaN / Inf
 * in a guide: garbage in, garbage out, like the magnitudes.
 * Limits: guidance is all rows of a call or none; a guide together with d_angles0_slots, guide_samples <= 0, guide_stride <
 * guide_samples or a pointer off 4-byte alignment is RFX_ERR_INVALID before any launch; so is L <= n_fft / 2 even at n_iter == 0 (the
 * guide is analysed with the reflect padding; the message is rfx_griffinlim's).  Honoured by rfx_griffinlim_ex,
 * rfx_waveform_from_mel_ex and rfx_audio_from_image_u8_ex (B = N x channels rows, clip after clip, as the mel rows);
 * rfx_inverse_mel_ex refuses a guide.  No workspace query grows: the guide is staged in audio buffers the first launch leaves free. */
typedef struct {
  uint32_t struct_size;
  uint32_t flags;
  uint64_t row_base;
  float magnitude_hint;
  float reserved;           /* must be 0 */
  const float* d_guide;     /* NULL: not guided (the call is rfx_call_options' call) */
  int64_t guide_stride;     /* elements between guide rows */
  int32_t guide_samples;    /* samples per guide row */
  int32_t reserved2;        /* must be 0 */
} rfx_guided_call_options;

/* rfx_guided_call_options grown once more, by the same mechanism (struct_size = sizeof(rfx_held_call_options); the first nine fields
 * are rfx_guided_call_options' own): HELD FRAMES.  A guided call uses the guide as a start and every iteration may move every frame;
 * where part of the clip is known audio (a continuation's left part, the kept spans of a partial regeneration, two known ends) the
 * frames of that part can be held at the guide's phase instead.
 *
 * d_hold_frames != NULL: (B, 2) int32 {head, tail} per row on the plan's device, 4-byte aligned.  Frame t of a row with T frames is
 * held iff t < h or t >= T - l, h = clamp(head, 0, T), l = clamp(tail, 0, T - h): any int32 pair is legal, device data is clamped, not
 * validated.  In the reference's loop, after `angles = angles.div(angles.abs().add(1e-16))`, angles[..., held] = a0[..., held] with a0
 * the guided start's angles; everything else stays as it is (tprev = rebuilt for all frames).  Exact consequences:
 *   (0, 0) for a row gives that row the bytes of the guided call (d_hold_frames == NULL);
 *   h + l == T gives that row the bytes of the guided call with n_iter == 0, whatever n_iter is;
 *   a sample covered only by held frames (every frame whose window reaches it is held) has at any n_iter the bytes it has at n_iter == 0.
 * A row's bytes depend on its magnitudes, its guide row and its pair alone - not on the other rows' pairs, its place in the batch, seed
 * or row_base.  Only the phase is held: the magnitudes stay the call's.
 * On the device the synthesis frame of a held frame is written once, by the first launch, and only read afterwards: the call compacts
 * the free frames into a list in its workspace (three small launches, no host read, no synchronisation, nothing allocated) and launches
 * 1 .. n_iter walk that list, so a held call does less work in proportion to what it holds.  h_launch_ms keeps n_iter + 1 entries, [0]
 * including the staging and the compaction.
 * Workspace: the entry's *_workspace_bytes_ex query with the call's options (the frame list, B T + a few int32, and on the specialised
 * engine the frame buffer of the per-frame form: a held call always takes that form, see rfx_griffinlim_form); at least the unheld query.
 * RFX_ERR_INVALID before any launch: d_hold_frames without d_guide, a pointer off 4-byte alignment, reserved3 != 0;
 * RFX_ERR_WORKSPACE: a workspace below the held query.  Honoured by the three entries that honour a guide; rfx_inverse_mel_ex refuses
 * it. */
typedef struct {
  uint32_t struct_size;
  uint32_t flags;
  uint64_t row_base;
  float magnitude_hint;
  float reserved;           /* must be 0 */
  const float* d_guide;
  int64_t guide_stride;
  int32_t guide_samples;
  int32_t reserved2;        /* must be 0 */
  const int32_t* d_hold_frames; /* NULL: nothing held (the call is rfx_guided_call_options' call) */
  uint64_t reserved3;       /* must be 0 */
} rfx_held_call_options;

/* rfx_held_call_options grown once more, by the same mechanism (struct_size = sizeof(rfx_masked_call_options); the first eleven
 * fields are rfx_held_call_options' own): MASKED CALLS.  Held frames keep whole frames; a partial regeneration that keeps the
 * source where a mask image is dark (a frequency band, a time-frequency pattern) knows the source's phase in BINS of frames.
 *
 * d_hold_bins != NULL: (B, T, hold_words) uint32 on the plan's device, 4-byte aligned, hold_words == rfx_hold_mask_words(plan) =
 * ceil(n_stft / 32) (276 for the default geometry).  Bin b of frame t of row r is held iff bit b & 31 of word b >> 5 of that frame is
 * set; bits at or above n_stft in the last word are ignored (they need not be zero).  rfx_hold_bins_from_bands below makes the mask
 * from a per-mel-band mask.  In the reference's loop, after `angles = angles.div(angles.abs().add(1e-16))`,
 * angles = torch.where(held, a0, angles) with held the (B, n_stft, T) boolean and a0 the guided start's angles; everything else stays
 * as it is (tprev = rebuilt for all bins, the momentum term, the final ISTFT).  Only the phase is held: the magnitudes stay the call's.
 * On the device the hold is applied through its linearity: with S_held = S in the held bins and 0 elsewhere, S_free = S - S_held and
 * c = ISTFT(S_held a0), every iterate is x_k = ISTFT(S_free proj(STFT(x_{k-1}) - m STFT(x_{k-2}))) + c with x_0 = ISTFT(S a0): the
 * iterations run on magnitudes that are zero in the held bins and the constant audio c is added to each generation as it is folded.
 * In float64 the two forms agree to 1e-14; in float32 they round differently (within a few dB of each other against float64).
 * Exact consequences (values compare with ==; the + c turns a -0.0 sample into +0.0, so these are not bit comparisons unless stated):
 *   n_iter == 0: the guided call's bytes, whatever the mask;
 *   an all-zero mask row: that row equals the guided call's row at the same n_iter, on the same form;
 *   an all-ones mask row: that row equals the guided call's row at n_iter == 0, whatever n_iter is;
 *   a row depends on its magnitudes, its guide row and its mask row alone - not on the other rows, its place in the batch, seed or
 *   row_base: bit for bit.
 * Launches: the guide's staging, the split X = S_held, one more first-launch-class launch and fold (c), the guided call's first
 * launch on S, the split X = S_free, then launches 1 .. n_iter on X; n_iter == 0 skips the splits and c.  A mask removes no
 * iteration work (a frame whose every bin is held still runs).  h_launch_ms keeps n_iter + 1 entries, [0] including the staging, the
 * split and the c launch.  On the specialised engine a masked call always takes RFX_GL_FORM_FRAMES (see rfx_griffinlim_form).
 * Workspace: the entry's *_workspace_bytes_ex query with the call's options (the per-frame form's frame buffer, one more magnitude
 * array X, and c: B rows of audio); at least the unmasked query.
 * RFX_ERR_INVALID before any launch, the output untouched: d_hold_bins without d_guide; together with d_hold_frames (in this version:
 * fully set frames in the mask express the same hold); together with d_angles0_slots; hold_words != rfx_hold_mask_words(plan); a
 * pointer off 4-byte alignment; reserved4 != 0.  RFX_ERR_WORKSPACE: a workspace below the masked query.  Honoured by
 * rfx_griffinlim_ex, rfx_waveform_from_mel_ex and rfx_audio_from_image_u8_ex (rows clip after clip, as the mel rows);
 * rfx_inverse_mel_ex refuses it.  A caller passing any of the three shorter struct sizes keeps exactly its behaviour and bytes. */
typedef struct {
  uint32_t struct_size;
  uint32_t flags;
  uint64_t row_base;
  float magnitude_hint;
  float reserved;           /* must be 0 */
  const float* d_guide;
  int64_t guide_stride;
  int32_t guide_samples;
  int32_t reserved2;        /* must be 0 */
  const int32_t* d_hold_frames;
  uint64_t reserved3;       /* must be 0 */
  const uint32_t* d_hold_bins; /* NULL: no bins held (the call is rfx_held_call_options' call) */
  int32_t hold_words;       /* words per frame of d_hold_bins: rfx_hold_mask_words(plan) */
  int32_t reserved4;        /* must be 0 */
} rfx_masked_call_options;

/* rfx_masked_call_options grown once more, by the same mechanism (struct_size = sizeof(rfx_loop_call_options); the first fourteen
 * fields are rfx_masked_call_options' own): LOOP CALLS.  loop == 1: the row's T columns are the STFT of a signal with period
 * P = hop T that runs from its end into its start - the tile is a loop, and the decode has no seam at the loop point.
 *
 * Definition.  h = n_fft / 2 (integer division), left = (n_fft - win_length) / 2, w the plan's window zero-padded to n_fft:
 *   analysis   frame t, element i is x[(hop t + i - h) mod P] w[i], followed by the plan's real FFT - torch.stft(center=False) of
 *              x[P - h:] || x || x[:n_fft - h] with the last frame dropped;
 *   synthesis  y[m] = (sum of w[i] frame_t[i] over hop t + i - h = m mod P) / env[m], env[m] the same sum of w[i]^2;
 *              P samples per row, for even and odd n_fft alike: rfx_griffinlim_loop_output_samples(plan, T) = hop T.
 * The loop is torchaudio's functional.griffinlim unchanged - the random start, the momentum with tprev = 0 first, the 1e-16 guard,
 * the final synthesis - with these two transforms in the place of torch.stft(center=True, reflect) and torch.istft.  env depends on
 * m mod hop alone and is never small (3.75 to 1e-6 at the default geometry): there is no n_fft / 2 edge zone.
 * On the device: the first launch (S angles0 -> frames) is the unlooped call's; launches 1 .. n_iter read their input modulo P
 * (compile-time variants of the frame kernels), and every fold is circular: a sample sums its covering frames as one chain from the
 * oldest covering frame on, the same chain wherever in the period it lies, times 1 / env from a hop-entry table made once per call.
 * Exact consequences, bit for bit: columns (and injected angles) rolled by k give the audio rolled by k hop; a row depends on its
 * magnitudes, its start and - through the random start only - on seed and row_base + its index, not on the batch.
 * A guide (d_guide) is allowed: it is fitted to P samples by the guided call's rule and its start is G / |G| of the circular STFT.
 * On the specialised engine a loop call always takes RFX_GL_FORM_FRAMES (the run form's sliding window and seams are not looped);
 * the chirp-z engine refuses a loop call (RFX_ERR_UNSUPPORTED).  h_launch_ms keeps n_iter + 1 entries.
 * Workspace: the entry's *_workspace_bytes_ex query with the call's options; 0 for a call that is refused (chirp-z, hop T < n_fft).
 * RFX_ERR_INVALID before any launch, the output untouched: loop > 1; reserved5 != 0; loop together with d_hold_frames or
 * d_hold_bins; hop T < n_fft (a frame must cover the period at most once: T >= 40 at the default geometry, the smallest T is in the
 * message).  RFX_ERR_WORKSPACE: a workspace below the loop query.  Honoured by rfx_griffinlim_ex, rfx_waveform_from_mel_ex and
 * rfx_audio_from_image_u8_ex (hop T samples / PCM frames per row then); rfx_inverse_mel_ex refuses it.  A caller passing any of the
 * four shorter struct sizes keeps exactly its behaviour and bytes. */
typedef struct {
  uint32_t struct_size;
  uint32_t flags;
  uint64_t row_base;
  float magnitude_hint;
  float reserved;           /* must be 0 */
  const float* d_guide;
  int64_t guide_stride;
  int32_t guide_samples;
  int32_t reserved2;        /* must be 0 */
  const int32_t* d_hold_frames;
  uint64_t reserved3;       /* must be 0 */
  const uint32_t* d_hold_bins;
  int32_t hold_words;
  int32_t reserved4;        /* must be 0 */
  uint32_t loop;            /* 0: the call is rfx_masked_call_options' call; 1: a loop call */
  uint32_t reserved5;       /* must be 0 */
} rfx_loop_call_options;

/* rfx_loop_call_options grown once more, by the same mechanism (struct_size = sizeof(rfx_start_call_options); the first sixteen
 * fields are rfx_loop_call_options' own): THE START.  Text-to-audio has no guide: only magnitudes exist, and the reference starts
 * Griffin-Lim from U[0,1) phases.  start == 1 starts it from phases built from the magnitudes alone instead (single-pass spectrogram
 * inversion with phase-vocoder peak tracking): no randomness, no guide, fewer iterations for the same spectral convergence at low
 * iteration counts on tonal material (README).  A call with start == 1 is rfx_peak_start (below) on the call's magnitudes followed
 * by the same call with those angles injected as d_angles0_slots - same bits; for the fused entries the magnitudes are the ones
 * their InverseMelScale stage leaves in the workspace.  A row's bytes then depend on its magnitudes alone - not on seed (the
 * InverseMelScale stage of a fused call still draws its own start from it), row_base, the other rows or its place in the batch.
 * loop == 1 together with start == 1 is served: the first launch of a loop call is the unlooped call's, and both transforms centre
 * frame t at hop t.  h_launch_ms keeps n_iter + 1 entries, [0] including the start.
 * Workspace: the entry's *_workspace_bytes_ex query with the call's options (the call without the start, plus the angles and
 * rfx_peak_start's own workspace); loop == 1 together with start == 1 is sized by the same query.
 * RFX_ERR_INVALID before any launch, the output untouched: start > 1; reserved6 != 0; start == 1 together with d_guide, with
 * d_angles0_slots, with d_hold_frames or with d_hold_bins (each is a start, or needs the guide's).  RFX_ERR_UNSUPPORTED: a plan whose
 * frame does not fit the LDS (rfx_peak_start).  RFX_ERR_WORKSPACE: a workspace below the query.  Honoured by rfx_griffinlim_ex,
 * rfx_waveform_from_mel_ex and rfx_audio_from_image_u8_ex; rfx_inverse_mel_ex refuses it.  A caller passing any of the five shorter
 * struct sizes keeps exactly its behaviour and bytes.  (A new struct, not a flag bit: flags == 2 stays refused.) */
typedef struct {
  uint32_t struct_size;
  uint32_t flags;
  uint64_t row_base;
  float magnitude_hint;
  float reserved;           /* must be 0 */
  const float* d_guide;
  int64_t guide_stride;
  int32_t guide_samples;
  int32_t reserved2;        /* must be 0 */
  const int32_t* d_hold_frames;
  uint64_t reserved3;       /* must be 0 */
  const uint32_t* d_hold_bins;
  int32_t hold_words;
  int32_t reserved4;        /* must be 0 */
  uint32_t loop;
  uint32_t reserved5;       /* must be 0 */
  uint32_t start;           /* 0: the call is rfx_loop_call_options' call; 1: the spectral-peak start */
  uint32_t reserved6;       /* must be 0 */
} rfx_start_call_options;

/* The workspace of a call of rfx_griffinlim_ex, rfx_waveform_from_mel_ex or rfx_audio_from_image_u8_ex with these options: pass the
 * call's own struct.  options is read exactly as the entry of the same name reads it (struct_size, flags, reserved fields, the
 * combination rules, pointer alignment; device pointers are tested for NULL and alignment and never dereferenced; row_base and
 * magnitude_hint do not enter the size).  Options the entry refuses give 0, with the entry's refusal in rfx_last_error under the
 * query's name.  options == NULL is the plain query (rfx_griffinlim_workspace_bytes, ...).  0 also for a NULL plan and for a loop
 * call the plan or T cannot serve (the chirp-z engine, hop T < n_fft). */
size_t rfx_griffinlim_workspace_bytes_ex(const rfx_plan* plan, int B, int T, const rfx_call_options* options);
size_t rfx_waveform_from_mel_workspace_bytes_ex(const rfx_plan* plan, int B, int T, const rfx_call_options* options);
size_t rfx_audio_from_image_workspace_bytes_ex(const rfx_plan* plan, int N, int stereo, int T, const rfx_call_options* options);

/* ---- the spectral-peak start: initial angles for Griffin-Lim from the magnitudes alone ---------------------------------------------
 * d_mag_slots: magnitudes in slot layout, B T frames (what rfx_pack_magnitudes and rfx_inverse_mel write); d_angles0_slots_out: B T
 * frames of complex64 in the layout d_angles0_slots takes - what rfx_pack_complex produces: conjugate slots conjugated, both copies
 * of the bins the specialised layout stores twice written, padding 0.  Row r is one clip-channel, m[k] the float32 magnitude of bin
 * k = 0 .. F - 1 of frame t, F = n_stft, N = n_fft.
 * Decisions, in float32 on the float32 inputs (exact: the same on every machine):
 *   thr = 1e-5f * max_k m[k] (NaN entries skipped); k is a peak iff 1 <= k <= F - 2, m[k] > m[k-1], m[k] >= m[k+1] and m[k] > thr
 *   (any comparison with a NaN is false); with the peaks p_0 < p_1 < ..., bin j belongs to p_i for the smallest i with
 *   j <= (p_i + p_{i+1}) / 2 (integer division), to the last peak if there is none.
 * Arithmetic, in double from the float32 inputs: with a, b, c = m[p-1], m[p], m[p+1], pos = p + clamp(0.5 (a - c) / (a - 2 b + c),
 *   -0.5, 0.5).  Phase is counted in turns.  A frame with no peak has phase 0 everywhere and cuts the chain; the first frame of a
 *   chain (t = 0, or after a frame with no peak) has phi[p] = 0 at every peak; otherwise, q being the peak of frame t - 1 that owns
 *   bin p, phi_t[p] = frac(phi_{t-1}[q] + 0.5 (pos_{t-1}[q] + pos_t[p]) hop / N) (the factor hop / N is formed once, in double).
 *   angles0[r, k, t] = (-1)^k (cos, sin)(2 pi phi_t[owner(k)]), cosine and sine formed in float32 from the fraction.  (Frames are
 *   referenced to their first sample, n_fft / 2 before the centre: a centred sinusoid alternates in sign from bin to bin.)
 * A row depends on its magnitudes alone.  Both copies of a bin the layout stores twice must be equal, as the library writes them.
 * Three launches (owners per frame; the chain, one workgroup per row, sequential over its frames; angles per frame), nothing
 * synchronises.  All three frame engines.  RFX_ERR_UNSUPPORTED, with the reason, for a plan whose frame does not fit the LDS:
 * n_stft above 10240 (the chain keeps two doubles per bin in 160 KiB).  B == 0 is a no-op.  Row and element offsets are 64-bit.
 * Workspace: B T n_stft (2 + 8) bytes, each part rounded up to 256 (the owner of every bin, position / phase of every peak); 0 for
 * a NULL plan. */
size_t rfx_peak_start_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_peak_start(const rfx_plan* plan, const float* d_mag_slots, int B, int T, void* d_angles0_slots_out, void* d_workspace,
                   size_t workspace_bytes, void* stream);

/* words per frame of a masked call's d_hold_bins: ceil(n_stft / 32); 0 for a NULL plan */
int rfx_hold_mask_words(const rfx_plan* plan);
/* A per-mel-band mask, in the layout of the mel tensor, to the bin mask of rfx_masked_call_options.  d_bands: (B, n_mels, T) uint8,
 * nonzero = held; d_hold_bins_out: (B, T, rfx_hold_mask_words(plan)) uint32.  For bin f let [lo_f, hi_f] be the first and last band
 * with a nonzero weight in the plan's filterbank at row f: bin f of frame t is held iff that range exists and every band in it is held
 * at t.  A bin no filter reaches is never held (it carries no information from the tile).  Every bit of every word is written; the
 * unused tail bits of the last word as 0.  The plan needs its filterbank (RFX_ERR_INVALID without). */
int rfx_hold_bins_from_bands(const rfx_plan* plan, const uint8_t* d_bands, int B, int T, uint32_t* d_hold_bins_out, void* stream);
/* [lo_f, hi_f] of every bin as plan creation computes them, without a GPU (as rfx_debug_plan_bank): lo, hi hold n_stft int16 each;
 * lo = hi = -1 for a bin with no band.  h_melfb: (n_stft, n_mels) float32. */
int rfx_debug_bin_bands(const rfx_params* params, const float* h_melfb, int16_t* lo, int16_t* hi);

/* ---- layout converters ------------------------------------------------------------------- */
/* (B, n_stft, T) float32 magnitudes -> slots (float32) */
int rfx_pack_magnitudes(const rfx_plan* plan, const float* d_lin_bft, int B, int T, float* d_slots, void* stream);
/* (B, n_stft, T) complex64 -> slots (complex64); conjugate slots are conjugated */
int rfx_pack_complex(const rfx_plan* plan, const void* d_bft, int B, int T, void* d_slots, void* stream);
/* slots (complex64) -> (B, n_stft, T) complex64 */
int rfx_unpack_complex(const rfx_plan* plan, const void* d_slots, int B, int T, void* d_bft, void* stream);

/* ---- forward: torchaudio.transforms.Spectrogram(power=None) [+ torch.abs] ------------------
 * spectrogram_converter.py:179 (+ :182).  d_wave: (B, Lw) float32, Lw > n_fft/2.
 * T = rfx_stft_frames(plan, Lw).  Either output may be NULL. */
int rfx_stft(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mag_slots, void* d_spec_slots,
             void* stream);

/* ---- quality of a decode: the two sums of spectral convergence, || |STFT(x)| - S || / || S ||, per row --------------------------
 * d_wave (B, L) float32, L = rfx_griffinlim_output_samples(plan, T) (its STFT has exactly T frames; L must exceed n_fft/2, as for
 * rfx_stft); d_mag_slots: the target S, magnitudes in slot layout, B * T frames (what rfx_inverse_mel writes and rfx_griffinlim
 * reads).  For row r, d_sums_out[2 r] = sum (a - m)^2 and d_sums_out[2 r + 1] = sum m^2 over every one of the n_stft bins of every
 * one of the T frames exactly once (padding positions and the second copy of the 440 bins the specialised layout stores twice are
 * not counted): a = the magnitude rfx_stft gives for the row (formed in the workspace), m = the target.  a - m is formed in double
 * from the two float32 values (exact); squares and sums are double: magnitudes up to the 1e33 of "Numeric range" square to 1e66.
 * Spectral convergence of a row is sqrt(sums[0] / sums[1]); of a clip, sqrt of the ratio of its channels' added sums.  Two sums,
 * not a ratio, so that the caller pools rows exactly and decides what a silent target (sum m^2 == 0) means.
 * Deterministic and batch-invariant: a row's reduction is one fixed tree whose shape depends on (T, plan) alone - no atomics,
 * nothing depends on B, on the row's place in the call or on the launch grid - so a row's 16 bytes are the same alone and in any
 * batch.  Each sum is within n * 2^-52 (relative; n = n_stft * T) of the exact sum of its float32 inputs.
 * Against the CPU oracle (oracle/riffusion_oracle.py spectral_convergence: torch.stft and both norms in float32) the value differs by
 * the ORACLE's float32 error: on 4-iteration Griffin-Lim results of 64-column ranges of the five golden tiles the oracle's own
 * float32-vs-float64 distance for the figure was measured at 1.3e-6 .. 8.8e-6 relative on one host and 4e-7 .. 6.0e-5 on another
 * (it moves with the input and with the host's torch build and thread count), while this entry's value sat 4e-9 .. 1.2e-8 from the
 * float64 figure.  The test therefore measures the oracle's distance on its own inputs in the same run and allows 2 times the
 * largest: this library's figure and the oracle's float32 figure each lie within that distance of the float64 figure - this one far
 * closer, its transform being float32 as well but its sums double - hence within twice of it of each other.
 * All three frame engines.  The rows are walked in groups, so the workspace is bounded whatever B is: the magnitudes of
 * max(1, 128 MiB / (T * frame_stride * 4 bytes)) rows plus 16 bytes per four frames of them - at most 128 MiB + 64 KiB + 512
 * bytes, or one row's magnitudes (and partial sums) when a row alone is larger.  B == 0 is a no-op.  d_mag_slots and d_workspace
 * must be 16-byte aligned.  Row and element offsets are 64-bit: B past 65535 and slot offsets past 2^31 elements are served. */
size_t rfx_spectral_error_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_spectral_error(const rfx_plan* plan, const float* d_wave /* (B, L) */, const float* d_mag_slots, int B, int T,
                       double* d_sums_out /* (B, 2) */, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- LOOP ENCODE: the forward entries on the circular STFT - the analysis half of rfx_loop_call_options -------------------------
 * A row of a *_loop forward entry is one period of a signal that runs from its end into its start: P = Lw samples, T = P / hop
 * frames.  With h = n_fft / 2 (integer division) and w the plan's window zero-padded to n_fft, frame t, element i is
 * x[(hop t + i - h) mod P] w[i]; the plan's real FFT follows.  This is the analysis a loop decode runs inside Griffin-Lim, so the
 * rfx_griffinlim_loop_output_samples(plan, T) samples a loop decode writes are a legal row and give its T frames back, and a tile
 * made this way closes: rolling a row by k hop rolls its columns by k, bit for bit.  A frame whose window lies inside [0, P) has the
 * bytes the plain entry gives for the same samples; only the frames whose window reaches over an end differ (the plain entries read
 * the reflected signal there, and make one frame more).
 * Lw must be a positive multiple of hop_length and at least n_fft (the loop decode's rule, hop T >= n_fft: a frame covers the period
 * at most once).  Any other Lw: RFX_ERR_INVALID before any launch, the outputs untouched, the message naming the nearest legal
 * lengths below and above ("none" below the smallest one).  Everything else - layouts, outputs, workspace rules, batch invariance,
 * the refusals - is the plain entry's.  On the device each entry runs the loop twin of the kernel its plain form runs, on all four
 * frame engines: the same code with the sample position wrapped instead of reflected (the chirp-z engine still refuses a loop
 * DECODE).  A workspace query answers 0 where the call would be refused; a fused loop entry gives exactly the bytes of its parts. */
/* frames a loop forward call makes of rows of Lw samples: Lw / hop_length, or 0 where the call would be refused */
int rfx_stft_loop_frames(const rfx_plan* plan, int Lw);
/* the length rule of a loop forward call, without a plan or a GPU (tests): RFX_OK, or the RFX_ERR_INVALID a loop forward call on
 * rows of Lw samples at these parameters gets, with its message */
int rfx_debug_loop_samples(const rfx_params* params, int Lw);
/* the nearest legal lengths that message names, as numbers (callers that state them in other units): *below the largest legal
 * length <= Lw, 0 where there is none; *above the smallest one >= Lw.  For a legal Lw both are Lw. */
int rfx_debug_loop_nearest_samples(const rfx_params* params, int Lw, int64_t* below, int64_t* above);
/* rfx_stft on the circular STFT: d_wave (B, Lw) float32 -> T = rfx_stft_loop_frames(plan, Lw) frames per row.  Either output may be NULL. */
int rfx_stft_loop(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mag_slots, void* d_spec_slots,
                  void* stream);
/* rfx_mel_from_waveform on the circular STFT: d_wave (B, Lw) -> d_mel_out (B, n_mels, T), T = rfx_stft_loop_frames(plan, Lw) */
size_t rfx_mel_loop_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_mel_from_waveform_loop(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace,
                               size_t workspace_bytes, void* stream);
/* rfx_image_from_waveform on the circular STFT: d_img_out (N, n_mels, T, 3).  Byte-identical to rfx_mel_from_waveform_loop followed
 * by rfx_image_encode_u8, d_clip_max included. */
size_t rfx_image_from_waveform_loop_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw);
int rfx_image_from_waveform_loop(const rfx_plan* plan, const float* d_wave, int N, int stereo, int Lw, const float* d_thresholds255,
                                 float* d_clip_max, uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream);
/* rfx_image_from_pcm16_clips on the circular STFT: exactly rfx_pcm16_clips_to_waveform followed by rfx_image_from_waveform_loop,
 * same bytes.  N == 0 is a no-op. */
size_t rfx_image_from_pcm16_clips_loop_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw);
int rfx_image_from_pcm16_clips_loop(const rfx_plan* plan, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts,
                                    const int64_t* d_starts, int N, int Lw, int stereo, const float* d_thresholds255, float* d_clip_max,
                                    uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream);
/* rfx_spectral_error of a loop decode: d_wave (B, hop T) float32 - what a loop decode of T frames writes; a = the magnitude
 * rfx_stft_loop gives for the row.  The same two double sums per row, the same fixed reduction tree, the same batch invariance and
 * the same bounded workspace as the plain entry.  T must satisfy the loop decode's rule (rfx_debug_loop_frames). */
size_t rfx_spectral_error_loop_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_spectral_error_loop(const rfx_plan* plan, const float* d_wave /* (B, hop T) */, const float* d_mag_slots, int B, int T,
                            double* d_sums_out /* (B, 2) */, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- inverse: torchaudio.transforms.GriffinLim(n_iter, momentum=0.99, rand_init=True, power=1)
 * spectrogram_converter.py:62-73, called at :204.
 * d_mag_slots: magnitudes in slot layout; d_angles0_slots: optional injected initial angles
 * (NULL = draw U[0,1) real/imag per bin from `seed`); d_wave_out: (B, rfx_griffinlim_output_samples(plan, T)) float32. */
/* Two device forms, chosen per call from B*T: the run-based fused kernel (one launch per iteration) for batches, and a
 * per-frame kernel + fold (two launches per iteration, every frame its own workgroup) for the few-tiles-per-request case;
 * the workspace query below accounts for whichever the shape will take. */
size_t rfx_griffinlim_workspace_bytes(const rfx_plan* plan, int B, int T);
/* (of a call with options - held frames, a mask, a loop, the spectral-peak start: rfx_griffinlim_workspace_bytes_ex above) */
/* samples per row a loop call writes for T frames: the period hop T; 0 for a NULL plan or T <= 0 */
int rfx_griffinlim_loop_output_samples(const rfx_plan* plan, int T);
/* the frame-count rule of a loop call, without a plan or a GPU (tests): RFX_OK, or the RFX_ERR_INVALID a loop call of T frames at
 * these parameters gets, with its message */
int rfx_debug_loop_frames(const rfx_params* params, int T);
/* samples per clip rfx_griffinlim writes for T frames: what torch.istft(center=True, length=None) returns,
 * hop*(T-1), plus one when n_fft is odd */
int rfx_griffinlim_output_samples(const rfx_plan* plan, int T);
int rfx_griffinlim(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                   int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                   void* stream);

/* rfx_griffinlim with per-call options (NULL = rfx_griffinlim) and, when h_launch_ms != NULL, rfx_griffinlim_timed's
 * per-launch durations (it then synchronises the stream). */
int rfx_griffinlim_ex(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                      int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                      void* stream, const rfx_call_options* options, float* h_launch_ms);

/* Same as rfx_griffinlim, but brackets every kernel launch with HIP events recorded on `stream`
 * and, after synchronising, writes the n_iter+1 launch durations (ms; [0] = the init ISTFT, [1] the
 * first iteration, [2..] the steady-state iterations) to the HOST array h_launch_ms.  Measurement
 * aid for bench.py's roofline figure; it synchronises the stream. */
int rfx_griffinlim_timed(const rfx_plan* plan, const float* d_mag_slots, const void* d_angles0_slots, uint64_t seed, int B,
                         int T, int n_iter, float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
                         void* stream, float* h_launch_ms);

/* slots (float32) -> (B, n_stft, T) float32 */
int rfx_unpack_magnitudes(const rfx_plan* plan, const float* d_slots, int B, int T, float* d_bft, void* stream);

/* ---- forward: mel_amplitudes_from_waveform, spectrogram_converter.py:165-185
 * Spectrogram(power=None) -> torch.abs -> MelScale (matmul with the filterbank, on the fp32 MFMA).
 * d_wave (B, Lw) float32 -> d_mel_out (B, n_mels, T) float32, T = rfx_stft_frames(plan, Lw). */
size_t rfx_mel_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_mel_from_waveform(const rfx_plan* plan, const float* d_wave, int B, int Lw, float* d_mel_out, void* d_workspace,
                          size_t workspace_bytes, void* stream);

/* ---- forward, all the way to the image: SpectrogramImageConverter.spectrogram_image_from_audio's device half
 * (spectrogram_image_converter.py:30-51: spectrogram_from_audio, then image_util.image_from_spectrogram, image_util.py:27-54).
 * d_wave (N*C, Lw) float32 (C = 2 when stereo: the channels of clip n are rows 2n, 2n+1) -> d_img_out (N, n_mels, T, 3) uint8 and
 * d_clip_max (N floats: the EXIF MAX_VALUE, spectrogram_image_converter.py:45-49).  Byte-identical to rfx_mel_from_waveform
 * followed by rfx_image_encode_u8; the (N*C, n_mels, T) tensor is never written: the maximum is taken while the mel amplitudes
 * are formed and the encoder reads the forward kernel's frame-major scratch. */
size_t rfx_image_from_waveform_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw);
int rfx_image_from_waveform(const rfx_plan* plan, const float* d_wave, int N, int stereo, int Lw, const float* d_thresholds255,
                            float* d_clip_max, uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* The same from int16 PCM: the N clips of Lw frames that start at the frame offsets `starts` of one recording d_pcm (frames,
 * in_channels) int16 - see rfx_pcm16_clips_to_waveform below for the arguments and what is checked - are gathered into the
 * workspace and converted: exactly rfx_pcm16_clips_to_waveform (out_channels = stereo ? 2 : 1) followed by
 * rfx_image_from_waveform, same bytes.  N == 0 is a no-op. */
size_t rfx_image_from_pcm16_clips_workspace_bytes(const rfx_plan* plan, int N, int stereo, int Lw);
int rfx_image_from_pcm16_clips(const rfx_plan* plan, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts,
                               const int64_t* d_starts, int N, int Lw, int stereo, const float* d_thresholds255, float* d_clip_max,
                               uint8_t* d_img_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* Standalone torchaudio.transforms.MelScale.forward (spectrogram_converter.py:185) for callers that hold linear
 * magnitudes in the reference's (B, n_stft, T) layout: packs them into slots and runs the same MFMA projection.
 * Workspace: rfx_mel_scale_workspace_bytes. */
size_t rfx_mel_scale_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_mel_scale(const rfx_plan* plan, const float* d_lin_bft, int B, int T, float* d_mel_out, void* d_workspace,
                  size_t workspace_bytes, void* stream);

/* ---- BACKWARD of the forward path: the gradients torch.autograd gives through Spectrogram(power=None), torch.abs and MelScale ------
 * With h = n_fft / 2, left = (n_fft - win_length) / 2, w the window zero-padded to n_fft, a row x of Lw > h samples,
 * T = rfx_stft_frames of Lw, X the row's complex STFT as rfx_stft computes it, and g_mel (n_mels, T) the incoming gradient:
 *   1  bank adjoint       gS[k][t] = sum_m fb[k][m] g_mel[m][t], over the bands from the first to the last non-zero weight of bin k
 *                         (the per-bin table of rfx_debug_mel_adjoint), in increasing m
 *   2  magnitude adjoint  G[k][t] = gS[k][t] X[k][t] / |X[k][t]|, exactly 0 where |X| == 0 (torch's abs backward: a silent row has a
 *                         zero, finite gradient).  For rfx_stft_backward G is the caller's complex gradient, dL/dRe + i dL/dIm.
 *   3  frame adjoint      f_t[i] = sum_k Re G[k][t] cos(2 pi k i / n_fft) - Im G[k][t] sin(2 pi k i / n_fft): every one-sided bin
 *                         with weight 1 (n_fft irfft of G with the interior bins halved); the imaginary parts of bin 0 and of the
 *                         Nyquist bin of an even n_fft drop out.  Odd n_fft included.
 *   4  adjoint fold       gp[q] = sum_t w[q - hop t] f_t[q - hop t] as ONE chain from the oldest covering frame on; sample j of the
 *                         result is gp[h + j], plus gp[h - j] when 1 <= j <= h, plus gp[h + 2 (Lw - 1) - j] when
 *                         Lw - 1 - h <= j <= Lw - 2 (the reflect padding folded back), added in that order.  No envelope division,
 *                         no trimming, no atomics.
 * On the device, per group of rows: [the fused call: rfx_stft of the rows, spectrum into the workspace;] one kernel writes the
 * magnitude slots S' = weight[k] gS[k] / |X[k]| in the layout the plan's Griffin-Lim frame launch reads (slot order with its doubled
 * 440 bins on the specialised engine, position = bin on the generic and chirp-z engines, the row family's own order) - for
 * rfx_stft_backward the one-sided weights alone; the engine's existing first Griffin-Lim launch (MODE 0, per-frame form) synthesises
 * S' times the spectrum itself (or the caller's gradient) frame by frame; the fold kernel gathers step 4 per output sample.  All
 * four frame engines.  Range: S' = gS / |X| must be representable, i.e. |g| / |X| below 3e38 (|X| == 0 is served exactly).
 * Contract of the three entries: B == 0 is a no-op.  Refusals - Lw <= n_fft / 2, a NULL pointer, a workspace or complex gradient
 * that is not 16-byte aligned, a float tensor that is not 4-byte aligned, a workspace below the query - come before any launch and
 * leave the output untouched.  Row and element offsets are 64-bit.  Deterministic, and a row's bytes depend on that row alone: every
 * kernel works frame by frame or sample by sample, whatever B is and wherever the row's group falls.  BOUNDED WORKSPACE: the rows
 * are walked in groups of max(1, 256 MiB / row bytes) whole rows, row bytes = T * (frame_stride * 8 [fused call only] + slot stride * 4 +
 * frame pitch * 4) - 67 MB for a 512-frame row at the default geometry - so a query answers at most 256 MiB + 768 bytes, or one
 * row's bytes when a row alone is larger; it answers 0 where the call would be refused.  The loop forms of these three have no backward: the loop STFT has one
 * through the loss entries only (rfx_spectral_loss_backward_loop, "FUSED SPECTRAL LOSSES" below).
 *
 * rfx_stft_backward: steps 3 and 4.  d_grad_spec_slots: the complex gradient in slot layout - what rfx_pack_complex writes,
 * conjugate slots conjugated, both slots of a doubled bin filled - B * T frames; d_grad_wave (B, Lw) float32.
 * rfx_mel_scale_backward: step 1 alone, d_grad_mel (B, n_mels, T) -> d_grad_lin_bft in the reference's (B, n_stft, T) layout.  Its
 * workspace query answers 0 and d_workspace may be NULL.
 * rfx_mel_from_waveform_backward: the fused call, steps 1 to 4.  It re-analyses d_wave (B, Lw) - the caller saves the waveform only:
 * at 64 stereo tiles a kept spectrum would be 2.3 GB - and never writes the (B, n_stft, T) tensor. */
size_t rfx_stft_backward_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_stft_backward(const rfx_plan* plan, const void* d_grad_spec_slots, int B, int Lw, float* d_grad_wave, void* d_workspace,
                      size_t workspace_bytes, void* stream);
size_t rfx_mel_scale_backward_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_mel_scale_backward(const rfx_plan* plan, const float* d_grad_mel, int B, int T, float* d_grad_lin_bft, void* d_workspace,
                           size_t workspace_bytes, void* stream);
size_t rfx_mel_from_waveform_backward_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_mel_from_waveform_backward(const rfx_plan* plan, const float* d_wave, const float* d_grad_mel, int B, int Lw,
                                   float* d_grad_wave, void* d_workspace, size_t workspace_bytes, void* stream);
/* the per-bin adjoint table plan creation builds from a dense filterbank h_melfb [n_stft][n_mels] and uploads with the plan, without
 * a GPU (tests): for bin k the first band with a non-zero weight h_first[k], the number of bands up to the last non-zero one
 * h_count[k] (0: no band reaches the bin; 2 for a triangular bank, but taken from the bank) and their weights
 * h_weights[k * capacity + i], zero past the count.  *width_out receives the largest count (at least 1); the three tables are
 * nullable (a first call learns the width); a capacity below the width is refused. */
int rfx_debug_mel_adjoint(const rfx_params* params, const float* h_melfb, int32_t* h_first, int32_t* h_count, float* h_weights,
                          int capacity, int32_t* width_out);

/* ---- FUSED SPECTRAL LOSSES with device gradients: spectral convergence and log-magnitude L1 of the multi-resolution STFT loss ---------
 * Per row b of a (B, Lw) float32 waveform: T = rfx_stft_frames(Lw) (loop forms: Lw = hop T exactly, under the loop encode's length
 * rule, T = rfx_stft_loop_frames(Lw)); X the row's complex STFT as rfx_stft (loop: rfx_stft_loop) computes it; a = |X| what that entry
 * writes as magnitudes; m the target in slot layout, what rfx_pack_magnitudes writes; n = n_stft T bins, each counted once (the
 * counting rule of rfx_spectral_error); f = log_floor.
 * Forward, three double sums per row, d_sums_out (B, 3):
 *   num = sum (a - m)^2        den = sum m^2        lsum = sum | ln max(a, f) - ln max(m, f) |
 * num and den are bit for bit rfx_spectral_error's wherever that entry takes the shape: the same chunks, per-thread order and halving
 * tree.  lsum rides the same tree, each term formed in double from the two float32 values.  log_floor == 0 means "no log term": lsum is
 * 0 and no logarithm is evaluated.  A negative or non-finite floor, or 0 < f < 1e-18, is refused: 1 / f^2 must fit float32 in the
 * backward.  The caller forms the losses from the sums: convergence = sqrt(num / den), log_magnitude = lsum / n.
 * Backward.  With (g_sc, g_lg) the incoming gradients of the two losses of a row, d_coef (B, 2) float32 holds
 *   c_sc = g_sc / sqrt(num den) when num > 0 and den > 0, else 0 (the zero subgradient of the norm; a silent target gets no gradient)
 *   c_lg = g_lg / n
 * (the Python layer computes them with torch operations on the device: nothing is read back) and
 *   dL/da = c_sc (a - m) + c_lg sgn(ln max(a, f) - ln max(m, f)) [a >= f] / a        sgn(0) = 0; a == f passes (torch.clamp)
 * followed by steps 2, 3 and 4 above: torch.abs's backward with its zero rule (a == 0 gives exactly 0), the frame adjoint and the
 * adjoint fold.  For a loop row step 4 is the circular chain of the loop decode's fold: with q = j + h - left, sample j sums
 * w[q - hop t] f_(t mod T)[q - hop t] over the unwrapped covering frames t = ceil((q - win_length + 1) / hop) .. floor(q / hop),
 * oldest first - no envelope, no reflect partners; rolling the waveform and the target's columns by k hops rolls the gradient by
 * k hop samples bit for bit.  The target receives no gradient.  These entries are the loop STFT's only backward: the loop forms of
 * the forward entries above have none.
 * On the device, per group of rows.  Forward: the plan's forward transform into the workspace, then rfx_spectral_error's reduction
 * carrying the third sum (groups of 128 MiB of magnitudes).  Backward: rfx_mel_from_waveform_backward's sequence - re-analysis, one
 * kernel writing the magnitude slots S' = weight[k] (dL/da) / a, each from the magnitude of the very complex value it will multiply
 * (a = sqrtf(fmaf(re, re, im im)), the forward entries' own expression: the sign and a >= f are decided on the value the sums saw),
 * the engine's MODE 0 frame launch on S' X, the fold kernel (the circular one for loop rows) - in groups of 256 MiB, the fused
 * backward's row bytes.  All four frame engines, loop forms included (the chirp-z engine refuses a loop decode; its frame launch and
 * its loop forward transform exist).  The (B, n_stft, T) tensor is never written.
 * Contract: B == 0 is a no-op.  Refusals - a NULL pointer; d_mag_slots or the workspace not 16-byte aligned, d_sums_out not 8-byte,
 * another tensor not 4-byte aligned; Lw <= n_fft / 2; for a loop form a length that is no whole period (the message names the nearest
 * legal lengths); a bad floor; a workspace below the query - come before any launch and leave the output untouched; a size query
 * answers 0 where the call would refuse.  Offsets are 64-bit.  Deterministic; a row's bytes depend on that row alone. */
size_t rfx_spectral_loss_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_spectral_loss(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int Lw, float log_floor,
                      double* d_sums_out /* (B, 3) */, void* d_workspace, size_t workspace_bytes, void* stream);
size_t rfx_spectral_loss_loop_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_spectral_loss_loop(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, int B, int Lw, float log_floor,
                           double* d_sums_out /* (B, 3) */, void* d_workspace, size_t workspace_bytes, void* stream);
size_t rfx_spectral_loss_backward_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_spectral_loss_backward(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots, const float* d_coef /* (B, 2) */,
                               int B, int Lw, float log_floor, float* d_grad_wave, void* d_workspace, size_t workspace_bytes,
                               void* stream);
size_t rfx_spectral_loss_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int Lw);
int rfx_spectral_loss_backward_loop(const rfx_plan* plan, const float* d_wave, const float* d_mag_slots,
                                    const float* d_coef /* (B, 2) */, int B, int Lw, float log_floor, float* d_grad_wave,
                                    void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- INVERSE SPECTROGRAM: complex STFT -> audio (torchaudio.transforms.InverseSpectrogram), with its gradient -------------------------
 * With h = n_fft / 2, N = n_fft, w the window zero-padded to N, X (B, n_stft, T) complex64 in slot layout (what rfx_pack_complex and
 * rfx_stft write):
 *   PLAIN   y = torch.istft(X, n_fft, hop, win_length, window, center=True, normalized=False, onesided=True), L =
 *           rfx_griffinlim_output_samples(plan, T) samples per row.  It is the final synthesis of Griffin-Lim: per frame the N-point
 *           c2r transform (it ignores the imaginary part of bin 0 and of the Nyquist bin of an even N), times w, overlap-added as
 *           the engine's fold chains it, divided by the envelope env[p] = sum_t w^2[p - hop t] and trimmed by h.  The window must meet
 *           torch.istft's own condition: env non-zero over the L samples.
 *   LOOP    the circular synthesis of a loop decode (rfx_loop_call_options): frames and positions modulo the period hop T, hop T
 *           samples per row, the hop-entry circular envelope.  Needs hop T >= n_fft; a chirp-z plan answers RFX_ERR_UNSUPPORTED.
 * The entries do NOT split X into magnitudes and angles: the engine's first Griffin-Lim launch (MODE 0, per-frame form) runs on unit
 * magnitude slots and takes X itself where a decode injects its start angles, then the engine's fold writes the caller's rows.  So a
 * result need not equal rfx_griffinlim's at n_iter = 0 on (|X|, X / |X|) bit for bit - that route rounds |X| (X / |X|) - and is held to
 * the parity rule instead: its error against float64 torch.istft is within 6 dB of float32 torch.istft's own.  RANGE: the map is
 * linear, no range table is drawn and nothing is squared, so a result is X's scaled by the same power of two as long as
 * n_stft max|X| stays below 2^127 and the samples above the subnormals (the tests hold X 2^+-40).  Non-finite input gives non-finite
 * output in the rows that hold it.
 *   BACKWARD  for an incoming g (B, L) float32 the gradient with respect to X, in torch's convention dL/dRe + i dL/dIm, is
 *           G[k][t] = (c_k / N) sum_i w[i] u[hop t + i - h] e^(-2 pi i k i / N)
 *           u[q] = g[q] / env[q + h] for 0 <= q < L and 0 outside - zero extension, not reflection; c_k = 1 for bin 0 and for the
 *           Nyquist bin of an even N, else 2; the imaginary part of G is exactly 0 in the bins with c_k = 1.  Loop form:
 *           u[q] = g[q] renv[q mod hop], the sample index modulo hop T - the circular analysis of rfx_stft_loop as it is.
 * On the device, per group of rows, the backward stages u (one kernel, 16-byte stores: the envelope table of the engine's fold
 * applied), runs the plan's forward frame transform on it under a third index rule beside reflect and wrap - the ZERO-EXTENSION twin of
 * each engine's forward kernel, the same kernel text with a position outside [0, L) contributing an exact 0.0f; the loop form runs the
 * circular transform of rfx_stft_loop as it is - and one epilogue kernel applies c_k / N and the zero-imaginary rule while it writes
 * gradient slots in rfx_pack_complex's layout: conjugate slots conjugated, both slots of a doubled bin filled, padding 0.  All four
 * frame engines (the chirp-z engine for the plain forms).  The twin's exact test is rfx_debug_istft_backward_padded below: the
 * plain backward with u padded with zeros to the period P' = hop ceil((L + n_fft) / hop) and the circular transform in the twin's
 * place gives the same bits (it computes about n_fft / hop frames per row for nothing).
 * Contract of the four entries: B == 0 is a no-op.  Refusals - a NULL pointer; a spectrum, gradient-slot or workspace pointer that is
 * not 16-byte aligned, a float tensor that is not 4-byte aligned; a T the form cannot serve (plain: no sample; loop: hop T < n_fft,
 * the message names the fewest frames); a loop form on a chirp-z plan (RFX_ERR_UNSUPPORTED); a workspace below the query - come before
 * any launch and leave the outputs untouched; a query answers 0 where the call would be refused.  Offsets are 64-bit.  BOUNDED
 * WORKSPACE: rows are walked in groups of max(1, 256 MiB / row bytes) whole rows (at most 65535).  Deterministic, and a row's bytes
 * depend on that row alone.
 * d_spec_slots / d_grad_spec_slots: B * T frames of slots; d_wave_out / d_grad_wave: (B, L) float32, L the form's samples. */
size_t rfx_istft_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_istft(const rfx_plan* plan, const void* d_spec_slots, int B, int T, float* d_wave_out, void* d_workspace, size_t workspace_bytes,
              void* stream);
size_t rfx_istft_loop_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_istft_loop(const rfx_plan* plan, const void* d_spec_slots, int B, int T, float* d_wave_out, void* d_workspace,
                   size_t workspace_bytes, void* stream);
size_t rfx_istft_backward_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_istft_backward(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots, void* d_workspace,
                       size_t workspace_bytes, void* stream);
size_t rfx_istft_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_istft_backward_loop(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots, void* d_workspace,
                            size_t workspace_bytes, void* stream);
/* rfx_istft_backward by the padded circular route (tests): same arguments, same contract, a larger workspace, the same bytes */
size_t rfx_debug_istft_backward_padded_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_debug_istft_backward_padded(const rfx_plan* plan, const float* d_grad_wave, int B, int T, void* d_grad_spec_slots,
                                    void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- TIME STRETCH: the phase vocoder between rfx_stft and rfx_istft (torchaudio.transforms.TimeStretch) ----------------------------------
 * rfx_phase_vocoder is torchaudio.functional.phase_vocoder(X, rate, phase_advance = linspace(0, pi hop_length, n_stft)) on a complex
 * spectrogram in slot layout (what rfx_pack_complex and rfx_stft write): B * T frames in, B * T_out frames out, the same layout - both
 * slots of a doubled bin filled with one trajectory, conjugate slots conjugated, padding 0 - so the result goes to rfx_istft as it is.
 *   T_out   = ceil(T / rate) evaluated in double, the length of torch.arange(0, T, rate): rfx_phase_vocoder_frames (host only).
 *   step i  reads frames i0 = floor(i rate) and i0 + 1, i rate formed in double, alpha = (float)(i rate - i0); frames at or past T are 0.
 *   output  magnitude alpha |X[i0 + 1]| + (1 - alpha) |X[i0]|; phase angle(X[0]) at step 0, then the running sum of
 *           wrap(angle(X[i0 + 1]) - angle(X[i0]) - adv_k) + adv_k.
 * STEP POSITIONS ARE THE DOUBLE PRODUCTS (double)i * rate, one rounding each, the same on every machine.  torchaudio takes them from
 * torch.arange(0, T, rate) in the spectrogram's real dtype, whose value for step i is not that product: where i rate lies within
 * rounding of an integer arange can choose the neighbouring frame pair - the same magnitude to rounding, another phase trajectory
 * from that step on.  Of the 495 reduced fractions p/q in [0.25, 4] with q <= 24, p <= 48 at T = 512 the float64 CPU arange does so
 * at 168 rates (2/3, 4/3, 0.3 and 1.2 among them) and the float32 CPU arange at 46 (tools/survey_vocoder_steps.py,
 * profiles/time_stretch_steps.txt); tests/vocoder_oracle.py, the reference of every gate, takes the products.
 * PHASES ARE TURNS: adv_k = (hop k mod D) / D with D = 2 (n_stft - 1) in integers, the accumulator wrapped to [-1/2, 1/2] after every
 * step, sine and cosine taken of the wrapped turns.  Float32 torch sums the absolute phase - up to pi hop radians per frame - and loses
 * about a bit per doubling of T; this form does not (tests/test_vocoder_cpu.py holds it ABOVE float32 torch at T = 512).
 * rate == 1.0 copies the input bit for bit, as torchaudio returns it.  One rate per call.  No gradient and no loop form: the
 * accumulated phase does not close over a period.
 * One kernel, one thread per slot position, rows on the grid's second axis, a serial walk over the T_out frames (rfx_vocoder.hip).
 * rfx_time_stretch is, per group of rows, exactly rfx_stft -> rfx_phase_vocoder -> rfx_istft: d_wave (B, Lw) float32 -> d_wave_out
 * (B, rfx_time_stretch_samples(plan, Lw, rate)) float32, hop (T_out - 1) (+ n_fft % 2) samples per row with T = rfx_stft_frames(plan, Lw)
 * - the same bytes as the three calls on all rows at once.  BOUNDED WORKSPACE: groups of max(1, 256 MiB / bytes of a row's two
 * spectrograms) whole rows (at most 65535), plus what rfx_istft asks for a group.
 * Contract: B == 0 is a no-op.  RFX_ERR_INVALID with a message, before any launch, the outputs untouched: a NULL pointer; a rate that
 * is not finite or not positive; T < 1; a frame count past 2^31 - 1; slots off 8-byte alignment or d_out_slots == d_spec_slots; for
 * rfx_time_stretch what rfx_stft refuses for Lw (Lw <= n_fft / 2) and rfx_istft for T_out (no sample), a workspace off 16-byte or a
 * waveform off 4-byte alignment.  RFX_ERR_WORKSPACE: a workspace below the query.  A query answers 0 where the call would be refused. */
int rfx_phase_vocoder_frames(int T, double rate, int* T_out);
int rfx_phase_vocoder(const rfx_plan* plan, const void* d_spec_slots, int B, int T, double rate, void* d_out_slots, void* stream);
size_t rfx_time_stretch_workspace_bytes(const rfx_plan* plan, int B, int Lw, double rate);
int rfx_time_stretch_samples(const rfx_plan* plan, int Lw, double rate);
int rfx_time_stretch(const rfx_plan* plan, const float* d_wave, int B, int Lw, double rate, float* d_wave_out, void* d_workspace,
                     size_t workspace_bytes, void* stream);
/* The kernel's position table, without a plan or a GPU (tests; options NULL = defaults): per position of a frame of complex slots
 * h_bin the bin it holds (-1: padding), h_src the PRIMARY position of that bin - the one rfx_unpack_complex reads; -1: padding -,
 * h_advance the bin's advance in turns, frac(hop k / D), negated where the position holds the conjugate, h_conj 1 where it does.
 * *stride_out: positions per frame; the arrays are optional and need capacity >= *stride_out. */
int rfx_debug_vocoder_table(const rfx_params* params, const rfx_plan_options* options, int32_t* h_bin, int32_t* h_src, float* h_advance,
                            uint8_t* h_conj, int capacity, int32_t* stride_out);

/* ---- SINC RESAMPLE: torchaudio.functional.resample, band-limited, float32 (torchaudio.transforms.Resample) --------------------------------
 * resample(waveform, orig, new, lowpass_filter_width = lpw, rolloff, resampling_method = "sinc_interp_hann") on rows of float32
 * samples.  With g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lpw o / base):
 *   length  L samples in, K = ceil(n L / o) samples out, exact in integers: rfx_resample_sinc_frames (host only).  (torchaudio rounds
 *           the quotient to float32 before the ceil; the two agree below 2^24 samples.)
 *   output  j = q n + p, 0 <= p < n, is the sum over i of x[q o + i - width] k_p[i], x zero outside [0, L), with
 *           k_p[i] = sinc(pi t) cos^2(pi t / (2 lpw)) base / o,  t = clamp((-p / n + (i - width) / o) base, -lpw, lpw).
 * DROPPED TAPS: torchaudio's dense kernel has 2 width + o taps per phase; at all but about 2 lpw o / base + 1 of them (13 to 25) the
 * clamp holds t at +-lpw, where the window is cos^2(pi / 2) - 4e-33 in float64, not 0.  This library drops the taps with
 * |t| >= lpw: a difference below 1e-30 of a sample per tap.
 * Only the Hann window is stated; there is no entry for torchaudio's "sinc_interp_kaiser".
 * THE TABLE (rfx_resample_sinc_table, host only, no GPU; as rfx_image_resize_coefficients: the host computes, the caller uploads):
 * h_first[p], p < n, the offset from q o of the first tap phase p keeps (negative at a row's start); h_taps[k n + p], k < ntaps, the
 * weights TAP-MAJOR, computed in double and rounded once to float32 - the kernel torchaudio.transforms.Resample holds -, ntaps the
 * longest run over the phases, shorter phases filled with 0.  `capacity` counts the floats of h_taps; h_first needs n entries.  With
 * both arrays NULL the call answers *n_out and *ntaps_out alone.  RFX_ERR_UNSUPPORTED with a message where the table, 4 n ntaps
 * bytes, would pass RFX_RESAMPLE_MAX_TABLE_BYTES: every integer semitone shift within +-12 at 8 to 96 kHz stays below 8.5 MiB.
 * rfx_resample_sinc: d_in (B, L) float32 -> d_out (B, K) float32 on the device that owns d_out, d_first / d_taps the uploaded table of
 * (orig, new).  One kernel (rfx_resample.hip): one thread per output sample and block of 4 rows, the taps accumulated in ascending
 * order with one fmaf each; sample indices are 64-bit.  orig == new copies the input, as torchaudio returns it (the table is not read).
 * Contract: B == 0 is a no-op.  RFX_ERR_INVALID with a message, before any launch, the outputs untouched: a NULL pointer; a
 * frequency that is not positive; L < 1; K past 2^31 - 1; ntaps < 1; a pointer off 4-byte alignment; d_in and d_out overlapping;
 * for the table a lowpass_filter_width < 1, a rolloff outside (0, 1], one array without the other or a capacity below n ntaps.  The
 * kernel tests every index it forms from the table against the row, so a table of another pair gives wrong samples, not a fault. */
#define RFX_RESAMPLE_MAX_TABLE_BYTES (16 << 20)
int rfx_resample_sinc_frames(int L, int orig_freq, int new_freq, int* K);
int rfx_resample_sinc_table(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int32_t* h_first, float* h_taps,
                            int64_t capacity, int32_t* n_out, int32_t* ntaps_out);
int rfx_resample_sinc(const float* d_in, int B, int L, int orig_freq, int new_freq, const int32_t* d_first, const float* d_taps, int ntaps,
                      float* d_out, void* stream);

/* ---- PITCH SHIFT: the time stretch, then the resampler back to the duration (torchaudio.transforms.PitchShift) ----------------------------
 * rfx_pitch_shift is torchaudio.functional.pitch_shift(waveform, sample_rate, n_steps, bins_per_octave) at the plan's STFT parameters
 * and sample rate: d_wave (B, Lw) float32 -> d_wave_out (B, Lw) float32, the key moved by n_steps / bins_per_octave octaves at the
 * same tempo.  Per group of rows it is exactly
 *   1. rfx_time_stretch at rate = 2^(-n_steps / bins_per_octave), Ls samples per row;
 *   2. cut, or pad with zeros, to len_stretch = round(Lw / rate) (ties to even, as Python rounds);
 *   3. rfx_resample_sinc from orig = int(sample_rate / rate) (rfx_pitch_shift_resample_freq, host only) to sample_rate, with the
 *      caller's table of that pair at lowpass_filter_width 6, rolloff 0.99;
 *   4. cut, or pad with zeros, to Lw
 * - the same bytes as the separate calls on all rows at once.  Steps 2 and 4 make no pass of their own: the resampler reads zeros
 * past min(Ls, len_stretch) and stores min(K, Lw) samples.  n_steps == 0 copies the input (no workspace, no table).  A shift so small
 * that orig == sample_rate runs steps 1, 2 and 4 and does not read the table.
 * ONE DEPARTURE: where len_stretch exceeds Ls = hop (T_out - 1) (+ n_fft % 2) - by less than one hop - torch.istft(length =
 * len_stretch) keeps len_stretch - Ls samples of its untrimmed tail; this library pads zeros there, as rfx_istft's callers do
 * everywhere else.  With o / n the reduced pair of step 3 and base = min(o, n) 0.99, the samples this can reach are the outputs
 * j >= floor((Ls - 6 o / base) n / o): the last ceil((len_stretch - Ls) n / o + 6 n / base) + 1 of the K, less what step 4 cuts.
 * BOUNDED WORKSPACE (rfx_pitch_shift_workspace_bytes): the stretched rows of a group, plus what rfx_time_stretch asks for the group;
 * the groups are rfx_time_stretch's own.  No gradient, no loop form, one shift per call.
 * Contract: B == 0 is a no-op.  RFX_ERR_INVALID with a message, before any launch, the output untouched: a NULL pointer; n_steps
 * not finite; bins_per_octave < 1; what rfx_time_stretch refuses for Lw at the rate; len_stretch, orig or K past 2^31 - 1; what
 * rfx_resample_sinc refuses of the table; a workspace off 16-byte or a waveform off 4-byte alignment; d_wave and d_wave_out
 * overlapping.  RFX_ERR_UNSUPPORTED: a table past RFX_RESAMPLE_MAX_TABLE_BYTES.  RFX_ERR_WORKSPACE: a workspace below the query.
 * A query answers 0 where the call would be refused, and for n_steps == 0. */
size_t rfx_pitch_shift_workspace_bytes(const rfx_plan* plan, int B, int Lw, double n_steps, int bins_per_octave);
int rfx_pitch_shift_resample_freq(const rfx_plan* plan, int Lw, double n_steps, int bins_per_octave);
int rfx_pitch_shift(const rfx_plan* plan, const float* d_wave, int B, int Lw, double n_steps, int bins_per_octave, const int32_t* d_first,
                    const float* d_taps, int ntaps, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- inverse: torchaudio.transforms.InverseMelScale (SGD, max_iter = params.max_mel_iters,
 * tolerance_loss 1e-5, tolerance_change 1e-8, lr 0.1, momentum 0.9), spectrogram_converter.py:87-99,
 * called at :201.  d_mel (B, n_mels, T); the B rows are grouped into clips of `channels_per_clip`
 * consecutive rows, each clip being one call of the reference (its loss mean couples the clip's
 * channels and frames).  d_spec0: optional injected start (B, T, n_stft) float32 in the reference's
 * own layout, NULL = U[0,1) from `seed`.  Output: linear magnitudes in slot layout, ready for
 * rfx_griffinlim. */
/* which SGD kernel rfx_inverse_mel runs for this plan's filterbank: 4 = wave kernel (one wave per frame, weights as a line per
 * group: the default 512-filter HTK bank, with or without slaney normalisation), 2 = group kernel with per-wave register budgets sized to
 * the default 512-filter HTK bank (with or without slaney normalisation), 3 = the same kernel with the wider budget set
 * (mel_scale_type "slaney"), 5 = line-form group kernel (round 5: banks with groups of up to 62 bins whose long groups are lines -
 * 512 filters up to the Nyquist frequency, e.g. the 20 Hz .. 20 kHz of the reference's test/spectrogram_converter_test.py:46-53,
 * or 256 / 384 filters over 0 - 10 kHz), 1 = group kernel with a uniform budget (other banks whose groups fit 8 / 24 bins),
 * 0 = general LDS kernel (any banded bank), -1 = not banded (rfx_inverse_mel refuses) */
int rfx_plan_imel_kernel(const rfx_plan* plan);
/* 1 when that kernel (2, 3, 4 or 5) computes a bin's gradient in unit form, d1 + (d0 - d1) w0: valid when the two weights of every
 * bin of the long groups sum to one, i.e. triangular filters without area normalisation (mel_scale_norm None); 0 = both
 * weights are multiplied out (mel_scale_norm "slaney", other kernels) */
int rfx_plan_imel_unit_form(const rfx_plan* plan);
size_t rfx_inverse_mel_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_inverse_mel(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                    uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream);

int rfx_inverse_mel_ex(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, const float* d_spec0,
                       uint64_t seed, float* d_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream,
                       const rfx_call_options* options);

/* ---- inverse, closed form: torchaudio >= 2.1's InverseMelScale, relu(torch.linalg.lstsq(fb.T[None], mel, driver="gels").solution)
 * - the minimum-norm least-squares solution, clamped at zero.  Opt-in: rfx_inverse_mel above stays the default.
 * For a bank whose bins feed at most two adjacent filters G = fb^T fb is symmetric tridiagonal and the answer is
 * x = relu(fb G^-1 mel): per frame one n_mels-unknown tridiagonal solve (L D L^T factored in double at plan creation, the two
 * sweeps in float32, one fmaf per step in a fixed order) and a two-tap expansion, max(0, fmaf(w1, y[m0 + 1], w0 * y[m0])).
 * rfx_plan_lstsq_ok: 1 when the plan's bank admits it (rfx_debug_lstsq_bank says why not, without a GPU); on any other plan the
 * entry returns RFX_ERR_INVALID with that reason.
 * d_mel (B, n_mels, T) -> d_mag_slots: linear magnitudes in slot layout, ready for rfx_griffinlim, every position of every frame
 * written: padding positions and the bins no filter reaches are exactly 0.0 (the minimum-norm answer), both copies of a bin the
 * specialised layout stores twice are equal.  No seed, no channels_per_clip, no start: a frame's result is a function of that
 * frame's mel column and the plan alone - not of B, the row, the batch it travels in or the launch grid.
 * What differs from the SGD by construction: the bins outside the bank are zeros where the SGD leaves its U[0,1) start, and
 * nothing couples a clip's channels and frames (the SGD's stopping rule reads a loss mean over the whole clip).
 * Held against torch's float64 lstsq at no more than twice the distance of torch's own float32 "gels" (measured: 6e-8 against
 * 1.4e-7 relative L2).  Scale: every step is linear, so an input times 2^n gives the output times 2^n bit for bit while no
 * intermediate leaves float32's normal range - magnitudes between about 1e-30 and 1e30 for the reference's banks.
 * d_mag_slots must be 16-byte aligned.  Row and element offsets are 64-bit.  Workspace: B * n_mels * T floats. */
int rfx_plan_lstsq_ok(const rfx_plan* plan);
size_t rfx_inverse_mel_lstsq_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_inverse_mel_lstsq(const rfx_plan* plan, const float* d_mel, int B, int T, float* d_mag_slots, void* d_workspace,
                          size_t workspace_bytes, void* stream);

/* Its backward, as torch autograd differentiates relu(lstsq(...).solution) with respect to mel: for a gradient gx over the linear
 * bins, g_mel = G^-1 c with c = fb^T (gx where the relu is open) - G is symmetric, so the solve is the forward's on another
 * right-hand side, same tables, same sweeps.  The gradient is 0 where the forward's value before the clamp is <= 0 (torch.relu's
 * rule; the forward's `v > 0 ? v : 0` has it too).  The mask is not saved: the entry takes the forward's d_mel, runs the solve again
 * into its workspace and forms the value before the clamp with the forward's own expression, so the mask is the forward's x > 0 bit
 * for bit and a caller keeps (B, n_mels, T), not the slots.
 * d_mel (B, n_mels, T), d_grad_slots [B * T][frame stride] -> d_grad_mel (B, n_mels, T).  d_grad_slots is what rfx_pack_magnitudes
 * of torch's (B, n_stft, T) gradient holds.  EVERY BIN COUNTS ONCE: a bin the specialised layout stores twice is read from its first
 * slot only (the one rfx_debug_lstsq_collect reports); the second slot, the padding positions and the bins no filter reaches are
 * never read, whatever they hold.  c[m] sums filter m's bins in ascending bin order, one fmaf per bin, from 0 - no atomics; a frame's
 * result is a function of that frame's mel column, its gradient and the plan alone, not of B, the row or the launch grid.
 * Scale: linear in the gradient with power-of-two-exact roundings - d_grad_slots times 2^n gives d_grad_mel times 2^n bit for bit
 * while no intermediate leaves float32's normal range.
 * Refusals are the forward's: a null argument, a plan that is not rfx_plan_lstsq_ok (RFX_ERR_INVALID with the reason; the query
 * returns 0), a bad shape, more than 2^31 - 1 frames, d_grad_slots not 16-byte aligned, a workspace that is too small
 * (RFX_ERR_WORKSPACE).  Workspace: 2 * B * n_mels * T floats.  Inputs are not written. */
size_t rfx_inverse_mel_lstsq_backward_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_inverse_mel_lstsq_backward(const rfx_plan* plan, const float* d_mel, const float* d_grad_slots, int B, int T, float* d_grad_mel,
                                   void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- GUIDED DECODE, BACKWARD: the gradient of the zero-iteration phase-guided decode -------------------------------------------------
 * A guided call (rfx_guided_call_options) with n_iter = 0 returns w = ISTFT(S u), u = a / (|a| + 1e-16) the unit phase of
 * a = STFT(staged guide): linear in the magnitudes S, the guide a constant.  For an incoming g_w (B, L) float32, L the form's samples:
 *     G   = rfx_istft_backward(g_w)  (loop: rfx_istft_backward_loop)         the synthesis adjoint, gradient slots
 *     g_S = Re(conj(u) G) = u_re G_re + u_im G_im  per slot position         rfx_griffinlim_guided_backward: the STAGE entry
 *     g_mel = rfx_inverse_mel_lstsq_backward(mel, g_S)                       rfx_waveform_from_mel_guided_backward: the FUSED entry
 * The stage entry is the gradient of rfx_griffinlim_ex (guided, n_iter = 0) with respect to d_mag_slots; the fused entry that of
 * rfx_waveform_from_mel_ex (RFX_CALL_INVERSE_MEL_LSTSQ, guided, n_iter = 0) with respect to d_mel, and is the stage entry followed by
 * rfx_inverse_mel_lstsq_backward in one workspace - the same bytes.  Nothing but mel and the guide has to be kept from the forward:
 * the guide is analysed again, as rfx_mel_from_waveform_backward forms its spectrum again.
 *   THE GUIDE  d_guide (B, guide_samples) float32, contiguous rows, is staged as the forward stages it: cut to L samples or
 *     zero-padded at its end to L (loop: L = hop T), times the power of two that brings the row's peak into [2^14, 2^15) - a shorter
 *     guide equals the same guide zero-padded by the caller, guide * 2^m gives the same bytes - then transformed by the plan's forward
 *     frame kernel (rfx_stft: reflect padding; loop: rfx_stft_loop).  u is the forward's projection rule in IEEE operations (fmaf,
 *     sqrt, divide: a host emulator gives the device's bits); the forward's launch forms the same factor with one v_rsq_f32, 1 ulp
 *     from it, and its epsilon is the same 1e-16 expressed in the units of the row's range factor.  a == 0 gives u = 0 in both: a
 *     silent bin passes no gradient, a silent guide row gives a zero gradient row.  No gradient flows to the guide.
 *   RANGE  the forward's power-of-two range factors (row_scale) cancel inside the forward and never enter its derivative; the backward
 *     draws no range table and squares nothing of g_w, so g_w * 2^k gives g_S * 2^k and g_mel * 2^k bit for bit while no intermediate
 *     leaves float32's normal range (the tests hold 2^+-40).
 *   THE PROJECTION KERNEL  (rfx_guide_bwd.hip) reads G and a, two complex cubes in rfx_pack_complex's layout, 16 bytes per lane, and
 *     writes g_S in rfx_pack_magnitudes' layout, 16 bytes per lane: EVERY float of every frame is written - padding positions 0, both
 *     slots of a bin the specialised layout holds twice (each from the complex pair that slot multiplied), the bins no filter reaches -
 *     although rfx_inverse_mel_lstsq_backward reads only the counted copy of a bin.  No atomics; a frame's bytes are a function of that
 *     frame alone, not of B, the row's place or the grid.  It is bound by memory: 20 bytes per position.
 * d_grad_mag_slots: [B * T][frame stride] float32.  d_mel, d_grad_mel: (B, n_mels, T).
 * Contract: B == 0 is a no-op.  Refusals, all before any launch, outputs untouched: a NULL pointer; T < 2; B * T >= 2^31;
 * guide_samples <= 0; the plain form where the L samples of T frames are not more than the reflect padding n_fft / 2 (the forward
 * refuses such a guide); a loop form with hop T < n_fft, or on a chirp-z plan (RFX_ERR_UNSUPPORTED); the fused entries on a plan that
 * is not rfx_plan_lstsq_ok (RFX_ERR_INVALID with the reason); d_workspace or d_grad_mag_slots not 16-byte aligned, a float tensor not
 * 4-byte aligned; a workspace below the query (RFX_ERR_WORKSPACE).  A query answers 0 where the call would be refused.  BOUNDED
 * WORKSPACE of the stage entry: rows are walked in groups of max(1, 256 MiB / row bytes) whole rows; the fused entry holds g_S of all
 * B rows in front of it.  Inputs are not written. */
size_t rfx_griffinlim_guided_backward_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_griffinlim_guided_backward(const rfx_plan* plan, const float* d_guide, int guide_samples, const float* d_grad_wave, int B, int T,
                                   float* d_grad_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream);
size_t rfx_griffinlim_guided_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_griffinlim_guided_backward_loop(const rfx_plan* plan, const float* d_guide, int guide_samples, const float* d_grad_wave, int B,
                                        int T, float* d_grad_mag_slots, void* d_workspace, size_t workspace_bytes, void* stream);
size_t rfx_waveform_from_mel_guided_backward_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_waveform_from_mel_guided_backward(const rfx_plan* plan, const float* d_mel, const float* d_guide, int guide_samples,
                                          const float* d_grad_wave, int B, int T, float* d_grad_mel, void* d_workspace,
                                          size_t workspace_bytes, void* stream);
size_t rfx_waveform_from_mel_guided_backward_loop_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_waveform_from_mel_guided_backward_loop(const rfx_plan* plan, const float* d_mel, const float* d_guide, int guide_samples,
                                               const float* d_grad_wave, int B, int T, float* d_grad_mel, void* d_workspace,
                                               size_t workspace_bytes, void* stream);
/* The projection kernel's two position tables, without a plan or a GPU (tests): h_xpos_bin[x] the bin complex position x of a frame
 * holds (-1: padding), h_s2x[p] the complex position magnitude slot p goes with (-1: padding).  *stride_out: positions per frame,
 * the same for both; the arrays are optional and need capacity >= *stride_out (call once with NULL arrays to learn it). */
int rfx_debug_guide_project_tables(const rfx_params* params, int32_t* h_xpos_bin, int32_t* h_s2x, int capacity, int32_t* stride_out);

/* ---- inverse, in one call: SpectrogramConverter.waveform_from_mel_amplitudes, spectrogram_converter.py:187-204
 * (`self.inverse_mel_scaler(amplitudes_mel)` :201 then `self.inverse_spectrogram_func(amplitudes_linear)` :204).
 * d_mel (B, n_mels, T) -> d_wave_out (B, rfx_griffinlim_output_samples(plan, T)); clips of `channels_per_clip` rows as in
 * rfx_inverse_mel; both random starts from `seed` (the SGD start from seed, the phases from seed + 1).  Exactly rfx_inverse_mel
 * followed by rfx_griffinlim - same bits - with the linear magnitudes kept inside the workspace. */
size_t rfx_waveform_from_mel_workspace_bytes(const rfx_plan* plan, int B, int T);
int rfx_waveform_from_mel(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                          float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* With RFX_CALL_INVERSE_MEL_LSTSQ in options->flags: exactly rfx_inverse_mel_lstsq followed by rfx_griffinlim_ex with the same
 * options - same bits; the phases still come from seed + 1 and row_base, the Griffin-Lim range from magnitude_hint or the linear
 * magnitudes.  A plan that is not rfx_plan_lstsq_ok is refused (RFX_ERR_INVALID, with the reason) before anything is launched.
 * rfx_audio_from_image_u8_ex reads the flag in the same way.  The workspace queries cover both forms. */
int rfx_waveform_from_mel_ex(const rfx_plan* plan, const float* d_mel, int B, int T, int channels_per_clip, uint64_t seed, int n_iter,
                             float momentum, float* d_wave_out, void* d_workspace, size_t workspace_bytes, void* stream,
                             const rfx_call_options* options);

/* ---- image codec: riffusion/util/image_util.py -----------------------------------------------
 * decode = spectrogram_from_image (:81-108): d_img (N, H, W, 3) uint8 RGB -> (N*C, H, W) float32,
 *   C = 2 (G,B planes) when stereo else 1 (R plane); d_lut256[p] is the float32 value numpy's chain
 *   255-p, /255, **(1/power), *max_value gives for pixel value p (built on the host WITH numpy).
 * encode = image_from_spectrogram (:27-54): d_mel (N*C, M, T) float32 -> d_img_out (N, M, T, 3) uint8;
 *   the per-clip maximum is written to d_clip_max (N floats; it is the EXIF MAX_VALUE of
 *   spectrogram_image_converter.py:59); d_thresholds255[v] = smallest float32 ratio x/max whose
 *   numpy result is <= v (descending, built on the host WITH numpy). */
int rfx_image_decode_u8(const uint8_t* d_img, int N, int H, int W, int stereo, const float* d_lut256, float* d_mel_out,
                        void* stream);
int rfx_image_encode_u8(const float* d_mel, int N, int M, int T, int stereo, const float* d_thresholds255, float* d_clip_max,
                        uint8_t* d_img_out, void* stream);

/* ---- PCM tail: riffusion/util/audio_util.py:22-28.  d_wave (N*C, L) float32 -> d_pcm_out (N, L, C)
 * int16: joint peak normalisation over a clip's channels (when normalize != 0), truncation toward
 * zero.  d_clip_peak (N floats) receives max|x| per clip. */
int rfx_pcm16(const float* d_wave, int N, int C, int L, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* stream);

/* ---- int16 post-processing: riffusion/util/audio_util.py apply_filters and stitch_segments on the device ----------------
 * Both are CPython `audioop` integer arithmetic (mul, add, rms, max on 16-bit samples), reproduced byte for byte.
 *
 * rfx_pcm16_apply_filters: apply_filters(segment, compression=False) - apply_gain(-12 - dBFS), then normalize(headroom=0.1) -
 * on every clip of d_pcm_in (N, L, C) int16 (channels interleaved, as the bytes audioop sees) -> d_pcm_out, same shape; in place
 * when d_pcm_out == d_pcm_in.  d_gain_by_rms and d_boost_by_peak are two tables of 32769 doubles built on the host with
 * pydub's own expressions (audio_util.filter_gain_by_rms / filter_boost_by_peak): the gain factor for each audioop.rms value
 * (entry 0 = inf, dBFS = -inf) and the normalisation factor for each peak after that gain (entry 0 = 1.0).  The device
 * evaluates no pow or log.  Exactness: the result equals audioop's whenever L * C < 2^23 (audioop.rms sums the squares in
 * double, exact up to 2^53); larger clips are refused.  Workspace: rfx_pcm16_filters_workspace_bytes(N, L, C). */
size_t rfx_pcm16_filters_workspace_bytes(int N, int L, int C);
int rfx_pcm16_apply_filters(const int16_t* d_pcm_in, int N, int L, int C, const double* d_gain_by_rms, const double* d_boost_by_peak,
                            int16_t* d_pcm_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* rfx_pcm16_stitch: stitch_segments of the N clips of d_pcm (N, L, C) int16 -> d_out (out_frames, C) int16, as described by
 * the pieces of audio_util.stitch_plan (pydub's millisecond arithmetic of AudioSegment.append, resolved on the host).  Piece k
 * covers output frames [out_start_k, out_start_{k+1}) (the last one up to out_frames); frame out_start + t is source a at
 * frame a_off + t (kind 0), or audioop.add(audioop.mul(a, a_gain), audioop.mul(b, b_gain)) (kind 1); a source is clip
 * a_clip / b_clip of d_pcm, or silence when that index is negative.  h_pieces (host) is checked against N, L and out_frames
 * before anything is launched; d_pieces is the same table in device memory. */
typedef struct {
  int64_t out_start;
  int64_t a_off;
  int64_t b_off;
  double a_gain;
  double b_gain;
  int32_t a_clip;
  int32_t b_clip;
  int32_t kind;
  int32_t reserved;
} rfx_stitch_piece;
int rfx_pcm16_stitch(const int16_t* d_pcm, int N, int L, int C, const rfx_stitch_piece* h_pieces, const rfx_stitch_piece* d_pieces,
                     int n_pieces, int64_t out_frames, int16_t* d_out, void* stream);

/* rfx_pcm16_apply_filters_compressed: apply_filters(segment, compression=True) on every clip of d_pcm_in (N, L, C) int16 ->
 * d_pcm_out (in place when equal): normalize(0.1), apply_gain(-10 - dBFS), pydub 0.25.1 compress_dynamic_range, then exactly
 * rfx_pcm16_apply_filters.  Byte for byte audioop's result, for clips of L * C < 2^23 samples (larger ones are refused):
 *   - the window rms values come from exact int64 prefix sums (audioop's double sums are exact below 2^53);
 *   - the attenuation recurrence takes pydub's steps - one IEEE add or subtract, compares, selects - on the host-built tables
 *     of audio_util.compress_tables (every log is evaluated by the host), so its state is bitwise pydub's in both forms;
 *   - the factor 10^(-att/20) is the device's exp10, which may differ from Python's 10 ** y (libm pow) in its last bits.
 *     Every product x2 * g within `margin` of an integer is flagged (with a factor error of a few ulp, a product of at most
 *     2^15 moves by less than 2^-35: 2^-30 is ample) and recomputed on the host with pow, as CPython's float ** does.
 * The call therefore synchronises `stream` once, to read the flag count (the compression=False entries never do).  When more
 * than flag_capacity samples were flagged, n_flagged says how many and d_pcm_out is left unwritten (d_pcm_in is intact, also
 * in place): redo the batch on the host, or again with a larger list.  Workspace: rfx_pcm16_compress_filters_workspace_bytes. */
typedef enum {
  RFX_COMPRESS_SEQUENTIAL = 0,  /* one lane per clip runs all L steps: the definition */
  RFX_COMPRESS_CHUNKED = 1      /* one lane per chunk of a clip, repair rounds until every chunk starts from its predecessor's
                                   end: the same states, bit for bit */
} rfx_compress_form;
typedef struct {
  uint32_t struct_size;          /* sizeof(rfx_compress_options) */
  int32_t form;                  /* rfx_compress_form */
  int32_t look_frames;           /* int(attack ms * rate / 1000): the rms window */
  int32_t chunk_frames;          /* chunked form: frames per chunk (0 = default); raised until a clip has at most 2048 chunks */
  const double* d_gain10_by_rms; /* audio_util.filter_gain_by_rms(-10) */
  const double* d_gain12_by_rms; /* audio_util.filter_gain_by_rms() */
  const double* d_boost_by_peak; /* audio_util.filter_boost_by_peak(0.1) */
  const uint8_t* d_above;        /* audio_util.compress_tables: above, max_att, inc, dec (32769 entries each) */
  const double* d_max_att;
  const double* d_inc;
  const double* d_dec;
  double margin;                 /* flag products within this distance of an integer (>= 0; 0.5 or more flags every one) */
  void* d_flags;                 /* flag_capacity entries of 24 bytes (device memory) */
  int64_t flag_capacity;
  int32_t* d_rounds;             /* optional (NULL): N ints, the repair rounds each clip took (0 for the sequential form) */
  int64_t n_flagged;             /* out: samples flagged by this call */
} rfx_compress_options;
size_t rfx_pcm16_compress_filters_workspace_bytes(int N, int L, int C);
int rfx_pcm16_apply_filters_compressed(const int16_t* d_pcm_in, int N, int L, int C, rfx_compress_options* options, int16_t* d_pcm_out,
                                       void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- image resize: the bytes of Pillow's Image.resize(size, resample) on RGB uint8 tiles ---------------------------------------
 * The reference's audio-to-audio task widens each clip's tile to a multiple of 32 (scale_image_to_32_stride, BICUBIC), the
 * pipeline's preprocess_image shrinks a tile to a multiple of 32 (LANCZOS), and the task shrinks the pipeline's output back to
 * the clip's size (BICUBIC).  The algorithm is Pillow's 8-bit convolution resample (libImaging/Resample.c): per output column
 * (row) a window of input taps with weights from the filter, normalised in double and rounded to 22 fractional bits; each output
 * byte is clamp((2^21 + sum in * k) >> 22, 0, 255) in int32.  The horizontal pass runs first into a uint8 intermediate, then the
 * vertical pass; a pass whose size does not change is skipped, and equal sizes copy.  The result equals Image.resize byte for
 * byte.  Filters take PIL.Image.Resampling's values; NEAREST, BOX and HAMMING are not implemented.  Sizes are 1 .. 16384.
 *
 * rfx_image_resize_coefficients, host only (no GPU): the table of one axis, in_size -> out_size.  h_bounds receives 2 * out_size
 * ints (first tap, tap count), h_kk out_size * ksize ints (the fixed-point weights; capacity = entries h_kk holds).  Returns
 * ksize; with both pointers NULL it writes nothing and returns ksize.
 * rfx_image_resize_u8: d_in (N, H, W, 3) -> d_out (N, out_h, out_w, 3), both uint8 on one device.  d_bounds_x / d_kk_x are the
 * device copy of the table W -> out_w (may be NULL when out_w == W), d_bounds_y / d_kk_y that of H -> out_h (NULL when
 * out_h == H).  Workspace: rfx_image_resize_workspace_bytes, 0 unless both sizes change (the uint8 intermediate). */
typedef enum {
  RFX_RESIZE_LANCZOS = 1,
  RFX_RESIZE_BILINEAR = 2,
  RFX_RESIZE_BICUBIC = 3
} rfx_resize_filter;
int rfx_image_resize_coefficients(int in_size, int out_size, int filter, int32_t* h_bounds, int32_t* h_kk, int capacity);
size_t rfx_image_resize_workspace_bytes(int N, int H, int W, int out_h, int out_w, int filter);
int rfx_image_resize_u8(const uint8_t* d_in, int N, int H, int W, int out_h, int out_w, int filter, const int32_t* d_bounds_x,
                        const int32_t* d_kk_x, const int32_t* d_bounds_y, const int32_t* d_kk_y, uint8_t* d_out, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* ---- JPEG: the scan of Pillow's Image.save(f, "JPEG", quality=q) of an RGB uint8 tile, on the device -------------------------
 * The reference writes every spectrogram tile as a JPEG (cli.py's image_extension="jpg", server.py).  Pillow's defaults are
 * libjpeg's baseline encoder: YCbCr 4:2:0 (MCUs of 16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr), the Annex K quantisation tables
 * scaled by the quality, the slow integer DCT, the Annex K Huffman tables, no restart markers - integer arithmetic throughout,
 * reproduced byte for byte.  The device writes the entropy-coded scan and EOI; everything before it (SOI, APP0, APP1 with the
 * EXIF, DQT, SOF0, DHT, SOS) does not depend on the pixels and is the caller's (riffusion.util.image_util.jpeg_header).
 * Not implemented: other subsamplings, optimised Huffman tables, progressive scans, greyscale.
 *
 * rfx_jpeg_quant_tables, host only (no GPU): the two tables of `quality` (1 .. 100; anything else is RFX_ERR_UNSUPPORTED), 64
 *   entries each in natural (row-major) order, 1 .. 255 - what DQT carries in zigzag order and d_qtables in natural order.
 * rfx_jpeg_scan_capacity: bytes one image's scan and EOI take at most (0 for sizes outside 1 .. 65535).  A block codes to at
 *   most 22 bits of DC (the longest DC code, 11 bits, and 11 value bits) and 63 x 26 bits of AC (the longest AC code, 16 bits,
 *   and 10 value bits): 1660 bits; the blocks, rounded up to a byte, could all be 0xFF bytes and double with the stuffing, and EOI
 *   adds 2: 2 * ceil(1660 * 6 * ceil(W / 16) * ceil(H / 16) / 8) + 2.
 * rfx_jpeg_encode_u8: d_rgb (N, H, W, 3) uint8 -> image n's scan at d_scan + n * capacity, capacity = rfx_jpeg_scan_capacity,
 *   and its length in d_scan_bytes[n] (never above the capacity; bytes past it are not written).  d_qtables: the two tables as
 *   (2, 64) uint16 in device memory.  d_workspace holds rfx_jpeg_encode_workspace_bytes (0 for arguments the call refuses).
 *   H or W above 65535, a capacity that an int32 does not hold, or more blocks than one launch takes are RFX_ERR_UNSUPPORTED,
 *   refused before anything is launched.  All launches go to `stream`; nothing synchronises. */
int rfx_jpeg_quant_tables(int quality, uint16_t* h_luma64, uint16_t* h_chroma64);
size_t rfx_jpeg_scan_capacity(int H, int W);
size_t rfx_jpeg_encode_workspace_bytes(int N, int H, int W);
int rfx_jpeg_encode_u8(const uint8_t* d_rgb, int N, int H, int W, const uint16_t* d_qtables, uint8_t* d_scan, int32_t* d_scan_bytes,
                       void* d_workspace, void* stream);

/* ---- JPEG decode: np.asarray(Image.open(f).convert("RGB")) of a baseline JPEG tile, on the device ------------------------------
 * The other direction: files of the corpus to (N, H, W, 3) uint8 tiles, the pixels Pillow (libjpeg-turbo, the v6b API) decodes,
 * byte for byte - Huffman decoding, jpeg_idct_islow, h2v2_fancy_upsample (plain replication for W <= 4, as libjpeg chooses) and
 * ycc_rgb_convert are integer arithmetic throughout.  Taken: 8-bit baseline (SOF0), three components Y Cb Cr sampled 2x2, 1x1,
 * 1x1, one interleaved scan, no restart interval, any Huffman tables (so `optimize=True` files too).  Everything before the scan
 * is the caller's to parse (riffusion.util.image_util.jpeg_parse), which also keeps every other kind of file on the host.
 * The scan is decoded in parallel: its bit stream, without the stuffed zeros, is cut into subsequences of 1024 bits, one thread
 * each, 256 at a time in one workgroup per image; every thread decodes from the state its predecessor left, in rounds, until no
 * state changes (self-synchronisation), and a last pass writes the coefficients.  No workgroup waits for another one.
 *
 * rfx_jpeg_decode_u8: image n's entropy-coded bytes - what follows the SOS header, up to and not including EOI - are
 *   d_scans[offsets[n] .. offsets[n + 1]); h_scan_offsets (host) and d_scan_offsets (device memory) are the same N + 1 int64,
 *   not decreasing, the first not negative; d_scans is aligned to 16 bytes and holds offsets[N] bytes.  All images are H x W.
 *   d_qtables: (N, 2, 64) uint16, each image's luma and chroma table in natural (row-major) order.  d_huff: (N, 4, 272) uint8, each
 *   image's DC luma, AC luma, DC chroma and AC chroma table as DHT carries it: BITS[16], then HUFFVAL padded to 256.
 *   d_rgb: (N, H, W, 3) uint8.  d_status: (N) int32, one per image:
 *     0 decoded; 1 a marker inside the scan (0xFF followed by anything but 0x00, or as the last byte); 2 a Huffman table that is
 *     no prefix code of at most 256 symbols; 3 the scan ends inside a block; 4 bits that are no code of the table, or a DC size
 *     above 11 / an AC size above 10; 5 a run past coefficient 63; 6 blocks missing at the end of the scan, or more than 7 bits
 *     left over after the last block.  With several causes the largest is reported.
 *   An image with a non-zero status has undefined pixels; the others of the call are not affected.  No read leaves d_scans'
 *   offsets[N] bytes or the workspace, whatever the bytes are.  d_workspace holds rfx_jpeg_decode_workspace_bytes(N, H, W,
 *   offsets[N] - offsets[0]) (0 for arguments the call refuses).  H or W above 65535, a scan longer than 2^28 - 64 bytes, or more
 *   blocks or pixels than one launch takes (N * 6 * ceil(W / 16) * ceil(H / 16) or N * H * W above (2^31 - 1) * 256) are
 *   RFX_ERR_UNSUPPORTED, refused before anything is launched.  All launches go to `stream`; nothing synchronises. */
size_t rfx_jpeg_decode_workspace_bytes(int N, int H, int W, size_t total_scan_bytes);
int rfx_jpeg_decode_u8(const uint8_t* d_scans, const int64_t* h_scan_offsets, const int64_t* d_scan_offsets, int N, int H, int W,
                       const uint16_t* d_qtables, const uint8_t* d_huff, uint8_t* d_rgb, int32_t* d_status, void* d_workspace, void* stream);

/* ---- PNG: a lossless tile's IDAT payload, on the device ----------------------------------------------------------------------------
 * PNG is the reference's lossless tile format (audio-to-image, its seed images).  The device writes the zlib stream that is the
 * payload of the one IDAT chunk, with its Adler-32, and the chunk's CRC-32; signature, IHDR, eXIf and IEND do not depend on the
 * pixels and are the caller's (riffusion.util.image_util.png_file).  The stream is NOT the one zlib writes: zlib's LZ77 parse is
 * sequential.  It is a run-length + Huffman deflate (zlib's Z_RLE class), every step a function of the tile alone (csrc/
 * rfx_png_core.h states it in full): each row filtered with the one of PNG's five filters whose filtered bytes have the least sum of
 * absolute values as int8 (ties to the lowest type); the filtered stream cut every 32 rows; inside a block every run of equal bytes
 * as a literal and matches at distance 1 of up to 258 bytes; one dynamic-Huffman block per block with a literal/length code limited
 * to 15 bits by a stated rule; blocks joined at bit granularity.  Any PNG reader gets the tile's pixels back; the file's size is
 * that of Pillow's save(..., compress_type=zlib.Z_RLE).  Colour type 2 (RGB) or 0 (grey, for a tile whose three channels are equal
 * at every pixel), bit depth 8, no interlace.
 *
 * rfx_png_stream_capacity: bytes one tile's stream takes at most, for channels 3 or 1 (0 for anything else, or sizes outside
 *   1 .. 65535).  The filtered stream has S = H * (W * channels + 1) bytes in B = ceil(H / 32) blocks.  A token costs at most 15
 *   bits per byte it covers: a literal is one code of at most 15 bits for 1 byte, a match at most 15 + 5 + 1 bits (length code,
 *   extra bits, distance code) for at least 3.  A block's header is bounded by its field widths: 3 + 14 bits, 19 x 3 bits of
 *   code-length code, and for each of its 287 lengths at most a 7-bit symbol with 7 extra bits: 4092 bits; its end-of-block adds
 *   15.  With the 2 bytes of zlib header and the 4 of Adler-32: 2 + ceil((B * 4107 + 15 * S) / 8) + 4.  No stored or fixed-Huffman
 *   block is needed for the bound.
 * rfx_png_encode_u8: d_rgb (N, H, W, 3) uint8 -> tile n's stream at d_stream + n * capacity, capacity = rfx_png_stream_capacity(H,
 *   W, mode == 1 ? 1 : 3); its length in d_stream_bytes[n] (never above the capacity; no byte past the length is written); the
 *   CRC-32 of b"IDAT" + stream in d_crc[n]; what the tile was written with in d_channels[n].  mode 0: RGB.  mode 1: grey; a tile
 *   that is not grey gets d_channels[n] = 0, d_stream_bytes[n] = 0 and no stream, the other tiles are not affected.  mode 2: grey
 *   where R = G = B at every pixel, else RGB, decided on the device.  d_stream_bytes, d_crc and d_channels are N 32-bit words each,
 *   aligned to 4 bytes.  d_workspace holds rfx_png_encode_workspace_bytes(N, H, W) (0 for arguments the call refuses), aligned to
 *   256 bytes.  H or W above 65535, a capacity that an int32 does not hold, or more rows or stream pieces than one launch takes
 *   (N * H or N * ceil(capacity / 256) above 2^31 - 1) are RFX_ERR_UNSUPPORTED, refused before anything is launched.  All launches
 *   go to `stream`; nothing synchronises. */
#define RFX_PNG_RGB 0
#define RFX_PNG_GRAY 1
#define RFX_PNG_AUTO 2
size_t rfx_png_stream_capacity(int H, int W, int channels);
size_t rfx_png_encode_workspace_bytes(int N, int H, int W);
int rfx_png_encode_u8(const uint8_t* d_rgb, int N, int H, int W, int mode, uint8_t* d_stream, int32_t* d_stream_bytes, uint32_t* d_crc,
                      int32_t* d_channels, void* d_workspace, void* stream);

/* ---- PNG decode: np.asarray(Image.open(f).convert("RGB")) of a PNG tile, on the device ------------------------------------------
 * The other direction: files of the corpus to (N, H, W, 3) uint8 tiles, the pixels Pillow gives, byte for byte - inflate (RFC 1950
 * / 1951: stored, fixed and dynamic blocks, the Adler-32), PNG's five row filters and the step to RGB (grey three times, RGB as
 * is, RGBA without its alpha, palette[index]) are integer work throughout.  Taken: bit depth 8, colour type 0, 2, 3 or 6, no
 * interlace, whatever wrote the stream (zlib at any level and strategy, rfx_png_encode_u8).  The chunks are the caller's to walk
 * (riffusion.util.image_util.png_parse), which also keeps every other kind of file on the host.  A deflate stream is a chain, so
 * the parallelism is across the files of a call: one wave per image inflates with the 32 KiB window as a ring in LDS, its lanes
 * sharing table building, match copies and the write-out; one workgroup per image then unfilters row by row.  No workgroup
 * waits for another one, and every loop ends with the input or output it consumes.
 *
 * rfx_png_decode_u8: image n's zlib stream - its IDAT payloads concatenated in file order - is d_streams[offsets[n] ..
 *   offsets[n + 1]); h_stream_offsets (host) and d_stream_offsets (device memory) are the same N + 1 int64, not decreasing, the
 *   first not negative; d_streams is aligned to 16 bytes and holds offsets[N] bytes.  All images are H x W of `color_type`.
 *   d_palettes: (N, 256, 3) uint8 and d_palette_entries: (N) int32, each image's PLTE and its entry count; read for colour type 3
 *   only (NULL otherwise).  d_rgb: (N, H, W, 3) uint8.  d_status: (N) int32, one per image, the first cause in stream order:
 *     0 decoded; 1 the zlib header (CM, CINFO, FDICT, check bits); 2 block type 3, or a stored block's LEN != ~NLEN; 3 a dynamic
 *     header that does not define two usable prefix codes (HLIT > 286, HDIST > 30, a repeat with nothing before it or past the
 *     count, an over-subscribed code, an incomplete literal/length or code-length code, no end-of-block code, an incomplete
 *     distance code other than a single code of one bit or no code at all, RFC 1951's block of literals only); 4 bits that are no code, length symbol 286 / 287, distance symbol 30 /
 *     31; 5 a distance beyond the bytes produced so far; 6 the input ends inside the stream; 7 more output than H * (W * bpp + 1);
 *     8 fewer bytes at the final block's end; 9 Adler-32 mismatch; 10 bytes left over behind the Adler-32; 11 a filter type above
 *     4; 12 a palette index at or past the image's entry count.
 *   Status 0 means the pixels are Pillow's; the decoder refuses what it is not sure zlib and Pillow take the same way (refusing
 *   costs time, never correctness: the caller opens such a file with Pillow).  An image with a non-zero status has undefined
 *   pixels; the others of the call are not affected.  No read leaves d_streams' offsets[N] bytes or the workspace, whatever the
 *   bytes are.  d_workspace holds rfx_png_decode_workspace_bytes(N, H, W, color_type, offsets[N] - offsets[0]) (0 for arguments
 *   the call refuses), aligned to 256 bytes.  H or W above 65535, a stream longer than 2^28 - 64 bytes, or more filtered bytes than
 *   a launch indexes (N * H * (W * bpp + 1), each image rounded up to 256, above 2^63 - 1) are RFX_ERR_UNSUPPORTED, refused before
 *   anything is launched.  All launches go to `stream`; nothing synchronises. */
size_t rfx_png_decode_workspace_bytes(int N, int H, int W, int color_type, size_t total_stream_bytes);
int rfx_png_decode_u8(const uint8_t* d_streams, const int64_t* h_stream_offsets, const int64_t* d_stream_offsets, int N, int H, int W,
                      int color_type, const uint8_t* d_palettes, const int32_t* d_palette_entries, uint8_t* d_rgb, int32_t* d_status,
                      void* d_workspace, void* stream);

/* ---- int16 front end of the encode: pydub's set_frame_rate / set_channels and the clip slicing on the device -------------------
 * What the reference does on the host before every encode (cli.py:132-193, streamlit/tasks/audio_to_audio.py): AudioSegment
 * .set_channels (audioop.tomono(data, 2, 0.5, 0.5) / audioop.tostereo(data, 2, 1, 1)), .set_frame_rate
 * (audioop.ratecv(data, 2, channels, inrate, outrate, None): linear interpolation, weights 1 / 0, a fresh state), the slice into
 * clips and the int16 -> float32 (channels, samples) array.  Reproduced byte for byte.
 *
 * Exactness of the resample.  With a = in_rate / g, b = out_rate / g, g = gcd(in_rate, out_rate), L input frames give
 * K = floor((L - 1) * b / a) + 1 output frames; output k reads input frames n_k - 2 and n_k - 1 (frame -1 is zero),
 * n_k = 1 + ceil(k * a / b), with the weights d_k = (n_k - 1) * b - k * a and b - d_k, and is
 * trunc(((x[n_k - 2] << 16) * d_k + (x[n_k - 1] << 16) * (b - d_k)) / b) >> 16.  audioop evaluates the numerator and the division
 * in double: the numerator is exact below 2^53 and the truncated quotient is then the integer quotient, which holds for every
 * int16 input while b < 2^21.  Both reduced rates must therefore stay below 2^20; other pairs are refused
 * (RFX_ERR_UNSUPPORTED).  Every common pair passes (48000 <-> 44100 reduces to 160 <-> 147).  Equal rates copy (or only mix).
 * Not implemented: a carried ratecv state, weights other than 1 / 0, more than two channels.  All frame indices are 64-bit.
 *
 * rfx_pcm16_resample_frames, host only (no GPU): K for in_frames >= 1.
 * rfx_pcm16_resample: d_in (in_frames, in_channels) int16 interleaved -> d_out (out_frames, out_channels) int16, with
 *   out_frames = K.  When the channel counts differ (1 -> 2 or 2 -> 1) the mix is applied to the stored frames FIRST and the
 *   mixed recording is resampled: set_channels, then set_frame_rate - the batch CLI's order.  Pointers are frame-aligned
 *   (2 * channels bytes); d_in and d_out must not overlap.
 * rfx_pcm16_clips_to_waveform: clip i = frames [starts[i], starts[i] + Lw) of d_pcm (frames, in_channels) int16 ->
 *   d_wave_out rows i * out_channels + c, (N * out_channels, Lw) float32 - the layout rfx_image_from_waveform reads; the
 *   conversion is exact.  A channel mix is applied AFTER the slice, as spectrogram_image_from_audio's set_channels is.  Clips
 *   may overlap.  h_starts (host) is checked against frames and Lw before anything is launched; d_starts is the same table in
 *   device memory.  N == 0 is a no-op. */
int rfx_pcm16_resample_frames(int64_t in_frames, int in_rate, int out_rate, int64_t* out_frames);
int rfx_pcm16_resample(const int16_t* d_in, int64_t in_frames, int in_channels, int in_rate, int out_channels, int out_rate,
                       int16_t* d_out, int64_t out_frames, void* stream);
int rfx_pcm16_clips_to_waveform(const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts, const int64_t* d_starts,
                                int N, int Lw, int out_channels, float* d_wave_out, void* stream);

/* ---- inverse, all the way from the image: SpectrogramImageConverter.audio_from_spectrogram_image's device half
 * (spectrogram_image_converter.py:54-91: image_util.spectrogram_from_image, audio_from_spectrogram -> waveform_from_mel_amplitudes
 * on the image's (C, n_mels, T) tensor, audio_util.audio_from_waveform).  d_img (N, n_mels, T, 3) uint8 -> d_pcm_out (N, L, C) int16,
 * L = rfx_griffinlim_output_samples(plan, T); d_clip_peak (N floats) as rfx_pcm16; d_lut256 as rfx_image_decode_u8.  Exactly
 * rfx_image_decode_u8, rfx_waveform_from_mel (clips of C rows, `seed`), rfx_pcm16 - same bytes - with the tensors in between
 * kept inside the workspace. */
size_t rfx_audio_from_image_workspace_bytes(const rfx_plan* plan, int N, int stereo, int T);
int rfx_audio_from_image_u8(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                            int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                            size_t workspace_bytes, void* stream);

/* options->row_base counts ROWS (clip-channels): the call's first image is image row_base / C of the caller's batch */
int rfx_audio_from_image_u8_ex(const rfx_plan* plan, const uint8_t* d_img, int N, int T, int stereo, const float* d_lut256, uint64_t seed,
                               int n_iter, float momentum, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* d_workspace,
                               size_t workspace_bytes, void* stream, const rfx_call_options* options);

#ifdef __cplusplus
}
#endif
#endif /* RFX_H_ */
