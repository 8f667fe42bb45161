// Host emulator of the int16 front-end kernels (csrc/rfx_pcm_in.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_pcm_in_cpu.py with g++): it runs the functions of rfx_pcm_in_core.h that the kernels inline - the ratecv index,
// state and interpolation, the channel mix, the clip gather - the way the kernels walk them (runs of kRatecvRun output frames
// per thread, the state of a run's first frame from the closed form, the others from the recurrence), so that they are pinned
// against audioop and PcmSegment on the CPU.  The run walk (ratecv_run: state reuse, which frames are reloaded) is the kernel's own
// function; what the kernel has of its own is how a frame is fetched (load_mixed's dword loads) and how a run is stored.
#include <cstdint>
#include "../../riffusion-hobby_amd/csrc/rfx_pcm_in_core.h"

using namespace rfx;

// one launch of the resample kernel for channel counts known at compile time: the head frames as runs of one, then the runs
template <int C_IN, int C_OUT>
static void ratecv_launch(const int16_t* in, RatecvRates r, int64_t K, int64_t head, int16_t* out) {
  constexpr int CC = C_IN < C_OUT ? C_IN : C_OUT;
  const auto load = [&](int64_t frame, int (&v)[2]) {
    for (int c = 0; c < 2; ++c) v[c] = c < CC ? pcm_mixed_sample(in, frame, c, C_IN, C_OUT) : 0;
  };
  const int64_t n_runs = (K - head + kRatecvRun - 1) / kRatecvRun;
  for (int64_t i = 0; i < n_runs + head; ++i) {  // thread i of the grid
    const int64_t k0 = i < n_runs ? head + kRatecvRun * i : i - n_runs;
    const int64_t left = K - k0;
    const int count = i < n_runs ? (left < kRatecvRun ? (int)left : kRatecvRun) : 1;
    int16_t res[kRatecvRun * C_OUT];
    ratecv_run<C_OUT, CC>(k0, count, r, load, res);
    for (int j = 0; j < count * C_OUT; ++j) out[k0 * C_OUT + j] = res[j];
  }
}

extern "C" {

int64_t emu_ratecv_frames(int64_t L, int64_t in_rate, int64_t out_rate) { return ratecv_out_frames(L, ratecv_rates(in_rate, out_rate)); }

// (L, C_in) -> (K, C_out), K = emu_ratecv_frames(L, ...): mix, then ratecv; `head` as the launcher's (frames before the first run)
void emu_ratecv(const int16_t* in, int64_t L, int C_in, int64_t in_rate, int C_out, int64_t out_rate, int16_t* out, int64_t head) {
  const RatecvRates r = ratecv_rates(in_rate, out_rate);
  const int64_t K = ratecv_out_frames(L, r);
  if (head > K) head = K;
  if (C_in == 1 && C_out == 1) ratecv_launch<1, 1>(in, r, K, head, out);
  else if (C_in == 2 && C_out == 2) ratecv_launch<2, 2>(in, r, K, head, out);
  else if (C_in == 2) ratecv_launch<2, 1>(in, r, K, head, out);
  else ratecv_launch<1, 2>(in, r, K, head, out);
}

// N clips of Lw frames at starts[i] of an (L, C_in) recording -> (N * C_out, Lw) float32 planar, mix after the slice
void emu_clips(const int16_t* pcm, int C_in, const int64_t* starts, int N, int64_t Lw, int C_out, float* wave) {
  for (int n = 0; n < N; ++n)
    for (int64_t t = 0; t < Lw; ++t)
      for (int c = 0; c < C_out; ++c) wave[((int64_t)n * C_out + c) * Lw + t] = (float)pcm_mixed_sample(pcm, starts[n] + t, c, C_in, C_out);
}

int emu_tomono(int l, int r) { return pcm_tomono(l, r); }

}  // extern "C"
