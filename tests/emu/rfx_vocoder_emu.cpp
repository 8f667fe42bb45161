// Host emulator of the time stretch's kernel (riffusion-hobby_amd/csrc/rfx_vocoder.hip): the arithmetic and the walk are
// rfx_vocoder_core.h's own, compiled for the host (its sine and cosine in double, rounded once: the host has no sincospif).
//   emu_vocoder        (B, n_stft, T) complex64 in bin order -> (B, n_stft, T_out), every bin with its advance frac(hop k / D)
//   emu_voc_step       the frame pair and the weight of one output step (voc_step), for tests/test_vocoder_cpu.py to hold to i * rate
//   emu_vocoder_slots  rows of T frames of `stride` complex slots -> rows of T_out frames, position by position as the kernel does it,
//                      from the table rfx_debug_vocoder_table answers (bin's primary position, signed advance, conjugate flag)
// rate == 1 copies, as the drivers do.  Built by tests/test_vocoder_cpu.py with -ffp-contract=off.
#include <cstdint>
#include <cstring>

#include "../../riffusion-hobby_amd/csrc/rfx_vocoder_core.h"

using rfx::cf;

extern "C" {

long long emu_voc_frames(int T, double rate) { return rfx::voc_frames(T, rate); }

float emu_voc_advance(int hop, int k, int n_stft) { return rfx::voc_advance_turns(hop, k, n_stft); }

// the frame pair of step i: i0 = floor((double)i * rate), clamped below 2^31 - 1, and alpha, the weight of frame i0 + 1
int emu_voc_step(int i, double rate, float* alpha) { return rfx::voc_step(i, rate, alpha); }

int emu_vocoder(int n_stft, int hop, int B, int T, double rate, const float* X, float* Y) {
  const long long n = rfx::voc_frames(T, rate);
  if (n < 1) return -1;
  const int T_out = (int)n;
  if (rate == 1.0) {
    memcpy(Y, X, (size_t)B * n_stft * T * sizeof(cf));
    return T_out;
  }
  for (long long r = 0; r < (long long)B * n_stft; ++r) {
    const cf* in = reinterpret_cast<const cf*>(X) + (size_t)r * T;
    cf* out = reinterpret_cast<cf*>(Y) + (size_t)r * T_out;
    rfx::voc_walk(
        T, T_out, rate, rfx::voc_advance_turns(hop, (int)(r % n_stft), n_stft), [=](int j) { return in[j]; }, [=](int i, cf v) { out[i] = v; });
  }
  return T_out;
}

int emu_vocoder_slots(int stride, const int32_t* src, const float* adv, const uint8_t* conj, int rows, int T, double rate, const float* X,
                      float* Y) {
  const long long n = rfx::voc_frames(T, rate);
  if (n < 1) return -1;
  const int T_out = (int)n;
  if (rate == 1.0) {
    memcpy(Y, X, (size_t)rows * T * stride * sizeof(cf));
    return T_out;
  }
  for (int r = 0; r < rows; ++r)
    for (int p = 0; p < stride; ++p) {
      cf* out = reinterpret_cast<cf*>(Y) + (size_t)r * T_out * stride + p;
      if (src[p] < 0) {
        for (int i = 0; i < T_out; ++i) out[(size_t)i * stride] = cf{0.f, 0.f};
        continue;
      }
      const cf* in = reinterpret_cast<const cf*>(X) + (size_t)r * T * stride + src[p];
      const bool flip = conj[p] != conj[src[p]];
      rfx::voc_walk(
          T, T_out, rate, flip ? -adv[p] : adv[p], [=](int j) { return in[(size_t)j * stride]; },
          [=](int i, cf v) {
            if (flip) v.im = -v.im;
            out[(size_t)i * stride] = v;
          });
    }
  return T_out;
}

}  // extern "C"
