// Stand-alone driver of tests/emu/rfx_vocoder_emu.cpp for a sanitizer run (tests/test_vocoder_cpu.py builds the two files with
// -fsanitize=address,undefined and runs the program).  At an odd and an even FFT length, T = 1, 2, 9 and 41, rates above and below one
// and far from one, it runs the bin-order walk and the slot-order walk into heap buffers of exactly the documented sizes - so a read
// past frame T - 1 or a write past step T_out - 1 is an error of the program - and checks what needs no oracle: the frame count, the
// zero row, the copy at rate 1, a row alone against the row in the batch, the two slots of a doubled bin against each other, the
// padding.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_vocoder_core.h"

extern "C" {
long long emu_voc_frames(int T, double rate);
float emu_voc_advance(int hop, int k, int n_stft);
int emu_voc_step(int i, double rate, float* alpha);
int emu_vocoder(int n_stft, int hop, int B, int T, double rate, const float* X, float* Y);
int emu_vocoder_slots(int stride, const int32_t* src, const float* adv, const uint8_t* conj, int rows, int T, double rate, const float* X,
                      float* Y);
}

static int failures = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      ++failures;                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                       \
  } while (0)

static float noise(unsigned& s) {  // a fixed sequence in [-1, 1)
  s = s * 1664525u + 1013904223u;
  return (float)((double)(s >> 8) / 8388608.0 - 1.0);
}

int main() {
  const int geo[2][2] = {{505, 100}, {501, 26}};  // (n_stft, hop): n_fft 1009 and 1000
  const int frames[4] = {1, 2, 9, 41};
  const double rates[7] = {1.25, 0.75, 1.1, 0.9, 0.5, 3.7, 1.0};
  for (const auto& g : geo) {
    const int F = g[0], hop = g[1], B = 3;
    for (const int T : frames)
      for (const double rate : rates) {
        const long long n = emu_voc_frames(T, rate);
        CHECK(n == (long long)std::ceil((double)T / rate) && n >= 1);
        const int To = (int)n;
        unsigned seed = 11u + (unsigned)T;
        std::vector<float> X((size_t)B * F * T * 2), Y((size_t)B * F * To * 2, 123.f), Y1((size_t)F * To * 2, 123.f);
        for (float& v : X) v = noise(seed);
        std::memset(X.data() + (size_t)(B - 1) * F * T * 2, 0, (size_t)F * T * 2 * sizeof(float));  // the last row is silent
        CHECK(emu_vocoder(F, hop, B, T, rate, X.data(), Y.data()) == To);
        for (size_t i = (size_t)(B - 1) * F * To * 2; i < Y.size(); ++i) CHECK(Y[i] == 0.f);
        for (const float v : Y) CHECK(std::isfinite(v));
        if (rate == 1.0) CHECK(std::memcmp(X.data(), Y.data(), X.size() * sizeof(float)) == 0);
        CHECK(emu_vocoder(F, hop, 1, T, rate, X.data() + (size_t)F * T * 2, Y1.data()) == To);  // row 1 alone
        CHECK(std::memcmp(Y1.data(), Y.data() + (size_t)F * To * 2, Y1.size() * sizeof(float)) == 0);
        // slot order: positions 0 .. F - 1 hold their bins; F .. F + 3 hold bins 1 .. 4 a second time, as conjugates; then four of padding
        const int S = F + 8;
        std::vector<int32_t> src((size_t)S, -1);
        std::vector<float> adv((size_t)S, 0.f);
        std::vector<uint8_t> conj((size_t)S, 0);
        for (int p = 0; p < F + 4; ++p) {
          const int k = p < F ? p : p - F + 1;
          src[(size_t)p] = k;
          conj[(size_t)p] = p >= F;
          adv[(size_t)p] = p >= F ? -emu_voc_advance(hop, k, F) : emu_voc_advance(hop, k, F);
        }
        std::vector<float> Xs((size_t)T * S * 2, 7.f), Ys((size_t)To * S * 2, 123.f);  // row 0 of X, frame-major; the secondary slots and the padding hold junk
        for (int t = 0; t < T; ++t)
          for (int k = 0; k < F; ++k) {
            Xs[((size_t)t * S + k) * 2] = X[((size_t)k * T + t) * 2];
            Xs[((size_t)t * S + k) * 2 + 1] = X[((size_t)k * T + t) * 2 + 1];
          }
        CHECK(emu_vocoder_slots(S, src.data(), adv.data(), conj.data(), 1, T, rate, Xs.data(), Ys.data()) == To);
        if (rate != 1.0)
          for (int i = 0; i < To; ++i) {
            for (int k = 0; k < F; ++k) {  // the primary slots are the bin-order walk, bit for bit
              CHECK(std::memcmp(&Ys[((size_t)i * S + k) * 2], &Y[((size_t)k * To + i) * 2], 2 * sizeof(float)) == 0);
            }
            for (int p = F; p < F + 4; ++p) {  // a conjugate slot is its bin's conjugate
              const float re = Ys[((size_t)i * S + p - F + 1) * 2], im = -Ys[((size_t)i * S + p - F + 1) * 2 + 1];
              CHECK(std::memcmp(&Ys[((size_t)i * S + p) * 2], &re, sizeof(float)) == 0 && std::memcmp(&Ys[((size_t)i * S + p) * 2 + 1], &im, sizeof(float)) == 0);
            }
            for (int p = F + 4; p < S; ++p) CHECK(Ys[((size_t)i * S + p) * 2] == 0.f && Ys[((size_t)i * S + p) * 2 + 1] == 0.f);
          }
      }
  }
  CHECK(emu_voc_frames(41, 0.0) == -1 && emu_voc_frames(41, -1.0) == -1 && emu_voc_frames(0, 1.25) == -1);
  CHECK(emu_voc_frames(41, std::nan("")) == -1 && emu_voc_frames(41, INFINITY) == -1 && emu_voc_frames(2147483647, 0.5) == -1);
  CHECK(emu_voc_frames(2147483647, 1.0) == 2147483647LL);
  // a step's pair: the floor of the double product; a product past 2^31 is clamped before the conversion (no undefined cast), a NULL alpha is allowed
  float al = -1.f;
  CHECK(emu_voc_step(21, 2.0 / 3.0, &al) == 14 && al == 0.f);
  CHECK(emu_voc_step(7, 0.3, &al) == 2 && al == (float)(7 * 0.3 - 2.0));
  CHECK(emu_voc_step(1000, 1e7, &al) == 2147483646 && al == 0.f);
  CHECK(emu_voc_step(2147483647, 1e300, nullptr) == 2147483646);
  CHECK(rfx::voc_wrap(0.75f) == -0.25f && rfx::voc_wrap(-0.75f) == 0.25f && rfx::voc_wrap(0.5f) == 0.5f && rfx::voc_wrap(-0.5f) == -0.5f);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
