// Host emulator of the two kernels of a masked Griffin-Lim call (csrc/rfx_holdmask.hip: holdmask_split_kernel,
// holdmask_bands_kernel).  TEST INFRASTRUCTURE ONLY (built by tests/test_hold_mask_cpu.py with g++): it runs the functions of
// rfx_holdmask_core.h that the kernels inline - the bin a position stands for in each slot order, the bit of a bin, the split, the
// word of the bin mask from a band mask - the way the launches walk them: one logical thread per position of a frame (split) or per
// (word, frame) of a row (bands).  What the kernels have of their own is the grid: rows on grid y in chunks of 65535, frames on z.
#include <cstddef>
#include <cstdint>
#include "../../riffusion-hobby_amd/csrc/rfx_holdmask_core.h"

using namespace rfx;

extern "C" {

int emu_holdmask_words(int n_stft) { return holdmask_words(n_stft); }
int emu_holdmask_spec_stride() { return kFrameStride; }
int emu_holdmask_slot_bin(int layout, int p, int n_stft, const int* bin_of) { return holdmask_slot_bin(layout, p, n_stft, bin_of); }

// S, X: [B*T][stride]; mask: (B, T, words) uint32
void emu_holdmask_split(int layout, const float* S, float* X, const uint32_t* mask, const int* bin_of, int B, int T, int stride, int n_stft,
                        int want_held) {
  const int words = holdmask_words(n_stft);
  for (size_t row = 0; row < (size_t)B; ++row)
    for (int p = 0; p < stride; ++p) {
      const int bin = holdmask_slot_bin(layout, p, n_stft, bin_of);
      for (int t = 0; t < T; ++t) {
        const size_t fr = row * (size_t)T + t, at = fr * (size_t)stride + p;
        X[at] = holdmask_split(S[at], bin, mask + fr * (size_t)words, want_held != 0);
      }
    }
}

// bands: (B, M, T) uint8; out: (B, T, words) uint32
void emu_holdmask_bands(const uint8_t* bands, const int16_t* lo, const int16_t* hi, uint32_t* out, int B, int M, int T, int n_stft) {
  const int words = holdmask_words(n_stft);
  for (size_t row = 0; row < (size_t)B; ++row)
    for (long long i = 0; i < (long long)T * words; ++i) {
      const int word = (int)(i / T), t = (int)(i - (long long)word * T);
      out[(row * (size_t)T + t) * (size_t)words + word] = holdmask_band_word(bands + row * (size_t)M * (size_t)T, T, t, lo, hi, word, n_stft);
    }
}

}  // extern "C"
