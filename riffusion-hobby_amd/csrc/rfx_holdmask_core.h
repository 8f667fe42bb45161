// rfx_holdmask_core.h - arithmetic of a masked Griffin-Lim call (include/rfx.h: rfx_masked_call_options; kernels in
// rfx_holdmask.hip), written once for the gfx950 kernels (hipcc) and the host emulator of the CPU tests
// (tests/emu/rfx_holdmask_emu.cpp, g++).
//
// A masked call holds the guide's phase in chosen BINS of chosen frames.  The hold is linear: with S_held = S where held and 0
// elsewhere, S_free = S - S_held and c = ISTFT(S_held a0), every iterate is
//   x_k = ISTFT(S_free proj(STFT(x_{k-1}) - m STFT(x_{k-2}))) + c,      x_0 = ISTFT(S a0),
// so the frame engines run unchanged on magnitudes that are zero in the held bins and a constant audio buffer is added to each
// generation.  What is left to do here: the SPLIT of a call's magnitude slots by the bit mask, in each of the three
// slot orders the engines read, and the expansion of a per-mel-band mask to the bin mask.
//
// The mask: (B, T, words) uint32, words = ceil(n_stft / 32); bin b of a frame is held iff bit b & 31 of word b >> 5 of the frame is
// set.  Bits at or above n_stft in the last word are never read.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rfx_core.h"

namespace rfx {

constexpr int kHoldMaskThreads = 256;

// the slot orders magnitudes come in
constexpr int kHoldMaskSpec = 0;   // specialised engine: slot_pos_f order, kFrameStride positions (rfx_pack_magnitudes' map; 440 bins twice)
constexpr int kHoldMaskPlain = 1;  // generic plans: position = bin, padded to the frame stride
constexpr int kHoldMaskTable = 2;  // row family's slot order: bin_of[position], -1 for padding (launch_fam_repack's table)

RFX_HD int holdmask_words(int n_stft) { return (n_stft + 31) >> 5; }

// the bin position p of a frame stands for; -1: a padding position
RFX_HD int holdmask_slot_bin(int layout, int p, int n_stft, const int* bin_of) {
  if (layout == kHoldMaskSpec) {
    int q, kb;
    if (!pos_f_to_slot(p, q, kb)) return -1;
    return slot_bin(q / 21, q % 21, kb, nullptr);  // (the second copy of a bin follows its bin)
  }
  if (layout == kHoldMaskTable) return bin_of[p];
  return p < n_stft ? p : -1;
}

RFX_HD bool holdmask_bit(const uint32_t* frame_words, int bin) { return (frame_words[bin >> 5] >> (bin & 31)) & 1u; }

// one position of X: want_held ? S_held : S_free; padding is written as 0
RFX_HD float holdmask_split(float s, int bin, const uint32_t* frame_words, bool want_held) {
  if (bin < 0) return 0.f;
  return holdmask_bit(frame_words, bin) == want_held ? s : 0.f;
}

// ---- band to bin: word `word` of frame t of one row of the bin mask from the row's per-band mask (n_mels, T), nonzero = held.
// lo[f] .. hi[f]: the first and last band with a nonzero weight at bin f (lo = -1: no filter reaches the bin, never held).  Bin f is
// held iff every band of that range is held at t.  Every bit is written; bits at or above n_stft are 0.
RFX_HD uint32_t holdmask_band_word(const uint8_t* bands_row, int T, int t, const int16_t* lo, const int16_t* hi, int word, int n_stft) {
  uint32_t w = 0;
  for (int i = 0; i < 32; ++i) {
    const int f = word * 32 + i;
    if (f >= n_stft) break;
    const int l = lo[f], h = hi[f];
    if (l < 0) continue;
    bool held = true;
    for (int m = l; m <= h; ++m) held = held && bands_row[(size_t)m * T + t] != 0;
    if (held) w |= 1u << i;
  }
  return w;
}

}  // namespace rfx
