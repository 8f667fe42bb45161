// rfx_jpeg_dec_core.h - decoding a baseline JPEG as Pillow (libjpeg-turbo, the v6b API) decodes it into an RGB image, written once
// for the gfx950 kernels (rfx_jpeg_dec.hip, hipcc) and the host emulator of the CPU tests (tests/emu/rfx_jpeg_dec_emu.cpp, g++).
// The files taken: 8 bit, three components, YCbCr 4:2:0, one interleaved scan, no restart interval, any Huffman tables.  Every
// step is integer arithmetic:
//   * entropy decoding: jdhuff.c - the canonical codes of a DHT table (BITS, HUFFVAL), a code's symbol, the value bits and their
//     EXTEND; DC as the difference to the previous block of the component, AC as run / size with ZRL and EOB.  Stricter than
//     libjpeg where a file Pillow itself writes never goes: a DC size above 11, an AC size above 10, a run past coefficient 63
//     and a ZRL that ends a block are errors here (the caller then hands the file to Pillow);
//   * the scan is decoded in parallel by self-synchronisation (Weissenberger & Schmidt, ICPP 2018): the unstuffed bit stream is
//     cut into subsequences of kJpdSubBits bits, each decoded from the state its predecessor left (jpd_decode_span), in rounds,
//     until no state changes; the states are then the true ones, a scan of the block counts gives every subsequence its first
//     block, and one more pass writes the coefficients;
//   * dequantisation and jidctint.c's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2), the result + 128 limited to 0 .. 255 (the
//     SIMD routines saturate where the C routine masks and looks up: the same for every value a real image reaches);
//   * jdsample.c's h2v2_fancy_upsample: 3/4 of the nearer and 1/4 of the further chroma row, then the same across columns with
//     the rounding 8 (even output columns) and 7 (odd ones); the first and the last chroma COLUMN (ceil(W / 2) - 1) are not
//     filtered outwards, and the rows above the first and below the last chroma ROW (ceil(H / 2) - 1) are copies of those rows;
//     an image of at most two chroma columns (W <= 4) gets h2v2_upsample instead, every chroma sample repeated 2 x 2;
//   * jdcolor.c's ycc_rgb_convert with its 16-bit fixed-point tables.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rfx_jpeg_core.h"

namespace rfx {

// ---- status of one image ------------------------------------------------------------------------------------------------------
constexpr int kJpdOk = 0;
constexpr int kJpdMarker = 1;     // 0xFF followed by anything but 0x00 inside the scan, or 0xFF as its last byte
constexpr int kJpdBadTable = 2;   // a Huffman table with more than 256 codes, or more codes of a length than that length has
constexpr int kJpdOutOfBits = 3;  // the scan ended inside a block
constexpr int kJpdBadCode = 4;    // bits that are no code of the table, or a size the baseline process does not have
constexpr int kJpdZigzag = 5;     // a run past coefficient 63
constexpr int kJpdLeftOver = 6;   // blocks missing at the end of the scan, or more than 7 bits left after the last block

// ---- the bit stream and its subsequences --------------------------------------------------------------------------------------
constexpr int kJpdSubBits = 1024;                       // S: bits of one subsequence (a multiple of 32)
constexpr int kJpdSubWords = kJpdSubBits / 32;          //
constexpr int kJpdGroup = 256;                          // subsequences one workgroup synchronises at a time (its threads)
constexpr int kJpdSymbolMaxBits = 27;                   // a 16-bit code and 11 value bits: what one peek of 32 bits must hold
constexpr int64_t kJpdMaxScanBytes = (1ll << 28) - 64;  // per image: bit positions are 32-bit
constexpr int kJpdHuffBytes = 272;                      // one table of d_huff: BITS[16], HUFFVAL[256]
constexpr int kJpdLutBits = 9;

// where image n's unstuffed stream lies in the workspace's byte area, and its 16-byte chunks in the chunk tables: functions of
// the scan offsets alone (off0 = offsets[0]).  A region holds the stream, rounded up to a word, and 8 bytes more: the two words
// a peek loads are always inside it.
RFX_JPG_HD int64_t jpd_region_offset(int64_t off, int64_t off0, int64_t n) { return ((off - off0 + 15) & ~(int64_t)15) + 64 * n; }
RFX_JPG_HD int64_t jpd_chunk_offset(int64_t off, int64_t off0, int64_t n) { return ((off & ~(int64_t)15) - (off0 & ~(int64_t)15)) / 16 + 2 * n; }

// the planes of one image: Y (16 mcu_h, 16 mcu_w), then Cb and Cr (8 mcu_h, 8 mcu_w) each
RFX_JPG_HD int64_t jpd_plane_bytes(const JpgGeom& g) { return 384 * g.mcus; }

// the decode's workspace (host arithmetic; the launcher, the C ABI's size query and the host emulator all take it from here):
// every image's unstuffed region, the chunk tables (`pre`: the zeros dropped before each 16-byte chunk), the unstuffed lengths,
// the coefficients (N, blocks, 64) int16 and the planes, each on a 256-byte boundary.  total_scan_bytes = offsets[N] - offsets[0].
struct JpdLayout {
  size_t unstuffed, pre, ulen, coef, planes, total;  // byte offsets, and the size
  size_t coef_bytes;                                 // the coefficients: cleared before every decode
};
inline JpdLayout jpeg_decode_workspace_layout(int N, int H, int W, size_t total_scan_bytes) {
  JpdLayout l{};
  if (N <= 0 || H <= 0 || W <= 0 || H > kJpgMaxSize || W > kJpgMaxSize) return l;
  const JpgGeom g = jpg_geom(H, W);
  size_t at = 0;
  const auto take = [&at](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  l.unstuffed = take((size_t)jpd_region_offset((int64_t)total_scan_bytes, 0, N) + 64);
  l.pre = take(((total_scan_bytes + 15) / 16 + 2 * (size_t)N + 2) * sizeof(uint32_t));
  l.ulen = take((size_t)N * sizeof(uint32_t));
  l.coef_bytes = (size_t)N * (size_t)g.blocks * 64 * sizeof(int16_t);
  l.coef = take(l.coef_bytes);
  l.planes = take((size_t)N * (size_t)jpd_plane_bytes(g));
  l.total = at;
  return l;
}

// ---- Huffman tables -------------------------------------------------------------------------------------------------------------
// jdhuff.c's derived table: maxcode[l] the largest code of length l (-1: none), valoff[l] = index of its first symbol - its
// first code; lut[top kJpdLutBits bits] = length << 8 | symbol for the codes of at most kJpdLutBits bits (0: a longer code).
struct JpdHuff {
  int32_t maxcode[17];
  int32_t valoff[17];
  uint16_t lut[1 << kJpdLutBits];
  uint8_t huffval[256];
};

// maxcode and valoff from BITS; false: not a prefix code of at most 256 symbols
RFX_JPG_HD bool jpd_huff_derive(const uint8_t* bits16, JpdHuff* h) {
  int32_t code = 0, k = 0;
  bool ok = true;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits16[l - 1];
    h->valoff[l] = k - code;
    k += n;
    code += n;
    h->maxcode[l] = n ? code - 1 : -1;
    if (code > (1 << l)) ok = false;
    code <<= 1;
  }
  h->maxcode[0] = -1;
  h->valoff[0] = 0;
  return ok && k <= 256;
}
// the code that starts `window` (32 bits, the first at the top), its length from `from` upwards: length << 8 | symbol, 0: none
RFX_JPG_HD uint32_t jpd_huff_search(const JpdHuff& h, uint32_t window, int from) {
  for (int l = from; l <= 16; ++l) {
    const int32_t code = (int32_t)(window >> (32 - l));
    if (code <= h.maxcode[l]) return ((uint32_t)l << 8) | h.huffval[(code + h.valoff[l]) & 255];
  }
  return 0;
}
RFX_JPG_HD uint16_t jpd_huff_lut_entry(const JpdHuff& h, int index) {
  const uint32_t e = jpd_huff_search(h, (uint32_t)index << (32 - kJpdLutBits), 1);
  return (e >> 8) <= (uint32_t)kJpdLutBits ? (uint16_t)e : (uint16_t)0;
}
RFX_JPG_HD uint32_t jpd_huff_symbol(const JpdHuff& h, uint32_t window) {
  const uint32_t e = h.lut[window >> (32 - kJpdLutBits)];
  return e ? e : jpd_huff_search(h, window, kJpdLutBits + 1);
}
// jdhuff.c's HUFF_EXTEND: the s value bits v of a coefficient
RFX_JPG_HD int jpd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// ---- one subsequence --------------------------------------------------------------------------------------------------------------
// The state between two codewords: the bit position of the next one, the block of the MCU it belongs to (0 .. 3 Y, 4 Cb, 5 Cr)
// and the zigzag index it codes (0: the DC difference).  `valid` is false where a decode from a wrong state ran into an error:
// the decode from the true state replaces it.  Two states are equal when all four fields are.
struct JpdState {
  uint32_t p;
  uint8_t blk, k, valid, pad;
};
RFX_JPG_HD bool jpd_same(const JpdState& a, const JpdState& b) { return a.p == b.p && a.blk == b.blk && a.k == b.k && a.valid == b.valid; }

// Decodes from `in` while the next codeword starts before `end` (<= total_bits) and fewer than max_blocks blocks are complete.
// peek(p): the 32 bits at bit p, the first at the top (bits past total_bits: anything).  emit(block, zigzag index, value) for
// every coefficient coded, block counted from this call's first.  *blocks: blocks completed.  *error: kJpdOk or what stopped it.
// lenient (the rounds that synchronise; the state `in` may be wrong): bits that are no code are skipped one at a time and a run
// past coefficient 63 ends the block, so that the decode goes on and can fall into step with the true one; only the end of the
// bits stops it.  Not lenient (the pass that writes, from true states): each of them is the image's error.
template <bool lenient, typename Peek, typename Emit>
RFX_JPG_HD JpdState jpd_decode_span(const JpdHuff* tables /* DC0 AC0 DC1 AC1 */, Peek&& peek, JpdState in, uint32_t end, uint32_t total_bits,
                                    int64_t max_blocks, Emit&& emit, int64_t* blocks, int* error) {
  uint32_t p = in.p;
  int blk = in.blk, k = in.k;
  int64_t nb = 0;
  int err = kJpdOk;
  while (p < end && nb < max_blocks) {
    const uint32_t w = peek(p);
    const JpdHuff& h = tables[(blk < 4 ? 0 : 2) + (k ? 1 : 0)];
    const uint32_t e = jpd_huff_symbol(h, w);
    const int len = (int)(e >> 8), sym = (int)(e & 255);
    const int s = k ? (sym & 15) : sym, run = k ? (sym >> 4) : 0;
    if (e == 0 || s > (k ? 10 : 11)) {
      if (lenient) {
        ++p;
        continue;
      }
      err = kJpdBadCode;
      break;
    }
    if (p + (uint32_t)(len + s) > total_bits) {
      err = kJpdOutOfBits;
      break;
    }
    bool done = false;
    if (s == 0 && k) {
      if (run == 15) {
        k += 16;
        if (k > 63) {
          if (!lenient) {
            err = kJpdZigzag;
            break;
          }
          done = true;
        }
      } else {
        done = true;  // EOB (jdhuff.c takes any run below 15 with size 0 for it)
      }
    } else {
      k += run;
      if (k > 63) {
        if (!lenient) {
          err = kJpdZigzag;
          break;
        }
        done = true;
      } else {
        if (s) emit(nb, k, jpd_extend((int)((w << len) >> (32 - s)), s));
        done = ++k == 64;
      }
    }
    p += (uint32_t)(len + s);
    if (done) {
      k = 0;
      blk = blk == 5 ? 0 : blk + 1;
      ++nb;
    }
  }
  *blocks = nb;
  *error = err;
  JpdState out;
  out.p = p;
  out.blk = (uint8_t)blk;
  out.k = (uint8_t)k;
  out.valid = err == kJpdOk;
  out.pad = 0;
  return out;
}

// ---- coefficients -> samples ------------------------------------------------------------------------------------------------------
// c: the block's 64 coefficients in natural order (kJpgNatural de-zigzags them when they are stored), q: its table in natural
// order -> the 64 samples 0 .. 255 in c.  jidctint.c; its shortcuts for columns and rows without AC terms give the same values.
RFX_JPG_HD void jpd_idct_1d(int* d, int stride, bool first) {
  constexpr int CB = 13, P1 = 2;
  int z2 = d[2 * stride], z3 = d[6 * stride];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * (-15137), tmp3 = z1 + z2 * 6270;
  z2 = d[0];
  z3 = d[4 * stride];
  int tmp0 = (z2 + z3) * (1 << CB), tmp1 = (z2 - z3) * (1 << CB);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7 * stride];
  tmp1 = d[5 * stride];
  tmp2 = d[3 * stride];
  tmp3 = d[stride];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446;
  tmp1 *= 16819;
  tmp2 *= 25172;
  tmp3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * (-16069) + z5;
  z4 = z4 * (-3196) + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const int sh = first ? CB - P1 : CB + P1 + 3;
  d[0] = RFX_JPG_DESCALE(tmp10 + tmp3, sh);
  d[7 * stride] = RFX_JPG_DESCALE(tmp10 - tmp3, sh);
  d[stride] = RFX_JPG_DESCALE(tmp11 + tmp2, sh);
  d[6 * stride] = RFX_JPG_DESCALE(tmp11 - tmp2, sh);
  d[2 * stride] = RFX_JPG_DESCALE(tmp12 + tmp1, sh);
  d[5 * stride] = RFX_JPG_DESCALE(tmp12 - tmp1, sh);
  d[3 * stride] = RFX_JPG_DESCALE(tmp13 + tmp0, sh);
  d[4 * stride] = RFX_JPG_DESCALE(tmp13 - tmp0, sh);
}
RFX_JPG_HD int jpd_limit(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
template <typename Q>
RFX_JPG_HD void jpd_dequant_idct(int* c, Q q) {
#pragma unroll
  for (int i = 0; i < 64; ++i) c[i] *= (int)q[i];
#pragma unroll
  for (int col = 0; col < 8; ++col) jpd_idct_1d(c + col, 8, true);
#pragma unroll
  for (int r = 0; r < 8; ++r) jpd_idct_1d(c + 8 * r, 1, false);
#pragma unroll
  for (int i = 0; i < 64; ++i) c[i] = jpd_limit(c[i] + 128);
}

// ---- samples -> pixels ------------------------------------------------------------------------------------------------------------

// one chroma sample of output pixel (x, y), plane c (8 mcu_h rows of cstride)
template <typename Px>
RFX_JPG_HD int jpd_upsample(Px c, int cstride, int H, int W, int x, int y) {
  const int cw = (W + 1) / 2, ch = (H + 1) / 2;
  const int cx = x >> 1, cy = y >> 1;
  if (cw <= 2) return c[(int64_t)cy * cstride + cx];  // jdsample.c: no more than two chroma columns are replicated, not filtered
  int ny = (y & 1) ? cy + 1 : cy - 1;  // the further row
  ny = ny < 0 ? 0 : (ny > ch - 1 ? ch - 1 : ny);
  const Px near = c + (int64_t)cy * cstride, far = c + (int64_t)ny * cstride;
  const int cur = 3 * near[cx] + far[cx];
  if (x & 1) return cx == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

// jdcolor.c: FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414) at 16 bits
RFX_JPG_HD void jpd_rgb(int y, int cb, int cr, uint8_t* rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = (uint8_t)jpd_limit(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = (uint8_t)jpd_limit(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  rgb[2] = (uint8_t)jpd_limit(y + ((116130 * cb + 32768) >> 16));
}

}  // namespace rfx
