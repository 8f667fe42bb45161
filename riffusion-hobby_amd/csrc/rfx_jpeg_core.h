// rfx_jpeg_core.h - baseline JPEG as Pillow writes an RGB image (`Image.save(f, "JPEG", quality=q)`: libjpeg's defaults - YCbCr
// 4:2:0, the Annex K tables, the slow integer DCT, no restart markers), written once for the gfx950 kernels (rfx_jpeg.hip, hipcc)
// and the host emulator of the CPU tests (tests/emu/rfx_jpeg_emu.cpp, g++).  Every step is integer arithmetic:
//   * colour: jccolor.c's 16-bit fixed point, FIX(x) = int(x * 65536 + 0.5) (jpg_ycc);
//   * planes: Y at full resolution; Cb and Cr the mean of 2 x 2 pixels with the bias 1, 2, 1, 2, ... along the output columns
//     (jcsample.c h2v2_downsample).  Past the right edge the last PIXEL column is replicated, past the bottom the last pixel row
//     up to an even height only, and then the last CHROMA row: the downsampler pads its input, the preprocessor its output;
//   * blocks: the MCU is 16 x 16 pixels, its blocks in the order Y00 Y01 Y10 Y11 Cb Cr.  A Y block that lies wholly past
//     ceil(W / 8) columns or ceil(H / 8) rows is not computed from pixels: it is a dummy (jccoefct.c), all AC zero and the DC of
//     the block before it in its MCU - so its DC difference is always 0;
//   * transform: level shift by -128, jfdctint.c (CONST_BITS 13, PASS1_BITS 2; the result is 8 x the DCT), then the division by
//     8 q rounded half away from zero;
//   * entropy coding: jchuff.c with the Annex K tables - DC as the difference to the previous block of the same component in
//     scan order, AC as run / size with ZRL and EOB, a negative value as the low bits of v - 1; the scan is padded with 1 bits
//     to a byte and every 0xFF byte is followed by 0x00.
// The device computes a block's bit count and its bits with the one walker (jpg_walk_dc / jpg_walk_ac), so the offsets of the
// scan and the packing cannot disagree.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RFX_JPG_HD __host__ __device__ __forceinline__
#else
#define RFX_JPG_HD inline __attribute__((always_inline))
#endif

namespace rfx {

constexpr int kJpgMaxSize = 65535;  // per axis: SOF0 holds 16 bits
// The longest code of one coefficient.  DC: the longest DC code is 11 bits (chroma, category 11) and carries 11 value bits: 22.
// AC: the longest AC code is 16 bits and a baseline coefficient has at most 10 value bits: 26 for each of the 63 (a ZRL or an EOB
// stands for coefficients that are then not coded, at 11 / 4 bits for 16 / at least 1 of them: less than coding them).
constexpr int kJpgBlockMaxBits = 22 + 63 * 26;  // 1660

// ---- tables ---------------------------------------------------------------------------------------------------------------
// ITU T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the four typical tables, as in the DHT segments Pillow writes
struct JpgHuffSpec {
  uint8_t bits[16];
  uint8_t vals[162];
};
constexpr JpgHuffSpec kJpgDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpgHuffSpec kJpgDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpgHuffSpec kJpgAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr JpgHuffSpec kJpgAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> (code << 8) | length, Annex C's code assignment; length 0: the table has no such symbol
struct JpgHuffTable {
  uint32_t e[256];
};
constexpr JpgHuffTable jpg_huff_table(const JpgHuffSpec& s) {
  JpgHuffTable t{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i) t.e[s.vals[k++]] = (code++ << 8) | (uint32_t)len;
    code <<= 1;
  }
  return t;
}
// [0] the luma tables, [1] the chroma tables (Cb and Cr)
struct JpgTables {
  JpgHuffTable dc[2], ac[2];
};
constexpr JpgTables kJpgTables = {{jpg_huff_table(kJpgDcLuma), jpg_huff_table(kJpgDcChroma)},
                                  {jpg_huff_table(kJpgAcLuma), jpg_huff_table(kJpgAcChroma)}};

// zigzag position -> natural (row-major) index
constexpr uint8_t kJpgNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 quantisation tables, natural order
constexpr uint8_t kJpgQuantLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                       14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                       18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kJpgQuantChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jcparam.c jpeg_quality_scaling + jpeg_add_quant_table with force_baseline: natural order, 1..255.  quality in 1..100.  Host.
inline void jpg_quant_tables(int quality, uint16_t* luma64, uint16_t* chroma64) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const int a = ((int)kJpgQuantLuma[i] * scale + 50) / 100, b = ((int)kJpgQuantChroma[i] * scale + 50) / 100;
    luma64[i] = (uint16_t)(a < 1 ? 1 : (a > 255 ? 255 : a));
    chroma64[i] = (uint16_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
  }
}

// ---- geometry --------------------------------------------------------------------------------------------------------------
// The blocks of an image are numbered in scan order: block b = 6 * mcu + k, mcu = my * mcu_w + mx, k = 0..3 Y (row-major in the
// MCU), 4 Cb, 5 Cr.
struct JpgGeom {
  int H, W;
  int mcu_w, mcu_h;  // ceil(W / 16), ceil(H / 16)
  int ybw, ybh;      // Y blocks that hold pixels: ceil(W / 8), ceil(H / 8)
  int64_t mcus;      // mcu_w * mcu_h
  int64_t blocks;    // 6 * mcus
};
RFX_JPG_HD JpgGeom jpg_geom(int H, int W) {
  JpgGeom g;
  g.H = H;
  g.W = W;
  g.mcu_w = (W + 15) / 16;
  g.mcu_h = (H + 15) / 16;
  g.ybw = (W + 7) / 8;
  g.ybh = (H + 7) / 8;
  g.mcus = (int64_t)g.mcu_w * g.mcu_h;
  g.blocks = 6 * g.mcus;
  return g;
}
// bytes of one image's scan before stuffing, at most: every block at kJpgBlockMaxBits, and the padding to a byte
RFX_JPG_HD uint64_t jpg_unstuffed_capacity(const JpgGeom& g) { return ((uint64_t)g.blocks * kJpgBlockMaxBits + 7) / 8; }
// ... and after it, with EOI: every byte could be 0xFF and get its 0x00
RFX_JPG_HD uint64_t jpg_scan_capacity(const JpgGeom& g) { return 2 * jpg_unstuffed_capacity(g) + 2; }

RFX_JPG_HD bool jpg_is_dummy(const JpgGeom& g, int64_t mcu, int k) {
  if (k >= 4) return false;
  const int mx = (int)(mcu % g.mcu_w), my = (int)(mcu / g.mcu_w);
  return 2 * mx + (k & 1) >= g.ybw || 2 * my + (k >> 1) >= g.ybh;
}

// ---- pixels -> samples ------------------------------------------------------------------------------------------------------
constexpr int kJpgFix299 = 19595, kJpgFix587 = 38470, kJpgFix114 = 7471, kJpgFix16874 = 11059, kJpgFix33126 = 21709,
              kJpgFix5 = 32768, kJpgFix41869 = 27439, kJpgFix08131 = 5329;
constexpr int kJpgHalf = 32768, kJpgOff = 128 << 16;

// component c (0 Y, 1 Cb, 2 Cr) of one pixel
RFX_JPG_HD int jpg_ycc(int c, int r, int g, int b) {
  if (c == 0) return (kJpgFix299 * r + kJpgFix587 * g + kJpgFix114 * b + kJpgHalf) >> 16;
  if (c == 1) return (-kJpgFix16874 * r - kJpgFix33126 * g + kJpgFix5 * b + kJpgOff + kJpgHalf - 1) >> 16;
  return (kJpgFix5 * r - kJpgFix41869 * g - kJpgFix08131 * b + kJpgOff + kJpgHalf - 1) >> 16;
}

// the 64 level-shifted samples of Y block (bx, by) of an (H, W, 3) image
template <typename Px>
RFX_JPG_HD void jpg_samples_y(Px rgb, int H, int W, int bx, int by, int* s) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int y = by * 8 + r;
    y = y < H ? y : H - 1;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int x = bx * 8 + c;
      x = x < W ? x : W - 1;
      const int64_t p = ((int64_t)y * W + x) * 3;
      s[r * 8 + c] = jpg_ycc(0, rgb[p], rgb[p + 1], rgb[p + 2]) - 128;
    }
  }
}

// the 64 level-shifted samples of the chroma block of MCU (mx, my), component comp (1 Cb, 2 Cr)
template <typename Px>
RFX_JPG_HD void jpg_samples_c(Px rgb, int H, int W, int mx, int my, int comp, int* s) {
  const int crows = (H + 1) / 2;  // chroma rows made of pixels (the last of an odd height from its one row, twice)
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int cy = my * 8 + r;
    cy = cy < crows ? cy : crows - 1;
    const int y0 = 2 * cy, y1 = 2 * cy + 1 < H ? 2 * cy + 1 : H - 1;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int cx = mx * 8 + c;
      const int x0 = 2 * cx < W ? 2 * cx : W - 1, x1 = 2 * cx + 1 < W ? 2 * cx + 1 : W - 1;
      const int64_t p00 = ((int64_t)y0 * W + x0) * 3, p01 = ((int64_t)y0 * W + x1) * 3, p10 = ((int64_t)y1 * W + x0) * 3,
                    p11 = ((int64_t)y1 * W + x1) * 3;
      const int sum = jpg_ycc(comp, rgb[p00], rgb[p00 + 1], rgb[p00 + 2]) + jpg_ycc(comp, rgb[p01], rgb[p01 + 1], rgb[p01 + 2]) +
                      jpg_ycc(comp, rgb[p10], rgb[p10 + 1], rgb[p10 + 2]) + jpg_ycc(comp, rgb[p11], rgb[p11 + 1], rgb[p11 + 2]);
      s[r * 8 + c] = ((sum + 1 + (cx & 1)) >> 2) - 128;
    }
  }
}

// ---- forward DCT and quantisation --------------------------------------------------------------------------------------------
#define RFX_JPG_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))
// one pass of jfdctint.c over eight values `stride` apart; first: the row pass (results scaled up by 2^PASS1_BITS)
RFX_JPG_HD void jpg_fdct_1d(int* d, int stride, bool first) {
  constexpr int CB = 13, P1 = 2;
  const int t0 = d[0] + d[7 * stride], t7 = d[0] - d[7 * stride], t1 = d[stride] + d[6 * stride], t6 = d[stride] - d[6 * stride];
  const int t2 = d[2 * stride] + d[5 * stride], t5 = d[2 * stride] - d[5 * stride], t3 = d[3 * stride] + d[4 * stride],
            t4 = d[3 * stride] - d[4 * stride];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int sh = first ? CB - P1 : CB + P1;
  if (first) {
    d[0] = (t10 + t11) << P1;
    d[4 * stride] = (t10 - t11) << P1;
  } else {
    d[0] = RFX_JPG_DESCALE(t10 + t11, P1);
    d[4 * stride] = RFX_JPG_DESCALE(t10 - t11, P1);
  }
  int z1 = (t12 + t13) * 4433;
  d[2 * stride] = RFX_JPG_DESCALE(z1 + t13 * 6270, sh);
  d[6 * stride] = RFX_JPG_DESCALE(z1 + t12 * (-15137), sh);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * (-16069) + z5;
  z4 = z4 * (-3196) + z5;
  d[7 * stride] = RFX_JPG_DESCALE(a4 + z1 + z3, sh);
  d[5 * stride] = RFX_JPG_DESCALE(a5 + z2 + z4, sh);
  d[3 * stride] = RFX_JPG_DESCALE(a6 + z2 + z3, sh);
  d[stride] = RFX_JPG_DESCALE(a7 + z1 + z4, sh);
}
RFX_JPG_HD void jpg_fdct(int* s) {
#pragma unroll
  for (int r = 0; r < 8; ++r) jpg_fdct_1d(s + 8 * r, 1, true);
#pragma unroll
  for (int c = 0; c < 8; ++c) jpg_fdct_1d(s + c, 8, false);
}
// a DCT output (8 x the coefficient) over the table entry q: round half away from zero
RFX_JPG_HD int jpg_quantise(int c, int q) {
  const int qv = q * 8, a = c < 0 ? -c : c;
  const int t = (a + (qv >> 1)) / qv;
  return c < 0 ? -t : t;
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------
// the size category of a value: bits of its magnitude
RFX_JPG_HD int jpg_nbits(int v) {
  const unsigned a = (unsigned)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}
// `put(bits, length)` receives every code together with its value bits: the DC difference ...
template <typename Put>
RFX_JPG_HD void jpg_walk_dc(const JpgTables& t, int tab, int diff, Put&& put) {
  const int s = jpg_nbits(diff);
  const uint32_t e = t.dc[tab].e[s];
  const uint32_t v = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1);
  put(((e >> 8) << s) | v, (int)(e & 255) + s);
}
// ... and the 63 AC coefficients zz[1..63] in zigzag order (zz == nullptr: all zero).  Returns the number of ZRLs.
template <typename Zz, typename Put>
RFX_JPG_HD int jpg_walk_ac(const JpgTables& t, int tab, Zz zz, bool all_zero, Put&& put) {
  int run = 0, zrl = 0;
  if (!all_zero) {
    for (int k = 1; k < 64; ++k) {
      const int v = zz[k];
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        const uint32_t e = t.ac[tab].e[0xF0];
        put(e >> 8, (int)(e & 255));
        run -= 16;
        ++zrl;
      }
      const int s = jpg_nbits(v);
      const uint32_t e = t.ac[tab].e[(run << 4) | s];
      put(((e >> 8) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), (int)(e & 255) + s);
      run = 0;
    }
  } else {
    run = 63;
  }
  if (run > 0) {
    const uint32_t e = t.ac[tab].e[0x00];
    put(e >> 8, (int)(e & 255));
  }
  return zrl;
}

// The DC difference block (mcu, k) codes.  coef: the image's blocks, 64 int16 each in zigzag order (dummy blocks are not
// stored: a dummy carries the DC of the block before it in its MCU, and block 0 of an MCU is never one).
template <typename Coef>
RFX_JPG_HD int jpg_dc_diff(const JpgGeom& g, Coef coef, int64_t mcu, int k) {
  if (jpg_is_dummy(g, mcu, k)) return 0;
  const int dc = coef[(mcu * 6 + k) * 64];
  int64_t pm = mcu;
  int pk = k - 1;
  if (k == 0 || k >= 4) {
    if (mcu == 0) return dc;
    pm = mcu - 1;
    pk = k == 0 ? 3 : k;
  }
  while (pk > 0 && pk < 4 && jpg_is_dummy(g, pm, pk)) --pk;
  return dc - coef[(pm * 6 + pk) * 64];
}

// ---- packing bits into the unstuffed stream ---------------------------------------------------------------------------------
// The stream is bytes, most significant bit first; it is written as 32-bit words whose bytes are in stream order.  A block
// starts at any bit: its first and its last word may be shared with its neighbours and are merged with `merge(index, word)` (an
// OR into zeroed memory); the words between are the block's alone and go to `store(index, word)`.
RFX_JPG_HD uint32_t jpg_stream_word(uint32_t msb_first) { return __builtin_bswap32(msb_first); }
template <typename Merge, typename Store>
struct JpgBitSink {
  Merge merge;
  Store store;
  uint64_t acc = 0;
  int fill;
  int64_t word;
  bool first = true;
  RFX_JPG_HD JpgBitSink(uint64_t bit_offset, Merge m, Store s) : merge(m), store(s), fill((int)(bit_offset & 31)), word((int64_t)(bit_offset >> 5)) {}
  RFX_JPG_HD void operator()(uint32_t bits, int len) {  // len <= 27, fill < 32
    acc = (acc << len) | bits;
    fill += len;
    if (fill >= 32) {
      const uint32_t w = jpg_stream_word((uint32_t)(acc >> (fill - 32)));
      if (first) merge(word, w);
      else store(word, w);
      first = false;
      ++word;
      fill -= 32;
    }
  }
  RFX_JPG_HD void finish() {
    if (fill > 0) merge(word, jpg_stream_word((uint32_t)(acc << (32 - fill))));
  }
};

}  // namespace rfx
