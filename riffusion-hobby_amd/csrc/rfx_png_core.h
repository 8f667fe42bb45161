// rfx_png_core.h - the IDAT payload of a lossless PNG tile (a zlib stream), written once for the gfx950 kernels (rfx_png.hip, hipcc)
// and the host emulator of the CPU tests (tests/emu/rfx_png_emu.cpp, g++).  The stream is not zlib's: it is a run-length + Huffman
// deflate (zlib's Z_RLE class) every step of which is a function of the tile alone, integer throughout, so that the device's bytes
// and the emulator's are the same bytes.  Any inflate reads it.
//   * tile: (H, W, 3) uint8, written with `channels` 3 (colour type 2) or 1 (colour type 0, channel 0 of a tile whose three
//     channels are equal at every pixel); bit depth 8, no interlace.  A row is W * channels bytes after its filter byte.
//   * filtering: every row on its own, from the UNFILTERED row above (zeros above row 0, and left of the first pixel).  All five
//     filters (None, Sub, Up, Average, Paeth) are tried; the cost of one is the sum over the row's W * channels filtered bytes of
//     |byte as int8| (the filter byte is not counted); the least cost wins, a tie goes to the lowest filter type.
//   * blocks: the filtered stream (filter byte, then the row) is cut every kPngBlockRows = 32 rows; the last block may be shorter.
//   * tokens: inside a block take each maximal run of equal bytes (a filter byte is a byte like any other; runs end at the block's
//     end).  The run's first byte is a literal.  The rest are matches at distance 1 of min(258, what is left) bytes while at least
//     3 bytes are left; what is then left (1 or 2 bytes) are literals.  No other match is used.
//   * codes: one dynamic-Huffman block per block.  The literal/length code is built from the block's histogram (its tokens and one
//     end-of-block) by png_code_lengths: the used symbols sorted by (count, symbol) ascending; Huffman's tree by the two-queue
//     method, a leaf before an internal node of equal weight; leaf depths above the limit are set to it and the count of codes per
//     length is repaired one unit of 2^-limit at a time (drop a code of the limit's length, split the deepest shorter code into two
//     one bit longer) until the Kraft sum is exactly 1; lengths are then dealt longest first along the sorted order, so among equal
//     counts the lower symbol gets the longer code.  Limit 15 over 286 symbols; the code-length code is built the same way, limit 7
//     over 19.  Codes are the canonical ones of RFC 1951 3.2.2, stored bit-reversed because deflate packs LSB-first.
//   * distance code: HDIST = 0, one code; its length is 1 (code `0`) in a block with a match, 0 in a block without.
//   * block header: BFINAL, BTYPE = 2, HLIT = 29 (all 286), HDIST = 0, HCLEN = 15 (all 19), then the 287 lengths run-length coded by
//     png_rle_lengths: a run of zeros as 18s of up to 138 while 11 or more remain, then one 17 for 3 .. 10, else plain zeros; a run
//     of another length as the length once, 16s of up to 6 while 3 or more remain, then the length itself.
//   * blocks follow one another at bit granularity after the zlib header 78 9C; the last has BFINAL, is padded with zero bits to a
//     byte and is followed by the Adler-32 of the filtered stream, big-endian.
//   * checksums in pieces: Adler-32 from per-row sums (png_adler_*), CRC-32 from per-piece CRCs multiplied by x^(8 * bytes after
//     the piece) mod P (png_crc_*).  Both combinations are sums (mod 65521, XOR), so the order of the pieces does not matter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RFX_PNG_HD __host__ __device__ __forceinline__
#else
#define RFX_PNG_HD inline __attribute__((always_inline))
#endif

namespace rfx {

constexpr int kPngMaxSize = 65535;    // per axis (the entry's limit; IHDR itself holds 31 bits)
constexpr int kPngBlockRows = 32;     // rows of the filtered stream per deflate block
constexpr int kPngLitLen = 286;       // literal/length symbols; 256 is end-of-block
constexpr int kPngEob = 256;
constexpr int kPngLens = 287;         // lengths in a block header: 286 literal/length and the one distance code
constexpr int kPngDist = 286;         // ... the index of the distance code's length in that sequence
constexpr int kPngMaxBits = 15;       // longest literal/length code
constexpr int kPngClSyms = 19;        // symbols of the code-length code
constexpr int kPngClMaxBits = 7;      // its longest code
constexpr int kPngMaxMatch = 258, kPngMinMatch = 3;
constexpr int kPngTokenMaxBits = kPngMaxBits + 5 + 1;  // a match: length code, its extra bits, the distance code
// a block header at most: BFINAL + BTYPE, HLIT + HDIST + HCLEN, 19 lengths of 3 bits, and for each of the 287 lengths at most one
// code-length symbol of 7 bits with 7 extra bits (a repeat symbol stands for 3 or more lengths: fewer symbols)
constexpr int kPngHeaderMaxBits = 3 + 14 + kPngClSyms * 3 + kPngLens * (kPngClMaxBits + 7);  // 4092
constexpr int kPngHeaderWords = (kPngHeaderMaxBits + 31) / 32;                               // 128

// ---- geometry ----------------------------------------------------------------------------------------------------------------
struct PngGeom {
  int H, W, ch;
  int64_t row;    // filtered bytes of a row: W * ch + 1
  int64_t bytes;  // the filtered stream: H * row
  int blocks;     // ceil(H / kPngBlockRows)
};
RFX_PNG_HD PngGeom png_geom(int H, int W, int ch) {
  PngGeom g;
  g.H = H;
  g.W = W;
  g.ch = ch;
  g.row = (int64_t)W * ch + 1;
  g.bytes = (int64_t)H * g.row;
  g.blocks = (H + kPngBlockRows - 1) / kPngBlockRows;
  return g;
}
// Bytes of one tile's zlib stream at most.  A token costs at most 15 bits per byte it covers: a literal is one code of at most 15
// bits for 1 byte, a match at most 15 + 5 + 1 = 21 bits for at least 3.  So a block of b bytes takes at most kPngHeaderMaxBits +
// 15 b + 15 (its end-of-block) bits, the blocks together blocks * (4092 + 15) + 15 * bytes, and the stream 2 bytes of zlib header,
// those bits padded to a byte, and 4 bytes of Adler-32.  No stored or fixed-Huffman block is needed for the bound to hold.
RFX_PNG_HD uint64_t png_stream_capacity(const PngGeom& g) {
  const uint64_t bits = (uint64_t)g.blocks * (kPngHeaderMaxBits + kPngMaxBits) + (uint64_t)kPngMaxBits * (uint64_t)g.bytes;
  return 2 + (bits + 7) / 8 + 4;
}

// ---- filtering ------------------------------------------------------------------------------------------------------------------
RFX_PNG_HD int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// filter `type` of byte x with a to its left, b above and c above-left
RFX_PNG_HD int png_filter_byte(int type, int x, int a, int b, int c) {
  const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
  return (x - pred) & 255;
}
RFX_PNG_HD int png_filter_cost(int f) { return f < 128 ? f : 256 - f; }
// byte j of row y of the tile as it is written with ch channels
template <typename Px>
RFX_PNG_HD int png_source_byte(Px rgb, int W, int ch, int y, int64_t j) {
  return ch == 1 ? rgb[((int64_t)y * W + j) * 3] : rgb[(int64_t)y * W * 3 + j];
}
// the five filtered values of byte j of row y
template <typename Px>
RFX_PNG_HD void png_filter_all(Px rgb, int W, int ch, int y, int64_t j, int* f0, int* f1, int* f2, int* f3, int* f4) {
  const int x = png_source_byte(rgb, W, ch, y, j);
  const int a = j >= ch ? png_source_byte(rgb, W, ch, y, j - ch) : 0;
  const int b = y > 0 ? png_source_byte(rgb, W, ch, y - 1, j) : 0;
  const int c = (y > 0 && j >= ch) ? png_source_byte(rgb, W, ch, y - 1, j - ch) : 0;
  *f0 = x;
  *f1 = (x - a) & 255;
  *f2 = (x - b) & 255;
  *f3 = (x - ((a + b) >> 1)) & 255;
  *f4 = (x - png_paeth(a, b, c)) & 255;
}
template <typename Px>
RFX_PNG_HD int png_filter_one(Px rgb, int W, int ch, int y, int64_t j, int type) {
  const int x = png_source_byte(rgb, W, ch, y, j);
  const int a = j >= ch ? png_source_byte(rgb, W, ch, y, j - ch) : 0;
  const int b = y > 0 ? png_source_byte(rgb, W, ch, y - 1, j) : 0;
  const int c = (y > 0 && j >= ch) ? png_source_byte(rgb, W, ch, y - 1, j - ch) : 0;
  return png_filter_byte(type, x, a, b, c);
}
// least cost, ties to the lowest type
RFX_PNG_HD int png_choose_filter(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4) {
  int best = 0;
  uint32_t cost = c0;
  if (c1 < cost) { best = 1; cost = c1; }
  if (c2 < cost) { best = 2; cost = c2; }
  if (c3 < cost) { best = 3; cost = c3; }
  if (c4 < cost) { best = 4; cost = c4; }
  return best;
}

// ---- tokens -----------------------------------------------------------------------------------------------------------------------
// length 3 .. 258 -> its symbol 257 .. 285, and the extra bits that follow the code
RFX_PNG_HD int png_length_symbol(int length, int* extra, int* extra_bits) {
  *extra = 0;
  *extra_bits = 0;
  if (length == kPngMaxMatch) return 285;
  const int l = length - kPngMinMatch;
  if (l < 8) return 257 + l;
  const int e = (31 - __builtin_clz((unsigned)l)) - 2;
  *extra = l & ((1 << e) - 1);
  *extra_bits = e;
  return 261 + 4 * e + ((l >> e) & 3);
}
RFX_PNG_HD int png_symbol_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// The token that starts at byte i of a block of n bytes, k bytes after the first byte of its run: 0 none (the byte lies inside
// a match), 1 a literal, 2 a match of *length.  byte(i): the block's bytes.
template <typename B>
RFX_PNG_HD int png_token(B&& byte, int64_t i, int64_t n, int64_t k, int* length) {
  *length = 0;
  if (k == 0) return 1;
  const int p = (int)((k - 1) % kPngMaxMatch);  // place in its piece of the run's rest
  if (p >= 2) return 0;                         // (a piece that holds places 0, 1 and 2 is a match)
  const int v = byte(i);
  if (p == 1) return (i + 1 < n && byte(i + 1) == v) ? 0 : 1;
  if (!(i + 2 < n && byte(i + 1) == v && byte(i + 2) == v)) return 1;
  int len = 3;
  while (len < kPngMaxMatch && i + len < n && byte(i + len) == v) ++len;
  *length = len;
  return 2;
}

// ---- code construction ---------------------------------------------------------------------------------------------------------
// working storage of the code builder (LDS on the device: nothing here is indexed in registers)
struct PngScratch {
  uint32_t counts[288];  // the histogram being coded
  uint32_t w[576];       // weights: leaves in sorted order, then the internal nodes in the order they are made
  uint16_t parent[576];
  uint16_t depth[576];
  uint16_t sorted[288];  // used symbols by (count, symbol) ascending
  uint16_t num[32];      // codes per length
  uint16_t next[32];
};
struct PngBlockCodes {
  uint8_t lens[288];    // [0, 286) literal/length, [286] the distance code
  uint16_t codes[288];  // bit-reversed
  uint8_t cl_lens[20];
  uint16_t cl_codes[20];
};

// place of symbol s among the used symbols of counts[0 .. nsym) by (count, symbol)
RFX_PNG_HD int png_rank(const uint32_t* counts, int nsym, int s) {
  const uint32_t c = counts[s];
  int r = 0;
  for (int t = 0; t < nsym; ++t) {
    const uint32_t o = counts[t];
    r += (o != 0 && (o < c || (o == c && t < s))) ? 1 : 0;
  }
  return r;
}

// sc.counts[0 .. nsym) and sc.sorted[0 .. n) (n >= 1 used symbols) -> lens[0 .. nsym), none above `limit`, Kraft sum exactly 1.
// One used symbol gets a companion (symbol 0, or 1 when it is 0 itself), both 1 bit: a code of one symbol alone is incomplete.
RFX_PNG_HD void png_code_lengths(PngScratch& sc, int nsym, int n, int limit, uint8_t* lens) {
  for (int s = 0; s < nsym; ++s) lens[s] = 0;
  if (n == 1) {
    const int s0 = sc.sorted[0];
    lens[s0] = 1;
    lens[s0 == 0 ? 1 : 0] = 1;
    return;
  }
  for (int i = 0; i < n; ++i) sc.w[i] = sc.counts[sc.sorted[i]];
  int li = 0, ii = n;
  for (int node = n; node < 2 * n - 1; ++node) {
    uint32_t sum = 0;
    for (int t = 0; t < 2; ++t) {
      const bool leaf = li < n && (ii >= node || sc.w[li] <= sc.w[ii]);
      const int pick = leaf ? li++ : ii++;
      sc.parent[pick] = (uint16_t)node;
      sum += sc.w[pick];
    }
    sc.w[node] = sum;
  }
  for (int l = 0; l <= limit; ++l) sc.num[l] = 0;
  sc.depth[2 * n - 2] = 0;
  for (int j = 2 * n - 3; j >= 0; --j) {
    const int d = sc.depth[sc.parent[j]] + 1;
    sc.depth[j] = (uint16_t)d;
    if (j < n) sc.num[d < limit ? d : limit] += 1;
  }
  uint32_t total = 0;  // Kraft sum in units of 2^-limit
  for (int l = 1; l <= limit; ++l) total += (uint32_t)sc.num[l] << (limit - l);
  while (total > (1u << limit)) {
    sc.num[limit] -= 1;
    for (int l = limit - 1; l > 0; --l)
      if (sc.num[l]) {
        sc.num[l] -= 1;
        sc.num[l + 1] += 2;
        break;
      }
    total -= 1;
  }
  int at = 0;
  for (int l = limit; l >= 1; --l)
    for (int c = sc.num[l]; c > 0; --c) lens[sc.sorted[at++]] = (uint8_t)l;
}

RFX_PNG_HD uint32_t png_reverse_bits(uint32_t c, int len) {
  c = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
  c = ((c & 0x3333u) << 2) | ((c >> 2) & 0x3333u);
  c = ((c & 0x0F0Fu) << 4) | ((c >> 4) & 0x0F0Fu);
  c = ((c & 0x00FFu) << 8) | ((c >> 8) & 0x00FFu);
  return c >> (16 - len);
}
// RFC 1951 3.2.2, bit-reversed
RFX_PNG_HD void png_assign_codes(PngScratch& sc, const uint8_t* lens, int nsym, int limit, uint16_t* codes) {
  for (int l = 0; l <= limit; ++l) sc.num[l] = 0;
  for (int s = 0; s < nsym; ++s) sc.num[lens[s]] += 1;
  sc.num[0] = 0;
  uint32_t code = 0;
  for (int l = 1; l <= limit; ++l) {
    code = (code + sc.num[l - 1]) << 1;
    sc.next[l] = (uint16_t)code;
  }
  for (int s = 0; s < nsym; ++s) {
    const int l = lens[s];
    uint32_t c = 0;
    if (l) {
      c = sc.next[l];
      sc.next[l] = (uint16_t)(c + 1);
      c = png_reverse_bits(c, l);
    }
    codes[s] = (uint16_t)c;
  }
}

// the lengths of a block header as code-length symbols: emit(symbol, extra, extra_bits)
template <typename Emit>
RFX_PNG_HD void png_rle_lengths(const uint8_t* lens, int n, Emit&& emit) {
  int i = 0;
  while (i < n) {
    const int v = lens[i];
    int r = 1;
    while (i + r < n && lens[i + r] == v) ++r;
    i += r;
    if (v == 0) {
      while (r >= 11) {
        const int t = r < 138 ? r : 138;
        emit(18, t - 11, 7);
        r -= t;
      }
      if (r >= 3) {
        emit(17, r - 3, 3);
        r = 0;
      }
      for (; r > 0; --r) emit(0, 0, 0);
    } else {
      emit(v, 0, 0);
      --r;
      while (r >= 3) {
        const int t = r < 6 ? r : 6;
        emit(16, t - 3, 2);
        r -= t;
      }
      for (; r > 0; --r) emit(v, 0, 0);
    }
  }
}

// HCLEN's order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
RFX_PNG_HD int png_cl_order(int k) {
  const uint64_t lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) |
                      (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
  const uint64_t hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
  return (int)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31);
}

// The codes of one block from its histogram: sc.counts[0 .. 286) (the tokens and one end-of-block) with sc.sorted[0 .. n) already
// in place.  Returns the bits of the block's tokens and end-of-block (without the header).
RFX_PNG_HD uint32_t png_block_codes(PngScratch& sc, int n, PngBlockCodes& bc) {
  png_code_lengths(sc, kPngLitLen, n, kPngMaxBits, bc.lens);
  uint32_t matches = 0, bits = 0;
  for (int s = 0; s < kPngLitLen; ++s) {
    bits += sc.counts[s] * (uint32_t)(bc.lens[s] + png_symbol_extra_bits(s));
    if (s > kPngEob) matches += sc.counts[s];
  }
  bc.lens[kPngDist] = matches ? 1 : 0;
  bc.lens[kPngDist + 1] = 0;
  png_assign_codes(sc, bc.lens, kPngLitLen, kPngMaxBits, bc.codes);
  bc.codes[kPngDist] = 0;
  bc.codes[kPngDist + 1] = 0;
  return bits + matches;
}

// The block's header through put(bits, count) (LSB-first; count <= 15).  Overwrites sc.counts.
template <typename Put>
RFX_PNG_HD void png_block_header(PngScratch& sc, PngBlockCodes& bc, bool final, Put&& put) {
  for (int s = 0; s < kPngClSyms; ++s) sc.counts[s] = 0;
  png_rle_lengths(bc.lens, kPngLens, [&](int sym, int, int) { sc.counts[sym] += 1; });
  int n = 0;
  for (int s = 0; s < kPngClSyms; ++s)
    if (sc.counts[s]) {
      sc.sorted[png_rank(sc.counts, kPngClSyms, s)] = (uint16_t)s;
      ++n;
    }
  png_code_lengths(sc, kPngClSyms, n, kPngClMaxBits, bc.cl_lens);
  png_assign_codes(sc, bc.cl_lens, kPngClSyms, kPngClMaxBits, bc.cl_codes);
  put(final ? 1u : 0u, 1);
  put(2u, 2);
  put((uint32_t)(kPngLitLen - 257), 5);
  put(0u, 5);
  put((uint32_t)(kPngClSyms - 4), 4);
  for (int k = 0; k < kPngClSyms; ++k) put(bc.cl_lens[png_cl_order(k)], 3);
  png_rle_lengths(bc.lens, kPngLens, [&](int sym, int extra, int extra_bits) {
    put(bc.cl_codes[sym], bc.cl_lens[sym]);
    if (extra_bits) put((uint32_t)extra, extra_bits);
  });
}

// ---- Adler-32 in rows ------------------------------------------------------------------------------------------------------------
// A row of R bytes d_0 .. d_{R-1} gives a = sum d_j and b = sum (R - j) d_j, both mod 65521.  With the rows r = 0 .. H - 1 of a
// stream of n = H R bytes:  A = 1 + sum a_r,  B = n + sum (b_r + (n - (r + 1) R) a_r), and the checksum is B << 16 | A.
constexpr uint32_t kPngAdlerMod = 65521;
RFX_PNG_HD uint32_t png_adler_row_term(uint32_t a, uint32_t b, int64_t bytes_after_row) {
  return (uint32_t)((b + (uint64_t)(bytes_after_row % kPngAdlerMod) * a) % kPngAdlerMod);
}
RFX_PNG_HD uint32_t png_adler_finish(uint32_t sum_a, uint32_t sum_terms, int64_t n) {
  const uint32_t A = (1 + sum_a) % kPngAdlerMod, B = (uint32_t)((n % kPngAdlerMod + sum_terms) % kPngAdlerMod);
  return (B << 16) | A;
}

// ---- CRC-32 in pieces ---------------------------------------------------------------------------------------------------------
// Polynomials over GF(2) mod P, reflected as in the CRC itself: bit 31 is x^0.  crc(A || B) = crc(A) x^(8 |B|) + crc(B) for the
// finished CRCs (the initial value and the final inversion cancel), so a message's CRC is the XOR of its pieces' CRCs, each
// multiplied by x^(8 * bytes after the piece).
constexpr uint32_t kPngCrcPoly = 0xEDB88320u;
RFX_PNG_HD constexpr uint32_t png_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kPngCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 * 2^k), k = 0 .. 31
struct PngCrcPowers {
  uint32_t p[32];
};
constexpr PngCrcPowers png_crc_powers() {
  PngCrcPowers t{};
  uint32_t v = 0x00800000u;  // x^8
  for (int k = 0; k < 32; ++k) {
    t.p[k] = v;
    v = png_crc_mul(v, v);
  }
  return t;
}
constexpr PngCrcPowers kPngCrcPowers = png_crc_powers();
// crc * x^(8 * bytes)
RFX_PNG_HD uint32_t png_crc_shift(uint32_t crc, uint64_t bytes, const PngCrcPowers& t) {
  for (int k = 0; bytes; ++k, bytes >>= 1)
    if (bytes & 1) crc = png_crc_mul(t.p[k & 31], crc);
  return crc;
}
RFX_PNG_HD constexpr uint32_t png_crc_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ kPngCrcPoly : i >> 1;
  return i;
}
constexpr uint32_t png_crc_idat() {  // crc32(b"IDAT")
  uint32_t c = 0xFFFFFFFFu;
  const uint8_t s[4] = {'I', 'D', 'A', 'T'};
  for (int i = 0; i < 4; ++i) c = png_crc_table_entry((c ^ s[i]) & 255u) ^ (c >> 8);
  return ~c;
}
constexpr uint32_t kPngCrcIdat = png_crc_idat();

}  // namespace rfx
