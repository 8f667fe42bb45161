// Host emulator of the PNG kernels (csrc/rfx_png.hip).  TEST INFRASTRUCTURE ONLY (built by tests/test_png_cpu.py with g++): the
// arithmetic of rfx_png_core.h in the kernels' stages - the grey test, the filter choice per row with its Adler-32 sums, the tokens
// and histogram of every block, the code builder, the blocks' bit offsets, the bits, the Adler-32 from the rows and the CRC-32 from
// 256-byte pieces - so that the stream is pinned against zlib's inflate and Pillow on the CPU and the device against this.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_png_core.h"

using namespace rfx;

namespace {

struct BitWriter {  // LSB-first into zeroed bytes, at any bit offset
  uint8_t* out;
  uint64_t at;
  void operator()(uint32_t bits, int count) {
    for (int i = 0; i < count; ++i, ++at)
      if ((bits >> i) & 1u) out[at >> 3] |= (uint8_t)(1u << (at & 7));
  }
};

uint32_t crc_of(const uint8_t* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = png_crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
  return ~c;
}

}  // namespace

extern "C" {

uint64_t emu_png_stream_capacity(int H, int W, int ch) { return png_stream_capacity(png_geom(H, W, ch)); }

// counts[0 .. nsym) -> lens[0 .. nsym) and the bit-reversed codes, by the block builder's rule.  Returns the used symbols.
int emu_png_code_lengths(const uint32_t* counts, int nsym, int limit, uint8_t* lens, uint16_t* codes) {
  PngScratch sc;
  int n = 0;
  for (int s = 0; s < nsym; ++s) {
    sc.counts[s] = counts[s];
    if (counts[s]) {
      sc.sorted[png_rank(counts, nsym, s)] = (uint16_t)s;
      ++n;
    }
  }
  if (n == 0) return 0;
  png_code_lengths(sc, nsym, n, limit, lens);
  png_assign_codes(sc, lens, nsym, limit, codes);
  return n;
}

// the token histogram of one block of n bytes (without the end-of-block): hist[0 .. 286)
void emu_png_block_histogram(const uint8_t* src, int64_t n, uint32_t* hist) {
  auto byte = [src](int64_t i) { return (int)src[i]; };
  for (int s = 0; s < kPngLitLen; ++s) hist[s] = 0;
  int64_t start = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (i == 0 || src[i] != src[i - 1]) start = i;
    int len, e, eb;
    const int kind = png_token(byte, i, n, i - start, &len);
    if (kind == 1) hist[src[i]] += 1;
    else if (kind == 2) hist[png_length_symbol(len, &e, &eb)] += 1;
  }
}

// (H, W, 3) uint8 -> the zlib stream of its IDAT chunk in `stream` (capacity bytes, zeroed here).  mode 0 RGB, 1 grey, 2 auto.
// Returns the stream's length (0 with *channels = 0 when mode 1 meets a colour tile), -1 when it would pass the capacity;
// *crc: CRC-32 of b"IDAT" + stream.  stats (may be null): [0] blocks without a match, [1] longest literal/length code,
// [2] blocks whose unlimited Huffman depth passed 15.
int64_t emu_png_encode_u8(const uint8_t* rgb, int H, int W, int mode, uint8_t* stream, uint64_t capacity, uint32_t* crc, int32_t* channels,
                          int64_t* stats) {
  // 0. grey?
  bool colour = false;
  for (int64_t p = 0; p < (int64_t)H * W && !colour; ++p) colour = rgb[3 * p] != rgb[3 * p + 1] || rgb[3 * p] != rgb[3 * p + 2];
  const int ch = mode == 0 ? 3 : (colour ? (mode == 1 ? 0 : 3) : 1);
  *channels = ch;
  *crc = 0;
  if (ch == 0) return 0;
  const PngGeom g = png_geom(H, W, ch);
  // 1. filter rows, and their Adler sums
  std::vector<uint8_t> filt((size_t)g.bytes);
  std::vector<uint32_t> row_a(H), row_b(H);
  const int64_t wc = g.row - 1;
  for (int y = 0; y < H; ++y) {
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int64_t j = 0; j < wc; ++j) {
      int f0, f1, f2, f3, f4;
      png_filter_all(rgb, W, ch, y, j, &f0, &f1, &f2, &f3, &f4);
      c0 += png_filter_cost(f0);
      c1 += png_filter_cost(f1);
      c2 += png_filter_cost(f2);
      c3 += png_filter_cost(f3);
      c4 += png_filter_cost(f4);
    }
    const int type = png_choose_filter(c0, c1, c2, c3, c4);
    uint8_t* out = filt.data() + (size_t)y * g.row;
    out[0] = (uint8_t)type;
    uint64_t a = (uint64_t)type, b = (uint64_t)g.row * type;
    for (int64_t j = 0; j < wc; ++j) {
      const int f = png_filter_one(rgb, W, ch, y, j, type);
      out[1 + j] = (uint8_t)f;
      a += f;
      b += (uint64_t)(g.row - 1 - j) * f;
    }
    row_a[y] = (uint32_t)(a % kPngAdlerMod);
    row_b[y] = (uint32_t)(b % kPngAdlerMod);
  }
  // 2. tokens -> histogram, 3. codes and headers, per block
  std::vector<PngBlockCodes> codes(g.blocks);
  std::vector<std::vector<uint8_t>> headers(g.blocks);
  std::vector<uint32_t> header_bits(g.blocks), block_bits(g.blocks);
  int64_t no_match = 0, longest = 0, deep = 0;
  for (int blk = 0; blk < g.blocks; ++blk) {
    const int rows = H - blk * kPngBlockRows < kPngBlockRows ? H - blk * kPngBlockRows : kPngBlockRows;
    const int64_t n = rows * g.row;
    const uint8_t* src = filt.data() + (size_t)blk * kPngBlockRows * g.row;
    auto byte = [src](int64_t i) { return (int)src[i]; };
    PngScratch sc;
    for (int s = 0; s < 288; ++s) sc.counts[s] = 0;
    int64_t start = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (i == 0 || src[i] != src[i - 1]) start = i;
      int len;
      const int kind = png_token(byte, i, n, i - start, &len);
      int e, eb;
      if (kind == 1) sc.counts[src[i]] += 1;
      else if (kind == 2) sc.counts[png_length_symbol(len, &e, &eb)] += 1;
    }
    sc.counts[kPngEob] = 1;
    int used = 0;
    for (int s = 0; s < kPngLitLen; ++s)
      if (sc.counts[s]) ++used;
    for (int s = kPngLitLen - 1; s >= 0; --s)  // (any order: a symbol's place depends on the counts alone)
      if (sc.counts[s]) sc.sorted[png_rank(sc.counts, kPngLitLen, s)] = (uint16_t)s;
    const uint32_t body = png_block_codes(sc, used, codes[blk]);
    int unlimited = 0;
    for (int i = 0; i < used; ++i) unlimited = sc.depth[i] > unlimited ? sc.depth[i] : unlimited;
    deep += used > 1 && unlimited > kPngMaxBits;
    for (int s = 0; s < kPngLitLen; ++s) longest = codes[blk].lens[s] > longest ? codes[blk].lens[s] : longest;
    no_match += codes[blk].lens[kPngDist] == 0;
    headers[blk].assign(kPngHeaderWords * 4, 0);
    BitWriter hw{headers[blk].data(), 0};
    png_block_header(sc, codes[blk], blk == g.blocks - 1, hw);
    if (hw.at > (uint64_t)kPngHeaderMaxBits) return -3;
    header_bits[blk] = (uint32_t)hw.at;
    block_bits[blk] = header_bits[blk] + body;
  }
  // 4. bit offsets, and the stream's size
  std::vector<uint64_t> block_at(g.blocks);
  uint64_t bits = 16;
  for (int blk = 0; blk < g.blocks; ++blk) {
    block_at[blk] = bits;
    bits += block_bits[blk];
  }
  const uint64_t bytes = (bits + 7) / 8 + 4;
  if (bytes > capacity) return -1;
  memset(stream, 0, capacity);
  stream[0] = 0x78;
  stream[1] = 0x9C;
  // 5. pack: blocks in reverse order, every block from its own offset
  for (int blk = g.blocks - 1; blk >= 0; --blk) {
    const int rows = H - blk * kPngBlockRows < kPngBlockRows ? H - blk * kPngBlockRows : kPngBlockRows;
    const int64_t n = rows * g.row;
    const uint8_t* src = filt.data() + (size_t)blk * kPngBlockRows * g.row;
    auto byte = [src](int64_t i) { return (int)src[i]; };
    const PngBlockCodes& bc = codes[blk];
    BitWriter w{stream, block_at[blk]};
    for (uint32_t k = 0; k < header_bits[blk]; ++k) w((headers[blk][k >> 3] >> (k & 7)) & 1u, 1);
    int64_t start = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (i == 0 || src[i] != src[i - 1]) start = i;
      int len;
      const int kind = png_token(byte, i, n, i - start, &len);
      if (kind == 1) w(bc.codes[src[i]], bc.lens[src[i]]);
      else if (kind == 2) {
        int e, eb;
        const int sym = png_length_symbol(len, &e, &eb);
        w(bc.codes[sym], bc.lens[sym]);
        if (eb) w((uint32_t)e, eb);
        w(0u, 1);
      }
    }
    w(bc.codes[kPngEob], bc.lens[kPngEob]);
    if (w.at != block_at[blk] + block_bits[blk]) return -2;
  }
  // 6. Adler-32 from the rows
  uint64_t sum_a = 0, sum_t = 0;
  for (int y = 0; y < H; ++y) {
    sum_a += row_a[y];
    sum_t += png_adler_row_term(row_a[y], row_b[y], g.bytes - (int64_t)(y + 1) * g.row);
  }
  const uint32_t adler = png_adler_finish((uint32_t)(sum_a % kPngAdlerMod), (uint32_t)(sum_t % kPngAdlerMod), g.bytes);
  for (int i = 0; i < 4; ++i) stream[bytes - 4 + i] = (uint8_t)(adler >> (24 - 8 * i));
  // 7. CRC-32 from 256-byte pieces, last piece first
  uint32_t c = png_crc_shift(kPngCrcIdat, bytes, kPngCrcPowers);
  for (int64_t piece = (int64_t)((bytes + 255) / 256) - 1; piece >= 0; --piece) {
    const uint64_t lo = (uint64_t)piece * 256, hi = lo + 256 < bytes ? lo + 256 : bytes;
    c ^= png_crc_shift(crc_of(stream + lo, (size_t)(hi - lo)), bytes - hi, kPngCrcPowers);
  }
  *crc = c;
  if (stats) {
    stats[0] = no_match;
    stats[1] = longest;
    stats[2] = deep;
  }
  return (int64_t)bytes;
}

}  // extern "C"
