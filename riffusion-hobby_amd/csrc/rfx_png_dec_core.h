// rfx_png_dec_core.h - decoding a PNG tile's IDAT payload into the RGB pixels Pillow gives (np.asarray(Image.open(f).convert("RGB"))),
// written once for the gfx950 kernels (rfx_png_dec.hip, hipcc) and the host emulator of the CPU tests (tests/emu/rfx_png_dec_emu.cpp,
// g++).  The files taken: 8 bit, colour type 0, 2, 3 or 6, not interlaced (riffusion.util.image_util.png_parse keeps every other
// file on the host).  Three steps, all integer arithmetic:
//   * inflate (RFC 1950 / 1951): the zlib header, stored, fixed and dynamic blocks, the Adler-32.  The output is the filtered
//     image, exactly H * (W * bpp + 1) bytes;
//   * unfilter (PNG filter method 0): types 0 .. 4 per row, the row above the first and the bytes left of the first pixel zeros,
//     Average the floor of the 9-bit sum, Paeth's ties in the order left, up, upper-left;
//   * to RGB: grey three times, RGB as is, RGBA without the alpha byte, palette[index].
// The code is written for one group of `lanes` lanes that run in step (a wave, a workgroup between barriers, or the host's one
// lane): everything that decides control flow is computed by every lane alike from the same bytes, and the loops marked
// "cooperative" hand element i to lane i mod lanes and end in w.sync().  How bytes are fetched and stored is the caller's:
//   Wave   int lane(), int lanes(), void sync()       sync: a barrier that also orders the shared arrays
//   Fetch  uint32_t word(uint32_t i, uint32_t n)      stream bytes i .. i + 3, first byte lowest, bytes at or past n as zeros; asked
//                                                     for by all lanes with the same i
//          uint8_t at(uint32_t i)                     stream byte i < n, any lane, any i
//   Store  void word(uint64_t i, uint32_t v)          filtered bytes i .. i + 3 (i a multiple of 4), void byte(uint64_t i, uint8_t v)
// The device is conservative: status 0 means that zlib and Pillow take the stream and give these pixels; whatever this code is
// not sure of gets a status, and the caller hands the file to Pillow.
//
// Termination: every block consumes at least 3 bits and every symbol at least 1; bytes behind the stream's end read as zeros and
// the first element that used one ends the call (kPngdInputEnds); no output position passes H * (W * bpp + 1) (kPngdTooMuch).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RFX_PNGD_HD __host__ __device__ __forceinline__
#else
#define RFX_PNGD_HD inline __attribute__((always_inline))
#endif

namespace rfx {

// ---- status of one image: the first cause in stream order ----------------------------------------------------------------------
constexpr int kPngdOk = 0;
constexpr int kPngdZlibHeader = 1;   // CM != 8, CINFO > 7, FDICT, or the check bits
constexpr int kPngdBlockType = 2;    // block type 3, or stored LEN != ~NLEN
constexpr int kPngdBadHeader = 3;    // a dynamic header that does not define two usable prefix codes
constexpr int kPngdBadCode = 4;      // bits that are no code, length symbol 286 / 287, distance symbol 30 / 31
constexpr int kPngdFarDistance = 5;  // a distance beyond the bytes produced so far
constexpr int kPngdInputEnds = 6;    // the input ends inside the stream
constexpr int kPngdTooMuch = 7;      // more output than H * (W * bpp + 1)
constexpr int kPngdTooLittle = 8;    // fewer bytes at the final block's end
constexpr int kPngdAdler = 9;        // Adler-32 mismatch
constexpr int kPngdLeftOver = 10;    // bytes behind the Adler-32
constexpr int kPngdFilterType = 11;  // a filter type above 4
constexpr int kPngdPaletteIndex = 12;  // a palette index at or past palette_entries

constexpr int kPngdMaxSize = 65535;                       // H and W
constexpr int64_t kPngdMaxStreamBytes = (1ll << 28) - 64;  // per image: byte and bit positions are 32-bit
constexpr int kPngdRingBytes = 32768;                     // the LZ77 window
constexpr int kPngdRingMask = kPngdRingBytes - 1;
constexpr int kPngdFlushBytes = 16384;  // the ring goes out once this much is new: with a symbol's 258 bytes still under the ring's size
constexpr int kPngdLitLutBits = 10, kPngdDistLutBits = 8, kPngdClenLutBits = 7;
constexpr int kPngdMaxLanes = 64;       // of the inflate's group (the Adler-32 partial sums)
constexpr uint32_t kPngdAdlerMod = 65521;
constexpr int kPngdSegBytes = 12288;    // the unfilter's piece of a row: a multiple of every bpp (1, 3, 4)

// a value every lane holds alike, said so: on the device it moves to a scalar register, and what depends on it - the branches
// of the symbol loop above all - becomes scalar work
RFX_PNGD_HD uint32_t pngd_uni(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}

RFX_PNGD_HD int pngd_bpp(int color_type) { return color_type == 0 || color_type == 3 ? 1 : color_type == 2 ? 3 : color_type == 6 ? 4 : 0; }
RFX_PNGD_HD uint64_t pngd_filtered_bytes(int H, int W, int bpp) { return (uint64_t)H * ((uint64_t)W * bpp + 1); }

// the decode's workspace: every image's filtered bytes (unfiltered in place when a row is longer than kPngdSegBytes), each image
// on a 256-byte boundary
struct PngdLayout {
  size_t filtered, per_image, total;
};
inline PngdLayout png_decode_workspace_layout(int N, int H, int W, int color_type) {
  PngdLayout l{};
  const int bpp = pngd_bpp(color_type);
  if (N <= 0 || H <= 0 || W <= 0 || H > kPngdMaxSize || W > kPngdMaxSize || !bpp) return l;
  l.per_image = (size_t)((pngd_filtered_bytes(H, W, bpp) + 255) / 256 * 256);
  l.total = (size_t)N * l.per_image;
  return l;
}

// ---- what the inflate keeps in shared memory (LDS on the device) -------------------------------------------------------------
// A prefix code: count[l] codes of l bits, the symbols sorted by (length, symbol), and lut[the next bits, first bit lowest] =
// symbol << 4 | length for the codes of at most the lut's bits (0: a longer code, or none).
struct PngdTables {
  uint16_t lit_lut[1 << kPngdLitLutBits];
  uint16_t dist_lut[1 << kPngdDistLutBits];  // (the code-length code's too, while a dynamic header is read)
  uint16_t lit_count[16], dist_count[16];
  uint16_t lit_symbol[288], dist_symbol[32];
  uint32_t adler_part[2 * kPngdMaxLanes];
  uint8_t lengths[320];  // the code lengths of the block being set up: 288 literal/length, then 32 distance
};
struct PngdInflateShared {
  uint32_t ring[kPngdRingBytes / 4];
  PngdTables t;
};
struct PngdUnfilterShared {
  uint8_t rows[2][kPngdSegBytes];
  uint8_t palette[768];
  uint8_t carry[8];  // left[4], upper-left[4] of the channels between two pieces of a row
  int32_t bad;
};
// (what tests/test_png_decode_isa.py holds the kernels to, beside the staging buffer rfx_png_dec.hip adds to the inflate's)
constexpr size_t kPngdInflateSharedBytes = sizeof(PngdInflateShared);
constexpr size_t kPngdUnfilterSharedBytes = sizeof(PngdUnfilterShared);

// ---- the bit stream: first bit lowest ----------------------------------------------------------------------------------------------
template <class Fetch>
struct PngdBits {
  Fetch& f;
  uint32_t n;     // bytes of the stream
  uint32_t in;    // bytes taken into `hold` (bytes behind the end count, as zeros)
  uint64_t hold;
  int nbits;
  RFX_PNGD_HD PngdBits(Fetch& fetch, uint32_t bytes) : f(fetch), n(bytes), in(0), hold(0), nbits(0) {}
  RFX_PNGD_HD void refill() {  // at least 32 bits afterwards: four bytes at a time
    if (nbits < 32) {
      hold |= (uint64_t)f.word(in, n) << nbits;
      in += 4;
      nbits += 32;
    }
  }
  RFX_PNGD_HD void drop(int k) {
    hold >>= k;
    nbits -= k;
  }
  RFX_PNGD_HD uint32_t bits(int k) {  // k <= 16
    refill();
    const uint32_t v = (uint32_t)hold & ((1u << k) - 1);
    drop(k);
    return v;
  }
  RFX_PNGD_HD uint64_t consumed_bits() const { return (uint64_t)in * 8 - (uint64_t)nbits; }
  RFX_PNGD_HD bool over() const { return consumed_bits() > (uint64_t)n * 8; }  // a bit behind the end was used
  RFX_PNGD_HD void align() { drop(nbits & 7); }
  // at a byte boundary: the byte position, the buffer emptied (the caller moves `in` on)
  RFX_PNGD_HD uint32_t to_bytes() {
    const uint32_t at = in - (uint32_t)(nbits >> 3);
    hold = 0;
    nbits = 0;
    in = at;
    return at;
  }
};

// ---- prefix codes ----------------------------------------------------------------------------------------------------------------
RFX_PNGD_HD uint32_t pngd_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// count, symbol and lut of the code with `n` lengths (0: symbol unused).  Returns the code space left over: 0 a complete code,
// above 0 an incomplete one, below 0 an over-subscribed one (then nothing else is valid).  *coded: the symbols that have a code.
template <class Wave>
RFX_PNGD_HD int pngd_build(const Wave& w, const uint8_t* lengths, int n, uint16_t* count, uint16_t* symbol, uint16_t* lut, int lut_bits,
                           int* coded) {
  // cooperative: the lut cleared, and one length's count per lane
  for (int i = w.lane(); i < (1 << lut_bits); i += w.lanes()) lut[i] = 0;
  for (int len = w.lane(); len < 16; len += w.lanes()) {
    int c = 0;
    for (int s = 0; s < n; ++s) c += lengths[s] == len;
    count[len] = (uint16_t)c;
  }
  w.sync();
  int left = 1, total = 0;
  for (int len = 1; len <= 15; ++len) {
    left = (left << 1) - (int)count[len];
    total += count[len];
    if (left < 0) return left;
  }
  *coded = total;
  // cooperative: one length's symbols per lane, in symbol order behind those of the shorter lengths
  for (int len = 1 + w.lane(); len <= 15; len += w.lanes()) {
    int at = 0;
    for (int k = 1; k < len; ++k) at += count[k];
    for (int s = 0; s < n; ++s)
      if (lengths[s] == len) symbol[at++] = (uint16_t)s;
  }
  w.sync();
  // cooperative: the k-th symbol's canonical code, reversed, at every lut index that starts with it
  for (int k = w.lane(); k < total; k += w.lanes()) {
    int first = 0, index = 0, len = 1;
    for (; len <= 15; ++len) {
      const int c = count[len];
      if (k < index + c) break;
      index += c;
      first = (first + c) << 1;
    }
    if (len <= lut_bits) {
      const uint16_t entry = (uint16_t)(symbol[k] << 4 | len);
      for (uint32_t j = pngd_reverse((uint32_t)(first + (k - index)), len); j < (1u << lut_bits); j += 1u << len) lut[j] = entry;
    }
  }
  w.sync();
  return left;
}

// the next symbol, its bits dropped; -1: the bits are no code (an incomplete code's unused patterns; the longest length dropped)
template <class Bits>
RFX_PNGD_HD int pngd_symbol(Bits& br, const uint16_t* lut, int lut_bits, const uint16_t* count, const uint16_t* symbol) {
  br.refill();
  uint32_t v = (uint32_t)br.hold;
  const uint32_t e = pngd_uni(lut[v & ((1u << lut_bits) - 1)]);
  if (e & 15) {
    br.drop((int)(e & 15));
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0, longest = 0;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)(v & 1);
    v >>= 1;
    const int c = (int)pngd_uni(count[len]);
    if (code - c < first) {
      br.drop(len);
      return (int)pngd_uni(symbol[index + (code - first)]);
    }
    if (c) longest = len;
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  br.drop(longest ? longest : 1);
  return -1;
}

// ---- the ring and the Adler-32 ---------------------------------------------------------------------------------------------------
// The ring's bytes [flushed, flushed + n) go out (cooperative; flushed a multiple of 4: whole words, then the last n mod 4 bytes)
// and into the Adler-32 (a, b).
template <class Wave, class Store>
RFX_PNGD_HD void pngd_flush(const Wave& w, const uint32_t* ring, uint64_t flushed, uint32_t n, Store& out, uint32_t* part, uint32_t* a, uint32_t* b) {
  const uint8_t* ring8 = reinterpret_cast<const uint8_t*>(ring);
  uint64_t s1 = 0, s2 = 0;
  const uint32_t words = n >> 2;
  for (uint32_t k = w.lane(); k < words; k += w.lanes()) {
    const uint64_t at = flushed + 4ull * k;
    const uint32_t v = ring[(at & kPngdRingMask) >> 2];
    out.word(at, v);
    const uint32_t x0 = v & 255, x1 = (v >> 8) & 255, x2 = (v >> 16) & 255, x3 = v >> 24, m = n - 4 * k;
    s1 += x0 + x1 + x2 + x3;
    s2 += (uint64_t)m * x0 + (uint64_t)(m - 1) * x1 + (uint64_t)(m - 2) * x2 + (uint64_t)(m - 3) * x3;
  }
  for (uint32_t k = 4 * words + w.lane(); k < n; k += w.lanes()) {
    const uint8_t x = ring8[(flushed + k) & kPngdRingMask];
    out.byte(flushed + k, x);
    s1 += x;
    s2 += (uint64_t)(n - k) * x;
  }
  part[2 * w.lane()] = (uint32_t)(s1 % kPngdAdlerMod);
  part[2 * w.lane() + 1] = (uint32_t)(s2 % kPngdAdlerMod);
  w.sync();
  uint64_t t1 = 0, t2 = 0;
  for (int l = 0; l < w.lanes(); ++l) {
    t1 += part[2 * l];
    t2 += part[2 * l + 1];
  }
  *b = (uint32_t)((*b + (uint64_t)(n % kPngdAdlerMod) * *a + t2) % kPngdAdlerMod);
  *a = (uint32_t)((*a + t1) % kPngdAdlerMod);
  w.sync();
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------
// The zlib stream `in` (n bytes) -> exactly `expected` filtered bytes through `out`; returns the status.  sh: the group's shared
// memory, its contents of no account before and after.
template <class Wave, class Fetch, class Store>
RFX_PNGD_HD int pngd_inflate(const Wave& w, Fetch& in, uint32_t n, uint64_t expected, Store& out, PngdInflateShared* sh) {
  PngdTables& t = sh->t;
  uint8_t* ring8 = reinterpret_cast<uint8_t*>(sh->ring);
  PngdBits<Fetch> br(in, n);
  {
    const uint32_t cmf = br.bits(8), flg = br.bits(8);
    if (br.over()) return kPngdInputEnds;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 32) || (cmf * 256 + flg) % 31) return kPngdZlibHeader;
  }
  uint64_t pos = 0, flushed = 0;
  uint32_t a = 1, b = 0;
  for (bool last = false; !last;) {
    const uint32_t head = br.bits(3);
    if (br.over()) return kPngdInputEnds;
    last = head & 1;
    const uint32_t type = head >> 1;
    if (type == 3) return kPngdBlockType;
    if (type == 0) {
      br.align();
      const uint32_t len = br.bits(16), nlen = br.bits(16);
      if (br.over()) return kPngdInputEnds;
      if (len != (nlen ^ 0xFFFFu)) return kPngdBlockType;
      const uint32_t at = br.to_bytes();
      const uint32_t avail = n - at;
      const uint64_t room = expected - pos;
      if (len > avail && avail <= room) return kPngdInputEnds;
      if (len > room) return kPngdTooMuch;
      w.sync();
      for (uint32_t done = 0; done < len;) {  // pieces that keep the new bytes under the ring's size
        const uint32_t piece = len - done < 256 ? len - done : 256;
        for (uint32_t i = w.lane(); i < piece; i += w.lanes()) ring8[(pos + i) & kPngdRingMask] = in.at(at + done + i);  // cooperative
        w.sync();
        done += piece;
        pos += piece;
        if (pos - flushed >= kPngdFlushBytes) {
          const uint32_t m = (uint32_t)(pos - flushed) & ~127u;
          pngd_flush(w, sh->ring, flushed, m, out, t.adler_part, &a, &b);
          flushed += m;
        }
      }
      br.in = at + len;
      continue;
    }
    // the block's two codes
    int nlit, ndist;
    if (type == 1) {
      nlit = 288;
      ndist = 32;
      for (int i = w.lane(); i < 320; i += w.lanes()) t.lengths[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);  // cooperative
      w.sync();
    } else {
      nlit = (int)br.bits(5) + 257;
      ndist = (int)br.bits(5) + 1;
      const int nclen = (int)br.bits(4) + 4;
      if (br.over()) return kPngdInputEnds;
      if (nlit > 286 || ndist > 30) return kPngdBadHeader;
      // the code-length code's lengths come in this order; all lanes read them alike, lane 0 writes
      for (int i = w.lane(); i < 19; i += w.lanes()) t.lengths[i] = 0;
      w.sync();
      for (int i = 0; i < nclen; ++i) {
        const int s = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1);  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const uint8_t v = (uint8_t)br.bits(3);
        if (w.lane() == 0) t.lengths[s] = v;
      }
      if (br.over()) return kPngdInputEnds;
      w.sync();
      int coded;
      if (pngd_build(w, t.lengths, 19, t.dist_count, t.dist_symbol, t.dist_lut, kPngdClenLutBits, &coded) != 0) return kPngdBadHeader;
      // (the lengths array is free again: the code-length code lives in count, symbol and lut)
      const int total = nlit + ndist;
      int prev = -1;  // the length before: a repeat needs one
      for (int idx = 0; idx < total;) {
        const int s = pngd_symbol(br, t.dist_lut, kPngdClenLutBits, t.dist_count, t.dist_symbol);
        if (br.over()) return kPngdInputEnds;
        if (s < 0) return kPngdBadHeader;
        int rep = 1, val = s;
        if (s == 16) {
          if (prev < 0) return kPngdBadHeader;
          val = prev;
          rep = 3 + (int)br.bits(2);
        } else if (s == 17) {
          val = 0;
          rep = 3 + (int)br.bits(3);
        } else if (s == 18) {
          val = 0;
          rep = 11 + (int)br.bits(7);
        }
        if (br.over()) return kPngdInputEnds;
        if (idx + rep > total) return kPngdBadHeader;
        // literal/length lengths at 0 .., distance lengths at 288 ..: a repeat runs from the one into the other
        for (int i = w.lane(); i < rep; i += w.lanes()) {  // cooperative
          const int j = idx + i;
          t.lengths[j < nlit ? j : 288 + (j - nlit)] = (uint8_t)val;
        }
        idx += rep;
        prev = val;
      }
      w.sync();
      if (t.lengths[256] == 0) return kPngdBadHeader;
    }
    {
      int coded;
      if (pngd_build(w, t.lengths, nlit, t.lit_count, t.lit_symbol, t.lit_lut, kPngdLitLutBits, &coded) != 0) return kPngdBadHeader;
      const int left = pngd_build(w, t.lengths + 288, ndist, t.dist_count, t.dist_symbol, t.dist_lut, kPngdDistLutBits, &coded);
      // an incomplete distance code is taken in the two forms RFC 1951 names: a single code of one bit, and no code at all
      // (a block of literals only: rfx_png_encode_u8 writes it); any distance symbol of the latter is then no code
      if (left < 0 || (left > 0 && coded != 0 && !(coded == 1 && t.dist_count[1] == 1))) return kPngdBadHeader;
    }
    // the block's symbols
    for (;;) {
      const int s = pngd_symbol(br, t.lit_lut, kPngdLitLutBits, t.lit_count, t.lit_symbol);
      if (br.over()) return kPngdInputEnds;
      if (s < 0) return kPngdBadCode;
      if (s < 256) {
        if (pos >= expected) return kPngdTooMuch;
        if (w.lane() == 0) ring8[pos & kPngdRingMask] = (uint8_t)s;
        ++pos;
      } else if (s == 256) {
        break;
      } else {
        if (s >= 286) return kPngdBadCode;
        uint32_t len;
        if (s < 265) {
          len = (uint32_t)s - 254;
        } else if (s == 285) {
          len = 258;
        } else {
          const int e = (s - 261) >> 2;
          len = ((4u + ((uint32_t)(s - 265) & 3)) << e) + 3 + br.bits(e);
        }
        const int ds = pngd_symbol(br, t.dist_lut, kPngdDistLutBits, t.dist_count, t.dist_symbol);
        if (br.over()) return kPngdInputEnds;
        if (ds < 0 || ds >= 30) return kPngdBadCode;
        uint32_t d;
        if (ds < 4) {
          d = (uint32_t)ds + 1;
        } else {
          const int e = (ds >> 1) - 1;
          d = ((2u + ((uint32_t)ds & 1)) << e) + 1 + br.bits(e);
        }
        if (br.over()) return kPngdInputEnds;
        if (d > pos) return kPngdFarDistance;
        if (len > expected - pos) return kPngdTooMuch;
        w.sync();
        // cooperative: out[pos + i] = out[pos - d + (i mod d)].  The bytes read lie in [pos - d, pos), none of them written here,
        // except where d + len passes the ring's size: there slot pos + i is the source of element i - (32768 - d), which an
        // earlier step (or, among the lanes of one step, the read before the write) has taken already
        const uint32_t from = (uint32_t)(pos - d) & kPngdRingMask, to = (uint32_t)pos & kPngdRingMask;
        if (d >= len) {
          for (uint32_t i = w.lane(); i < len; i += w.lanes()) {
            const uint8_t v = ring8[(from + i) & kPngdRingMask];
            ring8[(to + i) & kPngdRingMask] = v;
          }
        } else {
          for (uint32_t i = w.lane(); i < len; i += w.lanes()) {
            const uint8_t v = ring8[(from + i % d) & kPngdRingMask];
            ring8[(to + i) & kPngdRingMask] = v;
          }
        }
        w.sync();
        pos += len;
      }
      if (pos - flushed >= kPngdFlushBytes) {
        w.sync();
        const uint32_t m = (uint32_t)(pos - flushed) & ~127u;
        pngd_flush(w, sh->ring, flushed, m, out, t.adler_part, &a, &b);
        flushed += m;
      }
    }
  }
  if (pos < expected) return kPngdTooLittle;
  br.align();
  uint32_t want = 0;
  for (int i = 0; i < 4; ++i) want = want << 8 | br.bits(8);
  if (br.over()) return kPngdInputEnds;
  w.sync();
  pngd_flush(w, sh->ring, flushed, (uint32_t)(pos - flushed), out, t.adler_part, &a, &b);
  if (want != (b << 16 | a)) return kPngdAdler;
  if (br.to_bytes() < n) return kPngdLeftOver;
  return kPngdOk;
}

// ---- unfilter and RGB ------------------------------------------------------------------------------------------------------------
RFX_PNGD_HD int pngd_paeth(int a, int b, int c) {  // left, up, upper-left
  // with p = a + b - c: |p - a| = |b - c|, |p - b| = |a - c|, |p - c| = |(b - c) + (a - c)|
  const int db = b - c, da = a - c, dc = db + da;
  const int pa = db < 0 ? -db : db, pb = da < 0 ? -da : da, pc = dc < 0 ? -dc : dc;
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// One channel's walk along a piece for filter TYPE 1 (Sub), 3 (Average) or 4 (Paeth): bytes c, c + bpp, ... of `cur`, in place.
// Eight steps at a time: their bytes are loaded together, the chain runs in registers, the results are stored together; FULL says
// that all eight are inside the piece.
template <int TYPE, bool FULL>
RFX_PNGD_HD void pngd_walk8(uint8_t* cur, const uint8_t* up, int x, int n, int bpp, int* left, int* ul) {
  int f[8], above[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int at = x + j * bpp;
    const bool in = FULL || at < n;
    f[j] = in ? cur[at] : 0;
    above[j] = TYPE != 1 && in && up ? up[at] : 0;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (FULL || x + j * bpp < n) {
      const int pred = TYPE == 1 ? *left : TYPE == 3 ? (*left + above[j]) >> 1 : pngd_paeth(*left, above[j], *ul);
      *left = (f[j] + pred) & 255;
      *ul = above[j];
      f[j] = *left;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int at = x + j * bpp;
    if (FULL || at < n) cur[at] = (uint8_t)f[j];
  }
}
template <int TYPE>
RFX_PNGD_HD void pngd_walk(uint8_t* cur, const uint8_t* up, int c, int n, int bpp, uint8_t* carry) {
  int left = carry[c], ul = carry[4 + c], x = c;
  for (; x + 7 * bpp < n; x += 8 * bpp) pngd_walk8<TYPE, true>(cur, up, x, n, bpp, &left, &ul);
  if (x < n) pngd_walk8<TYPE, false>(cur, up, x, n, bpp, &left, &ul);
  carry[c] = (uint8_t)left;
  carry[4 + c] = (uint8_t)ul;
}

// One piece (n bytes, a multiple of bpp) of a row of filter type 0 .. 4 in `cur`, in place.  up: the same piece of the row above
// (nullptr: zeros).  carry: left[4], upper-left[4] as the piece before left them (zeros at a row's start).  Types 1, 3 and 4 walk
// the piece with one lane per channel; types 0 and 2 are cooperative.
template <class Wave>
RFX_PNGD_HD void pngd_unfilter_piece(const Wave& w, int type, uint8_t* cur, const uint8_t* up, int n, int bpp, uint8_t* carry) {
  if (type == 2) {
    if (up)
      for (int x = w.lane(); x < n; x += w.lanes()) cur[x] = (uint8_t)(cur[x] + up[x]);
  } else if (type != 0) {
    for (int c = w.lane(); c < bpp; c += w.lanes()) {
      if (type == 1) pngd_walk<1>(cur, up, c, n, bpp, carry);
      else if (type == 3) pngd_walk<3>(cur, up, c, n, bpp, carry);
      else pngd_walk<4>(cur, up, c, n, bpp, carry);
    }
  }
  w.sync();
}

// The RGB bytes of one unfiltered piece (cooperative over the 3 * n / bpp output bytes); rgb(j, v) stores output byte j of the piece.
// Returns false where a palette index is at or past `entries` (decided by all lanes alike through *bad).
template <class Wave, class Rgb>
RFX_PNGD_HD bool pngd_piece_rgb(const Wave& w, int color_type, const uint8_t* cur, int n, int bpp, const uint8_t* palette, int entries,
                                int32_t* bad, Rgb& rgb) {
  const int bytes = n / bpp * 3;
  bool mine = false;
  for (int j = w.lane(); j < bytes; j += w.lanes()) {
    const int px = j / 3, c = j - 3 * px;
    uint8_t v;
    if (color_type == 2) {
      v = cur[j];
    } else if (color_type == 6) {
      v = cur[4 * px + c];
    } else if (color_type == 0) {
      v = cur[px];
    } else {
      const int index = cur[px];
      mine |= index >= entries;
      v = palette[(index < entries ? index : 0) * 3 + c];
    }
    rgb(j, v);
  }
  if (color_type != 3) return true;
  if (mine) *bad = 1;
  w.sync();
  return *bad == 0;
}

// The filtered image `filt` (byte(i) of any lane; put(i, v) writes an unfiltered byte back over it, used only where a row has
// several pieces) -> the (H, W, 3) pixels through rgb(i, v).  Returns the status: 0, kPngdFilterType or kPngdPaletteIndex.
template <class Wave, class Filtered, class Rgb>
RFX_PNGD_HD int pngd_unfilter_image(const Wave& w, Filtered& filt, int H, int W, int color_type, const uint8_t* palette768, int entries, Rgb& rgb,
                                    PngdUnfilterShared* sh) {
  const int bpp = pngd_bpp(color_type);
  const int64_t row_bytes = (int64_t)W * bpp;
  const bool pieces = row_bytes > kPngdSegBytes;
  if (color_type == 3)
    for (int i = w.lane(); i < 768; i += w.lanes()) sh->palette[i] = palette768[i];
  if (w.lane() == 0) sh->bad = 0;
  w.sync();
  uint8_t* cur = sh->rows[0];
  uint8_t* above = sh->rows[1];
  for (int64_t y = 0; y < H; ++y) {
    const uint64_t row_at = (uint64_t)y * (uint64_t)(row_bytes + 1);
    const int type = (int)pngd_uni(filt.byte(row_at));
    if (type > 4) return kPngdFilterType;
    for (int i = w.lane(); i < 8; i += w.lanes()) sh->carry[i] = 0;
    for (int64_t s0 = 0; s0 < row_bytes; s0 += kPngdSegBytes) {
      const int n = (int)(row_bytes - s0 < kPngdSegBytes ? row_bytes - s0 : kPngdSegBytes);
      for (int i = w.lane(); i < n; i += w.lanes()) {  // cooperative
        cur[i] = filt.byte(row_at + 1 + (uint64_t)s0 + i);
        if (pieces && y > 0) above[i] = filt.byte(row_at - (uint64_t)(row_bytes + 1) + 1 + (uint64_t)s0 + i);
      }
      w.sync();
      pngd_unfilter_piece(w, type, cur, y > 0 ? above : nullptr, n, bpp, sh->carry);
      struct Out {
        Rgb& rgb;
        uint64_t base;
        RFX_PNGD_HD void operator()(int j, uint8_t v) { rgb(base + (uint64_t)j, v); }
      } o{rgb, ((uint64_t)y * (uint64_t)W + (uint64_t)(s0 / bpp)) * 3};
      if (!pngd_piece_rgb(w, color_type, cur, n, bpp, sh->palette, entries, &sh->bad, o)) return kPngdPaletteIndex;
      if (pieces) {
        for (int i = w.lane(); i < n; i += w.lanes()) filt.put(row_at + 1 + (uint64_t)s0 + i, cur[i]);  // cooperative
        w.sync();
      }
    }
    if (!pieces) {  // the row stays where it is and becomes the row above
      uint8_t* swap = cur;
      cur = above;
      above = swap;
      w.sync();
    }
  }
  return kPngdOk;
}

}  // namespace rfx
