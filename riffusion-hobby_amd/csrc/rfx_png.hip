// rfx_png.hip - the zlib stream of a PNG's IDAT chunk for (N, H, W, 3) uint8 tiles on the device: the run-length + Huffman deflate
// of rfx_png_core.h, with its Adler-32 and the chunk's CRC-32.  Three clears (the grey flags, the streams' words, the CRCs) and
// eight kernels, all on the caller's stream; no workgroup waits for another one:
//   1. png_grey_kernel (modes grey and auto): is R = G = B at every pixel of tile n?  An OR per tile.
//   2. png_filter_kernel: one workgroup per row tries the five filters, writes the chosen one's bytes and the row's Adler sums.
//   3. png_tokens_kernel<false>: one workgroup per block of 32 rows walks its bytes 1024 at a time (a max-scan carries the start of
//      the run in progress) and counts its tokens in an LDS histogram.  Counts are integers: the order of the adds does not matter.
//   4. png_build_kernel: one wave per block.  The lanes sort the used symbols by rank; lane 0 builds the length-limited code, the
//      code-length code and the block's header bits, all in LDS, and leaves the block's bit count.
//   5. png_tokens_kernel<true>: the same walk; every token's bits go to their place (a sum-scan of the bit counts) in an LDS window
//      of the stream, LSB-first.  The window's whole words are stored plainly, its first and last word, shared with its neighbours,
//      are merged into the zeroed stream with a vector atomic OR.
//   6. png_finish_kernel: one workgroup per tile sums the blocks' bits and the rows' Adler terms, writes the zlib header, the
//      Adler-32, the stream's length and the tile's channel count.
//   7. png_crc_kernel: one thread per 256-byte piece: its CRC-32 times x^(8 * bytes after it), XORed into the tile's CRC.
//   8. png_copy_kernel: the stream's bytes, and no byte after them, to the caller's buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_kernels.h"
#include "rfx_png_core.h"

namespace rfx {

namespace {

constexpr int kPngThreads = 256;
constexpr int kPngTokThreads = 1024;
constexpr int kPngPackWords = (31 + kPngTokThreads * kPngTokenMaxBits + 31) / 32 + 1;  // one round's window: 674 words
constexpr int kPngPiece = 256;                                                         // bytes of the stream per CRC thread
constexpr int kPngTableStride = 288;                                                   // histogram / code table entries per block

__constant__ PngCrcPowers c_png_crc_powers = kPngCrcPowers;

struct PngArgs {
  const uint8_t* rgb;
  int N, H, W, mode, nblk;
  uint32_t *colour, *row_a, *row_b, *hist, *table, *hdr, *hdr_bits, *block_bits;
  uint8_t* filt;
  uint64_t filt_stride;  // bytes of one tile's filtered stream at 3 channels
  uint32_t* words;       // the streams, zeroed
  uint64_t words_per_tile;
  uint8_t* stream;
  uint64_t capacity;
  int32_t* stream_bytes;
  uint32_t* crc;
  int32_t* channels;
};

// channels tile n is written with; 0: refused (mode grey, a colour tile)
__device__ __forceinline__ int tile_channels(int mode, uint32_t colour) { return mode == 0 ? 3 : (colour ? (mode == 1 ? 0 : 3) : 1); }

// sums of four values per thread over a workgroup of kPngThreads; lds: 16 words of 8 bytes
__device__ __forceinline__ void wg_sum4(unsigned long long v[4], unsigned long long* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
  }
  __syncthreads();  // the previous readers are done with lds
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) lds[wave * 4 + q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = lds[q] + lds[4 + q] + lds[8 + q] + lds[12 + q];
}

// inclusive max-scan / exclusive sum-scan of one value per thread over a workgroup of kPngTokThreads; lds: 17 words
__device__ __forceinline__ int wg_scan_max(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = o > v ? o : v;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = -1;
    for (int w = 0; w < kPngTokThreads / 64; ++w) {
      const int t = lds[w];
      lds[w] = run;
      run = t > run ? t : run;
    }
    lds[kPngTokThreads / 64] = run;
  }
  __syncthreads();
  *total = lds[kPngTokThreads / 64];
  const int before = lds[wave];
  return before > v ? before : v;
}
__device__ __forceinline__ uint32_t wg_scan_sum(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int w = 0; w < kPngTokThreads / 64; ++w) {
      const uint32_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[kPngTokThreads / 64] = run;
  }
  __syncthreads();
  *total = lds[kPngTokThreads / 64];
  return lds[wave] + inc - v;
}

// up to 32 bits into the zeroed stream at any bit
__device__ __forceinline__ void put_global(uint32_t* words, uint64_t words_per_tile, uint64_t bit, uint32_t v) {
  const uint64_t w = bit >> 5;
  const int sh = (int)(bit & 31);
  const uint32_t lo = v << sh, hi = sh ? v >> (32 - sh) : 0u;
  if (lo && w < words_per_tile) atomicOr(words + w, lo);
  if (hi && w + 1 < words_per_tile) atomicOr(words + w + 1, hi);
}

// the header of a block, LSB-first into its words
struct HeaderWriter {
  uint32_t* out;
  unsigned long long acc;
  int fill, word;
  uint32_t bits;
  __device__ __forceinline__ void operator()(uint32_t v, int count) {
    acc |= (unsigned long long)v << fill;
    fill += count;
    bits += (uint32_t)count;
    if (fill >= 32) {
      if (word < kPngHeaderWords) out[word] = (uint32_t)acc;
      ++word;
      acc >>= 32;
      fill -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (fill > 0 && word < kPngHeaderWords) out[word] = (uint32_t)acc;
  }
};

}  // namespace

__global__ void __launch_bounds__(kPngThreads) png_grey_kernel(PngArgs a, int groups) {
  const int n = blockIdx.x / groups, g = blockIdx.x - n * groups;
  const int64_t pixels = (int64_t)a.H * a.W;
  const uint8_t* img = a.rgb + (int64_t)n * pixels * 3;
  bool colour = false;
  for (int64_t p = (int64_t)g * kPngThreads + threadIdx.x; p < pixels; p += (int64_t)groups * kPngThreads) {
    const int r = img[3 * p], gr = img[3 * p + 1], b = img[3 * p + 2];
    colour = colour || r != gr || r != b;
  }
  if (colour) atomicOr(a.colour + n, 1u);
}

__global__ void __launch_bounds__(kPngThreads) png_filter_kernel(PngArgs a) {
  __shared__ unsigned long long lds[16];
  const int n = blockIdx.x / a.H, y = blockIdx.x - n * a.H;
  const int ch = tile_channels(a.mode, a.colour[n]);
  if (ch == 0) return;
  const uint8_t* img = a.rgb + (int64_t)n * a.H * a.W * 3;
  const int64_t wc = (int64_t)a.W * ch, row = wc + 1;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
  for (int64_t j = threadIdx.x; j < wc; j += kPngThreads) {
    int f0, f1, f2, f3, f4;
    png_filter_all(img, a.W, ch, y, j, &f0, &f1, &f2, &f3, &f4);
    c0 += png_filter_cost(f0);
    c1 += png_filter_cost(f1);
    c2 += png_filter_cost(f2);
    c3 += png_filter_cost(f3);
    c4 += png_filter_cost(f4);
  }
  // (a cost is at most 128 * 196605 < 2^25: two to a word of 64 bits)
  unsigned long long v[4] = {c0 | ((unsigned long long)c1 << 32), c2 | ((unsigned long long)c3 << 32), c4, 0};
  wg_sum4(v, lds);
  const int type = png_choose_filter((uint32_t)v[0], (uint32_t)(v[0] >> 32), (uint32_t)v[1], (uint32_t)(v[1] >> 32), (uint32_t)v[2]);
  uint8_t* out = a.filt + (uint64_t)n * a.filt_stride + (int64_t)y * row;
  unsigned long long sa = 0, sb = 0;
  if (threadIdx.x == 0) {
    out[0] = (uint8_t)type;
    sa = (unsigned long long)type;
    sb = (unsigned long long)row * type;
  }
  for (int64_t j = threadIdx.x; j < wc; j += kPngThreads) {
    const int f = png_filter_one(img, a.W, ch, y, j, type);
    out[1 + j] = (uint8_t)f;
    sa += (unsigned long long)f;
    sb += (unsigned long long)(row - 1 - j) * f;
  }
  unsigned long long s[4] = {sa, sb, 0, 0};
  wg_sum4(s, lds);
  if (threadIdx.x == 0) {
    a.row_a[(int64_t)n * a.H + y] = (uint32_t)(s[0] % kPngAdlerMod);
    a.row_b[(int64_t)n * a.H + y] = (uint32_t)(s[1] % kPngAdlerMod);
  }
}

template <bool kPack>
__global__ void __launch_bounds__(kPngTokThreads) png_tokens_kernel(PngArgs a) {
  __shared__ uint32_t s_scan[kPngTokThreads / 64 + 1];
  __shared__ uint32_t s_tab[kPngTableStride];  // the histogram, or the block's codes: code | length << 16
  __shared__ uint32_t s_words[kPack ? kPngPackWords : 1];
  __shared__ unsigned long long s_before;
  const int tid = threadIdx.x;
  const int n = blockIdx.x / a.nblk, blk = blockIdx.x - n * a.nblk;
  const int ch = tile_channels(a.mode, a.colour[n]);
  if (ch == 0) return;
  const int64_t row = (int64_t)a.W * ch + 1;
  const int rows = a.H - blk * kPngBlockRows < kPngBlockRows ? a.H - blk * kPngBlockRows : kPngBlockRows;
  const int len = (int)(rows * row);  // at most 32 * 196606
  const uint8_t* src = a.filt + (uint64_t)n * a.filt_stride + (int64_t)blk * kPngBlockRows * row;
  const int64_t bi = (int64_t)n * a.nblk + blk;
  auto byte = [src](int64_t i) { return (int)src[i]; };
  uint32_t* words = a.words + (uint64_t)n * a.words_per_tile;
  uint64_t bitbase = 0;
  if (kPack) {
    for (int s = tid; s < kPngTableStride; s += kPngTokThreads) s_tab[s] = a.table[bi * kPngTableStride + s];
    if (tid == 0) s_before = 0;
    __syncthreads();
    unsigned long long before = 0;
    for (int b = tid; b < blk; b += kPngTokThreads) before += a.block_bits[(int64_t)n * a.nblk + b];
    if (before) atomicAdd(&s_before, before);
    __syncthreads();
    const uint64_t block_at = 16 + s_before;  // after the zlib header
    const uint32_t hb = a.hdr_bits[bi];
    for (int w = tid; (uint32_t)w * 32u < hb; w += kPngTokThreads)
      put_global(words, a.words_per_tile, block_at + 32ull * w, a.hdr[bi * kPngHeaderWords + w]);
    bitbase = block_at + hb;
  } else {
    for (int s = tid; s < kPngTableStride; s += kPngTokThreads) s_tab[s] = 0;
    __syncthreads();
  }
  int run_start = 0;
  for (int base = 0; base < len; base += kPngTokThreads) {
    const int i = base + tid;
    const bool valid = i < len;
    if (kPack) {
      for (int w = tid; w < kPngPackWords; w += kPngTokThreads) s_words[w] = 0;  // (the scans below synchronise before any OR)
    }
    const int v = valid ? (int)src[i] : 0;
    const int flag = (valid && (i == 0 || v != (int)src[i - 1])) ? i : -1;
    int last;
    int start = wg_scan_max(flag, reinterpret_cast<int*>(s_scan), &last);
    start = start > run_start ? start : run_start;
    run_start = last > run_start ? last : run_start;
    int length = 0, kind = 0;
    if (valid) kind = png_token(byte, i, len, i - start, &length);
    if (!kPack) {
      if (kind == 1) atomicAdd(&s_tab[v], 1u);
      if (kind == 2) {
        int e, eb;
        atomicAdd(&s_tab[png_length_symbol(length, &e, &eb)], 1u);
      }
    } else {
      uint32_t bits = 0, count = 0;
      if (kind == 1) {
        const uint32_t t = s_tab[v];
        bits = t & 0xFFFFu;
        count = t >> 16;
      } else if (kind == 2) {
        int e, eb;
        const uint32_t t = s_tab[png_length_symbol(length, &e, &eb)];
        bits = (t & 0xFFFFu) | ((uint32_t)e << (t >> 16));
        count = (t >> 16) + (uint32_t)eb + 1u;  // ... and the distance code `0`
      }
      uint32_t total;
      const uint32_t off = wg_scan_sum(count, s_scan, &total);
      const uint32_t first = (uint32_t)(bitbase & 31);
      if (count) {
        const uint32_t at = first + off;
        const unsigned long long sh = (unsigned long long)bits << (at & 31);
        if ((uint32_t)sh) atomicOr(&s_words[at >> 5], (uint32_t)sh);
        if ((uint32_t)(sh >> 32)) atomicOr(&s_words[(at >> 5) + 1], (uint32_t)(sh >> 32));
      }
      __syncthreads();
      const int nwords = (int)((first + total + 31) >> 5);
      const uint64_t w0 = bitbase >> 5;
      for (int w = tid; w < nwords; w += kPngTokThreads) {
        const uint32_t x = s_words[w];
        if (w0 + w < a.words_per_tile) {  // (always: the capacity bounds every block's bits)
          if (w == 0 || w == nwords - 1) {
            if (x) atomicOr(words + w0 + w, x);
          } else {
            words[w0 + w] = x;
          }
        }
      }
      __syncthreads();  // before the window is cleared again
      bitbase += total;
    }
  }
  if (kPack) {
    if (tid == 0) put_global(words, a.words_per_tile, bitbase, s_tab[kPngEob] & 0xFFFFu);
  } else {
    __syncthreads();
    for (int s = tid; s < kPngTableStride; s += kPngTokThreads)
      a.hist[bi * kPngTableStride + s] = s == kPngEob ? 1u : (s < kPngLitLen ? s_tab[s] : 0u);
  }
}

__global__ void __launch_bounds__(64) png_build_kernel(PngArgs a) {
  __shared__ PngScratch sc;
  __shared__ PngBlockCodes bc;
  __shared__ int s_used;
  const int lane = threadIdx.x;
  const int64_t bi = blockIdx.x;
  const int n = (int)(bi / a.nblk), blk = (int)(bi - (int64_t)n * a.nblk);
  if (tile_channels(a.mode, a.colour[n]) == 0) return;
  if (lane == 0) s_used = 0;
  for (int s = lane; s < 288; s += 64) sc.counts[s] = s < kPngLitLen ? a.hist[bi * kPngTableStride + s] : 0u;
  __syncthreads();
  int used = 0;
  for (int s = lane; s < kPngLitLen; s += 64)
    if (sc.counts[s]) {
      sc.sorted[png_rank(sc.counts, kPngLitLen, s)] = (uint16_t)s;
      ++used;
    }
  if (used) atomicAdd(&s_used, used);
  __syncthreads();
  if (lane == 0) {
    const uint32_t body = png_block_codes(sc, s_used, bc);
    HeaderWriter hw{a.hdr + bi * kPngHeaderWords, 0ull, 0, 0, 0u};
    png_block_header(sc, bc, blk == a.nblk - 1, hw);
    hw.finish();
    a.hdr_bits[bi] = hw.bits;
    a.block_bits[bi] = hw.bits + body;
  }
  __syncthreads();
  for (int s = lane; s < kPngTableStride; s += 64) a.table[bi * kPngTableStride + s] = (uint32_t)bc.codes[s] | ((uint32_t)bc.lens[s] << 16);
}

__global__ void __launch_bounds__(kPngThreads) png_finish_kernel(PngArgs a) {
  __shared__ unsigned long long lds[16];
  const int n = blockIdx.x;
  const int ch = tile_channels(a.mode, a.colour[n]);
  if (ch == 0) {
    if (threadIdx.x == 0) {
      a.stream_bytes[n] = 0;
      a.channels[n] = 0;
    }
    return;
  }
  const int64_t row = (int64_t)a.W * ch + 1, bytes_in = (int64_t)a.H * row;
  unsigned long long v[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < a.nblk; b += kPngThreads) v[0] += a.block_bits[(int64_t)n * a.nblk + b];
  for (int y = threadIdx.x; y < a.H; y += kPngThreads) {
    const uint32_t ra = a.row_a[(int64_t)n * a.H + y], rb = a.row_b[(int64_t)n * a.H + y];
    v[1] += ra;
    v[2] += png_adler_row_term(ra, rb, bytes_in - (int64_t)(y + 1) * row);
  }
  wg_sum4(v, lds);
  if (threadIdx.x == 0) {
    const uint64_t bytes = (16 + v[0] + 7) / 8 + 4;
    const uint32_t adler = png_adler_finish((uint32_t)(v[1] % kPngAdlerMod), (uint32_t)(v[2] % kPngAdlerMod), bytes_in);
    uint32_t* words = a.words + (uint64_t)n * a.words_per_tile;
    put_global(words, a.words_per_tile, 0, 0x9C78u);
    for (int i = 0; i < 4; ++i) put_global(words, a.words_per_tile, 8 * (bytes - 4 + i), (adler >> (24 - 8 * i)) & 255u);
    a.stream_bytes[n] = (int32_t)bytes;
    a.channels[n] = ch;
  }
}

// thread t of tile n: piece t of the stream
__global__ void __launch_bounds__(kPngThreads) png_crc_kernel(PngArgs a, int pieces_per_tile) {
  __shared__ uint32_t s_table[256];
  s_table[threadIdx.x] = png_crc_table_entry(threadIdx.x);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * kPngThreads + threadIdx.x;
  const int n = (int)(t / pieces_per_tile);  // (pieces_per_tile is a multiple of 256: a workgroup lies in one tile)
  const int64_t piece = t - (int64_t)n * pieces_per_tile;
  const uint64_t bytes = (uint64_t)a.stream_bytes[n], lo = (uint64_t)piece * kPngPiece;
  uint32_t out = 0;
  if (lo < bytes) {
    const uint64_t hi = lo + kPngPiece < bytes ? lo + kPngPiece : bytes;
    const uint4* src = reinterpret_cast<const uint4*>(a.words + (uint64_t)n * a.words_per_tile + lo / 4);
    uint32_t c = 0xFFFFFFFFu;
    int left = (int)(hi - lo);
    for (int q = 0; q < kPngPiece / 16 && left > 0; ++q) {
      const uint4 x = src[q];
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i < left) c = s_table[(c ^ (w[i >> 2] >> (8 * (i & 3)))) & 255u] ^ (c >> 8);
      }
      left -= 16;
    }
    out = png_crc_shift(~c, bytes - hi, c_png_crc_powers);
    if (piece == 0) out ^= png_crc_shift(kPngCrcIdat, bytes, c_png_crc_powers);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) out ^= __shfl_xor(out, d, 64);
  if ((threadIdx.x & 63) == 0 && out) atomicXor(a.crc + n, out);
}

__global__ void __launch_bounds__(kPngThreads) png_copy_kernel(PngArgs a, int64_t groups) {
  const int n = (int)(blockIdx.x / groups);
  const uint64_t w = (uint64_t)(blockIdx.x - (int64_t)n * groups) * kPngThreads + threadIdx.x;
  const uint64_t bytes = (uint64_t)a.stream_bytes[n], p = 4 * w;
  if (p >= bytes || w >= a.words_per_tile) return;
  const uint32_t x = a.words[(uint64_t)n * a.words_per_tile + w];
  uint8_t* dst = a.stream + (uint64_t)n * a.capacity + p;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (p + i < bytes && p + i < a.capacity) dst[i] = (uint8_t)(x >> (8 * i));
}

PngLayout png_workspace_layout(int N, int H, int W) {
  PngLayout l{};
  if (N <= 0 || H <= 0 || W <= 0 || H > kPngMaxSize || W > kPngMaxSize) return l;
  const PngGeom g = png_geom(H, W, 3);
  const size_t nb = (size_t)N * (size_t)g.blocks;
  // one tile's stream in words: whole 256-byte pieces of 64 words
  l.words_per_tile = (((size_t)png_stream_capacity(g) + 3) / 4 + 63) / 64 * 64;
  l.filt_per_tile = ((size_t)g.bytes + 15) / 16 * 16;
  size_t at = 0;
  const auto take = [&at](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  l.colour = take((size_t)N * sizeof(uint32_t));
  l.row_a = take((size_t)N * H * sizeof(uint32_t));
  l.row_b = take((size_t)N * H * sizeof(uint32_t));
  l.hist = take(nb * kPngTableStride * sizeof(uint32_t));
  l.table = take(nb * kPngTableStride * sizeof(uint32_t));
  l.hdr = take(nb * kPngHeaderWords * sizeof(uint32_t));
  l.hdr_bits = take(nb * sizeof(uint32_t));
  l.block_bits = take(nb * sizeof(uint32_t));
  l.filt = take((size_t)N * l.filt_per_tile);
  l.words = take((size_t)N * l.words_per_tile * sizeof(uint32_t));
  l.total = at;
  return l;
}

hipError_t launch_png_encode(const uint8_t* rgb, int N, int H, int W, int mode, uint8_t* stream, size_t capacity, int32_t* stream_bytes,
                             uint32_t* crc, int32_t* channels, void* workspace, hipStream_t s) {
  const PngLayout l = png_workspace_layout(N, H, W);
  char* ws = reinterpret_cast<char*>(workspace);
  PngArgs a;
  a.rgb = rgb;
  a.N = N;
  a.H = H;
  a.W = W;
  a.mode = mode;
  a.nblk = png_geom(H, W, 3).blocks;
  a.colour = reinterpret_cast<uint32_t*>(ws + l.colour);
  a.row_a = reinterpret_cast<uint32_t*>(ws + l.row_a);
  a.row_b = reinterpret_cast<uint32_t*>(ws + l.row_b);
  a.hist = reinterpret_cast<uint32_t*>(ws + l.hist);
  a.table = reinterpret_cast<uint32_t*>(ws + l.table);
  a.hdr = reinterpret_cast<uint32_t*>(ws + l.hdr);
  a.hdr_bits = reinterpret_cast<uint32_t*>(ws + l.hdr_bits);
  a.block_bits = reinterpret_cast<uint32_t*>(ws + l.block_bits);
  a.filt = reinterpret_cast<uint8_t*>(ws + l.filt);
  a.filt_stride = l.filt_per_tile;
  a.words = reinterpret_cast<uint32_t*>(ws + l.words);
  a.words_per_tile = l.words_per_tile;
  a.stream = stream;
  a.capacity = capacity;
  a.stream_bytes = stream_bytes;
  a.crc = crc;
  a.channels = channels;
  hipError_t e = hipMemsetAsync(a.colour, 0, (size_t)N * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.words, 0, (size_t)N * l.words_per_tile * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(crc, 0, (size_t)N * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((int64_t)N * a.nblk);
  if (mode != 0) {
    const int64_t per_tile = ((int64_t)H * W + kPngThreads - 1) / kPngThreads;
    const int groups = (int)(per_tile < 64 ? per_tile : 64);
    hipLaunchKernelGGL(png_grey_kernel, dim3((unsigned)(N * groups)), dim3(kPngThreads), 0, s, a, groups);
  }
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((int64_t)N * H)), dim3(kPngThreads), 0, s, a);
  hipLaunchKernelGGL(png_tokens_kernel<false>, dim3(blocks), dim3(kPngTokThreads), 0, s, a);
  hipLaunchKernelGGL(png_build_kernel, dim3(blocks), dim3(64), 0, s, a);
  hipLaunchKernelGGL(png_tokens_kernel<true>, dim3(blocks), dim3(kPngTokThreads), 0, s, a);
  hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)N), dim3(kPngThreads), 0, s, a);
  const int pieces_per_tile = (int)((l.words_per_tile * 4 / kPngPiece + kPngThreads - 1) / kPngThreads * kPngThreads);
  hipLaunchKernelGGL(png_crc_kernel, dim3((unsigned)((int64_t)N * pieces_per_tile / kPngThreads)), dim3(kPngThreads), 0, s, a, pieces_per_tile);
  const int64_t groups = (int64_t)((l.words_per_tile + kPngThreads - 1) / kPngThreads);
  hipLaunchKernelGGL(png_copy_kernel, dim3((unsigned)(N * groups)), dim3(kPngThreads), 0, s, a, groups);
  return hipGetLastError();
}

}  // namespace rfx
