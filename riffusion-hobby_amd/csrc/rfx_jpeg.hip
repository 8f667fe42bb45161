// rfx_jpeg.hip - baseline JPEG scans of (N, H, W, 3) uint8 RGB tiles on the device, the bytes libjpeg (Pillow) writes
// (rfx_jpeg_core.h).  Five kernels and one clear, all on the caller's stream:
//   1. jpg_blocks_kernel: one thread per block -> its 64 quantised coefficients in zigzag order (int16) and the bits its AC part
//      codes to.  Threads are dealt by component plane, so a wave holds one kind of block and neighbouring blocks.
//   2. jpg_bits_scan_kernel: one workgroup per image -> each block's bit offset (its DC difference needs only the DC of the
//      previous block of its component) and the image's bit total.
//   3. jpg_pack_kernel: one thread per block writes its bits at its offset into the zeroed unstuffed stream; the first and last
//      word of a block, shared with its neighbours, are merged with a vector atomic OR, the words between stored plainly.  The
//      image's last block adds the 1-bits that pad the scan to a byte.
//   4. jpg_ff_scan_kernel: one workgroup per image counts the 0xFF bytes of every 16-byte chunk and scans the counts.
//   5. jpg_stuff_kernel: one thread per chunk copies its bytes to their place in the scan, a 0x00 after every 0xFF; the last
//      chunk adds EOI and the image's size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_jpeg_core.h"
#include "rfx_kernels.h"

namespace rfx {

namespace {

constexpr int kJpgThreads = 256;
constexpr int kJpgScanThreads = 1024;  // the two per-image scans: one workgroup walks the image's items 1024 at a time
constexpr int kJpgChunk = 16;          // bytes of the unstuffed stream per thread of the last two kernels

__constant__ JpgTables c_jpg_tables = kJpgTables;

// coefficient z of a block held as 32 words of two int16
struct PackedCoef {
  const uint32_t* w;
  __device__ __forceinline__ int operator[](int z) const { return (int16_t)(w[z >> 1] >> (16 * (z & 1))); }
};

// exclusive scan of one value per thread over a workgroup of kJpgScanThreads; *total: the sum.  lds: 17 words.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // the previous round's readers are done with lds
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int w = 0; w < kJpgScanThreads / 64; ++w) {
      const uint32_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[kJpgScanThreads / 64] = run;
  }
  __syncthreads();
  *total = lds[kJpgScanThreads / 64];
  return lds[wave] + inc - v;
}

}  // namespace

// thread t of image n: plane k = t / mcus (0..3 Y blocks, 4 Cb, 5 Cr), MCU t % mcus
__global__ void __launch_bounds__(kJpgThreads) jpg_blocks_kernel(const uint8_t* __restrict__ rgb, int64_t total, JpgGeom g,
                                                                 const uint16_t* __restrict__ qtables, int16_t* __restrict__ coef,
                                                                 uint16_t* __restrict__ acbits) {
  const int64_t t = (int64_t)blockIdx.x * kJpgThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t n = t / g.blocks, r = t - n * g.blocks;
  const int k = (int)(r / g.mcus);
  const int64_t mcu = r - (int64_t)k * g.mcus;
  const int64_t b = n * g.blocks + mcu * 6 + k;
  const int tab = k < 4 ? 0 : 1;
  if (jpg_is_dummy(g, mcu, k)) {  // no pixels, no coefficients: DC difference 0 and an EOB
    acbits[b] = (uint16_t)(c_jpg_tables.ac[0].e[0] & 255);
    return;
  }
  const uint8_t* img = rgb + n * (int64_t)g.H * g.W * 3;
  const int mx = (int)(mcu % g.mcu_w), my = (int)(mcu / g.mcu_w);
  int s[64];
  if (k < 4) jpg_samples_y(img, g.H, g.W, 2 * mx + (k & 1), 2 * my + (k >> 1), s);
  else jpg_samples_c(img, g.H, g.W, mx, my, k - 3, s);
  jpg_fdct(s);
  const uint16_t* q = qtables + 64 * tab;
  uint32_t* out32 = reinterpret_cast<uint32_t*>(coef + b * 64);  // a block's 128 bytes start on a 128-byte boundary
#pragma unroll
  for (int z = 0; z < 64; z += 2) {
    const int a = jpg_quantise(s[kJpgNatural[z]], q[kJpgNatural[z]]), c = jpg_quantise(s[kJpgNatural[z + 1]], q[kJpgNatural[z + 1]]);
    out32[z >> 1] = ((uint32_t)a & 0xFFFFu) | ((uint32_t)c << 16);
  }
  int bits = 0;  // (read back through the pointer the words were written with)
  jpg_walk_ac(c_jpg_tables, tab, PackedCoef{out32}, false, [&](uint32_t, int len) { bits += len; });
  acbits[b] = (uint16_t)bits;
}

__global__ void __launch_bounds__(kJpgScanThreads) jpg_bits_scan_kernel(JpgGeom g, const int16_t* __restrict__ coef,
                                                                        const uint16_t* __restrict__ acbits,
                                                                        uint64_t* __restrict__ bitoff, uint64_t* __restrict__ bit_total) {
  __shared__ uint32_t lds[kJpgScanThreads / 64 + 1];
  const int64_t n = blockIdx.x;
  const int16_t* c = coef + n * g.blocks * 64;
  uint64_t carry = 0;
  for (int64_t base = 0; base < g.blocks; base += kJpgScanThreads) {
    const int64_t b = base + threadIdx.x;
    uint32_t bits = 0;
    if (b < g.blocks) {
      const int64_t mcu = b / 6;
      const int k = (int)(b - mcu * 6);
      jpg_walk_dc(c_jpg_tables, k < 4 ? 0 : 1, jpg_dc_diff(g, c, mcu, k), [&](uint32_t, int len) { bits += len; });
      bits += acbits[n * g.blocks + b];
    }
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(bits, lds, &total);
    if (b < g.blocks) bitoff[n * g.blocks + b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) bit_total[n] = carry;
}

__global__ void __launch_bounds__(kJpgThreads) jpg_pack_kernel(int64_t total, JpgGeom g, const int16_t* __restrict__ coef,
                                                               const uint64_t* __restrict__ bitoff, const uint64_t* __restrict__ bit_total,
                                                               uint32_t* __restrict__ words, uint64_t words_per_image) {
  const int64_t t = (int64_t)blockIdx.x * kJpgThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t n = t / g.blocks, b = t - n * g.blocks;
  const int64_t mcu = b / 6;
  const int k = (int)(b - mcu * 6);
  const int tab = k < 4 ? 0 : 1;
  const int16_t* c = coef + n * g.blocks * 64;
  uint32_t* w = words + n * words_per_image;
  const uint64_t off = bitoff[t];
  if (off + kJpgBlockMaxBits + 7 > words_per_image * 32) return;  // cannot happen: every block's bits are bounded
  auto merge = [w](int64_t i, uint32_t v) { atomicOr(w + i, v); };
  auto store = [w](int64_t i, uint32_t v) { w[i] = v; };
  JpgBitSink<decltype(merge), decltype(store)> sink(off, merge, store);
  jpg_walk_dc(c_jpg_tables, tab, jpg_dc_diff(g, c, mcu, k), sink);
  jpg_walk_ac(c_jpg_tables, tab, c + b * 64, jpg_is_dummy(g, mcu, k), sink);
  if (b == g.blocks - 1) {
    const int pad = (int)((0 - bit_total[n]) & 7);
    if (pad) sink((1u << pad) - 1, pad);
  }
  sink.finish();
}

__global__ void __launch_bounds__(kJpgScanThreads) jpg_ff_scan_kernel(const uint8_t* __restrict__ unstuffed, uint64_t bytes_per_image,
                                                                      const uint64_t* __restrict__ bit_total, uint32_t* __restrict__ ffpre,
                                                                      uint64_t chunks_per_image, int32_t* __restrict__ scan_bytes) {
  __shared__ uint32_t lds[kJpgScanThreads / 64 + 1];
  const int64_t n = blockIdx.x;
  const uint64_t ub = (bit_total[n] + 7) >> 3;
  const int64_t chunks = (int64_t)((ub + kJpgChunk - 1) / kJpgChunk);
  const uint4* src = reinterpret_cast<const uint4*>(unstuffed + n * bytes_per_image);
  uint32_t* pre = ffpre + n * chunks_per_image;
  uint64_t carry = 0;
  for (int64_t base = 0; base < chunks; base += kJpgScanThreads) {
    const int64_t c = base + threadIdx.x;
    uint32_t ff = 0;
    if (c < chunks) {  // (the bytes past the scan's end in its last chunk are the zeros of the clear)
      const uint4 v = src[c];
      const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) ff += ((x[i] >> (8 * j)) & 255u) == 255u;
    }
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(ff, lds, &total);
    if (c < chunks) pre[c] = (uint32_t)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) scan_bytes[n] = (int32_t)(ub + carry + 2);
}

__global__ void __launch_bounds__(kJpgThreads) jpg_stuff_kernel(int64_t total, const uint8_t* __restrict__ unstuffed, uint64_t bytes_per_image,
                                                                const uint64_t* __restrict__ bit_total, const uint32_t* __restrict__ ffpre,
                                                                uint64_t chunks_per_image, uint8_t* __restrict__ scan, uint64_t capacity) {
  const int64_t t = (int64_t)blockIdx.x * kJpgThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t n = t / (int64_t)chunks_per_image, c = t - n * (int64_t)chunks_per_image;
  const uint64_t ub = (bit_total[n] + 7) >> 3;
  const uint64_t at = (uint64_t)c * kJpgChunk;
  if (at >= ub) return;
  const int valid = ub - at < (uint64_t)kJpgChunk ? (int)(ub - at) : kJpgChunk;
  const bool last = at + kJpgChunk >= ub;
  const uint64_t o = at + ffpre[n * chunks_per_image + c];
  if (o + 2 * (uint64_t)valid + (last ? 2 : 0) > capacity) return;  // cannot happen: capacity is twice the unstuffed bound + 2
  const uint4 v = reinterpret_cast<const uint4*>(unstuffed + n * bytes_per_image)[c];
  const uint32_t x[4] = {v.x, v.y, v.z, v.w};
  uint8_t* dst = scan + n * capacity + o;
#pragma unroll
  for (int i = 0; i < kJpgChunk; ++i) {
    if (i < valid) {
      const uint32_t byte = (x[i >> 2] >> (8 * (i & 3))) & 255u;
      *dst++ = (uint8_t)byte;
      if (byte == 255u) *dst++ = 0;
    }
  }
  if (last) {
    dst[0] = 0xFF;
    dst[1] = 0xD9;
  }
}

JpgLayout jpeg_workspace_layout(int N, int H, int W) {
  JpgLayout l{};
  if (N <= 0 || H <= 0 || W <= 0 || H > kJpgMaxSize || W > kJpgMaxSize) return l;
  const JpgGeom g = jpg_geom(H, W);
  const size_t nb = (size_t)N * (size_t)g.blocks;
  // one image's unstuffed stream: whole 16-byte chunks, and a chunk of slack for the pack kernel's last partial word
  l.unstuffed_per_image = ((size_t)jpg_unstuffed_capacity(g) + 2 * kJpgChunk - 1) / kJpgChunk * kJpgChunk;
  l.chunks_per_image = l.unstuffed_per_image / kJpgChunk;
  size_t at = 0;
  const auto take = [&at](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  l.coef = take(nb * 64 * sizeof(int16_t));
  l.acbits = take(nb * sizeof(uint16_t));
  l.bitoff = take(nb * sizeof(uint64_t));
  l.bit_total = take((size_t)N * sizeof(uint64_t));
  l.unstuffed = take((size_t)N * l.unstuffed_per_image);
  l.ffpre = take((size_t)N * l.chunks_per_image * sizeof(uint32_t));
  l.total = at;
  return l;
}

hipError_t launch_jpeg_encode(const uint8_t* rgb, int N, int H, int W, const uint16_t* qtables, uint8_t* scan, size_t capacity,
                              int32_t* scan_bytes, void* workspace, hipStream_t s) {
  const JpgGeom g = jpg_geom(H, W);
  const JpgLayout l = jpeg_workspace_layout(N, H, W);
  char* ws = reinterpret_cast<char*>(workspace);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
  uint16_t* acbits = reinterpret_cast<uint16_t*>(ws + l.acbits);
  uint64_t* bitoff = reinterpret_cast<uint64_t*>(ws + l.bitoff);
  uint64_t* bit_total = reinterpret_cast<uint64_t*>(ws + l.bit_total);
  uint8_t* unstuffed = reinterpret_cast<uint8_t*>(ws + l.unstuffed);
  uint32_t* ffpre = reinterpret_cast<uint32_t*>(ws + l.ffpre);
  const int64_t nblocks = (int64_t)N * g.blocks, nchunks = (int64_t)N * (int64_t)l.chunks_per_image;
  const auto grid = [](int64_t items) { return dim3((unsigned)((items + kJpgThreads - 1) / kJpgThreads)); };
  hipError_t e = hipMemsetAsync(unstuffed, 0, (size_t)N * l.unstuffed_per_image, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jpg_blocks_kernel, grid(nblocks), dim3(kJpgThreads), 0, s, rgb, nblocks, g, qtables, coef, acbits);
  hipLaunchKernelGGL(jpg_bits_scan_kernel, dim3((unsigned)N), dim3(kJpgScanThreads), 0, s, g, coef, acbits, bitoff, bit_total);
  hipLaunchKernelGGL(jpg_pack_kernel, grid(nblocks), dim3(kJpgThreads), 0, s, nblocks, g, coef, bitoff, bit_total,
                     reinterpret_cast<uint32_t*>(unstuffed), (uint64_t)(l.unstuffed_per_image / 4));
  hipLaunchKernelGGL(jpg_ff_scan_kernel, dim3((unsigned)N), dim3(kJpgScanThreads), 0, s, unstuffed, (uint64_t)l.unstuffed_per_image, bit_total,
                     ffpre, (uint64_t)l.chunks_per_image, scan_bytes);
  hipLaunchKernelGGL(jpg_stuff_kernel, grid(nchunks), dim3(kJpgThreads), 0, s, nchunks, unstuffed, (uint64_t)l.unstuffed_per_image, bit_total,
                     ffpre, (uint64_t)l.chunks_per_image, scan, (uint64_t)capacity);
  return hipGetLastError();
}

}  // namespace rfx
