// rfx_jpeg_dec.hip - baseline JPEG scans to (N, H, W, 3) uint8 RGB tiles on the device, the pixels libjpeg-turbo (Pillow) decodes
// (rfx_jpeg_dec_core.h).  Six kernels and one clear, all on the caller's stream; no workgroup waits for another one:
//   1. jpd_unstuff_scan_kernel: one workgroup per image counts, per aligned 16-byte chunk of its scan, the 0x00 bytes that follow
//      a 0xFF, and scans the counts; a 0xFF followed by anything else is the image's status.
//   2. jpd_unstuff_kernel: one thread per chunk copies its bytes without those zeros to their place in the image's region.
//   3. jpd_entropy_kernel: one workgroup per image, one thread per subsequence of kJpdSubBits bits, kJpdGroup subsequences at a
//      time with their bits and the image's four Huffman tables in LDS.  Every thread decodes its subsequence from an assumed
//      state, then in rounds from its predecessor's exit state while that state changes (__syncthreads and a flag in LDS; at most
//      as many rounds as the group has subsequences, since the first starts from the truth); a scan of the block counts gives
//      every subsequence its first block, and a last pass writes the coefficients (natural order, DC as differences) into the
//      cleared buffer.  The group's last exit state is the next group's truth.
//   4. jpd_dc_scan_kernel: one workgroup per image turns the DC differences into values, per component in scan order.
//   5. jpd_idct_kernel: one thread per block dequantises, transforms and writes 8 x 8 samples of its plane.
//   6. jpd_pixels_kernel: one thread per pixel upsamples the two chroma planes and converts to RGB.
// Every read of a scan is inside [offsets[0], offsets[N]) of d_scans rounded down to 16 bytes at the front, every read of the bit
// stream inside the image's region, every write inside the buffers the layout gives: whatever the bytes of the scan are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_jpeg_dec_core.h"
#include "rfx_kernels.h"

namespace rfx {

namespace {

constexpr int kJpdThreads = 256;
constexpr int kJpdScanThreads = 1024;
constexpr int kJpdChunk = 16;
// a group's words in LDS: one word of padding after every 32, so that threads at the same place of their subsequences are on
// different banks; two words more for the peek of the last subsequence
constexpr int kJpdLdsWords = kJpdGroup * kJpdSubWords + 2;
__device__ __forceinline__ int lds_word(int j) { return j + (j >> 5); }

// exclusive scan of one value per thread over a workgroup of THREADS; *total: the sum.  lds: THREADS / 64 + 1 words.
template <int THREADS>
__device__ __forceinline__ int32_t block_exclusive_scan(int32_t v, int32_t* lds, int32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();  // the previous scan's readers are done with lds
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t run = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
      const int32_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[THREADS / 64] = run;
  }
  __syncthreads();
  *total = lds[THREADS / 64];
  return lds[wave] + inc - v;
}

// the 16 bytes of the aligned chunk at `at` of the scans (total bytes) and the byte before them; bytes outside [lo, hi) read as
// 0x00 (before `lo`: nothing to stuff after; from `hi`: nothing)
struct JpdChunkBytes {
  uint8_t prev, b[kJpdChunk];
};
__device__ __forceinline__ JpdChunkBytes load_chunk(const uint8_t* __restrict__ scans, int64_t total, int64_t at, int64_t lo, int64_t hi) {
  JpdChunkBytes c;
  if (at + kJpdChunk <= total) {
    const uint4 v = *reinterpret_cast<const uint4*>(scans + at);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < kJpdChunk; ++i) c.b[i] = (uint8_t)(x[i >> 2] >> (8 * (i & 3)));
  } else {
#pragma unroll
    for (int i = 0; i < kJpdChunk; ++i) c.b[i] = at + i < total ? scans[at + i] : (uint8_t)0;
  }
#pragma unroll
  for (int i = 0; i < kJpdChunk; ++i)
    if (at + i < lo || at + i >= hi) c.b[i] = 0;
  c.prev = at - 1 >= lo ? scans[at - 1] : (uint8_t)0;
  return c;
}

}  // namespace

__global__ void __launch_bounds__(kJpdScanThreads) jpd_unstuff_scan_kernel(const uint8_t* __restrict__ scans, const int64_t* __restrict__ offsets,
                                                                           int N, uint32_t* __restrict__ pre, uint32_t* __restrict__ ulen,
                                                                           int32_t* __restrict__ status) {
  __shared__ int32_t lds[kJpdScanThreads / 64 + 1];
  __shared__ int s_marker;
  const int64_t n = blockIdx.x;
  const int64_t lo = offsets[n], hi = offsets[n + 1], total = offsets[N], first = lo & ~(int64_t)15;
  const int64_t chunks = (hi - first + kJpdChunk - 1) / kJpdChunk;
  uint32_t* p = pre + jpd_chunk_offset(lo, offsets[0], n);
  if (threadIdx.x == 0) s_marker = 0;
  __syncthreads();
  uint32_t carry = 0;
  for (int64_t base = 0; base < chunks; base += kJpdScanThreads) {
    const int64_t c = base + threadIdx.x;
    int32_t drops = 0;
    if (c < chunks) {
      const JpdChunkBytes v = load_chunk(scans, total, first + c * kJpdChunk, lo, hi);
      uint8_t before = v.prev;
      bool marker = false;
#pragma unroll
      for (int i = 0; i < kJpdChunk; ++i) {
        drops += before == 0xFF && v.b[i] == 0 && first + c * kJpdChunk + i < hi;
        marker |= before == 0xFF && v.b[i] != 0;
        before = v.b[i];
      }
      if (marker) s_marker = 1;
    }
    int32_t total_drops;
    const int32_t ex = block_exclusive_scan<kJpdScanThreads>(drops, lds, &total_drops);
    if (c < chunks) p[c] = carry + (uint32_t)ex;
    carry += (uint32_t)total_drops;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool dangling = hi > lo && scans[hi - 1] == 0xFF;
    ulen[n] = (uint32_t)(hi - lo) - carry;
    status[n] = s_marker || dangling ? kJpdMarker : kJpdOk;
  }
}

// grid (N, y): the threads of an image's workgroups stride over its chunks
__global__ void __launch_bounds__(kJpdThreads) jpd_unstuff_kernel(const uint8_t* __restrict__ scans, const int64_t* __restrict__ offsets, int N,
                                                                  const uint32_t* __restrict__ pre, uint8_t* __restrict__ unstuffed) {
  const int64_t n = blockIdx.x;
  const int64_t lo = offsets[n], hi = offsets[n + 1], total = offsets[N], first = lo & ~(int64_t)15;
  const int64_t chunks = (hi - first + kJpdChunk - 1) / kJpdChunk;
  const uint32_t* p = pre + jpd_chunk_offset(lo, offsets[0], n);
  uint8_t* out = unstuffed + jpd_region_offset(lo, offsets[0], n);
  for (int64_t c = (int64_t)blockIdx.y * kJpdThreads + threadIdx.x; c < chunks; c += (int64_t)gridDim.y * kJpdThreads) {
    const int64_t at = first + c * kJpdChunk;
    const JpdChunkBytes v = load_chunk(scans, total, at, lo, hi);
    // bytes of the image before this chunk, less the zeros dropped before it (never negative; the first chunk may start before lo)
    int64_t o = (at > lo ? at - lo : 0) - (int64_t)p[c];
    uint8_t before = v.prev;
#pragma unroll
    for (int i = 0; i < kJpdChunk; ++i) {
      if (at + i >= lo && at + i < hi && !(before == 0xFF && v.b[i] == 0)) out[o++] = v.b[i];
      before = v.b[i];
    }
  }
}

__global__ void __launch_bounds__(kJpdGroup) jpd_entropy_kernel(const uint8_t* __restrict__ unstuffed, const int64_t* __restrict__ offsets,
                                                                const uint32_t* __restrict__ ulen, const uint8_t* __restrict__ huff, JpgGeom g,
                                                                int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  __shared__ JpdHuff tables[4];
  __shared__ uint32_t bits[kJpdLdsWords + kJpdLdsWords / 32 + 1];
  __shared__ JpdState exit_state[kJpdGroup];
  __shared__ int32_t scan_lds[kJpdGroup / 64 + 1];
  __shared__ int s_flag[2], s_bad;
  __shared__ JpdState s_carry;
  __shared__ int64_t s_block_base;
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  const uint8_t* h = huff + n * 4 * kJpdHuffBytes;
  if (tid == 0) {
    s_flag[0] = s_flag[1] = s_bad = 0;
    s_carry = JpdState{0, 0, 0, 1, 0};
    s_block_base = 0;
  }
  __syncthreads();
  if (tid < 4 && !jpd_huff_derive(h + tid * kJpdHuffBytes, &tables[tid])) s_bad = 1;
  for (int i = tid; i < 4 * 256; i += kJpdGroup) tables[i >> 8].huffval[i & 255] = h[(i >> 8) * kJpdHuffBytes + 16 + (i & 255)];
  __syncthreads();
  if (s_bad) {  // (uniform)
    if (tid == 0) atomicMax(status + n, kJpdBadTable);
    return;
  }
  for (int i = tid; i < 4 << kJpdLutBits; i += kJpdGroup) tables[i >> kJpdLutBits].lut[i & ((1 << kJpdLutBits) - 1)] = jpd_huff_lut_entry(tables[i >> kJpdLutBits], i & ((1 << kJpdLutBits) - 1));

  const uint32_t bytes = ulen[n], total_bits = bytes * 8u;
  const int64_t region_words = ((int64_t)bytes + 3) / 4 + 2;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(unstuffed + jpd_region_offset(offsets[n], offsets[0], n));
  const int64_t nsub = ((int64_t)total_bits + kJpdSubBits - 1) / kJpdSubBits;
  int16_t* out_coef = coef + n * g.blocks * 64;
  const auto no_emit = [](int64_t, int, int) {};

  for (int64_t base = 0; base < nsub; base += kJpdGroup) {
    __syncthreads();  // the tables; the carry and the block base of the group before
    const JpdState carry = s_carry;
    const int64_t block_base = s_block_base;
    if (!carry.valid || block_base >= g.blocks) break;  // (uniform)
    const int count = (int)(nsub - base < kJpdGroup ? nsub - base : kJpdGroup);
    for (int j = tid; j < count * kJpdSubWords + 2; j += kJpdGroup) {
      const int64_t w = base * kJpdSubWords + j;
      bits[lds_word(j)] = w < region_words ? __builtin_bswap32(words[w]) : 0u;
    }
    __syncthreads();
    const int64_t word_base = base * kJpdSubWords;
    const auto peek = [&](uint32_t p) {
      const int j = (int)((int64_t)(p >> 5) - word_base);
      const uint64_t two = ((uint64_t)bits[lds_word(j)] << 32) | bits[lds_word(j + 1)];
      return (uint32_t)((two << (p & 31)) >> 32);
    };
    const bool active = tid < count;
    const uint32_t lo = (uint32_t)((base + tid) * kJpdSubBits);
    const int64_t e64 = (base + tid + 1) * kJpdSubBits;
    const uint32_t end = (uint32_t)(e64 < (int64_t)total_bits ? e64 : (int64_t)total_bits);
    JpdState last_in, mine;
    int64_t blocks = 0;
    const auto decodable = [&](const JpdState& in) { return in.valid && in.p >= lo && in.p < end; };
    const auto run = [&](const JpdState& in) {
      last_in = in;
      int err;
      if (!decodable(in)) {  // nothing to decode from: a state the true one will replace
        mine = JpdState{end, 0, 0, 0, 0};
        blocks = 0;
      } else {
        mine = jpd_decode_span<true>(tables, peek, in, end, total_bits, INT64_MAX, no_emit, &blocks, &err);
      }
      exit_state[tid] = mine;
    };
    if (active) run(tid ? JpdState{lo, 0, 0, 1, 0} : carry);
    for (int r = 1; r <= count; ++r) {
      __syncthreads();  // the exit states of the round before
      JpdState in = carry;
      if (active && tid) in = exit_state[tid - 1];
      __syncthreads();  // ... are read before any is replaced
      if (tid == 0) s_flag[(r + 1) & 1] = 0;
      if (active && !jpd_same(in, last_in)) {
        run(in);
        s_flag[r & 1] = 1;
      }
      __syncthreads();
      if (!s_flag[r & 1]) break;  // (uniform) no state changed: every one is the true one
    }
    int32_t group_blocks;
    const int32_t before = block_exclusive_scan<kJpdGroup>(active ? (int32_t)blocks : 0, scan_lds, &group_blocks);
    if (active && decodable(last_in)) {
      const int64_t first = block_base + before, room = g.blocks - first;
      if (room > 0) {
        int16_t* out = out_coef + first * 64;
        int64_t nb;
        int err;
        const JpdState at = jpd_decode_span<false>(tables, peek, last_in, end, total_bits, room,
                                                   [&](int64_t b, int k, int v) { out[b * 64 + kJpgNatural[k]] = (int16_t)v; }, &nb, &err);
        if (err != kJpdOk) atomicMax(status + n, err);
        else if (nb == room && total_bits - at.p > 7) atomicMax(status + n, kJpdLeftOver);
      }
    }
    if (tid == count - 1) {
      s_carry = mine;
      s_block_base = block_base + group_blocks;
    }
  }
  __syncthreads();
  if (tid == 0 && s_block_base < g.blocks) atomicMax(status + n, kJpdLeftOver);
}

__global__ void __launch_bounds__(kJpdScanThreads) jpd_dc_scan_kernel(JpgGeom g, int16_t* __restrict__ coef) {
  __shared__ int32_t lds[kJpdScanThreads / 64 + 1];
  int16_t* c = coef + (int64_t)blockIdx.x * g.blocks * 64;
  int32_t carry[3] = {0, 0, 0};
  for (int64_t base = 0; base < g.mcus; base += kJpdScanThreads) {
    const int64_t mcu = base + threadIdx.x;
    int32_t d[6] = {0, 0, 0, 0, 0, 0};
    if (mcu < g.mcus) {
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = c[(mcu * 6 + k) * 64];
    }
    const int32_t sums[3] = {d[0] + d[1] + d[2] + d[3], d[4], d[5]};
    int32_t ex[3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      int32_t total;
      ex[comp] = carry[comp] + block_exclusive_scan<kJpdScanThreads>(sums[comp], lds, &total);
      carry[comp] += total;
    }
    if (mcu < g.mcus) {
      int32_t y = ex[0];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        y += d[k];
        c[(mcu * 6 + k) * 64] = (int16_t)y;
      }
      c[(mcu * 6 + 4) * 64] = (int16_t)(ex[1] + d[4]);
      c[(mcu * 6 + 5) * 64] = (int16_t)(ex[2] + d[5]);
    }
  }
}

// thread t of image n: plane k = t / mcus (0 .. 3 Y blocks, 4 Cb, 5 Cr), MCU t % mcus, as the encoder deals them
__global__ void __launch_bounds__(kJpdThreads) jpd_idct_kernel(int64_t total, JpgGeom g, const int16_t* __restrict__ coef,
                                                               const uint16_t* __restrict__ qtables, uint8_t* __restrict__ planes) {
  const int64_t t = (int64_t)blockIdx.x * kJpdThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t n = t / g.blocks, r = t - n * g.blocks;
  const int k = (int)(r / g.mcus);
  const int64_t mcu = r - (int64_t)k * g.mcus;
  const int mx = (int)(mcu % g.mcu_w), my = (int)(mcu / g.mcu_w);
  const uint4* in = reinterpret_cast<const uint4*>(coef + (n * g.blocks + mcu * 6 + k) * 64);  // 128 bytes on a 128-byte boundary
  int c[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = in[i];
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[8 * i + 2 * j] = (int16_t)(x[j] & 0xFFFFu);
      c[8 * i + 2 * j + 1] = (int16_t)(x[j] >> 16);
    }
  }
  jpd_dequant_idct(c, qtables + (n * 2 + (k < 4 ? 0 : 1)) * 64);
  uint8_t* img = planes + n * jpd_plane_bytes(g);
  const int stride = k < 4 ? 16 * g.mcu_w : 8 * g.mcu_w;
  uint8_t* dst = k < 4 ? img + ((int64_t)(16 * my + 8 * (k >> 1)) * stride + 16 * mx + 8 * (k & 1))
                       : img + 256 * g.mcus + (k - 4) * 64 * g.mcus + ((int64_t)8 * my * stride + 8 * mx);
#pragma unroll
  for (int row = 0; row < 8; ++row) {
    uint2 v;
    v.x = (uint32_t)c[8 * row] | ((uint32_t)c[8 * row + 1] << 8) | ((uint32_t)c[8 * row + 2] << 16) | ((uint32_t)c[8 * row + 3] << 24);
    v.y = (uint32_t)c[8 * row + 4] | ((uint32_t)c[8 * row + 5] << 8) | ((uint32_t)c[8 * row + 6] << 16) | ((uint32_t)c[8 * row + 7] << 24);
    *reinterpret_cast<uint2*>(dst + (int64_t)row * stride) = v;  // 8 bytes on an 8-byte boundary
  }
}

__global__ void __launch_bounds__(kJpdThreads) jpd_pixels_kernel(int64_t total, JpgGeom g, const uint8_t* __restrict__ planes,
                                                                 uint8_t* __restrict__ rgb) {
  const int64_t t = (int64_t)blockIdx.x * kJpdThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t per = (int64_t)g.H * g.W, n = t / per, r = t - n * per;
  const int y = (int)(r / g.W), x = (int)(r - (int64_t)y * g.W);
  const uint8_t* img = planes + n * jpd_plane_bytes(g);
  const uint8_t* cb = img + 256 * g.mcus;
  const uint8_t* cr = cb + 64 * g.mcus;
  uint8_t px[3];
  jpd_rgb(img[(int64_t)y * 16 * g.mcu_w + x], jpd_upsample(cb, 8 * g.mcu_w, g.H, g.W, x, y), jpd_upsample(cr, 8 * g.mcu_w, g.H, g.W, x, y), px);
  rgb[t * 3] = px[0];
  rgb[t * 3 + 1] = px[1];
  rgb[t * 3 + 2] = px[2];
}

hipError_t launch_jpeg_decode(const uint8_t* scans, const int64_t* offsets, int64_t max_scan_bytes, size_t total_scan_bytes, int N, int H, int W,
                              const uint16_t* qtables, const uint8_t* huff, uint8_t* rgb, int32_t* status, void* workspace, hipStream_t s) {
  const JpgGeom g = jpg_geom(H, W);
  const JpdLayout l = jpeg_decode_workspace_layout(N, H, W, total_scan_bytes);
  char* ws = reinterpret_cast<char*>(workspace);
  uint8_t* unstuffed = reinterpret_cast<uint8_t*>(ws + l.unstuffed);
  uint32_t* pre = reinterpret_cast<uint32_t*>(ws + l.pre);
  uint32_t* ulen = reinterpret_cast<uint32_t*>(ws + l.ulen);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
  uint8_t* planes = reinterpret_cast<uint8_t*>(ws + l.planes);
  const int64_t nblocks = (int64_t)N * g.blocks, npixels = (int64_t)N * H * W;
  const auto grid = [](int64_t items) { return dim3((unsigned)((items + kJpdThreads - 1) / kJpdThreads)); };
  const int64_t chunk_groups = (max_scan_bytes / kJpdChunk + 2 + kJpdThreads - 1) / kJpdThreads;
  hipError_t e = hipMemsetAsync(coef, 0, l.coef_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jpd_unstuff_scan_kernel, dim3((unsigned)N), dim3(kJpdScanThreads), 0, s, scans, offsets, N, pre, ulen, status);
  hipLaunchKernelGGL(jpd_unstuff_kernel, dim3((unsigned)N, (unsigned)(chunk_groups < 64 ? chunk_groups : 64)), dim3(kJpdThreads), 0, s, scans,
                     offsets, N, pre, unstuffed);
  hipLaunchKernelGGL(jpd_entropy_kernel, dim3((unsigned)N), dim3(kJpdGroup), 0, s, unstuffed, offsets, ulen, huff, g, coef, status);
  hipLaunchKernelGGL(jpd_dc_scan_kernel, dim3((unsigned)N), dim3(kJpdScanThreads), 0, s, g, coef);
  hipLaunchKernelGGL(jpd_idct_kernel, grid(nblocks), dim3(kJpdThreads), 0, s, nblocks, g, coef, qtables, planes);
  hipLaunchKernelGGL(jpd_pixels_kernel, grid(npixels), dim3(kJpdThreads), 0, s, npixels, g, planes, rgb);
  return hipGetLastError();
}

}  // namespace rfx
