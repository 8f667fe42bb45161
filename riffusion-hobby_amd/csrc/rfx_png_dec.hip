// rfx_png_dec.hip - the zlib streams of PNG tiles to (N, H, W, 3) uint8 RGB tiles on the device, the pixels Pillow gives
// (rfx_png_dec_core.h holds the decoder; this file gives it its lanes, its LDS and its loads and stores).  Two kernels on the
// caller's stream; no workgroup waits for another one:
//   1. png_inflate_kernel: one workgroup of one wave per image.  A deflate stream is a chain - every symbol starts where the one
//      before ended - so the wave's lanes decode it alike, from the same bytes, and share the work that is not a chain: building
//      a block's decode tables, copying a match (lane i takes byte i), moving stored bytes, and streaming the 32 KiB window,
//      which is a ring in LDS, out to the image's filtered bytes in whole 256-byte lines with the Adler-32 on the way.  The stream
//      comes through a 4 KiB staging buffer in LDS, loaded 16 bytes per lane.
//   2. png_unfilter_kernel: one workgroup per image, rows in order, a row (or a piece of kPngdSegBytes of it) and the row above in
//      LDS: None and Up across the row, Sub, Average and Paeth along it with one lane per channel; then the RGB bytes, stored
//      across the row.
// Every read of a stream is inside [offsets[0] rounded down to 16, offsets[N]) of d_streams, every other access inside the buffers
// the layout and the entry give: whatever the bytes of the stream are.  Every loop ends with the input or the output it consumes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_kernels.h"
#include "rfx_png_dec_core.h"

namespace rfx {

namespace {

constexpr int kPngdInflateThreads = 64;  // one wave
constexpr int kPngdUnfilterThreads = 256;
constexpr int kPngdStageBytes = 4096;
static_assert(kPngdInflateThreads <= kPngdMaxLanes, "the Adler-32 partial sums are one pair per lane");

template <int THREADS>
struct Group {
  __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int lanes() const { return THREADS; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// the image's stream through the staging buffer: stage[0] is byte `base` of d_streams (a multiple of 16)
struct StreamFetch {
  const uint8_t* streams;
  int64_t lo, end_all;
  uint4* stage;
  int64_t base;
  __device__ __forceinline__ void load(int64_t a) {
    __syncthreads();  // (the bytes staged before are not needed any more)
    base = a & ~(int64_t)15;
    for (int v = (int)threadIdx.x; v < kPngdStageBytes / 16; v += kPngdInflateThreads) {
      const int64_t g = base + 16 * (int64_t)v;
      uint4 q = make_uint4(0, 0, 0, 0);
      if (g + 16 <= end_all) {
        q = *reinterpret_cast<const uint4*>(streams + g);
      } else {
        uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (g + j < end_all) word[j >> 2] |= (uint32_t)streams[g + j] << (8 * (j & 3));
        q = make_uint4(word[0], word[1], word[2], word[3]);
      }
      stage[v] = q;
    }
    __syncthreads();
  }
  // all lanes, the same i: bytes i .. i + 3 of the image's n, those at or past n as zeros
  __device__ __forceinline__ uint32_t word(uint32_t i, uint32_t n) {
    if (i >= n) return 0;
    const int64_t a = lo + (int64_t)i;
    if (a < base || a + 4 > base + kPngdStageBytes) load(a);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(stage);
    const uint32_t at = (uint32_t)(a - base);  // at most kPngdStageBytes - 4: both words are staged
    const uint64_t two = (uint64_t)words[at >> 2] | (uint64_t)words[(at >> 2) + (at & 3 ? 1 : 0)] << 32;
    const uint32_t v = (uint32_t)(two >> (8 * (at & 3)));
    const uint32_t left = n - i;
    return pngd_uni(left >= 4 ? v : v & ((1u << (8 * left)) - 1));
  }
  __device__ __forceinline__ uint8_t at(uint32_t i) const { return streams[lo + (int64_t)i]; }
};

struct FilteredStore {
  uint8_t* base;
  __device__ __forceinline__ void word(uint64_t i, uint32_t v) const { *reinterpret_cast<uint32_t*>(base + i) = v; }
  __device__ __forceinline__ void byte(uint64_t i, uint8_t v) const { base[i] = v; }
};
struct FilteredImage {
  uint8_t* base;
  __device__ __forceinline__ uint8_t byte(uint64_t i) const { return base[i]; }
  __device__ __forceinline__ void put(uint64_t i, uint8_t v) const { base[i] = v; }
};
struct RgbStore {
  uint8_t* base;
  __device__ __forceinline__ void operator()(uint64_t i, uint8_t v) const { base[i] = v; }
};

__global__ __launch_bounds__(kPngdInflateThreads) void png_inflate_kernel(const uint8_t* __restrict__ streams, const int64_t* __restrict__ offsets, int N,
                                                                         uint64_t expected, uint8_t* __restrict__ filtered, size_t per_image,
                                                                         int32_t* __restrict__ status) {
  __shared__ PngdInflateShared sh;
  __shared__ uint4 stage[kPngdStageBytes / 16];
  const int n = (int)blockIdx.x;
  const int64_t lo = offsets[n], hi = offsets[n + 1], end_all = offsets[N];
  int result;
  if (lo < 0 || hi < lo || hi > end_all || hi - lo > kPngdMaxStreamBytes) {
    result = kPngdInputEnds;  // offsets that are not the host's: nothing is read
  } else {
    StreamFetch in{streams, lo, end_all, stage, -((int64_t)1 << 40)};
    FilteredStore out{filtered + (size_t)n * per_image};
    result = pngd_inflate(Group<kPngdInflateThreads>(), in, (uint32_t)(hi - lo), expected, out, &sh);
  }
  if (threadIdx.x == 0) status[n] = result;
}

__global__ __launch_bounds__(kPngdUnfilterThreads) void png_unfilter_kernel(uint8_t* filtered, size_t per_image, int H, int W, int color_type,
                                                                           const uint8_t* __restrict__ palettes, const int32_t* __restrict__ palette_entries,
                                                                           uint8_t* __restrict__ rgb, int32_t* __restrict__ status) {
  __shared__ PngdUnfilterShared sh;
  const int n = (int)blockIdx.x;
  if (status[n] != kPngdOk) return;  // (the same for every lane)
  int entries = 0;
  if (color_type == 3) {
    entries = palette_entries[n];
    entries = entries < 0 ? 0 : entries > 256 ? 256 : entries;
  }
  FilteredImage filt{filtered + (size_t)n * per_image};
  RgbStore out{rgb + (size_t)n * (size_t)H * (size_t)W * 3};
  const int result = pngd_unfilter_image(Group<kPngdUnfilterThreads>(), filt, H, W, color_type, color_type == 3 ? palettes + (size_t)n * 768 : nullptr,
                                         entries, out, &sh);
  if (threadIdx.x == 0 && result != kPngdOk) status[n] = result;
}

}  // namespace

hipError_t launch_png_decode(const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int color_type, const uint8_t* palettes,
                             const int32_t* palette_entries, uint8_t* rgb, int32_t* status, void* workspace, hipStream_t s) {
  const PngdLayout l = png_decode_workspace_layout(N, H, W, color_type);
  uint8_t* filtered = reinterpret_cast<uint8_t*>(workspace) + l.filtered;
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)N), dim3(kPngdInflateThreads), 0, s, streams, offsets, N,
                     pngd_filtered_bytes(H, W, pngd_bpp(color_type)), filtered, l.per_image, status);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)N), dim3(kPngdUnfilterThreads), 0, s, filtered, l.per_image, H, W, color_type, palettes,
                     palette_entries, rgb, status);
  return hipGetLastError();
}

}  // namespace rfx
