// rfx_resize.hip - PIL.Image.resize of (N, H, W, 3) uint8 RGB tiles on the device, byte for byte (rfx_resize_core.h):
//   * horizontal pass: one workgroup per block of rows (rows of all tiles are contiguous, and the pass is per row).  The
//     block's input bytes are staged in LDS with 16-byte loads; each lane then takes four consecutive output pixels (12
//     bytes) of the block and writes them as three dwords.  The coefficient table is read-only and shared by every row: L2
//     serves it.
//   * vertical pass: one wave per output row; the row's weights are wave-uniform, and consecutive lanes take consecutive
//     bytes of the row, so every tap is one coalesced 64-byte load per wave.  (A form with 16 bytes per lane from 16-byte
//     loads returned wrong values for bytes 2 and 3 of each dword in its one GPU run, cause not found; it was dropped, as
//     audio-to-audio never changes the height.)
// The op is memory-bound: 5 taps for 501 -> 512, 7 for 512 -> 501.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_kernels.h"
#include "rfx_resize_core.h"

namespace rfx {

namespace {

constexpr int kRszThreads = 256;
constexpr int kRszStageBytes = 24576;  // input bytes a horizontal workgroup stages (whole rows; at least one row)

// rows per horizontal workgroup: as many whole rows as fit the staging budget, a multiple of four when there are four or
// more (then every block's output starts on a dword whenever the output does, even for odd row lengths)
int rsz_rows_per_block(int W) {
  int r = kRszStageBytes / (W * 3);
  if (r < 1) r = 1;
  if (r > 32) r = 32;
  if (r >= 4) r &= ~3;
  return r;
}

}  // namespace

__global__ void __launch_bounds__(kRszThreads) rsz_h_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t rows,
                                                            int W, int OW, int rows_per_block, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ kk, int ksize) {
  extern __shared__ uint4 rsz_stage_v[];
  uint8_t* stage = reinterpret_cast<uint8_t*>(rsz_stage_v);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int nr = (int)(rows - r0 < rows_per_block ? rows - r0 : rows_per_block);
  const int64_t IB = (int64_t)W * 3, OB = (int64_t)OW * 3;

  // ---- stage input bytes [r0 IB, (r0 + nr) IB) at LDS offset skew + j, skew = the span's offset inside its 16-byte chunk
  const uint8_t* g = in + r0 * IB;
  const int64_t span = nr * IB;
  const int skew = (int)(reinterpret_cast<uintptr_t>(g) & 15);
  const int64_t head = skew ? 16 - skew : 0;  // bytes before the first 16-byte boundary
  const int64_t body = head >= span ? 0 : (span - head) >> 4;
  for (int64_t j = threadIdx.x; j < (head < span ? head : span); j += kRszThreads) stage[skew + j] = g[j];
  const uint4* gv = reinterpret_cast<const uint4*>(g + head);
  uint4* sv = reinterpret_cast<uint4*>(stage + skew + head);  // skew + head is 0 or 16: 16-byte aligned
  for (int64_t v = threadIdx.x; v < body; v += kRszThreads) sv[v] = gv[v];
  for (int64_t j = head + (body << 4) + threadIdx.x; j < span; j += kRszThreads) stage[skew + j] = g[j];
  __syncthreads();

  // ---- four output pixels per lane and step
  const uint8_t* src = stage + skew;
  uint8_t* o = out + r0 * OB;
  const int64_t npix = (int64_t)nr * OW;
  const bool dwords = (reinterpret_cast<uintptr_t>(o) & 3) == 0;
  for (int64_t p0 = 4 * (int64_t)threadIdx.x; p0 < npix; p0 += 4 * kRszThreads) {
    int row = (int)(p0 / OW), ox = (int)(p0 - (int64_t)row * OW);
    uint32_t px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int r = 0, gg = 0, b = 0;
      if (p0 + q < npix) {
        int lo, n;
        rsz_span(bounds, ox, W, ksize, &lo, &n);
        rsz_pixel_taps(src + row * IB + (int64_t)lo * 3, 3, kk + (int64_t)ox * ksize, n, &r, &gg, &b);
      }
      px[q] = (uint32_t)r | ((uint32_t)gg << 8) | ((uint32_t)b << 16);
      if (++ox == OW) {
        ox = 0;
        ++row;
      }
    }
    uint8_t* dst = o + p0 * 3;
    if (dwords && p0 + 4 <= npix) {
      uint32_t* d = reinterpret_cast<uint32_t*>(dst);
      d[0] = px[0] | (px[1] << 24);
      d[1] = (px[1] >> 8) | (px[2] << 16);
      d[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
      for (int q = 0; q < 4 && p0 + q < npix; ++q) {
        dst[3 * q + 0] = (uint8_t)px[q];
        dst[3 * q + 1] = (uint8_t)(px[q] >> 8);
        dst[3 * q + 2] = (uint8_t)(px[q] >> 16);
      }
    }
  }
}

// one wave per output row (tile n, row oy) of RB bytes: out[n][oy][j] = taps over in[n][lo + i][j]
__global__ void __launch_bounds__(kRszThreads) rsz_v_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t out_rows,
                                                            int H, int OH, int64_t RB, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ kk, int ksize) {
  const int64_t orow = (int64_t)blockIdx.x * (kRszThreads / 64) + (threadIdx.x >> 6);
  if (orow >= out_rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t n = orow / OH;
  const int oy = (int)(orow - n * OH);
  int lo, cnt;
  rsz_span(bounds, oy, H, ksize, &lo, &cnt);
  const int32_t* k = kk + (int64_t)oy * ksize;
  const uint8_t* src = in + (n * H + lo) * RB;
  uint8_t* dst = out + orow * RB;
  for (int64_t j = lane; j < RB; j += 64) dst[j] = (uint8_t)rsz_byte_taps(src + j, RB, k, cnt);
}

size_t resize_workspace_bytes(int N, int H, int W, int OH, int OW) {
  return (OW != W && OH != H) ? (size_t)N * H * OW * 3 : 0;
}

hipError_t launch_resize(const uint8_t* in, int N, int H, int W, int OH, int OW, const int32_t* bounds_x, const int32_t* kk_x,
                         int ksize_x, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y, uint8_t* out, void* workspace,
                         hipStream_t s) {
  if (OW == W && OH == H) return hipMemcpyAsync(out, in, (size_t)N * H * W * 3, hipMemcpyDeviceToDevice, s);
  const uint8_t* src = in;
  if (OW != W) {
    uint8_t* dst = OH != H ? reinterpret_cast<uint8_t*>(workspace) : out;
    const int rpb = rsz_rows_per_block(W);
    const int64_t rows = (int64_t)N * H;
    const unsigned blocks = (unsigned)((rows + rpb - 1) / rpb);
    const size_t lds = (size_t)rpb * W * 3 + 32;
    hipLaunchKernelGGL(rsz_h_kernel, dim3(blocks), dim3(kRszThreads), lds, s, in, dst, rows, W, OW, rpb, bounds_x, kk_x, ksize_x);
    src = dst;
  }
  if (OH != H) {
    const int64_t RB = (int64_t)OW * 3, out_rows = (int64_t)N * OH;
    const unsigned blocks = (unsigned)((out_rows + kRszThreads / 64 - 1) / (kRszThreads / 64));
    hipLaunchKernelGGL(rsz_v_kernel, dim3(blocks), dim3(kRszThreads), 0, s, src, out, out_rows, H, OH, RB, bounds_y, kk_y, ksize_y);
  }
  return hipGetLastError();
}

}  // namespace rfx
