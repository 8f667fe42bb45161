// Host emulator of the resize kernels (csrc/rfx_resize.hip).  TEST INFRASTRUCTURE ONLY (built by tests/test_resize_cpu.py with
// g++): the coefficient planner of rfx_resize_core.h and the per-byte arithmetic the kernels inline, in the kernels' pass
// order (horizontal into a uint8 intermediate, then vertical), so that they are pinned against PIL.Image.resize on the CPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_resize_core.h"

using namespace rfx;

namespace {

struct Axis {
  int ksize = 0;
  std::vector<int32_t> bounds, kk;
};

Axis plan(int in_size, int out_size, int filter) {
  Axis a;
  a.ksize = rsz_ksize(in_size, out_size, filter);
  a.bounds.resize(2 * (size_t)out_size);
  a.kk.resize((size_t)out_size * a.ksize);
  std::vector<double> w(a.ksize);
  rsz_coefficients(in_size, out_size, filter, a.bounds.data(), a.kk.data(), w.data());
  return a;
}

}  // namespace

extern "C" {

int emu_resize_ksize(int in_size, int out_size, int filter) { return rsz_ksize(in_size, out_size, filter); }

// the tables rfx_image_resize_coefficients returns
int emu_resize_coefficients(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk) {
  std::vector<double> w(rsz_ksize(in_size, out_size, filter));
  return rsz_coefficients(in_size, out_size, filter, bounds, kk, w.data());
}

// (N, H, W, 3) uint8 -> (N, OH, OW, 3) uint8
int emu_resize_u8(const uint8_t* in, int N, int H, int W, int OH, int OW, int filter, uint8_t* out) {
  if (rsz_support(filter) == 0.0) return -1;
  std::vector<uint8_t> mid;
  const uint8_t* src = in;
  int cw = W;
  if (OW != W) {
    const Axis ax = plan(W, OW, filter);
    mid.resize((size_t)N * H * OW * 3);
    for (int64_t row = 0; row < (int64_t)N * H; ++row)
      for (int ox = 0; ox < OW; ++ox) {
        int lo, n, r, g, b;
        rsz_span(ax.bounds.data(), ox, W, ax.ksize, &lo, &n);
        rsz_pixel_taps(in + (row * W + lo) * 3, 3, ax.kk.data() + (int64_t)ox * ax.ksize, n, &r, &g, &b);
        uint8_t* o = mid.data() + (row * OW + ox) * 3;
        o[0] = (uint8_t)r;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)b;
      }
    src = mid.data();
    cw = OW;
  }
  const int64_t rb = (int64_t)cw * 3;
  if (OH != H) {
    const Axis ay = plan(H, OH, filter);
    for (int n = 0; n < N; ++n)
      for (int oy = 0; oy < OH; ++oy) {
        int lo, cnt;
        rsz_span(ay.bounds.data(), oy, H, ay.ksize, &lo, &cnt);
        const int32_t* k = ay.kk.data() + (int64_t)oy * ay.ksize;
        for (int64_t j = 0; j < rb; ++j)
          out[((int64_t)n * OH + oy) * rb + j] = (uint8_t)rsz_byte_taps(src + ((int64_t)n * H + lo) * rb + j, rb, k, cnt);
      }
  } else {
    memcpy(out, src, (size_t)N * H * rb);
  }
  return 0;
}

}  // extern "C"
