// Stand-alone driver of tests/emu/rfx_imel_lstsq_bwd_emu.cpp for a sanitizer run (tests/test_imel_lstsq_bwd_cpu.py builds the two files
// with -fsanitize=address,undefined and runs the program).  A handmade triangular bank of 7 filters over 40 bins (two bins at either
// end without a filter), its L D L^T factors and collect lists built here as rfx_plan_core.h builds them, heap buffers of exactly the
// documented sizes, B = 2 rows of T = 19 frames (more than kLsqBatch filters is not needed: 7 < 16 walks the short-batch path, and
// a second bank of 37 filters over 200 bins walks three batches).  Checks: an all-open mask gives G^-1 fb^T gx (double) to float32
// rounding; a gradient that lives only where the forward is 0 gives all-zero bits.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_imel_lstsq_core.h"

extern "C" {
void emu_inverse_mel_lstsq_backward(const float* fb, const float* nl, const float* inv_d, const int* ptr, const int* bin, const int* pos,
                                    const float* w, const float* mel, const float* gx, int B, int F, int M, int T, int stride, float* c_out,
                                    float* g_mel);
}

static int failures = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      ++failures;                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                       \
  } while (0)

static void run_bank(int F, int M, int lo, int hi) {
  using namespace rfx;
  const int B = 2, T = 19, stride = (F + 3) / 4 * 4;
  // triangles with centres evenly spaced over [lo, hi): every bin between two centres feeds both filters
  std::vector<float> fb((size_t)F * M, 0.f);
  std::vector<double> centre((size_t)M + 2);
  for (int m = 0; m < M + 2; ++m) centre[(size_t)m] = lo + (double)(hi - lo) * m / (M + 1);
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < M; ++m) {
      const double up = (f - centre[(size_t)m]) / (centre[(size_t)m + 1] - centre[(size_t)m]);
      const double down = (centre[(size_t)m + 2] - f) / (centre[(size_t)m + 2] - centre[(size_t)m + 1]);
      const double v = std::fmin(up, down);
      if (v > 0.0) fb[(size_t)f * M + m] = (float)v;
    }
  // G = fb^T fb = L D L^T in double, the two float32 tables
  std::vector<double> d((size_t)M, 0.0), e((size_t)M, 0.0), Dd((size_t)M), ld((size_t)M, 0.0);
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < M; ++m) {
      d[(size_t)m] += (double)fb[(size_t)f * M + m] * fb[(size_t)f * M + m];
      if (m + 1 < M) e[(size_t)m] += (double)fb[(size_t)f * M + m] * fb[(size_t)f * M + m + 1];
    }
  std::vector<float> nl((size_t)M, 0.f), inv_d((size_t)M);
  double D = d[0];
  for (int m = 0; m < M; ++m) {
    CHECK(D > 0.0);
    Dd[(size_t)m] = D;
    inv_d[(size_t)m] = (float)(1.0 / D);
    if (m + 1 < M) {
      ld[(size_t)m] = e[(size_t)m] / D;
      nl[(size_t)m] = (float)(-ld[(size_t)m]);
      D = d[(size_t)m + 1] - ld[(size_t)m] * e[(size_t)m];
    }
  }
  // the lists: per filter its bins ascending, position = bin
  std::vector<int> ptr((size_t)M + 1, 0), bin, pos;
  std::vector<float> w;
  for (int m = 0; m < M; ++m) {
    ptr[(size_t)m] = (int)w.size();
    for (int f = 0; f < F; ++f)
      if (fb[(size_t)f * M + m] != 0.f) {
        bin.push_back(f);
        pos.push_back(f);
        w.push_back(fb[(size_t)f * M + m]);
      }
  }
  ptr[(size_t)M] = (int)w.size();
  // mel = fb^T lin with lin > 0: every bin with a filter is open
  std::vector<float> mel((size_t)B * M * T), gx((size_t)B * T * stride), c((size_t)B * M * T), g((size_t)B * M * T, 123.f);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t) {
      for (int m = 0; m < M; ++m) {
        double acc = 0.0;
        for (int f = 0; f < F; ++f) acc += (double)fb[(size_t)f * M + m] * (1.0 + 0.5 * std::sin(0.3 * f + t + 7 * b));
        mel[((size_t)b * M + m) * T + t] = (float)acc;
      }
      for (int p = 0; p < stride; ++p) gx[((size_t)b * T + t) * stride + p] = (float)std::cos(0.7 * p + 1.3 * t + b);
    }
  emu_inverse_mel_lstsq_backward(fb.data(), nl.data(), inv_d.data(), ptr.data(), bin.data(), pos.data(), w.data(), mel.data(), gx.data(), B, F, M,
                                 T, stride, c.data(), g.data());
  double worst = 0.0, scale = 0.0;
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t) {
      std::vector<double> r((size_t)M, 0.0);
      for (int m = 0; m < M; ++m)
        for (int f = 0; f < F; ++f) r[(size_t)m] += (double)fb[(size_t)f * M + m] * gx[((size_t)b * T + t) * stride + f];
      for (int m = 1; m < M; ++m) r[(size_t)m] -= ld[(size_t)m - 1] * r[(size_t)m - 1];
      for (int m = M - 1; m >= 0; --m) r[(size_t)m] = r[(size_t)m] / Dd[(size_t)m] - (m + 1 < M ? ld[(size_t)m] * r[(size_t)m + 1] : 0.0);
      for (int m = 0; m < M; ++m) {
        worst = std::fmax(worst, std::fabs(r[(size_t)m] - g[((size_t)b * M + m) * T + t]));
        scale = std::fmax(scale, std::fabs(r[(size_t)m]));
      }
    }
  std::printf("bank %d x %d: worst |g_mel - double| %.3g of %.3g\n", F, M, worst, scale);
  CHECK(worst <= 1e-4 * scale);
  // a gradient only where no filter reaches, NaN included: every sum is +0.0
  for (size_t i = 0; i < gx.size(); ++i) gx[i] = 0.f;
  for (int bt = 0; bt < B * T; ++bt)
    for (int p = 0; p < stride; ++p) {
      bool reached = false;
      for (int m = 0; m < M && p < F; ++m) reached = reached || fb[(size_t)p * M + m] != 0.f;
      if (!reached) gx[(size_t)bt * stride + p] = p & 1 ? NAN : 5.f;
    }
  emu_inverse_mel_lstsq_backward(fb.data(), nl.data(), inv_d.data(), ptr.data(), bin.data(), pos.data(), w.data(), mel.data(), gx.data(), B, F, M,
                                 T, stride, nullptr, g.data());
  const std::vector<float> zeros(g.size(), 0.f);
  CHECK(std::memcmp(g.data(), zeros.data(), g.size() * sizeof(float)) == 0);
  // mel = -(fb^T lin): every bin closed, whatever the gradient
  for (float& v : mel) v = -v;
  for (size_t i = 0; i < gx.size(); ++i) gx[i] = (float)(i % 17) - 8.f;
  emu_inverse_mel_lstsq_backward(fb.data(), nl.data(), inv_d.data(), ptr.data(), bin.data(), pos.data(), w.data(), mel.data(), gx.data(), B, F, M,
                                 T, stride, nullptr, g.data());
  CHECK(std::memcmp(g.data(), zeros.data(), g.size() * sizeof(float)) == 0);
}

int main() {
  run_bank(40, 7, 2, 38);
  run_bank(200, 37, 5, 190);
  CHECK(rfx::lsq_collect_masked(1.f, 0.f, 0.f, 0.f, 3.f) == 0.f && rfx::lsq_collect_masked(1.f, 0.f, 1e-30f, 0.f, 3.f) == 3.f);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
