// Stand-alone driver of tests/emu/rfx_resample_emu.cpp for a sanitizer run (tests/test_resample_cpu.py builds the two files with
// -fsanitize=address,undefined and runs the program).  For pairs that go up and down, with few and many phases, and rows shorter
// than the filter, it builds the table into heap buffers of exactly n and n * ntaps entries and resamples heap rows of exactly L
// samples into rows of exactly K - so a read outside a row or the table, or a write past the last output, is an error of the
// program - and checks what needs no oracle: the output length, the zero row, a row alone against the row in the batch, a scaled
// input, an input delayed by o samples against the output delayed by n, a row cut short by `valid` against the row padded with
// zeros, and that the weights of a phase sum to about one.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
long long emu_rs_frames(long long L, int orig, int neu);
int emu_rs_table(int orig, int neu, int lpw, double rolloff, int32_t* first, float* taps, int32_t* n_out, int32_t* ntaps_out);
void emu_resample(const float* in, int rows, long long in_stride, long long valid, int o, int n, const int32_t* first, const float* taps,
                  int ntaps, float* out, long long out_stride, long long K);
}

static int failures = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      ++failures;                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                       \
  } while (0)

static float noise(unsigned& s) {  // a fixed sequence in [-1, 1)
  s = s * 1664525u + 1013904223u;
  return (float)((double)(s >> 8) / 8388608.0 - 1.0);
}

int main() {
  const int pairs[6][2] = {{2, 1}, {1, 2}, {55, 49}, {147, 160}, {7787, 7350}, {96000, 88200}};  // the last reduces to 160 / 147
  const int lengths[4] = {1, 5, 100, 777};
  for (const auto& pr : pairs) {
    int32_t n = 0, ntaps = 0;
    CHECK(emu_rs_table(pr[0], pr[1], 6, 0.99, nullptr, nullptr, &n, &ntaps) == 0 && n >= 1 && ntaps >= 12 && ntaps <= 26);
    std::vector<int32_t> first((size_t)n);
    std::vector<float> taps((size_t)n * ntaps);
    CHECK(emu_rs_table(pr[0], pr[1], 6, 0.99, first.data(), taps.data(), &n, &ntaps) == 0);
    // the reduced pair from the pair itself
    int a = pr[0], b = pr[1];
    while (b) {
      const int t = a % b;
      a = b;
      b = t;
    }
    const int ro = pr[0] / a;
    CHECK(n == pr[1] / a);
    for (int p = 0; p < n; p += (n > 64 ? n / 64 : 1)) {
      double sum = 0;
      for (int k = 0; k < ntaps; ++k) sum += taps[(size_t)k * n + p];
      CHECK(std::fabs(sum - 1.0) < 0.02);  // unit gain at 0 Hz
    }
    for (const int L : lengths) {
      const long long K = emu_rs_frames(L, pr[0], pr[1]);
      CHECK(K == ((long long)n * L + ro - 1) / ro && K >= 1);
      const int B = 3;
      unsigned seed = 5u + (unsigned)L;
      std::vector<float> X((size_t)B * L), Y((size_t)B * K, 123.f), Y1((size_t)K, 123.f);
      for (float& v : X) v = noise(seed);
      std::memset(X.data() + (size_t)(B - 1) * L, 0, (size_t)L * sizeof(float));  // the last row is silent
      emu_resample(X.data(), B, L, L, ro, n, first.data(), taps.data(), ntaps, Y.data(), K, K);
      for (size_t i = (size_t)(B - 1) * K; i < Y.size(); ++i) CHECK(Y[i] == 0.f);
      for (const float v : Y) CHECK(std::isfinite(v));
      emu_resample(X.data() + L, 1, L, L, ro, n, first.data(), taps.data(), ntaps, Y1.data(), K, K);  // row 1 alone
      CHECK(std::memcmp(Y1.data(), Y.data() + K, (size_t)K * sizeof(float)) == 0);
      // a scaled input: every product and sum scales exactly
      std::vector<float> Xs((size_t)L), Ys((size_t)K);
      for (int i = 0; i < L; ++i) Xs[i] = std::ldexp(X[(size_t)L + i], 40);
      emu_resample(Xs.data(), 1, L, L, ro, n, first.data(), taps.data(), ntaps, Ys.data(), K, K);
      for (long long j = 0; j < K; ++j) CHECK(Ys[j] == std::ldexp(Y1[j], 40));
      // delayed by o samples in a row of L + o: the output is delayed by n
      std::vector<float> Xd((size_t)L + ro, 0.f);
      std::memcpy(Xd.data() + ro, X.data() + L, (size_t)L * sizeof(float));
      const long long Kd = emu_rs_frames(L + ro, pr[0], pr[1]);
      CHECK(Kd == K + n);
      std::vector<float> Yd((size_t)Kd);
      emu_resample(Xd.data(), 1, L + ro, L + ro, ro, n, first.data(), taps.data(), ntaps, Yd.data(), Kd, Kd);
      CHECK(std::memcmp(Yd.data() + n, Y1.data(), (size_t)K * sizeof(float)) == 0);  // (zeros before the row either way: the whole row agrees)
      // `valid` below the row's length reads zeros there: the bits of a row padded with zeros
      if (L > 2) {
        const int cut = L / 2;
        std::vector<float> Xz(X.begin() + L, X.begin() + 2 * L), Yv((size_t)K), Yz((size_t)K);
        emu_resample(Xz.data(), 1, L, cut, ro, n, first.data(), taps.data(), ntaps, Yv.data(), K, K);
        for (int i = cut; i < L; ++i) Xz[i] = 0.f;
        emu_resample(Xz.data(), 1, L, L, ro, n, first.data(), taps.data(), ntaps, Yz.data(), K, K);
        CHECK(std::memcmp(Yv.data(), Yz.data(), (size_t)K * sizeof(float)) == 0);
      }
    }
  }
  CHECK(emu_rs_frames(2147483647LL, 1, 2) == -1 && emu_rs_frames(0, 2, 1) == -1 && emu_rs_frames(5, 0, 1) == -1);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
