// Host emulator of the forward path's backward (csrc/rfx_mel_bwd_core.h; include/rfx.h: rfx_mel_from_waveform_backward and
// rfx_stft_backward), in double.  TEST INFRASTRUCTURE ONLY (built by tests/test_mel_backward_cpu.py with g++, and with
// tests/emu/rfx_mel_bwd_emu_main.cpp as a stand-alone program under the sanitizers).  Steps 1, 2 and 4 are the core's own functions
// - the adjoint table's sum, the zero rule, the frame range and the three taps of the fold - instantiated for double; step 3, which
// the device leaves to the engines' MODE 0 frame launches, is the definition: the real part of the un-normalised inverse DFT of the
// one-sided gradient, every bin with weight 1 (a plain mixed-radix FFT over the prime factors of n_fft).
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_mel_bwd_core.h"

using namespace rfx;
using cd = std::complex<double>;

namespace {
// un-normalised DFT of any length, sign +1: exp(+2 pi i k n / N).  roots[j] = exp(sign 2 pi i j / N0) for the top-level length N0.
void dft_rec(const cd* in, cd* out, int n, int stride, const std::vector<cd>& roots, int N0) {
  if (n == 1) {
    out[0] = in[0];
    return;
  }
  int p = 2;
  while (n % p) ++p;
  const int m = n / p;
  std::vector<cd> sub((size_t)n);
  for (int r = 0; r < p; ++r) dft_rec(in + (size_t)r * stride, sub.data() + (size_t)r * m, m, stride * p, roots, N0);
  const int step = N0 / n;
  for (int k = 0; k < n; ++k) {
    cd s = 0.0;
    for (int r = 0; r < p; ++r) s += roots[(size_t)(((long long)r * k) % n) * step] * sub[(size_t)r * m + k % m];
    out[k] = s;
  }
}
std::vector<cd> make_roots(int N, int sign) {
  std::vector<cd> roots((size_t)N);
  const double pi2 = 6.283185307179586476925286766559;
  for (int j = 0; j < N; ++j) roots[(size_t)j] = cd(std::cos(pi2 * j / N), sign * std::sin(pi2 * j / N));
  return roots;
}

struct Geo {
  int n_fft, win, hop, h, left, n_stft;
  Geo(int n, int w, int s) : n_fft(n), win(w), hop(s), h(n / 2), left((n - w) / 2), n_stft(n / 2 + 1) {}
  int frames(int Lw) const { return 1 + (Lw + 2 * h - n_fft) / hop; }
};

// steps 3 and 4 from the one-sided gradient G [T][n_stft]: wf [T][win] = w f_t inside the window, then the fold
void frames_and_fold(const Geo& g, int Lw, int T, const double* window, const std::vector<cd>& G, double* grad) {
  const std::vector<cd> roots = make_roots(g.n_fft, +1);
  std::vector<double> wf((size_t)T * g.win);
  std::vector<cd> z((size_t)g.n_fft), y((size_t)g.n_fft);
  for (int t = 0; t < T; ++t) {
    for (int k = 0; k < g.n_fft; ++k) z[(size_t)k] = k < g.n_stft ? G[(size_t)t * g.n_stft + k] : cd(0.0);
    dft_rec(z.data(), y.data(), g.n_fft, 1, roots, g.n_fft);
    for (int i = 0; i < g.win; ++i) wf[(size_t)t * g.win + i] = window[i] * y[(size_t)(g.left + i)].real();
  }
  auto gp = [&](int q) {
    int tlo, thi;
    mel_bwd_frame_range(q, g.left, g.win, g.hop, T, tlo, thi);
    double acc = 0.0;
    for (int t = tlo; t <= thi; ++t) acc += wf[(size_t)t * g.win + (q - g.left - g.hop * t)];
    return acc;
  };
  for (int j = 0; j < Lw; ++j) grad[j] = mel_bwd_sample<double>(j, g.h, Lw, gp);
}
}  // namespace

extern "C" {

int emu_mel_bwd_frames(int n_fft, int win, int hop, int Lw) { return Geo(n_fft, win, hop).frames(Lw); }

// steps 1 - 4.  X [n_stft][T] (re, im) the row's STFT, g_mel [M][T], the adjoint table as rfx_debug_mel_adjoint gives it -> grad [Lw]
int emu_mel_from_waveform_backward(int n_fft, int win, int hop, int Lw, int M, const double* window, const double* Xre, const double* Xim,
                                   const int32_t* first, const int32_t* count, const float* wt, int width, const double* g_mel, double* grad) {
  const Geo g(n_fft, win, hop);
  if (Lw <= g.h) return -1;
  const int T = g.frames(Lw);
  std::vector<cd> G((size_t)T * g.n_stft);
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < g.n_stft; ++k) {
      if (first[k] < 0 || first[k] + count[k] > M) return -2;
      const double gs = mel_adjoint_bin<double>(first[k], count[k], wt + (size_t)k * width, [&](int m) { return g_mel[(size_t)m * T + t]; });
      const double re = Xre[(size_t)k * T + t], im = Xim[(size_t)k * T + t];
      const double s = mel_bwd_unit_scale(gs, re, im);
      G[(size_t)t * g.n_stft + k] = cd(s * re, s * im);
    }
  frames_and_fold(g, Lw, T, window, G, grad);
  return T;
}

// steps 3 and 4: G [n_stft][T] (re, im) is the incoming complex gradient itself
int emu_stft_backward(int n_fft, int win, int hop, int Lw, const double* window, const double* Gre, const double* Gim, double* grad) {
  const Geo g(n_fft, win, hop);
  if (Lw <= g.h) return -1;
  const int T = g.frames(Lw);
  std::vector<cd> G((size_t)T * g.n_stft);
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < g.n_stft; ++k) G[(size_t)t * g.n_stft + k] = cd(Gre[(size_t)k * T + t], Gim[(size_t)k * T + t]);
  frames_and_fold(g, Lw, T, window, G, grad);
  return T;
}

// the table's sum for one frame: out[k] = sum_i wt[k][i] g[first[k] + i], in double
void emu_mel_adjoint_apply(int F, const int32_t* first, const int32_t* count, const float* wt, int width, const double* g, double* out) {
  for (int k = 0; k < F; ++k) out[k] = mel_adjoint_bin<double>(first[k], count[k], wt + (size_t)k * width, [&](int m) { return g[m]; });
}

// A check that needs nothing but this file: the STFT of the definition (reflect padding, window, forward DFT) of a seeded row x, a
// seeded complex gradient G, and the adjoint identity Re <STFT x, G> == <x, emu_stft_backward G>.  Returns the relative defect
// |lhs - rhs| / sqrt(sum |X|^2 sum |G|^2); figures[0] = lhs, figures[1] = rhs.
double emu_stft_adjoint_defect(int n_fft, int win, int hop, int Lw, unsigned seed, double* figures) {
  const Geo g(n_fft, win, hop);
  const int T = g.frames(Lw);
  unsigned s = seed * 2654435761u + 12345u;
  auto rnd = [&s] {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 16777216.0 - 0.5;
  };
  std::vector<double> x((size_t)Lw), window((size_t)win), Gre((size_t)g.n_stft * T), Gim((size_t)g.n_stft * T), grad((size_t)Lw);
  for (auto& v : x) v = rnd();
  for (int i = 0; i < win; ++i) window[(size_t)i] = 0.5 - 0.5 * std::cos(6.283185307179586476925286766559 * i / win);
  for (auto& v : Gre) v = rnd();
  for (auto& v : Gim) v = rnd();
  const std::vector<cd> roots = make_roots(n_fft, -1);
  std::vector<cd> u((size_t)n_fft), y((size_t)n_fft);
  double lhs = 0.0, nx = 0.0, ng = 0.0;
  for (int t = 0; t < T; ++t) {
    for (int i = 0; i < n_fft; ++i) {
      const int j = i - g.left;
      u[(size_t)i] = j >= 0 && j < win ? window[(size_t)j] * x[(size_t)reflect_index(hop * t + i - g.h, Lw)] : 0.0;
    }
    dft_rec(u.data(), y.data(), n_fft, 1, roots, n_fft);
    for (int k = 0; k < g.n_stft; ++k) {
      const double gr = Gre[(size_t)k * T + t], gi = Gim[(size_t)k * T + t];
      lhs += y[(size_t)k].real() * gr + y[(size_t)k].imag() * gi;
      nx += std::norm(y[(size_t)k]);
      ng += gr * gr + gi * gi;
    }
  }
  emu_stft_backward(n_fft, win, hop, Lw, window.data(), Gre.data(), Gim.data(), grad.data());
  double rhs = 0.0;
  for (int j = 0; j < Lw; ++j) rhs += x[(size_t)j] * grad[(size_t)j];
  if (figures) {
    figures[0] = lhs;
    figures[1] = rhs;
  }
  return std::fabs(lhs - rhs) / std::sqrt(nx * ng);
}

}  // extern "C"
