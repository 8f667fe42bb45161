// rfx_istft_emu.cpp - host emulator of the inverse spectrogram's own arithmetic (csrc/rfx_istft_core.h), in double, for
// tests/test_istft_cpu.py.  The backward runs the way the device's test route does: the staging rule, the circular analysis of the
// staged row (loop_read_index) over the padded period - position by position what zero_outside gives - the slot rule per bin.  The forward is the definition's synthesis, for the adjoint
// identity.  The transforms are plain sums: small geometries only.
#include <math.h>

#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_istft_core.h"
#include "../../riffusion-hobby_amd/csrc/rfx_loop_core.h"

using namespace rfx;

namespace {
const double kPi = 3.14159265358979323846;

struct Geo {
  int n_fft, win, hop, T, loop, h, left, n_stft, L;
  std::vector<double> w;  // zero-padded to n_fft
};
Geo geo(int n_fft, int win, int hop, int T, int loop, const double* window) {
  Geo g{n_fft, win, hop, T, loop, n_fft / 2, (n_fft - win) / 2, n_fft / 2 + 1, loop ? hop * T : hop * (T - 1) + (n_fft & 1), {}};
  g.w.assign((size_t)n_fft, 0.0);
  for (int j = 0; j < win; ++j) g.w[(size_t)g.left + j] = window[j];
  return g;
}
// the envelope at output sample q: plain sum_t w^2[q + h - hop t] over the T frames, loop the circular one
double env_at(const Geo& g, int q) {
  double e = 0.0;
  if (g.loop) {  // every frame once, its positions modulo the period
    for (int t = 0; t < g.T; ++t)
      for (int i = 0; i < g.n_fft; ++i)
        if (loop_wrap((g.hop * t + i - g.h) % (g.hop * g.T), g.hop * g.T) == q) e += g.w[(size_t)i] * g.w[(size_t)i];
    return e;
  }
  for (int t = 0; t < g.T; ++t) {
    const int i = q + g.h - g.hop * t;
    if (i >= 0 && i < g.n_fft) e += g.w[(size_t)i] * g.w[(size_t)i];
  }
  return e;
}
}  // namespace

extern "C" {

int emu_istft_samples(int n_fft, int hop, int T, int loop) { return loop ? hop * T : hop * (T - 1) + (n_fft & 1); }
int emu_istft_pad_frames(int hop, int n_fft, int L) { return istft_pad_frames(hop, n_fft, L); }

// the zero-outside rule against the circular read of the padded period: the number of (t, i), t < T, where they disagree
long long emu_zero_outside_defects(int n_fft, int hop, int T) {
  const int L = hop * (T - 1) + (n_fft & 1), h = n_fft / 2, P = hop * istft_pad_frames(hop, n_fft, L);
  long long bad = 0;
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < n_fft; ++i) {
      const int p = hop * t + i - h;
      const int z = zero_outside(p, L), c = loop_read_index(p, P);
      if (z >= 0 ? c != z : c < L) ++bad;  // inside: the same sample; outside: the padding
    }
  return bad;
}

// the staging alone: g (L) -> u (pitch), table kinds as the device has them (tab_scaled: the table carries 2 / N and multiplies)
void emu_istft_stage(int n_fft, int win, int hop, int T, int loop, int tab_scaled, const double* window, const double* gr, double* u, int pitch) {
  const Geo g = geo(n_fft, win, hop, T, loop, window);
  const int period = loop ? hop : 0, entries = loop ? hop : g.L;
  std::vector<double> tab((size_t)entries);
  for (int q = 0; q < entries; ++q) {
    const double e = env_at(g, q);
    tab[(size_t)q] = loop ? (tab_scaled ? 2.0 / n_fft : 1.0) / e : tab_scaled ? (2.0 / n_fft) / e : e;
  }
  const bool divide = !loop && !tab_scaled;
  for (int col = 0; col < pitch; ++col) {
    const int entry = istft_stage_entry(col, g.L, period);
    u[col] = entry < 0 ? 0.0 : istft_stage_value(gr[col], tab[(size_t)entry], divide);
  }
}

// backward of one row: g (L) -> G (n_stft, T) as re / im planes
void emu_istft_backward(int n_fft, int win, int hop, int T, int loop, int tab_scaled, const double* window, const double* gr, double* G_re,
                        double* G_im) {
  const Geo g = geo(n_fft, win, hop, T, loop, window);
  const int Tp = loop ? T : istft_pad_frames(hop, n_fft, g.L), P = hop * Tp;
  std::vector<double> u((size_t)P);
  emu_istft_stage(n_fft, win, hop, T, loop, tab_scaled, window, gr, u.data(), P);
  const double unit = tab_scaled ? 0.5 : istft_unit_exact(n_fft);
  std::vector<double> fr((size_t)n_fft);
  for (int t = 0; t < T; ++t) {
    for (int i = 0; i < n_fft; ++i) fr[(size_t)i] = g.w[(size_t)i] * u[(size_t)loop_read_index(hop * t + i - g.h, P)];
    for (int k = 0; k < g.n_stft; ++k) {
      double re = 0.0, im = 0.0;
      for (int i = 0; i < n_fft; ++i) {
        const double a = -2.0 * kPi * (double)(((long long)k * i) % n_fft) / n_fft;
        re += fr[(size_t)i] * cos(a);
        im += fr[(size_t)i] * sin(a);
      }
      istft_grad_slot(k, n_fft, unit, re, im, G_re[(size_t)k * T + t], G_im[(size_t)k * T + t]);
    }
  }
}

// forward of one row by the definition: X (n_stft, T) as re / im planes -> y (L)
void emu_istft_forward(int n_fft, int win, int hop, int T, int loop, const double* window, const double* X_re, const double* X_im, double* y) {
  const Geo g = geo(n_fft, win, hop, T, loop, window);
  const int P = hop * T;
  std::vector<double> acc((size_t)g.L, 0.0);
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < n_fft; ++i) {
      if (g.w[(size_t)i] == 0.0) continue;
      const int p = hop * t + i - g.h;
      const int q = loop ? loop_wrap(p % P, P) : zero_outside(p, g.L);
      if (q < 0) continue;
      double f = 0.0;  // c2r: the imaginary parts of bin 0 and the Nyquist bin do not enter
      for (int k = 0; k < g.n_stft; ++k) {
        const double a = 2.0 * kPi * (double)(((long long)k * i) % n_fft) / n_fft;
        const double c = istft_bin_is_real(k, n_fft) ? 1.0 : 2.0;
        f += c * (X_re[(size_t)k * T + t] * cos(a) - (istft_bin_is_real(k, n_fft) ? 0.0 : X_im[(size_t)k * T + t]) * sin(a));
      }
      acc[(size_t)q] += g.w[(size_t)i] * f / n_fft;
    }
  for (int q = 0; q < g.L; ++q) y[q] = acc[(size_t)q] / env_at(g, q);
}

}  // extern "C"
