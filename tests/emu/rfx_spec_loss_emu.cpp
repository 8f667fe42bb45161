// Host emulator of the fused spectral losses (csrc/rfx_spec_loss_core.h; include/rfx.h: rfx_spectral_loss, rfx_spectral_loss_backward and
// their loop forms), in double.  TEST INFRASTRUCTURE ONLY (built by tests/test_spectral_loss_cpu.py with g++, and with
// tests/emu/rfx_spec_loss_emu_main.cpp as a stand-alone program under the sanitizers).  It takes the DFT and the plain fold from
// tests/emu/rfx_mel_bwd_emu.cpp, included as it stands, and adds what the loss entries add: the core's slot rule instantiated for
// double, the circular adjoint fold on the core's index rules (loop_fold_range, loop_frame), the core's own float32 chains
// (spec_loss_loop_sample) and the three sums on the logical threads of the two reduction kernels.
#include "rfx_mel_bwd_emu.cpp"

#include "../../riffusion-hobby_amd/csrc/rfx_spec_loss_core.h"

namespace {
// step 3: wf [T][win] = w f_t inside the window, from the one-sided gradient G [T][n_stft]
std::vector<double> windowed_frames(const Geo& g, int T, const double* window, const std::vector<cd>& G) {
  const std::vector<cd> roots = make_roots(g.n_fft, +1);
  std::vector<double> wf((size_t)T * g.win);
  std::vector<cd> z((size_t)g.n_fft), y((size_t)g.n_fft);
  for (int t = 0; t < T; ++t) {
    for (int k = 0; k < g.n_fft; ++k) z[(size_t)k] = k < g.n_stft ? G[(size_t)t * g.n_stft + k] : cd(0.0);
    dft_rec(z.data(), y.data(), g.n_fft, 1, roots, g.n_fft);
    for (int i = 0; i < g.win; ++i) wf[(size_t)t * g.win + i] = window[i] * y[(size_t)(g.left + i)].real();
  }
  return wf;
}
// the circular adjoint fold of windowed frames wf [T][win] -> out [hop T]: the chain of rfx_loop_core.h, oldest covering frame first
void circular_fold(const Geo& g, int T, const double* wf, double* out) {
  const int P = g.hop * T;
  for (int m = 0; m < P; ++m) {
    const int q = m + g.h - g.left;
    int tlo, thi;
    loop_fold_range(q, g.win, g.hop, tlo, thi);
    double acc = 0.0;
    for (int t = tlo; t <= thi; ++t) acc += wf[(size_t)loop_frame(t, T) * g.win + (q - g.hop * t)];
    out[m] = acc;
  }
}
}  // namespace

extern "C" {

// frames of a row of Lw samples: the plain count, or for a loop row Lw / hop (0: no legal loop length)
int emu_spec_loss_frames(int n_fft, int win, int hop, int Lw, int loop) {
  return loop ? loop_samples_frames(hop, n_fft, Lw) : Geo(n_fft, win, hop).frames(Lw);
}

// X [n_stft][T] (re, im) the row's STFT, target [n_stft][T], the row's coefficients and the floor -> grad [Lw]
int emu_spec_loss_backward(int n_fft, int win, int hop, int Lw, int loop, const double* window, const double* Xre, const double* Xim,
                           const double* target, double c_sc, double c_lg, double floor, double* grad) {
  const Geo g(n_fft, win, hop);
  const int T = emu_spec_loss_frames(n_fft, win, hop, Lw, loop);
  if (T <= 0 || (!loop && Lw <= g.h)) return -1;
  std::vector<cd> G((size_t)T * g.n_stft);
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < g.n_stft; ++k) {
      const double re = Xre[(size_t)k * T + t], im = Xim[(size_t)k * T + t];
      const double s = spec_loss_unit_scale<double>(spec_loss_abs(re, im), target[(size_t)k * T + t], c_sc, c_lg, floor);
      G[(size_t)t * g.n_stft + k] = cd(s * re, s * im);
    }
  if (!loop) {
    frames_and_fold(g, Lw, T, window, G, grad);
    return T;
  }
  const std::vector<double> wf = windowed_frames(g, T, window, G);
  circular_fold(g, T, wf.data(), grad);
  return T;
}

// the circular adjoint fold alone: wf [T][win] windowed frames -> out [hop T]
void emu_loop_fold(int n_fft, int win, int hop, int T, const double* wf, double* out) { circular_fold(Geo(n_fft, win, hop), T, wf, out); }

// the core's float32 chains over frames [T][pitch] (window sample j at shift + j): `window` non-null = un-windowed frames, the fma chain
void emu_loop_fold_f32(int n_fft, int win, int hop, int T, int pitch, int shift, const float* frames, const float* window, float* out) {
  const Geo g(n_fft, win, hop);
  for (int m = 0; m < hop * T; ++m) out[m] = spec_loss_loop_sample(frames, (size_t)pitch, shift, window, m, g.h, g.left, win, hop, T);
}

// the adjoint identity of the circular fold, needing nothing but this file: A x = the windowed circular framing of a seeded period x
// (frame t, window sample j reads x[(hop t + left + j - h) mod P]), y seeded frames; |<A x, y> - <x, A^T y>| / sqrt(|A x|^2 |y|^2)
double emu_loop_adjoint_defect(int n_fft, int win, int hop, int T, unsigned seed) {
  const Geo g(n_fft, win, hop);
  const int P = hop * T;
  unsigned s = seed * 2654435761u + 12345u;
  auto rnd = [&s] {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 16777216.0 - 0.5;
  };
  std::vector<double> x((size_t)P), window((size_t)win), y((size_t)T * win), wy((size_t)T * win), back((size_t)P);
  for (auto& v : x) v = rnd();
  for (int i = 0; i < win; ++i) window[(size_t)i] = 0.5 - 0.5 * std::cos(6.283185307179586476925286766559 * i / win);
  for (auto& v : y) v = rnd();
  double lhs = 0.0, na = 0.0, ny = 0.0;
  for (int t = 0; t < T; ++t)
    for (int j = 0; j < win; ++j) {
      const double ax = window[(size_t)j] * x[(size_t)loop_read_index(hop * t + g.left + j - g.h, P)];
      const double yy = y[(size_t)t * win + j];
      lhs += ax * yy;
      na += ax * ax;
      ny += yy * yy;
      wy[(size_t)t * win + j] = window[(size_t)j] * yy;
    }
  circular_fold(g, T, wy.data(), back.data());
  double rhs = 0.0;
  for (int m = 0; m < P; ++m) rhs += x[(size_t)m] * back[(size_t)m];
  return std::fabs(lhs - rhs) / std::sqrt(na * ny);
}

// the three sums of one row of T plain (bin-ordered) frames of fs floats, on the logical threads of the two kernels
void emu_spec_loss_sums(const float* a, const float* m, int T, int fs, int n_stft, float floor, double* out3) {
  const int chunks = qual_chunks(T);
  std::vector<SpecLossSums> partials((size_t)chunks), s((size_t)kQualThreads);
  auto tree = [&] {
    for (int stride = kQualThreads / 2; stride > 0; stride >>= 1)
      for (int tid = 0; tid < stride; ++tid) spec_loss_tree_step(s.data(), tid, stride);
  };
  for (int chunk = 0; chunk < chunks; ++chunk) {
    const int f0 = chunk * kQualFrames, f1 = f0 + kQualFrames < T ? f0 + kQualFrames : T;
    for (int tid = 0; tid < kQualThreads; ++tid)
      s[(size_t)tid] = floor > 0.f ? spec_loss_thread_partial<true, true>(a, m, f0, f1, fs, n_stft, floor, tid)
                                   : spec_loss_thread_partial<true, false>(a, m, f0, f1, fs, n_stft, floor, tid);
    tree();
    partials[(size_t)chunk] = s[0];
  }
  for (int tid = 0; tid < kQualThreads; ++tid) s[(size_t)tid] = spec_loss_combine_partial(partials.data(), chunks, tid);
  tree();
  out3[0] = s[0].num;
  out3[1] = s[0].den;
  out3[2] = s[0].lsum;
}

int emu_spec_loss_floor_ok(float f) { return spec_loss_floor_ok(f) ? 1 : 0; }

}  // extern "C"
