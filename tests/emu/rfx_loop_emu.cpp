// Host emulator of a loop call's index rules, folds and envelope (csrc/rfx_gl.hip: gl_frame_loop_kernel, gl_loop_fold_kernel,
// loop_renv_kernel; csrc/rfx_generic.hip: gen_gl_loop_kernel, gen_loop_fold_kernel; csrc/rfx_fam.hip: fam_gl_loop_kernel).  TEST
// INFRASTRUCTURE ONLY (built by tests/test_loop_decode_cpu.py with g++): it runs the functions of rfx_loop_core.h that the kernels
// inline, the way the launches walk them: one logical thread per window sample of a frame (gather), per sample of the period
// (folds), per entry of the table (envelope).  What the kernels have of their own is the grid and the transforms between the two.
#include <cstddef>
#include <cstdint>
#include "../../riffusion-hobby_amd/csrc/rfx_loop_core.h"

using namespace rfx;

extern "C" {

int emu_loop_valid(int hop, int T, int n_fft) { return loop_valid(hop, T, n_fft) ? 1 : 0; }
int emu_loop_min_frames(int hop, int n_fft) { return loop_min_frames(hop, n_fft); }
int emu_loop_wrap(int p, int P) { return loop_wrap(p, P); }

// the sample every window position j of frame t reads, as the generic kernel and the row family index it: element i = left + j of
// the padded frame at hop t + i - n_fft / 2 of the period
void emu_loop_gather(int n_fft, int win, int hop, int T, int t, int32_t* idx) {
  const int half = n_fft / 2, left = (n_fft - win) / 2, P = hop * T;
  for (int j = 0; j < win; ++j) idx[j] = loop_wrap(hop * t + (left + j) - half, P);
}
// ... as the specialised kernel indexes it: thread n' reads hop blocks fr - 5 .. fr + 4 (win == 10 hop, n_fft / 2 - left == 5 hop)
void emu_loop_gather_blocks(int hop, int T, int fr, int32_t* idx) {
  const int P = hop * T;
  for (int npr = 0; npr < hop; ++npr)
    for (int j = 0; j < 10; ++j) idx[j * hop + npr] = loop_wrap((fr + j - 5) * hop + npr, P);
}

// env[r], r < hop
void emu_loop_env(const float* win, int n_fft, int win_len, int hop, float* env) {
  for (int r = 0; r < hop; ++r) env[r] = loop_env(win, r, n_fft / 2, (n_fft - win_len) / 2, win_len, hop);
}
// the table the folds multiply by: scale / env[r]
void emu_loop_renv(const float* win, int n_fft, int win_len, int hop, float scale, float* renv) {
  for (int r = 0; r < hop; ++r) renv[r] = scale / loop_env(win, r, n_fft / 2, (n_fft - win_len) / 2, win_len, hop);
}

// the fold of windowed frames [T][pitch] (window sample j at shift + j) into out[0 .. hop T)
void emu_loop_fold_sum(const float* frames, int pitch, int shift, const float* renv, int n_fft, int win_len, int hop, int T, float* out) {
  const int P = hop * T, off = n_fft / 2 - (n_fft - win_len) / 2;
  for (int m = 0; m < P; ++m) out[m] = loop_fold_sum(frames, (size_t)pitch, shift, m + off, win_len, hop, T) * renv[m % hop];
}
// the fold of un-windowed frames [T][pitch] with the window
void emu_loop_fold_fma(const float* frames, int pitch, const float* win, const float* renv, int n_fft, int win_len, int hop, int T, float* out) {
  const int P = hop * T, off = n_fft / 2 - (n_fft - win_len) / 2;
  for (int m = 0; m < P; ++m) out[m] = loop_fold_fma(frames, (size_t)pitch, win, m + off, win_len, hop, T) * renv[m % hop];
}

}  // extern "C"
