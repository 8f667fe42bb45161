// Host emulator of the three kernels of the spectral-peak start (csrc/rfx_peak.hip: peak_owner_kernel, peak_chain_kernel,
// peak_angles_kernel).  TEST INFRASTRUCTURE ONLY (built by tests/test_peak_start_cpu.py with g++): it runs the functions of
// rfx_peak_core.h that the kernels inline - the frame maximum and threshold, the peak test, the owner rule, the interpolated position,
// the phase advance, the angle - the way the launches walk them: a frame in bin order gathered from its slot order, the owners of
// the frame, the chain over a row's frames with the previous frame's state by bin, one logical thread per output position.  What the
// kernels have of their own is the workgroup-wide scan that carries the nearest peak across the threads' chunks.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_holdmask_core.h"
#include "../../riffusion-hobby_amd/csrc/rfx_peak_core.h"

using namespace rfx;

extern "C" {

int emu_peak_spec_stride() { return kFrameStride; }
int emu_peak_max_bins() { return kPeakMaxBins; }
// the bin input position p stands for (-1: padding), in each of the three slot orders magnitudes come in
int emu_peak_in_bin(int layout, int p, int n_stft, const int* bin_of) { return holdmask_slot_bin(layout, p, n_stft, bin_of); }
// the bin output position p stands for and whether the slot holds its conjugate
int emu_peak_out_bin(int spec, int p, int n_stft, int* conj) {
  *conj = 0;
  if (!spec) return p < n_stft ? p : -1;
  int q, kb;
  if (!pos_c_to_slot(p, q, kb)) return -1;
  bool cj;
  const int bin = slot_bin(q / 21, q % 21, kb, &cj);
  *conj = cj ? 1 : 0;
  return bin;
}

// owners of one frame m[F] (0xFFFF everywhere: no peak)
void emu_peak_owners(const float* m, int F, uint16_t* own) { peak_frame_owners(m, F, own); }

// S: [B*T][stride_in] magnitudes in `layout`; angles: [B*T][stride_out] (re, im) float pairs, slot_pos_c order when spec_out else plain
void emu_peak_start(int layout, const float* S, const int* bin_of, int B, int T, int stride_in, int F, int hop, int n_fft, int spec_out,
                    float* angles, int stride_out) {
  std::vector<float> m((size_t)F);
  std::vector<uint16_t> own((size_t)F), own_prev((size_t)F);
  std::vector<double> phi((size_t)F), pos((size_t)F), phi_prev((size_t)F), pos_prev((size_t)F);
  for (size_t row = 0; row < (size_t)B; ++row)
    for (int t = 0; t < T; ++t) {
      const size_t fr = row * (size_t)T + t;
      for (int p = 0; p < stride_in; ++p) {
        const int bin = holdmask_slot_bin(layout, p, F, bin_of);
        if (bin >= 0) m[bin] = S[fr * (size_t)stride_in + p];
      }
      peak_frame_owners(m.data(), F, own.data());
      for (int k = 0; k < F; ++k) {
        if ((int)own[k] != k) continue;
        pos[k] = peak_pos(k, m[k - 1], m[k], m[k + 1]);
        const uint16_t q = t == 0 ? kPeakNone : own_prev[k];
        phi[k] = q == kPeakNone ? 0.0 : peak_advance(phi_prev[q], pos_prev[q], pos[k], peak_turns_per_bin(hop, n_fft));
      }
      for (int p = 0; p < stride_out; ++p) {
        int cj;
        const int bin = emu_peak_out_bin(spec_out, p, F, &cj);
        cf v{0.f, 0.f};
        if (bin >= 0) {
          v = peak_angle(own[bin] == kPeakNone ? 0.0 : phi[own[bin]], bin);
          if (cj) v.im = -v.im;
        }
        angles[2 * (fr * (size_t)stride_out + p)] = v.re;
        angles[2 * (fr * (size_t)stride_out + p) + 1] = v.im;
      }
      own_prev = own;
      phi_prev = phi;
      pos_prev = pos;
    }
}

}  // extern "C"
