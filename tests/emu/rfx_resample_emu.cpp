// Host emulator of the windowed-sinc resampler's kernel (riffusion-hobby_amd/csrc/rfx_resample.hip): the table, the start of an output
// and the sum are rfx_resample_core.h's own, compiled for the host.
//   emu_rs_frames    K = ceil(n L / o) of the reduced pair, -1 past 2^31 - 1 or for arguments the entry refuses
//   emu_rs_table     n and ntaps of a pair; with arrays, first [n] and taps [ntaps][n] as rfx_resample_sinc_table answers them
//   emu_resample     rows of `in_stride` floats, read as zero outside [0, valid), -> the first K outputs of each row, out_stride floats
//                    apart: sample by sample what a thread of the kernel does (a thread's four rows are independent sums)
// Built by tests/test_resample_cpu.py with -ffp-contract=off: the only fused operations are the explicit fmaf's.
#include <cstdint>
#include <cstring>

#include "../../riffusion-hobby_amd/csrc/rfx_resample_core.h"

extern "C" {

long long emu_rs_frames(long long L, int orig, int neu) {
  rfx::RsGeom g;
  if (L < 1 || !rfx::rs_geom(orig, neu, 1, 1.0, &g)) return -1;
  return rfx::rs_frames(L, g.o, g.n);
}

int emu_rs_table(int orig, int neu, int lpw, double rolloff, int32_t* first, float* taps, int32_t* n_out, int32_t* ntaps_out) {
  rfx::RsGeom g;
  if (!rfx::rs_geom(orig, neu, lpw, rolloff, &g)) return -1;
  const int ntaps = rfx::rs_ntaps(g);
  if (first && taps) rfx::rs_table(g, ntaps, first, taps);
  *n_out = (int32_t)g.n;
  *ntaps_out = ntaps;
  return 0;
}

void emu_resample(const float* in, int rows, long long in_stride, long long valid, int o, int n, const int32_t* first, const float* taps,
                  int ntaps, float* out, long long out_stride, long long K) {
  for (int r = 0; r < rows; ++r) {
    const float* row = in + (size_t)r * in_stride;
    for (long long j = 0; j < K; ++j) {
      const rfx::RsStart s = rfx::rs_start(j, o, n, first);
      rfx::rs_accumulate<1>(&row, valid, s.at, taps + s.p, n, ntaps, out + (size_t)r * out_stride + j);
    }
  }
}

}  // extern "C"
