// Host emulator of the compression kernels (csrc/rfx_compress.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_compression_cpu.py with g++): it runs the functions of rfx_compress_core.h and rfx_pcm_core.h that the kernels
// inline - prepare (normalize, gain to -10 dBFS, window rms from int64 prefix sums), the recurrence in both forms with the
// chunked form's repair rounds taken in the same order, the apply with its flags, the host patch, and the compression=False
// filters - so that they are pinned against PcmSegment on the CPU.
#include <cstdint>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_compress_core.h"

using namespace rfx;

namespace {

// the chunked form of one clip: what cmp_chunked_kernel's lanes do, one round at a time
int chunked(const uint16_t* rms, int64_t L, int64_t CH, const CmpTables& t, double* traj) {
  const int K = (int)((L + CH - 1) / CH);
  std::vector<double> st(K), en(K), want(K);
  std::vector<int> src(K);
  std::vector<char> quiet(K);
  auto b_of = [&](int k) { return (int64_t)k * CH; };
  auto e_of = [&](int k) { return (int64_t)k * CH + CH < L ? (int64_t)k * CH + CH : L; };
  for (int k = 0; k < K; ++k) {
    bool loud = false;
    en[k] = cmp_run(0.0, rms, t, traj, b_of(k), e_of(k), false, nullptr, &loud);
    st[k] = 0.0;
    quiet[k] = !loud;
  }
  int last = -1;
  for (int k = 0; k < K; ++k) {
    src[k] = last;
    if (!quiet[k]) last = k;
  }
  int rounds = 0;
  for (;;) {
    for (int k = 0; k < K; ++k) want[k] = src[k] >= 0 ? en[src[k]] : 0.0;
    bool any = false;
    for (int k = 0; k < K; ++k) {
      if (quiet[k] || cmp_bits(want[k]) == cmp_bits(st[k])) continue;
      bool hit = false;
      const double z = cmp_run(want[k], rms, t, traj, b_of(k), e_of(k), true, &hit, nullptr);
      if (!hit) en[k] = z;
      st[k] = want[k];
      any = true;
    }
    if (!any) break;
    ++rounds;
  }
  for (int k = 0; k < K; ++k)
    if (quiet[k] && src[k] >= 0)
      for (int64_t i = b_of(k); i < e_of(k); ++i) traj[i] = en[src[k]];
  return rounds;
}

}  // namespace

extern "C" {

// audioop.rms of every frame's window (L frames of C channels)
void emu_window_rms(const int16_t* x, int64_t L, int C, int64_t look, uint16_t* rms) {
  std::vector<int64_t> prefix(L + 1, 0);
  for (int64_t j = 0; j < L; ++j) {
    int64_t e = 0;
    for (int c = 0; c < C; ++c) e += (int64_t)x[j * C + c] * x[j * C + c];
    prefix[j + 1] = prefix[j] + e;
  }
  for (int64_t i = 0; i < L; ++i) rms[i] = (uint16_t)cmp_window_rms(prefix.data(), i, look, C);
}

// the recurrence over one clip's rms values; form 0 sequential, 1 chunked (chunk_frames as the C entry takes it).
// Returns the repair rounds.
int emu_attenuation(const uint16_t* rms, int64_t L, const uint8_t* above, const double* max_att, const double* inc, const double* dec,
                    int form, int64_t chunk_frames, double* traj) {
  const CmpTables t{above, max_att, inc, dec};
  if (form == 0) {
    cmp_run(0.0, rms, t, traj, 0, L, false, nullptr, nullptr);
    return 0;
  }
  return chunked(rms, L, cmp_chunk_frames(L, chunk_frames), t, traj);
}

// the whole of rfx_pcm16_apply_filters_compressed on an (N, L, C) batch; att (N x L, optional) receives the attenuations,
// rounds (N, optional) the repair rounds.  Returns the number of flagged samples (all of them patched).
int64_t emu_apply_filters_compressed(const int16_t* in, int N, int64_t L, int C, const double* gain10, const double* gain12,
                                     const double* boost, const uint8_t* above, const double* max_att, const double* inc,
                                     const double* dec, int64_t look, int form, int64_t chunk_frames, double margin, int16_t* out,
                                     double* att, int* rounds) {
  const int64_t count = L * C;
  int64_t flagged = 0;
  std::vector<double> traj(L);
  std::vector<uint16_t> rms(L);
  std::vector<int16_t> x2(count);
  for (int n = 0; n < N; ++n) {
    const int16_t* x = in + n * count;
    int mx = -32768, mn = 32767;
    for (int64_t i = 0; i < count; ++i) {
      mx = x[i] > mx ? x[i] : mx;
      mn = x[i] < mn ? x[i] : mn;
    }
    const double f_norm = boost[mx > -mn ? mx : -mn];
    int64_t s = 0;
    for (int64_t i = 0; i < count; ++i) {
      const int v = pcm_mul(x[i], f_norm);
      s += (int64_t)v * v;
    }
    const CmpFactors f{f_norm, gain10[pcm_rms(s, count)]};
    for (int64_t i = 0; i < count; ++i) x2[i] = (int16_t)cmp_x2(x[i], f);
    emu_window_rms(x2.data(), L, C, look, rms.data());
    const int r = emu_attenuation(rms.data(), L, above, max_att, inc, dec, form, chunk_frames, traj.data());
    if (rounds) rounds[n] = r;
    if (att)
      for (int64_t i = 0; i < L; ++i) att[n * L + i] = traj[i];
    int16_t* y = out + n * count;
    for (int64_t i = 0; i < count; ++i) {
      const double a = traj[i / C];
      int v = x2[i];
      if (a != 0.0) {
        const double g = cmp_gain_dev(a);
        v = pcm_mul(x2[i], g);
        if (x2[i] != 0 && cmp_near_integer(pcm_dmul((double)x2[i], g), margin)) {
          v = pcm_mul(x2[i], cmp_gain_host(a));  // the host's patch
          ++flagged;
        }
      }
      y[i] = (int16_t)v;
    }
    int64_t s3 = 0;
    int mx3 = -32768, mn3 = 32767;
    for (int64_t i = 0; i < count; ++i) {
      s3 += (int64_t)y[i] * y[i];
      mx3 = y[i] > mx3 ? y[i] : mx3;
      mn3 = y[i] < mn3 ? y[i] : mn3;
    }
    const PcmFactors pf = pcm_filter_factors(s3, count, mx3, mn3, gain12, boost);
    for (int64_t i = 0; i < count; ++i) y[i] = pcm_filter_sample(y[i], pf);
  }
  return flagged;
}

}  // extern "C"
