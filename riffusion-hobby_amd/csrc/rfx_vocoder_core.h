// rfx_vocoder_core.h - the phase vocoder of a time stretch (include/rfx.h "TIME STRETCH": rfx_phase_vocoder, rfx_time_stretch), written
// once for the kernel of rfx_vocoder.hip, the host half of plan creation (rfx_plan_core.h: vocoder_table) and the host emulator of
// the CPU tests (tests/emu/rfx_vocoder_emu.cpp).  It states
//   - the frame count and the frame pair of an output step, both in double;
//   - the per-bin arithmetic: magnitude and angle of a frame, the angle in TURNS; the wrapped advance; the wrapped accumulator; the
//     output from the wrapped turns;
//   - the walk over a bin's output steps that keeps the frame pair in registers and its loads ahead of the accumulator;
//   - the advance of a bin as an exact fraction, and the primary slot of a bin on the specialised engine.
//
// Definition (torchaudio.functional.phase_vocoder with phase_advance = linspace(0, pi hop, n_stft)), per bin k, X the bin's T frames,
// frames at or past T zero, T_out = ceil(T / rate):
//   step i        x = i rate (double), i0 = floor(x), alpha = (float)(x - i0)
//   magnitude     alpha |X[i0 + 1]| + (1 - alpha) |X[i0]|
//   phase         ph[0] = angle(X[0]);  ph[i + 1] = ph[i] + wrap(angle(X[i0 + 1]) - angle(X[i0]) - adv_k) + adv_k,  wrap to [-pi, pi]
//   output        magnitude (cos ph, sin ph)
// Why turns.  adv_k = pi hop k / (n_stft - 1) is up to pi hop radians per frame (1385 at hop 441) and float32 torch sums it as it is: after 512
// frames the sum is near 7e5 rad, where an ulp is 0.06 rad.  Only ph modulo 2 pi reaches the output, so here every phase is a
// fraction of a turn: adv_k = (hop k mod D) / D with D = 2 (n_stft - 1), exact in integers and rounded once; the accumulator is
// wrapped to [-1/2, 1/2] after every step (x - rintf(x) is exact), so no term ever exceeds one turn and every addition rounds at
// 2^-24 turns or below; sine and cosine are taken of the wrapped turns (sincospif), never of a large argument.
// Conjugation.  Every operation is odd in the angle (rintf rounds ties to even: rint(-x) = -rint(x)), so the trajectory of a
// conjugate slot is the conjugate of its bin's, number for number (x - x is +0 either way: only the sign of an exact zero can
// differ): a slot that holds conj X runs with -adv_k.  Two slots of one bin must agree in bits, so the kernel does not rely on this
// between them: both run the primary slot's trajectory and the one whose flag differs conjugates the result.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rfx_core.h"

namespace rfx {

// ---- frames -------------------------------------------------------------------------------------------------------------------------
// T_out = ceil(T / rate) in double, the length of torch.arange(0, T, rate); -1: not finite, rate <= 0, T < 1 or a count past 2^31 - 1
inline long long voc_frames(int T, double rate) {
  if (!(rate > 0.0) || !(rate <= 1.7976931348623157e308) || T < 1) return -1;
  const double n = ceil((double)T / rate);
  return n >= 1.0 && n <= 2147483647.0 ? (long long)n : -1;
}
// the frame pair (i0, i0 + 1) of step i and the weight of the second frame
RFX_HD int voc_step(int i, double rate, float* alpha) {
  const double x = (double)i * rate, f = floor(x);
  if (alpha) *alpha = (float)(x - f);
  return f < 2147483646.0 ? (int)f : 2147483646;  // (at or past T either way: a zero frame)
}

// ---- the advance of a bin, in turns ------------------------------------------------------------------------------------------------------
// frac(hop k / D), D = 2 (n_stft - 1): torchaudio's linspace(0, pi hop, n_stft)[k] / (2 pi) modulo 1, for even and odd n_fft alike
inline float voc_advance_turns(int hop, int k, int n_stft) {
  const long long D = 2LL * (n_stft - 1);
  return D > 0 ? (float)((double)(((long long)hop * k) % D) / (double)D) : 0.f;
}
// the slot rfx_unpack_complex reads bin k from on the specialised engine, and whether it holds the conjugate
inline int voc_spec_primary(int bin, bool* conj) {
  int k = bin;
  const bool cj = k % 40 > 20;
  if (cj) k = kNfft - k;
  if (conj) *conj = cj;
  const int k1 = k % 40, kp = k / 40;
  return slot_pos_c(k1 * 21 + kp % 21, kp / 21);
}
// A table entry as the kernel reads it: x = primary position of the position's bin | kVocFlip where exactly one of the two holds the
// conjugate (the walk then runs in the primary's orientation, with the advance negated, and the result is conjugated as it is
// written), -1 for padding; y = the bits of the position's own signed advance
constexpr int kVocFlip = 1 << 30;

// ---- per-bin arithmetic --------------------------------------------------------------------------------------------------------------------
struct VocPolar {
  float m, a;  // modulus (hypotf: no overflow of the squares at X 2^+-40), angle in turns
};
RFX_HD VocPolar voc_polar(cf v) { return VocPolar{hypotf(v.re, v.im), atan2f(v.im, v.re) * 0.15915494309189533577f}; }
RFX_HD float voc_wrap(float t) { return t - rintf(t); }  // exact for |t| < 2^23; to [-1/2, 1/2]
// one step of the accumulator: acc + wrap(a1 - a0 - adv) + adv, wrapped; advc = voc_wrap(adv), every intermediate within one turn
RFX_HD float voc_accumulate(float acc, float a0, float a1, float advc) {
  float d = voc_wrap(a1 - a0);
  d = voc_wrap(d - advc);
  return voc_wrap(acc + (d + advc));
}
RFX_HD void voc_sincos_turns(float t, float* s, float* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincospif(2.f * t, s, c);
#else
  const double a = 6.283185307179586476925286766559 * (double)t;  // (the host has no sincospif: double, rounded once)
  *s = (float)sin(a);
  *c = (float)cos(a);
#endif
}
RFX_HD cf voc_output(VocPolar p0, VocPolar p1, float alpha, float acc) {
  const float mag = alpha * p1.m + (1.f - alpha) * p0.m;
  float s, c;
  voc_sincos_turns(acc, &s, &c);
  return cf{mag * c, mag * s};
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------------
// All T_out steps of one bin.  load(j): frame j < T of the bin; store(i, v): output step i.  The pair of a step stays in registers in
// polar form: a step whose pair is the last one's loads nothing, one that moves by a frame loads one frame (every step at
// rate < 1 is one of the two).  Which frames a step needs depends on i and rate alone, so they are loaded two steps ahead of the
// accumulator and turned into polar form one step ahead: the only chain from step to step is voc_accumulate's three additions.
// The branches depend on the step alone - uniform over a wave.
template <class Load, class Store>
RFX_HD void voc_walk(int T, int T_out, double rate, float adv, Load load, Store store) {
  const cf zero{0.f, 0.f};
  const float advc = voc_wrap(adv);
  int cur = 0;  // the pair of the step at hand: frames cur, cur + 1
  VocPolar p0 = voc_polar(load(0)), p1 = voc_polar(T > 1 ? load(1) : zero);
  float acc = p0.a;
  // loaded for the next step: frames ja, ja + 1 where they are not in the pair at hand
  int ja = T_out > 1 ? voc_step(1, rate, nullptr) : 0;
  cf ra0 = zero, ra1 = zero;
  if (ja - cur >= 2 && ja < T) ra0 = load(ja);
  if (ja - cur >= 1 && ja + 1 < T) ra1 = load(ja + 1);
  for (int i = 0; i < T_out; ++i) {
    // 1: the loads of step i + 2
    const int jb = i + 2 < T_out ? voc_step(i + 2, rate, nullptr) : ja;
    cf rb0 = zero, rb1 = zero;
    if (jb - ja >= 2 && jb < T) rb0 = load(jb);
    if (jb - ja >= 1 && jb + 1 < T) rb1 = load(jb + 1);
    // 2: the pair of step i + 1
    VocPolar n0 = p0, n1 = p1;
    if (ja - cur == 1) {
      n0 = p1;
      n1 = voc_polar(ra1);
    } else if (ja - cur >= 2) {
      n0 = voc_polar(ra0);
      n1 = voc_polar(ra1);
    }
    // 3: step i
    float alpha;
    voc_step(i, rate, &alpha);
    store(i, voc_output(p0, p1, alpha, acc));
    acc = voc_accumulate(acc, p0.a, p1.a, advc);
    p0 = n0;
    p1 = n1;
    cur = ja;
    ja = jb;
    ra0 = rb0;
    ra1 = rb1;
  }
}

}  // namespace rfx
