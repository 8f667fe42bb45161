// rfx_imel_groups.hip - InverseMelScale SGD, group formulation: one workgroup of four waves per frame (the algorithm and the
// choice between the kernel families: rfx_imel.hip).  Bins whose first filter is g form group g (contiguous, disjoint):
//   A_g = sum w0*spec (into filter g)      B_g = sum w1*spec (into filter g+1)      pred_m = A_m + B_{m-1}
// A thread owns one short low-frequency group and one long high-frequency group with all of their
// state (spec, momentum buffer, both weights) in registers; per step it publishes A/B (4 LDS
// writes), crosses ONE barrier, reads its neighbours' B_{g-1} / A_{g+1} (4 LDS reads) and forms the
// two residuals it needs itself.  Nothing else touches memory inside the 200-step loop.
#include <hip/hip_runtime.h>

#include "rfx_imel.hip.h"

namespace rfx {

// ---------------------------------------------------------------------------------------------------
// Line form inside the group-kernel layout (round 5).  The wave kernel (rfx_imel_wave.hip) serves ONE bank shape (512 groups whose
// sizes fit its chunk budgets: the default 0 - 10 kHz bank); every bank with longer groups - 512 filters up to 16 / 20 / 22.05 kHz (the
// reference's own round-trip test runs 20 Hz .. 20 kHz, test/spectrogram_converter_test.py:46-53), 384 filters - fell through to
// the general LDS kernel: 169 ms per 64 tiles against 4.5.  The table form cannot take them either: with four registers per
// bin (spec, buffer, two weights) a 62-bin group does not fit a thread.  Here a thread keeps the group kernels' roles and LDS
// exchange (short group t, long group M-1-t; A and B published, one barrier per step, residuals formed from the neighbours'
// sums) but holds its LONG group in the wave kernel's line form - weights a0 + s0 i, momentum buffer C + G i (see rfx_imel_wave.hip),
// ONE register per bin plus a 0 / 1 mask per slot (group sizes vary inside a wave's class, and in unit form B = S - A must not see a
// padding slot) - while the short group stays in table form (group 0 of a bank may hold its first filter's rising edge and is not a line).
// The plan admits the kernel when the long groups M-256 .. M-1 are lines (rfx_plan_core.h, kImelKernelLine) and the budgets
// kImelLoCapLine / kImelHiCapLine hold every group.  Two waves per SIMD (the heaviest class holds 31 spec pairs + 31 masks).
template <int NP, bool UF>
struct LineGroup {
  static constexpr bool kUnitForm = UF, kLineForm = true;
  c2 spec[NP], mask[NP];
  float a0, s0, a1, s1;  // a1, s1 unused in unit form
  float C, G;            // the momentum buffer of the group's bin i is C + G i, in units of the STEP
};
template <int NP, bool UF>
__device__ __forceinline__ void group_load(LineGroup<NP, UF>& k, int g, const ImelArgs& a, int frame, unsigned rbase) {
  const ImelTables& tb = a.tb;
  const int f0 = g >= 0 ? tb.grp_start[g] : 0, n = g >= 0 ? tb.grp_start[g + 1] - f0 : 0;
  k.a0 = g >= 0 ? tb.lin[g] : 0.f;
  k.s0 = g >= 0 ? tb.lin[a.M + g] : 0.f;
  k.a1 = g >= 0 ? tb.lin[2 * a.M + g] : 0.f;
  k.s1 = g >= 0 ? tb.lin[3 * a.M + g] : 0.f;
  k.C = 0.f;
  k.G = 0.f;
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) {
    const bool ok = i < n;
    const int f = f0 + (ok ? i : 0);
    const float sp = ok ? a.sc * (a.spec0 ? a.spec0[(size_t)frame * a.n_stft + f] : rand_unit(rbase, f)) : 0.f;
    if (i & 1) { k.spec[i >> 1].y = sp; k.mask[i >> 1].y = ok ? 1.f : 0.f; }
    else       { k.spec[i >> 1].x = sp; k.mask[i >> 1].x = ok ? 1.f : 0.f; }
  }
}
// A = sum w0 x = a0 S + s0 Q with S = sum x_i, Q = sum i x_i (four accumulator chains); B likewise, or S - A in unit form
template <int NP, bool UF>
__device__ __forceinline__ void group_ab(const LineGroup<NP, UF>& k, float& A, float& B) {
  static_assert(NP >= 2, "a line group holds at least two pairs");
  c2 Sa = k.spec[0], Sb = k.spec[1], Qa = bc2(0.f), Qb = k.spec[1];
#pragma unroll
  for (int p = 2; p < NP; ++p) {
    if (p & 1) { Sb = Sb + k.spec[p]; Qb = __builtin_elementwise_fma(bc2((float)p), k.spec[p], Qb); }
    else       { Sa = Sa + k.spec[p]; Qa = __builtin_elementwise_fma(bc2((float)p), k.spec[p], Qa); }
  }
  const c2 S = Sa + Sb, Q = Qa + Qb;
  const float s = S.x + S.y, h = Q.x + Q.y;
  const float q = fmaf(2.f, h, S.y);  // sum i x_i over the slots (2p, 2p + 1) = 2 sum p (x_2p + x_2p+1) + sum x_2p+1
  A = fmaf(k.s0, q, k.a0 * s);
  B = UF ? s - A : fmaf(k.s1, q, k.a1 * s);
}
// The residuals enter times the step factor (n = nl d).  Gradient line cc + st i, buffer line (C, G) updated like
// torch.optim.SGD's buf.mul_(momentum).add_(grad), then x = clamp(x + mask (C + G i)) pair by pair
template <int NP, bool UF>
__device__ __forceinline__ void group_step(LineGroup<NP, UF>& k, float d0, float d1, float nl, unsigned long long /*nl2*/, float mom) {
  const float n0 = nl * d0, n1 = nl * d1;
  float cc, st;
  if (UF) {
    const float dd = n0 - n1;
    cc = fmaf(dd, k.a0, n1);
    st = dd * k.s0;
  } else {
    cc = fmaf(n1, k.a1, n0 * k.a0);
    st = fmaf(n1, k.s1, n0 * k.s0);
  }
  k.C = fmaf(mom, k.C, cc);
  k.G = fmaf(mom, k.G, st);
  const c2 base = c2{k.C, k.C + k.G}, s2 = bc2(k.G + k.G);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const c2 v = p == 0 ? base : __builtin_elementwise_fma(bc2((float)p), s2, base);
    k.spec[p] = pk_fma_clamp(k.spec[p], v, k.mask[p]);
  }
}
template <int NP, bool UF>
__device__ __forceinline__ void group_stage(const LineGroup<NP, UF>& k, int g, const ImelTables& tb, float* stage, float unscale) {
  if (g < 0) return;
  const int f0 = tb.grp_start[g], n = tb.grp_start[g + 1] - f0;
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i)
    if (i < n) stage[f0 + i - tb.f_lo] = unscale * ((i & 1) ? k.spec[i >> 1].y : k.spec[i >> 1].x);
}

// One frame on one workgroup; HI is the type that holds the thread's long group (table form or line form), the short group is
// always in table form.  `tid` is the thread's ROLE (0..255: which two groups it owns; roles 64c..64c+63 form size class c).
template <int NLO, class HI>
__device__ __forceinline__ void imel_group_body(ImelArgs a, char* smem, int tid, int frame) {
  constexpr bool UF = HI::kUnitForm;
  const ImelTables& tb = a.tb;
  const int M = a.M;
  float* Ab = reinterpret_cast<float*>(smem);  // [2][M + 4], entry m at index m + 1
  float* Bb = Ab + 2 * (M + 4);                // [2][M + 4]
  float* part = Bb + 2 * (M + 4);              // [max_iter][4] per-wave partial sums of diff^2

  const int b = frame / a.T, t = frame - b * a.T;
  const int clip = b / a.C;
  const int steps = a.it_limit ? a.it_limit[clip] : a.max_iter;
  if (a.it_limit && steps >= a.max_iter) return;  // fix-up pass: this clip never stopped early
  const unsigned rbase = rand_frame_key(a.seed, a.frame_base + (unsigned long long)frame);
  imel_set_scale(a, clip);

  int gH = (M - 1 - tid >= 0) ? M - 1 - tid : -1;           // long groups, counted down from the top
  int gL = (tid < M - kImelThreads) ? tid : -1;             // short groups, counted up from 0
  if constexpr (HI::kLineForm) {
    if (gH >= 0 && gH < tb.line_from) {  // a long group that is not a line: into the (free: the plan checked) table-form slot
      gL = gH;
      gH = -1;
    }
  }
  // the short groups keep both weights (the lowest bins sit below the first filter's centre and feed one filter only);
  // the long groups run in unit form when the plan found the bank fit for it (UF)
  GroupState<NLO, false> lo;
  HI hi;
  group_load(lo, gL, a, frame, rbase);
  group_load(hi, gH, a, frame, rbase);
  auto melat = [&](int m) { return (m >= 0 && m < M) ? a.sc * a.mel[((size_t)b * M + m) * a.T + t] : 0.f; };
  const float mL0 = gL >= 0 ? melat(gL) : 0.f, mL1 = gL >= 0 ? melat(gL + 1) : 0.f;
  const float mH0 = gH >= 0 ? melat(gH) : 0.f, mH1 = gH >= 0 ? melat(gH + 1) : 0.f;
  for (int i = tid; i < 4 * (M + 4); i += kImelThreads) Ab[i] = 0.f;  // Ab and Bb are contiguous: zero both incl. pads
  // The momentum buffer is kept in units of the gradient scale g = -2/(C T) of the loss mean (buf = g buf''): the step
  // spec -= lr buf becomes spec = fma(-lr g, buf'', spec) and the four products g * residual per step disappear
  const float lrg = a.lr * (-2.0f / (float)(a.C * a.T));
  const float nl = -lrg;
  // -lr g in both halves of an SGPR pair (wave-uniform: from kernel arguments only)
  const unsigned nlb = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, nl));
  const unsigned long long nl2 = ((unsigned long long)nlb << 32) | nlb;
  // an absent group (n_mels < 512) publishes zeros to the dump entry and reads the pads around it: the loop below has no
  // branches, and the four neighbour reads of a step go out together (one LDS round trip, not four)
  const int xL = (gL >= 0 ? gL : M + 1) + 1, xH = (gH >= 0 ? gH : M + 1) + 1;
  // unit form: the last group's second filter does not exist (its bins carry w1 == 0 in the bank): its residual is forced to 0
  const bool noH1 = UF && gH == M - 1;
  const int wave = tid >> 6;
  __syncthreads();

  // one SGD step; Ap / Bp = this step's half of the double buffers (the parity is a compile-time matter of the caller)
  auto sgd_step = [&](int it, float* __restrict__ Ap, float* __restrict__ Bp) {
    float AL, BL, AH, BH;
    group_ab(lo, AL, BL);
    group_ab(hi, AH, BH);
    Ap[xL] = AL; Bp[xL] = BL;
    Ap[xH] = AH; Bp[xH] = BH;
    __syncthreads();
    const float bLm = Bp[xL - 1], aLp = Ap[xL + 1], bHm = Bp[xH - 1], aHp = Ap[xH + 1];
    // residuals of the two filters each group feeds: d0 = diff[g], d1 = diff[g+1].  An absent group needs no special case:
    // its targets and sums are zero and the entries next to the dump are never written
    const float dL0 = mL0 - AL - bLm;
    const float dL1 = mL1 - aLp - BL;
    const float dH0 = mH0 - AH - bHm;
    const float dH1 = noH1 ? 0.f : mH1 - aHp - BH;
    // every filter's residual is owned exactly once; the loss history is kept in the reference's units
    const float uL = a.un * dL0, uH = a.un * dH0;
    const float sq = wave_sum(fmaf(uL, uL, uH * uH));
    if ((tid & 63) == 0) part[4 * it + wave] = sq;
    // (without the unit form the last filter needs nothing either: it has no successor and its d1 multiplies w1 == 0)
    group_step(lo, dL0, dL1, nl, nl2, a.momentum);
    group_step(hi, dH0, dH1, nl, nl2, a.momentum);
  };
  float* const A0 = Ab, * const A1 = Ab + (M + 4), * const B0 = Bb, * const B1 = Bb + (M + 4);
  int it = 0;
  for (; it + 1 < steps; it += 2) {
    sgd_step(it, A0, B0);
    sgd_step(it + 1, A1, B1);
  }
  if (it < steps) sgd_step(it, A0, B0);
  __syncthreads();

  float* stage = reinterpret_cast<float*>(smem + imel_group_lds_bytes(M, a.max_iter));  // behind the loss partials (imel_frame_lds_bytes)
  group_stage(lo, gL, tb, stage, a.un);
  group_stage(hi, gH, tb, stage, a.un);
  __syncthreads();
  imel_emit_frame(a, stage, frame, rbase, tid, kImelThreads);
  if (a.loss_hist && !a.it_limit)
    for (int i = tid; i < a.max_iter; i += kImelThreads)
      a.loss_hist[(size_t)frame * a.max_iter + i] = i < steps ? (part[4 * i] + part[4 * i + 1]) + (part[4 * i + 2] + part[4 * i + 3]) : 0.f;
}

// uniform register budget for every wave
template <int NLO, int NHI>
__global__ void __launch_bounds__(kImelThreads) imel_group_kernel(ImelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  imel_group_body<NLO, GroupState<NHI, false>>(a, smem, threadIdx.x, blockIdx.x);
}
// Group sizes fall with the role index (mel spacing is logarithmic): roles 64c..64c+63 form size class c, and each wave
// runs the body compiled for its class's maximum, so the long-group class no longer sets everybody's instruction count.
// All bodies execute the same sequence of barriers.  One frame per workgroup: several frames per workgroup with the classes
// dealt across the SIMDs, class dealing by hardware id and s_setprio by class were measured and rejected (DESIGN_HISTORY.md,
// "Measured and rejected: the Latin square" and round 3, second session).
template <int WPE, bool UF, int L0, int H0, int L1, int H1, int L2, int H2, int L3, int H3>
__global__ void __launch_bounds__(kImelThreads) __attribute__((amdgpu_waves_per_eu(WPE)))
imel_group_kernel_perwave(ImelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cls = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tid = cls * 64 + (threadIdx.x & 63);  // (the class as a wave-uniform constant of each case below)
  const int frame = blockIdx.x;
  switch (cls) {
    case 0: imel_group_body<L0, GroupState<H0, UF>>(a, smem, tid, frame); break;
    case 1: imel_group_body<L1, GroupState<H1, UF>>(a, smem, tid, frame); break;
    case 2: imel_group_body<L2, GroupState<H2, UF>>(a, smem, tid, frame); break;
    default: imel_group_body<L3, GroupState<H3, UF>>(a, smem, tid, frame); break;
  }
}
// the same with the long groups in line form
template <bool UF, int L0, int H0, int L1, int H1, int L2, int H2, int L3, int H3>
__global__ void __launch_bounds__(kImelThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) imel_line_kernel_perwave(ImelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cls = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tid = threadIdx.x;
  const int frame = blockIdx.x;
  switch (cls) {
    case 0: imel_group_body<L0, LineGroup<(H0 + 1) / 2, UF>>(a, smem, tid, frame); break;
    case 1: imel_group_body<L1, LineGroup<(H1 + 1) / 2, UF>>(a, smem, tid, frame); break;
    case 2: imel_group_body<L2, LineGroup<(H2 + 1) / 2, UF>>(a, smem, tid, frame); break;
    default: imel_group_body<L3, LineGroup<(H3 + 1) / 2, UF>>(a, smem, tid, frame); break;
  }
}

// waves per SIMD of the per-wave kernels: four with the default set (128 VGPRs, 16 waves per CU: 7.6 ms against 8.6 ms at three,
// measured); the wide set's class 0 holds 31 bins per thread (124 state registers): three (168 VGPRs)
constexpr int kImelWavesPerEu = 4, kImelWavesPerEuWide = 3;

template <bool WIDE, bool UF>
static void launch_perwave(const ImelArgs& a, size_t lds, hipStream_t stream) {
  constexpr const int* lo = WIDE ? kImelLoCapWide : kImelLoCap;
  constexpr const int* hi = WIDE ? kImelHiCapWide : kImelHiCap;
  constexpr int wpe = WIDE ? kImelWavesPerEuWide : kImelWavesPerEu;
  hipLaunchKernelGGL((imel_group_kernel_perwave<wpe, UF, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3]>), dim3(a.B * a.T), dim3(kImelThreads), lds,
                     stream, a);
}
template <bool UF>
static void launch_line(const ImelArgs& a, size_t lds, hipStream_t stream) {
  constexpr const int* lo = kImelLoCapLine;
  constexpr const int* hi = kImelHiCapLine;
  hipLaunchKernelGGL((imel_line_kernel_perwave<UF, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3]>), dim3(a.B * a.T), dim3(kImelThreads), lds, stream, a);
}

// one workgroup per frame, the fix-up pass too (it runs a different number of steps - and barriers - per clip)
hipError_t launch_imel_groups(const ImelArgs& a, ImelKernel kernel, hipStream_t stream) {
  const size_t lds = imel_frame_lds_bytes(a.M, a.max_iter, a.tb.f_hi - a.tb.f_lo);
  const bool uf = a.tb.unit_form != 0;
  switch (kernel) {
    case kImelKernelUniform: hipLaunchKernelGGL((imel_group_kernel<8, 24>), dim3(a.B * a.T), dim3(kImelThreads), lds, stream, a); break;
    case kImelKernelPerWave: uf ? launch_perwave<false, true>(a, lds, stream) : launch_perwave<false, false>(a, lds, stream); break;
    case kImelKernelPerWaveWide: uf ? launch_perwave<true, true>(a, lds, stream) : launch_perwave<true, false>(a, lds, stream); break;
    case kImelKernelLine: uf ? launch_line<true>(a, lds, stream) : launch_line<false>(a, lds, stream); break;
    default: return hipErrorInvalidValue;  // (not a group kernel)
  }
  return hipGetLastError();
}

}  // namespace rfx
