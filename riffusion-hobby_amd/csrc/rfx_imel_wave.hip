// rfx_imel_wave.hip - InverseMelScale SGD, the wave kernel: one wave per frame (the algorithm and the choice between the kernel
// families: rfx_imel.hip; the scaled state, the clamps and the epilogue it shares with the group kernels: rfx_imel.hip.h).
#include <hip/hip_runtime.h>

#include "rfx_imel.hip.h"

namespace rfx {

// ---------------------------------------------------------------------------------------------------
// Wave kernel (round 4): ONE wave per frame, no barrier and no LDS exchange inside the SGD loop.
//
// The group kernels (rfx_imel_groups.hip) cross a workgroup barrier per step with four waves of unequal length; 39 % of their wave-cycles
// are spent parked (profiles/r04_imel_pmc.json).  Here a frame is one wave: lane l owns eight groups, one per chunk of 64
// consecutive groups - group 64 c + l in the even chunks, 64 c + 63 - l in the odd ones (rfx_kernels.h::imel_wave_group) - so
//  * every lane carries 60 - 67 of the 4000 active bins although a group grows from 1 to 23 bins over the bank,
//  * the neighbours g - 1 and g + 1 of a lane's group sit in the adjacent lane (one DPP wave shift each) or, where two chunks
//    meet, in the lane itself (the `old` operand of the same DPP instruction: the shift leaves the end lane untouched),
//  * all state of the frame stays in the wave's VGPRs at two waves per SIMD.
// Two observations make the state small and the step cheap:
//  1. on a uniform bin grid a triangular filter's weight is LINEAR in the bin index inside a group, w0 = a0 + s0 i,
//     w1 = a1 + s1 i (least-squares line in double, checked against the table to 1e-6 per bin at plan creation,
//     ImelTables::lin), so with S = sum x_i and Q = sum i x_i
//        A = a0 S + s0 Q,  B = a1 S + s1 Q  (unit form, chunks 4 - 7 of a bank without area normalisation: B = S - A)
//        gradient of bin i = (d0 a0 + d1 a1) + (d0 s0 + d1 s1) i  =: cc + st i        - no weight registers;
//  2. the gradient is a line in i, the momentum buffer starts at zero and torch.optim.SGD updates it linearly
//     (buf <- momentum buf + grad, whatever the clamp does to x afterwards), so the buffer of a group's bin i IS the line
//     C + G i with C <- momentum C + cc, G <- momentum G + st: two scalars per group instead of a register per bin.
// A PAIR of bins (2p, 2p + 1) then costs four packed instructions per step - S += x; Q += p x (Q = 2 (Qx + Qy) + Sy);
// v = fma(p, (2 h, 2 h), (-lr g C, -lr g C + h)) with h = -lr g G; x = clamp(x + v) - minus the p = 0 and p = 1 terms that need
// no arithmetic: 132 packed instructions per frame and step where the group kernels issue 209.  The state is the scaled one
// of the group kernels (2^-60, output clamp), the residuals are formed in the same order.
// Padding slots (a lane's group is shorter than its chunk's budget) hold x = 0 and their step is multiplied by a per-lane
// 0 / 1 mask (x = clamp(fma(v, mask, x))) - only the pairs behind kImelWaveFullPairs can be padding and carry one.
// The per-step loss (sum of the squared residuals over the frame's filters, read by imel_scan_kernel) is summed by the LDS
// unit (ds_add_f32 of all lanes into one word: the unit is otherwise idle here), not by six DPP steps on the VALU.
// Numerics: not bit-identical to the group kernels (weights and buffer from lines: within one ulp of the GROUP's largest weight -
// the plan admits this kernel only if every bin's weight is within 4e-7 of that maximum of its fitted line, rfx_plan_core.h - sums in
// another order); emulated in numpy against the oracle (tests/test_imel_wave_form.py) rel-L2 3.1e-7 after 120 steps (table weights:
// 2.1e-7), on the device 8.9e-8 against the group kernels at T = 512, gate 1e-3.
// Measured per VALU instruction and SIMD at two waves per SIMD (tools/ubench/valu_rate.hip): v_pk_fma_f32 2.4 ns, v_fma_f32 1.5,
// v_mov_b32_dpp wave_shr 2.1: the kernel runs at the sum of its instructions' costs, i.e. the count is what is left to cut.
// ---------------------------------------------------------------------------------------------------
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;
// lane i receives `src` of lane i - 1 (SHR) or i + 1 (SHL); the lane at the end keeps `old`
template <int CTRL>
__device__ __forceinline__ float wave_shift(float old, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL, 0xf, 0xf, false));
}


// x = m x + c written over x (hipcc picks v_fmac, whose result lands in c's register, and copies it back every trip of the loop)
__device__ __forceinline__ void fma_in_place(float& x, unsigned m_sgpr, float c) { asm("v_fma_f32 %0, %1, %0, %2" : "+v"(x) : "s"(m_sgpr), "v"(c)); }

template <int NP, int NF, bool UF>  // NP pairs of slots, the first NF of them full in every lane
struct WvChunk {
  static constexpr int NT = NP - NF;
  c2 spec[NP];
  c2 mask[NT > 0 ? NT : 1];
  float C, G;            // the momentum buffer of the group's bin i is C + G i, in units of the STEP (-lr x gradient scale folded in)
};

template <int NP, int NF, bool UF>
__device__ __forceinline__ void wv_load(WvChunk<NP, NF, UF>& k, int g, const ImelArgs& a, int frame, unsigned rbase) {
  const ImelTables& tb = a.tb;
  const int f0 = tb.grp_start[g], n = tb.grp_start[g + 1] - f0;
  k.C = 0.f;
  k.G = 0.f;
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) {
    const bool ok = i < n;
    const int f = f0 + (ok ? i : 0);
    const float sp = ok ? a.sc * (a.spec0 ? a.spec0[(size_t)frame * a.n_stft + f] : rand_unit(rbase, f)) : 0.f;
    if (i & 1) k.spec[i >> 1].y = sp; else k.spec[i >> 1].x = sp;
    if (i >= 2 * NF) {
      if (i & 1) k.mask[(i >> 1) - NF].y = ok ? 1.f : 0.f; else k.mask[(i >> 1) - NF].x = ok ? 1.f : 0.f;
    }
  }
}
// The step is written phase by phase ACROSS chunks - the compiler keeps the source order of independent instructions: the
// packed sums of two chunks advance together (four accumulator chains), the scalar chains of a chunk pair share packed
// instructions (round 7, imel_wave_kernel), and the update forms all of a chunk's step pairs before it applies them.
template <int NPA, int NFA, int NPB, int NFB, bool UFA, bool UFB>
__device__ __forceinline__ void wv_sums2(const WvChunk<NPA, NFA, UFA>& ka, const WvChunk<NPB, NFB, UFB>& kb, c2& SA, c2& QA, c2& SB, c2& QB) {
  static_assert(NPA >= 2 && NPB >= 2, "every chunk holds at least two pairs");
  SA = ka.spec[0] + ka.spec[1];
  SB = kb.spec[0] + kb.spec[1];
  QA = ka.spec[1];
  QB = kb.spec[1];
#pragma unroll
  for (int p = 2; p < (NPA > NPB ? NPA : NPB); ++p) {
    if (p < NPA) SA = SA + ka.spec[p];
    if (p < NPB) SB = SB + kb.spec[p];
    if (p < NPA) QA = __builtin_elementwise_fma(bc2((float)p), ka.spec[p], QA);
    if (p < NPB) QB = __builtin_elementwise_fma(bc2((float)p), kb.spec[p], QB);
  }
}
// step of the pair p: v_p = (C, C + G) + 2p (G, G) - the same bits as p (2 G, 2 G): a power of two commutes with the product, so the
// chunk needs no w2 = G + G
template <int NP, int NF, bool UF>
__device__ __forceinline__ void wv_update(WvChunk<NP, NF, UF>& k, float vy) {
  const c2 base = c2{k.C, vy}, g2 = bc2(k.G);
  c2 v[NP];
  v[0] = base;
#pragma unroll
  for (int p = 1; p < NP; ++p) v[p] = __builtin_elementwise_fma(bc2((float)(2 * p)), g2, base);
#pragma unroll
  for (int p = 0; p < NP; ++p) k.spec[p] = p < NF ? pk_add_clamp(k.spec[p], v[p]) : pk_fma_clamp(k.spec[p], v[p], k.mask[p < NF ? 0 : p - NF]);
}
// s = x + y as one plain instruction: two of them feeding the halves of a pair are otherwise merged into a v_pk_add_f32 whose
// operands the compiler first gathers with two moves
__device__ __forceinline__ float wv_add(float x, float y) {
  float s;
  asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(x), "v"(y));
  return s;
}
// q = 2 h + y as the three-address v_fma_f32 (the two-address v_fmac would need a copy of y to land q in a pair half)
__device__ __forceinline__ float wv_fma2(float h, float y) {
  float q;
  asm("v_fma_f32 %0, 2.0, %1, %2" : "=v"(q) : "v"(h), "v"(y));
  return q;
}
// (x.y, y.x): the high half of one register pair and the low half of the next in one instruction
__device__ __forceinline__ c2 wv_gather(c2 x, c2 y) {
  c2 r;
  asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
// The line coefficients and mel targets of the chunk pair (2 j, 2 j + 1), one chunk per half: the per-group scalar chain of a step
// (A and B, residual, loss, gradient line) runs on both chunks of the pair in one packed instruction (round 7)
struct WvLines {
  c2 a0, s0, a1, s1;  // a1, s1 unused in unit form
  c2 m0;              // scaled mel target of filter g, for the group of each chunk
};
__device__ __forceinline__ void wv_load_lines(WvLines& l, int c, int lane, const ImelArgs& a, int b, int t) {
  const ImelTables& tb = a.tb;
  const int g0 = imel_wave_group(c, lane), g1 = imel_wave_group(c + 1, lane);
  l.a0 = c2{tb.lin[g0], tb.lin[g1]};
  l.s0 = c2{tb.lin[a.M + g0], tb.lin[a.M + g1]};
  l.a1 = c2{tb.lin[2 * a.M + g0], tb.lin[2 * a.M + g1]};
  l.s1 = c2{tb.lin[3 * a.M + g0], tb.lin[3 * a.M + g1]};
  l.m0 = c2{a.sc * a.mel[((size_t)b * a.M + g0) * a.T + t], a.sc * a.mel[((size_t)b * a.M + g1) * a.T + t]};
}
// the chunk's bins, unscaled, into the frame's LDS stage (bin order: entry f - f_lo)
template <int NP, int NF, bool UF>
__device__ __forceinline__ void wv_stage(const WvChunk<NP, NF, UF>& k, int g, const ImelTables& tb, float* stage, float unscale) {
  const int f0 = tb.grp_start[g], n = tb.grp_start[g + 1] - f0;
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i)
    if (i < n) stage[f0 + i - tb.f_lo] = unscale * ((i & 1) ? k.spec[i >> 1].y : k.spec[i >> 1].x);
}

#define RFX_WV_CHUNKS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

template <bool UFH>  // unit form in the upper four chunks (triangles without area normalisation); false: both weights everywhere
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) imel_wave_kernel(ImelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part = reinterpret_cast<float*>(smem);  // [max_iter] sum of diff^2 over the frame's filters, in the reference's units
  const ImelTables& tb = a.tb;
  const int lane = threadIdx.x, frame = blockIdx.x;
  const int b = frame / a.T, t = frame - b * a.T;
  const int clip = b / a.C;
  const int steps = a.it_limit ? a.it_limit[clip] : a.max_iter;
  if (a.it_limit && steps >= a.max_iter) return;  // fix-up pass: this clip never stopped early
  const unsigned rbase = rand_frame_key(a.seed, a.frame_base + (unsigned long long)frame);
  imel_set_scale(a, clip);
  for (int i = lane; i < a.max_iter; i += 64) part[i] = 0.f;
  const unsigned part_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;  // LDS byte address of part[0]

#define RFX_WV_DECL(c, UF) WvChunk<kImelWavePairs[c], kImelWaveFullPairs[c], UF> k##c;
  RFX_WV_DECL(0, false) RFX_WV_DECL(1, false) RFX_WV_DECL(2, false) RFX_WV_DECL(3, false)
  RFX_WV_DECL(4, UFH) RFX_WV_DECL(5, UFH) RFX_WV_DECL(6, UFH) RFX_WV_DECL(7, UFH)
#undef RFX_WV_DECL
#define RFX_WV_LOAD(c) wv_load(k##c, imel_wave_group(c, lane), a, frame, rbase);
  RFX_WV_CHUNKS(RFX_WV_LOAD)
#undef RFX_WV_LOAD
  WvLines l0, l1, l2, l3;
  wv_load_lines(l0, 0, lane, a, b, t);
  wv_load_lines(l1, 2, lane, a, b, t);
  wv_load_lines(l2, 4, lane, a, b, t);
  wv_load_lines(l3, 6, lane, a, b, t);

  const float nl = -(a.lr * (-2.0f / (float)(a.C * a.T)));  // the step in units of the gradient scale -2 / (C T), see rfx_imel_groups.hip::imel_group_body
  const unsigned mom_s = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, a.momentum));
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the zeroed loss words (one wave per workgroup: no barrier needed)

  for (int it = 0; it < steps; ++it) {
    // Round 7: every scalar of the chain below that a chunk has once per group is computed for the chunk PAIR (2 j, 2 j + 1) in
    // one packed instruction (the pairs are X01, X23, X45, X67, chunk 2 j in .x).  Contraction is off: each operation is written
    // as the one instruction the plain form of rounds 4 - 6 compiled to, so the bits are those of rounds 4 - 6.
#pragma clang fp contract(off)
    c2 sP01, sP23, sP45, sP67, qP01, qP23, qP45, qP67;
    {  // packed group sums (S = sum x, Q as in wv_sums2), then their scalar tails s = S.x + S.y, q = 2 (Q.x + Q.y) + S.y: the halves
       // of ONE register pair meet here, so these stay plain and land in the halves of the chunk pair's registers
      c2 S0, Q0, S1, Q1, S2, Q2, S3, Q3, S4, Q4, S5, Q5, S6, Q6, S7, Q7;
      wv_sums2(k0, k1, S0, Q0, S1, Q1);
      wv_sums2(k2, k3, S2, Q2, S3, Q3);
      wv_sums2(k4, k5, S4, Q4, S5, Q5);
      wv_sums2(k6, k7, S6, Q6, S7, Q7);
#define RFX_WV_T(c0, c1) sP##c0##c1 = c2{wv_add(S##c0.x, S##c0.y), wv_add(S##c1.x, S##c1.y)}; \
      qP##c0##c1 = c2{wv_fma2(Q##c0.x + Q##c0.y, S##c0.y), wv_fma2(Q##c1.x + Q##c1.y, S##c1.y)};
      RFX_WV_T(0, 1) RFX_WV_T(2, 3) RFX_WV_T(4, 5) RFX_WV_T(6, 7)
#undef RFX_WV_T
    }
    // A = a0 s + s0 q, B = a1 s + s1 q (unit form, chunks 4 - 7: B = s - A)
    const c2 A01 = __builtin_elementwise_fma(l0.s0, qP01, l0.a0 * sP01), A23 = __builtin_elementwise_fma(l1.s0, qP23, l1.a0 * sP23),
             A45 = __builtin_elementwise_fma(l2.s0, qP45, l2.a0 * sP45), A67 = __builtin_elementwise_fma(l3.s0, qP67, l3.a0 * sP67);
    const c2 B01 = __builtin_elementwise_fma(l0.s1, qP01, l0.a1 * sP01), B23 = __builtin_elementwise_fma(l1.s1, qP23, l1.a1 * sP23);
    const c2 B45 = UFH ? sP45 - A45 : __builtin_elementwise_fma(l2.s1, qP45, l2.a1 * sP45);
    const c2 B67 = UFH ? sP67 - A67 : __builtin_elementwise_fma(l3.s1, qP67, l3.a1 * sP67);
    // B of group g - 1: the previous lane of an even chunk (wave_shr), the next lane of an odd one (wave_shl); the end lane's
    // predecessor is the previous chunk's group in the lane itself.  Residual of filter g: d0 = (mel_g - A_g) - B_{g-1}
    // The shifts write over the B they take `old` from (the end lane's value), so p_c lands in the register of B_{c-1}: one chunk
    // off the pairing.  The subtractions stay plain and pair the residuals again (a packed form costs a move per shift)
    const c2 r01 = l0.m0 - A01, r23 = l1.m0 - A23, r45 = l2.m0 - A45, r67 = l3.m0 - A67;
    const c2 d01 = c2{r01.x - wave_shift<kDppWaveShr1>(0.f, B01.x), r01.y - wave_shift<kDppWaveShl1>(B01.x, B01.y)},
             d23 = c2{r23.x - wave_shift<kDppWaveShr1>(B01.y, B23.x), r23.y - wave_shift<kDppWaveShl1>(B23.x, B23.y)},
             d45 = c2{r45.x - wave_shift<kDppWaveShr1>(B23.y, B45.x), r45.y - wave_shift<kDppWaveShl1>(B45.x, B45.y)},
             d67 = c2{r67.x - wave_shift<kDppWaveShr1>(B45.y, B67.x), r67.y - wave_shift<kDppWaveShl1>(B67.x, B67.y)};
    {  // every filter's residual is owned exactly once; the loss history is kept in the reference's units.  The even chunks
       // accumulate in .x, the odd ones in .y, in the order of rounds 4 - 6
      const c2 un2 = bc2(a.un);
      const c2 u01 = un2 * d01, u23 = un2 * d23, u45 = un2 * d45, u67 = un2 * d67;
      const c2 sq = __builtin_elementwise_fma(u67, u67, __builtin_elementwise_fma(u45, u45, __builtin_elementwise_fma(u23, u23, u01 * u01)));
      // one ds_add_f32 of all 64 lanes into the step's word: the LDS unit adds them (written as asm: the compiler's atomic
      // optimizer would replace a uniform-address atomic by a 64-trip v_readlane loop on the VALU)
      asm volatile("ds_add_f32 %0, %1" ::"v"(part_lds + 4u * (unsigned)it), "v"(sq.x + sq.y) : "memory");
    }
    // From here on the residuals carry the step factor -lr g (n = -lr g d): everything below is linear in them, so the buffer
    // line (C, G) is kept in step units and needs no further scaling
    const c2 nl2 = bc2(nl);
    const c2 n001 = nl2 * d01, n023 = nl2 * d23, n045 = nl2 * d45, n067 = nl2 * d67;
    // residual of filter g + 1 = that of the next group: the next lane of an even chunk, the previous lane of an odd one, the
    // following chunk's in the end lane; filter 512 does not exist (chunk 7, lane 0: zero)
    // (the shifts' `old` values of a pair, (n0_{2j+1}, n0_{2j+2}), straddle two register pairs: one v_pk_mov_b32 gathers them)
    const c2 o01 = wv_gather(n001, n023), o23 = wv_gather(n023, n045), o45 = wv_gather(n045, n067), o67 = wv_gather(n067, bc2(0.f));
    const c2 n101 = c2{wave_shift<kDppWaveShl1>(o01.x, n001.x), wave_shift<kDppWaveShr1>(o01.y, n001.y)},
             n123 = c2{wave_shift<kDppWaveShl1>(o23.x, n023.x), wave_shift<kDppWaveShr1>(o23.y, n023.y)},
             n145 = c2{wave_shift<kDppWaveShl1>(o45.x, n045.x), wave_shift<kDppWaveShr1>(o45.y, n045.y)},
             n167 = c2{wave_shift<kDppWaveShl1>(o67.x, n067.x), wave_shift<kDppWaveShr1>(o67.y, n067.y)};
    // gradient line of every chunk: bin i of the group gets cc + st i (both weights: chunks 0 - 3; unit form: 4 - 7, with
    // dd = n0 - n1 formed as fma(nl, d0, -n1), the contraction rounds 4 - 6 compiled it to)
    const c2 cc01 = __builtin_elementwise_fma(n101, l0.a1, n001 * l0.a0), st01 = __builtin_elementwise_fma(n101, l0.s1, n001 * l0.s0);
    const c2 cc23 = __builtin_elementwise_fma(n123, l1.a1, n023 * l1.a0), st23 = __builtin_elementwise_fma(n123, l1.s1, n023 * l1.s0);
    c2 cc45, st45, cc67, st67;
    if (UFH) {
      const c2 dd45 = __builtin_elementwise_fma(nl2, d45, -n145), dd67 = __builtin_elementwise_fma(nl2, d67, -n167);
      cc45 = __builtin_elementwise_fma(dd45, l2.a0, n145);
      st45 = dd45 * l2.s0;
      cc67 = __builtin_elementwise_fma(dd67, l3.a0, n167);
      st67 = dd67 * l3.s0;
    } else {
      cc45 = __builtin_elementwise_fma(n145, l2.a1, n045 * l2.a0);
      st45 = __builtin_elementwise_fma(n145, l2.s1, n045 * l2.s0);
      cc67 = __builtin_elementwise_fma(n167, l3.a1, n067 * l3.a0);
      st67 = __builtin_elementwise_fma(n167, l3.s1, n067 * l3.s0);
    }
    // torch.optim.SGD: buf.mul_(momentum).add_(grad) for every bin of the group at once - the buffer line (C, G), in place -
    // then the step of the pair p: (C, C + G) + 2p (G, G).  (C, G) stay per chunk: the pair (C, C + G) the update reads must
    // sit in one register pair
#define RFX_WV_G(c, cc, st) fma_in_place(k##c.C, mom_s, cc); fma_in_place(k##c.G, mom_s, st); wv_update(k##c, k##c.C + k##c.G);
    RFX_WV_G(0, cc01.x, st01.x) RFX_WV_G(1, cc01.y, st01.y) RFX_WV_G(2, cc23.x, st23.x) RFX_WV_G(3, cc23.y, st23.y)
    RFX_WV_G(4, cc45.x, st45.x) RFX_WV_G(5, cc45.y, st45.y) RFX_WV_G(6, cc67.x, st67.x) RFX_WV_G(7, cc67.y, st67.y)
#undef RFX_WV_G
  }

  // the frame leaves through the LDS stage (imel_emit_frame): active bins parked in bin order, then one walk over the positions
  float* stage = part + a.max_iter;  // [f_hi - f_lo]
#define RFX_WV_STAGE(c) wv_stage(k##c, imel_wave_group(c, lane), tb, stage, a.un);
  RFX_WV_CHUNKS(RFX_WV_STAGE)
#undef RFX_WV_STAGE
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // one wave: its LDS operations execute in order, the compiler must keep them so
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  imel_emit_frame(a, stage, frame, rbase, lane, 64);
  if (a.loss_hist && !a.it_limit) {
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS atomics
    for (int i = lane; i < a.max_iter; i += 64) a.loss_hist[(size_t)frame * a.max_iter + i] = i < steps ? part[i] : 0.f;
  }
}
#undef RFX_WV_CHUNKS

// one wave per frame (the fix-up pass too: its frames are independent of each other)
hipError_t launch_imel_wave(const ImelArgs& a, hipStream_t stream) {
  const size_t lds = imel_wave_lds_bytes(a.max_iter, a.tb.f_hi - a.tb.f_lo);
  if (a.tb.unit_form) hipLaunchKernelGGL(imel_wave_kernel<true>, dim3(a.B * a.T), dim3(64), lds, stream, a);
  else hipLaunchKernelGGL(imel_wave_kernel<false>, dim3(a.B * a.T), dim3(64), lds, stream, a);
  return hipGetLastError();
}

}  // namespace rfx
