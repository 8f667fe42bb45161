// rfx_imel.hip.h - device helpers shared by the InverseMelScale SGD kernel families (rfx_imel.hip: the algorithm and the dispatch;
// rfx_imel_groups.hip: the group kernels; rfx_imel_wave.hip: the wave kernel): the wave-wide sum, the LDS sizes of a frame, the
// staged epilogue, the scaled state with its clamps, and the table-form group (four registers per bin) of the group kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_core.h"
#include "rfx_kernels.h"

namespace rfx {

constexpr int kImelThreads = 256;

template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true);
  return x + __builtin_bit_cast(float, y);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_rows(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, false);
  return x + __builtin_bit_cast(float, y);
}
// sum over the 64 lanes of a wave (wave-uniform result): 4 DPP adds inside the rows of 16, then the row sums travel up
// through lane 15 (row_bcast:15 into rows 1 and 3) and lane 31 (row_bcast:31 into rows 2 and 3); lane 63 holds the total
__device__ __forceinline__ float wave_sum(float x) {
  x = dpp_add<0xB1>(x);   // quad_perm [1,0,3,2]
  x = dpp_add<0x4E>(x);   // quad_perm [2,3,0,1]
  x = dpp_add<0x141>(x);  // row_half_mirror
  x = dpp_add<0x140>(x);  // row_mirror
  x = dpp_add_rows<0x142, 0xA>(x);  // row_bcast:15
  x = dpp_add_rows<0x143, 0xC>(x);  // row_bcast:31
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// LDS of one frame of the group formulation: A and B double-buffered ([2][M + 4] each: entry m at index m + 1, zero pads
// at m = -1 and m = M, a dump entry for absent groups at m = M + 1 and its right neighbour), per-wave partial losses
// [max_iter][4]
RFX_HD size_t imel_group_lds_bytes(int M, int max_iter) { return sizeof(float) * (size_t)(4 * (M + 4) + 4 * max_iter); }
// ... followed by the epilogue's stage: the frame's active bins in bin order (round 5, see imel_emit_frame)
RFX_HD size_t imel_frame_lds_bytes(int M, int max_iter, int band) { return imel_group_lds_bytes(M, max_iter) + sizeof(float) * (size_t)((band + 3) & ~3); }
// the wave kernel's frame: the loss words [max_iter] and the stage (16.8 KB for the default bank: eight waves per CU)
RFX_HD size_t imel_wave_lds_bytes(int max_iter, int band) { return sizeof(float) * ((size_t)max_iter + (size_t)band); }

// The frame leaves in POSITION order, 16 bytes per lane, whole lines per wave-wide store (round 5).  Until then every kernel
// stored bin by bin: 9408 four-byte stores per frame to slot positions 336 B apart, 64 cache lines per wave-wide store - alone
// (max_iter = 1) the wave kernel took 2.05 ms per 64 tiles for 1.23 GB, and 1.2 ms of it stayed exposed behind the 200 steps
// (profiles/r05_imel_epilogue.txt).  Now the threads park the active bins in LDS in bin order (`stage`, entry f - f_lo; the caller
// synchronises between the two halves), then walk the frame's positions: pos_bin says which bin a position holds - from the stage
// if a filter reaches it, its initial value (passed through bit for bit) if none does, zero for padding.
__device__ __forceinline__ void imel_emit_frame(const ImelArgs& a, const float* stage, int frame, unsigned rbase, int tid, int nthr) {
  const ImelTables& tb = a.tb;
  float* out = a.out_slots + (size_t)frame * a.out_stride;
  auto value_at = [&](int bin) {
    if (bin < 0) return 0.f;
    if (bin >= tb.f_lo && bin < tb.f_hi) return stage[bin - tb.f_lo];
    return a.spec0 ? a.spec0[(size_t)frame * a.n_stft + bin] : rand_unit(rbase, bin);
  };
  if ((a.out_stride & 3) == 0) {
    const int4* __restrict__ pb4 = reinterpret_cast<const int4*>(tb.pos_bin);
    float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
    for (int p4 = tid; p4 < (a.out_stride >> 2); p4 += nthr) {
      const int4 b = pb4[p4];
      out4[p4] = float4{value_at(b.x), value_at(b.y), value_at(b.z), value_at(b.w)};
    }
  } else {
    for (int p = tid; p < a.out_stride; p += nthr) out[p] = value_at(tb.pos_bin[p]);
  }
}

// Two things keep the per-bin cost of a step at five instructions for the long groups (seven in round 2):
//  * scaled state: spec, buf and the mel targets are held multiplied by kImelScale = 2^-60.  Every operation of the step
//    is linear except the clamp at zero, and a power-of-two factor commutes with fp32 rounding, so the scaled iteration is
//    the unscaled one bit for bit (as long as nothing leaves the normal range: values below 1.4e-20 in the reference's units
//    would, they sit 23+ orders of magnitude under a spectrogram's scale) - and `max(0, x)` becomes the VALU's free output
//    clamp to [0, 1] on the FMA that produces x (the upper bound is 1.15e18 in the reference's units);
//  * unit form (UF): between two filter centres the falling weight of filter g and the rising weight of filter g+1 sum to
//    one (torchaudio's melscale_fbanks, norm=None; checked to 1e-6 per bin at plan creation), so the gradient
//    d0 w0 + d1 w1 = d1 + (d0 - d1) w0: one FMA per bin less, and momentum folds into the first (`fma(mom, buf, d1)`).
//    The sums A and B keep both weights (a thread's unused register slots carry w0 = w1 = 0 and must stay out of them; their
//    spec values drift inside [0, 1] and touch nothing).  Unlike the power-of-two scaling above this is NOT bit-identical to
//    the two-weight form: the weights sum to one only to 1e-6 and the gradient is rounded differently; emulated on the CPU
//    against the oracle the two forms sit at the same distance (rel-L2 2.1e-7 both).
// Round 6: the exponent is per CLIP, chosen from the clip's largest mel amplitude (or the caller's magnitude_hint) by
// range_finish_kernel (rfx_range.hip) so that the largest target sits near 2^-35 whatever the units are - 2^-60 for the reference's
// default max_value = 30e6, as in rounds 2-5, and the same bits for ANY power of two (the scale commutes with rounding).  A fixed
// 2^-60 saturated silently above 1.15e18 and flushed below 1.4e-20 in the reference's units; now the supported range is the one
// include/rfx.h states ("Numeric range").
constexpr float kImelScale = 8.673617379884035e-19f;    // 2^-60: without a per-clip table (ImelArgs::clip_scale == nullptr)
constexpr float kImelUnscale = 1152921504606846976.0f;  // 2^60
// sets a.sc / a.un (scale into the state's units / back) for the frame's clip
__device__ __forceinline__ void imel_set_scale(ImelArgs& a, int clip) {
  a.sc = a.clip_scale ? a.clip_scale[2 * clip] : kImelScale;
  a.un = a.clip_scale ? a.clip_scale[2 * clip + 1] : kImelUnscale;
}

// Round 4: the per-bin state lives in register PAIRS (bins 2i and 2i+1 of the group) and every operation of the step is one
// v_pk_*_f32: a packed instruction does the work of two plain ones in one issue slot.  The arithmetic per bin is the plain
// form's, operation for operation: the group sums were already accumulated as even / odd partial sums, now the two halves of
// one accumulator.  A padding half (odd bin counts) carries w0 = w1 = 0 like every unused slot.  (The plain form it replaced:
// DESIGN_HISTORY.md, round 4.)
using c2 = float __attribute__((ext_vector_type(2)));
__device__ __forceinline__ c2 bc2(float x) { return c2{x, x}; }
// spec = clamp(spec + nl * buf, 0, 1): the output clamp of the packed FMA (the compiler does not fold it into v_pk_fma_f32: two
// v_max per pair); nl = -lr * gradient scale sits in both halves of an SGPR pair
__device__ __forceinline__ c2 pk_step_clamp(c2 spec, unsigned long long nl2, c2 buf) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 clamp" : "+v"(spec) : "s"(nl2), "v"(buf));
  return spec;
}
// x = clamp(x + v, 0, 1) / x = clamp(x + v m, 0, 1) for the line forms, whose step is a value per pair
__device__ __forceinline__ c2 pk_add_clamp(c2 x, c2 v) {
  asm("v_pk_add_f32 %0, %0, %1 clamp" : "+v"(x) : "v"(v));
  return x;
}
__device__ __forceinline__ c2 pk_fma_clamp(c2 x, c2 v, c2 m) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 clamp" : "+v"(x) : "v"(v), "v"(m));
  return x;
}

// A group in table form: spec, momentum buffer and both weights of every bin in registers.  Its four operations - load, the A / B
// sums, the step, the stage - have the signatures of the line-form group's (rfx_imel_groups.hip: LineGroup), so one kernel body
// serves either type; each uses the arguments it needs.
template <int N, bool UF>
struct GroupState {
  static constexpr int NP = (N + 1) / 2;
  static constexpr bool kUnitForm = UF, kLineForm = false;
  c2 spec[NP], buf[NP], w0[NP], w1[NP];
  int f0, n;  // first bin, bin count
};

// grp < 0: an absent group (no bins, every slot padding)
template <int N, bool UF>
__device__ __forceinline__ void group_load(GroupState<N, UF>& g, int grp, const ImelArgs& a, int frame, unsigned rbase) {
  const ImelTables& tb = a.tb;
  g.f0 = grp >= 0 ? tb.grp_start[grp] : 0;
  g.n = grp >= 0 ? tb.grp_start[grp + 1] - g.f0 : 0;
#pragma unroll
  for (int i = 0; i < 2 * g.NP; ++i) {
    const bool ok = i < g.n;
    const int f = g.f0 + (ok ? i : 0);
    const float w0 = ok ? tb.bin_w0[f] : 0.f, w1 = ok ? tb.bin_w1[f] : 0.f;
    const float sp = ok ? a.sc * (a.spec0 ? a.spec0[(size_t)frame * a.n_stft + f] : rand_unit(rbase, f)) : 0.f;
    if (i & 1) { g.w0[i >> 1].y = w0; g.w1[i >> 1].y = w1; g.spec[i >> 1].y = sp; g.buf[i >> 1].y = 0.f; }
    else       { g.w0[i >> 1].x = w0; g.w1[i >> 1].x = w1; g.spec[i >> 1].x = sp; g.buf[i >> 1].x = 0.f; }
  }
}
template <int N, bool UF>
__device__ __forceinline__ void group_ab(const GroupState<N, UF>& g, float& A, float& B) {
  c2 sa = bc2(0.f), sb = bc2(0.f);
#pragma unroll
  for (int i = 0; i < g.NP; ++i) {
    sa = __builtin_elementwise_fma(g.w0[i], g.spec[i], sa);
    sb = __builtin_elementwise_fma(g.w1[i], g.spec[i], sb);
  }
  A = sa.x + sa.y;
  B = sb.x + sb.y;
}
// d0, d1: the residuals of the group's two filters; nl = -lr * gradient scale, nl2 the same in both halves of an SGPR pair
template <int N, bool UF>
__device__ __forceinline__ void group_step(GroupState<N, UF>& g, float d0, float d1, float /*nl*/, unsigned long long nl2, float mom) {
  const c2 vm = bc2(mom), v0 = bc2(d0), v1 = bc2(d1), vd = bc2(d0 - d1);
#pragma unroll
  for (int i = 0; i < g.NP; ++i) {
    // torch.optim.SGD: buf.mul_(momentum).add_(grad); accumulating in place keeps buf in its register (a separate gradient
    // temporary costs a move per bin and step across the loop back-edge).  The first step's buf = grad needs no special case:
    // buf starts at +0 and momentum * 0 is +0
    c2 bnew;
    if (UF) {
      bnew = __builtin_elementwise_fma(vm, g.buf[i], v1);
      bnew = __builtin_elementwise_fma(vd, g.w0[i], bnew);
    } else {
      bnew = vm * g.buf[i];
      bnew = __builtin_elementwise_fma(v0, g.w0[i], bnew);
      bnew = __builtin_elementwise_fma(v1, g.w1[i], bnew);
    }
    g.buf[i] = bnew;
  }
#pragma unroll
  for (int i = 0; i < g.NP; ++i) g.spec[i] = pk_step_clamp(g.spec[i], nl2, g.buf[i]);
}
// the group's bins, unscaled, into the frame's LDS stage (bin order: entry f - f_lo)
template <int N, bool UF>
__device__ __forceinline__ void group_stage(const GroupState<N, UF>& g, int /*grp*/, const ImelTables& tb, float* stage, float unscale) {
#pragma unroll
  for (int i = 0; i < 2 * g.NP; ++i)
    if (i < g.n) stage[g.f0 + i - tb.f_lo] = unscale * ((i & 1) ? g.spec[i >> 1].y : g.spec[i >> 1].x);
}

}  // namespace rfx
