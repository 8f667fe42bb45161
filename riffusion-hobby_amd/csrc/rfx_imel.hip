// rfx_imel.hip - InverseMelScale on gfx950 (replaces torchaudio 0.13 transforms.InverseMelScale as
// constructed at riffusion/spectrogram_converter.py:87-99 and called at :201).
//
// The reference minimises  mean_{c,t} sum_m (mel - spec @ fb)^2  with torch.optim.SGD(lr 0.1,
// momentum 0.9) from a uniform random start, clamping at zero after every step, for max_iter steps
// (an early exit on the clip loss practically never fires at spectrogram scales).  Frames only
// interact through the 1/(C*T) factor of the mean and through that early exit, and the HTK
// filterbank is banded (<= 2 adjacent mel filters per linear bin), so each frame's whole
// optimisation runs inside one workgroup with all state on chip:
//   phase A  (thread per mel)   pred_m = sum_{f in band(m)} w * spec_f      spec, w in LDS
//                               diff_m = mel_m - pred_m                     -> LDS, sum diff^2 -> history
//   phase B  (thread per bin)   g = -(2/(C*T)) (diff_m0 w0 + diff_m0+1 w1); buf = mom*buf + g;
//                               spec = max(0, spec - lr*buf)                spec, buf, w in registers
// Bins whose filterbank row is zero never move: they pass their initial value through, exactly like
// the reference.  The per-frame loss history lets a follow-up scan reproduce the reference's early
// exit (it_stop per clip) and a fix-up launch re-runs the affected clips with that step count.
//
// This unit holds the general kernel (phases A and B as above, any banded bank), the early-stop scan and the choice between the
// kernel families; the faster formulations of the same iteration live in rfx_imel_groups.hip (one workgroup per frame, a thread
// owns whole groups of bins) and rfx_imel_wave.hip (one wave per frame), their shared device helpers in rfx_imel.hip.h.
#include <hip/hip_runtime.h>

#include "rfx_imel.hip.h"

namespace rfx {

// General kernel: any banded filterbank, spec and the weights in LDS (the fast families: rfx_imel_groups.hip, rfx_imel_wave.hip)
template <int BPT>  // bins per thread
__global__ void __launch_bounds__(kImelThreads) imel_kernel(ImelArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ImelTables& tb = a.tb;
  const int nb = tb.f_hi - tb.f_lo;
  float* spec_s = reinterpret_cast<float*>(smem);            // [nb]
  float* w_s = spec_s + ((nb + 3) & ~3);                     // [nnz]
  float* diff_s = w_s + ((tb.nnz + 3) & ~3);                 // [M + 1] (one pad entry for m0+1 == M)
  float* red_s = diff_s + ((a.M + 1 + 3) & ~3);              // [4] wave partials of sum diff^2
  float* hist_s = red_s + 4;                                 // [max_iter]

  const int frame = blockIdx.x;  // = b*T + t
  const int b = frame / a.T, t = frame - b * a.T;
  const int clip = b / a.C;
  const int tid = threadIdx.x;
  const int steps = a.it_limit ? a.it_limit[clip] : a.max_iter;
  if (a.it_limit && steps >= a.max_iter) return;  // fix-up pass: this clip never stopped early
  const int n_stft = a.n_stft;

  for (int i = tid; i < tb.nnz; i += kImelThreads) w_s[i] = tb.csr_w[i];
  if (tid == 0) diff_s[a.M] = 0.f;

  // ---- phase-B ownership: bins f = f_lo + tid + 256*j
  float spec[BPT], buf[BPT], w0[BPT], w1[BPT];
  int m0[BPT];
  const unsigned rbase = rand_frame_key(a.seed, a.frame_base + (unsigned long long)frame);
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const int f = tb.f_lo + tid + kImelThreads * j;
    const bool ok = f < tb.f_hi;
    m0[j] = ok ? tb.bin_m0[f] : -1;
    w0[j] = ok ? tb.bin_w0[f] : 0.f;
    w1[j] = ok ? tb.bin_w1[f] : 0.f;
    spec[j] = ok ? (a.spec0 ? a.spec0[(size_t)frame * n_stft + f] : rand_unit(rbase, f)) : 0.f;
    buf[j] = 0.f;
    if (m0[j] < 0) { m0[j] = a.M; w0[j] = 0.f; w1[j] = 0.f; }  // a zero row inside the range: reads the pad, never moves
    if (ok) spec_s[f - tb.f_lo] = spec[j];
  }
  // ---- phase-A ownership: even r counts mels up from 0, odd r counts down from M-1, so every
  // thread pairs a short low-frequency band with a long high-frequency one
  constexpr int kMaxMelPerThread = 4;  // M <= 1024
  const int n_rounds = (a.M + kImelThreads - 1) / kImelThreads;
  const int up_bound = min(a.M, kImelThreads * ((n_rounds + 1) / 2));
  float melv[kMaxMelPerThread];
  int mlist[kMaxMelPerThread], pbeg[kMaxMelPerThread], pend[kMaxMelPerThread], soff[kMaxMelPerThread];
#pragma unroll
  for (int r = 0; r < kMaxMelPerThread; ++r) {
    int m = -1;
    if (r < n_rounds) {
      if ((r & 1) == 0) {
        m = (r / 2) * kImelThreads + tid;
        if (m >= up_bound) m = -1;
      } else {
        m = a.M - 1 - (r / 2) * kImelThreads - tid;
        if (m < up_bound) m = -1;
      }
    }
    mlist[r] = m;
    melv[r] = m >= 0 ? a.mel[((size_t)b * a.M + m) * a.T + t] : 0.f;
    pbeg[r] = m >= 0 ? tb.csr_ptr[m] : 0;
    pend[r] = m >= 0 ? tb.csr_ptr[m + 1] : 0;
    soff[r] = m >= 0 ? (tb.band_lo[m] - tb.f_lo) - pbeg[r] : 0;  // spec_s[soff + p] pairs with w_s[p]
  }
  const float gscale = -2.0f / (float)(a.C * a.T);
  __syncthreads();

  for (int it = 0; it < steps; ++it) {
    // ---- phase A
    float sq = 0.f;
#pragma unroll
    for (int r = 0; r < kMaxMelPerThread; ++r) {
      const int m = mlist[r];
      if (m < 0) continue;
      const int p1 = pend[r];
      const float* sp = spec_s + soff[r];
      // eight LDS pairs in flight per trip (the band length varies per mel: clamp + zero weight)
      float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
      for (int p = pbeg[r]; p < p1; p += 8) {
        float w[8], sv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int q = min(p + i, p1 - 1);
          w[i] = (p + i < p1) ? w_s[q] : 0.f;
          sv[i] = sp[q];
        }
        acc0 = fmaf(w[0], sv[0], acc0); acc1 = fmaf(w[1], sv[1], acc1);
        acc2 = fmaf(w[2], sv[2], acc2); acc3 = fmaf(w[3], sv[3], acc3);
        acc0 = fmaf(w[4], sv[4], acc0); acc1 = fmaf(w[5], sv[5], acc1);
        acc2 = fmaf(w[6], sv[6], acc2); acc3 = fmaf(w[7], sv[7], acc3);
      }
      const float acc = (acc0 + acc1) + (acc2 + acc3);
      const float d = melv[r] - acc;
      diff_s[m] = d;
      sq = fmaf(d, d, sq);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if ((tid & 63) == 0) red_s[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) hist_s[it] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    // ---- phase B
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const float g = gscale * fmaf(diff_s[m0[j]], w0[j], diff_s[min(m0[j] + 1, a.M)] * w1[j]);
      buf[j] = (it == 0) ? g : fmaf(a.momentum, buf[j], g);
      spec[j] = fmaxf(0.f, fmaf(-a.lr, buf[j], spec[j]));
      const int f = tb.f_lo + tid + kImelThreads * j;
      if (f < tb.f_hi) spec_s[f - tb.f_lo] = spec[j];
    }
    __syncthreads();
  }

  // ---- results: moved bins from registers, untouched bins straight from the init
  float* out = a.out_slots + (size_t)frame * a.out_stride;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const int f = tb.f_lo + tid + kImelThreads * j;
    if (f < tb.f_hi) {
      out[tb.bin_pos[f]] = spec[j];
      const int p2 = tb.bin_pos2[f];
      if (p2 >= 0) out[p2] = spec[j];
    }
  }
  for (int f = tid; f < n_stft; f += kImelThreads) {
    if (f >= tb.f_lo && f < tb.f_hi) continue;
    const float v = a.spec0 ? a.spec0[(size_t)frame * n_stft + f] : rand_unit(rbase, f);
    out[tb.bin_pos[f]] = v;
    const int p2 = tb.bin_pos2[f];
    if (p2 >= 0) out[p2] = v;
  }
  // padding positions are zeroed so that later consumers never see garbage
  if (a.plain) {
    for (int p = n_stft + tid; p < a.out_stride; p += kImelThreads) out[p] = 0.f;
  } else {
    for (int p = tid; p < kFrameStride; p += kImelThreads) {
      int q, kb;
      if (!pos_f_to_slot(p, q, kb)) out[p] = 0.f;
    }
  }
  if (a.loss_hist && !a.it_limit)
    for (int i = tid; i < a.max_iter; i += kImelThreads) a.loss_hist[(size_t)frame * a.max_iter + i] = i < steps ? hist_s[i] : 0.f;
}

// one workgroup per clip: replays the reference's stopping rule on the clip-mean loss.  Thread (g, i) sums
// iteration i over every fourth frame (loads coalesce across i), the four partial sums meet in LDS, then one
// thread walks the max_iter means.
__global__ void __launch_bounds__(1024) imel_scan_kernel(const float* __restrict__ loss_hist, int* __restrict__ it_stop,
                                                        int* __restrict__ any_early, int nclips, int C, int T, int max_iter,
                                                        float tol_loss, float tol_change) {
  extern __shared__ float scan_smem[];  // [4][256] partial sums, then [max_iter] means
  float* part = scan_smem;
  float* mean = scan_smem + 1024;
  const int clip = blockIdx.x;
  if (clip >= nclips) return;
  const int nframes = C * T;
  const int i = threadIdx.x & 255, g = threadIdx.x >> 8;
  const float* base = loss_hist + (size_t)clip * nframes * max_iter;
  for (int it0 = 0; it0 < max_iter; it0 += 256) {
    const int it = it0 + i;
    float s0 = 0.f, s1 = 0.f;
    if (it < max_iter) {
      int f = g;
      for (; f + 4 < nframes; f += 8) {
        s0 += base[(size_t)f * max_iter + it];
        s1 += base[(size_t)(f + 4) * max_iter + it];
      }
      if (f < nframes) s0 += base[(size_t)f * max_iter + it];
    }
    part[g * 256 + i] = s0 + s1;
    __syncthreads();
    if (g == 0 && it < max_iter) mean[it] = ((part[i] + part[256 + i]) + (part[512 + i] + part[768 + i])) / (float)nframes;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float prev = __builtin_inff();
    int stop = max_iter;
    for (int it = 0; it < max_iter; ++it) {
      const float loss = mean[it];
      if (loss < tol_loss || fabsf(prev - loss) < tol_change) { stop = it + 1; break; }
      prev = loss;
    }
    it_stop[clip] = stop;
    if (stop < max_iter) atomicExch(any_early, 1);
  }
}

// Which kernel launch_imel runs for a bank / variant / step count (ImelKernel).  ONE place decides (round 6): the launcher below,
// rfx_plan_imel_kernel and imel_can_emit_fam_slots all ask here, so a bank whose frame does not fit the 64 KB of LDS a kernel gets
// without the opt-in attribute falls back to the general kernel everywhere at once.
ImelKernel imel_kernel_choice(const ImelTables& tb, int M, int max_iter, ImelVariant variant) {
  const int band = tb.f_hi - tb.f_lo;
  constexpr size_t kPlainLds = 64 * 1024;  // dynamic LDS a kernel may ask for without hipFuncAttributeMaxDynamicSharedMemorySize
  const bool frame_fits = imel_frame_lds_bytes(M, max_iter, band) <= kPlainLds;
  if (variant == kImelVariantBest) {
    if (tb.wave_ok && imel_wave_lds_bytes(max_iter, band) <= kPlainLds) return kImelKernelWave;
    if (tb.fast_ok != kImelKernelGeneral && frame_fits) return (ImelKernel)tb.fast_ok;
  } else if (variant == kImelVariantUniform) {
    // (the default set's banks fit the uniform budget too; the wide and line sets have no uniform fallback)
    if ((tb.fast_ok == kImelKernelUniform || tb.fast_ok == kImelKernelPerWave) && frame_fits) return kImelKernelUniform;
  }
  return kImelKernelGeneral;
}

hipError_t launch_imel(const ImelArgs& a, ImelVariant variant, hipStream_t stream) {
  const ImelKernel kernel = imel_kernel_choice(a.tb, a.M, a.max_iter, variant);
  if (kernel == kImelKernelWave) return launch_imel_wave(a, stream);
  if (kernel != kImelKernelGeneral) return launch_imel_groups(a, kernel, stream);
  const int nb = a.tb.f_hi - a.tb.f_lo;
  const size_t lds = sizeof(float) * (((nb + 3) & ~3) + ((a.tb.nnz + 3) & ~3) + ((a.M + 1 + 3) & ~3) + 4 + a.max_iter);
  const int bpt = (nb + kImelThreads - 1) / kImelThreads;
  if (bpt <= 16) {
    (void)hipFuncSetAttribute((const void*)imel_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(imel_kernel<16>, dim3(a.B * a.T), dim3(kImelThreads), lds, stream, a);
  } else {
    (void)hipFuncSetAttribute((const void*)imel_kernel<36>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(imel_kernel<36>, dim3(a.B * a.T), dim3(kImelThreads), lds, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_imel_scan(const float* loss_hist, int* it_stop, int* any_early, int nclips, int C, int T, int max_iter,
                            float tol_loss, float tol_change, hipStream_t stream) {
  hipLaunchKernelGGL(imel_scan_kernel, dim3(nclips), dim3(1024), sizeof(float) * (1024 + (size_t)max_iter), stream, loss_hist, it_stop, any_early, nclips, C, T,
                     max_iter, tol_loss, tol_change);
  return hipGetLastError();
}

}  // namespace rfx
