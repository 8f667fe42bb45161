// rfx_codec.hip - the two ends of the hot path on the device:
//   * uint8 spectrogram image <-> float mel amplitudes  (riffusion/util/image_util.py:13-110)
//   * float waveform -> peak-normalised int16 PCM       (riffusion/util/audio_util.py:22-28)
// All three are byte / integer exact by construction: the only transcendental in the chain
// (numpy's float32 power curve) is never evaluated on the device - the decoder gathers from a
// 256-entry table and the encoder searches 255 thresholds, both generated on the host by running
// numpy's own float32 chain over the finitely many cases.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_kernels.h"

namespace rfx {

// ---- decode: image_util.spectrogram_from_image (:81-108).  img (N, H, W, 3) uint8 RGB ->
// out (N*C, H, W) float32, C = 2 picks G,B (:89-91), C = 1 picks R (:92-93); rows flipped (:85);
// lut[p] = float32(((255 - p) / 255) ** (1/power) * max_value) as numpy computes it (:96-108).
// One workgroup per image row: the row's W pixels are contiguous (3 W bytes), the output rows (one per channel) are written in
// whole lines; no per-pixel index arithmetic (the first version unravelled a flat index with five 64-bit divisions per pixel:
// 0.22 ms per 64 tiles, a tenth of that now).
__global__ void __launch_bounds__(256) image_decode_kernel(const uint8_t* __restrict__ img, const float* __restrict__ lut,
                                                          float* __restrict__ out, int H, int W, int C) {
  __shared__ float lut_s[256];
  lut_s[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const size_t n = blockIdx.x / H;
  const int h = blockIdx.x - (int)n * H;  // output row; the image is stored top row = highest frequency (:85)
  const uint8_t* __restrict__ src = img + (n * H + (size_t)(H - 1 - h)) * W * 3;
  float* __restrict__ dst = out + (n * C * H + (size_t)h) * W;
  const size_t cstride = (size_t)H * W;
  for (int w = threadIdx.x; w < W; w += 256) {
    if (C == 2) {
      dst[w] = lut_s[src[3 * w + 1]];
      dst[cstride + w] = lut_s[src[3 * w + 2]];
    } else {
      dst[w] = lut_s[src[3 * w]];
    }
  }
}

// ---- per-clip maximum (of x or |x|) over `count` contiguous floats.  A clip is split over several
// workgroups (float4 loads); partial maxima meet in an atomicMax on an order-preserving integer key
// (positive NaN is the largest key, so np.max's NaN propagation comes for free), a last tiny kernel
// turns the keys back into floats in place.
// (max_key / key_value: rfx_kernels.h)
template <bool ABS>
__global__ void __launch_bounds__(256) clip_max_kernel(const float* __restrict__ x, unsigned* __restrict__ keys, size_t count, int splits) {
  __shared__ unsigned red[4];
  const int clip = blockIdx.x / splits, part = blockIdx.x - clip * splits;
  const size_t chunk = (((count + splits - 1) / splits) + 3) & ~(size_t)3;
  const size_t begin = (size_t)part * chunk, end = begin + chunk < count ? begin + chunk : count;
  const float* p = x + (size_t)clip * count;
  unsigned m = 0;  // key of the smallest value
  auto take = [&](float v) { m = max(m, max_key(ABS ? fabsf(v) : v)); };
  size_t i = begin;
  if ((reinterpret_cast<uintptr_t>(p + begin) & 15) == 0) {
    for (i = begin + 4 * (size_t)threadIdx.x; i + 3 < end; i += 4 * 256) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      take(v.x); take(v.y); take(v.z); take(v.w);
    }
    i = begin + ((end > begin ? end - begin : 0) & ~(size_t)3);  // scalar tail starts here
  }
  for (i += threadIdx.x; i < end; i += 256) take(p[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&keys[clip], max(max(red[0], red[1]), max(red[2], red[3])));
}
__global__ void clip_max_finish_kernel(unsigned* keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) reinterpret_cast<float*>(keys)[i] = key_value(keys[i]);
}

// ---- encode: image_util.image_from_spectrogram (:27-54).  mel (N*C, M, T) -> img (N, M, T, 3) uint8.
// q = uint8(255 - float32(pow(float32(x / max), power)) * 255): monotone non-increasing in the
// float32 ratio r = x / max, so q = number of thresholds thr[v] (v = 0..254, descending) with
// r < thr[v], where thr[v] is the smallest float32 r whose numpy result is <= v.
// One workgroup per image row (blockIdx.y = row h, blockIdx.z = clip n): no per-pixel 64-bit divisions; a thread takes four
// consecutive pixels: one 16-byte load per channel, twelve bytes of RGB out as three dwords (the first version divided a
// 64-bit pixel index three times per pixel and stored single bytes: 65 us per 64 tiles; now memory bound).
__global__ void __launch_bounds__(128) image_encode_kernel(const float* __restrict__ mel, const float* __restrict__ clip_max,
                                                          const float* __restrict__ thr, uint8_t* __restrict__ img, int M,
                                                          int T, int C) {
  __shared__ float thr_s[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) thr_s[i] = i < 255 ? thr[i] : -__builtin_inff();
  __syncthreads();
  const int h = blockIdx.y;  // image row (already flipped: row h shows mel bin M-1-h)
  const size_t n = blockIdx.z;
  const float mx = clip_max[n];
  auto quantise = [&](float x) {
    const float ratio = __fdiv_rn(x, mx);
    // thr_s is descending in v: find the count of v with ratio < thr[v]  (binary search, 8 steps)
    int lo = 0, hi = 255;  // answer in [0, 255]
#pragma unroll
    for (int step = 0; step < 8; ++step) {
      const int mid = (lo + hi) >> 1;
      if (ratio < thr_s[mid]) lo = mid + 1; else hi = mid;
    }
    return (unsigned)lo;
  };
  uint8_t* __restrict__ row_out = img + ((n * M + h) * (size_t)T) * 3;
  const bool aligned = (T & 3) == 0;  // rows of whole 16-byte groups: vector path
  for (int t0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x); t0 < T; t0 += 4 * gridDim.x * blockDim.x) {
    unsigned q[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const int npx = min(4, T - t0);
    for (int c = 0; c < C; ++c) {
      const float* __restrict__ src = mel + ((n * C + c) * M + (M - 1 - h)) * (size_t)T + t0;
      if (aligned) {
        const float4 v = *reinterpret_cast<const float4*>(src);
        q[c][0] = quantise(v.x); q[c][1] = quantise(v.y); q[c][2] = quantise(v.z); q[c][3] = quantise(v.w);
      } else {
        for (int p = 0; p < npx; ++p) q[c][p] = quantise(src[p]);
      }
    }
    unsigned char px[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (C == 1) { px[3 * p] = px[3 * p + 1] = px[3 * p + 2] = (unsigned char)q[0][p]; }
      else { px[3 * p] = 0; px[3 * p + 1] = (unsigned char)q[0][p]; px[3 * p + 2] = (unsigned char)q[1][p]; }
    }
    if (aligned) {  // 12 bytes = three dwords at a 4-byte aligned address (3 * t0 with t0 % 4 == 0, rows of 3 T bytes with T % 4 == 0)
      unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(row_out + 3 * (size_t)t0);
#pragma unroll
      for (int wd = 0; wd < 3; ++wd)
        dst[wd] = (unsigned)px[4 * wd] | ((unsigned)px[4 * wd + 1] << 8) | ((unsigned)px[4 * wd + 2] << 16) | ((unsigned)px[4 * wd + 3] << 24);
    } else {
      for (int b = 0; b < 3 * npx; ++b) row_out[3 * (size_t)t0 + b] = px[b];
    }
  }
}

// ---- encode from the forward kernels' frame-major scratch (rfx_image_from_waveform; round 5): mel_tm [N*C][T][Mpad] -> img
// (N, M, T, 3).  What rfx_image_encode_u8 does after a transpose to (N*C, M, T), without the transposed copy (134 MB written and
// read back per 64 tiles) and without a pass for the maximum (the forward kernel hands it over as a key).  A workgroup takes a tile
// of 128 frames x 32 mel bins per channel: whole 128-byte lines in (32 floats of a frame), transposed in LDS, and out as 384
// contiguous bytes per image row (twelve bytes per thread, whole lines).  Same quantiser as image_encode_kernel, bit for bit.
constexpr int kEncTmT = 128, kEncTmM = 32, kEncTmPitch = kEncTmT + 4;  // LDS row = one mel bin's 128 frames (+4: 16-byte reads stay aligned, rows shift banks)
__global__ void __launch_bounds__(256) image_encode_tm_kernel(const float* __restrict__ mel_tm, const unsigned* __restrict__ max_keys, int keys_per_image,
                                                             const float* __restrict__ clip_max_in, const float* __restrict__ thr,
                                                             uint8_t* __restrict__ img, float* __restrict__ clip_max_out, int M,
                                                             int Mpad, int T, int C) {
  __shared__ float thr_s[256];
  // C tiles of dynamic LDS (round 6: a static [2] kept a mono launch at four workgroups per CU for a tile it never touches)
  extern __shared__ __attribute__((aligned(16))) float tile_mem[];
  float (*tile)[kEncTmM][kEncTmPitch] = reinterpret_cast<float (*)[kEncTmM][kEncTmPitch]>(tile_mem);
  thr_s[threadIdx.x] = threadIdx.x < 255 ? thr[threadIdx.x] : -__builtin_inff();
  const int t0 = blockIdx.x * kEncTmT, m0 = blockIdx.y * kEncTmM;
  const size_t n = blockIdx.z;
  // the image's maximum: the largest of the keys the forward kernel's workgroups left for its rows (L2 hits), or a float
  __shared__ unsigned key_s[4];
  if (max_keys) {
    unsigned k = 0;
    for (int j = threadIdx.x; j < keys_per_image; j += 256) k = max(k, max_keys[n * keys_per_image + j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k = max(k, (unsigned)__shfl_xor((int)k, o));
    if ((threadIdx.x & 63) == 0) key_s[threadIdx.x >> 6] = k;
  }
  // in: thread (frame r of 32, quad of four mel bins): four passes over the tile's 128 frames
  {
    const int mq = 4 * (threadIdx.x & 7), r0 = threadIdx.x >> 3;
    for (int c = 0; c < C; ++c) {
      const float* __restrict__ src = mel_tm + ((n * C + c) * (size_t)T) * Mpad + m0 + mq;  // (m0 + mq + 3 < Mpad: Mpad % 64 == 0)
#pragma unroll
      for (int pass = 0; pass < kEncTmT / 32; ++pass) {
        const int r = r0 + 32 * pass, t = t0 + r;
        const float4 v = t < T ? *reinterpret_cast<const float4*>(src + (size_t)t * Mpad) : float4{0.f, 0.f, 0.f, 0.f};
        tile[c][mq][r] = v.x;
        tile[c][mq + 1][r] = v.y;
        tile[c][mq + 2][r] = v.z;
        tile[c][mq + 3][r] = v.w;
      }
    }
  }
  __syncthreads();
  const float mx = max_keys ? key_value(max(max(key_s[0], key_s[1]), max(key_s[2], key_s[3]))) : clip_max_in[n];
  if (clip_max_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) clip_max_out[n] = mx;
  // The level is the count of v with ratio < thr[v] (thr descending).  Rounds 1-5 found it with an eight-step binary search: eight
  // DEPENDENT LDS reads per pixel, which is what kept this kernel at half its byte bound.  Round 6: the table is a power curve
  // (image_util.py:32-38: level = 255 - 255 ratio^power), so the level is ESTIMATED with two transcendentals from an exponent
  // fitted to the table itself (no new argument: any table works), and four INDEPENDENT reads around the estimate settle it: the
  // thresholds remain the judge, bit for bit - if the window does not bracket the answer (never seen for the reference's
  // curves: the estimate is off by at most one level) the binary search runs.
  // thr[v] is the smallest ratio whose level is <= v: trunc(255 - 255 r^p) <= 128  <=>  r^p > 126 / 255, so p = log2(126 / 255) / log2(thr[128])
  // (with 127 / 255 - the first version - p came out 1.1 % low, one pixel in 200 fell outside the window and most WAVES ran the
  // search as well: 55 us instead of 48; tools/probe_encode.py)
  const float t128 = thr_s[128];
  const float pw = (t128 > 0.f && t128 < 1.f) ? __fdividef(-1.0170735f, __log2f(t128)) : 0.25f;
  auto quantise = [&](float x) {
    const float ratio = __fdiv_rn(x, mx);
    const float est = 255.f - 255.f * __builtin_amdgcn_exp2f(pw * __builtin_amdgcn_logf(ratio));  // v_log_f32 / v_exp_f32 (NaN for a negative or NaN ratio)
    int w = (int)est - 2;  // (a NaN converts to 0)
    w = w < 0 ? 0 : (w > 251 ? 251 : w);
    const bool c0 = ratio < thr_s[w], c1 = ratio < thr_s[w + 1], c2 = ratio < thr_s[w + 2], c3 = ratio < thr_s[w + 3];
    int lo = w + (int)c0 + (int)c1 + (int)c2 + (int)c3;
    if (!((c0 || w == 0) && (!c3 || w == 251))) {  // the window missed: the search of rounds 1-5
      int hi = 255;
      lo = 0;
#pragma unroll
      for (int step = 0; step < 8; ++step) {
        const int mid = (lo + hi) >> 1;
        if (ratio < thr_s[mid]) lo = mid + 1; else hi = mid;
      }
    }
    return (unsigned)lo;
  };
  // out: thread (mel bin of 8, four consecutive frames of the tile's 128): four passes over the tile's 32 mel bins
  const int tq = 4 * (threadIdx.x & 31), mr0 = threadIdx.x >> 5;
  const bool aligned = (T & 3) == 0;
#pragma unroll
  for (int pass = 0; pass < kEncTmM / 8; ++pass) {
    const int ml = mr0 + 8 * pass, m = m0 + ml, t = t0 + tq;
    if (m >= M || t >= T) continue;
    unsigned q[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int c = 0; c < C; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(&tile[c][ml][tq]);
      q[c][0] = quantise(v.x); q[c][1] = quantise(v.y); q[c][2] = quantise(v.z); q[c][3] = quantise(v.w);
    }
    unsigned char px[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (C == 1) { px[3 * p] = px[3 * p + 1] = px[3 * p + 2] = (unsigned char)q[0][p]; }
      else { px[3 * p] = 0; px[3 * p + 1] = (unsigned char)q[0][p]; px[3 * p + 2] = (unsigned char)q[1][p]; }
    }
    uint8_t* __restrict__ dst8 = img + ((n * M + (size_t)(M - 1 - m)) * T + t) * 3;  // image row h shows mel bin M - 1 - h
    if (aligned) {
      unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(dst8);
#pragma unroll
      for (int wd = 0; wd < 3; ++wd)
        dst[wd] = (unsigned)px[4 * wd] | ((unsigned)px[4 * wd + 1] << 8) | ((unsigned)px[4 * wd + 2] << 16) | ((unsigned)px[4 * wd + 3] << 24);
    } else {
      const int npx = min(4, T - t);
      for (int b = 0; b < 3 * npx; ++b) dst8[b] = px[b];
    }
  }
}

// ---- PCM tail: audio_util.audio_from_waveform (:22-28).  wave (N*C, L) float32 -> pcm (N, L, C) int16,
// samples * float32(32767 / max|clip|) truncated toward zero.
__global__ void __launch_bounds__(256) pcm16_kernel(const float* __restrict__ wave, const float* __restrict__ clip_peak,
                                                   int16_t* __restrict__ pcm, int L, int C, int normalize, size_t total) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // index over (N, L, C)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int c = (int)(i % C);
    const size_t r = i / C;
    const int l = (int)(r % L);
    const size_t n = r / L;
    float v = wave[(n * C + c) * L + l];
    if (normalize) {
      // numpy 1.x computes python-int / float32-scalar in float64 and then multiplies the float32
      // array by that scalar cast to float32
      const float scale = (float)(32767.0 / (double)clip_peak[n]);
      v = v * scale;
    }
    pcm[i] = (int16_t)(int)v;  // astype(np.int16): truncation toward zero
  }
}

static int grid_for(size_t total) {
  size_t b = (total + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b ? b : 1));
}

hipError_t launch_image_decode(const uint8_t* img, const float* lut, float* out, int N, int H, int W, int C, hipStream_t s) {
  // a dispatch holds fewer than 2^32 work-items per dimension: 256 x N x H reaches that at 32 768 images of 512 rows, where the
  // launch reports no error but the later images are never decoded - launch at most 65535 x 256 rows at a time
  const int per = H >= 65535 * 256 ? 1 : 65535 * 256 / H;
  for (int n0 = 0; n0 < N; n0 += per) {
    const int n = N - n0 < per ? N - n0 : per;
    hipLaunchKernelGGL(image_decode_kernel, dim3((unsigned)((size_t)n * H)), dim3(256), 0, s, img + (size_t)n0 * H * W * 3, lut,
                       out + (size_t)n0 * C * H * W, H, W, C);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t launch_clip_max(const float* x, float* out, int nclips, size_t count, bool abs_value, hipStream_t s) {
  unsigned* keys = reinterpret_cast<unsigned*>(out);
  hipError_t e = hipMemsetAsync(keys, 0, sizeof(unsigned) * nclips, s);
  if (e != hipSuccess) return e;
  // ~16 K floats per workgroup, at most 64 workgroups per clip
  int splits = (int)((count + 16383) / 16384);
  splits = splits < 1 ? 1 : (splits > 64 ? 64 : splits);
  if (abs_value) hipLaunchKernelGGL(clip_max_kernel<true>, dim3(nclips * splits), dim3(256), 0, s, x, keys, count, splits);
  else hipLaunchKernelGGL(clip_max_kernel<false>, dim3(nclips * splits), dim3(256), 0, s, x, keys, count, splits);
  hipLaunchKernelGGL(clip_max_finish_kernel, dim3((nclips + 255) / 256), dim3(256), 0, s, keys, nclips);
  return hipGetLastError();
}
hipError_t launch_image_encode(const float* mel, const float* clip_max, const float* thr, uint8_t* img, int N, int M, int T,
                               int C, hipStream_t s) {
  const int bx = (T + 4 * 128 - 1) / (4 * 128);
  hipLaunchKernelGGL(image_encode_kernel, dim3(bx < 1 ? 1 : bx, M, N), dim3(128), 0, s, mel, clip_max, thr, img, M, T, C);
  return hipGetLastError();
}
hipError_t launch_image_encode_tm(const float* mel_tm, const unsigned* max_keys, int keys_per_image, const float* clip_max_in, const float* thr,
                                  uint8_t* img, float* clip_max_out, int N, int M, int Mpad, int T, int C, hipStream_t s) {
  hipLaunchKernelGGL(image_encode_tm_kernel, dim3((T + kEncTmT - 1) / kEncTmT, (M + kEncTmM - 1) / kEncTmM, N), dim3(256),
                     sizeof(float) * (size_t)C * kEncTmM * kEncTmPitch, s, mel_tm, max_keys, keys_per_image, clip_max_in, thr, img, clip_max_out, M, Mpad, T, C);
  return hipGetLastError();
}
hipError_t launch_pcm16(const float* wave, const float* clip_peak, int16_t* pcm, int N, int L, int C, int normalize, hipStream_t s) {
  const size_t total = (size_t)N * L * C;
  hipLaunchKernelGGL(pcm16_kernel, dim3(grid_for(total)), dim3(256), 0, s, wave, clip_peak, pcm, L, C, normalize, total);
  return hipGetLastError();
}

}  // namespace rfx
