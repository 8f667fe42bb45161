// rfx_api_codec.hip - the C ABI of librfx.so (include/rfx.h), the entry points that take no plan: image decode / encode, int16 PCM,
// its filters, compressor and stitch, the image resize, the JPEG scan and its decode, the PNG stream and its decode, and the int16 front end of the encode (resample, channel
// mix, clip gather).  They run on the device that owns their output buffer.
#include "rfx_api.h"
#include "rfx_compress_core.h"
#include "rfx_jpeg_core.h"
#include "rfx_jpeg_dec_core.h"
#include "rfx_pcm_core.h"
#include "rfx_pcm_in_core.h"
#include "rfx_png_core.h"
#include "rfx_png_dec_core.h"
#include "rfx_resize_core.h"

using namespace rfx;

// device that owns a caller buffer (the entry points that take no plan; declared in rfx_api.h)
int rfx::device_of(const void* d_ptr, int* device) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, d_ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(RFX_ERR_INVALID, std::string("not a device pointer: ") + hipGetErrorString(e));
  }
  *device = attr.device;
  return RFX_OK;
}

int rfx_image_decode_u8(const uint8_t* d_img, int N, int H, int W, int stereo, const float* d_lut256, float* d_mel_out,
                        void* stream) {
  if (!d_img || !d_lut256 || !d_mel_out || N <= 0 || H <= 0 || W <= 0) return fail(RFX_ERR_INVALID, "rfx_image_decode_u8: bad argument");
  int dev;
  if (int rc = device_of(d_mel_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_image_decode(d_img, d_lut256, d_mel_out, N, H, W, stereo ? 2 : 1, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_image_encode_u8(const float* d_mel, int N, int M, int T, int stereo, const float* d_thresholds255, float* d_clip_max,
                        uint8_t* d_img_out, void* stream) {
  if (!d_mel || !d_thresholds255 || !d_clip_max || !d_img_out || N <= 0 || M <= 0 || T <= 0)
    return fail(RFX_ERR_INVALID, "rfx_image_encode_u8: bad argument");
  int dev;
  if (int rc = device_of(d_img_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  const int C = stereo ? 2 : 1;
  RFX_HIP(launch_clip_max(d_mel, d_clip_max, N, (size_t)C * M * T, false, (hipStream_t)stream));
  RFX_HIP(launch_image_encode(d_mel, d_clip_max, d_thresholds255, d_img_out, N, M, T, C, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_pcm16(const float* d_wave, int N, int C, int L, int normalize, float* d_clip_peak, int16_t* d_pcm_out, void* stream) {
  if (!d_wave || !d_clip_peak || !d_pcm_out || N <= 0 || C <= 0 || L <= 0) return fail(RFX_ERR_INVALID, "rfx_pcm16: bad argument");
  int dev;
  if (int rc = device_of(d_pcm_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  if (normalize) RFX_HIP(launch_clip_max(d_wave, d_clip_peak, N, (size_t)C * L, true, (hipStream_t)stream));
  RFX_HIP(launch_pcm16(d_wave, d_clip_peak, d_pcm_out, N, L, C, normalize, (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_pcm16_filters_workspace_bytes(int N, int L, int C) {
  if (N <= 0 || L <= 0 || C <= 0) return 0;
  return pcm_filters_workspace_bytes(N, L, C);
}

int rfx_pcm16_apply_filters(const int16_t* d_pcm_in, int N, int L, int C, const double* d_gain_by_rms, const double* d_boost_by_peak,
                            int16_t* d_pcm_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_pcm_in || !d_gain_by_rms || !d_boost_by_peak || !d_pcm_out || !d_workspace || N <= 0 || L <= 0 || C <= 0)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters: bad argument");
  if ((int64_t)L * C >= ((int64_t)1 << 23))
    return fail(RFX_ERR_UNSUPPORTED, "rfx_pcm16_apply_filters: L * C >= 2^23 (audioop.rms is exact only below that)");
  if (workspace_bytes < pcm_filters_workspace_bytes(N, L, C)) return fail(RFX_ERR_WORKSPACE, "rfx_pcm16_apply_filters: workspace too small");
  int dev;
  if (int rc = device_of(d_pcm_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_pcm_filters(d_pcm_in, N, L, C, d_gain_by_rms, d_boost_by_peak, d_pcm_out, d_workspace, (hipStream_t)stream));
  return RFX_OK;
}

int rfx_pcm16_stitch(const int16_t* d_pcm, int N, int L, int C, const rfx_stitch_piece* h_pieces, const rfx_stitch_piece* d_pieces,
                     int n_pieces, int64_t out_frames, int16_t* d_out, void* stream) {
  static_assert(sizeof(rfx_stitch_piece) == sizeof(PcmPiece), "rfx_stitch_piece is PcmPiece (rfx_pcm_core.h)");
  if (!d_pcm || !h_pieces || !d_pieces || !d_out || N <= 0 || L <= 0 || C <= 0 || n_pieces <= 0 || out_frames <= 0)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_stitch: bad argument");
  // every read the kernel will make stays inside the batch: checked here, on the host table
  if (h_pieces[0].out_start != 0) return fail(RFX_ERR_INVALID, "rfx_pcm16_stitch: the first piece must start at frame 0");
  for (int k = 0; k < n_pieces; ++k) {
    const rfx_stitch_piece& p = h_pieces[k];
    const int64_t next = k + 1 < n_pieces ? h_pieces[k + 1].out_start : out_frames;
    const int64_t count = next - p.out_start;
    bool ok = count > 0 && (p.kind == 0 || p.kind == 1);
    ok = ok && (p.a_clip < 0 || (p.a_clip < N && p.a_off >= 0 && p.a_off + count <= L));
    ok = ok && (p.kind == 0 || p.b_clip < 0 || (p.b_clip < N && p.b_off >= 0 && p.b_off + count <= L));
    if (!ok) return fail(RFX_ERR_INVALID, "rfx_pcm16_stitch: piece " + std::to_string(k) + " is empty or reads outside the batch");
  }
  int dev;
  if (int rc = device_of(d_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_pcm_stitch(d_pcm, L, C, d_pieces, n_pieces, out_frames, d_out, (hipStream_t)stream));
  return RFX_OK;
}

static bool resize_args_ok(int N, int H, int W, int out_h, int out_w, int filter) {
  const auto in_range = [](int v) { return v >= 1 && v <= kRszMaxSize; };
  return N >= 1 && in_range(H) && in_range(W) && in_range(out_h) && in_range(out_w) && rsz_support(filter) > 0.0;
}

int rfx_image_resize_coefficients(int in_size, int out_size, int filter, int32_t* h_bounds, int32_t* h_kk, int capacity) {
  if (in_size < 1 || in_size > kRszMaxSize || out_size < 1 || out_size > kRszMaxSize || rsz_support(filter) == 0.0)
    return fail(RFX_ERR_INVALID, "rfx_image_resize_coefficients: sizes must be in [1, 16384] and the filter RFX_RESIZE_LANCZOS, "
                                 "_BILINEAR or _BICUBIC");
  const int ksize = rsz_ksize(in_size, out_size, filter);
  if (!h_bounds && !h_kk) return ksize;
  if (!h_bounds || !h_kk) return fail(RFX_ERR_INVALID, "rfx_image_resize_coefficients: h_bounds and h_kk go together");
  if ((int64_t)capacity < (int64_t)out_size * ksize)
    return fail(RFX_ERR_WORKSPACE, "rfx_image_resize_coefficients: h_kk holds fewer than out_size * ksize entries");
  std::vector<double> w(ksize);
  return rsz_coefficients(in_size, out_size, filter, h_bounds, h_kk, w.data());
}

size_t rfx_image_resize_workspace_bytes(int N, int H, int W, int out_h, int out_w, int filter) {
  if (!resize_args_ok(N, H, W, out_h, out_w, filter)) return 0;
  return resize_workspace_bytes(N, H, W, out_h, out_w);
}

int rfx_image_resize_u8(const uint8_t* d_in, int N, int H, int W, int out_h, int out_w, int filter, const int32_t* d_bounds_x,
                        const int32_t* d_kk_x, const int32_t* d_bounds_y, const int32_t* d_kk_y, uint8_t* d_out, void* d_workspace,
                        size_t workspace_bytes, void* stream) {
  if (!d_in || !d_out || !resize_args_ok(N, H, W, out_h, out_w, filter))
    return fail(RFX_ERR_INVALID, "rfx_image_resize_u8: bad argument (N >= 1, sizes in [1, 16384], filter RFX_RESIZE_LANCZOS, "
                                 "_BILINEAR or _BICUBIC)");
  if (out_w != W && (!d_bounds_x || !d_kk_x)) return fail(RFX_ERR_INVALID, "rfx_image_resize_u8: the width changes: need d_bounds_x, d_kk_x");
  if (out_h != H && (!d_bounds_y || !d_kk_y)) return fail(RFX_ERR_INVALID, "rfx_image_resize_u8: the height changes: need d_bounds_y, d_kk_y");
  const size_t need = resize_workspace_bytes(N, H, W, out_h, out_w);
  if (need && (!d_workspace || workspace_bytes < need)) return fail(RFX_ERR_WORKSPACE, "rfx_image_resize_u8: workspace too small");
  int dev;
  if (int rc = device_of(d_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_resize(d_in, N, H, W, out_h, out_w, d_bounds_x, d_kk_x, rsz_ksize(W, out_w, filter), d_bounds_y, d_kk_y,
                        rsz_ksize(H, out_h, filter), d_out, d_workspace, (hipStream_t)stream));
  return RFX_OK;
}

// ---- what the four file-codec entries share ---------------------------------------------------------------------------------------
static_assert(kJpgMaxSize == kPngMaxSize && kPngMaxSize == kPngdMaxSize, "axis_ok checks the codecs' one per-axis limit");
static bool axis_ok(int H, int W) { return H >= 1 && W >= 1 && H <= kJpgMaxSize && W <= kJpgMaxSize; }
static int refuse_size(const char* who, int H, int W, bool jpeg) {
  return fail(RFX_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(H) + " x " + std::to_string(W) + " (H x W): " +
                                       (jpeg ? "a JPEG holds at most 65535 rows and columns" : "this entry takes at most 65535 rows and columns"));
}
// the host copy of a decode's N + 1 offsets (`what`: "scan" or "stream"): there, not negative, not decreasing, no image longer than
// max_bytes (2^28 - 64 for both decoders); *longest, when asked for, receives the longest image's bytes
static int check_stream_offsets(const char* who, const char* what, const int64_t* h_offsets, int N, int64_t max_bytes, int64_t* longest) {
  const std::string w(who), noun(what);
  if (!h_offsets) return fail(RFX_ERR_INVALID, w + ": h_" + noun + "_offsets is NULL");
  if (h_offsets[0] < 0) return fail(RFX_ERR_INVALID, w + ": the first " + noun + " offset is negative");
  int64_t most = 0;
  for (int n = 0; n < N; ++n) {
    const int64_t bytes = h_offsets[n + 1] - h_offsets[n];
    if (bytes < 0) return fail(RFX_ERR_INVALID, w + ": " + noun + " offsets must not decrease (image " + std::to_string(n) + ")");
    if (bytes > max_bytes)
      return fail(RFX_ERR_UNSUPPORTED, w + ": the " + noun + " of image " + std::to_string(n) + " is longer than 2^28 - 64 bytes");
    most = bytes > most ? bytes : most;
  }
  if (longest) *longest = most;
  return RFX_OK;
}

// ---- JPEG scan (rfx_jpeg.hip) ----------------------------------------------------------------------------------------------------
int rfx_jpeg_quant_tables(int quality, uint16_t* h_luma64, uint16_t* h_chroma64) {
  if (!h_luma64 || !h_chroma64) return fail(RFX_ERR_INVALID, "rfx_jpeg_quant_tables: null pointer");
  if (quality < 1 || quality > 100)
    return fail(RFX_ERR_UNSUPPORTED, "rfx_jpeg_quant_tables: quality " + std::to_string(quality) + " is outside 1 .. 100");
  jpg_quant_tables(quality, h_luma64, h_chroma64);
  return RFX_OK;
}

// what keeps an encode inside its index types: the scan's length is an int32, and the kernels take one thread per block / per
// 16-byte chunk, 256 to a workgroup, at most 2^31 - 1 workgroups
static const char* jpeg_batch_limit(int N, int H, int W) {
  const JpgGeom g = jpg_geom(H, W);
  if (jpg_scan_capacity(g) > (uint64_t)INT32_MAX) return "one image's scan capacity does not fit the int32 of d_scan_bytes";
  const uint64_t per_launch = (uint64_t)INT32_MAX * 256;
  const uint64_t chunks = (jpg_unstuffed_capacity(g) + 31) / 16;
  if ((uint64_t)N * (uint64_t)g.blocks > per_launch || (uint64_t)N * chunks > per_launch) return "more blocks than one launch takes; encode in pieces";
  return nullptr;
}

size_t rfx_jpeg_scan_capacity(int H, int W) { return axis_ok(H, W) ? (size_t)jpg_scan_capacity(jpg_geom(H, W)) : 0; }

size_t rfx_jpeg_encode_workspace_bytes(int N, int H, int W) {
  if (N < 1 || !axis_ok(H, W) || jpeg_batch_limit(N, H, W)) return 0;
  return jpeg_workspace_layout(N, H, W).total;
}

int rfx_jpeg_encode_u8(const uint8_t* d_rgb, int N, int H, int W, const uint16_t* d_qtables, uint8_t* d_scan, int32_t* d_scan_bytes,
                       void* d_workspace, void* stream) {
  if (N < 1 || H < 1 || W < 1) return fail(RFX_ERR_INVALID, "rfx_jpeg_encode_u8: N, H and W must be positive");
  if (!axis_ok(H, W)) return refuse_size("rfx_jpeg_encode_u8", H, W, true);
  if (const char* why = jpeg_batch_limit(N, H, W)) return fail(RFX_ERR_UNSUPPORTED, std::string("rfx_jpeg_encode_u8: ") + why);
  if (!d_rgb || !d_qtables || !d_scan || !d_scan_bytes || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_jpeg_encode_u8: null pointer");
  int dev;
  if (int rc = device_of(d_scan, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_jpeg_encode(d_rgb, N, H, W, d_qtables, d_scan, (size_t)jpg_scan_capacity(jpg_geom(H, W)), d_scan_bytes, d_workspace,
                             (hipStream_t)stream));
  return RFX_OK;
}

// ---- PNG stream (rfx_png.hip) -------------------------------------------------------------------------------------------------------
// what keeps an encode inside its index types: the stream's length is an int32, and the kernels take one workgroup per row and
// one thread per 256-byte piece of the stream, 256 to a workgroup, at most 2^31 - 1 workgroups
static const char* png_batch_limit(int N, int H, int W) {
  const uint64_t cap = png_stream_capacity(png_geom(H, W, 3));
  if (cap > (uint64_t)INT32_MAX) return "one tile's stream capacity does not fit the int32 of d_stream_bytes";
  if ((uint64_t)N * (uint64_t)H > (uint64_t)INT32_MAX || (uint64_t)N * ((cap + 255) / 256 + 256) > (uint64_t)INT32_MAX)
    return "more rows or stream pieces than one launch takes; encode in pieces";
  return nullptr;
}

size_t rfx_png_stream_capacity(int H, int W, int channels) {
  if (!axis_ok(H, W) || (channels != 1 && channels != 3)) return 0;
  return (size_t)png_stream_capacity(png_geom(H, W, channels));
}

size_t rfx_png_encode_workspace_bytes(int N, int H, int W) {
  if (N < 1 || !axis_ok(H, W) || png_batch_limit(N, H, W)) return 0;
  return png_workspace_layout(N, H, W).total;
}

int rfx_png_encode_u8(const uint8_t* d_rgb, int N, int H, int W, int mode, uint8_t* d_stream, int32_t* d_stream_bytes, uint32_t* d_crc,
                      int32_t* d_channels, void* d_workspace, void* stream) {
  if (N < 1 || H < 1 || W < 1) return fail(RFX_ERR_INVALID, "rfx_png_encode_u8: N, H and W must be positive");
  if (mode != RFX_PNG_RGB && mode != RFX_PNG_GRAY && mode != RFX_PNG_AUTO)
    return fail(RFX_ERR_INVALID, "rfx_png_encode_u8: mode must be RFX_PNG_RGB, RFX_PNG_GRAY or RFX_PNG_AUTO");
  if (!axis_ok(H, W)) return refuse_size("rfx_png_encode_u8", H, W, false);
  if (const char* why = png_batch_limit(N, H, W)) return fail(RFX_ERR_UNSUPPORTED, std::string("rfx_png_encode_u8: ") + why);
  if (!d_rgb || !d_stream || !d_stream_bytes || !d_crc || !d_channels || !d_workspace) return fail(RFX_ERR_INVALID, "rfx_png_encode_u8: null pointer");
  if (reinterpret_cast<uintptr_t>(d_stream_bytes) % 4 || reinterpret_cast<uintptr_t>(d_crc) % 4 || reinterpret_cast<uintptr_t>(d_channels) % 4 ||
      reinterpret_cast<uintptr_t>(d_workspace) % 256)
    return fail(RFX_ERR_INVALID, "rfx_png_encode_u8: d_stream_bytes, d_crc and d_channels must be aligned to 4 bytes, d_workspace to 256");
  int dev;
  if (int rc = device_of(d_stream, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_png_encode(d_rgb, N, H, W, mode, d_stream, (size_t)png_stream_capacity(png_geom(H, W, mode == RFX_PNG_GRAY ? 1 : 3)),
                            d_stream_bytes, d_crc, d_channels, d_workspace, (hipStream_t)stream));
  return RFX_OK;
}

// ---- JPEG decode (rfx_jpeg_dec.hip) -----------------------------------------------------------------------------------------------
// what keeps a decode inside its index types: one thread per block and per pixel, 256 to a workgroup, at most 2^31 - 1 workgroups
static const char* jpeg_decode_batch_limit(int N, int H, int W) {
  const uint64_t per_launch = (uint64_t)INT32_MAX * 256;
  if ((uint64_t)N * (uint64_t)jpg_geom(H, W).blocks > per_launch || (uint64_t)N * (uint64_t)H * (uint64_t)W > per_launch)
    return "more blocks or pixels than one launch takes; decode in pieces";
  return nullptr;
}

size_t rfx_jpeg_decode_workspace_bytes(int N, int H, int W, size_t total_scan_bytes) {
  if (N < 1 || !axis_ok(H, W) || jpeg_decode_batch_limit(N, H, W) || total_scan_bytes > (size_t)N * (size_t)kJpdMaxScanBytes) return 0;
  return jpeg_decode_workspace_layout(N, H, W, total_scan_bytes).total;
}

int rfx_jpeg_decode_u8(const uint8_t* d_scans, const int64_t* h_scan_offsets, const int64_t* d_scan_offsets, int N, int H, int W,
                       const uint16_t* d_qtables, const uint8_t* d_huff, uint8_t* d_rgb, int32_t* d_status, void* d_workspace, void* stream) {
  if (N < 1 || H < 1 || W < 1) return fail(RFX_ERR_INVALID, "rfx_jpeg_decode_u8: N, H and W must be positive");
  if (!axis_ok(H, W)) return refuse_size("rfx_jpeg_decode_u8", H, W, true);
  if (const char* why = jpeg_decode_batch_limit(N, H, W)) return fail(RFX_ERR_UNSUPPORTED, std::string("rfx_jpeg_decode_u8: ") + why);
  int64_t longest = 0;
  if (int rc = check_stream_offsets("rfx_jpeg_decode_u8", "scan", h_scan_offsets, N, kJpdMaxScanBytes, &longest)) return rc;
  if (!d_scans || !d_scan_offsets || !d_qtables || !d_huff || !d_rgb || !d_status || !d_workspace)
    return fail(RFX_ERR_INVALID, "rfx_jpeg_decode_u8: null pointer");
  if (reinterpret_cast<uintptr_t>(d_scans) % 16) return fail(RFX_ERR_INVALID, "rfx_jpeg_decode_u8: d_scans must be aligned to 16 bytes");
  int dev;
  if (int rc = device_of(d_rgb, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_jpeg_decode(d_scans, d_scan_offsets, longest, (size_t)(h_scan_offsets[N] - h_scan_offsets[0]), N, H, W, d_qtables, d_huff, d_rgb,
                             d_status, d_workspace, (hipStream_t)stream));
  return RFX_OK;
}

// ---- PNG decode (rfx_png_dec.hip) -------------------------------------------------------------------------------------------------
static bool png_decode_type_ok(int color_type) { return pngd_bpp(color_type) != 0; }
// what keeps a decode inside its index types: one workgroup per image, and byte positions in the workspace and in d_rgb are int64
static const char* png_decode_batch_limit(int N, int H, int W, int color_type) {
  const uint64_t per_image = (pngd_filtered_bytes(H, W, pngd_bpp(color_type)) + 255) / 256 * 256;
  if (per_image > (uint64_t)INT64_MAX / (uint64_t)N) return "more filtered bytes than one launch indexes; decode in pieces";
  return nullptr;
}

size_t rfx_png_decode_workspace_bytes(int N, int H, int W, int color_type, size_t total_stream_bytes) {
  if (N < 1 || !axis_ok(H, W) || !png_decode_type_ok(color_type) || png_decode_batch_limit(N, H, W, color_type) ||
      total_stream_bytes > (size_t)N * (size_t)kPngdMaxStreamBytes)
    return 0;
  return png_decode_workspace_layout(N, H, W, color_type).total;
}

int rfx_png_decode_u8(const uint8_t* d_streams, const int64_t* h_stream_offsets, const int64_t* d_stream_offsets, int N, int H, int W,
                      int color_type, const uint8_t* d_palettes, const int32_t* d_palette_entries, uint8_t* d_rgb, int32_t* d_status,
                      void* d_workspace, void* stream) {
  if (N < 1 || H < 1 || W < 1) return fail(RFX_ERR_INVALID, "rfx_png_decode_u8: N, H and W must be positive");
  if (!png_decode_type_ok(color_type)) return fail(RFX_ERR_INVALID, "rfx_png_decode_u8: color_type must be 0, 2, 3 or 6");
  if (!axis_ok(H, W)) return refuse_size("rfx_png_decode_u8", H, W, false);
  if (const char* why = png_decode_batch_limit(N, H, W, color_type)) return fail(RFX_ERR_UNSUPPORTED, std::string("rfx_png_decode_u8: ") + why);
  if (int rc = check_stream_offsets("rfx_png_decode_u8", "stream", h_stream_offsets, N, kPngdMaxStreamBytes, nullptr)) return rc;
  if (!d_streams || !d_stream_offsets || !d_rgb || !d_status || !d_workspace || (color_type == 3 && (!d_palettes || !d_palette_entries)))
    return fail(RFX_ERR_INVALID, "rfx_png_decode_u8: null pointer");
  if (reinterpret_cast<uintptr_t>(d_streams) % 16) return fail(RFX_ERR_INVALID, "rfx_png_decode_u8: d_streams must be aligned to 16 bytes");
  if (reinterpret_cast<uintptr_t>(d_workspace) % 256 || reinterpret_cast<uintptr_t>(d_status) % 4 || reinterpret_cast<uintptr_t>(d_stream_offsets) % 8 ||
      (color_type == 3 && reinterpret_cast<uintptr_t>(d_palette_entries) % 4))
    return fail(RFX_ERR_INVALID, "rfx_png_decode_u8: d_workspace must be aligned to 256 bytes, d_stream_offsets to 8, d_status and d_palette_entries to 4");
  int dev;
  if (int rc = device_of(d_rgb, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_png_decode(d_streams, d_stream_offsets, N, H, W, color_type, d_palettes, d_palette_entries, d_rgb, d_status, d_workspace,
                            (hipStream_t)stream));
  return RFX_OK;
}

size_t rfx_pcm16_compress_filters_workspace_bytes(int N, int L, int C) {
  if (N <= 0 || L <= 0 || C <= 0) return 0;
  return cmp_workspace_layout(N, L, C).total;
}

int rfx_pcm16_apply_filters_compressed(const int16_t* d_pcm_in, int N, int L, int C, rfx_compress_options* o, int16_t* d_pcm_out,
                                       void* d_workspace, size_t workspace_bytes, void* stream) {
  static_assert(sizeof(CmpFlag) == 24, "rfx_compress_options.d_flags entries are CmpFlag (rfx_compress_core.h)");
  if (!d_pcm_in || !o || !d_pcm_out || !d_workspace || N <= 0 || L <= 0 || C <= 0)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: bad argument");
  if (o->struct_size != sizeof(rfx_compress_options))
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: options->struct_size is not sizeof(rfx_compress_options)");
  if (!o->d_gain10_by_rms || !o->d_gain12_by_rms || !o->d_boost_by_peak || !o->d_above || !o->d_max_att || !o->d_inc || !o->d_dec)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: a table is missing");
  if ((o->form != RFX_COMPRESS_SEQUENTIAL && o->form != RFX_COMPRESS_CHUNKED) || o->look_frames < 0 || o->chunk_frames < 0 ||
      !(o->margin >= 0.0) || o->flag_capacity < 0 || (o->flag_capacity > 0 && !o->d_flags))
    return fail(RFX_ERR_INVALID, "rfx_pcm16_apply_filters_compressed: bad option");
  if ((int64_t)L * C >= ((int64_t)1 << 23))
    return fail(RFX_ERR_UNSUPPORTED, "rfx_pcm16_apply_filters_compressed: L * C >= 2^23 (audioop.rms is exact only below that)");
  const CmpLayout w = cmp_workspace_layout(N, L, C);
  if (workspace_bytes < w.total) return fail(RFX_ERR_WORKSPACE, "rfx_pcm16_apply_filters_compressed: workspace too small");
  int dev;
  if (int rc = device_of(d_pcm_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  const hipStream_t s = (hipStream_t)stream;
  RFX_HIP(launch_cmp_compress(d_pcm_in, N, L, C, o->d_boost_by_peak, o->d_gain10_by_rms, o->d_above, o->d_max_att, o->d_inc, o->d_dec,
                              o->look_frames, o->form, o->chunk_frames, o->margin, o->d_flags, o->flag_capacity, o->d_rounds, d_workspace, s));
  // the one synchronisation of this path: how many products need the host's pow
  unsigned long long n = 0;
  RFX_HIP(hipMemcpyAsync(&n, (char*)d_workspace + w.count, sizeof n, hipMemcpyDeviceToHost, s));
  RFX_HIP(hipStreamSynchronize(s));
  o->n_flagged = (int64_t)n;
  if ((int64_t)n > o->flag_capacity) return RFX_OK;  // documented: d_pcm_out is not written, the caller redoes the batch on the host
  int16_t* x3 = reinterpret_cast<int16_t*>((char*)d_workspace + w.x3);
  if (n > 0) {
    std::vector<CmpFlag> h(n);
    RFX_HIP(hipMemcpyAsync(h.data(), o->d_flags, n * sizeof(CmpFlag), hipMemcpyDeviceToHost, s));
    RFX_HIP(hipStreamSynchronize(s));
    const int64_t total = (int64_t)N * L * C;
    for (CmpFlag& f : h) {
      if (f.index < 0 || f.index >= total) return fail(RFX_ERR_HIP, "rfx_pcm16_apply_filters_compressed: corrupt flag list");
      f.value = pcm_mul(f.x2, cmp_gain_host(f.att));
    }
    RFX_HIP(hipMemcpyAsync(o->d_flags, h.data(), n * sizeof(CmpFlag), hipMemcpyHostToDevice, s));
    RFX_HIP(launch_cmp_scatter(o->d_flags, (int64_t)n, x3, s));
    RFX_HIP(hipStreamSynchronize(s));  // h is released on return
  }
  RFX_HIP(launch_pcm_filters(x3, N, L, C, o->d_gain12_by_rms, o->d_boost_by_peak, d_pcm_out, (char*)d_workspace + w.filters, s));
  return RFX_OK;
}

// ---- int16 front end of the encode (rfx_pcm_in.hip) -----------------------------------------------------------------------------
// the reduced rates of a conversion, or an error: both rates positive, both reduced rates below 2^20 (rfx_pcm_in_core.h)
static int resample_rates(const char* who, int in_rate, int out_rate, RatecvRates* r) {
  if (in_rate <= 0 || out_rate <= 0) return fail(RFX_ERR_INVALID, std::string(who) + ": rates must be positive");
  *r = ratecv_rates(in_rate, out_rate);
  if (r->a >= kRatecvRateLimit || r->b >= kRatecvRateLimit)
    return fail(RFX_ERR_UNSUPPORTED, std::string(who) + ": reduced rates " + std::to_string(r->a) + " -> " + std::to_string(r->b) +
                                         " (rate / gcd) must stay below 2^20: audioop's double division is only then the exact quotient");
  return RFX_OK;
}
static bool channels_ok(int c) { return c == 1 || c == 2; }
static bool frame_aligned(const void* p, int channels) { return reinterpret_cast<uintptr_t>(p) % (2 * (size_t)channels) == 0; }

int rfx_pcm16_resample_frames(int64_t in_frames, int in_rate, int out_rate, int64_t* out_frames) {
  if (in_frames <= 0 || !out_frames) return fail(RFX_ERR_INVALID, "rfx_pcm16_resample_frames: bad argument (in_frames >= 1, out_frames not NULL)");
  RatecvRates r;
  if (int rc = resample_rates("rfx_pcm16_resample_frames", in_rate, out_rate, &r)) return rc;
  if (in_frames > INT64_MAX / kRatecvRateLimit) return fail(RFX_ERR_INVALID, "rfx_pcm16_resample_frames: in_frames too large");
  *out_frames = ratecv_out_frames(in_frames, r);
  return RFX_OK;
}

int rfx_pcm16_resample(const int16_t* d_in, int64_t in_frames, int in_channels, int in_rate, int out_channels, int out_rate,
                       int16_t* d_out, int64_t out_frames, void* stream) {
  if (in_frames <= 0) return fail(RFX_ERR_INVALID, "rfx_pcm16_resample: in_frames must be positive");
  if (!channels_ok(in_channels) || !channels_ok(out_channels)) return fail(RFX_ERR_INVALID, "rfx_pcm16_resample: channel counts must be 1 or 2");
  int64_t K = 0;
  if (int rc = rfx_pcm16_resample_frames(in_frames, in_rate, out_rate, &K)) return rc;
  if (out_frames != K)
    return fail(RFX_ERR_INVALID, "rfx_pcm16_resample: out_frames is " + std::to_string(out_frames) + ", " + std::to_string(in_frames) +
                                     " frames give " + std::to_string(K) + " (rfx_pcm16_resample_frames)");
  // one thread per run of kRatecvRun output frames, 256 threads per workgroup, at most 2^31 - 1 workgroups in a launch
  if (K > ((int64_t)INT32_MAX - 1) * 256 * kRatecvRun)
    return fail(RFX_ERR_UNSUPPORTED, "rfx_pcm16_resample: " + std::to_string(K) + " output frames are more than one launch holds; resample in pieces");
  if (!d_in || !d_out) return fail(RFX_ERR_INVALID, "rfx_pcm16_resample: null pointer");
  if (!frame_aligned(d_in, in_channels) || !frame_aligned(d_out, out_channels))
    return fail(RFX_ERR_INVALID, "rfx_pcm16_resample: pointers must be aligned to a frame (2 * channels bytes)");
  int dev;
  if (int rc = device_of(d_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_pcm_ratecv(d_in, in_channels, in_rate, out_channels, out_rate, d_out, K, (hipStream_t)stream));
  return RFX_OK;
}

namespace rfx {
// what rfx_pcm16_clips_to_waveform and rfx_image_from_pcm16_clips check before any launch (N > 0): sizes, channel counts, and -
// on the host copy of the starts - that every clip lies inside the recording; then the recording's pointer and its alignment
int check_pcm_clips(const char* who, const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts, int N, int Lw,
                    int out_channels) {
  if (frames <= 0 || Lw <= 0) return fail(RFX_ERR_INVALID, std::string(who) + ": frames and Lw must be positive");
  if (!channels_ok(in_channels) || !channels_ok(out_channels)) return fail(RFX_ERR_INVALID, std::string(who) + ": channel counts must be 1 or 2");
  if (!h_starts) return fail(RFX_ERR_INVALID, std::string(who) + ": h_starts is NULL");
  for (int i = 0; i < N; ++i)
    if (h_starts[i] < 0 || h_starts[i] > frames - Lw)
      return fail(RFX_ERR_INVALID, std::string(who) + ": clip " + std::to_string(i) + " (frames " + std::to_string(h_starts[i]) + " + " +
                                       std::to_string(Lw) + ") reaches outside the recording of " + std::to_string(frames) + " frames");
  if (!d_pcm) return fail(RFX_ERR_INVALID, std::string(who) + ": null pointer");
  if (!frame_aligned(d_pcm, in_channels)) return fail(RFX_ERR_INVALID, std::string(who) + ": d_pcm must be aligned to a frame (2 * channels bytes)");
  return RFX_OK;
}
}  // namespace rfx

int rfx_pcm16_clips_to_waveform(const int16_t* d_pcm, int64_t frames, int in_channels, const int64_t* h_starts, const int64_t* d_starts,
                                int N, int Lw, int out_channels, float* d_wave_out, void* stream) {
  if (N < 0) return fail(RFX_ERR_INVALID, "rfx_pcm16_clips_to_waveform: N is negative");
  if (N == 0) return RFX_OK;
  if (int rc = check_pcm_clips("rfx_pcm16_clips_to_waveform", d_pcm, frames, in_channels, h_starts, N, Lw, out_channels)) return rc;
  if (!d_starts || !d_wave_out) return fail(RFX_ERR_INVALID, "rfx_pcm16_clips_to_waveform: null pointer");
  int dev;
  if (int rc = device_of(d_wave_out, &dev)) return rc;
  RFX_ON_DEVICE(dev);
  RFX_HIP(launch_pcm_clips(d_pcm, in_channels, d_starts, N, Lw, out_channels, d_wave_out, (hipStream_t)stream));
  return RFX_OK;
}
