// Host emulator of the PNG decode kernels (csrc/rfx_png_dec.hip).  TEST INFRASTRUCTURE ONLY (built by tests/test_png_decode_cpu.py
// with g++): the code of rfx_png_dec_core.h in the kernels' two stages - every image's zlib stream inflated into its filtered
// bytes in the workspace, then unfiltered and converted to RGB - run by one lane, so that it is pinned against zlib and Pillow on
// the CPU.  Every buffer has exactly the size the device's has (the stream of one image, the workspace of the layout, the shared
// structures), so that a sanitizer build (RFX_PNGD_EMU_MAIN: a stand-alone program) sees any access past them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_png_dec_core.h"

using namespace rfx;

namespace {

struct OneLane {
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() const {}
};
struct VectorFetch {
  const std::vector<uint8_t>& v;
  uint32_t word(uint32_t i, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t j = 0; j < 4; ++j)
      if ((uint64_t)i + j < n) r |= (uint32_t)v.at(i + j) << (8 * j);
    return r;
  }
  uint8_t at(uint32_t i) { return v.at(i); }
};
struct FilteredStore {
  uint8_t* base;
  uint64_t size;
  void word(uint64_t i, uint32_t v) {
    if (i + 4 > size) std::abort();
    std::memcpy(base + i, &v, 4);
  }
  void byte(uint64_t i, uint8_t v) {
    if (i >= size) std::abort();
    base[i] = v;
  }
};
struct FilteredImage {
  uint8_t* base;
  uint64_t size;
  uint8_t byte(uint64_t i) {
    if (i >= size) std::abort();
    return base[i];
  }
  void put(uint64_t i, uint8_t v) {
    if (i >= size) std::abort();
    base[i] = v;
  }
};
struct RgbStore {
  uint8_t* base;
  uint64_t size;
  void operator()(uint64_t i, uint8_t v) {
    if (i >= size) std::abort();
    base[i] = v;
  }
};

}  // namespace

extern "C" {

int64_t emu_png_dec_workspace_bytes(int N, int H, int W, int color_type) { return (int64_t)png_decode_workspace_layout(N, H, W, color_type).total; }
int64_t emu_png_dec_inflate_shared_bytes() { return (int64_t)kPngdInflateSharedBytes; }
int64_t emu_png_dec_unfilter_shared_bytes() { return (int64_t)kPngdUnfilterSharedBytes; }
int emu_png_dec_seg_bytes() { return kPngdSegBytes; }

// The packed batch as rfx_png_decode_u8 takes it: streams holds exactly offsets[N] bytes, image n's zlib stream is
// [offsets[n], offsets[n + 1]); palettes (N, 256, 3) and entries (N) for colour type 3 (else unused) -> rgb (N, H, W, 3), status (N).
// workspace: exactly the layout's bytes; afterwards it holds every image's filtered bytes.  Returns 0, or -1 for arguments the
// entry refuses.
int emu_png_decode_batch(const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int color_type, const uint8_t* palettes,
                         const int32_t* entries, uint8_t* rgb, int32_t* status, uint8_t* workspace) {
  const int bpp = pngd_bpp(color_type);
  if (N < 1 || H < 1 || W < 1 || H > kPngdMaxSize || W > kPngdMaxSize || !bpp || offsets[0] < 0) return -1;
  for (int n = 0; n < N; ++n)
    if (offsets[n + 1] < offsets[n] || offsets[n + 1] - offsets[n] > kPngdMaxStreamBytes) return -1;
  const PngdLayout l = png_decode_workspace_layout(N, H, W, color_type);
  const uint64_t expected = pngd_filtered_bytes(H, W, bpp);
  const OneLane w;
  // 1. png_inflate_kernel: one group per image
  for (int n = 0; n < N; ++n) {
    const std::vector<uint8_t> stream(streams + offsets[n], streams + offsets[n + 1]);  // (exactly the stream: nothing readable behind it)
    std::unique_ptr<PngdInflateShared> sh(new PngdInflateShared);
    std::memset(sh.get(), 0xA5, sizeof(PngdInflateShared));
    VectorFetch in{stream};
    FilteredStore out{workspace + l.filtered + (size_t)n * l.per_image, expected};
    status[n] = pngd_inflate(w, in, (uint32_t)stream.size(), expected, out, sh.get());
  }
  // 2. png_unfilter_kernel: one group per image
  for (int n = 0; n < N; ++n) {
    if (status[n] != kPngdOk) continue;
    std::unique_ptr<PngdUnfilterShared> sh(new PngdUnfilterShared);
    std::memset(sh.get(), 0xA5, sizeof(PngdUnfilterShared));
    FilteredImage filt{workspace + l.filtered + (size_t)n * l.per_image, expected};
    RgbStore out{rgb + (size_t)n * H * W * 3, (uint64_t)H * W * 3};
    status[n] = pngd_unfilter_image(w, filt, H, W, color_type, color_type == 3 ? palettes + (size_t)n * 768 : nullptr,
                                    color_type == 3 ? entries[n] : 0, out, sh.get());
  }
  return 0;
}

}  // extern "C"

#ifdef RFX_PNGD_EMU_MAIN
// The sanitizer program: `<case> <out>`.  The case: int32 N, H, W, colour type; the N + 1 int64 offsets; (N, 768) palettes; N int32
// entries; the offsets[N] stream bytes - decoded in buffers of exactly the sizes the entry documents.  Writes the N int32 statuses,
// then the pixels of the images with status 0 (the others' as zeros), and prints "batch <rc>".
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[4];
  if (std::fread(head, 4, 4, f) != 4 || head[0] < 1 || head[0] > 4096 || head[1] < 1 || head[2] < 1 || head[1] > kPngdMaxSize || head[2] > kPngdMaxSize) return 2;
  const int N = head[0], H = head[1], W = head[2], ct = head[3];
  std::vector<int64_t> offsets((size_t)N + 1);
  std::vector<uint8_t> palettes((size_t)N * 768);
  std::vector<int32_t> entries((size_t)N);
  if (std::fread(offsets.data(), 8, offsets.size(), f) != offsets.size() || std::fread(palettes.data(), 1, palettes.size(), f) != palettes.size() ||
      std::fread(entries.data(), 4, entries.size(), f) != entries.size() || offsets[0] < 0 || offsets[N] < offsets[0] || offsets[N] > (1 << 28))
    return 2;
  std::vector<uint8_t> streams((size_t)offsets[N]);
  if (!streams.empty() && std::fread(streams.data(), 1, streams.size(), f) != streams.size()) return 2;
  std::fclose(f);
  const PngdLayout l = png_decode_workspace_layout(N, H, W, ct);
  std::vector<uint8_t> rgb((size_t)N * H * W * 3, 0), workspace(l.total, 0xA5);
  std::vector<int32_t> status((size_t)N, -1);
  const int rc = emu_png_decode_batch(streams.data(), offsets.data(), N, H, W, ct, palettes.data(), entries.data(), rgb.data(), status.data(), workspace.data());
  for (int n = 0; n < N; ++n)
    if (status[n] != 0) std::memset(rgb.data() + (size_t)n * H * W * 3, 0, (size_t)H * W * 3);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(status.data(), 4, status.size(), o);
  std::fwrite(rgb.data(), 1, rgb.size(), o);
  std::fclose(o);
  std::printf("batch %d\n", rc);
  return 0;
}
#endif
