// Host emulator of the JPEG kernels (csrc/rfx_jpeg.hip).  TEST INFRASTRUCTURE ONLY (built by tests/test_jpeg_cpu.py with g++): the
// per-block arithmetic of rfx_jpeg_core.h in the kernels' stages - blocks to zigzag coefficients and AC bit counts, the scan of the
// bit counts, every block packed at its own bit offset into a zeroed word stream (first and last word merged with OR), the 0xFF
// count per 16-byte chunk and its scan, the stuffed copy with EOI - so that they are pinned against Pillow's files on the CPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_jpeg_core.h"

using namespace rfx;

extern "C" {

int emu_jpeg_quant_tables(int quality, uint16_t* luma64, uint16_t* chroma64) {
  if (quality < 1 || quality > 100) return -1;
  jpg_quant_tables(quality, luma64, chroma64);
  return 0;
}

uint64_t emu_jpeg_scan_capacity(int H, int W) { return jpg_scan_capacity(jpg_geom(H, W)); }

// (H, W, 3) uint8 and the (2, 64) tables in natural order -> the scan and EOI in `scan` (capacity bytes).  Returns its length,
// or -1 when it would pass the capacity; *zrl receives the number of ZRL codes emitted.
int64_t emu_jpeg_encode_u8(const uint8_t* rgb, int H, int W, const uint16_t* qtables, uint8_t* scan, uint64_t capacity, int64_t* zrl) {
  const JpgGeom g = jpg_geom(H, W);
  const JpgTables& t = kJpgTables;
  // 1. blocks
  std::vector<int16_t> coef((size_t)g.blocks * 64, 0x7fff);  // (dummy blocks stay unwritten, as on the device)
  std::vector<uint32_t> acbits(g.blocks);
  int64_t n_zrl = 0;
  for (int64_t mcu = 0; mcu < g.mcus; ++mcu)
    for (int k = 0; k < 6; ++k) {
      const int64_t b = mcu * 6 + k;
      const int tab = k < 4 ? 0 : 1;
      if (jpg_is_dummy(g, mcu, k)) {
        acbits[b] = t.ac[0].e[0] & 255;
        continue;
      }
      const int mx = (int)(mcu % g.mcu_w), my = (int)(mcu / g.mcu_w);
      int s[64];
      if (k < 4) jpg_samples_y(rgb, H, W, 2 * mx + (k & 1), 2 * my + (k >> 1), s);
      else jpg_samples_c(rgb, H, W, mx, my, k - 3, s);
      jpg_fdct(s);
      int16_t* out = coef.data() + b * 64;
      for (int z = 0; z < 64; ++z) out[z] = (int16_t)jpg_quantise(s[kJpgNatural[z]], qtables[64 * tab + kJpgNatural[z]]);
      uint32_t bits = 0;
      n_zrl += jpg_walk_ac(t, tab, out, false, [&](uint32_t, int len) { bits += len; });
      acbits[b] = bits;
    }
  // 2. bit offsets
  std::vector<uint64_t> bitoff(g.blocks);
  uint64_t total = 0;
  for (int64_t b = 0; b < g.blocks; ++b) {
    uint32_t bits = acbits[b];
    jpg_walk_dc(t, b % 6 < 4 ? 0 : 1, jpg_dc_diff(g, coef.data(), b / 6, (int)(b % 6)), [&](uint32_t, int len) { bits += len; });
    if (bits > (uint32_t)kJpgBlockMaxBits) return -2;
    bitoff[b] = total;
    total += bits;
  }
  // 3. pack: blocks in reverse order, to show that a block needs nothing but its own offset
  const uint64_t ub = (total + 7) / 8;
  std::vector<uint32_t> words((ub + 31) / 16 * 4, 0);
  uint32_t* w = words.data();
  for (int64_t b = g.blocks - 1; b >= 0; --b) {
    const int64_t mcu = b / 6;
    const int k = (int)(b % 6), tab = k < 4 ? 0 : 1;
    auto merge = [w](int64_t i, uint32_t v) { w[i] |= v; };
    auto store = [w](int64_t i, uint32_t v) { w[i] = v; };
    JpgBitSink<decltype(merge), decltype(store)> sink(bitoff[b], merge, store);
    jpg_walk_dc(t, tab, jpg_dc_diff(g, coef.data(), mcu, k), sink);
    jpg_walk_ac(t, tab, coef.data() + b * 64, jpg_is_dummy(g, mcu, k), sink);
    if (b == g.blocks - 1) {
      const int pad = (int)((0 - total) & 7);
      if (pad) sink((1u << pad) - 1, pad);
    }
    sink.finish();
  }
  // 4. 0xFF bytes per 16-byte chunk, scanned
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words.data());
  const int64_t chunks = (int64_t)((ub + 15) / 16);
  std::vector<uint32_t> ffpre(chunks);
  uint64_t ff = 0;
  for (int64_t c = 0; c < chunks; ++c) {
    ffpre[c] = (uint32_t)ff;
    for (int i = 0; i < 16; ++i) ff += bytes[c * 16 + i] == 0xFF;
  }
  if (ub + ff + 2 > capacity) return -1;
  // 5. the stuffed copy
  for (int64_t c = 0; c < chunks; ++c) {
    uint8_t* dst = scan + c * 16 + ffpre[c];
    for (int i = 0; i < 16 && (uint64_t)(c * 16 + i) < ub; ++i) {
      *dst++ = bytes[c * 16 + i];
      if (bytes[c * 16 + i] == 0xFF) *dst++ = 0;
    }
    if (c == chunks - 1) {
      dst[0] = 0xFF;
      dst[1] = 0xD9;
    }
  }
  if (zrl) *zrl = n_zrl;
  return (int64_t)(ub + ff + 2);
}

}  // extern "C"
