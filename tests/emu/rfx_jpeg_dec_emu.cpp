// Host emulator of the JPEG decode kernels (csrc/rfx_jpeg_dec.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_jpeg_decode_cpu.py with g++): the arithmetic of rfx_jpeg_dec_core.h in the kernels' stages - the stuffed zeros
// counted per 16-byte chunk, scanned and dropped; the four Huffman tables derived; the subsequences of every group decoded from
// an assumed state and then, in rounds, from their predecessors' exit states until none changes (the "threads" of a round all
// read the states of the round before); the scan of the block counts; the pass that writes the coefficients; the DC prefix
// sums; dequantisation and IDCT into the three planes; upsampling and colour conversion - so that they are pinned against
// Pillow's decode on the CPU.  Every buffer has exactly the size the device's workspace gives it, so that a sanitizer build
// (RFX_JPD_EMU_MAIN: a stand-alone program) sees any read past them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_jpeg_dec_core.h"

using namespace rfx;

extern "C" {

int emu_jpeg_dec_sub_bits() { return kJpdSubBits; }
int emu_jpeg_dec_group() { return kJpdGroup; }

// scan: the entropy-coded bytes of one image (after SOS, without EOI); qtables (2, 64) uint16 natural order; huff (4, 272)
// uint8 DC0 AC0 DC1 AC1 -> rgb (H, W, 3).  Returns the status.  info[0]: the most rounds a group took to synchronise (the first
// decode from the assumed states not counted), info[1]: subsequences, info[2]: groups, info[3]: rounds summed over the groups.
int emu_jpeg_decode_u8(const uint8_t* scan_in, int64_t scan_bytes, int H, int W, const uint16_t* qtables, const uint8_t* huff,
                       uint8_t* rgb, int32_t* info) {
  if (H < 1 || W < 1 || H > kJpgMaxSize || W > kJpgMaxSize || scan_bytes < 0 || scan_bytes > kJpdMaxScanBytes) return -1;
  const JpgGeom g = jpg_geom(H, W);
  const std::vector<uint8_t> scan(scan_in, scan_in + scan_bytes);  // (exactly the scan: nothing readable behind it)
  int status = kJpdOk;
  // 1. the zeros to drop, per 16-byte chunk, scanned
  const int64_t chunks = (scan_bytes + 15) / 16;
  std::vector<uint32_t> pre(chunks);
  uint32_t drops = 0;
  const auto dropped = [&](int64_t i) { return i > 0 && scan[i] == 0 && scan[i - 1] == 0xFF; };
  for (int64_t c = 0; c < chunks; ++c) {
    pre[c] = drops;
    for (int64_t i = c * 16; i < c * 16 + 16 && i < scan_bytes; ++i) {
      drops += dropped(i);
      if (i > 0 && scan[i - 1] == 0xFF && scan[i] != 0) status = kJpdMarker;
    }
  }
  if (scan_bytes > 0 && scan[scan_bytes - 1] == 0xFF) status = kJpdMarker;
  const int64_t ulen = scan_bytes - drops;
  // 2. the compacted copy, in a region of the device's size: the stream rounded up to a word and two words more
  std::vector<uint32_t> words((ulen + 3) / 4 + 2, 0);
  {
    uint8_t* u = reinterpret_cast<uint8_t*>(words.data());
    for (int64_t c = 0; c < chunks; ++c) {
      int64_t o = c * 16 - pre[c];
      for (int64_t i = c * 16; i < c * 16 + 16 && i < scan_bytes; ++i)
        if (!dropped(i)) u[o++] = scan[i];
    }
  }
  const uint32_t total_bits = (uint32_t)(ulen * 8);
  const auto peek = [&](uint32_t p) {
    const uint64_t two = ((uint64_t)__builtin_bswap32(words[p >> 5]) << 32) | __builtin_bswap32(words[(p >> 5) + 1]);
    return (uint32_t)((two << (p & 31)) >> 32);
  };
  // 3. tables
  std::vector<JpdHuff> tables(4);
  for (int t = 0; t < 4; ++t) {
    if (!jpd_huff_derive(huff + t * kJpdHuffBytes, &tables[t])) status = kJpdBadTable;
    std::memcpy(tables[t].huffval, huff + t * kJpdHuffBytes + 16, 256);
  }
  std::vector<int16_t> coef((size_t)g.blocks * 64, 0);
  const int64_t nsub = ((int64_t)total_bits + kJpdSubBits - 1) / kJpdSubBits;
  int32_t rounds_max = 0, rounds_sum = 0, groups = 0;
  if (status != kJpdBadTable) {
    for (int t = 0; t < 4; ++t)
      for (int i = 0; i < (1 << kJpdLutBits); ++i) tables[t].lut[i] = jpd_huff_lut_entry(tables[t], i);
    // 4. the groups of subsequences
    JpdState carry{0, 0, 0, 1, 0};
    int64_t block_base = 0;
    const auto no_emit = [](int64_t, int, int) {};
    for (int64_t base = 0; base < nsub && carry.valid && block_base < g.blocks; base += kJpdGroup, ++groups) {
      const int n = (int)(nsub - base < kJpdGroup ? nsub - base : kJpdGroup);
      std::vector<JpdState> exit_state(n), last_in(n);
      std::vector<int64_t> count(n);
      const auto span_end = [&](int i) {
        const int64_t e = (base + i + 1) * kJpdSubBits;
        return (uint32_t)(e < total_bits ? e : total_bits);
      };
      const auto run = [&](int i, JpdState in) {
        last_in[i] = in;
        const uint32_t lo = (uint32_t)((base + i) * kJpdSubBits);
        int err;
        if (!in.valid || in.p < lo || in.p >= span_end(i)) {  // nothing to decode from: a state the true one will replace
          exit_state[i] = JpdState{span_end(i), 0, 0, 0, 0};
          count[i] = 0;
          return;
        }
        exit_state[i] = jpd_decode_span<true>(tables.data(), peek, in, span_end(i), total_bits, INT64_MAX, no_emit, &count[i], &err);
      };
      for (int i = 0; i < n; ++i) run(i, i ? JpdState{(uint32_t)((base + i) * kJpdSubBits), 0, 0, 1, 0} : carry);
      int rounds = 0;
      for (int r = 1; r <= n; ++r) {  // n rounds at most: subsequence 0 starts from the truth
        std::vector<JpdState> in(n);
        for (int i = 0; i < n; ++i) in[i] = i ? exit_state[i - 1] : carry;
        bool changed = false;
        for (int i = 0; i < n; ++i)
          if (!jpd_same(in[i], last_in[i])) {
            run(i, in[i]);
            changed = true;
          }
        if (!changed) break;
        rounds = r;
      }
      rounds_max = rounds > rounds_max ? rounds : rounds_max;
      rounds_sum += rounds;
      // the first block of every subsequence, and the pass that writes (in reverse order: a subsequence needs only its own state)
      std::vector<int64_t> first(n);
      int64_t at = block_base;
      for (int i = 0; i < n; ++i) {
        first[i] = at;
        at += count[i];
      }
      for (int i = n - 1; i >= 0; --i) {
        const JpdState in = last_in[i];
        if (!in.valid || in.p < (uint32_t)((base + i) * kJpdSubBits) || in.p >= span_end(i)) continue;
        const int64_t room = g.blocks - first[i];
        if (room <= 0) continue;
        int16_t* out = coef.data() + first[i] * 64;
        int64_t nb;
        int err;
        const JpdState end = jpd_decode_span<false>(tables.data(), peek, in, span_end(i), total_bits, room,
                                             [&](int64_t b, int k, int v) { out[b * 64 + kJpgNatural[k]] = (int16_t)v; }, &nb, &err);
        if (err != kJpdOk && status == kJpdOk) status = err;
        if (err == kJpdOk && nb == room && total_bits - end.p > 7 && status == kJpdOk) status = kJpdLeftOver;
      }
      block_base = at;
      carry = exit_state[n - 1];
    }
    if (block_base < g.blocks && status == kJpdOk) status = kJpdLeftOver;
  }
  if (info) {
    info[0] = rounds_max;
    info[1] = (int32_t)nsub;
    info[2] = groups;
    info[3] = rounds_sum;
  }
  // 5. DC differences -> values, per component in scan order
  int dc[3] = {0, 0, 0};
  for (int64_t b = 0; b < g.blocks; ++b) {
    const int comp = b % 6 < 4 ? 0 : (int)(b % 6) - 3;
    dc[comp] += coef[b * 64];
    coef[b * 64] = (int16_t)dc[comp];
  }
  // 6. planes
  const int ys = 16 * g.mcu_w, cs = 8 * g.mcu_w;
  std::vector<uint8_t> planes((size_t)jpd_plane_bytes(g));
  uint8_t* yp = planes.data();
  uint8_t* cbp = yp + 256 * g.mcus;
  uint8_t* crp = cbp + 64 * g.mcus;
  for (int64_t b = 0; b < g.blocks; ++b) {
    const int64_t mcu = b / 6;
    const int k = (int)(b % 6), mx = (int)(mcu % g.mcu_w), my = (int)(mcu / g.mcu_w);
    int c[64];
    for (int i = 0; i < 64; ++i) c[i] = coef[b * 64 + i];
    jpd_dequant_idct(c, qtables + (k < 4 ? 0 : 64));
    uint8_t* dst = k < 4 ? yp + ((int64_t)(16 * my + 8 * (k >> 1)) * ys + 16 * mx + 8 * (k & 1))
                         : (k == 4 ? cbp : crp) + ((int64_t)8 * my * cs + 8 * mx);
    const int stride = k < 4 ? ys : cs;
    for (int r = 0; r < 8; ++r)
      for (int x = 0; x < 8; ++x) dst[(int64_t)r * stride + x] = (uint8_t)c[r * 8 + x];
  }
  // 7. pixels
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      jpd_rgb(yp[(int64_t)y * ys + x], jpd_upsample((const uint8_t*)cbp, cs, H, W, x, y), jpd_upsample((const uint8_t*)crp, cs, H, W, x, y),
              rgb + ((int64_t)y * W + x) * 3);
  return status;
}

}  // extern "C"

#ifdef RFX_JPD_EMU_MAIN
// The sanitizer program of the damaged-scan tests: reads one case from a file - int32 H, W, scan bytes; the (2, 64) uint16
// tables; the (4, 272) Huffman tables; the scan - decodes it and prints "status <s>".
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[3];
  std::vector<uint16_t> q(128);
  std::vector<uint8_t> huff(4 * kJpdHuffBytes);
  if (std::fread(head, 4, 3, f) != 3 || std::fread(q.data(), 2, 128, f) != 128 || std::fread(huff.data(), 1, huff.size(), f) != huff.size() ||
      head[0] < 1 || head[1] < 1 || head[0] > 4096 || head[1] > 4096 || head[2] < 0)
    return 2;
  std::vector<uint8_t> scan((size_t)head[2]);
  if (head[2] && std::fread(scan.data(), 1, scan.size(), f) != scan.size()) return 2;
  std::fclose(f);
  std::vector<uint8_t> rgb((size_t)head[0] * head[1] * 3);
  int32_t info[4];
  std::printf("status %d\n", emu_jpeg_decode_u8(scan.data(), head[2], head[0], head[1], q.data(), huff.data(), rgb.data(), info));
  return 0;
}
#endif
