// Host emulator of the JPEG decode kernels (csrc/rfx_jpeg_dec.hip).  TEST INFRASTRUCTURE ONLY (built by
// tests/test_jpeg_decode_cpu.py with g++): the arithmetic of rfx_jpeg_dec_core.h in the kernels' stages - the stuffed zeros
// counted per 16-byte chunk, scanned and dropped; the four Huffman tables derived; the subsequences of every group decoded from
// an assumed state and then, in rounds, from their predecessors' exit states until none changes (the "threads" of a round all
// read the states of the round before); the scan of the block counts; the pass that writes the coefficients; the DC prefix
// sums; dequantisation and IDCT into the three planes; upsampling and colour conversion - so that they are pinned against
// Pillow's decode on the CPU.  Every buffer has exactly the size the device's workspace gives it, so that a sanitizer build
// (RFX_JPD_EMU_MAIN: a stand-alone program) sees any read past them.  emu_jpeg_decode_batch is the packed batch: N scans back to
// back at any byte offsets, stages 1 and 2 indexed as the two unstuff kernels index them (the aligned first chunk, the chunk
// tables at jpd_chunk_offset, the regions at jpd_region_offset, the bytes outside [lo, hi) masked, the 1024-chunk passes and
// their carry, the copy's grid of min(chunk groups of the longest scan, 64) workgroups whose threads stride over an image's
// chunks) inside one workspace of the device's layout, so that the regions can be compared with the device's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../riffusion-hobby_amd/csrc/rfx_jpeg_dec_core.h"

using namespace rfx;

namespace {
constexpr int kEmuChunk = 16;           // rfx_jpeg_dec.hip's kJpdChunk
constexpr int kEmuScanThreads = 1024;   // ... and kJpdScanThreads: the chunks of one pass of the unstuff scan
constexpr int kEmuThreads = 256;        // ... kJpdThreads: the threads of one workgroup of jpd_unstuff_kernel
constexpr int kEmuUnstuffGridY = 64;    // ... and the most workgroups launch_jpeg_decode gives one image there
}  // namespace

namespace {

// stages 3 .. 7 of one image: words - its unstuffed region (the stream of ulen bytes, rounded up to a word, and two words more),
// coef (blocks, 64) and planes (jpd_plane_bytes) - its parts of the workspace.  status: what stages 1 and 2 found.
// With several causes the status is the largest of them, as the kernels' atomicMax leaves it.
int decode_unstuffed(const uint32_t* words, int64_t ulen, int status, int H, int W, const uint16_t* qtables, const uint8_t* huff, int16_t* coef,
                     uint8_t* planes, uint8_t* rgb, int32_t* info) {
  const JpgGeom g = jpg_geom(H, W);
  const uint32_t total_bits = (uint32_t)(ulen * 8);
  const auto peek = [&](uint32_t p) {
    const uint64_t two = ((uint64_t)__builtin_bswap32(words[p >> 5]) << 32) | __builtin_bswap32(words[(p >> 5) + 1]);
    return (uint32_t)((two << (p & 31)) >> 32);
  };
  // 3. tables
  std::vector<JpdHuff> tables(4);
  bool bad_table = false;
  const auto flag = [&status](int cause) { status = cause > status ? cause : status; };
  for (int t = 0; t < 4; ++t) {
    if (!jpd_huff_derive(huff + t * kJpdHuffBytes, &tables[t])) bad_table = true;
    std::memcpy(tables[t].huffval, huff + t * kJpdHuffBytes + 16, 256);
  }
  std::memset(coef, 0, (size_t)g.blocks * 64 * sizeof(int16_t));
  const int64_t nsub = ((int64_t)total_bits + kJpdSubBits - 1) / kJpdSubBits;
  int32_t rounds_max = 0, rounds_sum = 0, groups = 0;
  if (bad_table) flag(kJpdBadTable);  // (the entropy kernel returns here: no coefficient is written)
  if (!bad_table) {
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
        int16_t* out = coef + first[i] * 64;
        int64_t nb;
        int err;
        const JpdState end = jpd_decode_span<false>(tables.data(), peek, in, span_end(i), total_bits, room,
                                             [&](int64_t b, int k, int v) { out[b * 64 + kJpgNatural[k]] = (int16_t)v; }, &nb, &err);
        if (err != kJpdOk) flag(err);
        else if (nb == room && total_bits - end.p > 7) flag(kJpdLeftOver);
      }
      block_base = at;
      carry = exit_state[n - 1];
    }
    if (block_base < g.blocks) flag(kJpdLeftOver);
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
  uint8_t* yp = planes;
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

}  // namespace

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
  std::vector<int16_t> coef((size_t)g.blocks * 64);
  std::vector<uint8_t> planes((size_t)jpd_plane_bytes(g));
  return decode_unstuffed(words.data(), ulen, status, H, W, qtables, huff, coef.data(), planes.data(), rgb, info);
}

int emu_jpeg_dec_scan_threads() { return kEmuScanThreads; }
// the chunks one trip of jpd_unstuff_kernel's grid copies at most: an image with more sends its threads round again
int emu_jpeg_dec_unstuff_trip_chunks() { return kEmuUnstuffGridY * kEmuThreads; }

// the six offsets of the device's workspace and its size: out[0 .. 6] = unstuffed, pre, ulen, coef, planes, total, coef_bytes
void emu_jpeg_dec_layout(int N, int H, int W, int64_t total_scan_bytes, int64_t* out) {
  const JpdLayout l = jpeg_decode_workspace_layout(N, H, W, (size_t)total_scan_bytes);
  const size_t v[7] = {l.unstuffed, l.pre, l.ulen, l.coef, l.planes, l.total, l.coef_bytes};
  for (int i = 0; i < 7; ++i) out[i] = (int64_t)v[i];
}
// where image n's region and chunk table start inside the `unstuffed` and `pre` areas (bytes, uint32 entries)
int64_t emu_jpeg_dec_region_offset(int64_t off, int64_t off0, int64_t n) { return jpd_region_offset(off, off0, n); }
int64_t emu_jpeg_dec_chunk_offset(int64_t off, int64_t off0, int64_t n) { return jpd_chunk_offset(off, off0, n); }

// The packed batch as rfx_jpeg_decode_u8 takes it: scans holds exactly offsets[N] bytes, image n's are [offsets[n], offsets[n + 1]);
// qtables (N, 2, 64), huff (N, 4, 272) -> rgb (N, H, W, 3), status (N).  workspace: exactly the layout's `total` bytes; afterwards
// it holds what the device's holds: the regions, the chunk tables, the lengths, the coefficients (natural order, DC as values)
// and the planes.  With several causes an image's status is the largest, as on the device.  Returns 0, or -1 for arguments the
// entry refuses.
int emu_jpeg_decode_batch(const uint8_t* scans, const int64_t* offsets, int N, int H, int W, const uint16_t* qtables, const uint8_t* huff,
                          uint8_t* rgb, int32_t* status, uint8_t* workspace) {
  if (N < 1 || H < 1 || W < 1 || H > kJpgMaxSize || W > kJpgMaxSize || offsets[0] < 0) return -1;
  int64_t longest = 0;
  for (int n = 0; n < N; ++n) {
    if (offsets[n + 1] < offsets[n] || offsets[n + 1] - offsets[n] > kJpdMaxScanBytes) return -1;
    longest = offsets[n + 1] - offsets[n] > longest ? offsets[n + 1] - offsets[n] : longest;
  }
  // launch_jpeg_decode's gridDim.y of jpd_unstuff_kernel: the call's longest scan decides it for every image
  const int64_t chunk_groups = (longest / kEmuChunk + 2 + kEmuThreads - 1) / kEmuThreads;
  const int64_t grid_y = chunk_groups < kEmuUnstuffGridY ? chunk_groups : kEmuUnstuffGridY;
  const JpgGeom g = jpg_geom(H, W);
  const int64_t total = offsets[N], off0 = offsets[0];
  const JpdLayout l = jpeg_decode_workspace_layout(N, H, W, (size_t)(total - off0));
  uint8_t* unstuffed = workspace + l.unstuffed;
  uint32_t* pre = reinterpret_cast<uint32_t*>(workspace + l.pre);
  uint32_t* ulen = reinterpret_cast<uint32_t*>(workspace + l.ulen);
  int16_t* coef = reinterpret_cast<int16_t*>(workspace + l.coef);
  uint8_t* planes = workspace + l.planes;
  // load_chunk: the 16 bytes at `at` (a multiple of 16) and the one before; bytes outside [lo, hi) read as 0
  struct Chunk {
    uint8_t prev, b[kEmuChunk];
  };
  const auto load_chunk = [&](int64_t at, int64_t lo, int64_t hi) {
    Chunk c;
    for (int i = 0; i < kEmuChunk; ++i) c.b[i] = at + i < total ? scans[at + i] : (uint8_t)0;
    for (int i = 0; i < kEmuChunk; ++i)
      if (at + i < lo || at + i >= hi) c.b[i] = 0;
    c.prev = at - 1 >= lo ? scans[at - 1] : (uint8_t)0;
    return c;
  };
  for (int64_t n = 0; n < N; ++n) {
    const int64_t lo = offsets[n], hi = offsets[n + 1], first = lo & ~(int64_t)15;
    const int64_t chunks = (hi - first + kEmuChunk - 1) / kEmuChunk;
    uint32_t* p = pre + jpd_chunk_offset(lo, off0, n);
    // 1. jpd_unstuff_scan_kernel: passes of kEmuScanThreads chunks, an exclusive scan inside a pass, the carry between passes
    bool marker = false;
    uint32_t carry = 0;
    for (int64_t base = 0; base < chunks; base += kEmuScanThreads) {
      uint32_t in_pass = 0;
      for (int64_t c = base; c < base + kEmuScanThreads && c < chunks; ++c) {
        const Chunk v = load_chunk(first + c * kEmuChunk, lo, hi);
        uint8_t before = v.prev;
        uint32_t drops = 0;
        for (int i = 0; i < kEmuChunk; ++i) {
          drops += before == 0xFF && v.b[i] == 0 && first + c * kEmuChunk + i < hi;
          marker |= before == 0xFF && v.b[i] != 0;
          before = v.b[i];
        }
        p[c] = carry + in_pass;
        in_pass += drops;
      }
      carry += in_pass;
    }
    const bool dangling = hi > lo && scans[hi - 1] == 0xFF;
    ulen[n] = (uint32_t)(hi - lo) - carry;
    status[n] = marker || dangling ? kJpdMarker : kJpdOk;
  }
  // (every image's chunk table is written before any is read, as the launches are ordered: tables that overlapped would show)
  for (int64_t n = 0; n < N; ++n) {
    const int64_t lo = offsets[n], hi = offsets[n + 1], first = lo & ~(int64_t)15;
    const int64_t chunks = (hi - first + kEmuChunk - 1) / kEmuChunk;
    const uint32_t* p = pre + jpd_chunk_offset(lo, off0, n);
    // 2. jpd_unstuff_kernel: every thread of the image's grid_y workgroups, striding by the grid
    uint8_t* out = unstuffed + jpd_region_offset(lo, off0, n);
    for (int64_t thread = 0; thread < grid_y * kEmuThreads; ++thread)
      for (int64_t c = thread; c < chunks; c += grid_y * kEmuThreads) {
        const int64_t at = first + c * kEmuChunk;
        const Chunk v = load_chunk(at, lo, hi);
        int64_t o = (at > lo ? at - lo : 0) - (int64_t)p[c];
        uint8_t before = v.prev;
        for (int i = 0; i < kEmuChunk; ++i) {
          if (at + i >= lo && at + i < hi && !(before == 0xFF && v.b[i] == 0)) out[o++] = v.b[i];
          before = v.b[i];
        }
      }
    // 3 .. 7: the image's region as the entropy kernel loads it - words past the region read as 0, the bytes of its last
    // words that stage 2 did not write as they are
    const int64_t region_words = ((int64_t)ulen[n] + 3) / 4 + 2;
    std::vector<uint32_t> words((size_t)region_words);
    std::memcpy(words.data(), out, (size_t)region_words * 4);
    const int rest = decode_unstuffed(words.data(), ulen[n], kJpdOk, H, W, qtables + n * 128, huff + n * 4 * kJpdHuffBytes,
                                      coef + n * g.blocks * 64, planes + n * jpd_plane_bytes(g), rgb + n * (int64_t)H * W * 3, nullptr);
    status[n] = rest > status[n] ? rest : status[n];
  }
  return 0;
}

}  // extern "C"

#ifdef RFX_JPD_EMU_MAIN
// The sanitizer program.  `<case>`: one damaged-scan case - int32 H, W, scan bytes; the (2, 64) uint16 tables; the (4, 272) Huffman
// tables; the scan - decoded, prints "status <s>".  `batch <case> <out>`: one packed batch - int32 N, H, W; the N + 1 int64
// offsets; (N, 2, 64) uint16; (N, 4, 272) uint8; the offsets[N] bytes - decoded in buffers of exactly the sizes the entry
// documents; writes the N int32 statuses, the pixels and the workspace to <out> and prints "batch <rc>".
static int batch_main(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  int32_t head[3];
  if (std::fread(head, 4, 3, f) != 3 || head[0] < 1 || head[0] > 4096 || head[1] < 1 || head[2] < 1 || head[1] > kJpgMaxSize || head[2] > kJpgMaxSize)
    return 2;
  const int N = head[0], H = head[1], W = head[2];
  std::vector<int64_t> offsets((size_t)N + 1);
  std::vector<uint16_t> q((size_t)N * 128);
  std::vector<uint8_t> huff((size_t)N * 4 * kJpdHuffBytes);
  if (std::fread(offsets.data(), 8, offsets.size(), f) != offsets.size() || std::fread(q.data(), 2, q.size(), f) != q.size() ||
      std::fread(huff.data(), 1, huff.size(), f) != huff.size() || offsets[0] < 0 || offsets[N] < offsets[0] || offsets[N] > (1 << 28))
    return 2;
  std::vector<uint8_t> scans((size_t)offsets[N]);
  if (!scans.empty() && std::fread(scans.data(), 1, scans.size(), f) != scans.size()) return 2;
  std::fclose(f);
  const JpdLayout l = jpeg_decode_workspace_layout(N, H, W, (size_t)(offsets[N] - offsets[0]));
  std::vector<uint8_t> rgb((size_t)N * H * W * 3), workspace(l.total, 0xA5);
  std::vector<int32_t> status((size_t)N, -1);
  const int rc = emu_jpeg_decode_batch(scans.data(), offsets.data(), N, H, W, q.data(), huff.data(), rgb.data(), status.data(), workspace.data());
  FILE* o = std::fopen(out, "wb");
  if (!o) return 2;
  std::fwrite(status.data(), 4, status.size(), o);
  std::fwrite(rgb.data(), 1, rgb.size(), o);
  std::fwrite(workspace.data(), 1, workspace.size(), o);
  std::fclose(o);
  std::printf("batch %d\n", rc);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "batch")) return batch_main(argv[2], argv[3]);
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
