// Host emulator of the free-frame compaction of a held Griffin-Lim call (csrc/rfx_guide.hip: hold_count_kernel, hold_scan_kernel,
// hold_fill_kernel).  TEST INFRASTRUCTURE ONLY (built by tests/test_held_frames_cpu.py with g++): it runs the functions of
// rfx_guide_core.h that the kernels inline - the clamp, the rows a thread owns, the places of the count and of the chunk offsets, the
// list entry - the way the three launches walk them: per chunk of kHoldChunkRows rows one workgroup of kHoldThreads logical threads,
// thread tid owning kHoldRowsPerThread consecutive rows; one workgroup scanning the chunks' counts kHoldThreads at a time with a
// carry; the fill writing every row's span from its own offset.  What the kernels have of their own is the shuffle / LDS exchange
// of the prefix sums and the wave-per-row order of the stores.
#include <cstdint>
#include <vector>
#include "../../riffusion-hobby_amd/csrc/rfx_guide_core.h"

using namespace rfx;

extern "C" {

long long emu_hold_list_words(long long B, int T) { return (long long)hold_list_words(B, T); }
int emu_hold_chunk_rows() { return kHoldChunkRows; }
int emu_hold_is_held(int t, int head, int tail, int T) { return hold_is_held(t, head, tail, T) ? 1 : 0; }

// hold: (B, 2) int32; list: hold_list_words(B, T) ints
void emu_hold_list(const int32_t* hold, long long B, int T, int32_t* list) {
  const long long chunks = hold_chunks(B);
  int32_t* offs = list + hold_chunk_offsets_at(B, T);
  for (long long chunk = 0; chunk < chunks; ++chunk) {  // hold_count_kernel, workgroup `chunk`
    int total = 0;
    for (int tid = 0; tid < kHoldThreads; ++tid)
      for (int e = 0; e < kHoldRowsPerThread; ++e) total += hold_row_span(hold, hold_thread_row(chunk, tid, e), B, T).count;
    offs[chunk] = total;
  }
  int carry = 0;  // hold_scan_kernel, one workgroup
  for (long long c0 = 0; c0 < chunks; c0 += kHoldThreads) {
    int before = 0;
    for (int tid = 0; tid < kHoldThreads; ++tid) {
      const long long c = c0 + tid;
      const int v = c < chunks ? offs[c] : 0;
      if (c < chunks) offs[c] = carry + before;
      before += v;
    }
    carry += before;
  }
  list[hold_count_at(B, T)] = carry;
  for (long long chunk = 0; chunk < chunks; ++chunk) {  // hold_fill_kernel, workgroup `chunk`
    int at = offs[chunk];
    for (int tid = 0; tid < kHoldThreads; ++tid)
      for (int e = 0; e < kHoldRowsPerThread; ++e) {
        const long long row = hold_thread_row(chunk, tid, e);
        const HoldSpan s = hold_row_span(hold, row, B, T);
        for (int i = 0; i < s.count; ++i) list[(size_t)at + i] = hold_list_entry(row, T, s, i);
        at += s.count;
      }
  }
}

}  // extern "C"
