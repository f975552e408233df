// batch_wide_weights_check.cpp -- the address arithmetic of the weighted kernels of a wide batch (nka_amd/csrc/host_logic.hpp:
// wide_wgt_offset with wide_len_owns, wide_len_nchunk and wide_chunk_len; the sweep of nka_batch_dev.hpp restated) against a
// brute-force model, built with the sanitizer flags of `make -C nka_amd/csrc hostcheck` (tests/test_batch_wide_weights_cpu.py
// runs it).  For every length 1 ... 3C + 33, every chunk, every thread and both forms of the weights (one row per system at the
// slot stride, one row for all at stride 0): the weight elements a workgroup reads lie inside the system's row and below its
// length, each is read once, a 16-byte load starts on 16 bytes, and a chunk beyond the system's own reads nothing.  The offsets
// are held against __int128 at the largest legal nsys x stride.
#include "../../nka_amd/csrc/host_logic.hpp"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                                                                                                  \
  do {                                                                                                                    \
    if (!(cond)) {                                                                                                        \
      if (failures++ < 20) { std::fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
    }                                                                                                                     \
  } while (0)

using namespace nka_host;

constexpr int kThreads = 64 * kBatchWaves;
constexpr int kTile = 2 * kThreads;

// what ld_tile / ld_pair of a 16-byte aligned vector read for thread t's pair at i of a chunk of n elements: a 16-byte load where
// both elements exist, else the elements below n one by one -> the elements read, and whether the load was the wide one
struct Read {
  long long i[2];
  int count;
  bool wide;
};
static Read pair_read(long long i, long long n, bool full) {
  Read r{{0, 0}, 0, false};
  if (full || i + 1 < n) {
    r.i[0] = i;
    r.i[1] = i + 1;
    r.count = 2;
    r.wide = true;
    return r;
  }
  if (i < n) r.i[r.count++] = i;
  if (i + 1 < n) r.i[r.count++] = i + 1;
  return r;
}

int main() {
  const long long C = kWideChunk;
  const long long vlen = 3 * C + 33;
  const BatchLayout lay = batch_layout(vlen, 3);
  CHECK(lay.stride % 32 == 0 && lay.stride >= vlen, "the slot stride %lld", (long long)lay.stride);
  CHECK(C % kTile == 0, "a chunk is whole tiles");
  const int nsys = 3;
  const long long nchunk = wide_nchunk(vlen);
  CHECK(nchunk == 4, "3C + 33 is four chunks");
  for (int form = 0; form < 2; form++) {
    const long long stride = form == 0 ? lay.stride : 0;      // one row per system, or the row all systems share
    const long long rows = form == 0 ? nsys : 1;
    std::vector<int> seen((size_t)(rows * lay.stride));
    for (long long len = 1; len <= vlen; len++) {
      for (int sys = 0; sys < nsys; sys += (len % 64 == 1 ? 1 : 2)) {      // (every system at every 64th length, 0 and 2 elsewhere)
        std::fill(seen.begin(), seen.end(), 0);
        const long long row0 = sys * stride;
        long long chunks_read = 0;
        for (long long c = 0; c < nchunk; c++) {
          if (!wide_len_owns(len, c)) continue;      // the workgroup returns before it reads anything
          chunks_read++;
          const long long n = wide_chunk_len(len, c);
          CHECK(n >= 1 && n <= C && c * C + n <= len, "chunk %lld of length %lld holds %lld elements", c, len, n);
          const long long off = wide_wgt_offset(sys, stride, c);
          CHECK(off == row0 + c * C, "wide_wgt_offset(%d, %lld, %lld) = %lld", sys, stride, c, off);
          CHECK((off * 8) % 16 == 0, "chunk %lld of system %d starts at byte %lld", c, sys, off * 8);
          // batch_sweep: the full tiles, then the ragged one with guards
          long long base = 0;
          for (; base + kTile <= n; base += kTile)
            for (int t = 0; t < kThreads; t++) {
              const Read r = pair_read(base + 2 * t, n, true);
              CHECK(((off + r.i[0]) * 8) % 16 == 0, "a 16-byte load at byte %lld", (off + r.i[0]) * 8);
              for (int q = 0; q < r.count; q++) {
                const long long e = off + r.i[q];
                CHECK(e >= row0 && e < row0 + len, "system %d, length %lld, chunk %lld reads weight %lld of its row", sys, len, c, e - row0);
                if (e >= 0 && e < (long long)seen.size()) seen[(size_t)e]++;
              }
            }
          if (base < n)
            for (int t = 0; t < kThreads; t++) {
              const Read r = pair_read(base + 2 * t, n, false);
              if (r.wide) CHECK(((off + r.i[0]) * 8) % 16 == 0, "a 16-byte load at byte %lld", (off + r.i[0]) * 8);
              for (int q = 0; q < r.count; q++) {
                const long long e = off + r.i[q];
                CHECK(e >= row0 && e < row0 + len, "system %d, length %lld, chunk %lld reads weight %lld of its row", sys, len, c, e - row0);
                if (e >= 0 && e < (long long)seen.size()) seen[(size_t)e]++;
              }
            }
        }
        CHECK(chunks_read == wide_len_nchunk(len), "length %lld is read by %lld chunks", len, chunks_read);
        // every weight below the length exactly once, nothing else of the buffer
        for (long long e = 0; e < (long long)seen.size(); e++) {
          const int want = (e >= row0 && e < row0 + len) ? 1 : 0;
          if (seen[(size_t)e] != want) {
            CHECK(false, "form %d, system %d, length %lld: element %lld of the buffer read %d times", form, sys, len, e, seen[(size_t)e]);
            break;
          }
        }
      }
    }
  }
  // the largest legal batch: nsys = 65535 systems of NKA_HIP_BATCH_WIDE_MAX_VLEN = 512 C elements at mvec = 32; 64 bits hold it
  {
    const long long cap = 512 * C, nsys = 65535;
    const BatchLayout lay = batch_layout(cap, 32);
    for (long long sys : {0LL, 1LL, 4095LL, 4096LL, 32767LL, 32768LL, 65534LL})
      for (long long c : {0LL, 1LL, 255LL, 256LL, 511LL})
        for (long long stride : {(long long)lay.stride, 0LL}) {
          const __int128 want = (__int128)sys * stride + (__int128)c * C;
          const long long got = wide_wgt_offset(sys, stride, c);
          CHECK((__int128)got == want, "wide_wgt_offset(%lld, %lld, %lld) wrapped", sys, stride, c);
          CHECK(want * 8 + (__int128)C * 8 <= (__int128)nsys * lay.stride * 8, "chunk (%lld, %lld) leaves the weight buffer", sys, c);
          CHECK(want * 8 < ((__int128)1 << 63), "byte offset beyond 63 bits");
          if (sys >= 4096 && stride) CHECK(want * 8 >= ((__int128)1 << 32), "the case is beyond 2^32 bytes");
        }
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch_wide_weights_check: OK\n");
  return 0;
}
