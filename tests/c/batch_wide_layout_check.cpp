// batch_wide_layout_check.cpp -- the layout arithmetic of the WIDE batched accelerator (nka_amd/csrc/host_logic.hpp: wide_nchunk,
// wide_chunk_len, wide_part_index, wide_sums_lds, wide_combine_lds, wide_scalar_lds) against brute-force models, built with the
// sanitizer flags of `make -C nka_amd/csrc hostcheck` (tests/test_batch_wide_cpu.py runs it).  Every element a piece owns is
// painted into a map and collisions are counted, instead of trusting the closed forms.
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

static void paint(std::vector<int> &map, long long off, long long len, int tag) {
  for (long long i = off; i < off + len; i++) {
    CHECK(i >= 0 && i < (long long)map.size(), "piece %d leaves the block at %lld of %zu", tag, i, map.size());
    if (i < 0 || i >= (long long)map.size()) return;
    CHECK(map[(size_t)i] == 0, "pieces %d and %d overlap at %lld", map[(size_t)i], tag, i);
    map[(size_t)i] = tag;
  }
}
static void no_hole(const std::vector<int> &map, const char *what, int mvec) {
  for (int x : map) CHECK(x != 0, "a hole in %s at mvec %d", what, mvec);
}

int main() {
  const long long C = kWideChunk;
  CHECK(C % 512 == 0 && (C == 2048 || C == 4096 || C == 8192), "chunk %lld", C);
  // the chunks of a system: every element in exactly one, every chunk but the last full, offsets multiples of the tile
  for (long long vlen : {1LL, 2LL, 513LL, C - 1, C, C + 1, 2 * C + 513, 3 * C, 1024 * C - 1, 1024 * C}) {
    const long long nc = wide_nchunk(vlen);
    CHECK(nc >= 1 && nc <= kWideMaxChunks && (nc - 1) * C < vlen && vlen <= nc * C, "nchunk %lld of vlen %lld", nc, vlen);
    long long covered = 0;
    for (long long c = 0; c < nc; c++) {
      const long long len = wide_chunk_len(vlen, c);
      CHECK(len >= 1 && len <= C && (c == nc - 1 || len == C), "chunk %lld of vlen %lld holds %lld", c, vlen, len);
      CHECK(c * C == covered, "chunk %lld of vlen %lld does not start where the last ended", c, vlen);
      covered += len;
    }
    CHECK(covered == vlen, "the chunks of vlen %lld cover %lld", vlen, covered);
  }
  for (int mvec = 1; mvec <= 32; mvec++) {
    const int m1 = mvec + 1;
    // the partial sums: every (sys, entry, chunk) cell its own, none left over
    for (int nchunk : {1, 2, 3, 17}) {
      const int nsys = 3;
      std::vector<int> pmap((size_t)wide_part_count(nsys, mvec, nchunk), 0);
      int tag = 0;
      for (int s = 0; s < nsys; s++)
        for (int e = 0; e < 2 + 2 * mvec; e++)
          for (int c = 0; c < nchunk; c++) {
            paint(pmap, wide_part_index(s, e, c, mvec, nchunk), 1, ++tag);
            if (c > 0) CHECK(wide_part_index(s, e, c, mvec, nchunk) == wide_part_index(s, e, c - 1, mvec, nchunk) + 1, "chunks of an entry lie together");
          }
      no_hole(pmap, "the partial sums", mvec);
    }
    CHECK(wide_part_index(65534, 1 + 2 * mvec, 1023, mvec, 1024) == wide_part_count(65535, mvec, 1024) - 1, "the last cell of the largest batch");
    for (int nchunk : {1, 5, 1024}) {
      // sums kernel
      const WideLds l = wide_sums_lds(mvec, nchunk);
      std::vector<int> dmap((size_t)l.ndouble, 0), imap((size_t)l.nint, 0);
      paint(dmap, l.stage, nchunk, 1);
      paint(dmap, l.sm, kBatchWaves * kBatchAcc, 2);
      paint(dmap, l.res, kBatchAcc + 1, 3);
      paint(imap, l.next, m1 + 1, 4);
      paint(imap, l.ps, m1, 5);
      paint(imap, l.hdr, 8, 6);
      no_hole(dmap, "the doubles of the sums kernel", mvec);
      no_hole(imap, "the int32 of the sums kernel", mvec);
      CHECK(l.bytes() == 8u * dmap.size() + 4u * imap.size() && 4 * l.bytes() <= 160u * 1024u, "LDS of the sums kernel: %zu bytes", l.bytes());
      // scalar kernel: the narrow kernel's pieces, then the stage, then the int32 pieces
      const WideScalarLds w = wide_scalar_lds(mvec, nchunk);
      const BatchLds &b = w.b;
      std::vector<int> sd((size_t)b.ndouble, 0), si((size_t)b.nint, 0);
      paint(sd, b.h, (long long)(m1 + 1) * (m1 + 1), 1);
      paint(sd, b.c, m1 + 1, 2);
      paint(sd, b.red, 2 + 2 * mvec, 3);
      paint(sd, b.cc, m1, 4);
      paint(sd, b.sm, kBatchWaves * kBatchAcc, 5);
      paint(sd, b.res, kBatchAcc + 1, 6);
      paint(sd, w.stage, nchunk, 7);
      paint(si, b.next, m1 + 1, 8);
      paint(si, b.prev, m1 + 1, 9);
      paint(si, b.ps, m1, 10);
      paint(si, b.cs, m1, 11);
      paint(si, b.hdr, 8, 12);
      no_hole(sd, "the doubles of the scalar kernel", mvec);
      no_hole(si, "the int32 of the scalar kernel", mvec);
      CHECK(b.bytes() == 8u * sd.size() + 4u * si.size() && b.bytes() <= 40u * 1024u, "LDS of the scalar kernel: %zu bytes", b.bytes());
    }
    const WideLds k = wide_combine_lds(mvec);
    std::vector<int> cd((size_t)k.ndouble, 0), ci((size_t)k.nint, 0);
    paint(cd, k.cc, m1, 1);
    paint(ci, k.cs, m1, 2);
    paint(ci, k.hdr, 8, 3);
    no_hole(cd, "the doubles of the combine kernel", mvec);
    no_hole(ci, "the int32 of the combine kernel", mvec);
    CHECK(k.bytes() == 8u * cd.size() + 4u * ci.size(), "LDS of the combine kernel");
  }
  if (failures) {
    std::fprintf(stderr, "batch_wide_layout_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("batch_wide_layout_check: chunks of a system, partial sums of three systems, LDS of the sums, scalar and combine kernels: OK\n");
  return 0;
}
