// batch_wide_step_layout_check.cpp -- the one buffer the solve step of a wide batch adds (nka_amd/csrc/host_logic.hpp:
// wide_fpart_count, wide_fpart_index: one partial of <f,f> per system and chunk) against a brute-force model, and the layout of
// the partial sums of every wide batch restated as it was before the step existed, built with the sanitizer flags of
// `make -C nka_amd/csrc hostcheck` (tests/test_batch_wide_step_cpu.py runs it).  Every cell is painted into a map and
// collisions are counted, instead of trusting the closed forms.
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

static void paint(std::vector<int> &map, long long off, int tag) {
  CHECK(off >= 0 && off < (long long)map.size(), "cell %d leaves the buffer at %lld of %zu", tag, off, map.size());
  if (off < 0 || off >= (long long)map.size()) return;
  CHECK(map[(size_t)off] == 0, "cells %d and %d overlap at %lld", map[(size_t)off], tag, off);
  map[(size_t)off] = tag;
}

// what the two functions of the partial sums returned before the step was added, written out
static long long part_count_before(long long nsys, int mvec, long long nchunk) { return nsys * (2 + 2 * mvec) * nchunk; }
static long long part_index_before(long long sys, int entry, long long c, int mvec, long long nchunk) {
  return (sys * (2 + 2 * mvec) + entry) * nchunk + c;
}

int main() {
  for (int nchunk : {1, 2, 9, 257, 512}) {
    for (int nsys : {1, 3, 6}) {
      // fpart: every (sys, chunk) cell hit once, none outside nsys x nchunk, the chunks of a system together and in order
      std::vector<int> fmap((size_t)wide_fpart_count(nsys, nchunk), 0);
      CHECK((long long)fmap.size() == (long long)nsys * nchunk, "fpart holds %zu cells for %d x %d", fmap.size(), nsys, nchunk);
      int tag = 0;
      for (int s = 0; s < nsys; s++)
        for (int c = 0; c < nchunk; c++) {
          paint(fmap, wide_fpart_index(s, c, nchunk), ++tag);
          if (c > 0) CHECK(wide_fpart_index(s, c, nchunk) == wide_fpart_index(s, c - 1, nchunk) + 1, "the chunks of a system lie together");
        }
      for (int x : fmap) CHECK(x != 0, "a hole in fpart at %d x %d", nsys, nchunk);
      // a system with a length of its own adds its first chunks only: they are its own cells
      for (int s = 0; s < nsys; s++)
        for (int nown = 1; nown <= nchunk; nown += (nchunk > 16 ? 37 : 1))
          CHECK(wide_fpart_index(s, nown - 1, nchunk) < wide_fpart_index(s, 0, nchunk) + nchunk, "system %d reads beyond its cells", s);
      // the partial sums of every wide batch: the values of before
      for (int mvec : {1, 3, 10, 20, 32}) {
        CHECK(wide_part_count(nsys, mvec, nchunk) == part_count_before(nsys, mvec, nchunk), "wide_part_count moved at mvec %d", mvec);
        for (int s = 0; s < nsys; s++)
          for (int e = 0; e < 2 + 2 * mvec; e++)
            for (int c = 0; c < nchunk; c++)
              CHECK(wide_part_index(s, e, c, mvec, nchunk) == part_index_before(s, e, c, mvec, nchunk), "wide_part_index moved at (%d, %d, %d)", s, e, c);
      }
    }
  }
  // the largest batch: the last cell is the last of the buffer, inside 64 bits
  CHECK(wide_fpart_index(65534, 1023, 1024) == wide_fpart_count(65535, 1024) - 1, "the last cell of the largest batch");
  CHECK(wide_part_index(65534, 65, 1023, 32, 1024) == part_count_before(65535, 32, 1024) - 1, "the last partial of the largest batch");
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch_wide_step_layout_check: OK\n");
  return 0;
}
