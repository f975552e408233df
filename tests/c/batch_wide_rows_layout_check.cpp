// batch_wide_rows_layout_check.cpp -- the LDS of the wide batch's scalar kernel with the scalar step on one wavefront
// (nka_amd/csrc/host_logic.hpp: wide_scalar_rows_lds, wide_rows_nlmax; nka_hip_batch_set_scalar_step), built with the sanitizer
// flags of `make -C nka_amd/csrc hostcheck` (target widerowscheck; tests/test_batch_wide_rows_cpu.py runs it).  Every byte of every
// piece is painted into a map and collisions are counted, instead of trusting the closed forms; the pieces it shares with the
// one-thread kernel must lie where wide_scalar_lds puts them, so that the text ahead of and behind phase 4 reads the same cells.
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

// `count` elements of `size` bytes from byte `at`
static void paint(std::vector<int> &map, long long at, long long count, int size, int tag) {
  CHECK(at >= 0 && at + count * size <= (long long)map.size(), "piece %d leaves the LDS: %lld + %lld x %d of %zu", tag, at, count, size, map.size());
  CHECK(at % size == 0, "piece %d is not aligned to %d bytes at %lld", tag, size, at);
  for (long long i = at; i < at + count * size && i >= 0 && i < (long long)map.size(); i++) {
    CHECK(map[(size_t)i] == 0, "pieces %d and %d overlap at byte %lld", map[(size_t)i], tag, i);
    map[(size_t)i] = tag;
  }
}

int main() {
  size_t largest = 0;
  for (int mvec = 1; mvec <= 32; mvec++) {
    const int m1 = mvec + 1;
    const int nl = wide_rows_nlmax(mvec);
    CHECK(nl >= m1 && nl <= kWideRowsMaxList && (nl == 6 || nl == 11 || nl == 21 || nl == 33), "mvec %d runs the instance of %d rows", mvec, nl);
    if (mvec > 1) CHECK(wide_rows_nlmax(mvec - 1) <= nl, "the instances grow with mvec");
    for (int nchunk : {1, 2, 257, 512, kWideMaxChunks}) {
      const WideScalarRowsLds l = wide_scalar_rows_lds(mvec, nchunk);
      const WideScalarLds one = wide_scalar_lds(mvec, nchunk);
      const BatchLds &b = l.b;
      std::vector<int> map(b.bytes(), 0);
      const long long ints = 8LL * b.ndouble;      // the int32 pieces start behind all doubles
      paint(map, 8LL * b.h, (m1 + 1) * (m1 + 1), 8, 1);
      paint(map, 8LL * b.c, m1 + 1, 8, 2);
      paint(map, 8LL * b.red, 2 + 2 * mvec, 8, 3);
      paint(map, 8LL * b.cc, m1, 8, 4);
      paint(map, 8LL * b.sm, kBatchWaves * kBatchAcc, 8, 5);
      paint(map, 8LL * b.res, kBatchAcc + 1, 8, 6);
      paint(map, 8LL * l.stage, nchunk, 8, 7);
      paint(map, 8LL * l.a, (m1 + 1) * (m1 + 1), 8, 8);      // rows 0 ... nl <= m1, LDA = m1 + 1; the last word takes the dump
      paint(map, ints + 4LL * b.next, m1 + 1, 4, 9);
      paint(map, ints + 4LL * b.prev, m1 + 1, 4, 10);
      paint(map, ints + 4LL * b.ps, m1, 4, 11);
      paint(map, ints + 4LL * b.cs, m1, 4, 12);
      paint(map, ints + 4LL * b.hdr, 8, 4, 13);
      for (size_t i = 0; i < map.size(); i++) CHECK(map[i] != 0, "a hole at byte %zu (mvec %d, %d chunks)", i, mvec, nchunk);
      CHECK(b.bytes() <= 64 * 1024, "%zu bytes at mvec %d, %d chunks: more than a launch may ask for without a function attribute", b.bytes(), mvec, nchunk);
      // the largest index the device function forms in the matrix: row nl = m1 of LDA = m1 + 1, column m1
      CHECK((long long)m1 * (m1 + 1) + m1 == (long long)(m1 + 1) * (m1 + 1) - 1, "the dump word is the last of the matrix");
      // what the two kernels share lies where it lay: the doubles up to and including the stage, and every int32 offset
      CHECK(b.h == one.b.h && b.c == one.b.c && b.red == one.b.red && b.cc == one.b.cc && b.sm == one.b.sm && b.res == one.b.res &&
                l.stage == one.stage, "a double piece moved at mvec %d", mvec);
      CHECK(b.next == one.b.next && b.prev == one.b.prev && b.ps == one.b.ps && b.cs == one.b.cs && b.hdr == one.b.hdr && b.nint == one.b.nint,
            "an int32 piece moved at mvec %d", mvec);
      CHECK(b.ndouble == one.b.ndouble + (m1 + 1) * (m1 + 1), "the matrix is all that was added");
      if (b.bytes() > largest) largest = b.bytes();
    }
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch_wide_rows_layout_check: OK (mvec 20: %zu bytes at 32 chunks, %zu at 512; mvec 32: %zu at 512, %zu at 1024, the largest %zu)\n",
              wide_scalar_rows_lds(20, 32).b.bytes(), wide_scalar_rows_lds(20, 512).b.bytes(), wide_scalar_rows_lds(32, 512).b.bytes(),
              wide_scalar_rows_lds(32, 1024).b.bytes(), largest);
  return 0;
}
