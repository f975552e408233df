// batch_waves_rows_layout_check.cpp -- the LDS of the wave batch's kernel with the scalar step on the whole wavefront
// (nka_amd/csrc/host_logic.hpp: waves_rows_lds, waves_rows_max_mvec, waves_rows_nlmax; nka_hip_batch_create_waves_rows), built with
// the sanitizer flags of `make -C nka_amd/csrc hostcheck` (target wavesrowscheck; tests/test_batch_waves_rows_cpu.py runs it).  For
// every mvec 1 ... cap every byte of every piece of all four wavefronts -- the working copy and the matrix behind it -- is painted
// into a map and collisions are counted, instead of trusting the closed forms; the copy's pieces must lie where waves_lds puts
// them, so that the text ahead of and behind phase 4 reads the same cells.  THE CAP IS DERIVED: the layout fits 64 KiB at the cap
// and does not at cap + 1.  It prints "cap N" and one line per mvec, "waves_rows mvec copy_bytes a_bytes total_bytes".
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
  static_assert(kWavesGroup == 4, "four wavefronts");
  constexpr int cap = waves_rows_max_mvec();
  const long long limit = 64 * 1024;
  CHECK(kWavesRowsLdsLimit == limit, "the dynamic LDS a launch may ask for without a function attribute");
  CHECK(cap >= 1 && cap <= 32, "the cap %d lies inside the batch's range of mvec", cap);
  CHECK(waves_rows_lds(cap).bytes() <= limit, "%lld bytes at the cap %d", (long long)waves_rows_lds(cap).bytes(), cap);
  CHECK(waves_rows_lds(cap + 1).bytes() > limit, "%lld bytes at %d: the cap is not the last that fits", (long long)waves_rows_lds(cap + 1).bytes(), cap + 1);
  std::printf("cap %d\n", cap);
  for (int mvec = 1; mvec <= cap + 1; mvec++) {      // (cap + 1: the layout itself is sound there too; it only does not fit)
    const int m1 = mvec + 1;
    const WavesRowsLds L = waves_rows_lds(mvec);
    const WavesLds one = waves_lds(mvec);
    const BatchLds &b = L.copy;
    const int nl = waves_rows_nlmax(mvec);
    if (mvec <= cap) {
      CHECK(nl >= m1 && nl <= kWideRowsMaxList && (nl == 6 || nl == 11 || nl == 21 || nl == cap + 1), "mvec %d runs the instance of %d rows", mvec, nl);
      if (mvec > 1) CHECK(waves_rows_nlmax(mvec - 1) <= nl, "the instances grow with mvec");
      CHECK(L.bytes() <= limit, "mvec %d: %lld bytes of LDS", mvec, (long long)L.bytes());
    }
    if (mvec > 1) CHECK(L.bytes() > waves_rows_lds(mvec - 1).bytes(), "the size grows with mvec (the cap is found by walking up)");
    CHECK(L.copy_bytes == one.copy_bytes && L.copy_bytes % 16 == 0, "mvec %d: the copy is that of waves_lds", mvec);
    CHECK(L.a_bytes % 16 == 0 && L.a_bytes >= 8LL * (m1 + 1) * (m1 + 1) && L.a_bytes < 8LL * (m1 + 1) * (m1 + 1) + 16,
          "mvec %d: a_bytes %lld", mvec, (long long)L.a_bytes);
    CHECK(L.stride_bytes() == L.copy_bytes + L.a_bytes && L.bytes() == 4 * L.stride_bytes(), "mvec %d: the same copy, then the matrix, four times", mvec);
    CHECK(b.h == one.copy.h && b.c == one.copy.c && b.red == one.copy.red && b.cc == one.copy.cc && b.sm == one.copy.sm && b.res == one.copy.res &&
              b.ndouble == one.copy.ndouble, "a double piece moved at mvec %d", mvec);
    CHECK(b.next == one.copy.next && b.prev == one.copy.prev && b.ps == one.copy.ps && b.cs == one.copy.cs && b.hdr == one.copy.hdr &&
              b.nint == one.copy.nint, "an int32 piece moved at mvec %d", mvec);
    std::vector<int> lds((size_t)L.bytes(), 0);
    for (int w = 0; w < kWavesGroup; w++) {
      const long long d0 = L.base(w), i0 = d0 + 8LL * b.ndouble, a0 = L.a_base(w);      // the kernel: shd, shi = shd + ndouble, A
      CHECK(d0 % 16 == 0 && i0 % 8 == 0 && a0 % 16 == 0, "mvec %d: copy %d starts at %lld, its matrix at %lld", mvec, w, d0, a0);
      CHECK(a0 == d0 + L.copy_bytes && a0 >= i0 + 4LL * b.nint, "mvec %d: the matrix of wavefront %d starts behind its copy", mvec, w);
      int tag = 100 * (w + 1);
      paint(lds, d0 + 8LL * b.h, (m1 + 1) * (m1 + 1), 8, ++tag);
      paint(lds, d0 + 8LL * b.c, m1 + 1, 8, ++tag);
      paint(lds, d0 + 8LL * b.red, 2 + 2 * mvec, 8, ++tag);
      paint(lds, d0 + 8LL * b.cc, m1, 8, ++tag);
      paint(lds, d0 + 8LL * b.sm, kBatchWaves * kBatchAcc, 8, ++tag);      // (unused by this kind; part of the layout)
      paint(lds, d0 + 8LL * b.res, kBatchAcc + 1, 8, ++tag);
      paint(lds, i0 + 4LL * b.next, m1 + 1, 4, ++tag);
      paint(lds, i0 + 4LL * b.prev, m1 + 1, 4, ++tag);
      paint(lds, i0 + 4LL * b.ps, m1, 4, ++tag);
      paint(lds, i0 + 4LL * b.cs, m1, 4, ++tag);
      paint(lds, i0 + 4LL * b.hdr, 8, 4, ++tag);
      paint(lds, a0, (m1 + 1) * (m1 + 1), 8, ++tag);      // rows 0 ... nl <= m1, LDA = m1 + 1; the last word takes the dump
      // every painted byte of the wavefront's own extent carries this wavefront's tags
      for (long long i = d0; i < d0 + L.stride_bytes(); i++)
        CHECK(lds[(size_t)i] == 0 || lds[(size_t)i] / 100 == w + 1, "mvec %d: wavefront %d holds a byte of wavefront %d", mvec, w, lds[(size_t)i] / 100 - 1);
    }
    // the largest index the device function forms in the matrix: row nl = m1 of LDA = m1 + 1, column m1
    CHECK((long long)m1 * (m1 + 1) + m1 == (long long)(m1 + 1) * (m1 + 1) - 1, "the dump word is the last of the matrix");
    std::printf("waves_rows %d %lld %lld %lld\n", mvec, (long long)L.copy_bytes, (long long)L.a_bytes, (long long)L.bytes());
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch_waves_rows_layout_check: OK (cap %d: %lld bytes, %d: %lld; mvec 20: %lld)\n", cap, (long long)waves_rows_lds(cap).bytes(), cap + 1,
              (long long)waves_rows_lds(cap + 1).bytes(), (long long)waves_rows_lds(20).bytes());
  return 0;
}
