// batch_rows_layout_check.cpp -- the LDS of the narrow batch's kernel with the scalar step on wavefront 0 (nka_amd/csrc/
// host_logic.hpp: batch_rows_lds, batch_rows_nlmax; nka_hip_batch_create_rows), built with the sanitizer flags of
// `make -C nka_amd/csrc hostcheck` (target rowscheck; tests/test_batch_rows_cpu.py runs it).  For every mvec 1 ... 32 every byte of
// every piece -- the working copy of batch_lds and the matrix behind it -- is painted into a map and collisions are counted,
// instead of trusting the closed forms: no two pieces overlap, doubles lie on 8 bytes, the matrix on 16, and every piece of the
// working copy lies where batch_lds puts it, so that the phases around phase 4 read the same cells in either instance.  It
// prints one line per mvec, "rows mvec copy_bytes a_off a_bytes total_bytes nlmax".
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
  const int cap = 32;      // = NKA_HIP_BATCH_MAX_MVEC (include/nka_hip_batch.h): no cap of its own
  const long long limit = 40 * 1024;      // four workgroups per CU by LDS (160 KiB)
  for (int mvec = 1; mvec <= cap; mvec++) {
    const int m1 = mvec + 1;
    const BatchRowsLds L = batch_rows_lds(mvec);
    const BatchLds one = batch_lds(mvec);
    const BatchLds &b = L.b;
    const int nl = batch_rows_nlmax(mvec);
    CHECK(nl >= m1 && (nl == 11 || nl == 21 || nl == 33) && nl <= kWideRowsMaxList, "mvec %d runs the instance of %d rows", mvec, nl);
    CHECK(nl == (m1 <= 11 ? 11 : m1 <= 21 ? 21 : 33), "mvec %d: the smallest instance that holds the list, not %d", mvec, nl);
    if (mvec > 1) CHECK(batch_rows_nlmax(mvec - 1) <= nl, "the instances grow with mvec");
    CHECK(L.bytes() <= limit, "mvec %d: %lld bytes of LDS", mvec, (long long)L.bytes());
    if (mvec > 1) CHECK(L.bytes() > batch_rows_lds(mvec - 1).bytes(), "the size grows with mvec");
    // the working copy: the pieces of batch_lds, at its offsets
    CHECK(b.h == one.h && b.c == one.c && b.red == one.red && b.cc == one.cc && b.sm == one.sm && b.res == one.res && b.ndouble == one.ndouble,
          "a double piece moved at mvec %d", mvec);
    CHECK(b.next == one.next && b.prev == one.prev && b.ps == one.ps && b.cs == one.cs && b.hdr == one.hdr && b.nint == one.nint,
          "an int32 piece moved at mvec %d", mvec);
    CHECK(b.bytes() == one.bytes(), "mvec %d: the copy is that of batch_lds", mvec);
    const long long i0 = 8LL * b.ndouble, a0 = L.a_off;      // the kernel: shd = smem, shi = shd + ndouble, A = smem + a_off
    CHECK(a0 % 16 == 0 && a0 >= (long long)one.bytes() && a0 < (long long)one.bytes() + 16, "mvec %d: the matrix starts at %lld behind %zu bytes", mvec, a0, one.bytes());
    CHECK(L.a_bytes == 8LL * (m1 + 1) * (m1 + 1) && L.bytes() == a0 + L.a_bytes, "mvec %d: a_bytes %lld", mvec, (long long)L.a_bytes);
    std::vector<int> lds((size_t)L.bytes(), 0);
    int tag = 0;
    paint(lds, 8LL * b.h, (m1 + 1) * (m1 + 1), 8, ++tag);
    paint(lds, 8LL * b.c, m1 + 1, 8, ++tag);
    paint(lds, 8LL * b.red, 2 + 2 * mvec, 8, ++tag);
    paint(lds, 8LL * b.cc, m1, 8, ++tag);
    paint(lds, 8LL * b.sm, kBatchWaves * kBatchAcc, 8, ++tag);
    paint(lds, 8LL * b.res, kBatchAcc + 1, 8, ++tag);
    paint(lds, i0 + 4LL * b.next, m1 + 1, 4, ++tag);
    paint(lds, i0 + 4LL * b.prev, m1 + 1, 4, ++tag);
    paint(lds, i0 + 4LL * b.ps, m1, 4, ++tag);
    paint(lds, i0 + 4LL * b.cs, m1, 4, ++tag);
    paint(lds, i0 + 4LL * b.hdr, 8, 4, ++tag);
    const int atag = ++tag;
    paint(lds, a0, (m1 + 1) * (m1 + 1), 8, atag);      // rows 0 ... nl <= m1, LDA = m1 + 1; the last word takes the dump
    for (long long i = 0; i < (long long)one.bytes(); i++) CHECK(lds[(size_t)i] != atag, "mvec %d: the matrix reaches into the working copy at byte %lld", mvec, i);
    for (long long i = 0; i < (long long)one.bytes(); i++) CHECK(lds[(size_t)i] != 0, "mvec %d: byte %lld of the working copy belongs to no piece", mvec, i);
    // the largest index the device function forms in the matrix: row nl = m1 of LDA = m1 + 1, column m1
    CHECK((long long)m1 * (m1 + 1) + m1 == (long long)(m1 + 1) * (m1 + 1) - 1, "the dump word is the last of the matrix");
    std::printf("rows %d %zu %lld %lld %lld %d\n", mvec, one.bytes(), a0, (long long)L.a_bytes, (long long)L.bytes(), nl);
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch_rows_layout_check: OK (mvec 5: %lld bytes, 10: %lld, 20: %lld, 32: %lld)\n", (long long)batch_rows_lds(5).bytes(),
              (long long)batch_rows_lds(10).bytes(), (long long)batch_rows_lds(20).bytes(), (long long)batch_rows_lds(32).bytes());
  return 0;
}
