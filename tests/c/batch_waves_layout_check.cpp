// batch_waves_layout_check.cpp -- the layout arithmetic of the wave batch (nka_amd/csrc/host_logic.hpp: waves_lds, waves_ngroup,
// waves_k) against a brute-force model, built with the sanitizer flags of `make -C nka_amd/csrc hostcheck` and run by
// `make wavescheck` (tests/test_batch_waves_cpu.py).  For every mvec 1 ... 32: the four working copies painted piece by piece
// into a byte map -- no two pieces overlap, none leaves the 64 KiB a launch may ask for, every copy starts on 16 bytes and every
// double on 8 --; for every nsys 1 ... 4097 the grid covers every system and no workgroup is empty; waves_k against a count.
// It prints one line per mvec -- "waves mvec copy_bytes total_bytes" -- which the Python helper of the tests is held against.
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
    CHECK(i >= 0 && i < (long long)map.size(), "piece %d leaves the allocation at %lld of %zu", tag, i, map.size());
    if (i < 0 || i >= (long long)map.size()) return;
    CHECK(map[(size_t)i] == 0, "pieces %d and %d overlap at %lld", map[(size_t)i], tag, i);
    map[(size_t)i] = tag;
  }
}

int main() {
  static_assert(kWavesGroup == 4 && kWavesTile == 128, "four wavefronts, a pair per lane and tile");
  const long long limit = 64 * 1024;
  for (int mvec = 1; mvec <= 32; mvec++) {
    const int m1 = mvec + 1;
    const WavesLds L = waves_lds(mvec);
    const BatchLds &b = L.copy;
    CHECK(L.copy_bytes % 16 == 0 && L.copy_bytes >= (long long)b.bytes() && L.copy_bytes < (long long)b.bytes() + 16,
          "mvec %d: copy_bytes %lld against %zu", mvec, (long long)L.copy_bytes, b.bytes());
    CHECK(L.bytes() == 4 * L.copy_bytes && L.bytes() <= limit, "mvec %d: %lld bytes of LDS", mvec, (long long)L.bytes());
    std::vector<int> lds((size_t)L.bytes(), 0);
    for (int w = 0; w < kWavesGroup; w++) {
      const long long d0 = L.base(w), i0 = d0 + 8LL * b.ndouble;      // the kernel: shd = smem + base(w), shi = shd + ndouble
      CHECK(d0 % 16 == 0 && i0 % 8 == 0, "mvec %d: copy %d starts at %lld", mvec, w, d0);
      int tag = 100 * (w + 1);
      paint(lds, d0 + 8LL * b.h, 8LL * (m1 + 1) * (m1 + 1), ++tag);
      paint(lds, d0 + 8LL * b.c, 8LL * (m1 + 1), ++tag);
      paint(lds, d0 + 8LL * b.red, 8LL * (2 + 2 * mvec), ++tag);
      paint(lds, d0 + 8LL * b.cc, 8LL * m1, ++tag);
      paint(lds, d0 + 8LL * b.sm, 8LL * kBatchWaves * kBatchAcc, ++tag);      // (unused by this kind; part of the layout)
      paint(lds, d0 + 8LL * b.res, 8LL * (kBatchAcc + 1), ++tag);
      paint(lds, i0 + 4LL * b.next, 4LL * (m1 + 1), ++tag);
      paint(lds, i0 + 4LL * b.prev, 4LL * (m1 + 1), ++tag);
      paint(lds, i0 + 4LL * b.ps, 4LL * m1, ++tag);
      paint(lds, i0 + 4LL * b.cs, 4LL * m1, ++tag);
      paint(lds, i0 + 4LL * b.hdr, 4LL * 8, ++tag);
      // every byte of the copy's own extent that is painted carries this copy's tags
      for (long long i = d0; i < d0 + L.copy_bytes; i++)
        CHECK(lds[(size_t)i] == 0 || lds[(size_t)i] / 100 == w + 1, "mvec %d: copy %d holds a byte of copy %d", mvec, w, lds[(size_t)i] / 100 - 1);
    }
    std::printf("waves %d %lld %lld\n", mvec, (long long)L.copy_bytes, (long long)L.bytes());
  }
  // the grid: wavefront w of workgroup g owns system 4 g + w
  for (long long nsys = 1; nsys <= 4097; nsys++) {
    const long long g = waves_ngroup(nsys);
    CHECK(g * kWavesGroup >= nsys, "nsys %lld: %lld workgroups do not reach the last system", nsys, g);
    CHECK((g - 1) * kWavesGroup < nsys, "nsys %lld: the last of %lld workgroups is empty", nsys, g);
  }
  CHECK(waves_ngroup(2147483647LL) == 536870912LL, "the largest nsys");
  // waves_k: two fma per lane and tile, six levels
  for (long long n = 1; n <= 5000; n++) {
    long long tiles = 0;
    for (long long lo = 0; lo < n; lo += kWavesTile) tiles++;
    CHECK(waves_k(n) == 2 * tiles + 6, "waves_k(%lld) = %lld", n, (long long)waves_k(n));
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
