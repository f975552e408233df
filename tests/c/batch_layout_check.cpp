// batch_layout_check.cpp -- the layout arithmetic of the batched accelerator (nka_amd/csrc/host_logic.hpp: batch_layout,
// batch_lds, batch_ic_count / batch_dc_count) against brute-force models, built with the sanitizer flags of
// `make -C nka_amd/csrc hostcheck` (tests/test_batch_cpu.py runs it).  The models paint every element a piece owns into a
// map and count collisions, instead of trusting the closed forms.
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

// paint [off, off + len) of `map` with `tag`; a cell painted twice is a collision
static void paint(std::vector<int> &map, long long off, long long len, int tag) {
  for (long long i = off; i < off + len; i++) {
    CHECK(i >= 0 && i < (long long)map.size(), "piece %d leaves the block at %lld of %zu", tag, i, map.size());
    if (i < 0 || i >= (long long)map.size()) return;
    CHECK(map[(size_t)i] == 0, "pieces %d and %d overlap at %lld", map[(size_t)i], tag, i);
    map[(size_t)i] = tag;
  }
}

int main() {
  for (int mvec = 1; mvec <= 32; mvec++) {
    const int m1 = mvec + 1;
    // the control block, piece by piece as Ctl lays it out (nka_ctl.hpp)
    int ic = 0, dc = 0;
    ic += 16; ic += m1 + 1; ic += m1 + 1; ic += m1 + kMaxPerPass; ic += m1 + kMaxPerPass;
    dc += 2; for (int i = 0; i <= m1; i++) for (int j = 0; j <= m1; j++) dc++;
    dc += m1 + 1; dc += m1 + kMaxPerPass; dc += 2 + 2 * mvec; dc += 16;
    CHECK(ic == batch_ic_count(mvec) && dc == batch_dc_count(mvec), "control block counts at mvec %d", mvec);

    // LDS of a workgroup: every piece inside, none overlapping, doubles 8-byte aligned, four workgroups per CU (160 KiB)
    const BatchLds l = batch_lds(mvec);
    std::vector<int> dmap((size_t)l.ndouble, 0), imap((size_t)l.nint, 0);
    paint(dmap, l.h, (long long)(m1 + 1) * (m1 + 1), 1);
    paint(dmap, l.c, m1 + 1, 2);
    paint(dmap, l.red, 2 + 2 * mvec, 3);
    paint(dmap, l.cc, m1, 4);
    paint(dmap, l.sm, kBatchWaves * kBatchAcc, 5);
    paint(dmap, l.res, kBatchAcc + 1, 6);
    paint(imap, l.next, m1 + 1, 7);
    paint(imap, l.prev, m1 + 1, 8);
    paint(imap, l.ps, m1, 9);
    paint(imap, l.cs, m1, 10);
    paint(imap, l.hdr, 8, 11);
    for (int x : dmap) CHECK(x != 0, "a hole in the doubles at mvec %d", mvec);
    for (int x : imap) CHECK(x != 0, "a hole in the int32 at mvec %d", mvec);
    CHECK(l.bytes() == 8u * dmap.size() + 4u * imap.size(), "bytes at mvec %d", mvec);
    CHECK(4 * l.bytes() <= 160u * 1024u, "four workgroups do not fit a CU at mvec %d: %zu bytes each", mvec, l.bytes());

    for (long long vlen : {1LL, 2LL, 7LL, 31LL, 32LL, 33LL, 64LL, 65LL, 257LL, 700LL, 4099LL, 65535LL, 65536LL}) {
      const BatchLayout L = batch_layout(vlen, mvec);
      CHECK(L.stride >= vlen && L.stride % 32 == 0 && L.stride - vlen < 32, "slot stride %lld for vlen %lld", (long long)L.stride, vlen);
      CHECK(L.sys_stride == L.stride * m1 && L.sys_stride % 32 == 0, "system stride");
      CHECK(L.ic_stride >= ic && L.ic_stride % 32 == 0 && L.ic_stride - ic < 32, "ic stride %d for %d", L.ic_stride, ic);
      CHECK(L.dc_stride >= dc && L.dc_stride % 32 == 0 && L.dc_stride - dc < 32, "dc stride %d for %d", L.dc_stride, dc);
      if (vlen <= 700) {      // three systems, every slot of each painted into one allocation
        const int nsys = 3;
        std::vector<int> vmap((size_t)(L.sys_stride * nsys), 0);
        for (int s = 0; s < nsys; s++)
          for (int k = 1; k <= m1; k++) paint(vmap, s * L.sys_stride + (k - 1) * L.stride, vlen, 100 * s + k);
        std::vector<int> cmap((size_t)L.ic_stride * nsys, 0), emap((size_t)L.dc_stride * nsys, 0);
        for (int s = 0; s < nsys; s++) {
          paint(cmap, (long long)s * L.ic_stride, ic, s + 1);
          paint(emap, (long long)s * L.dc_stride, dc, s + 1);
        }
      }
    }
  }
  if (failures) {
    std::fprintf(stderr, "batch_layout_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("batch_layout_check: control block counts, strides, slots of three systems, LDS pieces: OK\n");
  return 0;
}
