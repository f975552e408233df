// batch_lanes_layout_check.cpp -- the layout arithmetic of the lane batch (nka_amd/csrc/host_logic.hpp: lanes_lds, lanes_group,
// lanes_slot_offset, lanes_slot_alloc_elems, lanes_vector_bytes) against a brute-force model, built with the sanitizer flags of
// `make -C nka_amd/csrc hostcheck` and run by `make lanescheck` (tests/test_batch_lanes_cpu.py).  For every mvec 1 ... 32: the
// group size against the LDS budget, the working copies of all lanes painted byte by byte, the bank rule, the interleaved slots
// of three groups with a ragged last one painted element by element, and the largest legal arguments against __int128.
// It prints one line per mvec -- "lanes mvec G lane_bytes" -- which the Python helper of the tests is held against.
#include "../../nka_amd/csrc/host_logic.hpp"

#include <cstdio>
#include <set>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                                                                                                  \
  do {                                                                                                                    \
    if (!(cond)) {                                                                                                        \
      if (failures++ < 20) { std::fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
    }                                                                                                                     \
  } while (0)

using namespace nka_host;
typedef __int128 wide_t;

static void paint(std::vector<int> &map, long long off, long long len, int tag) {
  for (long long i = off; i < off + len; i++) {
    CHECK(i >= 0 && i < (long long)map.size(), "piece %d leaves the allocation at %lld of %zu", tag, i, map.size());
    if (i < 0 || i >= (long long)map.size()) return;
    CHECK(map[(size_t)i] == 0, "pieces %d and %d overlap at %lld", map[(size_t)i], tag, i);
    map[(size_t)i] = tag;
  }
}

int main() {
  static_assert(kLanesThreads == 64, "one wavefront");
  CHECK(kLanesLdsBudget <= 160 * 1024, "the LDS of a CU");
  std::set<int> sizes;
  for (int mvec = 1; mvec <= 32; mvec++) {
    const int m1 = mvec + 1, G = lanes_group(mvec);
    const LanesLds L = lanes_lds(mvec);
    sizes.insert(G);
    // ---- the group ----
    CHECK(G >= 1 && G <= kLanesThreads, "mvec %d: G = %d", mvec, G);
    CHECK(L.bytes(G) <= kLanesLdsBudget, "mvec %d: %lld bytes of LDS", mvec, (long long)L.bytes(G));
    CHECK(G == kLanesThreads || L.bytes(G + 1) > kLanesLdsBudget, "mvec %d: G = %d is not the largest that fits", mvec, G);
    // ---- the bank rule: odd strides, and hence 32 lanes of a group on 32 distinct banks, at any common offset ----
    CHECK(L.dstride % 2 == 1 && L.istride % 2 == 1, "mvec %d: strides %d, %d are not odd", mvec, L.dstride, L.istride);
    CHECK(L.dstride >= L.ndouble && L.istride >= L.nint, "mvec %d: a copy does not fit its stride", mvec);
    for (int half = 0; half < 2; half++) {
      std::set<long long> b64, b32;
      const long long ibytes0 = 8LL * G * L.dstride;
      for (int l = 32 * half; l < 32 * (half + 1) && l < G; l++) {
        b64.insert((8 * L.dbase(l) / 4) % 64);              // ds_read_b64: bank (a / 4) mod 64 of the first dword; the pair is (b, b + 1)
        b32.insert(((ibytes0 + 4 * L.ibase(l)) / 4) % 32);  // ds_read_b32: bank (a / 4) mod 32
      }
      const size_t want = (size_t)std::max(0, std::min(32, G - 32 * half));
      CHECK(b64.size() == want && b32.size() == want, "mvec %d: lanes of one group share a bank", mvec);
      for (long long b : b64) CHECK(b % 2 == 0, "an 8-byte access starts on an even dword");
    }
    // ---- the working copies of all lanes, byte by byte ----
    std::vector<int> lds((size_t)L.bytes(G), 0);
    const long long ibytes0 = 8LL * G * L.dstride;
    for (int l = 0; l < G; l++) {
      const long long d0 = 8 * L.dbase(l), i0 = ibytes0 + 4 * L.ibase(l);
      int tag = 100 * (l + 1);
      paint(lds, d0 + 8LL * L.h, 8LL * (m1 + 1) * (m1 + 1), tag + 1);
      paint(lds, d0 + 8LL * L.c, 8LL * (m1 + 1), tag + 2);
      paint(lds, d0 + 8LL * L.red, 8LL * (2 + 2 * mvec), tag + 3);
      paint(lds, d0 + 8LL * L.cc, 8LL * m1, tag + 4);
      paint(lds, i0 + 4LL * L.next, 4LL * (m1 + 1), tag + 5);
      paint(lds, i0 + 4LL * L.prev, 4LL * (m1 + 1), tag + 6);
      paint(lds, i0 + 4LL * L.ps, 4LL * m1, tag + 7);
      paint(lds, i0 + 4LL * L.cs, 4LL * m1, tag + 8);
      paint(lds, i0 + 4LL * L.hdr, 4LL * 8, tag + 9);
      CHECK(d0 % 8 == 0 && i0 % 4 == 0, "alignment");
    }
    CHECK(kLanesHdrLive >= 6 && kLanesHdrLive < 8, "the live flag lies inside hdr, behind the HDR_ entries");
    // ---- the interleaved slots of three groups, the last one ragged, element by element ----
    for (long long vlen : {1LL, 2LL, 7LL, 33LL, 64LL}) {
      const long long nsys = 2LL * G + (G > 1 ? G / 2 : 1);      // the last group holds fewer systems than G (or G = 1)
      const long long elems = lanes_slot_alloc_elems(vlen, mvec, G, nsys);
      CHECK(lanes_ngroup(nsys, G) == 3, "three groups");
      CHECK(elems == 3LL * m1 * vlen * G, "the last group is allocated whole");
      CHECK(lanes_vector_bytes(vlen, mvec, G, nsys) == 16 * elems, "both allocations, in bytes");
      std::vector<int> map((size_t)elems, 0);
      for (long long s = 0; s < nsys; s++)
        for (int k = 1; k <= m1; k++)
          for (long long i = 0; i < vlen; i++) {
            const long long off = lanes_slot_offset(vlen, mvec, G, s, k, i);
            paint(map, off, 1, (int)(s * 64 + k));
            // what the kernel forms: the group's base, the lane, and ((k - 1) vlen + i) G
            CHECK(off == (s / G) * lanes_group_stride(vlen, mvec, G) + s % G + ((k - 1) * vlen + i) * G, "the kernel's form of the offset");
            if (s % G != 0) CHECK(off == lanes_slot_offset(vlen, mvec, G, s - 1, k, i) + 1, "the lanes of a group are not contiguous");
          }
    }
    std::printf("lanes %d %d %lld\n", mvec, G, (long long)L.lane_bytes());
  }
  CHECK(sizes.count(64) == 1, "no mvec runs a full wavefront");
  {
    int odd_small = 0;
    for (int g : sizes) if (g < 64 && (g & (g - 1)) != 0) odd_small++;
    CHECK(odd_small >= 2, "the tests want two group sizes below 64 that are no power of two");
  }
  // ---- the largest legal arguments: every offset and size inside int64, equal to the model in __int128 ----
  struct Big { long long nsys, vlen; int mvec; };
  for (const Big &g : {Big{2147483647LL, 64, 32}, Big{2147483647LL, 64, 1}, Big{2147483647LL, 1, 1}, Big{254204, 64, 32}, Big{70001, 8, 3}}) {
    const int G = lanes_group(g.mvec);
    const wide_t m1 = g.mvec + 1, ng = ((wide_t)g.nsys + G - 1) / G;
    const wide_t want = ng * m1 * g.vlen * G, lim = (wide_t)INT64_MAX;
    CHECK(16 * want <= lim, "the model itself leaves int64");
    CHECK((wide_t)lanes_slot_alloc_elems(g.vlen, g.mvec, G, g.nsys) == want, "allocation, large");
    CHECK((wide_t)lanes_vector_bytes(g.vlen, g.mvec, G, g.nsys) == 16 * want, "bytes, large");
    const wide_t last = ((((wide_t)(g.nsys - 1) / G) * m1 + (m1 - 1)) * g.vlen + (g.vlen - 1)) * G + (g.nsys - 1) % G;
    CHECK((wide_t)lanes_slot_offset(g.vlen, g.mvec, G, g.nsys - 1, g.mvec + 1, g.vlen - 1) == last, "the last element, large");
    CHECK(last < want, "the last element lies inside");
  }
  if (failures) {
    std::fprintf(stderr, "batch_lanes_layout_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("batch_lanes_layout_check: group sizes, LDS copies byte by byte, the bank rule, interleaved slots of three groups, the largest arguments: OK\n");
  return 0;
}
