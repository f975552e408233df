// batch_store32_check.cpp -- the layout arithmetic of a batch with binary32 storage (nka_amd/csrc/host_logic.hpp:
// batch_slot_offset, batch_pending_offset, batch_slot_alloc_bytes, batch_pending_alloc_bytes, batch_vector_bytes) against a
// brute-force layout, built with the sanitizer flags of `make -C nka_amd/csrc hostcheck` (tests/test_batch_store32_cpu.py runs
// it).  Small shapes are painted byte by byte; the largest legal arguments are held against the same formulas in __int128.
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
typedef __int128 wide_t;

// paint bytes [off, off + len) of an allocation of map.size() bytes; a byte painted twice is a collision
static void paint(std::vector<int> &map, long long off, long long len, int tag) {
  for (long long i = off; i < off + len; i++) {
    CHECK(i >= 0 && i < (long long)map.size(), "piece %d leaves the allocation at byte %lld of %zu", tag, i, map.size());
    if (i < 0 || i >= (long long)map.size()) return;
    CHECK(map[(size_t)i] == 0, "pieces %d and %d overlap at byte %lld", map[(size_t)i], tag, i);
    map[(size_t)i] = tag;
  }
}

int main() {
  CHECK(batch_slot_elem_bytes(kBatchStoreF64) == 8 && batch_slot_elem_bytes(kBatchStoreF32) == 4, "element sizes");
  // ---- small shapes, byte by byte: three systems, both storages ----
  for (int mvec : {1, 2, 6, 10, 20, 32})
    for (long long vlen : {1LL, 2LL, 31LL, 32LL, 33LL, 63LL, 65LL, 513LL, 700LL})
      for (int storage : {kBatchStoreF64, kBatchStoreF32}) {
        const int nsys = 3, m1 = mvec + 1;
        const BatchLayout L = batch_layout(vlen, mvec);
        const long long eb = batch_slot_elem_bytes(storage);
        const long long slot_bytes = batch_slot_alloc_bytes(L, nsys, storage), pend_bytes = batch_pending_alloc_bytes(L, nsys, storage);
        CHECK(slot_bytes == eb * nsys * m1 * L.stride, "slot allocation");
        CHECK(pend_bytes == (storage == kBatchStoreF32 ? 8LL * nsys * L.stride : 0LL), "pending allocation");
        CHECK(batch_vector_bytes(L, nsys, storage) == 2 * slot_bytes + 2 * pend_bytes, "total");
        CHECK(batch_vector_bytes(L, nsys, storage) == 2LL * nsys * L.stride * (storage == kBatchStoreF32 ? 4 * m1 + 8 : 8 * m1),
              "the formula of the header");
        std::vector<int> smap((size_t)slot_bytes, 0), pmap((size_t)pend_bytes, 0);
        for (int s = 0; s < nsys; s++) {
          for (int k = 1; k <= m1; k++) {
            const long long off = batch_slot_offset(L, s, k) * eb;
            paint(smap, off, vlen * eb, 100 * s + k);
            CHECK(off % 128 == 0, "a slot row is not 128-byte aligned: %lld", off);      // hence every pair (2t, 2t + 1) on 2 * eb bytes
            for (long long i = 0; i + 1 < vlen; i += 2) CHECK((off + i * eb) % (2 * eb) == 0, "pair %lld of a slot row", i);
          }
          if (storage == kBatchStoreF32) {
            const long long off = batch_pending_offset(L, s) * 8;
            paint(pmap, off, vlen * 8, 1000 + s);
            CHECK(off % 256 == 0, "a pending row is not 256-byte aligned: %lld", off);
          }
        }
      }
  // ---- the largest legal arguments, and a batch beyond 2^31 elements and 2^32 bytes: every offset and size inside int64 ----
  struct Big { long long nsys, vlen; int mvec; };
  for (const Big &g : {Big{3976, 16384, 32}, Big{65535, 16384, 32}, Big{2147483647LL, 16384, 32}, Big{2147483647LL, 1, 1}, Big{32800, 16384, 1}})
    for (int storage : {kBatchStoreF64, kBatchStoreF32}) {
      const BatchLayout L = batch_layout(g.vlen, g.mvec);
      const wide_t eb = storage == kBatchStoreF32 ? 4 : 8, st = (g.vlen + 31) / 32 * 32, m1 = g.mvec + 1;
      const wide_t last = ((wide_t)(g.nsys - 1) * m1 + (m1 - 1)) * st;                  // first element of the last slot row
      const wide_t want_slots = eb * g.nsys * m1 * st, want_pend = storage == kBatchStoreF32 ? (wide_t)8 * g.nsys * st : 0;
      const wide_t lim = (wide_t)INT64_MAX;
      CHECK(want_slots <= lim && 2 * (want_slots + want_pend) <= lim, "the model itself leaves int64");
      CHECK((wide_t)batch_slot_offset(L, g.nsys - 1, g.mvec + 1) == last, "offset of the last slot row");
      CHECK((wide_t)batch_slot_offset(L, g.nsys - 1, g.mvec + 1) * eb + (wide_t)g.vlen * eb <= want_slots, "the last slot row ends inside");
      CHECK((wide_t)batch_pending_offset(L, g.nsys - 1) == (wide_t)(g.nsys - 1) * st, "offset of the last pending row");
      CHECK((wide_t)batch_slot_alloc_bytes(L, g.nsys, storage) == want_slots, "slot allocation, large");
      CHECK((wide_t)batch_pending_alloc_bytes(L, g.nsys, storage) == want_pend, "pending allocation, large");
      CHECK((wide_t)batch_vector_bytes(L, g.nsys, storage) == 2 * (want_slots + want_pend), "total, large");
    }
  {      // the large case of the GPU test: its float allocation passes both boundaries
    const BatchLayout L = batch_layout(16384, 32);
    CHECK(batch_slot_alloc_bytes(L, 3976, kBatchStoreF32) > (1LL << 32) && L.sys_stride * 3976 > (1LL << 31), "the large case does not cross");
  }
  if (failures) {
    std::fprintf(stderr, "batch_store32_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("batch_store32_check: slot and pending rows of three systems byte by byte, alignment of rows and pairs, the formula, the largest arguments: OK\n");
  return 0;
}
