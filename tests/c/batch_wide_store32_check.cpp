// batch_wide_store32_check.cpp -- the address arithmetic of the binary32 instances of a wide batch (nka_hip_batch_create_wide_stored;
// nka_amd/csrc/host_logic.hpp: batch_slot_offset and batch_pending_offset with wide_len_owns, wide_chunk_len and the chunk's start;
// the sweep of nka_batch_dev.hpp restated) against a brute-force model, built with the sanitizer flags of `make -C nka_amd/csrc
// hostcheck` (tests/test_batch_wide_store32_cpu.py runs it).  Three systems of 3C + 33 elements: for every length 1 ... 3C + 33 the
// bytes of a FLOAT slot row and of the binary64 PENDING row that the chunks of a system touch are painted one by one -- every byte
// below the length exactly once, nothing else of either allocation, no two accesses overlapping; an 8-byte access of a float pair
// starts on 8 bytes and a 16-byte access of a pending pair on 16; a chunk beyond the system's own touches nothing.  Every offset and
// size is held against __int128 at the largest legal arguments.
#include "../../nka_amd/csrc/host_logic.hpp"

#include <cstdio>
#include <cstring>
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

// thread t's pair at i of a chunk of n elements, element size eb, the chunk's first element `off` elements into the allocation
// `bytes`: one access of 2 eb bytes where both elements exist (ld_tile32 / st_tile32, ld_tile / st_tile of an aligned vector), else
// the elements below n one by one
static void touch(std::vector<unsigned char> &bytes, long long off, long long i, long long n, bool full, int eb) {
  const bool pair = full || i + 1 < n;
  if (pair) CHECK(((off + i) * eb) % (2 * eb) == 0, "an access of %d bytes at byte %lld", 2 * eb, (off + i) * eb);
  for (int q = 0; q < 2; q++) {
    if (!pair && !(i + q < n)) continue;
    const long long b0 = (off + i + q) * eb;
    for (int b = 0; b < eb; b++) {
      CHECK(b0 + b >= 0 && b0 + b < (long long)bytes.size(), "byte %lld lies outside the allocation", b0 + b);
      if (b0 + b >= 0 && b0 + b < (long long)bytes.size()) bytes[(size_t)(b0 + b)]++;
    }
  }
}

static void sweep(std::vector<unsigned char> &bytes, long long off, long long n, int eb) {
  long long base = 0;
  for (; base + kTile <= n; base += kTile)
    for (int t = 0; t < kThreads; t++) touch(bytes, off, base + 2 * t, n, true, eb);
  if (base < n)
    for (int t = 0; t < kThreads; t++)
      if (base + 2 * t < n) touch(bytes, off, base + 2 * t, n, false, eb);
}

// every byte of [lo, lo + len) once, nothing else
static void painted(const std::vector<unsigned char> &bytes, long long lo, long long len, const char *what, int sys, long long length) {
  static const std::vector<unsigned char> zeros(1 << 22, 0), ones(1 << 22, 1);      // (the common case in three memcmp)
  const long long size = (long long)bytes.size();
  if (size <= (long long)zeros.size() && lo >= 0 && lo + len <= size && std::memcmp(bytes.data(), zeros.data(), (size_t)lo) == 0 &&
      std::memcmp(bytes.data() + lo, ones.data(), (size_t)len) == 0 && std::memcmp(bytes.data() + lo + len, zeros.data(), (size_t)(size - lo - len)) == 0)
    return;
  for (long long b = 0; b < (long long)bytes.size(); b++) {
    const int want = (b >= lo && b < lo + len) ? 1 : 0;
    if (bytes[(size_t)b] != want) {
      CHECK(false, "%s, system %d, length %lld: byte %lld touched %d times, not %d", what, sys, length, b, (int)bytes[(size_t)b], want);
      return;
    }
  }
}

int main() {
  const long long C = kWideChunk;
  const long long vlen = 3 * C + 33;
  const int mvec = 3, m1 = mvec + 1, nsys = 3;
  const BatchLayout lay = batch_layout(vlen, mvec);
  CHECK(lay.stride % 32 == 0 && lay.stride >= vlen && lay.sys_stride == lay.stride * m1, "the strides %lld, %lld", (long long)lay.stride, (long long)lay.sys_stride);
  CHECK(C % kTile == 0 && C % 2048 == 0, "a chunk is whole tiles and starts on a multiple of 2048 elements");
  const long long nchunk = wide_nchunk(vlen);
  CHECK(nchunk == 4, "3C + 33 is four chunks");
  CHECK(batch_slot_alloc_bytes(lay, nsys, kBatchStoreF32) == 4 * lay.sys_stride * nsys, "the float slots");
  CHECK(batch_pending_alloc_bytes(lay, nsys, kBatchStoreF32) == 8 * lay.stride * nsys, "the pending rows");
  CHECK(batch_pending_alloc_bytes(lay, nsys, kBatchStoreF64) == 0, "binary64 storage has no pending rows");
  std::vector<unsigned char> slots((size_t)batch_slot_alloc_bytes(lay, nsys, kBatchStoreF32));
  std::vector<unsigned char> pend((size_t)batch_pending_alloc_bytes(lay, nsys, kBatchStoreF32));
  for (long long len = 1; len <= vlen; len++) {
    for (int sys = 0; sys < nsys; sys += (len % 64 == 1 ? 1 : 2)) {      // (every system at every 64th length, 0 and 2 elsewhere)
      const int slot = 1 + (int)((len + sys) % m1);
      std::memset(slots.data(), 0, slots.size());
      std::memset(pend.data(), 0, pend.size());
      const long long srow = batch_slot_offset(lay, sys, slot), prow = batch_pending_offset(lay, sys);
      CHECK(srow == (long long)sys * lay.sys_stride + (long long)(slot - 1) * lay.stride && prow == (long long)sys * lay.stride, "the rows of system %d", sys);
      CHECK((srow * 4) % 128 == 0 && (prow * 8) % 256 == 0, "a float row starts on 128 bytes, a pending row on 256");
      long long chunks = 0;
      for (long long c = 0; c < nchunk; c++) {
        if (!wide_len_owns(len, c)) continue;      // the workgroup returns before it touches anything
        chunks++;
        const long long n = wide_chunk_len(len, c), lo = c * C;
        CHECK(n >= 1 && n <= C && lo + n <= len, "chunk %lld of length %lld holds %lld elements", c, len, n);
        CHECK(((srow + lo) * 4) % 8 == 0 && ((prow + lo) * 8) % 16 == 0, "chunk %lld starts inside a pair", c);
        sweep(slots, srow + lo, n, 4);
        sweep(pend, prow + lo, n, 8);
      }
      CHECK(chunks == wide_len_nchunk(len), "length %lld is touched by %lld chunks", len, chunks);
      painted(slots, srow * 4, len * 4, "float slot", sys, len);
      painted(pend, prow * 8, len * 8, "pending row", sys, len);
    }
  }
  // the largest legal batch: nsys = 65535 systems of NKA_HIP_BATCH_WIDE_MAX_VLEN = 512 C elements at mvec = 32; 64 bits hold it
  {
    const long long cap = 512 * C, big = 65535;
    const int mv = 32;
    const BatchLayout l = batch_layout(cap, mv);
    const __int128 stride = l.stride, ss = l.sys_stride;
    CHECK(stride == cap && ss == stride * (mv + 1), "the strides at the cap");
    CHECK((__int128)batch_slot_alloc_bytes(l, big, kBatchStoreF32) == 4 * ss * big, "the float slots at the cap");
    CHECK((__int128)batch_pending_alloc_bytes(l, big, kBatchStoreF32) == 8 * stride * big, "the pending rows at the cap");
    CHECK((__int128)batch_vector_bytes(l, big, kBatchStoreF32) == 2 * (__int128)big * stride * (4 * (mv + 1) + 8), "the formula of the header at the cap");
    CHECK((__int128)batch_vector_bytes(l, big, kBatchStoreF64) == 2 * (__int128)big * stride * 8 * (mv + 1), "binary64 at the cap");
    for (long long sys : {0LL, 1LL, 123LL, 124LL, 4095LL, 4096LL, 32767LL, 32768LL, 65534LL})
      for (int slot : {1, 2, mv, mv + 1})
        for (long long c : {0LL, 1LL, 255LL, 256LL, 511LL}) {
          const __int128 want = (__int128)sys * ss + (__int128)(slot - 1) * stride + (__int128)c * C;
          const long long got = batch_slot_offset(l, sys, slot) + c * C;
          CHECK((__int128)got == want, "the slot offset (%lld, %d, %lld) wrapped", sys, slot, c);
          CHECK(want * 4 + (__int128)C * 4 <= 4 * ss * big && want * 4 < ((__int128)1 << 63), "chunk (%lld, %d, %lld) leaves the float slots", sys, slot, c);
          const __int128 pwant = (__int128)sys * stride + (__int128)c * C;
          const long long pgot = batch_pending_offset(l, sys) + c * C;
          CHECK((__int128)pgot == pwant, "the pending offset (%lld, %lld) wrapped", sys, c);
          CHECK(pwant * 8 + (__int128)C * 8 <= 8 * stride * big && pwant * 8 < ((__int128)1 << 63), "chunk (%lld, %lld) leaves the pending rows", sys, c);
          if (sys >= 124) CHECK(want >= ((__int128)1 << 31) && want * 4 >= ((__int128)1 << 32), "the case is beyond 2^31 elements");
        }
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch_wide_store32_check: OK\n");
  return 0;
}
