// batch_large_check.cpp -- the host-callable arithmetic of the batched accelerator (nka_amd/csrc/host_logic.hpp) at the LARGEST
// legal arguments, against the same formulas in __int128: the index and size expressions that the kernels and the host share
// must not leave 64 bits -- or, where they are int, 32 -- anywhere a legal batch can take them.  Built with the sanitizer flags of
// `make -C nka_amd/csrc hostcheck` (tests/test_batch_large_cpu.py runs it): UBSan stops at the first signed overflow.
// It also restates the overflow guard of check_rows / weights_ldw (nka_batch.hip) and holds it at its edge.
#include "../../nka_amd/csrc/host_logic.hpp"

#include <cstdint>
#include <cstdio>

static int failures = 0;
#define CHECK(cond, ...)                                                                                                  \
  do {                                                                                                                    \
    if (!(cond)) {                                                                                                        \
      if (failures++ < 20) { std::fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
    }                                                                                                                     \
  } while (0)

using namespace nka_host;
typedef __int128 wide_t;

// check_rows (nka_batch.hip) refuses ld when this holds, so that the span (nsys - 1) ld + n, in bytes, stays inside 64 bits
static bool rows_refused(int64_t ld, int64_t n, int64_t nsys) { return ld > (INT64_MAX / (int64_t)sizeof(double) - n) / nsys; }

int main() {
  const int mvec = 32;                                   // NKA_HIP_BATCH_MAX_MVEC
  const long long nsys = 65535, cap = 1048576;           // the most systems and the longest system of a wide batch
  const long long nchunk = wide_nchunk(cap);
  CHECK(nchunk == cap / kWideChunk && nchunk <= kWideMaxChunks, "the longest wide system has %lld chunks", nchunk);

  // the partial sums: count and the last cell
  const wide_t count = (wide_t)nsys * (2 + 2 * mvec) * nchunk;
  CHECK((wide_t)wide_part_count(nsys, mvec, nchunk) == count, "wide_part_count at the largest batch");
  CHECK((wide_t)wide_part_count(65535, 32, 512) == (wide_t)65535 * 66 * 512, "wide_part_count(65535, 32, 512)");
  const wide_t last = ((wide_t)(nsys - 1) * (2 + 2 * mvec) + (2 + 2 * mvec - 1)) * nchunk + (nchunk - 1);
  CHECK((wide_t)wide_part_index(nsys - 1, 2 + 2 * mvec - 1, nchunk - 1, mvec, nchunk) == last && last == count - 1,
        "the last partial cell is the last cell of the buffer");
  CHECK((wide_t)wide_part_index(65534, 65, 511, 32, 512) == ((wide_t)65534 * 66 + 65) * 512 + 511, "wide_part_index(65534, 65, 511, 32, 512)");
  CHECK(count * (wide_t)sizeof(double) <= (wide_t)INT64_MAX, "the partial buffer's bytes leave 64 bits");

  // chunk lengths at the cap, at the last chunk, and one element either side of the last chunk edge
  for (long long vlen : {cap, cap - 1, cap - kWideChunk + 1, cap - kWideChunk}) {
    const long long nc = wide_nchunk(vlen), c = nc - 1;
    const wide_t rest = (wide_t)vlen - (wide_t)c * kWideChunk;
    const long long want = (long long)(rest < kWideChunk ? rest : (wide_t)kWideChunk);
    CHECK(wide_chunk_len(vlen, c) == want && want >= 1, "wide_chunk_len(%lld, %lld)", vlen, c);
    CHECK(wide_len_chunk_len(vlen, c) == want, "wide_len_chunk_len(%lld, %lld)", vlen, c);
    CHECK(wide_len_nchunk(vlen) == nc && wide_len_owns(vlen, c) && !wide_len_owns(vlen, nc), "the chunks a length of %lld owns", vlen);
    CHECK(wide_chunk_len(vlen, 0) == (vlen < kWideChunk ? vlen : kWideChunk), "the first chunk of %lld", vlen);
    CHECK(batch_len_valid(vlen, cap) && !batch_len_valid(cap + 1, cap), "length %lld in a batch of %lld", vlen, cap);
  }

  // the slots: the last element of the last system of the largest batch the library agrees to allocate (1e13 bytes of slots)
  {
    const BatchLayout lay = batch_layout(cap, mvec);
    CHECK((wide_t)lay.sys_stride == (wide_t)(mvec + 1) * lay.stride && lay.stride == cap, "the layout of the longest system");
    const wide_t end = (wide_t)(nsys - 1) * lay.sys_stride + (wide_t)mvec * lay.stride + cap;
    CHECK(end * 8 <= (wide_t)INT64_MAX, "the slots of the largest batch leave 64 bits");
    const BatchLayout nar = batch_layout(16384, mvec);      // the narrow batch at its cap: INT32_MAX systems stay inside 64 bits too
    CHECK((wide_t)INT32_MAX * nar.sys_stride * 8 <= (wide_t)INT64_MAX, "the slots of a narrow batch of 2^31 - 1 systems");
    CHECK((wide_t)INT32_MAX * nar.ic_stride * 4 <= (wide_t)INT64_MAX && (wide_t)INT32_MAX * nar.dc_stride * 8 <= (wide_t)INT64_MAX, "its control blocks");
  }

  // LDS at mvec = 32: every offset is an int and every size fits the 64 KiB (narrow: 40 KiB, four workgroups per CU) it is given
  {
    const int m1 = mvec + 1;
    const BatchLds l = batch_lds(mvec);
    const wide_t nd = (wide_t)(m1 + 1) * (m1 + 1) + (m1 + 1) + (2 + 2 * mvec) + m1 + kBatchWaves * kBatchAcc + kBatchAcc + 1;
    const wide_t ni = (wide_t)2 * (m1 + 1) + 2 * m1 + 8;
    CHECK((wide_t)l.ndouble == nd && (wide_t)l.nint == ni, "batch_lds(32): %d doubles, %d int32", l.ndouble, l.nint);
    CHECK((wide_t)l.bytes() == nd * 8 + ni * 4 && l.bytes() <= 40 * 1024, "batch_lds(32) takes %zu bytes", l.bytes());
    const int nc = (int)nchunk;
    const WideLds s = wide_sums_lds(mvec, nc);
    CHECK((wide_t)s.ndouble == (wide_t)nc + kBatchWaves * kBatchAcc + kBatchAcc + 1 && (wide_t)s.nint == (wide_t)(m1 + 1) + m1 + 8,
          "wide_sums_lds(32, %d): %d doubles, %d int32", nc, s.ndouble, s.nint);
    CHECK((wide_t)s.bytes() == (wide_t)s.ndouble * 8 + (wide_t)s.nint * 4 && s.bytes() <= 64 * 1024, "wide_sums_lds takes %zu bytes", s.bytes());
    const WideLds c = wide_combine_lds(mvec);
    CHECK(c.ndouble == m1 && c.nint == m1 + 8 && c.bytes() == (size_t)m1 * 8 + (size_t)(m1 + 8) * 4, "wide_combine_lds(32)");
    const WideScalarLds w = wide_scalar_lds(mvec, nc);
    CHECK((wide_t)w.b.ndouble == nd + nc && w.stage == l.ndouble && (wide_t)w.b.nint == ni, "wide_scalar_lds(32, %d)", nc);
    CHECK((wide_t)w.b.bytes() == (nd + nc) * 8 + ni * 4 && w.b.bytes() <= 64 * 1024, "wide_scalar_lds takes %zu bytes", w.b.bytes());
    // ... and with the most chunks the constants allow
    const WideScalarLds wm = wide_scalar_lds(mvec, kWideMaxChunks);
    CHECK(wm.b.bytes() <= 64 * 1024 && wide_sums_lds(mvec, kWideMaxChunks).bytes() <= 64 * 1024, "LDS at %d chunks", kWideMaxChunks);
  }

  // the guard of check_rows at its edge: the largest ld it lets through keeps the span, in bytes, inside 64 bits; one more is refused
  {
    const int64_t shapes[][2] = {{1, 1}, {16384, 1}, {16384, 4096}, {16384, 32800}, {16384, INT32_MAX}, {1048576, 65535}, {1, INT32_MAX}, {4099, 2052}};
    for (const auto &sh : shapes) {
      const int64_t n = sh[0], ns = sh[1];
      const int64_t edge = (INT64_MAX / (int64_t)sizeof(double) - n) / ns;
      CHECK(!rows_refused(edge, n, ns) && rows_refused(edge + 1, n, ns), "the edge of the guard at n %lld, nsys %lld", (long long)n, (long long)ns);
      const wide_t span = (wide_t)(ns - 1) * edge + n;      // what check_rows hands to the span check, in doubles
      CHECK(span * 8 <= (wide_t)INT64_MAX, "an accepted ld leaves 64 bits at n %lld, nsys %lld", (long long)n, (long long)ns);
      const int64_t span64 = (int64_t)(ns - 1) * edge + n;  // the same in the host's own arithmetic: UBSan watches it
      CHECK((wide_t)span64 == span && (wide_t)(span64 * (int64_t)sizeof(double)) == span * 8, "the span in int64 at n %lld, nsys %lld", (long long)n, (long long)ns);
      // (the guard bounds nsys ld + n, one row more than the span: what it refuses first is past 64 bits by that measure)
      CHECK(((wide_t)ns * (edge + 1) + n) * 8 > (wide_t)INT64_MAX, "the guard is not at its edge, n %lld, nsys %lld", (long long)n, (long long)ns);
    }
  }

  if (failures) {
    std::fprintf(stderr, "batch_large_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("batch_large_check: partial cells, chunk lengths, slots, LDS and the row guard at the largest legal arguments: OK\n");
  return 0;
}
