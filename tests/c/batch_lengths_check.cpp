// batch_lengths_check.cpp -- what the kernels and the host share about a system's OWN length inside a longer batch
// (nka_amd/csrc/host_logic.hpp: batch_len_valid, wide_len_nchunk, wide_len_owns, wide_len_chunk_len; nka_hip_batch_set_lengths)
// against brute-force models, for EVERY length 1 ... 3 CHUNK + 33.  Built with the sanitizer flags of `make -C nka_amd/csrc
// hostcheck` (tests/test_batch_lengths_cpu.py runs it).  The partial cells a system reads are painted into a buffer of the size
// the batch allocates, so an index outside it is an address error and not only a failed comparison.
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

int main() {
  const long long C = kWideChunk, vlen = 3 * C + 33, tile = 512;
  const int mvec = 3, nsys = 3, sys = 1, nentry = 2 + 2 * mvec;
  const long long nchunk = wide_nchunk(vlen);      // the batch's: the stride of the partials and the first grid index
  CHECK(nchunk == 4, "a batch of 3 CHUNK + 33 elements has %lld chunks", nchunk);
  for (long long bad : {0LL, -1LL, -2147483647LL - 1, vlen + 1, 2147483647LL}) CHECK(!batch_len_valid(bad, vlen), "length %lld accepted", bad);
  std::vector<int> part((size_t)wide_part_count(nsys, mvec, nchunk), 0);
  const long long lo_cell = wide_part_index(sys, 0, 0, mvec, nchunk), hi_cell = wide_part_index(sys + 1, 0, 0, mvec, nchunk);
  for (long long len = 1; len <= vlen; len++) {
    CHECK(batch_len_valid(len, vlen), "length %lld refused", len);
    long long model = 0;      // ceil(len / CHUNK) by counting
    for (long long e = 0; e < len; e += C) model++;
    const long long own = wide_len_nchunk(len);
    CHECK(own == model && own >= 1 && own <= nchunk, "length %lld owns %lld chunks, the model says %lld", len, own, model);
    CHECK(own == wide_nchunk(len), "a batch created with vlen = %lld has other chunks", len);
    long long covered = 0;
    for (long long c = 0; c < nchunk; c++) {      // every workgroup of the grid
      CHECK(wide_len_owns(len, c) == (c < own), "length %lld, chunk %lld", len, c);
      if (!wide_len_owns(len, c)) continue;       // (returns before it reads anything)
      const long long n = wide_len_chunk_len(len, c);
      CHECK(n >= 1 && n <= C, "length %lld, chunk %lld holds %lld", len, c, n);
      CHECK(c == own - 1 || n % tile == 0, "length %lld: chunk %lld of %lld is not whole tiles (%lld)", len, c, own, n);
      CHECK(n == wide_chunk_len(len, c), "length %lld, chunk %lld: not the chunk of a batch of that length", len, c);
      CHECK(c * C == covered && covered + n <= vlen, "length %lld, chunk %lld leaves the row", len, c);
      covered += n;
      for (int e = 0; e < nentry; e++) {          // the partial this workgroup writes, and the scalar kernel reads
        const long long i = wide_part_index(sys, e, c, mvec, nchunk);
        CHECK(i >= lo_cell && i < hi_cell, "length %lld: cell %lld of entry %d, chunk %lld, is outside the system's cells", len, i, e, c);
        part[(size_t)i]++;
      }
    }
    CHECK(covered == len, "the chunks of length %lld cover %lld", len, covered);
    // the chunk-order chain of an entry reads p[0 .. own) from the entry's first cell: inside the entry's own nchunk cells
    for (int e = 0; e < nentry; e++)
      CHECK(wide_part_index(sys, e, 0, mvec, nchunk) + own <= wide_part_index(sys, e, 0, mvec, nchunk) + nchunk, "entry %d", e);
  }
  for (long long i = 0; i < (long long)part.size(); i++) CHECK((part[(size_t)i] != 0) == (i >= lo_cell && i < hi_cell), "cell %lld", i);
  if (failures) {
    std::fprintf(stderr, "batch_lengths_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("batch_lengths_check: every length 1 ... %lld: chunks owned, chunk lengths, partial cells: OK\n", vlen);
  return 0;
}
