// host_logic_check.cpp -- the pure host-side arithmetic of libnka_hip.so (nka_amd/csrc/host_logic.hpp: the very text the
// library compiles) against brute-force models, built with g++ -fsanitize=address,undefined (make -C nka_amd/csrc hostcheck)
// and run on the CPU by tests/test_sanitizers_cpu.py.  Exit 0 = every check passed and no sanitizer report.
//   host_logic_check            all checks
//   host_logic_check plant      the same, then a deliberately PLANTED heap overflow: the run must die with an AddressSanitizer
//                               report -- the proof that the build really is instrumented (the test asserts that it does)
#include "../../nka_amd/csrc/host_logic.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace nka_host;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
  do {                                                                            \
    if (!(cond)) {                                                                \
      if (failures++ < 20) { std::fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
    }                                                                             \
  } while (0)

static void check_pass_widths() {
  for (int total = 1; total <= 4000; total++) {
    const int np = balanced_passes(total);
    CHECK(np >= 1 && (long long)np * kMaxPerPass >= total && (long long)(np - 1) * kMaxPerPass < total, "total %d np %d", total, np);
    std::vector<int> w((size_t)np + 2, -12345);          // (guards either side: balanced_widths must write w[0..np) only)
    balanced_widths(total, np, w.data() + 1);
    CHECK(w[0] == -12345 && w[(size_t)np + 1] == -12345, "total %d: wrote outside its array", total);
    int sum = 0, lo = 1 << 30, hi = 0, primes = 0, primes_balanced = 0;
    for (int p = 0; p < np; p++) {
      const int x = w[(size_t)p + 1];
      CHECK(x >= 1 && x <= kMaxPerPass, "total %d pass %d width %d", total, p, x);
      sum += x;
      lo = std::min(lo, x);
      hi = std::max(hi, x);
      primes += heavy_prime(x);
      primes_balanced += heavy_prime(total / np + (p < total % np ? 1 : 0));
    }
    CHECK(sum == total, "total %d: widths add up to %d", total, sum);
    CHECK(hi - lo <= 1 + np, "total %d: widths %d..%d are not balanced", total, lo, hi);      // (each move for a prime shifts one vector)
    if (np <= 2) CHECK(hi - lo <= 3, "total %d: widths %d..%d", total, lo, hi);
    CHECK(primes <= primes_balanced, "total %d: more heavy primes (%d) than the plain balanced split (%d)", total, primes, primes_balanced);
  }
  int w2[2];
  balanced_widths(62, 2, w2);
  CHECK(w2[0] + w2[1] == 62 && !heavy_prime(w2[0]) && !heavy_prime(w2[1]), "62 = %d + %d", w2[0], w2[1]);      // (62 = 32 + 30)
  for (int x = -5; x <= 200; x++) CHECK(round_up4(x) % 4 == 0 && round_up4(x) >= std::max(x, 1) && round_up4(x) < std::max(x, 1) + 4, "round_up4(%d)", x);
  for (int count = 1; count <= 3000; count++) {
    const int g = many_groups(count);
    int sum = 0;
    for (int p = 0; p < g; p++) {
      const int x = many_group_width(count, p);
      CHECK(x >= 1 && x <= kManyMax, "count %d group %d width %d", count, p, x);
      sum += x;
    }
    CHECK(sum == count && (long long)(g - 1) * kManyMax < count, "count %d groups %d sum %d", count, g, sum);
  }
}

// THE LAUNCH RULES.  Rings: properties, and a literal table (a changed ring is a deliberate edit of the table).
static void check_rings() {
  static const int ring[32] = {1, 2, 3, 4, 5, 6, 7, 4, 3, 5, 11, 4, 13, 7, 5, 4, 17, 6, 19, 4, 3, 22, 23, 4, 5, 26, 3, 4, 29, 5, 31, 4};
  static const int pairs[32] = {1, 2, 3, 2, 5, 2, 7, 2, 3, 2, 11, 2, 13, 2, 3, 2, 17, 2, 19, 2, 3, 2, 23, 2, 5, 2, 3, 2, 29, 2, 31, 2};
  static_assert(win_ring(20) == 4 && win_ring_pairs(20) == 2, "the rings are compile-time values: template arguments of the kernels");
  for (int w = 1; w <= 32; w++) {
    const int r = win_ring(w), rp = win_ring_pairs(w);
    CHECK(r >= 1 && w % r == 0 && rp >= 1 && w % rp == 0, "width %d: rings %d, %d must divide it", w, r, rp);
    CHECK(r == ring[w - 1] && rp == pairs[w - 1], "width %d: rings %d, %d, the table says %d, %d", w, r, rp, ring[w - 1], pairs[w - 1]);
    // the whole width as the ring: beyond 7 exactly the primes and 22, 26 (heavy_prime and the note on 22 / 26 rely on it)
    bool prime = w > 1;
    for (int d = 2; d * d <= w; d++) prime = prime && w % d != 0;
    if (w > 7) CHECK((r == w) == (prime || w == 22 || w == 26), "width %d: ring %d", w, r);
    if (heavy_prime(w)) CHECK(r == w && rp == w, "heavy prime %d: rings %d, %d", w, r, rp);
  }
}

// Ticket counters: the two spellings the rule had before it moved to host_logic.hpp, transcribed literally.
static int tickets_array_model(int pb_tickets, bool tickets, int64_t ntile, int T, int64_t g, int words) {      // launch_combine_win_1
  int ng = pb_tickets;
  if (ng < 0) ng = (ntile * T >= 64 * g) ? (words >= 22 ? 1 : 2) : 0;
  if (ng > 0 && (g % ng != 0 || ntile >= ((int64_t)1 << 31) - 2 * nka::kMaxGrid || !tickets)) ng = 0;
  return ng;
}
static int tickets_vector_model(int ticket_groups, bool tickets, int64_t ntile, int g, int words) {      // update_many_keep, T = 1
  const bool win = true;                      // (the 8-byte kernels take no tickets: the caller does not ask)
  int ng = ticket_groups;
  if (ng < 0) ng = (win && ntile >= (int64_t)64 * g) ? (words >= 22 ? 1 : 2) : 0;
  if (!win || !tickets || g % std::max(ng, 1) != 0 || ntile >= ((int64_t)1 << 31) - 2 * nka::kMaxGrid) ng = 0;
  return ng;
}
static void check_tickets() {
  const int64_t wrap = ((int64_t)1 << 31) - 2 * 4096;
  for (int forced : {-1, 0, 1, 2, 4, 8})
    for (int have = 0; have < 2; have++)
      for (int T : {1, 2})
        for (int grid : {1, 2, 3, 255, 256, 4096})
          for (int words : {21, 22})
            for (int64_t ntile : {(int64_t)0, (int64_t)64 * grid - 1, (int64_t)64 * grid, wrap - 1, wrap}) {
              const int ng = ticket_counters(forced, have != 0, ntile, T, grid, words);
              const int a = tickets_array_model(forced, have != 0, ntile, T, grid, words);
              CHECK(ng == a, "tickets(%d, %d, %lld, %d, %d, %d) = %d, the array spelling gives %d", forced, have, (long long)ntile, T, grid, words, ng, a);
              if (T == 1) {
                const int v = tickets_vector_model(forced, have != 0, ntile, grid, words);
                CHECK(ng == v, "tickets(%d, %d, %lld, 1, %d, %d) = %d, the vector spelling gives %d", forced, have, (long long)ntile, grid, words, ng, v);
              }
              CHECK(ng >= 0 && (ng == 0 || (have && grid % ng == 0 && ntile < wrap)), "tickets: %d counters for a grid of %d", ng, grid);
              // the prediction before the grid is known (one block per CU) is the rule's own answer where one or two counters divide the grid
              CHECK(tickets_expected(forced, have != 0, ntile, grid) == (forced != 0 && have && ntile >= (int64_t)64 * grid), "tickets_expected");
              if (forced < 0 && grid % 2 == 0 && ntile < wrap)
                CHECK(tickets_expected(forced, have != 0, ntile, grid) == (ticket_counters(forced, have != 0, ntile, 1, grid, words) > 0), "tickets_expected against ticket_counters");
            }
}

// The persistent grid and the blocks per CU against brute force; the values tests/test_exact_sums_cpu.py pins from Python.
static void check_grid() {
  for (int nloads = 1; nloads <= 70; nloads++) {
    int b = 1;
    while (b * nloads < 22) b++;                // the fewest blocks that keep 22 loads per thread in flight on a CU
    CHECK(blocks_per_cu(nloads) == b, "blocks_per_cu(%d) = %d, brute force %d", nloads, blocks_per_cu(nloads), b);
  }
  for (int num_cu : {1, 8, 256})
    for (int per_cu = 1; per_cu <= 8; per_cu++)
      for (int64_t ntile : {(int64_t)0, (int64_t)1, (int64_t)num_cu * per_cu - 1, (int64_t)num_cu * per_cu, (int64_t)num_cu * per_cu + 1, (int64_t)1000000000}) {
        int g = nka::kMaxGrid;                  // the largest grid of at most kMaxGrid blocks, per_cu per CU, one per tile -- but one at least
        while (g > 1 && (g > num_cu * per_cu || g > ntile)) g--;
        CHECK(persistent_grid(num_cu, per_cu, ntile) == g, "persistent_grid(%d, %d, %lld) = %d, brute force %d", num_cu, per_cu, (long long)ntile, persistent_grid(num_cu, per_cu, ntile), g);
      }
  auto vec_grid = [](int64_t n, int num_cu, int vec, int nloads) { return persistent_grid(num_cu, std::min(8, blocks_per_cu(nloads)), n / (256 * vec)); };
  const int nl[9] = {2, 3, 5, 6, 9, 10, 11, 22, 27}, want[9] = {2048, 2048, 1280, 1024, 768, 768, 512, 256, 256};
  for (int i = 0; i < 9; i++) CHECK(vec_grid(100000000, 256, 2, nl[i]) == want[i], "vector grid at %d loads: %d", nl[i], vec_grid(100000000, 256, 2, nl[i]));
  CHECK(vec_grid(100000000, 1024, 2, 2) == 4096, "kMaxGrid");
  CHECK(vec_grid(1, 256, 2, 2) == 1 && vec_grid(1023, 256, 2, 2) == 1 && vec_grid(1024, 256, 2, 2) == 2 && vec_grid(1023, 256, 1, 2) == 3, "short vectors");
}

// The list word against a model of device and host: updates (with dependence drops the host cannot see), relax, restart, and
// a word that reaches host memory whenever the device gets that far (any published word not older than the last one seen).
// SAFETY: the bound is never below the true list length at the entry of an update (the passes are launched at its width);
// EXACTNESS: it equals the true length whenever the newest word has arrived (a caller that synchronises once per iteration).
static void check_list_word() {
  std::mt19937_64 rng(12345);
  for (int trial = 0; trial < 4000; trial++) {
    const int mvec = 1 + (int)(rng() % 40);
    int64_t seq = 0, valid_after = 0;
    std::vector<int64_t> relaxed_after;
    int list_ub = 0;                          // the host's own count (nka_hip_state::list_ub)
    int L = 0;                                // the device's list length, pending pair included
    bool pending = false;
    std::vector<std::pair<int64_t, int>> published;      // (update number, list length at its exit), in order
    size_t seen = 0;                          // index + 1 of the newest word that has reached host memory (0 = none)
    for (int step = 0; step < 300; step++) {
      const unsigned r = (unsigned)(rng() % 100);
      if (r < 70) {                           // accel_update
        if (seen < published.size() && rng() % 2) seen += 1 + (size_t)(rng() % (published.size() - seen));     // the device got further
        const unsigned long long word = seen ? (((unsigned long long)published[seen - 1].first << kListWordLenBits) | (unsigned long long)published[seen - 1].second) : 0ull;
        const int ub = list_bound_from_word(list_ub, word, seq, valid_after, relaxed_after);
        CHECK(ub >= L && ub <= list_ub, "trial %d step %d: bound %d, true length %d, host count %d", trial, step, ub, L, list_ub);
        if (seen && published[seen - 1].first == seq && published[seen - 1].first > valid_after)
          CHECK(ub == L, "trial %d step %d: the newest word has arrived, bound %d != true length %d", trial, step, ub, L);
        const int d = L > 0 && rng() % 3 == 0 ? (int)(rng() % (unsigned)(L + 1)) : 0;      // dependence drops / s == 0 (device only)
        const int ncomb = std::min(L - d, mvec);
        L = ncomb + 1;
        const int comb_ub = pending ? std::min(ub, mvec) : ub;           // update_impl
        list_ub = comb_ub + 1;
        CHECK(list_ub >= L, "trial %d step %d: host count %d below the true length %d after an update", trial, step, list_ub, L);
        seq++;
        pending = true;
        published.push_back({seq, L});
      } else if (r < 85) {                    // relax (nka_hip_relax)
        if (pending) {
          pending = false;
          list_ub = std::max(list_ub - 1, 0);
          L--;
          relaxed_after.push_back(seq);
        }
      } else if (r < 93) {                    // restart (nka_hip_restart): words of updates enqueued so far are stale
        pending = false;
        list_ub = 0;
        L = 0;
        valid_after = seq;
        relaxed_after.clear();
      } else if (!published.empty()) {        // the caller synchronises: the newest word is there
        seen = published.size();
      }
      CHECK(relaxed_after.size() <= 300, "relaxed_after grows without bound");
    }
    // stale words and words from the future are ignored
    std::vector<int64_t> none;
    CHECK(list_bound_from_word(7, ((unsigned long long)(seq + 5) << kListWordLenBits) | 3ull, seq, valid_after, none) == 7, "a word from the future was used");
    CHECK(list_bound_from_word(7, ((unsigned long long)valid_after << kListWordLenBits) | 3ull, seq, valid_after, none) == 7, "a stale word was used");
  }
  // update numbers up to 2^43: no shift overflow
  std::vector<int64_t> none;
  const int64_t big = (1ll << 43) - 1;
  CHECK(list_bound_from_word(21, ((unsigned long long)big << kListWordLenBits) | 20ull, big, 0, none) == 20, "large update number");
}

// BufferBook::held against a brute-force interval model on a synthetic address space.
static void check_buffer_book() {
  std::mt19937_64 rng(777);
  std::vector<double> arena(1 << 16);         // real addresses, never dereferenced by held()
  for (int trial = 0; trial < 3000; trial++) {
    const int64_t n = 1 + (int64_t)(rng() % 97);
    const int64_t block = n * (int64_t)(2 + rng() % 5);
    const double *w = arena.data() + 1000, *v = w + block + (int64_t)(rng() % 50);
    BufferBook book;
    std::vector<const double *> all;
    for (int k = 0; k < 12; k++) {
      const double *q = arena.data() + 20000 + (int64_t)(rng() % 30000);
      book.taken.insert(q);
      all.push_back(q);
    }
    for (int k = 0; k < 4; k++) {
      const double *q = (rng() & 1) ? all[(size_t)(rng() % all.size())] : w + (int64_t)(rng() % (uint64_t)block);
      book.lent.insert(q);
    }
    for (int probe = 0; probe < 200; probe++) {
      const double *p = (rng() % 3 == 0) ? all[(size_t)(rng() % all.size())] + (int64_t)(rng() % (uint64_t)(2 * n)) - n
                                         : arena.data() + (int64_t)(rng() % 60000);
      bool want = false;
      if (!book.lent.count(p)) {
        auto hit = [&](const double *q, int64_t len) { return p < q + len && q < p + n; };
        want = hit(w, block) || hit(v, block);
        for (const double *q : book.taken) want = want || hit(q, n);
      }
      CHECK(book.held(p, n, w, v, block) == want, "trial %d probe at %td: held() says %d", trial, p - arena.data(), (int)!want);
    }
    // an empty slice (vlen 0) hands over a null buffer every time: nothing is held at the null address
    BufferBook none;
    CHECK(!none.held(nullptr, 0, w, v, block), "null buffer of an empty slice");
  }
}

// The decoding of a control-block snapshot (num_vec, get_state, digest of both handle types) at the smallest shapes that can
// go wrong.  Every block is an exact-size heap array: a read outside it is an AddressSanitizer report.
static void check_snapshot() {
  using namespace nka;
  auto blocks = [](int mvec, std::vector<int32_t> &ic, std::vector<double> &dc) {
    Ctl c{};
    c.mvec = mvec;
    ic.assign((size_t)c.ic_count(), 0);
    dc.assign((size_t)c.dc_count(), 0.0);
  };
  std::vector<int32_t> ic;
  std::vector<double> dc;
  // mvec = 1 (two slots): empty list; one entry, pending or not; both entries
  blocks(1, ic, dc);
  int32_t *next = ic.data() + IC_HEADER, *prev = next + 3;
  CHECK(snapshot_num_vec(ic.data(), 1) == 0, "mvec 1: empty list");
  ic[IC_FIRST] = ic[IC_LAST] = 2;
  CHECK(snapshot_num_vec(ic.data(), 1) == 1, "mvec 1: one entry");
  ic[IC_PENDING] = 1;
  CHECK(snapshot_num_vec(ic.data(), 1) == 0, "mvec 1: a one-entry list that is the pending pair");
  next[2] = 1;
  prev[1] = 2;
  ic[IC_LAST] = 1;
  CHECK(snapshot_num_vec(ic.data(), 1) == 1, "mvec 1: pending pair and one vector");
  // mvec = 2 (three slots), list 3 -> 1 -> 2: not slot order; h and c distinct everywhere
  blocks(2, ic, dc);
  const int m1 = 3;
  next = ic.data() + IC_HEADER;
  prev = next + (m1 + 1);
  ic[IC_SUBSPACE] = 1; ic[IC_PENDING] = 0; ic[IC_FIRST] = 3; ic[IC_LAST] = 2; ic[IC_FREE] = 0;
  next[3] = 1; next[1] = 2; next[2] = 0;
  prev[3] = 0; prev[1] = 3; prev[2] = 1;
  next[0] = -7; prev[0] = -9;                   // entry 0 is not a slot: it must not reach the outputs
  double *hh = dc.data() + DC_HEADER, *cc = hh + (m1 + 1) * (m1 + 1);
  for (int i = 0; i <= m1; i++) {
    for (int j = 0; j <= m1; j++) hh[i * (m1 + 1) + j] = 100.0 * i + j;      // the reference's h(i,j), 1-based; row / column 0 unused
    cc[i] = 1000.0 + i;
  }
  CHECK(snapshot_num_vec(ic.data(), 2) == 3, "mvec 2: list 3 -> 1 -> 2");
  ic[IC_PENDING] = 1;
  CHECK(snapshot_num_vec(ic.data(), 2) == 2, "mvec 2: the same with a pending pair");
  int32_t subspace = -1, pending = -1, first = -1, last = -1, free_ = -1;
  std::vector<int32_t> onext((size_t)m1, -1), oprev((size_t)m1, -1);
  std::vector<double> oh((size_t)m1 * m1, -1.0), oc((size_t)m1, -1.0);
  snapshot_unpack(ic.data(), dc.data(), 2, &subspace, &pending, &first, &last, &free_, onext.data(), oprev.data(), oh.data(), oc.data());
  CHECK(subspace == 1 && pending == 1 && first == 3 && last == 2 && free_ == 0, "scalars %d %d %d %d %d", subspace, pending, first, last, free_);
  for (int k = 1; k <= m1; k++) {
    CHECK(onext[(size_t)k - 1] == next[k] && oprev[(size_t)k - 1] == prev[k], "links of slot %d: %d %d", k, onext[(size_t)k - 1], oprev[(size_t)k - 1]);
    CHECK(oc[(size_t)k - 1] == 1000.0 + k, "c of slot %d: %g", k, oc[(size_t)k - 1]);
    for (int j = 1; j <= m1; j++)      // column-major m1 x m1, 0-based
      CHECK(oh[(size_t)(k - 1) + (size_t)(j - 1) * m1] == 100.0 * k + j, "h(%d,%d): %g", k, j, oh[(size_t)(k - 1) + (size_t)(j - 1) * m1]);
  }
  snapshot_unpack(ic.data(), dc.data(), 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);      // every output is optional
  // links that cycle (1 -> 2 -> 1 ...): the walk ends after mvec + 1 steps, inside the block
  ic[IC_PENDING] = 0; ic[IC_FIRST] = 1;
  next[1] = 2; next[2] = 1;
  CHECK(snapshot_num_vec(ic.data(), 2) == 2 + 2, "cycling links: the walk stops one past the mvec + 1 slots");
  next[1] = 1;
  CHECK(snapshot_num_vec(ic.data(), 2) == 2 + 2, "a slot linked to itself");
  // FNV-1a, the published vectors; the digest mixes ic first, then dc, from the library's own seed
  CHECK(fnv1a(nullptr, 0) == 0xcbf29ce484222325ull, "FNV-1a of the empty input");
  CHECK(fnv1a("a", 1) == 0xaf63dc4c8601ec8cull, "FNV-1a of \"a\"");
  CHECK(snapshot_digest({}, {}) == kDigestSeed && kDigestSeed == 1469598103934665603ull, "digest of two empty blocks: the seed");
  const std::vector<int32_t> i1 = {0x64636261};                                   // "abcd"
  const std::vector<double> d1 = {1.5};
  unsigned char bytes[12];
  std::memcpy(bytes, i1.data(), 4);
  std::memcpy(bytes + 4, d1.data(), 8);
  CHECK(snapshot_digest(i1, d1) == fnv1a(bytes, 12, kDigestSeed), "digest: the bytes of ic, then those of dc");
  std::memcpy(bytes, d1.data(), 8);
  std::memcpy(bytes + 8, i1.data(), 4);
  CHECK(snapshot_digest(i1, d1) != fnv1a(bytes, 12, kDigestSeed), "digest: dc first gives another value");
}

int main(int argc, char **argv) {
  check_pass_widths();
  check_rings();
  check_tickets();
  check_grid();
  check_list_word();
  check_buffer_book();
  check_snapshot();
  if (failures) {
    std::fprintf(stderr, "host_logic_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("host_logic_check: pass widths, launch groups, rings, ticket counters, grids, list word, buffer book, snapshot decoding: OK\n");
  if (argc > 1 && !std::strcmp(argv[1], "plant")) {
    // PLANTED: balanced_widths asked for one pass more than its array holds
    int *w = static_cast<int *>(std::malloc(sizeof(int) * 2));
    balanced_widths(70, 3, w);
    std::printf("planted overflow was NOT caught: %d\n", w[0]);
    std::free(w);
    return 0;
  }
  return 0;
}
