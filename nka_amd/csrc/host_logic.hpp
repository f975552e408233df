// host_logic.hpp -- the PURE host-side arithmetic of libnka_hip.so: pass widths, the launch rules (ring sizes, persistent grids,
// ticket counters), the decoding of the list word and of a control-block snapshot, who holds which buffer, launch groups of
// the vector hooks.  No HIP, no device state: the .hip files include it,
// and tests/c/host_logic_check.cpp compiles the same text with g++ -fsanitize=address,undefined and checks every function
// against a brute-force model on the CPU (`make -C nka_amd/csrc hostcheck`, tests/test_sanitizers_cpu.py) -- the part of the
// host code a sanitizer can see without a GPU (the reference's stand-in is its `defined` invariant check,
// /root/reference/src-F08/nka_type.F90:460-524).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <set>
#include <vector>

#include "nka_ctl.hpp"

namespace nka_host {

using nka::kMaxPerPass;        // largest list width one launch of the streaming kernels takes
using nka::kListWordLenBits;   // list word = update number << 20 | list length at its exit
constexpr int kManyMax = 24;           // vectors per launch of the batched vector hooks (= vec_ops.hip)

inline int round_up4(int x) { return ((std::max(x, 1) + 3) / 4) * 4; }

// A list of `total` > kMaxPerPass entries in the fewest passes of BALANCED widths (33 -> 17 + 16, 70 -> 24 + 23 + 23): every
// pass then runs the rolling-window kernel at (nearly) its exact width instead of one full pass of 32 and one that is mostly
// padding (measured in round 5, profiles/r05/multipass.txt: mvec = 33 at 0.58 of the roofline against 0.76 at mvec = 32).
inline int balanced_passes(int total) { return (total + kMaxPerPass - 1) / kMaxPerPass; }
// The widths whose only ring is the whole width (win_ring / win_ring_pairs: primes) AND large: 23, 29, 31.
inline bool heavy_prime(int w) { return w == 23 || w == 29 || w == 31; }
// (22 and 26 -- twice a prime: no ring in win_ring's list either -- were tried the same way in round 5: padding to 24 / 28 makes PA
//  3-4 % SLOWER and the update +1...2 % (compact), -1 % (src-F08): not kept, profiles/r05/multipass.txt)
// widths[0..np): balanced, then one vector moved between two passes wherever that removes a heavy prime without making another
inline void balanced_widths(int total, int np, int *w) {
  for (int p = 0; p < np; p++) w[p] = total / np + (p < total % np ? 1 : 0);
  for (int i = 0; i < np; i++) {
    if (!heavy_prime(w[i])) continue;
    for (int j = 0; j < np; j++) {
      if (j == i) continue;
      if (w[i] + 1 <= kMaxPerPass && w[j] > 1 && !heavy_prime(w[j] - 1)) { w[i]++; w[j]--; break; }          // (w[i] + 1 is even)
      if (w[j] + 1 <= kMaxPerPass && !heavy_prime(w[j] + 1) && !heavy_prime(w[i] - 1)) { w[i]--; w[j]++; break; }
    }
  }
}

// Launch groups of the batched hooks of the abstract-vector flavour: balanced too (25 = 13 + 12, not 24 + 1).
inline int many_groups(int count) { return count <= kManyMax ? 1 : (count + kManyMax - 1) / kManyMax; }
inline int many_group_width(int count, int p) { const int np = many_groups(count); return count / np + (p < count % np ? 1 : 0); }

// THE LAUNCH RULES of the streaming kernels, one definition for the array flavour (nka_hip.hip) and the vector workspace
// (vec_ops.hip).
// The ring size of the rolling-window kernels: a small divisor of the width (4, 5, 6, 3 or 7), or the width itself when it
// is prime (then every load of a tile is in flight and each is re-issued for the next tile as soon as it has been consumed).
// Rings of 2, width/4 and width/2 measured slower than 4 (profiles/r02/ab_inproc_pipelined_passes.txt).
constexpr int win_ring(int width) {
  return width % 4 == 0 ? 4 : width % 5 == 0 ? 5 : width % 6 == 0 ? 6 : width % 3 == 0 ? 3 : width % 7 == 0 ? 7 : width;
}
// What streams TWO vectors per entry (the flavours F08 and F08-vector, the pair lists of the vector workspace) keeps the same
// number of loads in flight with half the ring: 2 pairs where the width is even (in-process A/B at m = 20: -3.5 % at
// n = 1.25e7, equal at 1e8; the compact flavour loses 13 % with a ring of 2 single loads).
constexpr int win_ring_pairs(int width) {
  return width % 2 == 0 ? 2 : width % 3 == 0 ? 3 : width % 5 == 0 ? 5 : width % 7 == 0 ? 7 : width;
}
// Blocks per CU when each thread keeps `nloads` 16-byte loads in flight per tile.  Measured on MI355X (n = 1.25e7 and 1e8,
// m = 20): ONE block per CU is fastest once a block has >= 22 loads per thread in flight (88 KiB per CU); more blocks per CU
// only add write/read interleaving in the mixed pass (PB 0.46 -> 0.52 ms at 4 per CU).  Narrow instantiations get
// proportionally more blocks to keep ~88 KiB in flight.
inline int blocks_per_cu(int nloads) { return std::max(1, (22 + nloads - 1) / nloads); }
// Persistent grid: `per_cu` blocks on each CU (the caller caps it by the occupancy of its kernel), so every block is
// co-resident and the grid-stride loops stay balanced; at most one block per tile and kMaxGrid in all, at least one.
inline int persistent_grid(int num_cu, int per_cu, int64_t ntile) {
  const int64_t g = std::min<int64_t>((int64_t)num_cu * per_cu, std::max<int64_t>(ntile, 1));
  return (int)std::max<int64_t>(std::min<int64_t>(g, nka::kMaxGrid), 1);
}
// Tile tickets (k_combine_win, k_update_many_keep_win), in-process A/B (profiles/r02/ab_inproc_tile_tickets.txt): PB
// -3...-10 % at n = 1e8 (the slower the box's static pass, the larger the gain), -2...-4 % at 1.25e7, 0 (m = 20) to -10 %
// (m = 10) at 1e7, +3 % at 3e6 -> from 64 tiles of 512 elements per block.  ONE counter while a tile carries >= 22 words per
// element and 512 elements (<= ~60 tickets/us), two below that (a single counter saturates).
constexpr int kTicketTilesPerBlock = 64;
// How many counters hand out the `ntile` tiles of `T` * 512 elements to `grid` blocks; 0 = static mapping.  `forced` >= 0 is
// the caller's tuning field, < 0 the rule above.  None where the grid does not divide among the counters, where the tickets
// (32-bit: the tiles plus what the blocks draw past the end) could wrap, or where the handle has no counters.
inline int ticket_counters(int forced, bool have_counters, int64_t ntile, int T, int grid, int words) {
  int ng = forced;
  if (ng < 0) ng = (ntile * T >= (int64_t)kTicketTilesPerBlock * grid) ? (words >= 22 ? 1 : 2) : 0;
  if (ng > 0 && (grid % ng != 0 || ntile >= ((int64_t)1 << 31) - 2 * nka::kMaxGrid || !have_counters)) ng = 0;
  return ng;
}
// The same decision before the grid is known (one block per CU): will the automatic rule hand out `ntile` tiles by tickets?
inline bool tickets_expected(int forced, bool have_counters, int64_t ntile, int num_cu) {
  return forced != 0 && have_counters && ntile >= (int64_t)kTicketTilesPerBlock * num_cu;
}

// THE LIST WORD (include/nka_hip_ext.h: nka_hip_list_bound).  PB of update number u publishes (u, list length at its exit).
// The host's upper bound on the list length at the entry of the next update: its own count `ub`, tightened by the word if the
// word is fresh enough to be trusted -- newer than the last restart (`valid_after`) and not from the future (`seq` = updates
// enqueued so far) -- plus one per update enqueued since, minus one per relax() that dropped a pending pair since
// (`relaxed_after`: the update number before each such relax; entries older than the word are dropped: they are part of
// every later word).  Never above `ub`, never negative.
inline int list_bound_from_word(int ub, unsigned long long word, int64_t seq, int64_t valid_after, std::vector<int64_t> &relaxed_after) {
  const int64_t u = (int64_t)(word >> kListWordLenBits);
  if (u <= valid_after || u > seq) return ub;
  int64_t len = (int64_t)(word & ((1ull << kListWordLenBits) - 1)) + (seq - u);
  size_t keep = 0;
  for (int64_t r : relaxed_after)
    if (r >= u) {
      len--;
      relaxed_after[keep++] = r;
    }
  relaxed_after.resize(keep);
  return (int)std::min<int64_t>(ub, std::max<int64_t>(len, 0));
}

// WHO HOLDS WHICH BUFFER, as far as the host can know it (the out-of-place entry, nka_hip_accel_update_swap).  `taken` = every
// buffer outside the two slot-major allocations that a slot table entry may name; `lent` = the free buffers handed to the
// caller for its next input (they may lie anywhere, the slot-major allocations included).  Every such buffer holds n doubles.
struct BufferBook {
  std::set<const double *> taken, lent;
  // Does [p, p + n) touch memory the library holds -- one of the two slot-major blocks [w, w + block), [v, v + block) or a taken
  // buffer -- that it has NOT lent to the caller?
  bool held(const double *p, int64_t n, const double *w, const double *v, int64_t block) const {
    if (lent.count(p)) return false;
    n = std::max<int64_t>(n, 1);
    // (address arithmetic on integers: p - n may lie before any object)
    const uintptr_t P = reinterpret_cast<uintptr_t>(p), N = (uintptr_t)n * sizeof(double), B = (uintptr_t)block * sizeof(double);
    auto overlaps = [&](const double *q, uintptr_t len) {
      const uintptr_t Q = reinterpret_cast<uintptr_t>(q);
      return P < Q + len && Q < P + N;
    };
    if (overlaps(w, B) || overlaps(v, B)) return true;
    // every taken buffer holds n doubles: one of them overlaps [p, p + n) iff its base lies in (p - n, p + n)
    const uintptr_t lo = P >= N ? P - N : 0;
    auto it = taken.upper_bound(reinterpret_cast<const double *>(lo));
    if (P < N && !taken.empty() && reinterpret_cast<uintptr_t>(*taken.begin()) == 0) it = taken.begin();
    return it != taken.end() && reinterpret_cast<uintptr_t>(*it) < P + N;
  }
};

// A SNAPSHOT OF THE CONTROL BLOCK on the host (`ic`, `dc`: the two arrays of a Ctl of `mvec`, copied from the device): what the
// accessors of both handle types (nka_hip_num_vec / _get_state / _state_digest and their nka_hip_batch_ siblings) report.
// Vectors in the subspace: the list length (F08:224-229; the walk ends after mvec + 1 steps whatever the links say) less the
// pending pair (F08:230).
inline int snapshot_num_vec(const int32_t *ic, int mvec) {
  const int32_t *next = ic + nka::IC_HEADER;
  int n = 0;
  for (int k = ic[nka::IC_FIRST]; k != 0 && n <= mvec + 1; k = next[k]) n++;
  return ic[nka::IC_PENDING] ? n - 1 : n;
}
// The state as the reference's get-state hands it out (every output optional): slots 1-based on the device, arrays 0-based
// here; h column-major m1 x m1 with h[(i-1) + (j-1) m1] = the reference's h(i,j).
inline void snapshot_unpack(const int32_t *ic, const double *dc, int mvec, int32_t *subspace, int32_t *pending, int32_t *first,
                            int32_t *last, int32_t *free_, int32_t *next, int32_t *prev, double *h, double *c) {
  const int m1 = mvec + 1;
  if (subspace) *subspace = ic[nka::IC_SUBSPACE];
  if (pending) *pending = ic[nka::IC_PENDING];
  if (first) *first = ic[nka::IC_FIRST];
  if (last) *last = ic[nka::IC_LAST];
  if (free_) *free_ = ic[nka::IC_FREE];
  const int32_t *nx = ic + nka::IC_HEADER, *pv = nx + (m1 + 1);
  const double *hh = dc + nka::DC_HEADER, *cc = hh + (m1 + 1) * (m1 + 1);
  for (int k = 1; k <= m1; k++) {
    if (next) next[k - 1] = nx[k];
    if (prev) prev[k - 1] = pv[k];
    if (c) c[k - 1] = cc[k];
  }
  if (h)
    for (int j = 1; j <= m1; j++)
      for (int i = 1; i <= m1; i++) h[(i - 1) + (size_t)(j - 1) * m1] = hh[i * (m1 + 1) + j];
}
// FNV-1a, 64 bits.  The digest of a snapshot mixes the bytes of ic, then those of dc, from the seed the library has always used
// (the published offset basis less its last decimal digit): digests are compared between ranks, runs and versions, so it stays.
constexpr uint64_t kFnvOffsetBasis = 14695981039346656037ull, kFnvPrime = 1099511628211ull;
constexpr uint64_t kDigestSeed = 1469598103934665603ull;
inline uint64_t fnv1a(const void *p, size_t nbytes, uint64_t h = kFnvOffsetBasis) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < nbytes; i++) {
    h ^= b[i];
    h *= kFnvPrime;
  }
  return h;
}
inline uint64_t snapshot_digest(const std::vector<int32_t> &ic, const std::vector<double> &dc) {
  return fnv1a(dc.data(), dc.size() * sizeof(double), fnv1a(ic.data(), ic.size() * sizeof(int32_t), kDigestSeed));
}

// THE BATCHED ACCELERATOR (include/nka_hip_batch.h, nka_batch.hip): where the pieces of system `sys` lie.  Host and kernel
// compile this text; tests/c/batch_layout_check.cpp holds it against a brute-force model (no two pieces overlap, every
// stride a multiple of 32 doubles, the LDS budget).
constexpr int kBatchWaves = 4;                   // wavefronts of a workgroup (256 threads)
constexpr int kBatchGroup = 4;                   // older vectors per sweep of the sums
constexpr int kBatchAcc = 2 * kBatchGroup + 1;   // their two sums each, and <f,w1'>
// control block of one system: the counts of a Ctl (nka_ctl.hpp) of that mvec, asked of one with no arrays behind it
NKA_HOST_DEVICE constexpr int batch_ic_count(int mvec) { nka::Ctl c{}; c.mvec = mvec; return c.ic_count(); }
NKA_HOST_DEVICE constexpr int batch_dc_count(int mvec) { nka::Ctl c{}; c.mvec = mvec; return c.dc_count(); }
struct BatchLayout {
  int64_t stride;        // doubles between the slots of a system: vlen rounded up to 32 (256 bytes)
  int64_t sys_stride;    // doubles between systems in the w and the v allocation: (mvec + 1) slots
  int32_t ic_stride;     // int32 between the control blocks (a multiple of 32: 128 bytes)
  int32_t dc_stride;     // doubles between them (a multiple of 32: 256 bytes)
};
NKA_HOST_DEVICE constexpr BatchLayout batch_layout(int64_t vlen, int mvec) {
  const int64_t stride = ((vlen < 1 ? 1 : vlen) + 31) / 32 * 32;
  return BatchLayout{stride, stride * (mvec + 1), (batch_ic_count(mvec) + 31) / 32 * 32, (batch_dc_count(mvec) + 31) / 32 * 32};
}
// BINARY32 STORAGE (nka_hip_batch_create_stored, NKA_HIP_BATCH_STORE_F32): the w and the v allocation hold binary32 elements at
// the SAME strides in elements -- a row then starts on a multiple of 32 floats, 128 bytes, and a pair (2t, 2t + 1) on a multiple
// of 8 bytes --, and the raw pending pair lives in two allocations of one binary64 row per system at the slot stride.  Offsets
// are in ELEMENTS of the allocation they index and formed in 64 bits.  tests/c/batch_store32_check.cpp holds all of it against a
// brute-force layout, the largest legal arguments included.
constexpr int kBatchStoreF64 = 0, kBatchStoreF32 = 1;      // = NKA_HIP_BATCH_STORE_F64 / _F32
NKA_HOST_DEVICE constexpr int64_t batch_slot_elem_bytes(int storage) { return storage == kBatchStoreF32 ? 4 : 8; }
NKA_HOST_DEVICE constexpr int64_t batch_slot_offset(const BatchLayout &l, int64_t sys, int slot /* 1-based */) {
  return sys * l.sys_stride + (int64_t)(slot - 1) * l.stride;
}
NKA_HOST_DEVICE constexpr int64_t batch_pending_offset(const BatchLayout &l, int64_t sys) { return sys * l.stride; }
// bytes of EACH of the two slot allocations (w, v) and of EACH of the two pending buffers (none with binary64 storage)
NKA_HOST_DEVICE constexpr int64_t batch_slot_alloc_bytes(const BatchLayout &l, int64_t nsys, int storage) {
  return batch_slot_elem_bytes(storage) * l.sys_stride * nsys;
}
NKA_HOST_DEVICE constexpr int64_t batch_pending_alloc_bytes(const BatchLayout &l, int64_t nsys, int storage) {
  return storage == kBatchStoreF32 ? 8 * l.stride * nsys : 0;
}
// all stored vectors of a batch: 2 nsys stride 8 (mvec + 1) bytes in binary64, 2 nsys stride (4 (mvec + 1) + 8) in binary32
NKA_HOST_DEVICE constexpr int64_t batch_vector_bytes(const BatchLayout &l, int64_t nsys, int storage) {
  return 2 * (batch_slot_alloc_bytes(l, nsys, storage) + batch_pending_alloc_bytes(l, nsys, storage));
}
// LDS of one workgroup: doubles first (offsets in doubles), then int32 (offsets in int32 from the end of the doubles)
struct BatchLds {
  int h, c, red, cc, sm, res, ndouble;      // h [(m1+1)^2], c [m1+1], red [2+2 mvec], cc [m1], sm [waves][kBatchAcc], res [kBatchAcc+1]
  int next, prev, ps, cs, hdr, nint;        // next, prev [m1+1], ps, cs [m1], hdr [8]
  NKA_HOST_DEVICE constexpr size_t bytes() const { return sizeof(double) * (size_t)ndouble + sizeof(int32_t) * (size_t)nint; }
};
NKA_HOST_DEVICE constexpr BatchLds batch_lds(int mvec) {
  const int m1 = mvec + 1;
  BatchLds l{};
  l.h = 0;
  l.c = l.h + (m1 + 1) * (m1 + 1);
  l.red = l.c + (m1 + 1);
  l.cc = l.red + (2 + 2 * mvec);
  l.sm = l.cc + m1;
  l.res = l.sm + kBatchWaves * kBatchAcc;
  l.ndouble = l.res + kBatchAcc + 1;
  l.next = 0;
  l.prev = l.next + (m1 + 1);
  l.ps = l.prev + (m1 + 1);
  l.cs = l.ps + m1;
  l.hdr = l.cs + m1;
  l.nint = l.hdr + 8;
  return l;
}
// ... and of the instances of k_batch_update that run the scalar step on wavefront 0 (nka_hip_batch_create_rows with
// nka_hip_batch_set_scalar_step; batch_scalar_step_rows of nka_batch_dev.hpp): every piece of batch_lds(mvec) AT THE SAME OFFSET,
// and behind the int32 pieces, on the next multiple of 16 bytes, the dense position-indexed matrix with its right-hand-side row,
// (mvec + 2)^2 doubles.  9 168 bytes at mvec = 20, 20 496 at 32: at most 40 KiB, four workgroups per CU by LDS, and far below the
// 64 KiB a launch may ask for without a function attribute.  tests/c/batch_rows_layout_check.cpp paints every piece.
struct BatchRowsLds {
  BatchLds b;               // the working copy, as in batch_lds
  int64_t a_off;            // bytes from the start of the LDS to the matrix: b.bytes() rounded up to 16
  int64_t a_bytes;          // bytes of the matrix
  NKA_HOST_DEVICE constexpr int64_t bytes() const { return a_off + a_bytes; }
};
NKA_HOST_DEVICE constexpr BatchRowsLds batch_rows_lds(int mvec) {
  const BatchLds b = batch_lds(mvec);
  return BatchRowsLds{b, ((int64_t)b.bytes() + 15) / 16 * 16, (int64_t)sizeof(double) * (mvec + 2) * (mvec + 2)};
}
// the instance of that step for a narrow batch of `mvec`: the smallest of 11 / 21 / 33 rows that holds mvec + 1 (no 6-row
// instance: the wide and the wave batch gain 0.86 ... 0.99 at mvec = 5, the 11-row instance serves those lists)
NKA_HOST_DEVICE constexpr int batch_rows_nlmax(int mvec) { return mvec + 1 <= 11 ? 11 : mvec + 1 <= 21 ? 21 : 33; }

// THE LANE BATCH (nka_hip_batch_create_lanes, nka_batch_lanes.hip): ONE LANE PER SYSTEM.  A workgroup is one wavefront and
// advances G = lanes_group(mvec) systems, lane l system g * G + l of group g; the grid is lanes_ngroup(nsys, G) workgroups.
// tests/c/batch_lanes_layout_check.cpp paints every piece below.
//   LDS      every lane owns a working copy -- the h, c, red, cc, next, prev, ps, cs, hdr pieces of batch_lds -- in two regions:
//            the doubles of lane l at l * dstride doubles, and behind the doubles of all G lanes the int32 of lane l at
//            l * istride int32.  THE BANK RULE: dstride is an ODD number of doubles and istride an ODD number of int32.  A
//            ds_read_b64 is served in two groups of 32 lanes with bank (a / 4) mod 64, a ds_read_b32 with bank (a / 4) mod 32:
//            with the lanes of a group at the same offset of their copies, lane l starts at dword 2 l dstride (mod 64), 32
//            distinct even values for l = 0 ... 31 exactly when dstride is odd, and at dword l istride (mod 32), 32 distinct
//            values exactly when istride is odd -- no two lanes of a group on one bank.
//   G        the largest count, at most 64 (one wavefront), whose copies fit kLanesLdsBudget.  64 KiB: the dynamic LDS a
//            launch may ask for without an attribute of the function, and two to three workgroups per CU (160 KiB).
//   SLOTS    the batch's own storage is INTERLEAVED across the systems of a group: element i of slot k (1-based) of system sys
//            lies at lanes_slot_offset = (((sys / G) (mvec + 1) + (k - 1)) vlen + i) G + sys % G doubles, so the load of
//            element i by the lanes of a wavefront is one contiguous run of G doubles.  The last group is allocated whole.
//            Every offset is formed in 64 bits.
constexpr int kLanesThreads = 64;                       // one wavefront per workgroup
constexpr int kLanesMaxVlen = 64;                       // = NKA_HIP_BATCH_LANES_MAX_VLEN = kOrdAutoMax (nka_device.hpp)
constexpr int64_t kLanesLdsBudget = 64 * 1024;          // bytes of LDS of one workgroup, at most the 160 KiB of a CU
constexpr int kLanesHdrLive = 6;                        // hdr[6]: the lane's system takes part (beside the HDR_ entries 0 ... 5)
struct LanesLds {
  int h, c, red, cc, ndouble, dstride;      // offsets in doubles inside a lane's doubles; dstride: doubles between lanes (odd)
  int next, prev, ps, cs, hdr, nint, istride;   // offsets in int32 inside a lane's int32; istride: int32 between lanes (odd)
  NKA_HOST_DEVICE constexpr int64_t lane_bytes() const { return 8 * (int64_t)dstride + 4 * (int64_t)istride; }
  NKA_HOST_DEVICE constexpr int64_t bytes(int G) const { return lane_bytes() * G; }
  // where the pieces of lane l start: in doubles from the start of the LDS, and in int32 from the end of all doubles
  NKA_HOST_DEVICE constexpr int64_t dbase(int l) const { return (int64_t)l * dstride; }
  NKA_HOST_DEVICE constexpr int64_t ibase(int l) const { return (int64_t)l * istride; }
};
NKA_HOST_DEVICE constexpr LanesLds lanes_lds(int mvec) {
  const BatchLds b = batch_lds(mvec);
  const int m1 = mvec + 1;
  LanesLds l{};
  l.h = b.h;
  l.c = b.c;
  l.red = b.red;
  l.cc = b.cc;
  l.ndouble = l.cc + m1;      // (no sm, no res: a lane's sums never leave its registers)
  l.dstride = l.ndouble | 1;
  l.next = b.next;
  l.prev = b.prev;
  l.ps = b.ps;
  l.cs = b.cs;
  l.hdr = b.hdr;
  l.nint = b.nint;
  l.istride = l.nint | 1;
  return l;
}
NKA_HOST_DEVICE constexpr int lanes_group(int mvec) {
  const int64_t g = kLanesLdsBudget / lanes_lds(mvec).lane_bytes();
  return g > kLanesThreads ? kLanesThreads : (int)g;
}
NKA_HOST_DEVICE constexpr int64_t lanes_ngroup(int64_t nsys, int G) { return (nsys + G - 1) / G; }
NKA_HOST_DEVICE constexpr int64_t lanes_group_stride(int64_t vlen, int mvec, int G) { return (int64_t)(mvec + 1) * vlen * G; }
NKA_HOST_DEVICE constexpr int64_t lanes_slot_offset(int64_t vlen, int mvec, int G, int64_t sys, int slot /* 1-based */, int64_t i) {
  return (((sys / G) * (mvec + 1) + (slot - 1)) * vlen + i) * G + sys % G;
}
// doubles of EACH of the two slot allocations (w, v), and the bytes of both together (nka_hip_batch_vector_bytes)
NKA_HOST_DEVICE constexpr int64_t lanes_slot_alloc_elems(int64_t vlen, int mvec, int G, int64_t nsys) {
  return lanes_ngroup(nsys, G) * lanes_group_stride(vlen, mvec, G);
}
NKA_HOST_DEVICE constexpr int64_t lanes_vector_bytes(int64_t vlen, int mvec, int G, int64_t nsys) {
  return 2 * 8 * lanes_slot_alloc_elems(vlen, mvec, G, nsys);
}

// THE WAVE BATCH (nka_hip_batch_create_waves, nka_batch_waves.hip): ONE WAVEFRONT PER SYSTEM.  A workgroup is kWavesGroup = 4
// wavefronts, wavefront w of workgroup g owns system 4 g + w; the grid is waves_ngroup(nsys) workgroups.  The storage and the
// control blocks are the narrow batch's (batch_layout).  tests/c/batch_waves_layout_check.cpp paints every piece below.
//   LDS      four working copies, each in the layout of batch_lds(mvec) (sm and res stay unused: a wavefront's sums never leave
//            its registers); the copy of wavefront w starts at w * copy_bytes, copy_bytes = batch_lds(mvec).bytes() rounded up to
//            16 bytes.  22.2 KiB at mvec = 20, 46.1 KiB at 32: below the 64 KiB a launch may ask for without a function attribute.
//   SUMS     a tile is kWavesTile = 128 elements, lane l owns the pair 2l, 2l + 1 of every tile: two fma per lane and tile,
//            then the six-level butterfly of wave_sum -- waves_k(n) roundings on the longest path to the result.
constexpr int kWavesGroup = 4;                          // systems (wavefronts) per workgroup, = kBatchWaves
constexpr int kWavesTile = 128;                         // elements per sweep step of a wavefront
struct WavesLds {
  BatchLds copy;            // the pieces inside one working copy (doubles first, then int32 from the end of the doubles)
  int64_t copy_bytes;       // bytes between the copies of two wavefronts: a multiple of 16
  NKA_HOST_DEVICE constexpr int64_t base(int w) const { return (int64_t)w * copy_bytes; }      // bytes from the start of the LDS
  NKA_HOST_DEVICE constexpr int64_t bytes() const { return kWavesGroup * copy_bytes; }
};
NKA_HOST_DEVICE constexpr WavesLds waves_lds(int mvec) {
  const BatchLds b = batch_lds(mvec);
  return WavesLds{b, ((int64_t)b.bytes() + 15) / 16 * 16};
}
// ... and of the instances that run the scalar step on the whole wavefront (nka_hip_batch_create_waves_rows with
// nka_hip_batch_set_scalar_step; batch_scalar_step_rows of nka_batch_dev.hpp): behind the working copy of wavefront w, the copy of
// waves_lds at the same offsets, lies that wavefront's dense position-indexed matrix with its right-hand-side row, (mvec + 2)^2
// doubles rounded up to 16 bytes; wavefront w starts at w * stride_bytes.  36 672 bytes at mvec = 20.  THE CAP ON mvec IS DERIVED:
// waves_rows_max_mvec() is the largest mvec whose four copies and four matrices fit kWavesRowsLdsLimit = 64 KiB, the dynamic LDS
// a launch may ask for without a function attribute -- 28 (64 832 bytes; 29 needs 68 992).
// tests/c/batch_waves_rows_layout_check.cpp paints every piece.
constexpr int64_t kWavesRowsLdsLimit = 64 * 1024;
struct WavesRowsLds {
  BatchLds copy;            // the pieces inside one working copy, as in WavesLds
  int64_t copy_bytes;       // = waves_lds(mvec).copy_bytes: where the matrix starts behind the start of the copy
  int64_t a_bytes;          // bytes of one matrix: a multiple of 16
  NKA_HOST_DEVICE constexpr int64_t stride_bytes() const { return copy_bytes + a_bytes; }
  NKA_HOST_DEVICE constexpr int64_t base(int w) const { return (int64_t)w * stride_bytes(); }      // the copy of wavefront w
  NKA_HOST_DEVICE constexpr int64_t a_base(int w) const { return base(w) + copy_bytes; }           // its matrix
  NKA_HOST_DEVICE constexpr int64_t bytes() const { return kWavesGroup * stride_bytes(); }
};
NKA_HOST_DEVICE constexpr WavesRowsLds waves_rows_lds(int mvec) {
  const WavesLds w = waves_lds(mvec);
  return WavesRowsLds{w.copy, w.copy_bytes, ((int64_t)sizeof(double) * (mvec + 2) * (mvec + 2) + 15) / 16 * 16};
}
NKA_HOST_DEVICE constexpr int waves_rows_max_mvec() {
  int m = 0;
  while (waves_rows_lds(m + 1).bytes() <= kWavesRowsLdsLimit) m++;      // (the size grows with mvec)
  return m;
}
// the instance of the wavefront step for a wave batch of `mvec`: the classes of the wide batch, the last one holding the cap's list
NKA_HOST_DEVICE constexpr int waves_rows_nlmax(int mvec) {
  return mvec + 1 <= 6 ? 6 : mvec + 1 <= 11 ? 11 : mvec + 1 <= 21 ? 21 : waves_rows_max_mvec() + 1;
}
NKA_HOST_DEVICE constexpr int64_t waves_ngroup(int64_t nsys) { return (nsys + kWavesGroup - 1) / kWavesGroup; }
NKA_HOST_DEVICE constexpr int64_t waves_k(int64_t n) { return 2 * (((n < 1 ? 1 : n) + kWavesTile - 1) / kWavesTile) + 6; }

// THE WIDE BATCH (nka_hip_batch_create_wide, nka_batch_wide.hip): a system is nchunk = ceil(vlen / kWideChunk) chunks, one
// workgroup each, and an update is four launches: norm, sums, scalar, combine.  tests/c/batch_wide_layout_check.cpp paints
// every piece below.  (NKA_BATCH_WIDE_CHUNK: the candidate builds that chose the constant, tools/batch_throughput.py --wide.)
#ifndef NKA_BATCH_WIDE_CHUNK
#define NKA_BATCH_WIDE_CHUNK 2048
#endif
constexpr int64_t kWideChunk = NKA_BATCH_WIDE_CHUNK;      // = NKA_HIP_BATCH_WIDE_CHUNK: a multiple of the tile of 512 elements
constexpr int kWideMaxChunks = 1024;                      // bounds the chunk-order chain and the partial buffer
static_assert(kWideChunk % 512 == 0 && kWideChunk >= 512, "a chunk is whole tiles");
NKA_HOST_DEVICE constexpr int64_t wide_nchunk(int64_t vlen) { return ((vlen < 1 ? 1 : vlen) + kWideChunk - 1) / kWideChunk; }
NKA_HOST_DEVICE constexpr int64_t wide_chunk_len(int64_t vlen, int64_t c) {
  return vlen - c * kWideChunk < kWideChunk ? vlen - c * kWideChunk : kWideChunk;
}
// partial sums: entry j of red[] (0 <= j < 2 + 2 mvec) of system sys, chunk c -- the chunks of an entry lie together, in order
NKA_HOST_DEVICE constexpr int64_t wide_part_count(int64_t nsys, int mvec, int64_t nchunk) { return nsys * (2 + 2 * mvec) * nchunk; }
NKA_HOST_DEVICE constexpr int64_t wide_part_index(int64_t sys, int entry, int64_t c, int mvec, int64_t nchunk) {
  return (sys * (2 + 2 * mvec) + entry) * nchunk + c;
}
// THE SOLVE STEP of a wide batch (nka_hip_batch_create_wide_step, nka_batch_wide.hip): one partial of <f,f> per system and
// chunk in a buffer of its own, the chunks of a system together and in order -- the partials above keep their cells.
// tests/c/batch_wide_step_layout_check.cpp paints every cell.
NKA_HOST_DEVICE constexpr int64_t wide_fpart_count(int64_t nsys, int64_t nchunk) { return nsys * nchunk; }
NKA_HOST_DEVICE constexpr int64_t wide_fpart_index(int64_t sys, int64_t c, int64_t nchunk) { return sys * nchunk + c; }
// PER-SYSTEM LENGTHS (nka_hip_batch_set_lengths): a system of len elements, 1 <= len <= vlen, in a batch laid out for vlen.  It
// owns the first wide_len_nchunk(len) chunks of its row -- the chunks of a batch created with vlen = len, of the same lengths --
// and its partials keep the BATCH's nchunk as stride, so every index it reads lies in its own cells.  The workgroups of the
// other chunks return before they read anything.  tests/c/batch_lengths_check.cpp holds all of it for every len.
NKA_HOST_DEVICE constexpr bool batch_len_valid(int64_t len, int64_t vlen) { return len >= 1 && len <= vlen; }
NKA_HOST_DEVICE constexpr int64_t wide_len_nchunk(int64_t len) { return wide_nchunk(len); }
NKA_HOST_DEVICE constexpr bool wide_len_owns(int64_t len, int64_t c) { return c >= 0 && c < wide_len_nchunk(len); }
NKA_HOST_DEVICE constexpr int64_t wide_len_chunk_len(int64_t len, int64_t c) { return wide_chunk_len(len, c); }      // (c owned)
// DIAGONAL DOT WEIGHTS of a wide batch (nka_hip_batch_create_wide_ext): element 0 of chunk c of the weight row of system sys, in
// doubles from the start of the batch's weight buffer -- rows lie wgt_stride apart, the slot stride (a multiple of 32 doubles),
// or 0 apart in the form all systems share; a chunk starts on a multiple of kWideChunk elements, so the offset is a multiple of
// 16 bytes in either form.  Every product is 64-bit.  tests/c/batch_wide_weights_check.cpp holds it against __int128 and walks
// what a workgroup reads from there for every length.
NKA_HOST_DEVICE constexpr int64_t wide_wgt_offset(int64_t sys, int64_t wgt_stride, int64_t c) { return sys * wgt_stride + c * kWideChunk; }
// LDS of the sums and the combine kernel: doubles first, then int32 (a piece a kernel lacks has length 0; the norm kernel
// holds sm [waves] and res [2] only, declared where it uses them)
struct WideLds {
  int stage, sm, res, cc, ndouble;      // stage [nchunk]: the partials of <d,d>; sm [waves][nacc]; res [nacc + 1]; cc [m1]
  int next, ps, cs, hdr, nint;          // next [m1+1], ps [m1], cs [m1], hdr [8]
  NKA_HOST_DEVICE constexpr size_t bytes() const { return sizeof(double) * (size_t)ndouble + sizeof(int32_t) * (size_t)nint; }
};
NKA_HOST_DEVICE constexpr WideLds wide_sums_lds(int mvec, int nchunk) {
  const int m1 = mvec + 1;
  WideLds l{};
  l.stage = 0;
  l.sm = l.stage + nchunk;
  l.res = l.sm + kBatchWaves * kBatchAcc;
  l.cc = l.res + kBatchAcc + 1;
  l.ndouble = l.cc;
  l.next = 0;
  l.ps = l.next + (m1 + 1);
  l.cs = l.ps + m1;
  l.hdr = l.cs;
  l.nint = l.hdr + 8;
  return l;
}
NKA_HOST_DEVICE constexpr WideLds wide_combine_lds(int mvec) {
  const int m1 = mvec + 1;
  WideLds l{};
  l.stage = l.sm = l.res = l.cc = 0;
  l.ndouble = l.cc + m1;
  l.next = l.ps = l.cs = 0;
  l.hdr = l.cs + m1;
  l.nint = l.hdr + 8;
  return l;
}
// LDS of the scalar kernel: the working copy of the narrow kernel (batch_lds), then stage [nchunk] behind its doubles
struct WideScalarLds {
  BatchLds b;      // (b.ndouble counts the stage too: the int32 pieces start behind it)
  int stage;
};
NKA_HOST_DEVICE constexpr WideScalarLds wide_scalar_lds(int mvec, int nchunk) {
  WideScalarLds l{batch_lds(mvec), 0};
  l.stage = l.b.ndouble;
  l.b.ndouble += nchunk;
  return l;
}
// ... and of its instances that run the scalar step on one wavefront (nka_hip_batch_set_scalar_step; batch_scalar_step_rows of
// nka_batch_dev.hpp): the same pieces, then the dense position-indexed matrix with its right-hand-side row, a [(m1+1)^2], behind
// the stage.  13.0 KiB at mvec = 20 and 24.0 KiB at 32 with 512 chunks, 28.0 KiB with 1024: below the 64 KiB a launch may ask for
// without a function attribute.  tests/c/batch_wide_rows_layout_check.cpp paints every piece.
constexpr int kWideRowsMaxList = 33;                      // the longest list the wavefront step holds in registers: mvec + 1 <= 33
struct WideScalarRowsLds {
  BatchLds b;      // (b.ndouble counts the stage and the matrix too: the int32 pieces start behind them)
  int stage, a;
};
NKA_HOST_DEVICE constexpr WideScalarRowsLds wide_scalar_rows_lds(int mvec, int nchunk) {
  WideScalarRowsLds l{batch_lds(mvec), 0, 0};
  l.stage = l.b.ndouble;
  l.a = l.stage + nchunk;
  l.b.ndouble = l.a + (mvec + 2) * (mvec + 2);
  return l;
}
// the instance of the wavefront step for a batch of `mvec`: the smallest of 6 / 11 / 21 / 33 rows that holds mvec + 1
NKA_HOST_DEVICE constexpr int wide_rows_nlmax(int mvec) { return mvec + 1 <= 6 ? 6 : mvec + 1 <= 11 ? 11 : mvec + 1 <= 21 ? 21 : kWideRowsMaxList; }

}  // namespace nka_host
