// nka_device.hpp -- the device functions the kernels of this library are written in, with their constants: list word,
// peer-to-peer exchange, fixed-order reductions, 8/16-byte accesses, operands of the sums, the reference-order sum, tile tickets,
// the combine statement, Lst and the scalar step's list surgery / Cholesky / substitutions.  It defines NO kernel.
#pragma once

#include "nka_ctl.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "nka_device.hpp is written for gfx950 (CDNA4) only: v_permlane32_swap / v_permlane16_swap reductions, 160 KiB LDS, tile shapes measured on MI355X.  Build with --offload-arch=gfx950."
#endif

namespace nka {

constexpr int kBlock = 256;  // 4 wavefronts of 64
constexpr int kWavesPerBlock = kBlock / 64;   // (kMaxGrid, the bound on a persistent grid: nka_ctl.hpp)

#ifdef NKA_SOLVE_STAMPS
#define NKA_STAMP(ctl, i) do { if (threadIdx.x == 0) (ctl).stamps()[i] = (double)__builtin_amdgcn_s_memtime(); } while (0)
#define NKA_STAMP0(ctl, i) do { if (blockIdx.x == 0 && threadIdx.x == 0) (ctl).stamps()[i] = (double)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define NKA_STAMP(ctl, i) do { } while (0)
#define NKA_STAMP0(ctl, i) do { } while (0)
#endif

// PB, first thread of block 0, before its first tile: the store is posted while the pass streams, so it costs the
// update nothing and has landed long before the pass ends (a caller that synchronises once per iteration -- every
// solver reads a residual norm -- sees the word of the update it has just waited for).  ncomb + 1 = the combined
// entries plus the new pending pair = the list length at the exit of this update.
// Words 1..3 of the record belong to the out-of-place updates: the buffers the update displaced (PC_OLD_W / PC_OLD_V),
// written BEFORE the number of that update, which is stored with release semantics; other updates leave them alone.
__device__ __forceinline__ void list_word_publish(const Ctl &ctl, int ncomb, int swapping) {
  if (ctl.hw != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    if (swapping) {      // an out-of-place update: what it displaced (words 1, 2), then its number (word 3)
      ctl.hw[1] = (unsigned long long)ctl.pc[PC_OLD_W];       // (offsets from Vecs::w, like everything in the block)
      ctl.hw[2] = (unsigned long long)ctl.pc[PC_OLD_V];
      __hip_atomic_store(ctl.hw + 3, ctl.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __hip_atomic_store(ctl.hw, (ctl.seq << kListWordLenBits) | (unsigned long long)(ncomb + 1), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- the peer-to-peer exchange (struct P2P, nka_ctl.hpp) ----
// where entry e of row `src` lies in rank q's mailbox: the value, and its flag
__device__ inline double *p2p_val(const P2P &x, int q, int slot, int src, int e) {
  return reinterpret_cast<double *>(x.base + x.off[q]) + ((size_t)slot * x.n + src) * x.cap + e;
}
__device__ inline unsigned long long *p2p_flag(const P2P &x, int q, int slot, int src, int e) {
  return reinterpret_cast<unsigned long long *>(x.base + x.off[q]) + (size_t)2 * x.n * x.cap + ((size_t)slot * x.n + src) * x.cap + e;
}
// One lane sends entry e of exchange `seq` to rank q: the value, then the flag released at system scope.
__device__ __forceinline__ void p2p_send_one(const P2P &x, int q, unsigned long long seq, int e, double v) {
  const int slot = (int)(seq & 1ull);
  __hip_atomic_store(p2p_val(x, q, slot, x.me, e), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(p2p_flag(x, q, slot, x.me, e), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// A whole wavefront sends entry e (lanes q = lane, lane + 64, ... < n each serve one peer); v is uniform.
__device__ __forceinline__ void p2p_send_wave(const P2P &x, unsigned long long seq, int e, double v) {
  for (int q = threadIdx.x & 63; q < x.n; q += 64) p2p_send_one(x, q, seq, e, v);
}
// Entry e of exchange `seq`, summed over the ranks in rank order (one lane).  Bounded wait.
__device__ __forceinline__ double p2p_gather_one(const P2P &x, unsigned long long seq, int e) {
  const int slot = (int)(seq & 1ull);
  double acc = 0.0;
  bool late = false;
  const long long t0 = wall_clock64();
  for (int r = 0; r < x.n; r++) {
    unsigned long long *fl = p2p_flag(x, x.me, slot, r, e);
    while (!late && __hip_atomic_load(fl, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != seq) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock64() - t0 > x.timeout_ticks) late = true;
    }
    const double v = __hip_atomic_load(p2p_val(x, x.me, slot, r, e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    acc = (r == 0) ? v : acc + v;
  }
  if (late) {
    *x.status = 1;
    acc = __builtin_nan("");
  }
  return acc;
}
// The gather at the head of the scalar step: red[e] <- sum over ranks, e < count, by the threads of ONE workgroup; then the
// exchange number moves on.  (Each thread reads back only entries it wrote itself or after the barrier.)
__device__ __forceinline__ void p2p_gather_block(const P2P &x, double *red, int count) {
  const unsigned long long seq = *x.xseq;
  for (int e = threadIdx.x; e < count; e += blockDim.x) red[e] = p2p_gather_one(x, seq, e);
  __syncthreads();
  if (threadIdx.x == 0) *x.xseq = seq + 1;
}

__device__ __forceinline__ double readlane_f64(double x, int src_lane_uniform) {
  union { double d; int i[2]; } u;
  u.d = x;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], src_lane_uniform);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], src_lane_uniform);
  return u.d;
}

// ---- reductions ---------------------------------------------------------------
// Sum over the wavefront, valid in LANE 0: the butterfly x += x[lane + off], off = 32, 16, 8, 4, 2, 1 -- the tree
// __shfl_down builds, hence the same bits -- but through REGISTERS: gfx950's v_permlane32_swap / v_permlane16_swap
// for the two steps that cross a row of 16 lanes, DPP row_shl for the four inside row 0 (after the step with
// offset 16 only lanes 0..15 carry partial sums that reach lane 0).  __shfl_down is two ds_bpermute_b32 and an
// LDS wait per step: the 42 sums of a PA block took 22 k cycles (~9.5 us of a 15 us launch at n = 1e5) that way.
__device__ __forceinline__ double swap_sum32(double A, double B);
__device__ __forceinline__ double swap_sum16(double A, double B);
template <int N> __device__ __forceinline__ double row_shl_sum(double x);
__device__ __forceinline__ double wave_sum(double x) {
  x = swap_sum32(x, x);
  x = swap_sum16(x, x);
  x = row_shl_sum<8>(x);
  x = row_shl_sum<4>(x);
  x = row_shl_sum<2>(x);
  return row_shl_sum<1>(x);
}

// The first two butterfly steps for TWO sums at once.  swap_sum32(A, B): lanes 0..31 get A[i] + A[i+32], lanes
// 32..63 get B[i-32] + B[i]; swap_sum16(A, B), row by row of 16 lanes: (A.r0 + A.r1, B.r0 + B.r1, A.r2 + A.r3,
// B.r2 + B.r3).  The same pairs the butterfly of wave_sum adds, parked in the half / row that the butterfly
// leaves idle.
__device__ __forceinline__ double swap_sum32(double A, double B) {
  union U { double d; unsigned u[2]; } a, b;
  a.d = A;
  b.d = B;
#pragma unroll
  for (int w = 0; w < 2; w++) {
    const auto r = __builtin_amdgcn_permlane32_swap(a.u[w], b.u[w], false, false);
    a.u[w] = r[0];
    b.u[w] = r[1];
  }
  return a.d + b.d;
}
__device__ __forceinline__ double swap_sum16(double A, double B) {
  union U { double d; unsigned u[2]; } a, b;
  a.d = A;
  b.d = B;
#pragma unroll
  for (int w = 0; w < 2; w++) {
    const auto r = __builtin_amdgcn_permlane16_swap(a.u[w], b.u[w], false, false);
    a.u[w] = r[0];
    b.u[w] = r[1];
  }
  return a.d + b.d;
}
// x[i] + x[i+N] inside every row of 16 lanes (lanes whose partner is outside the row keep x + x: never used)
template <int N> __device__ __forceinline__ double row_shl_sum(double x) {
  union U { double d; unsigned u[2]; } a, b;
  a.d = x;
  b.u[0] = __builtin_amdgcn_update_dpp(a.u[0], a.u[0], 0x100 + N, 0xf, 0xf, false);
  b.u[1] = __builtin_amdgcn_update_dpp(a.u[1], a.u[1], 0x100 + N, 0xf, 0xf, false);
  return a.d + b.d;
}

// Sum NACC per-thread accumulators over the block (fixed order: lanes by butterfly, then waves 0..3) and store
// column a at partials[a*G + block].  Every sum is the tree of wave_sum -- the same bits -- but the NACC
// butterflies share their steps: the step with offset 32 folds accumulators k and k + H1 into one register
// (lower / upper half of the wavefront), the step with offset 16 folds registers k and k + H2 (even / odd rows),
// the four steps inside a row then serve four accumulators each.  ~NACC/4 x 6 exchange-and-add groups instead of
// NACC x 6 (42 sums of PA at m = 20: 9.9 k -> ~3 k cycles; with __shfl_down 22 k).
template <int NACC>
__device__ __forceinline__ void block_reduce_store(const double (&acc)[NACC], double *partials, int G) {
  __shared__ double sm[kWavesPerBlock][NACC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr int H1 = (NACC + 1) / 2, H2 = (H1 + 1) / 2;
  double r1[H1], r2[H2];
#pragma unroll
  for (int k = 0; k < H1; k++) r1[k] = swap_sum32(acc[k], acc[k + H1 < NACC ? k + H1 : k]);
#pragma unroll
  for (int k = 0; k < H2; k++) r2[k] = swap_sum16(r1[k], r1[k + H2 < H1 ? k + H2 : k]);
  const int row = lane >> 4;
#pragma unroll
  for (int k = 0; k < H2; k++) {
    double x = r2[k];
    x = row_shl_sum<8>(x);
    x = row_shl_sum<4>(x);
    x = row_shl_sum<2>(x);
    x = row_shl_sum<1>(x);
    // row 0: accumulator k; row 1: k + H2 (a register of the second half); rows 2, 3: the same + H1
    const int reg = k + (row & 1) * H2;
    const int a = reg + (row >> 1) * H1;
    if ((lane & 15) == 0 && reg < H1 && a < NACC) sm[wv][a] = x;
  }
  __syncthreads();
  for (int a = threadIdx.x; a < NACC; a += kBlock) {
    double r = sm[0][a];
#pragma unroll
    for (int q = 1; q < kWavesPerBlock; q++) r += sm[q][a];
    partials[(size_t)a * G + blockIdx.x] = r;
  }
}

// ---- 8-B / 16-B per lane streaming accesses ---------------------------------------
// Non-temporal (nt) loads and stores (nt stores: +2-3 % on the mixed pass against plain ones).
typedef double d2 __attribute__((ext_vector_type(2)));
template <int VEC> struct VecT;
template <> struct VecT<1> { using type = double; };
template <> struct VecT<2> { using type = d2; };

template <int VEC> __device__ __forceinline__ typename VecT<VEC>::type ld(const double *p);
template <> __device__ __forceinline__ double ld<1>(const double *p) { return __builtin_nontemporal_load(p); }
template <> __device__ __forceinline__ d2 ld<2>(const double *p) {
  return __builtin_nontemporal_load(reinterpret_cast<const d2 *>(p));
}
__device__ __forceinline__ void st(double *p, double x) { __builtin_nontemporal_store(x, p); }
__device__ __forceinline__ void st(double *p, d2 x) { __builtin_nontemporal_store(x, reinterpret_cast<d2 *>(p)); }

__device__ __forceinline__ double ex(double x, int) { return x; }
__device__ __forceinline__ double ex(d2 x, int i) { return x[i]; }
__device__ __forceinline__ void setc(double &x, int, double val) { x = val; }
__device__ __forceinline__ void setc(d2 &x, int i, double val) { x[i] = val; }

// `normed` (round 5, NKA_HIP_SUMS_BLOCKED_ROUNDED): the norm is already known -- red[0] holds the GLOBAL sum d^2 of a pass of
// its own (k_norm_diff) -- and the sums are formed on the ROUNDED w1' = fl(d/s) (bit 1 of `normed`: fl((1/s)*d), the
// F08-vector flavour), the value PB stores: acc[1] = <f,w1'>, acc[2+j] = <w1',w_j> as the reference defines them (F08:286-290,
// 371), in blocks and with fma.  The scalar step then takes them as they are (kSolvePrenorm).
__device__ __forceinline__ double pa_operand(double d, int normed, double s, double rs) {
  if (normed == 0) return d;
  if (s == 0.0) return 0.0;                       // (the scalar step relaxes, F08:275: these sums are dead)
  return (normed & 2) ? rs * d : d / s;
}

// SKIP OF THE LAST VECTOR.  With the list full (pending pair + mvec older entries) the oldest entry is dropped for capacity
// (F08:301-309) before its Gram entry or its projection is looked at -- unless an earlier entry is dropped as dependent
// (F08:326-345) or s == 0 relaxes (F08:275), which is rare.  `skip` of k_dots_win / k_finalize_dots / k_solve_rows:
//   kSkipMay     this launch may leave that vector out (the host's conditions hold: update_impl, skip_last_applies); it does
//                when the device agrees -- the plan says so (IC_PLAN_SKIP), a pair is pending and the plan holds mvec entries.
//                PA then treats the last plan entry as a dead ring slot, its two sums read 0, and a scalar step that finds
//                it needs them after all raises IC_REDO and returns BEFORE any store of state;
//   kSkipRepair  a guarded launch behind that scalar step: returns at once unless IC_REDO is set.  The three of them form
//                the two missing sums (same grid, same per-thread tile sequence => the bits of the unskipped pass), store
//                them, and run the scalar step again, which clears IC_REDO and holds the skip off for mvec updates.
enum { kSkipMay = 1, kSkipRepair = 2 };
__device__ __forceinline__ bool skip_last_planned(const Ctl &ctl, int skip, int pending, int nolder) {
  return (skip & kSkipMay) && pending && nolder == ctl.mvec && ctl.ic[IC_PLAN_SKIP] != 0;
}
__device__ __forceinline__ bool skip_repair_idle(const Ctl &ctl, int skip) { return (skip & kSkipRepair) && ctl.ic[IC_REDO] == 0; }

// DIAGONAL WEIGHTS (nka_hip_set_dot_weights): every product of the weighted passes takes fl(w_i * a_i) as its FIRST operand
// and the unweighted value as its second, fma(fl(w a), b, acc); the order of the sums is the unweighted kernels'.  The
// passes that form sums (k_norm_diff, k_dots, k_dots_win) take `bool WGT = false`: with false these helpers return `a` and
// no weight is loaded -- the instructions of the plain kernels -- with true the weights (n doubles, 256-byte aligned, found
// through Ctl::pc[PC_WGT] like every other buffer) stream beside f and w1 in the same 16-byte non-temporal loads.
template <bool WGT, class V>
__device__ __forceinline__ double wgt_first(const V &om, int q, double a) {
  if constexpr (WGT) return ex(om, q) * a;
  else return a;
}
template <bool WGT>
__device__ __forceinline__ double wgt_at(const double *__restrict__ wgt, int64_t i, double a) {
  if constexpr (WGT) return wgt[i] * a;
  else return a;
}

// ---- sums in the REFERENCE'S ORDER (k_dots_ordered) ----
constexpr int kOrdThreads = 256;
constexpr int kOrdChunkMax = 512;
constexpr int kOrdMaxMvec = 250;                     // two sums per thread and eight elements per LDS row at least
constexpr int kOrdAutoMax = 64;                      // NKA_HIP_SUMS_AUTO sums in the reference's order up to this length (where it costs nothing)
constexpr int kOrdLdsDoubles = 16000;                // 125 KiB of dynamic LDS (one workgroup; 160 KiB per CU on gfx950) ...
constexpr int kOrdLdsPad = 16;                       // ... plus what ord_sum may read past the last row
__host__ __device__ inline int ord_chunk(int rows) {
  int c = kOrdLdsDoubles / (rows < 1 ? 1 : rows) - 1;
  return c > kOrdChunkMax ? kOrdChunkMax : (c < 8 ? 8 : c);
}
__host__ __device__ inline size_t ord_lds_bytes(int rows) {
  return sizeof(double) * ((size_t)rows * (ord_chunk(rows) + 1) + kOrdLdsPad);
}
// a + x[0]*y[0] + x[1]*y[1] + ... in THAT order, one rounding per product and per addition; the LDS reads of the next eight
// elements are in flight while the eight additions of this batch wait for one another (rows are padded: reading up to
// seven elements past `len` stays inside the allocation; those products are not added).
__device__ __forceinline__ double ord_sum(double a, const double *x, const double *y, int len) {
#pragma clang fp contract(off)      // products and additions stay separate roundings whatever the build's flags
  double xb[8], yb[8];
#pragma unroll
  for (int u = 0; u < 8; u++) { xb[u] = x[u]; yb[u] = y[u]; }
  for (int i0 = 0; i0 < len; i0 += 8) {
    double xn[8], yn[8];
#pragma unroll
    for (int u = 0; u < 8; u++) { xn[u] = x[i0 + 8 + u]; yn[u] = y[i0 + 8 + u]; }
    if (i0 + 8 <= len) {
#pragma unroll
      for (int u = 0; u < 8; u++) a = a + xb[u] * yb[u];
    } else {
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (i0 + u < len) a = a + xb[u] * yb[u];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) { xb[u] = xn[u]; yb[u] = yn[u]; }
  }
  return a;
}
// Chunk [c0, c0+len) of the older w's into LDS rows 2..: eight rows at a time, two elements of each row per thread (a chunk
// has at most 512 elements): sixteen loads in flight per thread, the row addresses uniform (scalar loads of the plan).
__device__ __forceinline__ void ord_load_older(double *sh, int S, const Vecs &vs, const long long *pw, int nolder, int64_t c0, int len) {
  const int i0 = threadIdx.x, i1 = threadIdx.x + kOrdThreads;
  static_assert(kOrdChunkMax <= 2 * kOrdThreads, "two elements of a row per thread cover a chunk");
  for (int p0 = 0; p0 < nolder; p0 += 8) {
    double v0[8], v1[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int p = p0 + u < nolder ? p0 + u : nolder - 1;      // (the last group repeats a row: the loads stay unconditional)
      const double *wp = vs.w + pw[p] + c0;
      v0[u] = i0 < len ? wp[i0] : 0.0;
      v1[u] = i1 < len ? wp[i1] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      if (p0 + u >= nolder) continue;
      double *dst = sh + (size_t)(2 + p0 + u) * S;
      if (i0 < len) dst[i0] = v0[u];
      if (i1 < len) dst[i1] = v1[u];
    }
  }
}

// ---- PB: the combine statement (COMB: see k_combine, nka_kernels.hpp) and the tile tickets ----
template <int COMB>
__device__ __forceinline__ double comb1(double x, double c, double w, double v) {
  if (COMB == 0) return (x - c * w) + c * v;
  if (COMB == 1) return ((-c) * w + c * v) + x;
  return x + c * (v - w);
}

// TILE TICKETS (`tickets` != nullptr).  With the static mapping (tile t -> block t mod G) the
// blocks of a mixed read/write pass drift apart -- by 5 % of the launch, i.e. ~40 tiles, at
// n = 1e8 -- and the chip then works on a ~40 MB window of each of the 27 streams at once.
// tools/hbm_probe (modes d, e, g; profiles/r02/hbm_probe_tile_tickets.txt) shows the same
// streams moving 8-14 % faster when every block takes its next tile from ONE global counter:
// the blocks then advance as a compact front (all end within 5 us of each other) and the DRAMs
// see one narrow window per stream.  A block's first two tiles are static (b, b + G); thread 0
// requests the tile after next with a returning atomic at the top of an iteration and publishes it
// in LDS at the end (one workgroup barrier per tile): the OTHER three waves never wait for the
// atomic, wave 0 does (see ticket_request).  `ng` counters (128 B apart), counter g serving the blocks with b % ng == g and
// the tiles = g (mod ng): a single counter saturates near 60-75 tickets/us, which short lists
// exceed.  The last block to finish resets the counters (a second counter, `done`), so a launch
// always finds them zero.  Elementwise pass: which block handles a tile changes no bit.
constexpr int kTicketStride = 32;                 // uint32 words between counters (128 B)
constexpr int kTicketGroupsMax = 8;
constexpr int kTicketWords = kTicketStride * (kTicketGroupsMax + 1);   // ng counters + `done`
constexpr unsigned kNoTicket = 0xffffffffu;

// thread 0: the tile after next of this block's group (returning atomic; the value is used a tile later).
// hipcc's atomic optimiser broadcasts the result with v_readfirstlane right behind the instruction, so
// wave 0 does wait for the atomic here (s_waitcnt vmcnt(0)); measured against an inline-asm request
// whose result is only read at the end of the tile, that costs 0-2 % of PB -- and the asm form needs a
// hand-counted s_waitcnt that turned out NOT to be safe: stores retire out of order with respect to the
// atomic, a short tile read its ticket too early (tests caught it).  The plain form stays.
__device__ __forceinline__ unsigned ticket_request(unsigned *group_counter, unsigned base, unsigned ng, unsigned grp) {
  return (atomicAdd(group_counter, 1u) + base) * ng + grp;
}
// end of a tile: thread 0 publishes what it was given, every thread learns the block's tile after next
// (two LDS words used alternately: a word is rewritten only after another barrier)
__device__ __forceinline__ int64_t ticket_publish(unsigned *s_next, unsigned &par, unsigned claimed, int64_t ntile) {
  if (threadIdx.x == 0) s_next[par] = claimed;
  __syncthreads();
  const unsigned nx = s_next[par];
  par ^= 1u;
  return nx == kNoTicket ? ntile : (int64_t)nx;
}
// end of the kernel: every ticket request of this block has returned; the block that arrives last
// resets the counters, so the next launch finds them zero
__device__ __forceinline__ void ticket_finish(unsigned *tickets, int ng, int G) {
  if (threadIdx.x != 0) return;
  unsigned *const done = tickets + kTicketGroupsMax * kTicketStride;
  if (atomicAdd(done, 1u) == (unsigned)G - 1u) {
    for (int g = 0; g < ng; g++) atomicExch(tickets + g * kTicketStride, 0u);
    atomicExch(done, 0u);
  }
}

// ---- scalar kernels: list surgery + Cholesky + substitutions on one wavefront ----
// Working copy of the control arrays in LDS (indices as in the Fortran: slots
// 1..M1, 0 = end of list).
struct Lst {
  int32_t *next, *prev;
  double *h;   // h[i*(M1+1)+j] == reference h(i,j)
  double *c;
  int first, last, free_, subspace, pending, m1, mvec;
  double vtol;
  __device__ double &H(int i, int j) { return h[i * (m1 + 1) + j]; }
};

// F08:439-457
__device__ inline void lst_relax(Lst &L) {
  if (!L.pending) return;
  const int dropped = L.first;
  L.first = L.next[dropped];
  if (L.first == 0) L.last = 0; else L.prev[L.first] = 0;
  L.next[dropped] = L.free_;
  L.free_ = dropped;
  L.pending = 0;
}

// F08:422-436
__device__ inline void lst_restart(Lst &L) {
  L.subspace = 0;
  L.pending = 0;
  L.first = 0;
  L.last = 0;
  L.free_ = 1;
  for (int k = 1; k < L.m1; k++) L.next[k] = k + 1;
  L.next[L.m1] = 0;
}

// F08:295-351.  Row-by-row Cholesky of the Gram matrix in list order; capacity
// drop of the last entry; dependence drop when the pivot hkk <= vtol^2.  The
// subtraction order of the inner loop (i ascending in list order) is preserved:
// with equal dot products the decisions equal the reference's bit for bit.
__device__ inline void lst_factor(Lst &L) {
  L.H(L.first, L.first) = 1.0;
  int k = L.next[L.first];
  int nvec = 1;
  while (k != 0) {
    nvec++;
    if (nvec > L.mvec) {
      L.next[L.last] = L.free_;
      L.free_ = k;
      L.last = L.prev[k];
      L.next[L.last] = 0;
      break;
    }
    double hkk = 1.0;
    for (int j = L.first; j != k; j = L.next[j]) {
      double hkj = L.H(j, k);
      for (int i = L.first; i != j; i = L.next[i]) hkj = hkj - L.H(k, i) * L.H(j, i);
      hkj = hkj / L.H(j, j);
      hkk = hkk - hkj * hkj;
      L.H(k, j) = hkj;
    }
    if (hkk > L.vtol * L.vtol) {
      L.H(k, k) = sqrt(hkk);
    } else {
      const int p = L.prev[k], nx = L.next[k];
      L.next[p] = nx;
      if (nx == 0) L.last = p; else L.prev[nx] = p;
      L.next[k] = L.free_;
      L.free_ = k;
      k = p;
      nvec--;
    }
    k = L.next[k];
  }
  L.subspace = 1;
  L.pending = 0;
}

// F08:369-392 (c holds the right-hand side on entry)
__device__ inline void lst_solve(Lst &L) {
  for (int j = L.first; j != 0; j = L.next[j]) {
    double cj = L.c[j];
    for (int i = L.first; i != j; i = L.next[i]) cj = cj - L.H(j, i) * L.c[i];
    L.c[j] = cj / L.H(j, j);
  }
  for (int j = L.last; j != 0; j = L.prev[j]) {
    double cj = L.c[j];
    for (int i = L.last; i != j; i = L.prev[i]) cj = cj - L.H(i, j) * L.c[i];
    L.c[j] = cj / L.H(j, j);
  }
}

// F08:406-417
__device__ inline void lst_prepend(Lst &L, int slot) {
  L.prev[slot] = 0;
  L.next[slot] = L.first;
  if (L.first == 0) L.last = slot; else L.prev[L.first] = slot;
  L.first = slot;
  L.pending = 1;
}

constexpr int kSolveThreads = 64;  // ONE wavefront

// ---- the transfers between a control block and an Lst ----
// the working arrays ARE the control block in global memory: no copy in, none back
__device__ __forceinline__ void lst_on_ctl(Lst &L, const Ctl &ctl) {
  L.m1 = ctl.m1();
  L.mvec = ctl.mvec;
  L.h = ctl.h();
  L.c = ctl.c();
  L.next = ctl.next();
  L.prev = ctl.prev();
}
// the five list scalars, control block -> Lst and back.  (vtol stays a line at the callers and the copy INTO a working copy
// stays written out in lst_load and k_batch_update: as functions they moved instructions of kernels held to their machine code.)
__device__ __forceinline__ void lst_load_scalars(Lst &L, const Ctl &ctl) {
  L.subspace = ctl.ic[IC_SUBSPACE];
  L.pending = ctl.ic[IC_PENDING];
  L.first = ctl.ic[IC_FIRST];
  L.last = ctl.ic[IC_LAST];
  L.free_ = ctl.ic[IC_FREE];
}
__device__ __forceinline__ void lst_store_scalars(const Lst &L, const Ctl &ctl) {
  ctl.ic[IC_SUBSPACE] = L.subspace;
  ctl.ic[IC_PENDING] = L.pending;
  ctl.ic[IC_FIRST] = L.first;
  ctl.ic[IC_LAST] = L.last;
  ctl.ic[IC_FREE] = L.free_;
}
// h, c and the links of a working copy back to the control block, strided over the `nthreads` threads that call
__device__ __forceinline__ void lst_copy_out(const Lst &L, const Ctl &ctl, int nthreads) {
  const int m1 = L.m1, nh = (m1 + 1) * (m1 + 1);
  for (int i = threadIdx.x; i < nh; i += nthreads) ctl.h()[i] = L.h[i];
  for (int i = threadIdx.x; i < m1 + 1; i += nthreads) {
    ctl.c()[i] = L.c[i];
    ctl.next()[i] = L.next[i];
    ctl.prev()[i] = L.prev[i];
  }
}

// dynamic LDS: next[M1+1], prev[M1+1] (int32) then h[(M1+1)^2], c[M1+1] (double).
// in_global != 0 (mvec > 140: the (mvec+2)^2 matrix no longer fits the 160 KiB of LDS): the working
// arrays ARE the control block in global memory -- no copy in, none back; slow (every step of the
// list-ordered loops is a dependent global access), but the reference has no limit on mvec
// (F08:185-200) and neither has this build.
__device__ inline void lst_load(Lst &L, const Ctl &ctl, unsigned char *smem, int in_global = 0) {
  const int m1 = ctl.m1(), nh = (m1 + 1) * (m1 + 1);
  if (in_global) {
    lst_on_ctl(L, ctl);
  } else {
    L.m1 = m1;
    L.mvec = ctl.mvec;
    L.h = reinterpret_cast<double *>(smem);
    L.c = L.h + nh;
    L.next = reinterpret_cast<int32_t *>(L.c + (m1 + 1));
    L.prev = L.next + (m1 + 1);
    for (int i = threadIdx.x; i < nh; i += kSolveThreads) L.h[i] = ctl.h()[i];
    for (int i = threadIdx.x; i < m1 + 1; i += kSolveThreads) {
      L.c[i] = ctl.c()[i];
      L.next[i] = ctl.next()[i];
      L.prev[i] = ctl.prev()[i];
    }
  }
  lst_load_scalars(L, ctl);
  L.vtol = ctl.dc[DC_VTOL];
  __syncthreads();
}

__host__ __device__ constexpr size_t lst_smem_bytes(int mvec) {
  const int m1 = mvec + 1;
  return (size_t)((m1 + 1) * (m1 + 1) + (m1 + 1)) * sizeof(double) + 2 * (size_t)(m1 + 1) * sizeof(int32_t);
}

// Lane 0 writes the scalars and the plan for the next update; all lanes copy
// the arrays back.
__device__ inline void lst_store(Lst &L, const Ctl &ctl, int in_global = 0) {
  __syncthreads();
  if (!in_global) lst_copy_out(L, ctl, kSolveThreads);
  if (threadIdx.x == 0) {
    lst_store_scalars(L, ctl);
    // plan for the next update's PA
    ctl.ic[IC_PLAN_PENDING] = L.pending;
    ctl.ic[IC_PLAN_FIRST] = L.first;
    int n = 0;
    int32_t *ps = ctl.plan_slots();
    const long long *wt = ctl.wtab();
    for (int k = L.pending ? L.next[L.first] : L.first; k != 0; k = L.next[k]) {
      ctl.plan_w()[n] = wt[k];       // the streaming passes get addresses, not slots (Ctl::pc)
      ps[n++] = k;
    }
    ctl.ic[IC_PLAN_NOLDER] = n;
    ctl.pc[PC_FIRST_W] = wt[L.first];      // (entry 0 of the table is a valid dummy: first == 0 without a list)
  }
}

// The slot that receives the new pair gets its buffers here.  An out-of-place update (swap_w / swap_v != kNoBuffer,
// nka_hip_accel_update_swap) EXCHANGES them: the caller's buffer, which holds f_in, becomes the slot's w -- no copy --
// and a spare buffer of the library becomes its v; what the slot held before is reported in PC_OLD_W / PC_OLD_V.
__device__ inline void assign_new_buffers(const Ctl &ctl, int slot, long long swap_w, long long swap_v) {
  long long *wt = ctl.wtab(), *vt = ctl.vtab();
  if (swap_w != kNoBuffer) { ctl.pc[PC_OLD_W] = wt[slot]; wt[slot] = swap_w; }      // (other updates leave PC_OLD_* alone:
  if (swap_v != kNoBuffer) { ctl.pc[PC_OLD_V] = vt[slot]; vt[slot] = swap_v; }      //  the host may collect them later)
  ctl.pc[PC_NEW_W] = wt[slot];
  ctl.pc[PC_NEW_V] = vt[slot];
}

// `mode` of the scalar step.  kSolveRcp: the F08-vector flavour, whose
// normalisation is a multiplication by 1/s.  kSolvePrenorm: red[1] and the Gram
// row red[2..] were already evaluated on the NORMALISED w1' (the host
// dot-product path, nka_hip_set_host_dot) and are taken as they are.
enum { kSolveRcp = 1, kSolvePrenorm = 2 };
__device__ __forceinline__ double solve_nrm(double x, double s, double rs, int mode) {
  return (mode & kSolvePrenorm) ? x : ((mode & kSolveRcp) ? rs * x : x / s);
}

}  // namespace nka
