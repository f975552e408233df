// nka_kernels.hpp -- gfx950 (CDNA4, wave64) kernels of the NKA accel_update hot path.
//
// One update is TWO HBM-streaming passes around one scalar step:
//   PA  k_dots    : pure-read pass.  While w1 (the raw previous f), f and the L
//                   stored w's stream past once it accumulates ALL the inner
//                   products the update needs:  sum d^2 with d = w1 - f
//                   (F08:266-267), <f,d>, <d,w_k> (F08:286-290) and <f,w_k>
//                   (F08:371).  The Gram row of the normalised w1' = d/s follows
//                   by one scalar division per entry in k_solve.  Reads (2+L)n
//                   words, writes nothing -- a kernel without stores streams at
//                   ~6.8 TB/s on MI355X, one with any store at ~5.3 TB/s
//                   (tools/hbm_probe.hip), so every store of the update is
//                   concentrated in PB.
//   --  k_finalize_dots (fixed-order sums => bitwise reproducible), [one
//       all-reduce of 2+2*mvec doubles], k_solve (s, s == 0 -> relax F08:275,
//       Cholesky with drops F08:295-351, both substitutions F08:369-392, list
//       surgery) on ONE wavefront.
//   PB  k_combine : w1' = (w1-f)/s and v1' = v1/s (F08:282-283) formed in
//                   registers and stored, f <- f - sum c_k w_k + sum c_k v_k in
//                   list order (F08:395-399), and the two ring stores w_new = f_in
//                   (F08:361), v_new = f_out (F08:404).  Reads (1+2k)n, writes 5n;
//                   in the C flavour's compact storage (see k_combine) (2+k)n.
// That moves 8n(8+L+2k) bytes per update -- 8n(9+L+k) compact; one stream less with the list full, whose last vector PA
// does not read (kSkipMay, nka_device.hpp) -- against the
// 8n(11+L+2k) of the three-pass schedule of SURVEY.md 8(d), with ONE
// synchronisation point.
// Round 5: lists longer than 32 run PA and PB as balanced passes of the same window kernels (`base` into the plans);
// with several ranks the final sums can go straight into every rank's mailbox and the scalar step gathers them (struct
// P2P: no communication kernel); the reference-order pass k_dots_ordered continues the running sums from rank to rank.
//
// Everything is fp64 and bandwidth bound (0.29 flop/byte): no MFMA.  Vectors are
// slot-major, each slot contiguous and 256-B aligned, read with 16-B/lane
// non-temporal loads (1 KiB per wave instruction).  Compiled with
// -ffp-contract=off: the elementwise statements are rounded exactly like the
// reference expressions; the dot products use explicit fma().
//
// F08 = /root/reference/src-F08/nka_type.F90.
#pragma once

#include "nka_chain.hpp"

namespace nka {

// ONE includer only (nka_hip.hip): the non-template kernels below are plain definitions with external linkage, so a second
// translation unit that included this header would define them again and the library would not link.

// The peer-to-peer exchange (P2P) in its generic form (the hook behind nka_hip_allreduce_now, the self-test and the
// reference-order chain): one workgroup sends its `count` values to every rank, then gathers.
__global__ __launch_bounds__(128) void k_p2p_allreduce(P2P x, double *buf, int count) {
  const unsigned long long seq = *x.xseq;
  for (int i = threadIdx.x; i < count * x.n; i += blockDim.x) p2p_send_one(x, i % x.n, seq, i / x.n, buf[i / x.n]);
  __syncthreads();
  p2p_gather_block(x, buf, count);
}

// ---- PA: every inner product of the update in one pure-read pass --------------------
// MAXL stored vectors per pass; entries beyond the actual count re-read f (cache
// hit) into accumulators that are discarded, which keeps every load of a tile
// unconditional so that all MAXL+2 of them are in flight together.
// acc: [0] sum d^2, [1] <f,d>, [2+j] <d,w_j>, [2+MAXL+j] <f,w_j>.  (`normed`, WGT: pa_operand, wgt_first in nka_device.hpp)
template <int MAXL, int VEC, bool WGT = false>
__global__ __launch_bounds__(kBlock) void k_dots(Ctl ctl, Vecs vs, const double *__restrict__ f,
                                                 double *__restrict__ partials, int pass, int normed) {
  const double *wgt = WGT ? vs.w + ctl.pc[PC_WGT] : nullptr;      // (WGT = false: never read)
  using V = typename VecT<VEC>::type;
  constexpr int NACC = 2 * MAXL + 2;
  const int G = gridDim.x;
  const double s_n = normed ? sqrt(ctl.red()[0]) : 1.0, rs_n = 1.0 / s_n;
  const int pending = ctl.ic[IC_PLAN_PENDING];
  const int nolder = ctl.ic[IC_PLAN_NOLDER];
  const int base = pass * MAXL;
  // no pending pair: d = f - f = 0 and its sums are discarded by k_finalize_dots
  const double *w1 = pending ? vs.w + ctl.pc[PC_FIRST_W] : f;
  const long long *pw = ctl.plan_w();
  const double *wk[MAXL];
#pragma unroll
  for (int j = 0; j < MAXL; j++) {
    const int p = base + j;
    wk[j] = (p < nolder) ? vs.w + pw[p] : f;
  }
  double acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = 0.0;

  const int64_t ntile = vs.n / (kBlock * VEC);
  for (int64_t t = blockIdx.x; t < ntile; t += G) {
    const int64_t e = t * (kBlock * VEC) + threadIdx.x * VEC;
    const V fv = ld<VEC>(f + e);
    const V w1v = ld<VEC>(w1 + e);
    V omv = {};
    if constexpr (WGT) omv = ld<VEC>(wgt + e);
    V wkv[MAXL];
#pragma unroll
    for (int j = 0; j < MAXL; j++) wkv[j] = ld<VEC>(wk[j] + e);
    // keep all MAXL+2 loads of the tile in flight: no FMA may be scheduled
    // between them (hipcc otherwise serialises load/wait/use to save registers)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < VEC; q++) {
      const double fq = ex(fv, q);
      const double d = pa_operand(ex(w1v, q) - fq, normed, s_n, rs_n);      // F08:266 ((-1)*f + w1 in F08V:237: same bits)
      const double dw = wgt_first<WGT>(omv, q, d), fw = wgt_first<WGT>(omv, q, fq);
      acc[0] = fma(dw, d, acc[0]);
      acc[1] = fma(fw, d, acc[1]);
#pragma unroll
      for (int j = 0; j < MAXL; j++) {
        acc[2 + j] = fma(dw, ex(wkv[j], q), acc[2 + j]);
        acc[2 + MAXL + j] = fma(fw, ex(wkv[j], q), acc[2 + MAXL + j]);
      }
    }
  }
  if ((int)blockIdx.x == G - 1) {  // ragged tail, scalar
    for (int64_t i = ntile * (kBlock * VEC) + threadIdx.x; i < vs.n; i += kBlock) {
      const double fq = f[i];
      const double d = pa_operand(w1[i] - fq, normed, s_n, rs_n);
      const double dw = wgt_at<WGT>(wgt, i, d), fw = wgt_at<WGT>(wgt, i, fq);
      acc[0] = fma(dw, d, acc[0]);
      acc[1] = fma(fw, d, acc[1]);
#pragma unroll
      for (int j = 0; j < MAXL; j++) {
        const double x = wk[j][i];
        acc[2 + j] = fma(dw, x, acc[2 + j]);
        acc[2 + MAXL + j] = fma(fw, x, acc[2 + MAXL + j]);
      }
    }
  }
  block_reduce_store<NACC>(acc, partials, G);
}

// The norm pass of NKA_HIP_SUMS_BLOCKED_ROUNDED: sum d^2 with d = w1 - f (F08:266-267) over this rank's slice, two streams,
// per-block partial sums in column 0 of `partials` (k_norm_fin adds them in a fixed order).  WGT: sum fl(w d)*d, three streams.
template <bool WGT = false>
__global__ __launch_bounds__(kBlock) void k_norm_diff(Ctl ctl, Vecs vs, const double *__restrict__ f,
                                                      double *__restrict__ partials) {
  const double *wgt = WGT ? vs.w + ctl.pc[PC_WGT] : nullptr;
  const int G = gridDim.x;
  const double *w1 = vs.w + ctl.pc[PC_FIRST_W];
  const bool v2 = (reinterpret_cast<uintptr_t>(f) % 16) == 0;      // (slot bases are 256-byte aligned)
  double acc = 0.0;
  int64_t done = 0;
  if (v2) {
    const int64_t ntile = vs.n / (kBlock * 2);
    int64_t t = blockIdx.x;
    // Round 6 (the pass runs in every update since it became the default): kNormAhead tiles' loads go out before the first
    // of them is consumed -- two loads in flight per thread kept one block per CU at 4.0 TB/s; the accumulation visits the
    // tiles in the same order as the plain loop below, so the partial sums carry the same bits
    constexpr int kNormAhead = 8;
    for (; t + (int64_t)(kNormAhead - 1) * G < ntile; t += (int64_t)kNormAhead * G) {
      d2 fv[kNormAhead], wv[kNormAhead], om[kNormAhead] = {};   // (om: WGT only)
#pragma unroll
      for (int u = 0; u < kNormAhead; u++) {
        const int64_t e = (t + (int64_t)u * G) * (kBlock * 2) + threadIdx.x * 2;
        fv[u] = ld<2>(f + e);
        wv[u] = ld<2>(w1 + e);
        if constexpr (WGT) om[u] = ld<2>(wgt + e);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kNormAhead; u++)
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const double d = wv[u][q] - fv[u][q];
          acc = fma(wgt_first<WGT>(om[u], q, d), d, acc);
        }
    }
    for (; t < ntile; t += G) {
      const int64_t e = t * (kBlock * 2) + threadIdx.x * 2;
      const d2 fv = ld<2>(f + e), wv = ld<2>(w1 + e);
      d2 om = {};
      if constexpr (WGT) om = ld<2>(wgt + e);
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const double d = wv[q] - fv[q];
        acc = fma(wgt_first<WGT>(om, q, d), d, acc);
      }
    }
    done = ntile * (kBlock * 2);
  }
  // scalar path: the ragged tail (last block), or everything when f is not 16-byte aligned (grid-stride over elements)
  if (v2) {
    if ((int)blockIdx.x == G - 1)
      for (int64_t i = done + threadIdx.x; i < vs.n; i += kBlock) {
        const double d = w1[i] - f[i];
        acc = fma(wgt_at<WGT>(wgt, i, d), d, acc);
      }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < vs.n; i += (int64_t)G * kBlock) {
      const double d = w1[i] - f[i];
      acc = fma(wgt_at<WGT>(wgt, i, d), d, acc);
    }
  }
  const double one[1] = {acc};
  block_reduce_store<1>(one, partials, G);
}
// ... and its final sum, one wavefront, into red[0] (zero without a pending pair: nothing stale reaches the exchange)
__global__ __launch_bounds__(64) void k_norm_fin(Ctl ctl, const double *__restrict__ partials, int G) {
  double r = 0.0;
  for (int b = threadIdx.x; b < G; b += 64) r += partials[b];
  r = wave_sum(r);
  if (threadIdx.x == 0) ctl.red()[0] = ctl.ic[IC_PLAN_PENDING] ? r : 0.0;
}

// PA with a SMALL ROLLING WINDOW of loads.  tools/hbm_probe (mode f) showed that a
// pure-read kernel with the arithmetic of this pass runs at 7.15 TB/s when each wave
// keeps only ~6 loads in flight and re-issues one as soon as one has been consumed,
// against 6.4-6.7 TB/s for k_dots with all 22 loads of a tile in flight: fewer streams
// are open at any moment (DRAM page locality) and the fp64 FMAs interleave with the
// load issue.  Here the MAXL stored vectors of a tile go through a ring of W registers
// (slot j mod W holds vector j; when vector j has been accumulated its slot is re-loaded
// with vector j+W of this tile or vector j+W-MAXL of the block's next tile), and f, w1
// of the next tile are requested as soon as this tile's copies are in d / fq.  Same
// products, same per-thread accumulation order => same bits as k_dots.  Single pass, VEC = 2.
// `base` (round 5): the first plan entry of this launch.  A list longer than kMaxPerPass is served by several launches of
// BALANCED exact widths (33 = 17 + 16: enqueue_pa), each on its own part of the plan; only the launch with base == 0 has its
// first two sums (d^2, <f,d>) used (k_finalize_dots).
template <int MAXL, int W, bool WGT = false>
__global__ __launch_bounds__(kBlock) void k_dots_win(Ctl ctl, Vecs vs, const double *__restrict__ f,
                                                     double *__restrict__ partials, int base, int normed, int skip) {
  constexpr int VEC = 2;
  using V = typename VecT<VEC>::type;
  constexpr int NACC = 2 * MAXL + 2;
  static_assert(MAXL % W == 0, "the ring must divide the stored vectors of a tile");
  if (skip_repair_idle(ctl, skip)) return;                 // (a guarded repair launch with nothing to repair: nka_device.hpp)
  NKA_STAMP0(ctl, 10);
  const int G = gridDim.x;
  const int pending = ctl.ic[IC_PLAN_PENDING];
  const double s_n = normed ? sqrt(ctl.red()[0]) : 1.0, rs_n = 1.0 / s_n;      // (see k_dots: sums on the rounded w1')
  // the list is full and its last vector is about to be dropped for capacity: that plan entry is a dead slot too
  const int nplan = ctl.ic[IC_PLAN_NOLDER];
  const bool skip_last = skip_last_planned(ctl, skip, pending, nplan);
  const int nolder = nplan - (skip_last ? 1 : 0) - base;   // entries of the plan from `base` on (<= 0: none, every slot dead)
  // ... and where it is this launch's last ring slot (a launch as wide as the list: the only one that pays), that ONE slot
  // reads f's first tile instead of f at the tile at hand, as PB's dead slots do (half of such a re-read comes from HBM
  // again, k_combine_win).  The tile number is uniform, so the choice is made on the scalar side of the address.
  const bool last_far = skip_last && ctl.mvec - base == MAXL;
  const long long *pw = ctl.plan_w() + base;
  const double *w1p = vs.w + ctl.pc[PC_FIRST_W];           // (read whether pending or not: no branch around a load)
  const double *w1 = pending ? w1p : f;
  const double *wgt = WGT ? vs.w + ctl.pc[PC_WGT] : nullptr;      // (WGT = false: never read)
  // every plan slot is requested at once, whether the list reaches it or not (the plan array is longer than any
  // width): written as `j < nolder ? slots[j] ...` each slot became a branch around its own s_load + s_waitcnt --
  // twenty serial scalar round trips, 4.2 k cycles of prologue at m = 20 against 2 k at m = 5
  long long sl[MAXL];
#pragma unroll
  for (int j = 0; j < MAXL; j++) sl[j] = pw[j];
  const double *wk[MAXL];
#pragma unroll
  for (int j = 0; j < MAXL; j++) wk[j] = (j < nolder) ? vs.w + sl[j] : f;
  double acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = 0.0;

  const int64_t ntile = vs.n / (kBlock * VEC);
  // (dead ring slots -- a launch wider than the list -- re-read f at the tile at hand here.  Sending them to f's first
  //  tile, as PB does (k_combine_win), was measured in this pass too: 25 more VGPRs for the per-slot offsets and
  //  +2...5 % of PA with NO dead slot, which is every launch of a caller that synchronises once per iteration, since PA
  //  then runs at exactly the list length; profiles/r04/ab_dead_slot.txt.  The ONE slot of a skipped last vector does go
  //  there -- `last_far` above: a scalar choice, no register per slot)
#define DEAD_OFF(j, off, off_far) ((j) == MAXL - 1 ? (off_far) : (off))
  V fv, w1v, omv = {}, ring[W];      // (omv: WGT only)
  int64_t t = blockIdx.x;
  if (t < ntile) {
    const int64_t e = t * (kBlock * VEC) + threadIdx.x * VEC;
    const int64_t ef = (last_far ? 0 : t) * (kBlock * VEC) + threadIdx.x * VEC;
    fv = ld<VEC>(f + e);
    w1v = ld<VEC>(w1 + e);
    if constexpr (WGT) omv = ld<VEC>(wgt + e);
#pragma unroll
    for (int j = 0; j < W; j++) ring[j] = ld<VEC>(wk[j] + (DEAD_OFF(j, e, ef)));
  }
  NKA_STAMP0(ctl, 11);
  for (; t < ntile; t += G) {
    const int64_t e = t * (kBlock * VEC) + threadIdx.x * VEC;
    const int64_t tn = (t + G < ntile) ? t + G : t;     // the last iteration prefetches its own tile again
    const int64_t en = tn * (kBlock * VEC) + threadIdx.x * VEC;
    const int64_t ef = (last_far ? 0 : t) * (kBlock * VEC) + threadIdx.x * VEC;        // (the skipped last slot: DEAD_OFF)
    const int64_t enf = (last_far ? 0 : tn) * (kBlock * VEC) + threadIdx.x * VEC;
    double dq[VEC], fq[VEC];      // (weighted: the first operands fl(w d), fl(w f); the second ones are not kept)
#pragma unroll
    for (int q = 0; q < VEC; q++) {
      const double fx = ex(fv, q);
      const double dx = pa_operand(ex(w1v, q) - fx, normed, s_n, rs_n);      // F08:266 (and F08:283 when the norm is known)
      dq[q] = wgt_first<WGT>(omv, q, dx);
      fq[q] = wgt_first<WGT>(omv, q, fx);
      acc[0] = fma(dq[q], dx, acc[0]);
      acc[1] = fma(fq[q], dx, acc[1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    fv = ld<VEC>(f + en);
    w1v = ld<VEC>(w1 + en);
    if constexpr (WGT) omv = ld<VEC>(wgt + en);
#pragma unroll
    for (int j = 0; j < MAXL; j++) {
      const V x = ring[j % W];
      __builtin_amdgcn_sched_barrier(0);
      if (j + W < MAXL) ring[j % W] = ld<VEC>(wk[j + W] + (DEAD_OFF(j + W, e, ef)));
      else ring[j % W] = ld<VEC>(wk[j + W - MAXL] + (DEAD_OFF(j + W - MAXL, en, enf)));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < VEC; q++) {
        acc[2 + j] = fma(dq[q], ex(x, q), acc[2 + j]);
        acc[2 + MAXL + j] = fma(fq[q], ex(x, q), acc[2 + MAXL + j]);
      }
    }
  }
  if ((int)blockIdx.x == G - 1) {  // ragged tail, scalar
    for (int64_t i = ntile * (kBlock * VEC) + threadIdx.x; i < vs.n; i += kBlock) {
      const double fx = f[i];
      const double d = pa_operand(w1[i] - fx, normed, s_n, rs_n);
      const double dw = wgt_at<WGT>(wgt, i, d), fw = wgt_at<WGT>(wgt, i, fx);
      acc[0] = fma(dw, d, acc[0]);
      acc[1] = fma(fw, d, acc[1]);
#pragma unroll
      for (int j = 0; j < MAXL; j++) {
        const double x = wk[j][i];
        acc[2 + j] = fma(dw, x, acc[2 + j]);
        acc[2 + MAXL + j] = fma(fw, x, acc[2 + MAXL + j]);
      }
    }
  }
  NKA_STAMP0(ctl, 12);
  block_reduce_store<NACC>(acc, partials, G);
  NKA_STAMP0(ctl, 13);
#undef DEAD_OFF
}

// Set-time check of a weight vector (nka_hip_set_dot_weights): out[0] += entries that are not finite or below zero,
// out[1] = min over their indices (starts at ~0).  Grid-stride; runs once per set, not in an update.
__global__ __launch_bounds__(kBlock) void k_check_weights(const double *__restrict__ w, int64_t n,
                                                          unsigned long long *out) {
  unsigned long long bad = 0, first = ~0ull;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double x = w[i];
    if (!(x >= 0.0 && x <= __DBL_MAX__)) {      // NaN, -Inf, +Inf, negative (-0.0 is >= 0)
      bad++;
      if ((unsigned long long)i < first) first = (unsigned long long)i;
    }
  }
  if (bad) {
    atomicAdd(out, bad);
    atomicMin(out + 1, first);
  }
}

// Final sums of one PA pass scattered into red[] (layout above).  One wavefront
// per column (grid = 2*MAXL+2 blocks of 64): each lane sums its strided share in
// order, then a butterfly -- the same bits on every run.
constexpr int kFinThreads = 64;
// `ncover` = entries of each row that the passes of this update write (npass*MAXL):
// pass 0 zeroes the rest, so red[] never carries stale sums into the all-reduce.
// `x.base` != nullptr: the sums do not stay here -- each one goes to row `me` of every rank's mailbox (P2P above) and the
// scalar step gathers them; red[] is then written by that gather.
template <int MAXL>
__global__ __launch_bounds__(kFinThreads) void k_finalize_dots(Ctl ctl, const double *__restrict__ partials, int G,
                                                               int pass, int ncover, int base, P2P x, int keep0 = 0,
                                                               int skip = 0) {
  if (skip_repair_idle(ctl, skip)) return;
  const int lane = threadIdx.x;
  const int c = blockIdx.x;
  const bool p2p = x.base != nullptr;
  const unsigned long long xs = p2p ? *x.xseq : 0ull;
  // the column's partial sums are requested BEFORE the plan is known (whether the column is live only decides
  // if its sum or a zero is stored): the two memory round trips overlap instead of following one another
  double r = 0.0;
  for (int b = lane; b < G; b += kFinThreads) r += partials[(size_t)c * G + b];
  r = wave_sum(r);
  const int pending = ctl.ic[IC_PLAN_PENDING];
  // (a skipped last vector, k_dots_win: its column is dead like the columns past the list, both rows read 0)
  const int nplan = ctl.ic[IC_PLAN_NOLDER];
  const int nolder = nplan - (skip_last_planned(ctl, skip, pending, nplan) ? 1 : 0);
  // (`base` = first plan entry of this pass: pass * MAXL for the passes of equal width, the running sum of the widths
  //  for the balanced passes of the window kernels)
  if (pass == 0 && c == 0)
    for (int p = ncover + lane; p < ctl.mvec; p += kFinThreads) {
      if (p2p) {
        for (int q = 0; q < x.n; q++) {
          p2p_send_one(x, q, xs, 2 + p, 0.0);
          p2p_send_one(x, q, xs, 2 + ctl.mvec + p, 0.0);
        }
      } else {
        ctl.red()[2 + p] = 0.0;
        ctl.red()[2 + ctl.mvec + p] = 0.0;
      }
    }
  int dst = -1;
  bool live = false;
  if (c < 2) {
    if (pass == 0 && !(keep0 && c == 0)) { dst = c; live = pending != 0; }      // (keep0: red[0] holds the norm of a pass of its own)
  } else if (c < 2 + MAXL) {
    const int p = base + (c - 2);
    if (p < ctl.mvec) { dst = 2 + p; live = pending && p < nolder; }
  } else {
    const int p = base + (c - 2 - MAXL);
    if (p < ctl.mvec) { dst = 2 + ctl.mvec + p; live = p < nolder; }
  }
  if (dst < 0) return;
  if (p2p) {
    p2p_send_wave(x, xs, dst, live ? readlane_f64(r, 0) : 0.0);
    return;
  }
  if (lane == 0) ctl.red()[dst] = live ? r : 0.0;
}

// ---- PA in the REFERENCE'S ORDER: every sum of the update as the reference forms it ---------------
// One workgroup.  The reference's inner products are sequential sums of rounded products (its default dot product:
// C .c:200-208; `dot_product(x, y)` in F08:216-219, compiled without contraction as oracle/Makefile does), the norm first
// (F08:267), then -- with w1' = d/s (F08:283; (1/s)*d in the vector flavour, F08V:256) already ROUNDED -- the Gram row
// <w1',w_k> (F08:286-290) and the projections <f,w_k>, <f,w1'> (F08:371).  This kernel forms exactly those: element after
// element, one rounding per product and per addition (no fma).  A chunk of f, of the normalised w1' and of every older w is
// staged in LDS by the whole workgroup (coalesced); then thread r walks the chunk for sum r, so that the only serial
// thing per element is the addition itself.  Rows are `chunk + 1` apart (the lanes of a wavefront read different rows at
// the same element: an odd stride spreads them over the banks).  red[] then holds  [0] sum d^2, [1] <f,w1'>,
// [2+p] <w1',w_p>, [2+mvec+p] <f,w_p>  -- the scalar step takes [1] and the Gram row as they are (kSolvePrenorm) -- and,
// the scalar step and PB's statements being bit-exact given their inputs, the update returns THE REFERENCE'S BITS.
// Cost: two chains of n dependent additions (the norm, then the sums on w1'), 20-30 ns per element on an otherwise idle
// MI355X (tools/sum_order_cost.py, profiles/r04/sum_order_cost.txt): on par with the blocked PA and its final sums up to
// n = 64 (the default there), +12-18 us per update at n = 512, 40 ms per update at n = 1e6.  Single rank only: the Gram row needs the GLOBAL norm
// first, i.e. a second exchange (nka_hip_set_sum_order).
// SHARDED (round 5): the reference's sum over the GLOBAL vector is one chain of additions through the slices in rank
// order, so rank r CONTINUES the running sums of rank r-1: `carry` != 0 starts every accumulator from the value red[]
// holds (the prefix over the ranks before this one) instead of 0, and the update is made in two kinds of rounds (nka_hip.hip,
// ordered_chain): phase 1 = the norm only (red[0]); phase 2 = with s from the GLOBAL red[0], the sums on the rounded w1'
// and on f (red[1..]).  phase 0 = both in one launch, the single-rank form described above.
enum { kOrdAll = 0, kOrdNorm = 1, kOrdRows = 2 };
__global__ __launch_bounds__(kOrdThreads) void k_dots_ordered(Ctl ctl, Vecs vs, const double *__restrict__ f, int rcp,
                                                              int chunk, int phase, int carry) {
  extern __shared__ double ord_sh[];
  __shared__ double sum_dd;
  const int t = threadIdx.x;
  const int pending = ctl.ic[IC_PLAN_PENDING];
  const int nolder = ctl.ic[IC_PLAN_NOLDER];
  const int mvec = ctl.mvec;
  const int64_t n = vs.n;
  const int S = chunk + 1;                           // row stride in LDS
  const double *w1 = pending ? vs.w + ctl.pc[PC_FIRST_W] : f;
  const long long *pw = ctl.plan_w();
  double *red = ctl.red();
  double *row_f = ord_sh, *row_w1 = ord_sh + S;      // rows 2.. : the older w's
  const bool single = n <= chunk && phase == kOrdAll;   // the whole vectors fit: every global load of the update is issued ONCE

  // The sums on the ROUNDED w1' wait for the norm, those on f alone do not: they live in DIFFERENT wavefronts, so that the
  // second kind is summed while thread 0 sums the norm.  Threads 0..127 own the w1' sums  r = t, t + 128  (r = 0: <f,w1'>;
  // 1 <= r <= nolder: <w1',w_(r-1)>), threads 128..255 the sums on f  p = t - 128, t  (<f,w_p>, p < nolder).
  double acc[2] = {0.0, 0.0};
  const double *xr[2] = {row_f, row_f}, *yr[2] = {row_f, row_f};
  int dst[2] = {-1, -1};                             // where the sum goes in red[]
  const bool on_w1 = t < kOrdThreads / 2;
  for (int q = 0; q < 2; q++) {
    if (on_w1) {
      const int r = t + q * (kOrdThreads / 2);
      if (r > nolder) continue;
      if (r == 0) { xr[q] = row_f; yr[q] = row_w1; dst[q] = 1; }
      else { xr[q] = row_w1; yr[q] = ord_sh + (size_t)(2 + (r - 1)) * S; dst[q] = 2 + (r - 1); }
    } else {
      const int p = (t - kOrdThreads / 2) + q * (kOrdThreads / 2);
      if (p >= nolder) continue;
      xr[q] = row_f; yr[q] = ord_sh + (size_t)(2 + p) * S; dst[q] = 2 + mvec + p;
    }
  }

  if (carry)
    for (int q = 0; q < 2; q++)
      if (dst[q] >= 0) acc[q] = red[dst[q]];           // the running sums of the ranks before this one
  // ---- first pass: the norm (F08:266-267); with everything resident also the sums on f alone, on the other threads ----
  double s = 0.0;
  if (phase == kOrdRows) {
    if (pending) s = sqrt(red[0]);                     // the GLOBAL sum d^2 of the norm rounds
    if (t == 0) sum_dd = red[0];
    __syncthreads();
  } else {
    double dd = (carry && t == 0) ? red[0] : 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
      const int len = (int)(n - c0 < chunk ? n - c0 : chunk);
      if (!pending && !single) break;
      for (int i = t; i < len; i += kOrdThreads) {
        const double fi = f[c0 + i];
        row_f[i] = fi;
        row_w1[i] = w1[c0 + i] - fi;                 // d (F08:266; (-1)*f + w1 in F08V:237: same bits)
      }
      if (single) ord_load_older(ord_sh, S, vs, pw, nolder, c0, len);
      __syncthreads();
      if (t == 0 && pending) dd = ord_sum(dd, row_w1, row_w1, len);
      if (single && !on_w1)
        for (int q = 0; q < 2; q++)
          if (dst[q] >= 0) acc[q] = ord_sum(acc[q], xr[q], yr[q], len);
      if (!single) __syncthreads();
    }
    if (t == 0) sum_dd = dd;
    __syncthreads();
    if (pending) s = sqrt(sum_dd);
    if (phase == kOrdNorm) {                           // a norm round of a sharded update: red[0] and nothing else
      if (t == 0 && pending) red[0] = sum_dd;
      return;
    }
  }
  const bool normed = pending && s != 0.0;           // (s == 0: the scalar step relaxes, F08:268-275; the w1' sums are dead)
  const double rs = 1.0 / s;

  // ---- second pass: the sums on the ROUNDED w1' (and, if the vectors did not fit, those on f alone) ----
  if (single) {
    if (normed) {
      for (int i = t; i < (int)n; i += kOrdThreads) row_w1[i] = rcp ? rs * row_w1[i] : row_w1[i] / s;   // the value PB stores as w1'
      __syncthreads();
      if (on_w1)
        for (int q = 0; q < 2; q++)
          if (dst[q] >= 0) acc[q] = ord_sum(acc[q], xr[q], yr[q], (int)n);
    }
  } else {
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
      const int len = (int)(n - c0 < chunk ? n - c0 : chunk);
      for (int i = t; i < len; i += kOrdThreads) {
        const double fi = f[c0 + i];
        row_f[i] = fi;
        if (normed) {
          const double d = w1[c0 + i] - fi;
          row_w1[i] = rcp ? rs * d : d / s;          // the value PB stores as w1'
        }
      }
      ord_load_older(ord_sh, S, vs, pw, nolder, c0, len);
      __syncthreads();
      if (normed || !on_w1)
        for (int q = 0; q < 2; q++)
          if (dst[q] >= 0) acc[q] = ord_sum(acc[q], xr[q], yr[q], len);
      __syncthreads();
    }
  }
  // red[]: zero what this update does not cover (nothing stale reaches a later reader), then the sums
  __syncthreads();
  if (!carry) {                                        // (a continuing rank keeps the prefix of the sums it does not own: zeros)
    for (int i = t + (phase == kOrdRows ? 1 : 0); i < 2 + 2 * mvec; i += kOrdThreads) red[i] = 0.0;
  }
  __syncthreads();
  if (t == 0 && pending && phase == kOrdAll) red[0] = sum_dd;
  for (int q = 0; q < 2; q++)
    if (dst[q] >= 0 && (normed || !on_w1)) red[dst[q]] = acc[q];
}

// ---- The same sums, ONE WORKGROUP PER SUM (long vectors): the chain of nka_chain.hpp ----
__global__ __launch_bounds__(kChainThreads) void k_chain_sums(Ctl ctl, Vecs vs, const double *__restrict__ f, int rcp,
                                                              int set, int with_f, int ub, int walk, const double *probe) {
  extern __shared__ __attribute__((aligned(16))) double prod[];   // kChainLdsBytes
  __shared__ ChainSummary summ[kChainGroupBlocks];
  __shared__ double sh_a;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const ChainSum cs = chain_decode(ctl, vs, f, rcp, set, with_f, ub, blockIdx.x, probe);
  if (cs.kind < 0) return;
  // wavefront w loads, multiplies and summarises block w of a group (elements [1024 w, 1024 w + 1024))
  ChainBlockRegs regs;
  double *myblk = prod + wave * kChainBlockLds;
  auto load = [&](int64_t g0) { chain_load_block(cs, regs, g0 + wave * kChainBlock, lane, g0 + kChainGroup <= cs.n); };
  auto store = [&]() { chain_store_block(cs, regs, myblk, lane); };
  double *red = ctl.red();
  ChainStamps stamps;
  const double a = chain_drive(red[cs.dst], cs.n, prod, summ, &sh_a, walk, stamps, load, store);
  if (t == 0) red[cs.dst] = a;
#ifdef NKA_CHAIN_STAMPS
  if (t == 0 && set == kChainProbe)
    for (int i = 0; i < 8; i++) { ctl.stamps()[i] = (double)stamps.st[i]; ctl.stamps()[8 + i] = (double)stamps.cnt[i]; }
  // (10 ns ticks: load issue, summary, wait, apply, wait, store; then the block counts)
#endif
}

// ---- The same sums, MANY compute units per sum (round 5, the longest vectors) ------------------------------------
// k_chain_sums gives a sum one compute unit: its blocks are summarised eight at a time and the summaries applied in
// between.  But a block's summary needs only the SIGN AND EXPONENT of the running sum at its start -- and those follow from
// an ordinary blocked prefix sum (off by rounding noise, i.e. wrong only when the sum is within ~1e-13 of a power of two,
// which the apply step notices).  So the summaries of ALL blocks of ALL sums are made by the whole device:
//   k_chain_blocks(mode 0)   one wavefront per (block, sum): the block's products, summed any way -> pred[sum][block]
//   k_chain_predict          per sum: exclusive prefix of those, from red[dst] -> the predicted running sum at each block
//   k_chain_blocks(mode 1)   one wavefront per (block, sum): the summary under the predicted sign and exponent
//   k_chain_apply            per sum, ONE wavefront: 64 summaries at a time -- one scalar parity chain, one prefix sum, each
//                            block checked against the sum it would start from, the longest run of acceptable blocks goes
//                            in at once; a block that does not is loaded, summarised again if the exponent was
//                            mispredicted, else walked (chain_block_serial), and the run goes on behind it.
// Same functions, same acceptance rule, same bits as k_chain_sums; what remains sequential is ~10 ns per accepted block and
// the walk of the blocks that meet an end of their binade.
__global__ __launch_bounds__(kChainThreads) void k_chain_blocks(Ctl ctl, Vecs vs, const double *__restrict__ f, int rcp,
                                                                int set, int with_f, int ub, int nsum, long long nfull,
                                                                double *__restrict__ pred, ChainSummary *__restrict__ summ,
                                                                int mode, const double *probe) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double prod[];   // kChainLdsBytes: one block per wavefront
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const long long item = (long long)blockIdx.x * kChainWaves + wave;      // (no barrier in this kernel: wavefronts are on their own)
  if (item >= nfull * nsum) return;
  const int b = (int)(item % nsum);                                        // the sums of one block side by side: f and w1 come from L2
  const long long blk = item / nsum;
  const ChainSum cs = chain_decode(ctl, vs, f, rcp, set, with_f, ub, b, probe);
  if (cs.kind < 0) return;
  ChainBlockRegs regs;
  double *myblk = prod + wave * kChainBlockLds;
  chain_load_block(cs, regs, blk * kChainBlock, lane, true);
  chain_store_block(cs, regs, myblk, lane);
  if (mode == 0) {
    double pl[kChainLaneElems];
    chain_lane_read(pl, myblk, lane);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kChainLaneElems; j++) acc = acc + pl[j];
    const double tot = wave_scan_add_f64(acc);
    if (lane == 63) pred[(long long)b * nfull + blk] = tot;
  } else {
    const ChainSummary sm = chain_block_summary(pred[(long long)b * nfull + blk], myblk);
    if (lane == 0) summ[(long long)b * nfull + blk] = sm;
  }
}

constexpr int kChainPredictThreads = 256;
__global__ __launch_bounds__(kChainPredictThreads) void k_chain_predict(Ctl ctl, Vecs vs, const double *f, int rcp, int set,
                                                                        int with_f, int ub, long long nfull,
                                                                        double *__restrict__ pred, const double *probe) {
  __shared__ double seg_sum[kChainPredictThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  const ChainSum cs = chain_decode(ctl, vs, f, rcp, set, with_f, ub, b, probe);
  if (cs.kind < 0) return;
  double *p = pred + (long long)b * nfull;
  const long long seg = (nfull + kChainPredictThreads - 1) / kChainPredictThreads;
  const long long lo = t * seg, hi = lo + seg < nfull ? lo + seg : nfull;
  double acc = 0.0;
  for (long long i = lo; i < hi; i++) acc += p[i];
  seg_sum[t] = acc;
  __syncthreads();
  if (t == 0) {
    double run = ctl.red()[cs.dst];                    // the sum the chain starts from
    for (int i = 0; i < kChainPredictThreads; i++) { const double v = seg_sum[i]; seg_sum[i] = run; run += v; }
  }
  __syncthreads();
  double run = seg_sum[t];
  for (long long i = lo; i < hi; i++) { const double v = p[i]; p[i] = run; run += v; }
}

__global__ __launch_bounds__(64) void k_chain_apply(Ctl ctl, Vecs vs, const double *__restrict__ f, int rcp, int set,
                                                    int with_f, int ub, long long nfull,
                                                    const ChainSummary *__restrict__ summ, int walk, const double *probe) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double blk_lds[kChainBlockLds];
  const int lane = threadIdx.x, b = blockIdx.x;
  const ChainSum cs = chain_decode(ctl, vs, f, rcp, set, with_f, ub, b, probe);
  if (cs.kind < 0) return;
  double *red = ctl.red();
  double a = red[cs.dst];
  ChainRun run;
  chain_run_enter(run, a);
  ChainBlockRegs regs, ahead;                          // the operands of the block in hand; of the block behind it (see below)
  long long ahead_of = -1;                             // which block `ahead` holds
  const ChainSummary *mysum = summ + (long long)b * nfull;
  ChainSummary none;
  none.hi = 0; none.total = 0.0; none.gmin = none.gmax = 0.f; none.adj = 0;
#ifdef NKA_CHAIN_STAMPS
  unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tw = 0, t0_;   // blocks: in runs / singly / summarised again / walked
#define NKA_APPLY_COUNT(i, v) cnt[i] += (v);
#else
#define NKA_APPLY_COUNT(i, v)
#endif
  ChainSummary next = (lane < nfull && !walk) ? mysum[lane] : none;       // (the summaries of the batch after this one are in
  for (long long k0 = 0; k0 < nfull; k0 += 64) {                          //  flight while this one is applied)
    const int nb = (int)(nfull - k0 < 64 ? nfull - k0 : 64);
    const ChainSummary mine = next;
    next = (k0 + 64 + lane < nfull && !walk) ? mysum[k0 + 64 + lane] : none;
    int k = 0;
    bool try_run = true;                               // (right behind a block that did not go in, its successor is tried alone first)
    while (k < nb) {
      if (run.hi != 0 && !walk && !try_run) {
        ChainSummary one;
        one.total = readlane_f64(mine.total, k);
        one.gmin = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.gmin), k));
        one.gmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.gmax), k));
        one.adj = __builtin_amdgcn_readlane(mine.adj, k);
        one.hi = __builtin_amdgcn_readlane(mine.hi, k);
        if (chain_block_apply(run, one)) { k++; try_run = true; NKA_APPLY_COUNT(1, 1) continue; }
      }
      if (run.hi != 0 && !walk && try_run) {
        const bool cand = lane >= k && lane < nb;
        const int ae = (mine.adj & 0xffff) - kChainAdjBias, ao = ((mine.adj >> 16) & 0xffff) - kChainAdjBias;
        const bool usable = cand && mine.hi == run.hi;
        // the parity each block starts from, if every block before it goes in (a scalar chain over two ballot masks)
        const int tpar = __double2loint(fabs(mine.total) + 0x1p52) & 1;     // (|total| < 2^52 in any block that goes in)
        const unsigned long long pe = __ballot(usable && ((tpar ^ ae) & 1)), po = __ballot(usable && ((tpar ^ ao) & 1));
        unsigned long long odd = 0;
        if (pe == po) {                                // (no block's flip depends on the parity it meets: a prefix XOR)
          unsigned long long x = pe;
          x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
          odd = ((__builtin_amdgcn_readfirstlane(__double2loint(run.S)) & 1) ? ~0ull : 0ull) ^ (x << 1);
        } else {
          unsigned long long p = (unsigned long long)(__builtin_amdgcn_readfirstlane(__double2loint(run.S)) & 1);
          for (int i = k; i < nb; i++) {
            odd |= p << i;
            p ^= ((p ? po : pe) >> i) & 1ull;
          }
        }
        const double tk_ = usable ? mine.total + (double)(((odd >> lane) & 1ull) ? ao : ae) : 0.0;
        const double incl = wave_scan_add_f64(tk_);
        const double Sk = run.S + (incl - tk_);
        constexpr double kEdge = 0x1p34;
        const bool ok = usable && (Sk + (double)mine.gmin >= 0x1p52 + kEdge) && (Sk + (double)mine.gmax <= 0x1p53 - kEdge);
        const unsigned long long need = (nb == 64 ? ~0ull : (1ull << nb) - 1ull) & ~((1ull << k) - 1ull);
        const unsigned long long failm = need & ~__ballot(ok);
        const int F = failm ? __ffsll((long long)failm) - 1 : nb;
        if (F > k) {
          run.S = run.S + readlane_f64(incl, F - 1);
          NKA_APPLY_COUNT(0, F - k)
          k = F;
          continue;
        }
      }
      // block k0 + k on its own: its products into LDS; summarised under the sum's present exponent if the prediction
      // missed it, else (or failing that) walked.  A sum that meets an end of its binade stays there for a while: the
      // operands of the NEXT block are requested before this one is walked, so that its walk, if it comes to that, finds them.
      const long long kb = k0 + k;
      if (ahead_of == kb) regs = ahead;
      else chain_load_block(cs, regs, kb * kChainBlock, lane, true);
      if (kb + 1 < nfull) { chain_load_block(cs, ahead, (kb + 1) * kChainBlock, lane, true); ahead_of = kb + 1; }
      chain_store_block(cs, regs, blk_lds, lane);
      bool done = false;
      const int hi_k = __builtin_amdgcn_readlane(mine.hi, k);
      if (!walk && run.hi != 0 && run.hi != hi_k) {
        const ChainSummary sm = chain_block_summary(run.S * run.unscale, blk_lds);
        done = chain_block_apply(run, sm);
        if (done) { NKA_APPLY_COUNT(2, 1) }
      }
      if (!done) {
        NKA_APPLY_COUNT(3, 1)
#ifdef NKA_CHAIN_STAMPS
        t0_ = wall_clock64();
#endif
        if (run.hi != 0) a = run.S * run.unscale;
        a = chain_block_serial(a, blk_lds, kChainBlock);
        chain_run_enter(run, a);
#ifdef NKA_CHAIN_STAMPS
        tw += wall_clock64() - t0_;
#endif
      }
      k++;
      try_run = false;
    }
  }
  if (run.hi != 0) a = run.S * run.unscale;
  const long long e0 = nfull * kChainBlock;
  if (e0 < cs.n) {                                     // the last, partial block
    chain_load_block(cs, regs, e0, lane, false);
    chain_store_block(cs, regs, blk_lds, lane);
    a = chain_block_serial(a, blk_lds, (int)(cs.n - e0));
  }
  if (lane == 0) red[cs.dst] = a;
#ifdef NKA_CHAIN_STAMPS
  if (lane == 0 && set == kChainProbe) {
    for (int i = 0; i < 8; i++) ctl.stamps()[8 + i] = (double)cnt[i];
    ctl.stamps()[3] = (double)tw;                       // (10 ns ticks spent walking)
  }
#endif
#undef NKA_APPLY_COUNT
}

// ---- PB: normalise the pending pair, combine, and all five stores -----------------
// COMB 0: x/s          ; (f - c*w) + c*v       F08:282-283, 397
// COMB 1: (1/s)*x      ; ((-c)*w + c*v) + f    F08V:255-256 scale(1/s), :374 update3_
//                                              (grid_vector_type.F90:117,151)
// COMB 2: x/s          ; f + c*(v - w)         C .c:317-320, 423
// The k loop runs in list order with the reference's association, so given the
// same coefficients the result is bit-identical to the reference's k passes.
//
// COMPACT storage (COMB 2 only).  The C reference combines with the DIFFERENCE
// v_k - w_k (f += c*(v - w), .c:423).  For a normalised pair that difference
// never changes, so this flavour stores u_k = fl(v_k' - w_k') in the v array
// when the pair is normalised and reads ONE vector per pair ever after:
// f + c*u_k is bit-identical to the C statement, and PB reads k+2 vectors
// instead of 2k+1.  (The pending slot still holds the raw w = f_in, v = f_out.)
//
// MAXK (slot, coefficient) pairs per pass, fully unrolled: offsets and
// coefficients sit in SGPRs and all loads of a tile are issued together.  Pairs
// beyond the actual count re-read f and are not applied.  Pass 0 stores
// w_new = f_in and, if this update normalises (IC_NORMED), treats pair 0 -- the
// pending slot, still holding the raw previous f and update -- as
// w1' = (w1-f)/s, v1' = v1/s formed in registers and stored back.  The last pass
// stores v_new = f_out.
enum { kPbNoStoreW = 1, kPbNoStoreF = 2,     // `flags` of PB in an out-of-place update (nka_hip_accel_update_swap)
       kPbNotFirst = 8, kPbNotLast = 16,      // rolling-window PB over a list longer than kMaxPerPass: not the first / not the
                                              // last of its passes (enqueue_pb; in place only)
       kPbMayDefer = 32 };                    // k_combine_win<.., DEFER = true> may leave v_new unstored (see there)

template <int MAXK, int VEC, int COMB>
__global__ __launch_bounds__(kBlock) void k_combine(Ctl ctl, Vecs vs, double *f, int pass, int last_pass, int flags) {
  using V = typename VecT<VEC>::type;
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  constexpr int NW = COMPACT ? 1 : MAXK;   // w vectors loaded per tile
  const int G = gridDim.x;
  const int ncomb = ctl.ic[IC_NCOMB];
  double *wnew = vs.w + ctl.pc[PC_NEW_W], *vnew = vs.w + ctl.pc[PC_NEW_V];
  const long long *cw = ctl.comb_w(), *cv = ctl.comb_v();
  const double *cc = ctl.comb_c();
  const int base = pass * MAXK;
  // Out-of-place update (kPbNoStoreW / kPbNoStoreF): the caller's buffer f IS w_new and must keep f_in, and f_out goes
  // to v_new only -- so between the passes of a long list the running value lives in v_new, never in f.
  const bool oop = (flags & kPbNoStoreF) != 0;
  const double *src = (oop && pass > 0) ? vnew : f;
  const bool store_w = (pass == 0) && !(flags & kPbNoStoreW), store_v = (last_pass != 0) || oop;
  const bool store_f = !oop && (last_pass != 0 ? (ncomb > 0) : true);  // nothing to combine: f stays as it is
  const bool norm0 = (pass == 0) && ctl.ic[IC_NORMED];
  const double s = ctl.dc[DC_S];
  const double rs = 1.0 / s;
  if (pass == 0) list_word_publish(ctl, ncomb, flags & kPbNoStoreW);

  double *wk[MAXK], *vk[MAXK];
  double ck[MAXK];
#pragma unroll
  for (int j = 0; j < MAXK; j++) {
    const int k = base + j;
    const bool live = k < ncomb;
    wk[j] = live ? vs.w + cw[k] : f;
    vk[j] = live ? vs.w + cv[k] : f;
    ck[j] = cc[k];
  }

  const int64_t ntile = vs.n / (kBlock * VEC);
  for (int64_t t = blockIdx.x; t < ntile; t += G) {
    const int64_t e = t * (kBlock * VEC) + threadIdx.x * VEC;
    const V fin = ld<VEC>(src + e);
    V wv[NW], vv[MAXK];
    if (!COMPACT || norm0) wv[0] = ld<VEC>(wk[0] + e); else wv[0] = fin;
#pragma unroll
    for (int j = 1; j < NW; j++) wv[j] = ld<VEC>(wk[j] + e);
#pragma unroll
    for (int j = 0; j < MAXK; j++) vv[j] = ld<VEC>(vk[j] + e);
    __builtin_amdgcn_sched_barrier(0);  // every load of the tile in flight before any arithmetic
    if (norm0) {
#pragma unroll
      for (int q = 0; q < VEC; q++) {
        const double d = ex(wv[0], q) - ex(fin, q);
        const double wn = RCP ? rs * d : d / s;
        const double vn = RCP ? rs * ex(vv[0], q) : ex(vv[0], q) / s;
        setc(wv[0], q, wn);
        setc(vv[0], q, COMPACT ? vn - wn : vn);
      }
      st(wk[0] + e, wv[0]);
      st(vk[0] + e, vv[0]);
    }
    V x = fin;
#pragma unroll
    for (int j = 0; j < MAXK; j++) {
      if (base + j < ncomb) {
#pragma unroll
        for (int q = 0; q < VEC; q++) {
          if (COMPACT) setc(x, q, ex(x, q) + ck[j] * ex(vv[j], q));
          else setc(x, q, comb1<COMB>(ex(x, q), ck[j], ex(wv[j < NW ? j : 0], q), ex(vv[j], q)));
        }
      }
    }
    if (store_w) st(wnew + e, fin);
    if (store_v) st(vnew + e, x);
    if (store_f) st(f + e, x);
  }
  if ((int)blockIdx.x == G - 1) {  // ragged tail, scalar
    for (int64_t i = ntile * (kBlock * VEC) + threadIdx.x; i < vs.n; i += kBlock) {
      const double fin = src[i];
      double x = fin;
#pragma unroll
      for (int j = 0; j < MAXK; j++) {
        if (base + j < ncomb) {
          double v = vk[j][i];
          double w = (!COMPACT || (j == 0 && norm0)) ? wk[j][i] : 0.0;
          if (j == 0 && norm0) {
            const double d = w - fin;
            w = RCP ? rs * d : d / s;
            v = RCP ? rs * v : v / s;
            if (COMPACT) v = v - w;
            wk[0][i] = w;
            vk[0][i] = v;
          }
          x = COMPACT ? x + ck[j] * v : comb1<COMB>(x, ck[j], w, v);
        }
      }
      if (store_w) wnew[i] = fin;
      if (store_v) vnew[i] = x;
      if (store_f) f[i] = x;
    }
  }
}

// ---- PB with a SMALL ROLLING WINDOW of loads ---------------------------------------
// tools/hbm_probe (mode m): a kernel reading 22 streams and writing 5 moves 5.5 TB/s with
// every load of a tile in flight, 5.7 software-pipelined, 5.9 when each wave keeps only a
// ring of FOUR loads in flight and re-issues a slot the moment it has been consumed
// (pure reads: 7.25 against 7.0 TB/s) -- fewer streams are open in the DRAMs at any
// moment, and the load issue never stops for the arithmetic or the stores.  Here the MAXK
// pairs of a tile go through a ring of W (pair j in slot j mod W; a consumed slot is
// re-loaded with pair j+W of this tile or pair j+W-MAXK of the block's next tile); f
// and, with compact storage, the raw w of the pending pair are requested one tile ahead.
// Same arithmetic in the same order => same bits as k_combine.  Single pass, VEC = 2.
//
// PASSES (round 5).  A list longer than kMaxPerPass pairs is combined by several launches of balanced exact widths, each on
// the pairs [base, base + MAXK) of the plan, f carrying the running value in between (the k loop of F08:395-399 cut into
// consecutive pieces: same statements in the same order, same bits).  The FIRST pass (no kPbNotFirst) normalises the pending
// pair -- pair 0 of the plan -- and stores w_new = f_in; the LAST (no kPbNotLast) stores v_new = f_out; every pass stores f.
//
// DEFERRED v OF THE PENDING PAIR (DEFER = true: compact storage, in place, one pass; chosen by the host, update_impl).  PB stores
// the accelerated f twice, into the caller's f and into v_new, and v_new is read exactly once: by the next PB, to form
// u1' = fl(v1/s) - w1'.  With kPbMayDefer in `flags` and a plan to combine, this instantiation leaves v_new UNSTORED and raises
// PC_VDEFER.  The next update's scalar step then hands its PB -- this instantiation again, the host sees to that -- a replay
// plan (Ctl::rp_v ...): the vectors and coefficients the missing v was combined from,
//     v1 = w1 + c_prev,0 u_0 + c_prev,1 u_1 + ...     (w1 raw = the f_in of that update; list order; separate mul and add:
//                                                      the statements that formed f_out, hence its bits)
// and combine_win_replay below forms it while it streams the u_j -- the same vectors this update combines, plus those it has
// just dropped, read in place of v1: one store less, no load more.  Everything that reads the slot otherwise first runs
// k_materialise_v (host: ensure_v).  The other instantiations contain nothing of this.
template <int MAXK, int W, int T>
__device__ __forceinline__ void combine_win_replay(const Ctl &ctl, const Vecs &vs, double *f, unsigned *tickets, int ng, int flags,
                                                   int np, unsigned *s_next) {
  constexpr int VEC = 2;
  using V = typename VecT<VEC>::type;
  constexpr int TILE = kBlock * VEC * T;
  const int64_t ntile = vs.n / TILE;
  const bool has_tail = ntile * TILE < vs.n;
  const int G = (int)gridDim.x - (has_tail ? 1 : 0);
  const bool tail_block = has_tail && (int)blockIdx.x == G;
  const int ncomb = ctl.ic[IC_NCOMB];                      // >= 1: entry 0 is the pending pair, normalised now
  double *wnew = vs.w + ctl.pc[PC_NEW_W], *vnew = vs.w + ctl.pc[PC_NEW_V];
  double *w1 = vs.w + ctl.comb_w()[0], *u1 = vs.w + ctl.comb_v()[0];
  const double c0 = ctl.comb_c()[0];
  const unsigned keep = (unsigned)ctl.rp_keep()[0];        // bit j: entry j of the replay plan is combined into f as well
  const bool store_w = !(flags & kPbNoStoreW), store_f = !(flags & kPbNoStoreF);
  const bool store_v = !((flags & kPbMayDefer) && ncomb > 0);
  const double s = ctl.dc[DC_S];
  // Both coefficient sets go through LDS into VGPRs: as uniform values they would want 4 MAXK SGPRs on top of the addresses.
  __shared__ double s_cf[2 * MAXK];
  for (int j = threadIdx.x; j < 2 * MAXK; j += kBlock) {
    const int k = j < MAXK ? j : j - MAXK;
    s_cf[j] = k < np ? (j < MAXK ? ctl.rp_cprev()[k] : ctl.rp_cnew()[k]) : 0.0;
  }
  __syncthreads();
  double cp[MAXK], cn[MAXK];
  const double *uk[MAXK];
  long long slv[MAXK];
#pragma unroll
  for (int j = 0; j < MAXK; j++) {
    cp[j] = s_cf[j];
    cn[j] = s_cf[MAXK + j];
    slv[j] = ctl.rp_v()[j];
  }
#pragma unroll
  for (int j = 0; j < MAXK; j++) uk[j] = j < np ? vs.w + slv[j] : f;

  const int lane_off = threadIdx.x * VEC;
#define DEAD_OFF(live, off) ((live) ? (off) : (int64_t)lane_off)      // (dead ring slots: see k_combine_win)
  V finv[T], w0v[T], rv[W][T];
  int64_t t = tail_block ? ntile : (int64_t)blockIdx.x;
  if (t < ntile) {
    const int64_t e = t * TILE + lane_off;
#pragma unroll
    for (int q = 0; q < T; q++) {
      finv[q] = ld<VEC>(f + e + q * (kBlock * VEC));
      w0v[q] = ld<VEC>(w1 + e + q * (kBlock * VEC));
    }
#pragma unroll
    for (int j = 0; j < W; j++)
#pragma unroll
      for (int q = 0; q < T; q++) rv[j][q] = ld<VEC>(uk[j] + DEAD_OFF(j < np, e) + q * (kBlock * VEC));
  }
  list_word_publish(ctl, ncomb, flags & kPbNoStoreW);
  const unsigned grp = tickets ? blockIdx.x % (unsigned)ng : 0u;
  unsigned *const my_ticket = tickets ? tickets + grp * kTicketStride : nullptr;
  const unsigned ticket_base = tickets ? 2u * (unsigned)G / (unsigned)ng : 0u;
  int64_t tnext = t + G;
  unsigned par = 0;
  while (t < ntile) {
    const int64_t e = t * TILE + lane_off;
    const bool more = tnext < ntile;
    unsigned claimed = kNoTicket;
    if (tickets && more && threadIdx.x == 0) claimed = ticket_request(my_ticket, ticket_base, (unsigned)ng, grp);
    const int64_t tn = more ? tnext : t;
    const int64_t en = tn * TILE + lane_off;
    V fin[T], w0[T], v1[T], x[T], kept[MAXK][T];
#pragma unroll
    for (int q = 0; q < T; q++) {
      fin[q] = finv[q];
      w0[q] = w0v[q];
      v1[q] = w0[q];
      if (store_w) st(wnew + e + q * (kBlock * VEC), fin[q]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < T; q++) {
      finv[q] = ld<VEC>(f + en + q * (kBlock * VEC));
      w0v[q] = ld<VEC>(w1 + en + q * (kBlock * VEC));
    }
#pragma unroll
    for (int j = 0; j < MAXK; j++) {
#pragma unroll
      for (int q = 0; q < T; q++) kept[j][q] = rv[j % W][q];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < T; q++) {
        if (j + W < MAXK) rv[j % W][q] = ld<VEC>(uk[j + W] + DEAD_OFF(j + W < np, e) + q * (kBlock * VEC));
        else rv[j % W][q] = ld<VEC>(uk[j + W - MAXK] + DEAD_OFF(j + W - MAXK < np, en) + q * (kBlock * VEC));
      }
      __builtin_amdgcn_sched_barrier(0);
      if (j < np) {
#pragma unroll
        for (int q = 0; q < T; q++)
#pragma unroll
          for (int c = 0; c < VEC; c++) setc(v1[q], c, ex(v1[q], c) + cp[j] * ex(kept[j][q], c));
      }
    }
#pragma unroll
    for (int q = 0; q < T; q++) {
      V wn, un;
#pragma unroll
      for (int c = 0; c < VEC; c++) {
        const double d = ex(w0[q], c) - ex(fin[q], c);
        const double wq = d / s;
        const double vq = ex(v1[q], c) / s;
        setc(wn, c, wq);
        setc(un, c, vq - wq);
        setc(x[q], c, ex(fin[q], c) + c0 * (vq - wq));
      }
      st(w1 + e + q * (kBlock * VEC), wn);
      st(u1 + e + q * (kBlock * VEC), un);
    }
#pragma unroll
    for (int j = 0; j < MAXK; j++) {
      if (j < np && ((keep >> j) & 1u)) {
#pragma unroll
        for (int q = 0; q < T; q++)
#pragma unroll
          for (int c = 0; c < VEC; c++) setc(x[q], c, ex(x[q], c) + cn[j] * ex(kept[j][q], c));
      }
    }
#pragma unroll
    for (int q = 0; q < T; q++) {
      if (store_v) st(vnew + e + q * (kBlock * VEC), x[q]);
      if (store_f) st(f + e + q * (kBlock * VEC), x[q]);
    }
    const int64_t t2 = tickets ? ticket_publish(s_next, par, claimed, ntile) : tnext + G;
    t = tnext;
    tnext = t2;
  }
  if (tickets && !tail_block) ticket_finish(tickets, ng, G);
  if (tail_block) {  // ragged tail, scalar
    for (int64_t i = ntile * TILE + threadIdx.x; i < vs.n; i += kBlock) {
      const double fin = f[i], w0 = w1[i];
      double v1 = w0, kept[MAXK];
#pragma unroll
      for (int j = 0; j < MAXK; j++) {
        kept[j] = 0.0;
        if (j < np) {
          kept[j] = uk[j][i];
          v1 = v1 + cp[j] * kept[j];
        }
      }
      const double d = w0 - fin;
      const double wq = d / s;
      const double vq = v1 / s;
      const double un = vq - wq;
      w1[i] = wq;
      u1[i] = un;
      double x = fin + c0 * un;
#pragma unroll
      for (int j = 0; j < MAXK; j++)
        if (j < np && ((keep >> j) & 1u)) x = x + cn[j] * kept[j];
      if (store_w) wnew[i] = fin;
      if (store_v) vnew[i] = x;
      if (store_f) f[i] = x;
    }
  }
#undef DEAD_OFF
}

// v of the pending pair where an update has deferred it (PC_VDEFER; returns at once where none has, like the repair launches
// of the skipped last vector): f_out = f_in + c_0 u_0 + c_1 u_1 + ... with the statements of PB in PB's order, from the
// combine plan as that update left it.  `clear` != 0: a second launch behind the first that only clears the word (no block of
// the first may find it clear while another still streams); relax and restart launch that one alone.
__global__ __launch_bounds__(kBlock) void k_materialise_v(Ctl ctl, Vecs vs, int clear) {
  if (ctl.pc[PC_VDEFER] == 0) return;
  if (clear) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl.pc[PC_VDEFER] = 0;
    return;
  }
  const int ncomb = ctl.ic[IC_NCOMB];
  const double *w = vs.w + ctl.pc[PC_NEW_W];
  double *v = vs.w + ctl.pc[PC_NEW_V];
  const long long *cv = ctl.comb_v();
  const double *cc = ctl.comb_c();
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < vs.n; i += (int64_t)gridDim.x * kBlock) {
    double x = w[i];
    for (int j = 0; j < ncomb; j++) x = x + cc[j] * (vs.w + cv[j])[i];
    v[i] = x;
  }
}

template <int MAXK, int COMB, int W, int T = 1, bool DEFER = false>
__global__ __launch_bounds__(kBlock) void k_combine_win(Ctl ctl, Vecs vs, double *f, unsigned *tickets, int ng, int flags,
                                                        int base) {
  // T = 16-byte pieces per thread, stream and tile (tile = 512*T elements, 4*T KiB per stream and
  // block): T = 2 halves the ticket rate, which is what lets SHORT lists use one counter (a
  // single counter saturates near 60-75 tickets/us; tools/hbm_probe mode i: 12 + 5 streams move
  // 6.3-6.4 TB/s with T = 2 and one counter against 5.7 with T = 1 and two, 5.4 static).
  constexpr int VEC = 2;
  using V = typename VecT<VEC>::type;
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  constexpr int TILE = kBlock * VEC * T;
  static_assert(MAXK % W == 0, "the ring must divide the pairs of a tile");
  NKA_STAMP0(ctl, 14);
  __shared__ unsigned s_next[2];
  // The ragged tail (n mod TILE elements, scalar) has a block of its own, the LAST of the grid, launched only when
  // there is a tail: appended to the last tile block's work it made that block -- and so the launch -- one memory
  // round trip longer (2.3 us of a 13 us launch at n = 1e5).  Elementwise pass: who handles an element changes no bit.
  const int64_t ntile = vs.n / TILE;
  const bool has_tail = ntile * TILE < vs.n;
  const int G = (int)gridDim.x - (has_tail ? 1 : 0);       // tile blocks
  const bool tail_block = has_tail && (int)blockIdx.x == G;
  const int ncomb_all = ctl.ic[IC_NCOMB];
  const int ncomb = ncomb_all - base;                      // pairs of the plan from `base` on (this launch applies the first MAXK)
  double *wnew = vs.w + ctl.pc[PC_NEW_W], *vnew = vs.w + ctl.pc[PC_NEW_V];
  const long long *cw = ctl.comb_w() + base, *cv = ctl.comb_v() + base;
  const double *cc = ctl.comb_c() + base;
  // (uniform: out-of-place update.  The two scalar branches around the stores cost the in-place path nothing measurable:
  //  interleaved A/B against a build with unconditional stores, profiles/r04/ab_pb_flags.txt)
  const bool first_pass = !(flags & kPbNotFirst), last_pass = !(flags & kPbNotLast);
  const bool store_w = !(flags & kPbNoStoreW) && first_pass, store_f = !(flags & kPbNoStoreF);
  const bool store_v = last_pass && !(DEFER && (flags & kPbMayDefer) && ncomb_all > 0);
  const bool norm0 = first_pass && ctl.ic[IC_NORMED] != 0;
  if constexpr (DEFER) {
    static_assert(COMPACT, "the deferred v exists for compact storage only");
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl.pc[PC_VDEFER] = store_v ? 0 : 1;      // (nothing in this launch reads the word)
    const int np = norm0 ? (int)ctl.pc[PC_VREPLAY] : 0;
    if (np > 0) {                                // (uniform) the pending pair's v was deferred: form it on the way
      combine_win_replay<MAXK, W, T>(ctl, vs, f, tickets, ng, flags, np, s_next);
      return;
    }
  }
  const double s = ctl.dc[DC_S];
  const double rs = 1.0 / s;

  double *wk[MAXK], *vk[MAXK];
  double ck[MAXK];
  long long slw[MAXK], slv[MAXK];
#pragma unroll
  for (int j = 0; j < MAXK; j++) {     // all addresses and coefficients in one batch of scalar loads (see k_dots_win)
    if (!COMPACT || j == 0) slw[j] = cw[j];      // (compact storage reads w of the pending pair only)
    slv[j] = cv[j];
    ck[j] = cc[j];
  }
#pragma unroll
  for (int j = 0; j < MAXK; j++) {
    const bool live = j < ncomb;
    wk[j] = (live && (!COMPACT || j == 0)) ? vs.w + slw[COMPACT ? 0 : j] : f;
    vk[j] = live ? vs.w + slv[j] : f;
  }
  // compact storage reads w only for the pending pair that is normalised now
  const double *w0src = norm0 ? wk[0] : f;

  const int lane_off = threadIdx.x * VEC;                  // piece q of a tile starts q*512 elements further
  // A launch wider than the list (the host's bound is one too high in the update that takes a dependence drop, and too high
  // by more for a caller that never synchronises) has DEAD ring slots.  They re-read f's first tile (4 KiB that stay in the
  // caches) rather than the tile at hand, half of which came from HBM again (PMC: 19.55 words per element where the list
  // needs 19; PB -2.5 % with the first tile, neutral without dead slots).
#define DEAD_OFF(live, off) ((live) ? (off) : (int64_t)lane_off)
  V finv[T], w0v[T], rw[COMPACT ? 1 : W][T], rv[W][T];
  int64_t t = tail_block ? ntile : (int64_t)blockIdx.x;
  if (t < ntile) {
    const int64_t e = t * TILE + lane_off;
#pragma unroll
    for (int q = 0; q < T; q++) {
      finv[q] = ld<VEC>(f + e + q * (kBlock * VEC));
      if (COMPACT) w0v[q] = ld<VEC>(w0src + e + q * (kBlock * VEC));
    }
#pragma unroll
    for (int j = 0; j < W; j++)
#pragma unroll
      for (int q = 0; q < T; q++) {
        if (!COMPACT) rw[j][q] = ld<VEC>(wk[j] + DEAD_OFF(j < ncomb, e) + q * (kBlock * VEC));
        rv[j][q] = ld<VEC>(vk[j] + DEAD_OFF(j < ncomb, e) + q * (kBlock * VEC));
      }
  }
  if (first_pass) list_word_publish(ctl, ncomb_all, flags & kPbNoStoreW);      // (behind the first ring of loads: nothing waits for it)
  // ticket counter of this block's group; ticket k of group g is tile (k + 2G/ng)*ng + g
  const unsigned grp = tickets ? blockIdx.x % (unsigned)ng : 0u;
  unsigned *const my_ticket = tickets ? tickets + grp * kTicketStride : nullptr;
  const unsigned ticket_base = tickets ? 2u * (unsigned)G / (unsigned)ng : 0u;
  int64_t tnext = t + G;
  unsigned par = 0;
  while (t < ntile) {
    const int64_t e = t * TILE + lane_off;
    const bool more = tnext < ntile;
    unsigned claimed = kNoTicket;
    if (tickets && more && threadIdx.x == 0) claimed = ticket_request(my_ticket, ticket_base, (unsigned)ng, grp);
    const int64_t tn = more ? tnext : t;                 // the last iteration prefetches its own tile again
    const int64_t en = tn * TILE + lane_off;
    V fin[T], w0[T], x[T];
#pragma unroll
    for (int q = 0; q < T; q++) {
      fin[q] = finv[q];
      w0[q] = COMPACT ? w0v[q] : fin[q];
      x[q] = fin[q];
      if (store_w) st(wnew + e + q * (kBlock * VEC), fin[q]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < T; q++) {
      finv[q] = ld<VEC>(f + en + q * (kBlock * VEC));
      if (COMPACT) w0v[q] = ld<VEC>(w0src + en + q * (kBlock * VEC));
    }
#pragma unroll
    for (int j = 0; j < MAXK; j++) {
      V wj[T], vj[T];
#pragma unroll
      for (int q = 0; q < T; q++) {
        wj[q] = COMPACT ? w0[q] : rw[COMPACT ? 0 : j % W][q];
        vj[q] = rv[j % W][q];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < T; q++) {
        if (j + W < MAXK) {
          if (!COMPACT) rw[COMPACT ? 0 : j % W][q] = ld<VEC>(wk[j + W] + DEAD_OFF(j + W < ncomb, e) + q * (kBlock * VEC));
          rv[j % W][q] = ld<VEC>(vk[j + W] + DEAD_OFF(j + W < ncomb, e) + q * (kBlock * VEC));
        } else {
          if (!COMPACT) rw[COMPACT ? 0 : j % W][q] = ld<VEC>(wk[j + W - MAXK] + DEAD_OFF(j + W - MAXK < ncomb, en) + q * (kBlock * VEC));
          rv[j % W][q] = ld<VEC>(vk[j + W - MAXK] + DEAD_OFF(j + W - MAXK < ncomb, en) + q * (kBlock * VEC));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (j == 0 && norm0) {
#pragma unroll
        for (int q = 0; q < T; q++) {
#pragma unroll
          for (int c = 0; c < VEC; c++) {
            const double d = ex(wj[q], c) - ex(fin[q], c);
            const double wn = RCP ? rs * d : d / s;
            const double vn = RCP ? rs * ex(vj[q], c) : ex(vj[q], c) / s;
            setc(wj[q], c, wn);
            setc(vj[q], c, COMPACT ? vn - wn : vn);
          }
          st(wk[0] + e + q * (kBlock * VEC), wj[q]);
          st(vk[0] + e + q * (kBlock * VEC), vj[q]);
        }
      }
      if (j < ncomb) {
#pragma unroll
        for (int q = 0; q < T; q++)
#pragma unroll
          for (int c = 0; c < VEC; c++) {
            if (COMPACT) setc(x[q], c, ex(x[q], c) + ck[j] * ex(vj[q], c));
            else setc(x[q], c, comb1<COMB>(ex(x[q], c), ck[j], ex(wj[q], c), ex(vj[q], c)));
          }
      }
    }
#pragma unroll
    for (int q = 0; q < T; q++) {
      if (store_v) st(vnew + e + q * (kBlock * VEC), x[q]);
      if (store_f) st(f + e + q * (kBlock * VEC), x[q]);
    }
#ifdef NKA_SOLVE_STAMPS
    if (t == (int64_t)blockIdx.x) NKA_STAMP0(ctl, 15);       // block 0: its first tile is done
#endif
    const int64_t t2 = tickets ? ticket_publish(s_next, par, claimed, ntile) : tnext + G;
    t = tnext;
    tnext = t2;
  }
  if (tickets && !tail_block) ticket_finish(tickets, ng, G);
  if (tail_block) {  // ragged tail, scalar
    for (int64_t i = ntile * TILE + threadIdx.x; i < vs.n; i += kBlock) {
      const double fin = f[i];
      double x = fin;
#pragma unroll
      for (int j = 0; j < MAXK; j++) {
        if (j < ncomb) {
          double v = vk[j][i];
          double w = (!COMPACT || (j == 0 && norm0)) ? wk[j][i] : 0.0;
          if (j == 0 && norm0) {
            const double d = w - fin;
            w = RCP ? rs * d : d / s;
            v = RCP ? rs * v : v / s;
            if (COMPACT) v = v - w;
            wk[0][i] = w;
            vk[0][i] = v;
          }
          x = COMPACT ? x + ck[j] * v : comb1<COMB>(x, ck[j], w, v);
        }
      }
      if (store_w) wnew[i] = fin;
      if (store_v) vnew[i] = x;
      if (store_f) f[i] = x;
    }
  }
#undef DEAD_OFF
}

__global__ __launch_bounds__(kSolveThreads) void k_restart(Ctl ctl, int in_global) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Lst L;
  lst_load(L, ctl, smem, in_global);
  if (threadIdx.x == 0) lst_restart(L);
  lst_store(L, ctl, in_global);
}

__global__ __launch_bounds__(kSolveThreads) void k_relax(Ctl ctl, int in_global) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Lst L;
  lst_load(L, ctl, smem, in_global);
  if (threadIdx.x == 0) lst_relax(L);
  lst_store(L, ctl, in_global);
}

// The scalar part of accel_update between PA and PB, reference loops verbatim on one lane.
// `phase`: 0 = the whole step.  The user-dot-product path (nka_hip_set_host_dot) runs it in two halves so that
// the host can ask the user's dp for the projection row AFTER the drop decisions, as the reference does (F08:371
// comes behind F08:295-347): 1 = norm, s == 0 -> relax, Gram row, factorisation with drops; 2 = new slot, the
// substitutions on the right-hand side the host has put into c[] BY SLOT, combine plan, prepend.
__global__ __launch_bounds__(kSolveThreads) void k_solve(Ctl ctl, int mode, int in_global, int phase, long long swap_w,
                                                         long long swap_v, P2P x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (x.base != nullptr) p2p_gather_block(x, ctl.red(), ctl.red_count());      // the sums of all ranks, in rank order
  Lst L;
  lst_load(L, ctl, smem, in_global);
  if (threadIdx.x == 0) {
    const double *red = ctl.red();
    const int32_t *ps = ctl.plan_slots();
    const int nolder = ctl.ic[IC_PLAN_NOLDER];
    const int entry_first = L.first;
    bool normed = (phase == 2) ? ctl.ic[IC_NORMED] != 0 : false;
    double s = (phase == 2) ? ctl.dc[DC_S] : 0.0;
    if (phase != 2) {
      if (L.pending) {
        s = sqrt(red[0]);                       // F08:267
        ctl.dc[DC_S] = s;
        if (s == 0.0) {                         // F08:275
          lst_relax(L);
          ctl.ic[IC_NRELAX] += 1;
        }
      }
      const double rs = 1.0 / s;
      if (L.pending) {
        normed = true;
        // Gram row of w1' = d/s from the raw sums <d,w_k> of PA (F08:286-290)
        for (int p = 0; p < nolder; p++) L.H(L.first, ps[p]) = solve_nrm(red[2 + p], s, rs, mode);
        lst_factor(L);
      }
      ctl.ic[IC_NORMED] = normed ? 1 : 0;
    }
    if (phase != 1) {
      const double rs = 1.0 / s;
      const int slot = L.free_;
      L.free_ = L.next[slot];
      int ncomb = 0;
      if (L.subspace) {
        if (phase == 0) {
          if (normed) L.c[entry_first] = solve_nrm(red[1], s, rs, mode);   // <f,w1'> = <f,d>/s
          for (int p = 0; p < nolder; p++) L.c[ps[p]] = red[2 + ctl.mvec + p];
        }
        lst_solve(L);
        for (int k = L.first; k != 0; k = L.next[k]) {
          ctl.comb_slots()[ncomb] = k;
          ctl.comb_w()[ncomb] = ctl.wtab()[k];
          ctl.comb_v()[ncomb] = ctl.vtab()[k];
          ctl.comb_c()[ncomb] = L.c[k];
          ncomb++;
        }
      }
      ctl.ic[IC_NCOMB] = ncomb;
      ctl.ic[IC_NEW] = slot;
      assign_new_buffers(ctl, slot, swap_w, swap_v);     // (before lst_store resolves the next plan through the tables)
      lst_prepend(L, slot);
    }
  }
  lst_store(L, ctl, in_global);
}

// ---- the same scalar step with the O(m^3) arithmetic spread over ONE wavefront ----
// k_solve above runs the reference loops verbatim on one lane (~130 us at m=20: every step waits
// on an LDS-resident linked list).  k_solve_rows linearises the list, gathers the Gram entries
// into a dense position-indexed matrix and factorises it RIGHT-LOOKING: when column i is reached
// its pivot is final (decide keep / drop exactly as F08:326), the column is scaled by one division
// per row (lanes = rows) and every trailing entry gets
//      a(p,q) <- a(p,q) - a(p,i)*a(q,i)
// Each entry thus receives the same subtractions in the same (ascending i) order as the
// reference's inner loop F08:316-319, then the same division F08:320 -- bit-identical results,
// ~m sequential steps instead of ~m^3/3.  The right-hand side rides along as one more row (forward
// substitution, F08:369-379); the back-substitution (F08:382-392) is column-oriented in the same
// way.  List surgery (drops, free-list pushes in list order, new slot, prepend) is O(m) and done
// redundantly by all lanes on private copies of the scalars.  Requires mvec+1 <= kSolveWaveMax;
// larger subspaces use k_solve.
//
// What sets the run time of a LONE wavefront (tools/solve_phases.py, s_memtime stamps;
// profiles/r02 and r03/solve_phases*.txt for the forms tried) is, in this order: serial round trips
// (LDS ~130 cycles, global ~500-2000), taken branches (~20 cycles each), and the issue rate of
// dependent fp64 instructions (~6 cycles each; sqrt and divide are ~15-instruction chains).  So:
//   * ONE global round trip at entry: every load of the state, sums and plan issued before the first
//     is waited for (as plain loops the compiler emits load -> wait -> ds_write per iteration);
//   * the list order comes from the plan (no walk); lane p holds row p of the matrix IN REGISTERS,
//     pivots and column entries travel by v_readlane with a uniform source lane (a scalar
//     broadcast): no LDS access and no barrier inside the factorisation;
//   * constant trip counts and guards instead of break / continue, no per-entry branches: both
//     loops unroll completely and the inner one is straight-line code;
//   * `alive` as a 64-bit mask: drops are visited by count-trailing-zeros, compaction by
//     population count, in parallel;
//   * the factor goes to LDS once (the back-substitution reads COLUMNS of it, requested as one
//     batch) and to the stored matrix by slot with branch-free predicated addresses; the plan of
//     the next update is written in parallel.
// History: k_solve_wave (LDS-resident, round 2: ~66 k cycles at m = 20), k_solve_wave2 (pairs dealt
// to lanes, LDS column exchange with two barriers per column: 42.9 k), a ds_bpermute variant
// (50 k, not kept), this one: 26.4 k.  The rare path without a new pair (after relax / s == 0)
// keeps the first version's gather-and-substitute code.
constexpr int kSolveWaveMax = 63;     // (round 5: 48 -> 63, one more instantiation: the lanes were there; mvec <= 62)

__host__ __device__ inline size_t solve_wave_smem_bytes(int mvec) {
  const int nl = mvec + 1;
  size_t b = (lst_smem_bytes(mvec) + 15) / 16 * 16;
  b += (size_t)((nl + 1) * (nl + 1) + 3 * nl + (2 + 2 * mvec)) * sizeof(double);
  b += (size_t)(3 * nl + 1) * sizeof(int32_t);                // (+1: keeps the pointer tables behind them 8-byte aligned)
  b = (b + 7) / 8 * 8;
  b += (size_t)(2 * (nl + 1)) * sizeof(long long);            // slot -> buffer tables (Ctl::wtab / vtab)
  return b;
}

// NLMAX >= list length is a template parameter: both loops of the factorisation are fully unrolled so
// that the row a[] stays in registers (62 VGPRs at NLMAX = 21, 116 at 48; no scratch).  Column i:
// l_p = a_p[i] / L_ii on every lane, then for q = i+1 .. (uniform loop) a_p[q] -= l_p * l_q with
// l_q = readlane(l, q) -- lanes p <= q update entries nobody reads.
template <int NLMAX>
__global__ __launch_bounds__(kSolveThreads) void k_solve_rows(Ctl ctl, int mode, long long swap_w, long long swap_v,
                                                              long long id_stride, long long id_vbase, P2P x, int skip, int vd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  if (skip_repair_idle(ctl, skip)) return;     // (the second scalar step of an update that skipped: nothing to repair)
  // `vd`: the PB behind this step is the instantiation that can replay a deferred v (k_combine_win, DEFER): this step tells it
  // whether to (PC_VREPLAY) and writes the replay plan.  Lane p holds what entry p - 1 of the OLD combine plan was combined
  // with -- the old plan IS this update's list of older entries, position p -- before the new plan overwrites it.
  const bool vd_in = vd != 0 && ctl.pc[PC_VDEFER] != 0;
  double vd_cprev = 0.0;
  long long vd_v = 0;
  if (vd != 0 && lane >= 1 && lane <= ctl.mvec) {
    vd_cprev = ctl.comb_c()[lane - 1];
    vd_v = ctl.comb_v()[lane - 1];
  }
  // peer-to-peer exchange: wait for the rows of all ranks and add them in rank order (P2P above); red[] then holds the
  // global sums like after an all-reduce (lane e reads back below what it has just written itself)
  if (x.base != nullptr) p2p_gather_block(x, ctl.red(), ctl.red_count());
  const int m1 = ctl.m1(), NL = m1, LDA = NL + 1, M = ctl.mvec, nh = (m1 + 1) * (m1 + 1);
  Lst L;
  L.m1 = m1;
  L.mvec = M;
  L.h = reinterpret_cast<double *>(smem);
  L.c = L.h + nh;
  L.next = reinterpret_cast<int32_t *>(L.c + (m1 + 1));
  L.prev = L.next + (m1 + 1);
  double *A = reinterpret_cast<double *>(smem + (lst_smem_bytes(ctl.mvec) + 15) / 16 * 16);
  double *bb = A + (NL + 1) * LDA + 2 * NL;   // (the 2*NL doubles in between are unused)
  double *redL = bb + NL;
  int32_t *ord = reinterpret_cast<int32_t *>(redL + (2 + 2 * M));
  int32_t *psL = ord + 2 * NL;
  long long *wtL = reinterpret_cast<long long *>((reinterpret_cast<uintptr_t>(psL + NL + 1) + 7) / 8 * 8);   // [m1 + 1]
  long long *vtL = wtL + (m1 + 1);                                                                            // [m1 + 1]
  NKA_STAMP(ctl, 0);
  // ---- one global round trip: EVERY load is issued before the first is waited for (written as plain
  //      loops the compiler emits load -> s_waitcnt vmcnt(0) -> ds_write per iteration: eleven serial
  //      round trips of ~500 cycles at mvec = 20).  m1 + 1 <= kSolveWaveMax + 1 <= 64 and
  //      2 + 2 mvec <= 128, so the lists, sums and plan take one or two loads a lane; the Gram
  //      matrix kHB a lane (mvec <= 21), the rest of a larger one in the old loop.
  const int nolder = ctl.ic[IC_PLAN_NOLDER];
  const int hold_in = ctl.ic[IC_SKIP_HOLD];
  {
    constexpr int kHB = 8;
    static_assert(kSolveWaveMax + 1 <= kSolveThreads, "lists: one load a lane");
    const double *gh = ctl.h(), *gred = ctl.red();
    double hreg[kHB], rreg[2], creg = 0.0;
    long long wtreg = 0, vtreg = 0;
    int32_t nreg = 0, preg = 0, psreg = 0;
#pragma unroll
    for (int k = 0; k < kHB; k++) hreg[k] = (lane + kSolveThreads * k < nh) ? gh[lane + kSolveThreads * k] : 0.0;
#pragma unroll
    for (int k = 0; k < 2; k++) rreg[k] = (lane + kSolveThreads * k < 2 + 2 * M) ? gred[lane + kSolveThreads * k] : 0.0;
    if (lane < m1 + 1) {
      creg = ctl.c()[lane];
      nreg = ctl.next()[lane];
      preg = ctl.prev()[lane];
      // id_stride != 0: the slot -> buffer tables are still the ones of creation (no out-of-place update yet): slot k at
      // (k-1)*stride of the two slot-major allocations -- computed, not loaded (two more cache lines in the entry round
      // trip cost the one-wavefront step ~1 us at small n)
      if (id_stride != 0) {
        wtreg = (long long)(lane - 1) * id_stride;
        vtreg = id_vbase + (long long)(lane - 1) * id_stride;
      } else {
        wtreg = ctl.wtab()[lane];
        vtreg = ctl.vtab()[lane];
      }
    }
    if (lane < M) psreg = ctl.plan_slots()[lane];        // (bounded by mvec, not by the count still on its way)
#pragma unroll
    for (int k = 0; k < kHB; k++)
      if (lane + kSolveThreads * k < nh) L.h[lane + kSolveThreads * k] = hreg[k];
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (lane + kSolveThreads * k < 2 + 2 * M) redL[lane + kSolveThreads * k] = rreg[k];
    if (lane < m1 + 1) {
      L.c[lane] = creg;
      L.next[lane] = nreg;
      L.prev[lane] = preg;
      wtL[lane] = wtreg;
      vtL[lane] = vtreg;
    }
    if (lane < nolder) psL[lane] = psreg;
    for (int i = lane + kSolveThreads * kHB; i < nh; i += kSolveThreads) L.h[i] = gh[i];
  }
  lst_load_scalars(L, ctl);
  L.vtol = ctl.dc[DC_VTOL];
  const int entry_pending = L.pending;
  // PA left out the last vector of a full list (nka_device.hpp, kSkipMay: the same three conditions as there): its two sums
  // read 0.  The capacity drop normally ends the list before either is looked at; where this step is about to need them
  // -- s == 0 keeps the whole older list, a dependence drop makes room for the last entry -- it raises IC_REDO and returns
  // with NOTHING of the state stored (everything so far went to LDS and registers): the guarded launches behind it form
  // the sums and run this step again (kSkipRepair), which then takes them as any other.
  const bool skipped = !(skip & kSkipRepair) && skip_last_planned(ctl, skip, entry_pending, nolder);
  bool redo = false;
  __syncthreads();
  NKA_STAMP(ctl, 1);
  const double vtol2 = L.vtol * L.vtol;

  // ---- phase 0: norm, s == 0 -> relax, Gram row of w1' = d/s, right-hand side
  const int entry_first = L.first;
  int normed = 0;
  double s = 0.0;
  if (L.pending) {
    s = sqrt(redL[0]);                        // F08:267
    if (s == 0.0) lst_relax(L);               // F08:275
  }
  if (skipped && s == 0.0) redo = true;       // (every older entry stays: the projection on the last one is needed)
  if (L.pending) normed = 1;
  {
    const double rs = 1.0 / s;
    for (int p = lane; p < nolder; p += kSolveThreads) {
      if (normed) L.H(L.first, psL[p]) = solve_nrm(redL[2 + p], s, rs, mode);         // F08:286-290
      L.c[psL[p]] = redL[2 + M + p];                                                 // F08:371
    }
    if (normed && lane == 0) L.c[entry_first] = solve_nrm(redL[1], s, rs, mode);     // <f,w1'> = <f,d>/s
  }
  if (redo) {                                    // s == 0 with the last vector skipped (uniform; nothing stored yet)
    if (lane == 0) {
      ctl.ic[IC_REDO] = 1;
      ctl.ic[IC_NREDO] += 1;
    }
    return;
  }
  __syncthreads();
  // list position -> slot WITHOUT walking the list: with a new pair this call the list is `first` followed
  // by the plan (the older entries in list order, which PA's sums follow too; every operation that changes
  // the list rewrites the plan).  The path without a new pair walks the list itself, below.
  const int nl = normed ? 1 + nolder : 0;
  const int myord = normed ? (lane == 0 ? entry_first : (lane <= nolder ? psL[lane - 1] : 0)) : 0;
  NKA_STAMP(ctl, 2);
  const uint64_t listmask = (nl >= 64) ? ~0ull : ((1ull << nl) - 1);
  uint64_t alive = listmask;
  int capdrop = -1;
  bool forward_done = false;
  double ddr = 1.0;    // lane p: running pivot 1 - sum l^2 of list position p
  double Ldr = 1.0;    // lane p: accepted pivot sqrt(hkk)
  double yr = 0.0;     // lane p: right-hand side / solution of list position p
  int nk = 0;

  if (normed) {
    // ---- phase 1: right-looking Cholesky with drops (F08:295-347), rows 0..nl-1,
    //      plus the right-hand side as row nl (lane p scales row p of each column).
    // Row p of the matrix is gathered into the registers of lane p (the loads are issued as a batch).
    double a[NLMAX];
#pragma unroll
    for (int q = 0; q < NLMAX; q++) {
      const int oq = __builtin_amdgcn_readlane(myord, q);      // slot of list position q (0 beyond the list)
      a[q] = (lane < nl) ? L.H(oq, myord)                      // raw <w_q,w_p>, q newer (used for q < p only)
                         : L.c[oq];                            // row nl: rhs <f,w_q>
    }
    NKA_STAMP(ctl, 3);
    int kept = 0;
    bool open_ = true;                           // false once the capacity drop has ended the list (F08:309 exit)
    // (constant trip counts, guards instead of break / continue: both loops must unroll completely)
#pragma unroll
    for (int i = 0; i < NLMAX; i++) {
      bool keep = false;
      double Lii = 1.0;
      if (open_ && i < nl) {
        if (i == 0) {
          keep = true;                           // F08:295 h(first,first) = 1
        } else if (kept + 1 > L.mvec) {
          capdrop = i;                           // F08:301-308 capacity: i is the last entry
          open_ = false;
        } else {
          if (skipped && i == nl - 1) redo = true;      // the last position is evaluated after all: its row was not summed
          const double hkk = readlane_f64(ddr, i);
          keep = hkk > vtol2;                    // F08:326
          if (keep) Lii = sqrt(hkk);
        }
        if (!keep) alive &= ~(1ull << i);
      }
      if (keep) {
        kept++;
        if (lane == i) Ldr = Lii;
        const double l = a[i] / Lii;             // F08:320 (row nl: F08:377); rows <= i: unused
        a[i] = l;
        if (lane > i && lane < nl) ddr = ddr - l * l;            // F08:321
#pragma unroll
        for (int q = i + 1; q < NLMAX; q++)                      // (no guard q < nl: straight-line code; columns
          a[q] = a[q] - l * readlane_f64(l, q);                  //  beyond the list hold values nobody reads)
                                                                 // trailing entry (p,q), p > q: F08:317 (row nl: F08:374)
      }
    }
    NKA_STAMP(ctl, 4);
    if (redo) {                                  // (uniform; no global store has happened yet)
      if (lane == 0) {
        ctl.ic[IC_REDO] = 1;
        ctl.ic[IC_NREDO] += 1;
      }
      return;
    }
    // ---- phase 2: the factor back by slot, and into LDS for the back-substitution (which reads
    //      COLUMNS of it); replay the drops in list order
    // (branch-free: a lone wavefront pays ~20 cycles for every taken branch.  Rows are written whole --
    //  the part right of the diagonal and the columns beyond the list, folded onto column nl, are
    //  read by nobody -- and an entry that must NOT reach the stored factor goes to a dump word.)
    {
      double *const dump = A + NL * LDA + NL;
      const uint64_t rowbits = (lane < nl && ((alive >> lane) & 1)) ? (alive & ((1ull << lane) - 1)) : 0ull;
      if (lane <= nl) {
#pragma unroll
        for (int q = 0; q < NLMAX; q++) A[lane * LDA + (q < nl ? q : nl)] = a[q];
      }
#pragma unroll
      for (int q = 0; q < NLMAX; q++) {
        const int oq = __builtin_amdgcn_readlane(myord, q);
        double *const dst = ((rowbits >> q) & 1) ? &L.H(myord, oq) : dump;
        *dst = a[q];
      }
    }
    __syncthreads();
    if (lane < nl && ((alive >> lane) & 1)) L.H(myord, myord) = Ldr;
    if (lane < nl) yr = A[nl * LDA + lane];    // forward-substituted right-hand side of position p
    forward_done = true;
    for (uint64_t dm = ~alive & listmask & ~1ull; dm != 0; dm &= dm - 1) {
      const int p = __builtin_ctzll(dm);
      const int k = __builtin_amdgcn_readlane(myord, p);
      if (p == capdrop) {                      // F08:303-307
        L.next[L.last] = L.free_;
        L.free_ = k;
        L.last = L.prev[k];
        L.next[L.last] = 0;
      } else {                                 // F08:331-340
        const int pv = L.prev[k], nx = L.next[k];
        L.next[pv] = nx;
        if (nx == 0) L.last = pv; else L.prev[nx] = pv;
        L.next[k] = L.free_;
        L.free_ = k;
      }
    }
    L.subspace = 1;
    L.pending = 0;
    __syncthreads();
  }

  // ---- phase 3: new slot, then the substitutions on the current list
  NKA_STAMP(ctl, 5);
  const int slot = L.free_;                    // F08:357-358
  L.free_ = L.next[slot];
  // buffers of the new pair (every lane computes the same values; lane 0 writes them): an out-of-place update exchanges
  // them (assign_new_buffers).  The new slot is never one of the entries combined below (it comes off the free list).
  const long long new_w = swap_w != kNoBuffer ? swap_w : wtL[slot], new_v = swap_v != kNoBuffer ? swap_v : vtL[slot];
  if (lane == 0) {
    if (swap_w != kNoBuffer) ctl.pc[PC_OLD_W] = wtL[slot];  // (other updates leave PC_OLD_* alone: the host may collect them later)
    if (swap_v != kNoBuffer) ctl.pc[PC_OLD_V] = vtL[slot];
    ctl.pc[PC_NEW_W] = new_w;
    ctl.pc[PC_NEW_V] = new_v;
    ctl.pc[PC_FIRST_W] = new_w;                // the new pair is the pending pair of the next update
    if (swap_w != kNoBuffer) ctl.wtab()[slot] = swap_w;
    if (swap_v != kNoBuffer) ctl.vtab()[slot] = swap_v;
  }
  if (forward_done) {
    // back-substitution F08:382-392 in position space: the factor lies in A, its
    // diagonal in Ldr, the forward-substituted right-hand side in yr
    NKA_STAMP(ctl, 6);
    // column `lane` of the factor, requested as ONE batch of LDS reads (rows / lanes beyond the list fold
    // onto row / column nl: valid addresses, values nobody uses)
    double t[NLMAX];
#pragma unroll
    for (int i = 0; i < NLMAX; i++) t[i] = A[(i < nl ? i : nl) * LDA + (lane < nl ? lane : nl)];
#pragma unroll
    for (int i = NLMAX - 1; i >= 0; i--) {
      if (i < nl && ((alive >> i) & 1)) {
        const double ci = readlane_f64(yr, i) / readlane_f64(Ldr, i);
        if (lane == i) yr = ci;
        if (lane < i && ((alive >> lane) & 1)) yr = yr - t[i] * ci;
      }
    }
    NKA_STAMP(ctl, 7);
    nk = __builtin_popcountll(alive & listmask);
    if (lane < nl && ((alive >> lane) & 1)) {
      const int r = __builtin_popcountll(alive & ((1ull << lane) - 1));   // position among the kept entries
      ctl.comb_slots()[r] = myord;
      ctl.comb_c()[r] = yr;
      ctl.plan_slots()[r] = myord;             // the next update's older entries: this list, in order
      const long long wb = wtL[myord];
      ctl.comb_w()[r] = wb;                    // ... and their addresses for the streaming passes (Ctl::pc)
      ctl.comb_v()[r] = vtL[myord];
      ctl.plan_w()[r] = wb;
      L.c[myord] = yr;
    }
    if (vd_in && lane >= 1 && lane < nl) {      // the replay plan: position `lane` of this list was entry lane - 1 of the old plan
      ctl.rp_v()[lane - 1] = vd_v;
      ctl.rp_cprev()[lane - 1] = vd_cprev;
      ctl.rp_cnew()[lane - 1] = yr;             // (of a dropped position: never read, rp_keep)
    }
  } else if (L.subspace) {
    // no new pair this call (after relax / s == 0): substitute on the stored factor
    for (int k = L.first; k != 0; k = L.next[k]) ord[nk++] = k;
    __syncthreads();
    for (int p = lane; p < nk; p += kSolveThreads) bb[p] = L.c[ord[p]];
    for (int idx = lane; idx < nk * nk; idx += kSolveThreads) {
      const int p = idx / nk, q = idx - p * nk;
      if (p >= q) A[p * LDA + q] = L.H(ord[p], ord[q]);
    }
    __syncthreads();
    for (int i = 0; i < nk; i++) {             // forward, F08:369-379
      const double ci = bb[i] / A[i * LDA + i];
      __syncthreads();
      if (lane == 0) bb[i] = ci;
      for (int j = i + 1 + lane; j < nk; j += kSolveThreads) bb[j] = bb[j] - A[j * LDA + i] * ci;
      __syncthreads();
    }
    for (int i = nk - 1; i >= 0; i--) {        // backward, F08:382-392
      const double ci = bb[i] / A[i * LDA + i];
      __syncthreads();
      if (lane == 0) bb[i] = ci;
      for (int j = lane; j < i; j += kSolveThreads) bb[j] = bb[j] - A[i * LDA + j] * ci;
      __syncthreads();
    }
    for (int p = lane; p < nk; p += kSolveThreads) {
      ctl.comb_slots()[p] = ord[p];
      ctl.comb_c()[p] = bb[p];
      ctl.plan_slots()[p] = ord[p];
      ctl.comb_w()[p] = wtL[ord[p]];
      ctl.comb_v()[p] = vtL[ord[p]];
      ctl.plan_w()[p] = wtL[ord[p]];
      L.c[ord[p]] = bb[p];
    }
  }
  __syncthreads();
  lst_prepend(L, slot);                        // F08:406-417 (every lane, same values)
  NKA_STAMP(ctl, 8);
  // ---- state back to global memory (the plan was written above: without a subspace
  //      the list was empty before the prepend, so the next update has no older entry)
  __syncthreads();
  lst_copy_out(L, ctl, kSolveThreads);
  if (lane == 0) {
    ctl.dc[DC_S] = s;
    if (entry_first != 0 && !normed && entry_pending) ctl.ic[IC_NRELAX] += 1;
    ctl.ic[IC_NEW] = slot;
    ctl.ic[IC_NCOMB] = nk;
    ctl.ic[IC_NORMED] = normed;
    lst_store_scalars(L, ctl);
    ctl.ic[IC_PLAN_PENDING] = L.pending;
    ctl.ic[IC_PLAN_FIRST] = L.first;
    ctl.ic[IC_PLAN_NOLDER] = nk;
    // the next update may skip unless a repair is recent: one that has just run holds the skip off for the following mvec
    // updates, so that a solve which takes dependence drops at a full list in update after update pays one repair in mvec + 1
    int hold = hold_in > 0 ? hold_in - 1 : 0;
    if (skip & kSkipRepair) {
      hold = M;
      ctl.ic[IC_REDO] = 0;
    }
    ctl.ic[IC_SKIP_HOLD] = hold;
    ctl.ic[IC_PLAN_SKIP] = hold == 0 ? 1 : 0;
    if (vd != 0) {
      // a deferred v is replayed by the PB behind this step when the pending pair is normalised now; where s == 0 has dropped
      // the pair (F08:275) nobody needs its v any more.  Either way the word is clear until that PB defers again.
      ctl.pc[PC_VREPLAY] = (vd_in && normed) ? nl - 1 : 0;
      ctl.rp_keep()[0] = (long long)((alive & listmask) >> 1);
      ctl.pc[PC_VDEFER] = 0;
    }
  }
  NKA_STAMP(ctl, 9);
}

}  // namespace nka
