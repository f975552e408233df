// nka_chain.hpp -- the arithmetic of the reference-order sums of LONG vectors: a sequential sum of rounded products taken
// through blocks of 1 024 elements whose roundings are summarised as integer arithmetic.  Device functions and their
// constants only; the kernels built from them are k_chain_* (nka_kernels.hpp) and k_dot_chain (vec_ops.hip).
#pragma once

#include "nka_device.hpp"

namespace nka {

// ---- The same sums, ONE WORKGROUP PER SUM (round 5, long vectors) ----------------------------------
// k_dots_ordered walks every sum on one compute unit and waits for each chunk's loads before it adds: 40 ns per element.
// A sequential sum is a chain of n dependent roundings whatever is done, but (1) the 2 + 2L sums of an update are
// independent chains once the norm is known, (2) the products are not part of any chain and (3) -- see chain_block_summary --
// while the running sum stays inside one binade its roundings are roundings to a FIXED grid, which is integer
// arithmetic and therefore associative.  Here sum c has workgroup c to itself: its eight wavefronts load the next group of
// 8 192 elements, round the products into LDS and summarise one block of 1 024 each, and wavefront 0 takes the group
// through the chain.  Two launches per update: set kChainNorm = the norm (block 0) and, with `with_f`, the sums on f alone (blocks
// 1..ub); set kChainRows = with s from red[0], <f,w1'> (block 0), the Gram row on the ROUNDED w1' (blocks 1..ub) and,
// with `with_f`, the sums on f alone (blocks ub+1..2ub) -- the sharded rounds of ordered_chain take the second form (their
// norm rounds hold red[0] only).  EVERY chain starts from the value red[] holds: the host zeroes red[] where no prefix of
// other ranks is to be continued (0 + p == p: the same bits as starting at 0).
constexpr int kChainWaves = 8;
constexpr int kChainThreads = 64 * kChainWaves;
constexpr int kChainLaneElems = 16;                               // consecutive elements of a block per lane
constexpr int kChainBlock = 64 * kChainLaneElems;                 // elements per step of the chain
constexpr int kChainGroupBlocks = kChainWaves;                    // one block of a group per wavefront
constexpr int kChainGroup = kChainGroupBlocks * kChainBlock;      // elements whose products are in LDS at a time
constexpr int kChainPerThread = kChainGroup / kChainThreads;
constexpr int kChainRow = 2 * 64 + 4;                             // doubles between the PAIR rows of a block in LDS: row k holds
                                                                  // elements 2k, 2k+1 of every lane, lane after lane -- the
                                                                  // lanes of a wavefront read 16 bytes each, side by side
constexpr int kChainBlockLds = (kChainLaneElems / 2) * kChainRow;
constexpr int kChainGroupLds = kChainGroupBlocks * kChainBlockLds;
constexpr size_t kChainLdsBytes = sizeof(double) * kChainGroupLds;   // (dynamic: beyond the 64 KiB of static LDS)
enum { kChainNorm = 0, kChainRows = 1, kChainProbe = 2 };   // (probe: <f, probe> from red[2 + mvec], diagnostic entry)
enum { kChainKindNorm = 0, kChainKindFW1 = 1, kChainKindW1W = 2, kChainKindFW = 3 };
// where element i of a group lies in LDS
__device__ __forceinline__ int chain_idx(int i) {
  const int blk = i / kChainBlock, ib = i % kChainBlock;
  const int lane = ib / kChainLaneElems, j = ib % kChainLaneElems;
  return blk * kChainBlockLds + (j / 2) * kChainRow + 2 * lane + (j & 1);
}
// the 16 products of lane `lane` of a block, in order
__device__ __forceinline__ void chain_lane_read(double (&p)[kChainLaneElems], const double *blk, int lane) {
  using V2 = typename VecT<2>::type;
#pragma unroll
  for (int k = 0; k < kChainLaneElems / 2; k++) {
    const V2 v = *reinterpret_cast<const V2 *>(blk + k * kChainRow + 2 * lane);
    p[2 * k] = v.x;
    p[2 * k + 1] = v.y;
  }
}

// a + p[0] + p[1] + ... + p[len-1] in THAT order, one rounding per addition: the chain as it stands (every lane does the
// same additions on the same LDS words: no divergence, the sum stays wave-uniform).  One lane's worth (16 products) per
// step, read while the additions of the step before wait for one another, two steps per trip (no register copies): the
// loop is the chain of dependent v_add_f64 and little else (2.3 ns each, tools/micro/dep_add.hip).
__device__ __forceinline__ double chain_block_serial(double a, const double *blk, int len, int g = 0) {   // (from lane g on)
#pragma clang fp contract(off)
  const int ng = len / kChainLaneElems;                 // whole lanes
  if (g < ng) {
    double A[kChainLaneElems], B[kChainLaneElems];
    chain_lane_read(A, blk, g);
    for (; g + 2 <= ng; g += 2) {
      chain_lane_read(B, blk, g + 1);
      __builtin_amdgcn_sched_barrier(0);                 // (the reads of the NEXT lane go out before this lane's additions)
#pragma unroll
      for (int j = 0; j < kChainLaneElems; j++) a = a + A[j];
      __builtin_amdgcn_sched_barrier(0);
      chain_lane_read(A, blk, g + 3 <= ng ? g + 2 : g);   // (the last trip re-reads: the loads stay unconditional)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kChainLaneElems; j++) a = a + B[j];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (g < ng) {                                        // (A holds lane g whenever a whole lane remains)
#pragma unroll
      for (int j = 0; j < kChainLaneElems; j++) a = a + A[j];
      g++;
    }
  }
  for (int i = g * kChainLaneElems; i < len; i++) a = a + blk[chain_idx(i)];
  return a;
}

// reductions and one scan over the 64 lanes through DPP (row shifts, then the row broadcasts of gfx9)
template <int CTRL, int RM> __device__ __forceinline__ float dpp_f32(float x, float old) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, RM, 0xf, false));
}
template <int CTRL, int RM> __device__ __forceinline__ int dpp_i32(int x, int old) {
  return __builtin_amdgcn_update_dpp(old, x, CTRL, RM, 0xf, false);
}
template <int CTRL, int RM> __device__ __forceinline__ double dpp_f64(double x, double old) {
  union { double d; int u[2]; } a, o, r;
  a.d = x; o.d = old;
  r.u[0] = __builtin_amdgcn_update_dpp(o.u[0], a.u[0], CTRL, RM, 0xf, false);
  r.u[1] = __builtin_amdgcn_update_dpp(o.u[1], a.u[1], CTRL, RM, 0xf, false);
  return r.d;
}
// lane l: the operation over lanes 0..l  (OP 0: +, 1: min, 2: max; `idn` the operation's identity: what lanes without a
// source take)
#define NKA_WAVE_SCAN(T, DPP)                                                                        \
  x = op(x, DPP<0x111, 0xf>(x, idn)); x = op(x, DPP<0x112, 0xf>(x, idn)); x = op(x, DPP<0x114, 0xf>(x, idn)); \
  x = op(x, DPP<0x118, 0xf>(x, idn)); x = op(x, DPP<0x142, 0xa>(x, idn)); x = op(x, DPP<0x143, 0xc>(x, idn)); \
  return x;
template <int OP> __device__ __forceinline__ float wave_scan_f32(float x, const float idn) {
  auto op = [](float a, float b) { return OP == 0 ? a + b : OP == 1 ? fminf(a, b) : fmaxf(a, b); };
  NKA_WAVE_SCAN(float, dpp_f32)
}
__device__ __forceinline__ int wave_scan_add_i32(int x) {
  auto op = [](int a, int b) { return a + b; };
  const int idn = 0;
  NKA_WAVE_SCAN(int, dpp_i32)
}
__device__ __forceinline__ double wave_scan_add_f64(double x) {
  auto op = [](double a, double b) { return a + b; };
  const double idn = 0.0;
  NKA_WAVE_SCAN(double, dpp_f64)
}
#undef NKA_WAVE_SCAN

// One step of a chain over a FULL block of products without walking it element after element.
// While  2^e <= |a| < 2^(e+1)  every representable neighbour of the running sum is a multiple of u = 2^(e-52), so
// fl(a + p) = u * (S + R(p/u)) with S = |a|/u an integer in [2^52, 2^53) and R the rounding of t = p/u to an integer,
// halves going to whichever neighbour makes S + R EVEN (round-to-nearest-even acts on the sum's significand).  The
// additions of integers are exact and associative; the only thing a step inherits from its predecessors is the PARITY of
// S, and only a halfway case reads it (after which the sum is even whatever it was).  So each lane takes 16 consecutive
// products: r = rne(t) (t + 1.5*2^52 - 1.5*2^52), the halfway flag |t - r| == 0.5, the plain sum of the r's, its own
// parity map and the corrections (+-1) a halfway case owes under either incoming parity; ballots carry the parity from
// lane to lane and one prefix sum places every lane's excursion.  That SUMMARY of a block depends on the running sum only
// through its sign and exponent (chain_block_summary), so the wavefronts of the workgroup take one block each under the
// exponent the group starts with; wavefront 0 then walks the summaries (chain_block_apply): a block is accepted iff it
// was summarised under the sum's present sign and exponent, every prefix provably stays inside the binade and every
// lane's sum of |r| < 2^51 (r exact, lane sums exact; NaN and Inf fail the comparison).  The prefix bounds are kept in SINGLE precision,
// rounded to nearest: they are off by < 2^33 units, and the acceptance window leaves 2^34 units (2^-18 of the binade)
// at either end -- which also covers the corrections (<= 1024) and the one inexact case (sums beyond 2^53 are only ever
// formed in blocks that leave the window by far more than their error).  Otherwise the block is summarised again under
// the present exponent or, failing that, walked (chain_block_serial).  Same bits as the walk by construction;
// tests/test_chain_sums_gpu.py holds the two to each other and to numpy's sequential accumulate on adversarial inputs
// (halfway cases under both parities, binade crossings, cancellation, zeros, subnormals, overflow, NaN).
// what one lane makes of its 16 consecutive products under the scale of the sum's binade
struct ChainLane {
  double base, absl;         // sum of the r's; sum of their magnitudes (< 2^51: every r and every partial sum exact)
  double pmin, pmax;         // least / greatest prefix sum inside the lane, the empty one (0) included
  int par, differ;           // parity of the lane's sum if it starts even; whether starting odd still flips it (no halfway case met)
  int adj0, adj1;            // corrections the halfway cases owe if the lane starts even / odd
};
__device__ __forceinline__ ChainLane chain_lane_pass(const double (&pl)[kChainLaneElems], double scale) {
#pragma clang fp contract(off)
  constexpr double M = 6755399441055744.0;                         // 1.5 * 2^52
  ChainLane ln;
  ln.base = ln.absl = ln.pmin = ln.pmax = 0.0;
  ln.differ = 1; ln.adj0 = ln.adj1 = 0;
  int parw = 0;
  bool halfway = false;
#pragma unroll
  for (int j = 0; j < kChainLaneElems; j++) {
    const double t = pl[j] * scale;                                // exact (a power of two), |t| tiny if it underflows
    const double tm = t + M;                                       // rounds t to an integer, halves to even
    const double r = tm - M;
    const double diff = t - r;                                     // exact
    halfway |= fabs(diff) == 0.5;
    parw ^= __double2loint(tm);
    ln.base = ln.base + r;
    ln.absl = ln.absl + fabs(r);
    ln.pmin = fmin(ln.pmin, ln.base);
    ln.pmax = fmax(ln.pmax, ln.base);
  }
  if (__any(halfway)) {                                            // the parity bookkeeping in its own pass
    parw = 0;
#pragma unroll
    for (int j = 0; j < kChainLaneElems; j++) {
      const double t = pl[j] * scale;
      const double tm = t + M;
      const double diff = t - (tm - M);
      if (fabs(diff) == 0.5) {                                     // halfway: r is the EVEN neighbour of t, r + 2 diff the odd one
        const int tau = diff > 0.0 ? 1 : -1;
        // r being even, S + r has the parity of S: an odd S takes the other neighbour, and the sum is even either way
        if (parw & 1) ln.adj0 += tau;
        if ((parw ^ ln.differ) & 1) ln.adj1 += tau;
        parw = 0; ln.differ = 0;
      } else {
        parw ^= __double2loint(tm);
      }
    }
  }
  ln.par = parw & 1;
  return ln;
}
// the parity each lane starts from if the block starts EVEN (q), and whether a block starting odd flips it (no halfway
// case in any lane before this one)
__device__ __forceinline__ void chain_lane_parity(const ChainLane &ln, int lane, int &q, bool &flips) {
  const unsigned long long T = __ballot(ln.differ == 0), A = __ballot(ln.par);
  const unsigned long long lt = (1ull << lane) - 1ull, Tl = T & lt;
  flips = Tl == 0;
  if (flips) q = __popcll(A & lt) & 1;
  else {
    const int h = 63 - __clzll(Tl);                                // the last lane before this one that met a halfway case
    q = __popcll(A & lt & ~((1ull << h) - 1ull)) & 1;
  }
}

struct ChainSummary {
  double total;              // sum of the r's
  float gmin, gmax;          // least / greatest prefix bound
  int adj;                   // corrections if S starts even (low half) / odd (high half), each biased by kChainAdjBias
  int hi;                    // sign and exponent word the summary assumed; 0: none, or a product out of range
};
constexpr int kChainAdjBias = 64 * kChainLaneElems;
__device__ __forceinline__ bool chain_scalable(double a) {
  const int ef = (__double2hiint(a) >> 20) & 0x7ff;
  return ef >= 1023 - 900 && ef <= 1023 + 900;                    // not zero, subnormal, Inf, NaN; scale factors in range
}
__device__ __forceinline__ ChainSummary chain_block_summary(double a, const double *blk) {
#pragma clang fp contract(off)
  ChainSummary sm;
  sm.hi = 0; sm.total = 0.0; sm.gmin = sm.gmax = 0.f; sm.adj = 0;
  if (!chain_scalable(a)) return sm;
  const int lane = threadIdx.x & 63;
  const int hi = __double2hiint(a);
  const int e = ((hi >> 20) & 0x7ff) - 1023;
  const double scale = __hiloint2double((hi & (int)0x80000000) | ((1023 + 52 - e) << 20), 0);    // +-2^(52-e): S > 0
  double pl[kChainLaneElems];
  chain_lane_read(pl, blk, lane);
  const ChainLane ln = chain_lane_pass(pl, scale);
  const bool bad = !(ln.absl < 0x1p51);                            // some |t| >= 2^51 / Inf / NaN: r = rne(t) and the lane's sums are exact below that
  // where the lane's excursion lies: the prefix before it + its own least / greatest prefix, in single precision
  const float basef = (float)ln.base;
  const float exclf = wave_scan_f32<0>(basef, 0.f) - basef;
  const float lo = wave_scan_f32<1>(exclf + (float)ln.pmin, __builtin_inff());
  const float up = wave_scan_f32<2>(exclf + (float)ln.pmax, -__builtin_inff());
  int q;
  bool flips;
  chain_lane_parity(ln, lane, q, flips);
  const int qo = flips ? q ^ 1 : q;
  const int packed = ((q ? ln.adj1 : ln.adj0) + kChainLaneElems) | (((qo ? ln.adj1 : ln.adj0) + kChainLaneElems) << 16);
  const int adjs = wave_scan_add_i32(packed);
  const double tot = wave_scan_add_f64(ln.base);
  sm.total = readlane_f64(tot, 63);
  sm.gmin = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lo), 63));
  sm.gmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(up), 63));
  sm.adj = __builtin_amdgcn_readlane(adjs, 63);
  sm.hi = __any(bad) ? 0 : (hi & (int)0xfff00000);
  return sm;
}
// The running sum through summarised blocks.  S = |a| / u as long as blocks are accepted (ChainRun); leaving that form
// gives the double back.
struct ChainRun {
  double S, unscale;
  int hi;                    // sign and exponent word of the sum S stands for; 0: none (a is authoritative)
};
__device__ __forceinline__ void chain_run_enter(ChainRun &run, double a) {
  run.hi = 0;
  if (!chain_scalable(a)) return;
  const int hi = __double2hiint(a);
  const int e = ((hi >> 20) & 0x7ff) - 1023;
  const double scale = __hiloint2double((hi & (int)0x80000000) | ((1023 + 52 - e) << 20), 0);
  run.unscale = __hiloint2double((hi & (int)0x80000000) | ((1023 - 52 + e) << 20), 0);
  run.S = a * scale;                                               // exact, an integer in [2^52, 2^53)
  run.hi = hi & (int)0xfff00000;
}
__device__ __forceinline__ bool chain_block_apply(ChainRun &run, const ChainSummary &sm) {
#pragma clang fp contract(off)
  if (sm.hi == 0 || run.hi != sm.hi) return false;
  constexpr double kEdge = 0x1p34;
  if (!(run.S + (double)sm.gmin >= 0x1p52 + kEdge) || !(run.S + (double)sm.gmax <= 0x1p53 - kEdge)) return false;
  const int odd = __double2loint(run.S) & 1;                       // the parity of S: the last bit of the significand
  const int adj = ((odd ? sm.adj >> 16 : sm.adj) & 0xffff) - kChainAdjBias;
  run.S = run.S + (sm.total + (double)adj);
  return true;
}

// The loop of one sum: `load(g0)` brings the operands of the group that starts at element g0 into the caller's registers
// (wavefront w: block w of the group), `store()` rounds their products into the wavefront's block of `prod`.  Returns the
// sum (valid in thread 0).  The whole workgroup calls it.
struct ChainStamps {
#ifdef NKA_CHAIN_STAMPS
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};    // 10 ns ticks of wavefront 0: load issue, summary, wait, apply, wait, store
  unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // blocks: in a run / on their own / summarised again / walked
#endif
};
template <class Load, class Store>
__device__ __forceinline__ double chain_drive(double a, int64_t n, double *prod, ChainSummary *summ, double *sh_a_p, int walk,
                                              ChainStamps &stamps, Load load, Store store) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  double *myblk = prod + wave * kChainBlockLds;
  if (t == 0) *sh_a_p = a;
  if (n > 0) { load(0); store(); }
  __syncthreads();
#ifdef NKA_CHAIN_STAMPS
  unsigned long long tk = wall_clock64(), tn;
#define NKA_CHAIN_STAMP(i) tn = wall_clock64(); stamps.st[i] += tn - tk; tk = tn;
#define NKA_CHAIN_COUNT(i, v) stamps.cnt[i] += (v);
#else
#define NKA_CHAIN_STAMP(i)
#define NKA_CHAIN_COUNT(i, v)
#endif
  for (int64_t g0 = 0; g0 < n; g0 += kChainGroup) {
    const bool more = g0 + kChainGroup < n;
    if (more) load(g0 + kChainGroup);                  // in flight while this group goes through the chain
    NKA_CHAIN_STAMP(0)
    const int glen = (int)(n - g0 < kChainGroup ? n - g0 : kChainGroup);
    const int nfull = glen / kChainBlock, nblk = (glen + kChainBlock - 1) / kChainBlock;
    // every wavefront summarises its block under the sign and exponent the group starts with ...
    const double a0 = *sh_a_p;
    if (wave < nfull && !walk) {
      const ChainSummary sm = chain_block_summary(a0, myblk);
      if (lane == 0) summ[wave] = sm;
    }
    NKA_CHAIN_STAMP(1)
    __syncthreads();
    NKA_CHAIN_STAMP(2)
    // ... and wavefront 0 takes the running sum through them: lane k holds the summary of block k
    if (wave == 0) {
      a = a0;
      ChainRun run;
      chain_run_enter(run, a);
      ChainSummary mine = summ[lane < kChainGroupBlocks ? lane : 0];
      int k = 0;
      while (k < nblk) {
        if (run.hi != 0 && !walk && k < nfull) {
          // every block from k on that applies whatever the parity of the sum: their totals as one prefix sum, each
          // checked against the sum it would start from; the longest run of acceptable blocks goes in at once
          const bool cand = lane >= k && lane < nfull;
          const int ae = (mine.adj & 0xffff) - kChainAdjBias, ao = ((mine.adj >> 16) & 0xffff) - kChainAdjBias;
          const bool usable = cand && mine.hi == run.hi;
          // the parity each block starts from, if every block before it goes in: block i flips it by the parity of its
          // total plus the correction it takes under the parity it meets (a short scalar chain over two bit masks)
          const int tpar = __double2loint(fabs(mine.total) + 0x1p52) & 1;     // (|total| < 2^52 in any block that goes in)
          const unsigned pe = (unsigned)__ballot(usable && ((tpar ^ ae) & 1)), po = (unsigned)__ballot(usable && ((tpar ^ ao) & 1));
          unsigned odd = 0;
          {
            unsigned p = (unsigned)__builtin_amdgcn_readfirstlane(__double2loint(run.S)) & 1u;   // (scalar: the chain runs on the SALU)
            for (int i = k; i < nfull; i++) {
              odd |= p << i;
              p ^= ((p ? po : pe) >> i) & 1u;
            }
          }
          const double tk_ = usable ? mine.total + (double)(((odd >> lane) & 1u) ? ao : ae) : 0.0;
          double incl = tk_;
          incl = incl + dpp_f64<0x111, 0xf>(incl, 0.0);
          incl = incl + dpp_f64<0x112, 0xf>(incl, 0.0);
          incl = incl + dpp_f64<0x114, 0xf>(incl, 0.0);
          const double Sk = run.S + (incl - tk_);
          constexpr double kEdge = 0x1p34;
          const bool ok = usable && (Sk + (double)mine.gmin >= 0x1p52 + kEdge) && (Sk + (double)mine.gmax <= 0x1p53 - kEdge);
          const unsigned long long need = ((1ull << nfull) - 1ull) & ~((1ull << k) - 1ull);
          const unsigned long long failm = need & ~__ballot(ok);
          const int F = failm ? __ffsll((long long)failm) - 1 : nfull;
          if (F > k) {
            run.S = run.S + readlane_f64(incl, F - 1);
            NKA_CHAIN_COUNT(0, F - k)
            k = F;
            continue;
          }
        }
        // block k on its own: under the parity of the sum, or summarised again under its present exponent, or walked
        const double *bk = prod + k * kChainBlockLds;
        const int len = glen - k * kChainBlock < kChainBlock ? glen - k * kChainBlock : kChainBlock;
        bool done = false;
        if (len == kChainBlock && !walk) {
          ChainSummary sm = summ[k];
          done = chain_block_apply(run, sm);
          if (done) { NKA_CHAIN_COUNT(1, 1) }
          if (!done && run.hi != 0 && run.hi != sm.hi) {           // another binade by now: summarise under the present one
            sm = chain_block_summary(run.S * run.unscale, bk);
            done = chain_block_apply(run, sm);
            if (done) { NKA_CHAIN_COUNT(2, 1) }
          }
        }
        if (!done) {
          if (run.hi != 0) a = run.S * run.unscale;
          if (len == kChainBlock && !walk) { NKA_CHAIN_COUNT(3, 1) }
          // (walked whole: accepting its first lanes and taking the rest again under the next exponent was measured -- a
          //  sum that meets an end of its binade hovers there, a round costs what walking 14 lanes costs and gained 5: a loss)
          a = chain_block_serial(a, bk, len);
          chain_run_enter(run, a);
        }
        k++;
      }
      if (run.hi != 0) a = run.S * run.unscale;
      if (t == 0) *sh_a_p = a;
    }
    NKA_CHAIN_STAMP(3)
    __syncthreads();
    NKA_CHAIN_STAMP(4)
    if (more) store();                                 // (each wavefront into its own block, which it alone summarises)
    NKA_CHAIN_STAMP(5)
  }
  return a;
#undef NKA_CHAIN_STAMP
#undef NKA_CHAIN_COUNT
}

// One sum of an update as the chain kernels see it: which vectors, which rounding of their product, where the sum goes.
struct ChainSum {
  int kind, dst;             // kChainKind...; index into red[].  kind < 0: this sum does not exist in this update
  const double *f, *w1, *wk; // f; the pending w (d = w1 - f); the older w of the sum (kinds W1W, FW)
  double s, rs;              // the norm of d and its reciprocal (kinds FW1, W1W)
  int rcp;                   // w1' = (1/s) * d (vector flavour) instead of d / s
  int64_t n;
  bool vec16;                // every base address allows 16-byte loads
};
// sum number b of a launch: set kChainNorm = the norm (b = 0) and, with `with_f`, the sums on f alone (b = 1..ub);
// set kChainRows = <f,w1'> (b = 0), the Gram row on the rounded w1' (b = 1..ub) and, with `with_f`, the sums on f alone
// (b = ub+1..2ub), s from red[0]; set kChainProbe = <f, probe> into red[2 + mvec] (diagnostic entry)
__device__ __forceinline__ ChainSum chain_decode(const Ctl &ctl, const Vecs &vs, const double *f, int rcp, int set, int with_f,
                                                 int ub, int b, const double *probe) {
  ChainSum cs;
  const int pending = ctl.ic[IC_PLAN_PENDING];
  const int nolder = ctl.ic[IC_PLAN_NOLDER];
  const int mvec = ctl.mvec;
  const long long *pw = ctl.plan_w();
  cs.kind = -1; cs.dst = 0;
  cs.f = f; cs.w1 = pending ? vs.w + ctl.pc[PC_FIRST_W] : f; cs.wk = f;
  cs.s = 0.0; cs.rcp = rcp; cs.n = vs.n;
  if (set == kChainProbe) {
    cs.kind = kChainKindFW; cs.dst = 2 + mvec; cs.wk = probe;
  } else if (set == kChainNorm) {
    if (b == 0) {
      if (pending) { cs.kind = kChainKindNorm; cs.dst = 0; }
    } else {
      const int p = b - 1;
      if (with_f && p < nolder) { cs.kind = kChainKindFW; cs.dst = 2 + mvec + p; cs.wk = vs.w + pw[p]; }
    }
  } else {
    if (pending) cs.s = sqrt(ctl.red()[0]);           // the GLOBAL sum d^2 (F08:267)
    const bool normed = pending && cs.s != 0.0;       // (s == 0: the scalar step relaxes, F08:268-275; the w1' sums are dead)
    if (b == 0) {
      if (normed) { cs.kind = kChainKindFW1; cs.dst = 1; }
    } else if (b <= ub) {
      const int k = b - 1;
      if (normed && k < nolder) { cs.kind = kChainKindW1W; cs.dst = 2 + k; cs.wk = vs.w + pw[k]; }
    } else {
      const int p = b - 1 - ub;
      if (with_f && p < nolder) { cs.kind = kChainKindFW; cs.dst = 2 + mvec + p; cs.wk = vs.w + pw[p]; }
    }
  }
  cs.rs = 1.0 / cs.s;
  cs.vec16 = ((reinterpret_cast<uintptr_t>(cs.f) | reinterpret_cast<uintptr_t>(cs.w1) | reinterpret_cast<uintptr_t>(cs.wk)) & 15) == 0;
  return cs;
}
// The operands of one block (1024 elements from e0 on) in a wavefront's registers: pair j*64 + lane of the block per load,
// i.e. 1 KiB per wave instruction ...
constexpr int kChainPairs = kChainLaneElems / 2;       // 16-byte loads per thread and vector
static_assert(kChainPairs == 8, "the pair mapping of chain_load_block / chain_store_block assumes 16 elements per lane");
// xf = f; xb = the SECOND operand of the kind -- the older w (kind FW) or the pending w1 (every other kind); xc = the older w
// of kind W1W.  (Round 6: three arrays named after the vectors, each written under its own branch, made the compiler sink the
// stores of two branches into one store through a pointer phi -- the arrays then lived partly in scratch, 48-80 bytes per
// lane in k_chain_sums / k_chain_blocks / k_chain_apply.  One destination per load, the ADDRESS selected instead.)
struct ChainBlockRegs {
  typename VecT<2>::type xf[kChainPairs], xb[kChainPairs], xc[kChainPairs];
};
__device__ __forceinline__ void chain_load_block(const ChainSum &cs, ChainBlockRegs &r, int64_t e0, int lane, bool full) {
  using V2 = typename VecT<2>::type;
  const int64_t n = cs.n;
  const bool vec16 = cs.vec16;
  auto ldpair = [&](const double *p, int64_t i) -> V2 {
    V2 v;
    if (full && vec16) v = *reinterpret_cast<const V2 *>(p + i);
    else if (full) { v.x = p[i]; v.y = p[i + 1]; }
    else { v.x = i < n ? p[i] : 0.0; v.y = i + 1 < n ? p[i + 1] : 0.0; }
    return v;
  };
  const int64_t i0 = e0 + 2 * lane;
  const double *const second = cs.kind == kChainKindFW ? cs.wk : cs.w1;
#pragma unroll
  for (int j = 0; j < kChainPairs; j++) { r.xf[j] = ldpair(cs.f, i0 + j * 128); r.xb[j] = ldpair(second, i0 + j * 128); }
  if (cs.kind == kChainKindW1W) {
#pragma unroll
    for (int j = 0; j < kChainPairs; j++) r.xc[j] = ldpair(cs.wk, i0 + j * 128);
  }
}
// ... and their rounded products where the lane that owns them reads them (blk: the block's kChainBlockLds doubles of LDS)
__device__ __forceinline__ void chain_store_block(const ChainSum &cs, const ChainBlockRegs &r, double *blk, int lane) {
#pragma clang fp contract(off)      // products and additions stay separate roundings whatever the build's flags
  using V2 = typename VecT<2>::type;
  const double s = cs.s, rs = cs.rs;
#pragma unroll
  for (int j = 0; j < kChainPairs; j++) {
    V2 p;
    if (cs.kind == kChainKindFW) { p.x = r.xf[j].x * r.xb[j].x; p.y = r.xf[j].y * r.xb[j].y; }
    else {
      const double d0 = r.xb[j].x - r.xf[j].x, d1 = r.xb[j].y - r.xf[j].y;   // F08:266 ((-1)*f + w1 in F08V:237: same bits)
      if (cs.kind == kChainKindNorm) { p.x = d0 * d0; p.y = d1 * d1; }
      else {
        const double n0 = cs.rcp ? rs * d0 : d0 / s, n1 = cs.rcp ? rs * d1 : d1 / s;   // the value PB stores as w1' (F08:283; F08V:256)
        if (cs.kind == kChainKindFW1) { p.x = r.xf[j].x * n0; p.y = r.xf[j].y * n1; }
        else { p.x = n0 * r.xc[j].x; p.y = n1 * r.xc[j].y; }
      }
    }
    // pair j*64 + lane of the block = elements 2 (j*64 + lane), +1: lane (j*64 + lane) / 8 of the chain, pair row lane % 8
    *reinterpret_cast<V2 *>(blk + (lane % kChainPairs) * kChainRow + 2 * (j * (64 / kChainPairs) + lane / kChainPairs)) = p;
  }
}

}  // namespace nka
