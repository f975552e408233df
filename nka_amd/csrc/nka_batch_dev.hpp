// nka_batch_dev.hpp -- what the two translation units of the batched accelerator share: nka_batch.hip (one workgroup per
// system, one launch per update) and nka_batch_wide.hip (a system split across workgroups, four launches per update).  The
// launch arguments, the loads and stores of a tile, the sweep over a span of elements, the fixed-order sums of a workgroup,
// the scalar step on a working copy, and the handle.  The device functions and BatchArgs sit in an unnamed namespace, as they
// did in nka_batch.hip: each unit compiles its own copy of the same text, and the kernels of nka_batch.hip keep their names.
#pragma once
#include "handles.hpp"
#include "nka_device.hpp"
#include "../../include/nka_hip_batch.h"

#include <cstdint>
#include <type_traits>

namespace {

using namespace nka;
using nka_host::kBatchAcc;
using nka_host::kBatchGroup;
using nka_host::kBatchWaves;
constexpr int kBatchThreads = 64 * kBatchWaves;
constexpr int kBatchTile = 2 * kBatchThreads;   // elements per sweep step: thread t owns 2t, 2t+1

struct BatchArgs {
  double *w, *v;        // system sys, slot k (1-based) at base + sys*sys_stride + (k-1)*stride
  int32_t *ic;          // control blocks in the layout of Ctl (nka_ctl.hpp), ic_stride / dc_stride apart
  double *dc;
  int64_t stride, sys_stride, n;
  int32_t ic_stride, dc_stride, mvec, nsys;
};

__host__ __device__ inline Ctl batch_ctl(const BatchArgs &a, int sys) {
  Ctl c{};
  c.ic = a.ic + (size_t)sys * a.ic_stride;
  c.dc = a.dc + (size_t)sys * a.dc_stride;
  c.mvec = a.mvec;
  return c;
}

// pair (i, i+1) of a vector of n elements, i even; beyond n: zeros (never accumulated, never stored)
__device__ __forceinline__ d2 ld_pair(const double *__restrict__ p, int64_t i, int64_t n, bool vec) {
  if (vec && i + 1 < n) return *reinterpret_cast<const d2 *>(p + i);
  d2 r;
  r[0] = i < n ? p[i] : 0.0;
  r[1] = i + 1 < n ? p[i + 1] : 0.0;
  return r;
}
__device__ __forceinline__ void st_pair(double *__restrict__ p, int64_t i, int64_t n, bool vec, d2 x) {
  if (vec && i + 1 < n) {
    *reinterpret_cast<d2 *>(p + i) = x;
    return;
  }
  if (i < n) p[i] = x[0];
  if (i + 1 < n) p[i + 1] = x[1];
}

// The same inside a FULL tile (no element beyond n): straight-line code, so that every load of a tile is in flight before
// the first is waited for; VEC = false (a row of f that is not 16-byte aligned): two 8-byte loads, the same values.
template <bool FULL, bool VEC>
__device__ __forceinline__ d2 ld_tile(const double *__restrict__ p, int64_t i, int64_t n) {
  if (!FULL) return ld_pair(p, i, n, VEC);
  if (VEC) return *reinterpret_cast<const d2 *>(p + i);
  d2 r;
  r[0] = p[i];
  r[1] = p[i + 1];
  return r;
}
template <bool FULL, bool VEC>
__device__ __forceinline__ void st_tile(double *__restrict__ p, int64_t i, int64_t n, d2 x) {
  if (!FULL) { st_pair(p, i, n, VEC, x); return; }
  if (VEC) { *reinterpret_cast<d2 *>(p + i) = x; return; }
  p[i] = x[0];
  p[i + 1] = x[1];
}
// BINARY32 STORAGE (nka_hip_batch.h, STORAGE): the same pair of a stored binary32 vector, one 8-byte access (rows start on 128
// bytes, i is even), widened exactly on the way in and narrowed on the way out -- round to nearest even, subnormals kept,
// beyond the range +-Inf -- so that what is stored is what a later load returns.
typedef float f2 __attribute__((ext_vector_type(2)));
template <bool FULL>
__device__ __forceinline__ d2 ld_tile32(const float *__restrict__ p, int64_t i, int64_t n) {
  d2 r;
  if (FULL || i + 1 < n) {
    const f2 x = *reinterpret_cast<const f2 *>(p + i);
    r[0] = (double)x[0];
    r[1] = (double)x[1];
    return r;
  }
  r[0] = i < n ? (double)p[i] : 0.0;
  r[1] = 0.0;
  return r;
}
template <bool FULL>
__device__ __forceinline__ void st_tile32(float *__restrict__ p, int64_t i, int64_t n, d2 x) {
  f2 y;
  y[0] = (float)x[0];
  y[1] = (float)x[1];
  if (FULL || i + 1 < n) { *reinterpret_cast<f2 *>(p + i) = y; return; }
  if (i < n) p[i] = y[0];
}
// q(x) of the STORAGE paragraph: the binary64 value a binary32 slot returns for x
__device__ __forceinline__ double batch_q32(double x) { return (double)(float)x; }

// One sweep over a system's elements: body(FULL, FVEC, i) for this thread's pair i = 2t, 2t + 512, ... -- the full tiles
// first, then the ragged one with guards.  The order in which a thread meets its elements is the same on every path.
template <class Body>
__device__ __forceinline__ void batch_sweep(int64_t n, bool fvec, Body body) {
  using T = std::true_type;
  using F = std::false_type;
  int64_t base = 0;
  if (fvec) for (; base + kBatchTile <= n; base += kBatchTile) body(T{}, T{}, base + 2 * threadIdx.x);
  else for (; base + kBatchTile <= n; base += kBatchTile) body(T{}, F{}, base + 2 * threadIdx.x);
  if (base < n) {
    if (fvec) body(F{}, T{}, base + 2 * threadIdx.x); else body(F{}, F{}, base + 2 * threadIdx.x);
  }
}

// the value PB stores as w1' (nka_device.hpp: pa_operand with `normed`)
template <bool RCP> __device__ __forceinline__ double batch_nrm(double x, double s, double rs) { return RCP ? rs * x : x / s; }

// Sums of NACC per-thread accumulators over the workgroup in a fixed order: lanes by the butterfly of wave_sum, then
// wavefronts 0, 1, 2, 3.  Result a in res[a] (LDS), valid after the trailing barrier.
template <int NACC>
__device__ __forceinline__ void batch_block_sum(const double (&acc)[NACC], double *sm, double *res) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < NACC; a++) {
    const double x = wave_sum(acc[a]);
    if (lane == 0) sm[wv * NACC + a] = x;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double r = sm[threadIdx.x];
#pragma unroll
    for (int q = 1; q < kBatchWaves; q++) r += sm[q * NACC + threadIdx.x];
    res[threadIdx.x] = r;
  }
  __syncthreads();
}

// MEMBERS OF A TRAILING PACK (k_waves_update of nka_batch_waves.hip, the four kernels of nka_batch_wide.hip: what an instance takes
// beside the update's arguments, so that an instance without a member keeps its arguments).  The batch's weight buffer and its row
// stride (0: the form all systems share): two kernel arguments, not a struct of two -- a pointer inside a struct cannot be
// __restrict__, and without it the weighted instances are scheduled differently
using WgtRows = const double *__restrict__;
enum class WgtStride : int64_t {};
// BINARY32 STORAGE (nka_hip_batch_create_stored, nka_hip_batch_create_wide_stored): the two pending buffers, nsys binary64 rows at
// the slot stride.  In k_batch_update (nka_batch.hip) the LAST member of the trailing pack; in the wide kernels ahead of the weights
struct Store32Args {
  double *pw, *pv;
};
// the T of pack...
template <class T, class First, class... Rest>
__host__ __device__ __forceinline__ const T &pack_get(const First &first, const Rest &...rest) {
  if constexpr (std::is_same<T, First>::value) return first; else return pack_get<T>(rest...);
}

enum { HDR_PENDING = 0, HDR_FIRST = 1, HDR_NOLDER = 2, HDR_NCOMB = 3, HDR_NEW = 4, HDR_NORMED = 5 };

// THE SCALAR STEP of one system, the statements of k_solve on the working copy L (one thread): s == 0 relaxes (F08:275), the
// Gram row of w1' and the factor, the right-hand side and the solve, the combine plan (cs, cc: slots and coefficients in list
// order), the new slot at the head of the list.  ps: the nolder older entries at entry, in list order; red: the system's
// sums.  Writes the five list scalars, DC_S and the plan's header to the control block.
__device__ __forceinline__ void batch_scalar_step(Lst &L, const Ctl &ctl, double s, int nolder, int mvec, const int32_t *ps,
                                                  const double *red, int32_t *cs, double *cc, int32_t *hdr) {
  const int entry_first = L.first;
  bool nrm = false;
  int nrelax = ctl.ic[IC_NRELAX];
  if (L.pending) {
    ctl.dc[DC_S] = s;
    if (s == 0.0) {                       // F08:275
      lst_relax(L);
      nrelax++;
    }
  }
  if (L.pending) {
    nrm = true;
    for (int p = 0; p < nolder; p++) L.H(L.first, ps[p]) = red[2 + p];      // Gram row of w1' (F08:286-290)
    lst_factor(L);
  }
  const int slot = L.free_;
  L.free_ = L.next[slot];
  int ncomb = 0;
  if (L.subspace) {
    if (nrm) L.c[entry_first] = red[1];
    for (int p = 0; p < nolder; p++) L.c[ps[p]] = red[2 + mvec + p];
    lst_solve(L);
    for (int k = L.first; k != 0; k = L.next[k]) {
      cs[ncomb] = k;
      cc[ncomb] = L.c[k];
      ncomb++;
    }
  }
  lst_prepend(L, slot);
  hdr[HDR_NCOMB] = ncomb;
  hdr[HDR_NEW] = slot;
  hdr[HDR_NORMED] = nrm ? 1 : 0;
  lst_store_scalars(L, ctl);
  ctl.ic[IC_NEW] = slot;
  ctl.ic[IC_NCOMB] = ncomb;
  ctl.ic[IC_NORMED] = nrm ? 1 : 0;
  ctl.ic[IC_NRELAX] = nrelax;
}

// one lane's LDS traffic ordered against the other lanes' of the SAME wavefront: the LDS serves a wavefront's instructions in the
// order they were issued, so what is left is to keep the compiler from moving an access across this point (wave_sync of
// nka_batch_waves.hip: a release fence, wave_barrier, an acquire fence, all at wavefront scope)
__device__ __forceinline__ void batch_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// THE SAME SCALAR STEP ON ONE WAVEFRONT (nka_hip_batch.h, SCALAR STEP): called by ALL 64 LANES of one wavefront on a working copy
// in LDS; L's scalars need be valid in lane 0 only (they are broadcast), s, nolder, mvec and every pointer are uniform.  What it
// leaves -- L.h, L.c, the links, the five scalars, cs, cc, hdr and the control-block words -- is BIT FOR BIT what
// batch_scalar_step leaves on the same inputs.  Wavefront-level means only (batch_wave_sync, readlane): no __syncthreads().
//   The algorithm is phases 0-3 of k_solve_rows (nka_kernels.hpp): lane p holds row p of the position-indexed Gram matrix in
// 2 NLMAX registers (NLMAX >= 1 + nolder), the right-hand side rides along as row nl, the Cholesky is right-looking -- at column i
// the pivot of position i is final, the column is scaled by one division a lane and every trailing entry (p, q) gets a(p,q) -=
// l_p l_q with l_q by v_readlane -- so every entry receives the subtractions of lst_factor's inner loop in the same order and then
// the same division; the back-substitution is column-oriented in the same way.  ~m sequential steps instead of ~m^3 / 3.
//   What the lone handle's kernel does not do and the one-thread step does -- nka_hip_batch_get_state and _state_digest cover
// all of h and c, so the debris is part of the contract:
//   * a DEPENDENCE-DROPPED row k is stored: lst_factor writes H(k, j) for every kept j ahead of k before it decides, and never
//     H(k, k); the row of the CAPACITY-DROPPED entry is not touched at all;
//   * c[ps[p]] = red[2 + mvec + p] is written RAW for every older entry, dropped ones too; only kept entries are overwritten by
//     the substitutions (row nl holds partially updated values at dropped positions: they never reach c);
//   * H(first, ps[p]) = red[2 + p] for every p < nolder;
//   * the drops replay in list order (capacity F08:303-307, dependence F08:331-340, each pushed on the head of the free list);
//     the pivot test is hkk > vtol * vtol, a NaN compares false and drops; after a dependence drop the last position of a full
//     list is evaluated by its pivot (kept + 1 > mvec is lst_factor's nvec > mvec).
//   Without a new pair (no pending pair, or s == 0, which relaxes) there is nothing to factor: lane 0 runs batch_scalar_step
// itself under a wavefront-uniform branch.  A: LDS scratch of (m1 + 1) x (m1 + 1) doubles, rows LDA = m1 + 1 apart (the factor by
// position for the column reads of the back-substitution, row nl the forward-substituted right-hand side; the last word takes
// what must not reach h).
template <int NLMAX>
__device__ __forceinline__ void batch_scalar_step_rows(Lst &L, const Ctl &ctl, double s, int nolder, int mvec, const int32_t *ps,
                                                       const double *red, int32_t *cs, double *cc, int32_t *hdr, double *A) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  L.pending = __builtin_amdgcn_readfirstlane(L.pending);
  if (!(L.pending && s != 0.0)) {      // (uniform) the rare paths: bit-equal by construction
    if (lane == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);
    return;
  }
  L.subspace = __builtin_amdgcn_readfirstlane(L.subspace);
  L.first = __builtin_amdgcn_readfirstlane(L.first);
  L.last = __builtin_amdgcn_readfirstlane(L.last);
  L.free_ = __builtin_amdgcn_readfirstlane(L.free_);
  L.vtol = readlane_f64(L.vtol, 0);
  const int NL = L.m1, LDA = NL + 1;
  const int entry_first = L.first;
  const int nl = 1 + nolder;      // the list at entry: the pending entry, then ps[0 ... nolder - 1]; nl <= m1 <= NLMAX
  const double vtol2 = L.vtol * L.vtol;
  // ---- phase 0: the Gram row of w1' (F08:286-290) and the raw right-hand sides (F08:371), every older entry
  if (lane == 0) {
    ctl.dc[DC_S] = s;
    L.H(entry_first, entry_first) = 1.0;      // F08:295
    L.c[entry_first] = red[1];
  }
  if (lane < nolder) {
    L.H(entry_first, ps[lane]) = red[2 + lane];
    L.c[ps[lane]] = red[2 + mvec + lane];
  }
  const int myord = lane == 0 ? entry_first : (lane <= nolder ? ps[lane - 1] : 0);      // slot of list position `lane`
  batch_wave_sync();
  const uint64_t listmask = (1ull << nl) - 1;      // (nl <= 33)
  uint64_t alive = listmask;
  int capdrop = -1;
  double ddr = 1.0;    // lane p: running pivot 1 - sum l^2 of list position p
  double Ldr = 1.0;    // lane p: accepted pivot sqrt(hkk)
  // ---- phase 1: right-looking Cholesky with drops (F08:295-347) on rows 0 ... nl - 1, the right-hand side as row nl
  double a[NLMAX];
#pragma unroll
  for (int q = 0; q < NLMAX; q++) {
    const int oq = __builtin_amdgcn_readlane(myord, q);      // slot of list position q (0 beyond the list)
    a[q] = (lane < nl) ? L.H(oq, myord)                      // raw <w_q, w_p>, q newer (used for q < p only)
                       : L.c[oq];                            // row nl: <f, w_q>
  }
  int kept = 0;
  bool open_ = true;      // false once the capacity drop has ended the list (F08:309)
#pragma unroll
  for (int i = 0; i < NLMAX; i++) {      // (constant trip counts, guards instead of break: both loops unroll completely)
    bool keep = false;
    double Lii = 1.0;
    if (open_ && i < nl) {
      if (i == 0) {
        keep = true;
      } else if (kept + 1 > mvec) {
        capdrop = i;      // F08:301-308: i is the last entry
        open_ = false;
      } else {
        const double hkk = readlane_f64(ddr, i);
        keep = hkk > vtol2;      // F08:326
        if (keep) Lii = sqrt(hkk);
      }
      if (!keep) alive &= ~(1ull << i);
    }
    if (keep) {
      kept++;
      if (lane == i) Ldr = Lii;
      const double l = a[i] / Lii;      // F08:320 (row nl: F08:377); rows <= i: unused
      a[i] = l;
      if (lane > i && lane < nl) ddr = ddr - l * l;      // F08:321
#pragma unroll
      for (int q = i + 1; q < NLMAX; q++) a[q] = a[q] - l * readlane_f64(l, q);      // F08:317 (row nl: F08:374)
    }
  }
  // ---- phase 2: the rows back by slot -- of a kept AND of a dependence-dropped position its entries at the kept columns ahead
  // of it, of the capacity-dropped position nothing --, and by position into A; the drops in list order
  {
    double *const dump = A + NL * LDA + NL;
    const bool stored = lane < nl && lane != capdrop;
    const uint64_t rowbits = stored ? (alive & ((1ull << lane) - 1)) : 0ull;
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
    if (lane >= 1 && lane < nl && ((alive >> lane) & 1)) L.H(myord, myord) = Ldr;      // F08:327 (position 0: the 1.0 above)
  }
  batch_wave_sync();
  double yr = 0.0;      // lane p: forward-substituted right-hand side, then the solution, of list position p
  if (lane < nl) yr = A[nl * LDA + lane];
  for (uint64_t dm = ~alive & listmask; dm != 0; dm &= dm - 1) {      // (every lane, the same values)
    const int p = __builtin_ctzll(dm);
    const int k = __builtin_amdgcn_readlane(myord, p);
    if (p == capdrop) {      // F08:303-307
      L.next[L.last] = L.free_;
      L.free_ = k;
      L.last = L.prev[k];
      L.next[L.last] = 0;
    } else {                 // F08:331-340
      const int pv = L.prev[k], nx = L.next[k];
      L.next[pv] = nx;
      if (nx == 0) L.last = pv; else L.prev[nx] = pv;
      L.next[k] = L.free_;
      L.free_ = k;
    }
  }
  L.subspace = 1;
  L.pending = 0;
  // ---- phase 3: the new slot; the back-substitution (F08:382-392) by columns; the plan
  const int slot = L.free_;      // F08:357-358
  L.free_ = L.next[slot];
  {
    double t[NLMAX];      // column `lane` of the factor (rows / lanes beyond the list fold onto row / column nl: values nobody uses)
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
  }
  const int ncomb = __builtin_popcountll(alive);
  if (lane < nl && ((alive >> lane) & 1)) {
    const int r = __builtin_popcountll(alive & ((1ull << lane) - 1));      // position among the kept entries
    cs[r] = myord;
    cc[r] = yr;
    L.c[myord] = yr;
  }
  lst_prepend(L, slot);      // F08:406-417 (every lane, the same values)
  if (lane == 0) {
    hdr[HDR_NCOMB] = ncomb;
    hdr[HDR_NEW] = slot;
    hdr[HDR_NORMED] = 1;
    lst_store_scalars(L, ctl);
    ctl.ic[IC_NEW] = slot;
    ctl.ic[IC_NCOMB] = ncomb;
    ctl.ic[IC_NORMED] = 1;      // (IC_NRELAX: batch_scalar_step writes back the value it read)
  }
}

}  // namespace

struct nka_hip_batch_state {
  int device = 0;
  hipStream_t stream = nullptr;
  int flavor = NKA_HIP_FLAVOR_C;
  int sum_order = NKA_HIP_SUMS_AUTO;
  double vtol = 0.01;
  BatchArgs k{};
  // diagonal dot-product weights (nka_hip_batch_set_dot_weights): nsys rows at the slot stride, allocated at the first set,
  // freed at destroy only and never moved -- a captured update holds the address.  The form all systems share lives in row 0.
  double *wgt = nullptr;
  double *wgt_stage = nullptr;              // the same shape: where the host entry puts the caller's rows for the check
  unsigned long long *wgt_chk = nullptr;    // two words of k_batch_check_weights
  bool weighted = false;
  int64_t wgt_stride = 0;                   // row stride the updates run with: k.stride, or 0 in the shared form
  // per-system lengths (nka_hip_batch_set_lengths): nsys int32, allocated at the first set, freed at destroy only and never
  // moved -- a captured update holds the address.  It only ever holds values that passed the check 1 <= len <= vlen.
  int32_t *len = nullptr;
  bool has_len = false;                     // the next update runs the instances that read it
  // binary32 storage (nka_hip_batch_create_stored): k.w / k.v then point at FLOAT allocations of the same strides in elements,
  // and the raw pending pair lives in pend_w / pend_v, nsys binary64 rows at the slot stride, allocated at creation, freed at
  // destroy only and never moved -- a captured update holds the addresses
  int storage = NKA_HIP_BATCH_STORE_F64;
  double *pend_w = nullptr, *pend_v = nullptr;
  int64_t vector_bytes = 0;                 // what the slots and the pending buffers asked of hipMalloc
  // a WIDE batch (nka_hip_batch_create_wide, nka_batch_wide.hip): a system is nchunk chunks of NKA_HIP_BATCH_WIDE_CHUNK elements
  bool wide = false;
  int32_t nchunk = 0;
  double *part = nullptr;                   // partial sums, nka_host::wide_part_index: nsys x (2 + 2 mvec) x nchunk
  double *plan_c = nullptr;                 // the combine plan from the scalar kernel to the combine: nsys x (mvec + 1) coefficients
  int32_t *plan_s = nullptr;                //   ... and slots, in list order (the control block's comb_c / comb_slots stay zero)
  // ... with the solve step (nka_hip_batch_create_wide_step, the same unit): the partials of <f,f>,
  // nka_host::wide_fpart_index: nsys x nchunk, allocated at creation, freed at destroy only and never moved
  bool wide_step = false;
  double *fpart = nullptr;
  // a LANE batch (nka_hip_batch_create_lanes, nka_batch_lanes.hip): one lane per system, lanes_group systems per workgroup; k.w
  // and k.v then hold the interleaved slots of nka_host::lanes_slot_offset (k.stride and k.sys_stride are not used)
  bool lanes = false;
  int32_t lanes_group = 0;
  // a WAVE batch (nka_hip_batch_create_waves, nka_batch_waves.hip): one wavefront per system; storage and control blocks are the
  // narrow batch's, nothing further is allocated
  bool waves = false;
  // ... of nka_hip_batch_create_waves_ext: the same batch, which also takes lengths and weights (the same unit and kernel)
  bool waves_ext = false;
  // ... of nka_hip_batch_create_waves_rows: a batch of either entry above (waves_ext = its `ext`) that offers the scalar step on the
  // whole wavefront; mvec is at most nka_host::waves_rows_max_mvec().  Until scalar_step below says so it launches what they launch
  bool waves_rows = false;
  // a WIDE batch of nka_hip_batch_create_wide_ext: the same batch, which also takes weights (the weighted instances of the norm and
  // the sums kernel of nka_batch_wide.hip); with wide_step as its `step` argument says.  A batch of
  // nka_hip_batch_create_wide_stored is such a batch whose `storage` may be NKA_HIP_BATCH_STORE_F32 (the binary32 instances of the
  // sums, the scalar and the combine kernel; the norm kernels read the pending rows through their BatchArgs)
  bool wide_ext = false;
  // a NARROW batch of nka_hip_batch_create_rows: the batch of nka_hip_batch_create / _create_stored (as `storage` says) that offers
  // the scalar step on wavefront 0 of a system's workgroup; nothing further is allocated.  Until scalar_step below says so it
  // launches what they launch
  bool narrow_rows = false;
  // how a wide batch runs its third launch, and a wave batch of nka_hip_batch_create_waves_rows and a narrow batch of
  // nka_hip_batch_create_rows phase 4 of their one launch
  // (nka_hip_batch_set_scalar_step): enqueue-side state only, read when a call is enqueued
  int scalar_step = NKA_HIP_BATCH_SCALAR_ONE_THREAD;
};

// nka_batch_wide.hip: the buffers of a wide batch (b->k is complete), and one update of it -- four launches on b->stream, the first
// two of them the weighted instances where b->weighted (a batch of nka_hip_batch_create_wide_ext, b->wide_ext)
int nka_batch_wide_alloc(nka_hip_batch_t b);
void nka_batch_wide_free(nka_hip_batch_t b);
void nka_batch_wide_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active);
// ... the same unit: the one buffer the solve step of a wide batch adds (b->nchunk is set), and one step -- the same four launches
int nka_batch_wide_step_alloc(nka_hip_batch_t b);
void nka_batch_wide_step_free(nka_hip_batch_t b);
void nka_batch_wide_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                         double *fnorm);
// nka_batch_lanes.hip: the slots of a lane batch (b->k.n, mvec, nsys are set; sets k.w, k.v, lanes_group and vector_bytes), one
// update and one solve step of it -- one launch each on b->stream --, and slot `slot` of system `sys` gathered to the host
int nka_batch_lanes_alloc(nka_hip_batch_t b);
void nka_batch_lanes_free(nka_hip_batch_t b);
void nka_batch_lanes_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active);
void nka_batch_lanes_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                          double *fnorm);
int nka_batch_lanes_get_slot(nka_hip_batch_t b, bool v, int32_t sys, int32_t slot, double *host_out);
// nka_batch_waves.hip: one update and one solve step of a wave batch -- one launch each on b->stream --, with the weights
// (b->weighted) and the lengths (b->has_len) that a batch of nka_hip_batch_create_waves_ext (b->waves_ext) may have set
void nka_batch_waves_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active);
void nka_batch_waves_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                          double *fnorm);
// nka_batch_rows.hip: one update and one solve step of a narrow batch of nka_hip_batch_create_rows (b->narrow_rows) while
// b->scalar_step is NKA_HIP_BATCH_SCALAR_WAVEFRONT -- one launch each on b->stream, the instance of k_batch_update (nka_batch_kernel.hpp)
// with the scalar step on wavefront 0, with the flavour, the storage, the weights and the lengths the batch has; fast sums only
void nka_batch_rows_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active);
void nka_batch_rows_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                         double *fnorm);
