// nka_batch_kernel.hpp -- k_batch_update, the one kernel of the narrow batch (one workgroup per system), and the members of its
// trailing pack.  Private to nka_amd/csrc: nka_batch.hip (the instances every narrow batch launches, the host entries) and
// nka_batch_rows.hip (the instances with the scalar step on wavefront 0, a unit of their own for the build's sake) include it,
// each behind nka_batch_dev.hpp and `using namespace nka`.  The phases are described at the head of nka_batch.hip.
#pragma once

#include "nka_batch_dev.hpp"

#include <cstdint>
#include <type_traits>

namespace {
using namespace nka;

// what a solve step takes beside the update's arguments; each pointer may be NULL (a workgroup-uniform branch, not an instance)
struct StepArgs {
  double *x;            // iterate rows, ldx apart: x = fl(x - f_out) where the system updates
  int64_t ldx;
  const double *tol;    // r <= tol[sys]: the system retires itself (active[sys] = 0) and nothing else of it is written
  double *fnorm;        // r = sqrt(dp(f, f)) of every system active on entry
};
// PER-SYSTEM LENGTHS (nka_hip_batch_set_lengths): the batch's buffer of nsys validated lengths, 1 <= len[sys] <= vlen.  It stands
// behind the StepArgs if there is one, so an instance without it keeps its arguments.
struct LenArgs {
  const int32_t *len;
};
// BINARY32 STORAGE (nka_hip_batch_create_stored): the two pending buffers, nsys binary64 rows at the slot stride (Store32Args,
// nka_batch_dev.hpp).  It stands behind the StepArgs and the LenArgs if there are any, so an instance without it keeps its
// arguments.
// THE SCALAR STEP ON WAVEFRONT 0 (nka_hip_batch_create_rows with nka_hip_batch_set_scalar_step): an empty member, the LAST of the
// pack; NLMAX: the rows batch_scalar_step_rows<NLMAX> holds in registers, >= mvec + 1 (nka_host::batch_rows_nlmax)
template <int NLMAX> struct BatchRows {};
template <class T> struct batch_rows_of { static constexpr int value = 0; };
template <int NLMAX> struct batch_rows_of<BatchRows<NLMAX>> { static constexpr int value = NLMAX; };
template <class... Pack> constexpr int batch_rows_nl = (0 + ... + batch_rows_of<Pack>::value);
// (a member of the pack is taken by its type: pack_get, nka_batch_dev.hpp)

// (where the pieces of a system lie, and the LDS of a workgroup -- 5.3 KB at mvec = 20, 11.2 KB at 32: host_logic.hpp)
static_assert(nka_host::batch_lds(NKA_HIP_BATCH_MAX_MVEC).bytes() <= 40 * 1024, "four workgroups of a batch must fit the LDS of a CU");
// ... with the wavefront step: the matrix behind the working copy, 9.2 KB at mvec = 20 and 20.5 KB at 32 -- still four workgroups
// per CU by LDS, and no function attribute
static_assert(nka_host::batch_rows_lds(NKA_HIP_BATCH_MAX_MVEC).bytes() <= 40 * 1024, "... and four workgroups with the wavefront step");
static_assert(nka_host::batch_rows_nlmax(NKA_HIP_BATCH_MAX_MVEC) == nka_host::kWideRowsMaxList && NKA_HIP_BATCH_MAX_MVEC + 1 <= nka_host::kWideRowsMaxList,
              "the wavefront step holds every list a batch can have");


// WGT = true: the diagonal weights of nka_hip_batch_set_dot_weights.  Row `sys` of the batch's weight buffer -- wgt_all +
// sys * wgt_stride, wgt_stride = 0 for the form all systems share -- is read like a stored vector, and fl(w_i * a_i) is the
// FIRST operand of every product (nka_device.hpp, DIAGONAL WEIGHTS); element -> thread map, per-thread order and reduction
// are those of WGT = false, which reads neither argument and is the unweighted kernel instruction for instruction.
// Step...: nothing (the update) or one StepArgs (the solve step, above); a step writes active[sys] = 0 when the system retires.
// A trailing LenArgs makes n = len[sys] -- one uniform scalar load at entry -- the length of EVERY phase: the ordered chains, the
// sweeps, the step's dp(f, f) and x -= f_out, the weight loads.  Nothing at an index >= len[sys] of f, x, the weight row or a slot
// is read or written; the element -> thread map and the per-thread order do not depend on n, so the system carries the bits of
// a batch created with vlen = len[sys].  Without it the instance is the one it was, instruction for instruction.
// A trailing Store32Args makes the instance one of BINARY32 STORAGE (COMB = 2 and the fast sums only): a.w / a.v are float
// allocations of the same strides in elements, an older pair is one 8-byte load widened exactly, the raw pending pair is read
// from and written to the binary64 rows pw / pv, and the normalised pair is narrowed once -- w1' = q(fl(d/s)) in phases 3 and 6
// alike, v = q(fl(fl(v1/s) - w1')) -- before it is used or stored, so the sums, the combine and the slot hold the same values.
// Element -> thread map, per-thread order, sweeps, block sums and the scalar step are those of every other instance.  Without
// it every such statement is discarded at compile time and the instance is the one it was, instruction for instruction.
// A trailing BatchRows<NLMAX> -- the LAST member, empty -- makes phase 4 batch_scalar_step_rows<NLMAX> on wavefront 0 (fast sums
// only) with the matrix of nka_host::batch_rows_lds behind the working copy; every other phase is the one it was, and so is
// every instance without the member, instruction for instruction: 96 instances (32 fast packs x 11 / 21 / 33 rows, compiled by
// nka_batch_rows.hip), none with scratch or a vector-register spill.
template <int COMB, bool ORDERED, bool WGT, class... Step>
__global__ __launch_bounds__(kBatchThreads) void k_batch_update(BatchArgs a, double *__restrict__ f_all, int64_t ld,
                                                                const int32_t *__restrict__ active,
                                                                const double *__restrict__ wgt_all, int64_t wgt_stride, Step... step) {
#pragma clang fp contract(off)      // elementwise statements and the reference-order sums round like the reference; fma is explicit
  constexpr bool STEP = (std::is_same<Step, StepArgs>::value || ...);
  constexpr bool LEN = (std::is_same<Step, LenArgs>::value || ...);
  constexpr bool S32 = (std::is_same<Step, Store32Args>::value || ...);
  constexpr int ROWS = batch_rows_nl<Step...>;      // > 0: phase 4 on wavefront 0 (batch_scalar_step_rows<ROWS>), the matrix in LDS
  static_assert(sizeof...(Step) == (STEP ? 1 : 0) + (LEN ? 1 : 0) + (S32 ? 1 : 0) + (ROWS > 0 ? 1 : 0),
                "at most one StepArgs, then at most one LenArgs, then at most one Store32Args, then at most one BatchRows<NLMAX>");
  static_assert(!S32 || (COMB == 2 && !ORDERED), "binary32 storage: the default flavour and the fast sums only");
  static_assert(ROWS == 0 || !ORDERED, "the wavefront step: the fast sums only");
  constexpr int NNRM = STEP ? 2 : 1;             // sums of phase 2: [<f,f>,] <d,d>, landing in res[kBatchAcc + 1 - NNRM ...]
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  const int sys = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;      // phase 0: nothing of this system is read or written

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nh = (m1 + 1) * (m1 + 1);
  const int64_t n = [&]() -> int64_t {
    if constexpr (LEN) return pack_get<LenArgs>(step...).len[sys]; else return a.n;      // (validated when it was set: 1 <= len[sys] <= a.n)
  }();
  const Ctl ctl = batch_ctl(a, sys);
  double *const f = f_all + (size_t)sys * ld;
  double *const W = a.w + (size_t)sys * a.sys_stride, *const V = a.v + (size_t)sys * a.sys_stride;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;      // (stored vectors: always 16-byte aligned)
  const double *wg = nullptr;                                        // this system's weights (rows: 16-byte aligned)
  if constexpr (WGT) wg = wgt_all + (size_t)sys * wgt_stride;
  [[maybe_unused]] float *W32 = nullptr, *V32 = nullptr;      // binary32 storage: this system's slots ...
  [[maybe_unused]] double *pw = nullptr, *pv = nullptr;       // ... and its rows of the pending buffers (16-byte aligned)
  if constexpr (S32) {
    W32 = reinterpret_cast<float *>(a.w) + (size_t)sys * a.sys_stride;
    V32 = reinterpret_cast<float *>(a.v) + (size_t)sys * a.sys_stride;
    pw = pack_get<Store32Args>(step...).pw + (size_t)sys * a.stride;
    pv = pack_get<Store32Args>(step...).pv + (size_t)sys * a.stride;
  }

  const nka_host::BatchLds lds = nka_host::batch_lds(mvec);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  Lst L;
  L.h = shd + lds.h;
  L.c = shd + lds.c;
  double *const red = shd + lds.red;
  double *const cc = shd + lds.cc;           // combine plan: coefficients in list order (slots: cs)
  double *const sm = shd + lds.sm;
  double *const res = shd + lds.res;
  L.next = shi + lds.next;
  L.prev = shi + lds.prev;
  int32_t *const ps = shi + lds.ps;          // older list entries at entry, in list order
  int32_t *const cs = shi + lds.cs;
  int32_t *const hdr = shi + lds.hdr;
  L.m1 = m1;
  L.mvec = mvec;

  // ---- phase 1: the working copy ----
  for (int i = t; i < nh; i += kBatchThreads) L.h[i] = ctl.h()[i];
  for (int i = t; i < m1 + 1; i += kBatchThreads) {
    L.c[i] = ctl.c()[i];
    L.next[i] = ctl.next()[i];
    L.prev[i] = ctl.prev()[i];
  }
  for (int i = t; i < 2 + 2 * mvec; i += kBatchThreads) red[i] = 0.0;      // an update rewrites every entry
  L.subspace = L.pending = L.first = L.last = L.free_ = 0;
  L.vtol = 0.0;
  __syncthreads();
  if (t == 0) {
    lst_load_scalars(L, ctl);
    L.vtol = ctl.dc[DC_VTOL];
    int no = 0;
    for (int k = L.pending ? L.next[L.first] : L.first; k != 0 && no < m1; k = L.next[k]) ps[no++] = k;
    hdr[HDR_PENDING] = L.pending;
    hdr[HDR_FIRST] = L.first;
    hdr[HDR_NOLDER] = no;
  }
  __syncthreads();
  const int pending = hdr[HDR_PENDING], nolder = hdr[HDR_NOLDER];
  const double *const w1 = pending ? (S32 ? pw : W + (size_t)(hdr[HDR_FIRST] - 1) * a.stride) : f;      // (binary32 storage: the pending row)
  const double *const w1s = S32 ? pw : pending ? w1 : W;      // always a stored (16-byte aligned) vector: for loads whose value may go unused

  // ---- phase 2: the norm (F08:266-267) ----
  double s = 0.0;
  if constexpr (STEP && ORDERED)
    if (t == 64) {      // dp(f, f), one chain, on a wavefront of its own: beside thread 0's chain where there is a pending pair
      double ff = 0.0;
#pragma unroll 4      // (the loads of four elements in flight; the additions stay one chain)
      for (int64_t i = 0; i < n; i++) {
        if constexpr (WGT) ff = ff + (wg[i] * f[i]) * f[i]; else ff = ff + f[i] * f[i];
      }
      res[kBatchAcc - 1] = ff;
    }
  if (pending) {
    if (ORDERED) {
      if (t == 0) {
        double dd = 0.0;
        for (int64_t i = 0; i < n; i++) {
          const double d = w1[i] - f[i];
          if constexpr (WGT) dd = dd + (wg[i] * d) * d; else dd = dd + d * d;
        }
        res[kBatchAcc] = dd;
      }
      __syncthreads();
    } else {
      double acc[NNRM] = {};
      batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
        constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
        const d2 fv = ld_tile<FULL, FV>(f, i, n), wv = ld_tile<FULL, true>(w1, i, n);
        d2 gv;
        if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
        for (int q = 0; q < 2; q++)
          if (FULL || i + q < n) {
            const double d = wv[q] - fv[q];
            if constexpr (WGT) acc[NNRM - 1] = fma(gv[q] * d, d, acc[NNRM - 1]); else acc[NNRM - 1] = fma(d, d, acc[NNRM - 1]);
            if constexpr (STEP) acc[0] = fma(WGT ? gv[q] * fv[q] : fv[q], fv[q], acc[0]);
          }
      });
      batch_block_sum<NNRM>(acc, sm, res + kBatchAcc + 1 - NNRM);
    }
    s = sqrt(res[kBatchAcc]);
    if (t == 0) red[0] = res[kBatchAcc];
  } else if constexpr (STEP) {      // no pending pair (first update, after a restart): f is swept alone
    if (ORDERED) {
      __syncthreads();      // (thread 64's chain)
    } else {
      double acc[1] = {0.0};
      batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
        constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
        const d2 fv = ld_tile<FULL, FV>(f, i, n);
        d2 gv;
        if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
        for (int q = 0; q < 2; q++)
          if (FULL || i + q < n) acc[0] = fma(WGT ? gv[q] * fv[q] : fv[q], fv[q], acc[0]);
      });
      batch_block_sum<1>(acc, sm, res + kBatchAcc - 1);
    }
  }
  // ---- STEP: the residual norm and the stop rule.  r comes from LDS behind a barrier and tol[sys] is written by nobody, so the
  // return is uniform across the workgroup; nothing but LDS has been written so far ----
  [[maybe_unused]] double *xrow = nullptr;      // this system's row of the iterate, if there is one
  [[maybe_unused]] bool xvec = false;
  if constexpr (STEP) {
    const StepArgs &st = pack_get<StepArgs>(step...);
    const double r = sqrt(res[kBatchAcc - 1]);
    if (t == 0 && st.fnorm != nullptr) st.fnorm[sys] = r;
    if (st.tol != nullptr && r <= st.tol[sys]) {      // (a NaN on either side: false, the system goes on)
      if (t == 0) const_cast<int32_t *>(active)[sys] = 0;
      return;
    }
    if (st.x != nullptr) {
      xrow = st.x + (size_t)sys * st.ldx;
      xvec = (reinterpret_cast<uintptr_t>(xrow) % 16) == 0;
    }
  }
  const bool normed = pending && s != 0.0;      // (s == 0: the scalar step relaxes, F08:275; NaN: goes on, like the reference)
  const double rs = 1.0 / s;

  // ---- phase 3: every other sum, on the rounded w1' (F08:286-290, 371) ----
  if (ORDERED) {
    // thread r <= nolder: r = 0 <f,w1'>, else <w1',w_(r-1)> (only if normed); thread 64 + p: <f,w_p>
    if (normed && t <= nolder) {
      const double *y = t == 0 ? f : W + (size_t)(ps[t - 1] - 1) * a.stride;
      double acc = 0.0;
      for (int64_t i = 0; i < n; i++) {
        const double wn = batch_nrm<RCP>(w1[i] - f[i], s, rs);
        if constexpr (WGT) acc = t == 0 ? acc + (wg[i] * y[i]) * wn : acc + (wg[i] * wn) * y[i];      // dp(f, w1'), dp(w1', w_p)
        else acc = acc + wn * y[i];
      }
      red[t == 0 ? 1 : 2 + (t - 1)] = acc;
    } else if (t >= 64 && t - 64 < nolder) {
      const double *y = W + (size_t)(ps[t - 64] - 1) * a.stride;
      double acc = 0.0;
      for (int64_t i = 0; i < n; i++) {
        if constexpr (WGT) acc = acc + (wg[i] * f[i]) * y[i]; else acc = acc + f[i] * y[i];
      }
      red[2 + mvec + (t - 64)] = acc;
    }
  } else {
    const int ngroup = (nolder + kBatchGroup - 1) / kBatchGroup;
    for (int g = 0; g < (ngroup > 0 ? ngroup : (normed ? 1 : 0)); g++) {
      const double *wk[kBatchGroup];
      [[maybe_unused]] const float *wk32[kBatchGroup];
#pragma unroll
      for (int j = 0; j < kBatchGroup; j++) {
        const int p = g * kBatchGroup + j;
        if constexpr (S32) wk32[j] = W32 + (nolder > 0 ? (size_t)(ps[p < nolder ? p : nolder - 1] - 1) * a.stride : (size_t)0);
        else wk[j] = nolder > 0 ? W + (size_t)(ps[p < nolder ? p : nolder - 1] - 1) * a.stride : w1s;   // (beyond the list: a re-read, discarded)
      }
      double acc[kBatchAcc];
#pragma unroll
      for (int q = 0; q < kBatchAcc; q++) acc[q] = 0.0;
      batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
        constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
        const d2 fv = ld_tile<FULL, FV>(f, i, n);
        const d2 dv = ld_tile<FULL, true>(w1s, i, n);     // (no pending pair: a stored vector whose value is not used)
        d2 wv[kBatchGroup];
#pragma unroll
        for (int j = 0; j < kBatchGroup; j++) {
          if constexpr (S32) wv[j] = ld_tile32<FULL>(wk32[j], i, n); else wv[j] = ld_tile<FULL, true>(wk[j], i, n);
        }
        d2 gv;
        if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
        for (int q = 0; q < 2; q++)
          if (FULL || i + q < n) {
            const double fq = fv[q];
            double fa = fq;                                  // first operand of the products on f: fl(w f), formed once
            if constexpr (WGT) fa = gv[q] * fq;
            if (normed) {
              double wn = batch_nrm<RCP>(dv[q] - fq, s, rs);
              if constexpr (S32) wn = batch_q32(wn);         // (binary32 storage: the value the slot will hold)
              double wa = wn;                               // first operand of the Gram row: fl(w w1')
              if constexpr (WGT) wa = gv[q] * wn;
              if (g == 0) acc[2 * kBatchGroup] = fma(fa, wn, acc[2 * kBatchGroup]);
#pragma unroll
              for (int j = 0; j < kBatchGroup; j++) acc[j] = fma(wa, wv[j][q], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < kBatchGroup; j++) acc[kBatchGroup + j] = fma(fa, wv[j][q], acc[kBatchGroup + j]);
          }
      });
      batch_block_sum<kBatchAcc>(acc, sm, res);
      if (t < kBatchGroup && g * kBatchGroup + t < nolder) {
        if (normed) red[2 + g * kBatchGroup + t] = res[t];
        red[2 + mvec + g * kBatchGroup + t] = res[kBatchGroup + t];
      }
      if (t == 0 && g == 0 && normed) red[1] = res[2 * kBatchGroup];
      // (res is rewritten only behind the two barriers of the next batch_block_sum)
    }
  }
  __syncthreads();

  // ---- phase 4: the scalar step, the statements of k_solve on this system's working copy ----
  if constexpr (ROWS > 0) {
    // wavefront 0, all 64 lanes (a wavefront-uniform branch; wavefronts 1-3 go on to the barrier below).  L's scalars are valid in
    // lane 0, which loaded them in phase 1; s is uniform (every thread read res[kBatchAcc]); ps and red[] are complete behind the
    // barrier above; the function has no workgroup barrier.  The matrix: behind the working copy (nka_host::batch_rows_lds)
    if (t < 64) batch_scalar_step_rows<ROWS>(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr, reinterpret_cast<double *>(smem + nka_host::batch_rows_lds(mvec).a_off));
  } else if (t == 0) {
    // (the statements of batch_scalar_step, nka_batch_dev.hpp, written out: as a call they moved registers of kernels held to
    // their machine code)
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
  __syncthreads();

  // ---- phase 5: the working copy back ----
  for (int i = t; i < nh; i += kBatchThreads) ctl.h()[i] = L.h[i];
  for (int i = t; i < m1 + 1; i += kBatchThreads) {
    ctl.c()[i] = L.c[i];
    ctl.next()[i] = L.next[i];
    ctl.prev()[i] = L.prev[i];
  }
  for (int i = t; i < 2 + 2 * mvec; i += kBatchThreads) ctl.red()[i] = red[i];

  // ---- phase 6: normalise the pending pair, combine, ring stores (F08:282-283, 361, 395-404) ----
  const int ncomb = hdr[HDR_NCOMB];
  const bool norm0 = hdr[HDR_NORMED] != 0;      // pair 0 of the plan is the pending pair, still raw
  double *const wnew = S32 ? pw : W + (size_t)(hdr[HDR_NEW] - 1) * a.stride, *const vnew = S32 ? pv : V + (size_t)(hdr[HDR_NEW] - 1) * a.stride;
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    if (!FULL && i >= n) return;
    const d2 fin = ld_tile<FULL, FV>(f, i, n);
    d2 x = fin;
    // STEP: the iterate's pair, loaded with the other loads of the tile -- in reference order (validation speed) only where it
    // is used, so that it holds no register across the combine: 60 VGPR like the plain instances, not 66
    [[maybe_unused]] d2 xit = {0.0, 0.0};
    if constexpr (STEP && !ORDERED)
      if (xrow != nullptr) xit = xvec ? ld_tile<FULL, true>(xrow, i, n) : ld_tile<FULL, false>(xrow, i, n);
    int j0 = 0;
    if constexpr (S32) {
      if (norm0) {      // pair 0 of the plan: raw in the pending rows; narrowed once, applied and stored as narrowed
        const size_t off = (size_t)(cs[0] - 1) * a.stride;
        d2 wv = ld_tile<FULL, true>(pw, i, n), vv = ld_tile<FULL, true>(pv, i, n);
        const double c = cc[0];
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const double wn = batch_q32(batch_nrm<RCP>(wv[q] - fin[q], s, rs));
          const double vn = batch_nrm<RCP>(vv[q], s, rs);
          wv[q] = wn;
          vv[q] = batch_q32(vn - wn);
          x[q] = x[q] + c * vv[q];
        }
        st_tile32<FULL>(W32 + off, i, n, wv);
        st_tile32<FULL>(V32 + off, i, n, vv);
        j0 = 1;
      }
    } else if (norm0) {      // pair 0 of the plan: the pending pair, still raw (F08:282-283)
      double *const wk = W + (size_t)(cs[0] - 1) * a.stride, *const vk = V + (size_t)(cs[0] - 1) * a.stride;
      d2 wv = ld_tile<FULL, true>(wk, i, n), vv = ld_tile<FULL, true>(vk, i, n);
      const double c = cc[0];
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const double wn = batch_nrm<RCP>(wv[q] - fin[q], s, rs);
        const double vn = batch_nrm<RCP>(vv[q], s, rs);
        wv[q] = wn;
        vv[q] = COMPACT ? vn - wn : vn;
        x[q] = COMPACT ? x[q] + c * vv[q] : comb1<COMB>(x[q], c, wv[q], vv[q]);
      }
      st_tile<FULL, true>(wk, i, n, wv);
      st_tile<FULL, true>(vk, i, n, vv);
      j0 = 1;
    }
    constexpr int U = 4;      // pairs whose loads are in flight together (beyond the plan: the last pair again, not applied)
    for (int j = j0; j < ncomb; j += U) {
      d2 wv[U], vv[U];
      double c[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int jj = j + u < ncomb ? j + u : ncomb - 1;
        const size_t off = (size_t)(cs[jj] - 1) * a.stride;
        c[u] = cc[jj];
        if constexpr (S32) vv[u] = ld_tile32<FULL>(V32 + off, i, n); else vv[u] = ld_tile<FULL, true>(V + off, i, n);
        if (!COMPACT) wv[u] = ld_tile<FULL, true>(W + off, i, n); else wv[u] = vv[u];
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (j + u < ncomb) {
#pragma unroll
          for (int q = 0; q < 2; q++) x[q] = COMPACT ? x[q] + c[u] * vv[u][q] : comb1<COMB>(x[q], c[u], wv[u][q], vv[u][q]);
        }
    }
    st_tile<FULL, true>(wnew, i, n, fin);
    st_tile<FULL, true>(vnew, i, n, x);
    if (ncomb > 0) st_tile<FULL, FV>(f, i, n, x);      // (nothing to combine: f stays as it is)
    if constexpr (STEP)
      if (xrow != nullptr) {
        if constexpr (ORDERED) xit = xvec ? ld_tile<FULL, true>(xrow, i, n) : ld_tile<FULL, false>(xrow, i, n);
        xit[0] = xit[0] - x[0];
        xit[1] = xit[1] - x[1];
        if (xvec) st_tile<FULL, true>(xrow, i, n, xit); else st_tile<FULL, false>(xrow, i, n, xit);
      }
  });
}

}  // namespace
