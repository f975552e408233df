// nka_batch_waves.hip -- the WAVE batch of include/nka_hip_batch.h (nka_hip_batch_create_waves, nka_hip_batch_create_waves_ext):
// ONE WAVEFRONT PER SYSTEM, four systems per workgroup, for systems between the lane batch (vlen <= 64) and the lengths at which
// the narrow batch (nka_batch.hip: a workgroup of 256 threads per system) fills its tiles.  Wavefront w of workgroup g owns system
// 4 g + w through every phase; the storage, the control blocks and every host entry are the narrow batch's.
//   0 skip      sys >= nsys or active[sys] == 0: the wavefront returns before any byte of the system is read or written
//   1 load      h, c and the links into the wavefront's working copy in LDS, all lanes; lane 0 lists the older entries (the list
//               length is read HERE, on the device: graphs from the first update)
//   2 norm      sum d^2, d = fl(w1 - f) [, sum f^2 in the same sweep: the step]; s = sqrt          -- a step may retire here
//   3 sums      on the ROUNDED w1' = batch_nrm<RCP>(d, s, 1/s): <f,w1'>, <w1',w_p>, <f,w_p>, kBatchGroup older vectors per sweep,
//               kBatchAcc accumulators; red[] zeros as in the narrow kernel
//   4 scalar    lane 0: batch_scalar_step (nka_batch_dev.hpp) on the wavefront's copy -- or, in the instances with a WavesRows
//               member (THE SCALAR STEP ON THE WAVEFRONT below), all 64 lanes: batch_scalar_step_rows, the same bits
//   5 store     the copy and red[] back to the control block, all lanes
//   6 combine   normalise the pending pair, combine in list order with comb1<COMB> (compact storage in flavour C),
//               w_new = f_in, v_new = f_out, f [, x = fl(x - f_out)]; four pairs' loads in flight
// SYNCHRONISATION: design 1 of the two the kind allows -- NO __syncthreads() ANYWHERE.  A wavefront never touches another
// wavefront's copy or another system's memory, so nothing orders wavefronts against each other, and a wavefront that is masked,
// retired or absent returns on its own while its three neighbours go on.  Inside a wavefront the LDS serves the instructions of
// the wavefront in the order they were issued; what is left is to keep the COMPILER from moving an LDS access of one lane across
// the point where another lane's access must have been issued: wave_sync() below -- a release fence, wave_barrier, an acquire
// fence, all at wavefront scope; no instruction beyond the waits the fences imply.  It stands wherever one lane writes LDS that
// another lane of the same wavefront reads (after the load, after lane 0's list walk, around the scalar step).  Global memory:
// every element of f, x and the slots is read and written by ONE lane in all phases (pair 2l, 2l + 1 of every tile), and the
// control block is read before it is written.  No flags, no spinning, no atomics, no cooperative launch.
// THE WAVE SUM.  A tile is kWavesTile = 128 elements; lane l owns the pair 2l, 2l + 1 of every tile and meets its pairs in
// increasing order on every path (full tiles: straight-line code, every load of the tile issued before the first wait; the ragged
// last tile: guarded).  A sum is two fma per lane and tile into the lane's accumulator, then the six-level butterfly of wave_sum
// (nka_device.hpp: x += x[lane + off], off = 32, 16, 8, 4, 2, 1, through registers), valid in lane 0.  Hence the longest chain of
// roundings that reaches the result:
//       waves_k(n) = 2 * ceil(n / 128) + 6                                                     (nka_host::waves_k)
// A row of f or x that is 16-byte aligned is read with 16-byte accesses, any other with two 8-byte accesses of the same pair;
// stored vectors are always 16-byte accesses.  The bits therefore depend on the system's own values alone: not on nsys, on the
// position or the wavefront the system lands on, on its neighbours, on ld / ldx or on the alignment of a row.  They are NOT the
// narrow batch's bits (its tile is 512 elements over 256 threads, plus three cross-wavefront additions): the contract is the
// numerical one of NKA_HIP_SUMS_BLOCKED_ROUNDED.
// ONE KERNEL, 24 INSTANCES (and 4 x 24 more with the scalar step on the wavefront, below): 3 flavours x {update, step} x {plain, weights, lengths, both}.  What an instance takes beside the
// update's arguments rides in the trailing pack (below), so an instance without a member keeps its arguments; a batch of
// nka_hip_batch_create_waves can set neither lengths nor weights and runs the plain instances only.
//   LENGTHS  A trailing LenArgs makes n = len[sys] -- one uniform load behind the `active` test -- the length of EVERY phase: the
//            sweeps, the step's <f,f> and x -= f_out, the weight loads.  Lane l owns the pair 2l, 2l + 1 of every 128-element tile
//            and meets its pairs in increasing order whatever n is, and the butterfly does not depend on n: the system carries the
//            bits of a wave batch created with vlen = len[sys], and nothing at an index >= len[sys] of f, x, the weight row or a
//            slot is read or written.
//   WEIGHTS  A leading WgtRows, WgtStride: row `sys` of the batch's weight buffer -- rows + sys * stride, 0 for the form all
//            systems share -- is read like a stored vector (16-byte aligned rows at the slot stride) in phases 2 and 3, and
//            fl(w_i a_i) is the FIRST operand of every product, the narrow batch's table: red[0] fma(fl(w d), d, .), red[1]
//            fma(fl(w f), w1', .), red[2+p] fma(fl(w w1'), w_p, .), red[2+m+p] fma(fl(w f), w_p, .), the step's <f,f>
//            fma(fl(w f), f, .); fl(w f) is formed once per element and sweep.  Phase 6 does not read the weights.  The chain of
//            roundings behind the first operand is the unweighted one: waves_k(n) stands.
// THE SCALAR STEP ON THE WAVEFRONT (nka_hip_batch_create_waves_rows, nka_hip_batch_set_scalar_step).  A trailing, empty
// WavesRows<NLMAX> -- the LAST member of the pack -- makes phase 4 batch_scalar_step_rows<NLMAX> (nka_batch_dev.hpp) on all 64
// lanes of the system's own wavefront: about mvec sequential steps instead of lane 0's O(mvec^3) chain, and bit for bit what lane
// 0 leaves, debris included.  It is built from wavefront-level means only, so nothing of SYNCHRONISATION changes: no workgroup
// barrier, a masked, retired or absent system's wavefront still returns before it touches LDS.  One more wave_sync() stands
// AHEAD of phase 4: in phase 3 lane 0 alone writes red[], and the rows step reads red[2 + lane] and ps[lane] in the other lanes.
// The LDS is nka_host::waves_rows_lds: the same copy, then the wavefront's matrix of (mvec + 2)^2 doubles, four times; the launch
// asks for that size and every other launch for exactly what it asked before.  Instance and size are chosen when a call is
// enqueued, so a captured call keeps both.  NLMAX by classes of mvec, 6 / 11 / 21 / cap + 1 rows (nka_host::waves_rows_nlmax); the
// cap on mvec, nka_host::waves_rows_max_mvec(), is where four copies and four matrices still fit 64 KiB.
#include "nka_batch_dev.hpp"

#include <cstdint>
#include <string>
#include <type_traits>

using namespace nka;

namespace {

using nka_host::kWavesGroup;
using nka_host::kWavesTile;
constexpr int kWavesThreads = 64 * kWavesGroup;

static_assert(kWavesGroup == kBatchWaves && kWavesThreads == kBatchThreads, "a workgroup is four wavefronts");
static_assert(kWavesTile == 2 * 64, "lane l owns the pair 2l, 2l + 1 of a tile");
static_assert(nka_host::waves_lds(NKA_HIP_BATCH_MAX_MVEC).bytes() <= 64 * 1024, "dynamic LDS a launch may ask for without an attribute");
static_assert(nka_host::waves_rows_lds(nka_host::waves_rows_max_mvec()).bytes() <= nka_host::kWavesRowsLdsLimit &&
                  nka_host::waves_rows_lds(nka_host::waves_rows_max_mvec() + 1).bytes() > nka_host::kWavesRowsLdsLimit &&
                  nka_host::waves_rows_max_mvec() >= 1 && nka_host::waves_rows_max_mvec() <= NKA_HIP_BATCH_MAX_MVEC,
              "... with the wavefront step: the cap on mvec is the last that fits without a function attribute");
static_assert(nka_host::waves_rows_max_mvec() + 1 <= nka_host::kWideRowsMaxList && nka_host::waves_rows_max_mvec() + 1 > 21,
              "the wavefront step holds every list such a batch can have (its masks are 64 bits, its lists at most 33 long)");
static_assert(NKA_HIP_BATCH_WAVES_MAX_VLEN <= NKA_HIP_BATCH_MAX_VLEN && NKA_HIP_BATCH_WAVES_MAX_VLEN % kWavesTile == 0,
              "the cap is whole tiles, inside the narrow batch's range (the storage is the narrow batch's)");

// THE TRAILING PACK of k_waves_update: [WgtRows, WgtStride][, StepArgs][, LenArgs][, WavesRows<NLMAX>], each at most once, in this order.
// WgtRows, WgtStride (nka_batch_dev.hpp): the batch's weight buffer and its row stride, the FIRST members
// what a solve step takes beside the update's arguments (the StepArgs of nka_batch.hip); each pointer may be NULL
struct StepArgs {
  double *x;
  int64_t ldx;
  const double *tol;
  double *fnorm;
};
// the batch's buffer of nsys validated lengths, 1 <= len[sys] <= vlen (the LenArgs of nka_batch.hip): the LAST member of the pack
// but for a WavesRows
struct LenArgs {
  const int32_t *len;
};
// THE SCALAR STEP ON THE WAVEFRONT (the head comment): an empty member, the LAST of the pack; NLMAX: the rows
// batch_scalar_step_rows<NLMAX> holds in registers, >= mvec + 1 (nka_host::waves_rows_nlmax)
template <int NLMAX> struct WavesRows {};
template <class T> struct waves_rows_of { static constexpr int value = 0; };
template <int NLMAX> struct waves_rows_of<WavesRows<NLMAX>> { static constexpr int value = NLMAX; };
template <class... Pack> constexpr int waves_rows_nl = (0 + ... + waves_rows_of<Pack>::value);      // 0: lane 0 alone
// LDS of an instance: with the matrices of the wavefront step where ROWS (host_logic.hpp)
template <bool ROWS> __host__ __device__ constexpr auto waves_layout(int mvec) {
  if constexpr (ROWS) return nka_host::waves_rows_lds(mvec); else return nka_host::waves_lds(mvec);
}

// one lane's LDS traffic ordered against the other lanes' of the SAME wavefront (the head comment, SYNCHRONISATION)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum over the wavefront, in every lane (wave_sum leaves it in lane 0)
__device__ __forceinline__ double wave_sum_all(double x) { return readlane_f64(wave_sum(x), 0); }

// One sweep over a system's elements at wavefront width: body(FULL, FVEC, i) for this lane's pair i = 2l, 2l + 128, ... -- the full
// tiles first, then the ragged one with guards (batch_sweep of nka_batch_dev.hpp with a tile of 128).
template <class Body>
__device__ __forceinline__ void waves_sweep(int64_t n, bool fvec, int lane, Body body) {
  using T = std::true_type;
  using F = std::false_type;
  int64_t base = 0;
  if (fvec) for (; base + kWavesTile <= n; base += kWavesTile) body(T{}, T{}, base + 2 * lane);
  else for (; base + kWavesTile <= n; base += kWavesTile) body(T{}, F{}, base + 2 * lane);
  if (base < n) {
    if (fvec) body(F{}, T{}, base + 2 * lane); else body(F{}, F{}, base + 2 * lane);
  }
}

// Pack...: the trailing pack above; a step writes active[sys] = 0 when the system retires.
template <int COMB, class... Pack>
__global__ __launch_bounds__(kWavesThreads) void k_waves_update(BatchArgs a, double *__restrict__ f_all, int64_t ld,
                                                                const int32_t *__restrict__ active, Pack... pack) {
#pragma clang fp contract(off)      // elementwise statements round like the reference; fma is explicit
  constexpr bool WGT = (std::is_same<Pack, WgtRows>::value || ...);
  constexpr bool STEP = (std::is_same<Pack, StepArgs>::value || ...);
  constexpr bool LEN = (std::is_same<Pack, LenArgs>::value || ...);
  constexpr int ROWS = waves_rows_nl<Pack...>;      // > 0: phase 4 on all 64 lanes (batch_scalar_step_rows<ROWS>), the matrix in LDS
  static_assert(WGT == (std::is_same<Pack, WgtStride>::value || ...) &&
                    sizeof...(Pack) == (WGT ? 2 : 0) + (STEP ? 1 : 0) + (LEN ? 1 : 0) + (ROWS > 0 ? 1 : 0),
                "at most one WgtRows with its WgtStride, then at most one StepArgs, then at most one LenArgs, then at most one WavesRows");
  constexpr int NNRM = STEP ? 2 : 1;      // sums of phase 2: [<f,f>,] <d,d>
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: addresses of the system in scalar registers)
  const int64_t sys = (int64_t)blockIdx.x * kWavesGroup + wv;
  // ---- phase 0: an absent or a masked system; the wavefront leaves alone ----
  if (sys >= a.nsys) return;
  if (active != nullptr && active[sys] == 0) return;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int mvec = a.mvec, m1 = mvec + 1, nh = (m1 + 1) * (m1 + 1);
  const int64_t n = [&]() -> int64_t {
    if constexpr (LEN) return pack_get<LenArgs>(pack...).len[sys]; else return a.n;      // (validated when it was set: 1 <= len[sys] <= a.n)
  }();
  const Ctl ctl = batch_ctl(a, (int)sys);
  double *const f = f_all + (size_t)sys * (size_t)ld;
  double *const W = a.w + (size_t)sys * (size_t)a.sys_stride, *const V = a.v + (size_t)sys * (size_t)a.sys_stride;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;      // (stored vectors: always 16-byte aligned)
  [[maybe_unused]] const double *wg = nullptr;                       // this system's weights (rows: 16-byte aligned)
  if constexpr (WGT) wg = pack_get<WgtRows>(pack...) + (size_t)sys * (size_t)pack_get<WgtStride>(pack...);

  const auto wl = waves_layout<(ROWS > 0)>(mvec);
  const nka_host::BatchLds &lds = wl.copy;
  double *const shd = reinterpret_cast<double *>(smem + wl.base(wv));      // this wavefront's working copy
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  Lst L;
  L.h = shd + lds.h;
  L.c = shd + lds.c;
  double *const red = shd + lds.red;
  double *const cc = shd + lds.cc;           // combine plan: coefficients in list order (slots: cs)
  L.next = shi + lds.next;
  L.prev = shi + lds.prev;
  int32_t *const ps = shi + lds.ps;          // older list entries at entry, in list order
  int32_t *const cs = shi + lds.cs;
  int32_t *const hdr = shi + lds.hdr;
  L.m1 = m1;
  L.mvec = mvec;

  // ---- phase 1: the working copy ----
  for (int i = lane; i < nh; i += 64) L.h[i] = ctl.h()[i];
  for (int i = lane; i < m1 + 1; i += 64) {
    L.c[i] = ctl.c()[i];
    L.next[i] = ctl.next()[i];
    L.prev[i] = ctl.prev()[i];
  }
  for (int i = lane; i < 2 + 2 * mvec; i += 64) red[i] = 0.0;      // an update rewrites every entry
  L.subspace = L.pending = L.first = L.last = L.free_ = 0;
  L.vtol = 0.0;
  wave_sync();
  if (lane == 0) {
    lst_load_scalars(L, ctl);
    L.vtol = ctl.dc[DC_VTOL];
    int no = 0;
    for (int k = L.pending ? L.next[L.first] : L.first; k != 0 && no < m1; k = L.next[k]) ps[no++] = k;
    hdr[HDR_PENDING] = L.pending;
    hdr[HDR_FIRST] = L.first;
    hdr[HDR_NOLDER] = no;
  }
  wave_sync();
  const int pending = hdr[HDR_PENDING], nolder = hdr[HDR_NOLDER];
  const double *const w1 = pending ? W + (size_t)(hdr[HDR_FIRST] - 1) * a.stride : W;      // (no pending pair: loaded, never used)

  // ---- phase 2: the norm (F08:266-267), and the step's residual norm ----
  double s = 0.0;
  [[maybe_unused]] double ff = 0.0;
  if (pending) {
    double acc[NNRM] = {};
    waves_sweep(n, fvec, lane, [&](auto full, auto fv_, int64_t i) {
      constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
      const d2 fv = ld_tile<FULL, FV>(f, i, n), wv_ = ld_tile<FULL, true>(w1, i, n);
      [[maybe_unused]] d2 gv;
      if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double d = wv_[q] - fv[q];
          if constexpr (WGT) acc[NNRM - 1] = fma(gv[q] * d, d, acc[NNRM - 1]); else acc[NNRM - 1] = fma(d, d, acc[NNRM - 1]);
          if constexpr (STEP) {
            if constexpr (WGT) acc[0] = fma(gv[q] * fv[q], fv[q], acc[0]); else acc[0] = fma(fv[q], fv[q], acc[0]);
          }
        }
    });
    const double dd = wave_sum_all(acc[NNRM - 1]);
    if constexpr (STEP) ff = wave_sum_all(acc[0]);
    s = sqrt(dd);
    if (lane == 0) red[0] = dd;
  } else if constexpr (STEP) {      // no pending pair (first update, after a restart): f is swept alone, the same chain
    double acc = 0.0;
    waves_sweep(n, fvec, lane, [&](auto full, auto fv_, int64_t i) {
      constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
      const d2 fv = ld_tile<FULL, FV>(f, i, n);
      [[maybe_unused]] d2 gv;
      if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);      // (the weights ride along)
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          if constexpr (WGT) acc = fma(gv[q] * fv[q], fv[q], acc); else acc = fma(fv[q], fv[q], acc);
        }
    });
    ff = wave_sum_all(acc);
  }
  // ---- STEP: the residual norm and the stop rule.  r is the same value in every lane and tol[sys] is written by nobody, so the
  // wavefront leaves as one; nothing but its own LDS has been written so far ----
  [[maybe_unused]] double *xrow = nullptr;      // this system's row of the iterate, if there is one
  [[maybe_unused]] bool xvec = false;
  if constexpr (STEP) {
    const StepArgs &st = pack_get<StepArgs>(pack...);
    const double r = sqrt(ff);
    if (lane == 0 && st.fnorm != nullptr) st.fnorm[sys] = r;
    if (st.tol != nullptr && r <= st.tol[sys]) {      // (a NaN on either side: false, the system goes on)
      if (lane == 0) const_cast<int32_t *>(active)[sys] = 0;
      return;
    }
    if (st.x != nullptr) {
      xrow = st.x + (size_t)sys * (size_t)st.ldx;
      xvec = (reinterpret_cast<uintptr_t>(xrow) % 16) == 0;
    }
  }
  const bool normed = pending && s != 0.0;      // (s == 0: the scalar step relaxes, F08:275; NaN: goes on, like the reference)
  const double rs = 1.0 / s;

  // ---- phase 3: every other sum, on the rounded w1' (F08:286-290, 371) ----
  const int ngroup = (nolder + kBatchGroup - 1) / kBatchGroup;
  for (int g = 0; g < (ngroup > 0 ? ngroup : (normed ? 1 : 0)); g++) {
    const double *wk[kBatchGroup];
#pragma unroll
    for (int j = 0; j < kBatchGroup; j++) {
      const int p = g * kBatchGroup + j;
      wk[j] = nolder > 0 ? W + (size_t)(ps[p < nolder ? p : nolder - 1] - 1) * a.stride : w1;   // (beyond the list: a re-read, discarded)
    }
    double acc[kBatchAcc];
#pragma unroll
    for (int q = 0; q < kBatchAcc; q++) acc[q] = 0.0;
    waves_sweep(n, fvec, lane, [&](auto full, auto fv_, int64_t i) {
      constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
      const d2 fv = ld_tile<FULL, FV>(f, i, n);
      const d2 dv = ld_tile<FULL, true>(w1, i, n);     // (no pending pair: a stored vector whose value is not used)
      d2 wv_[kBatchGroup];
#pragma unroll
      for (int j = 0; j < kBatchGroup; j++) wv_[j] = ld_tile<FULL, true>(wk[j], i, n);
      [[maybe_unused]] d2 gv;
      if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double fq = fv[q];
          double fa = fq;                                  // first operand of the products on f: fl(w f), formed once
          if constexpr (WGT) fa = gv[q] * fq;
          if (normed) {
            const double wn = batch_nrm<RCP>(dv[q] - fq, s, rs);
            double wa = wn;                                // first operand of the Gram row: fl(w w1')
            if constexpr (WGT) wa = gv[q] * wn;
            if (g == 0) acc[2 * kBatchGroup] = fma(fa, wn, acc[2 * kBatchGroup]);
#pragma unroll
            for (int j = 0; j < kBatchGroup; j++) acc[j] = fma(wa, wv_[j][q], acc[j]);
          }
#pragma unroll
          for (int j = 0; j < kBatchGroup; j++) acc[kBatchGroup + j] = fma(fa, wv_[j][q], acc[kBatchGroup + j]);
        }
    });
#pragma unroll
    for (int q = 0; q < kBatchAcc; q++) acc[q] = wave_sum(acc[q]);      // (valid in lane 0, which alone uses them)
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kBatchGroup; j++)
        if (g * kBatchGroup + j < nolder) {
          if (normed) red[2 + g * kBatchGroup + j] = acc[j];
          red[2 + mvec + g * kBatchGroup + j] = acc[kBatchGroup + j];
        }
      if (g == 0 && normed) red[1] = acc[2 * kBatchGroup];
    }
  }

  // ---- phase 4: the scalar step on this wavefront's working copy.  red and ps were written by lane 0: it runs the step itself,
  // or, with ROWS, all 64 lanes run it and read them behind a wave_sync ----
  if constexpr (ROWS > 0) {
    wave_sync();
    batch_scalar_step_rows<ROWS>(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr, reinterpret_cast<double *>(smem + wl.a_base(wv)));
  } else {
    if (lane == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);
  }
  wave_sync();

  // ---- phase 5: the working copy back ----
  for (int i = lane; i < nh; i += 64) ctl.h()[i] = L.h[i];
  for (int i = lane; i < m1 + 1; i += 64) {
    ctl.c()[i] = L.c[i];
    ctl.next()[i] = L.next[i];
    ctl.prev()[i] = L.prev[i];
  }
  for (int i = lane; i < 2 + 2 * mvec; i += 64) ctl.red()[i] = red[i];

  // ---- phase 6: normalise the pending pair, combine, ring stores (F08:282-283, 361, 395-404); the weights are not read ----
  const int ncomb = hdr[HDR_NCOMB];
  const bool norm0 = hdr[HDR_NORMED] != 0;      // pair 0 of the plan is the pending pair, still raw
  double *const wnew = W + (size_t)(hdr[HDR_NEW] - 1) * a.stride, *const vnew = V + (size_t)(hdr[HDR_NEW] - 1) * a.stride;
  waves_sweep(n, fvec, lane, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    if (!FULL && i >= n) return;
    const d2 fin = ld_tile<FULL, FV>(f, i, n);
    d2 x = fin;
    [[maybe_unused]] d2 xit = {0.0, 0.0};      // STEP: the iterate's pair, loaded with the other loads of the tile
    if constexpr (STEP)
      if (xrow != nullptr) xit = xvec ? ld_tile<FULL, true>(xrow, i, n) : ld_tile<FULL, false>(xrow, i, n);
    int j0 = 0;
    if (norm0) {      // pair 0 of the plan: the pending pair, still raw (F08:282-283)
      double *const wk = W + (size_t)(cs[0] - 1) * a.stride, *const vk = V + (size_t)(cs[0] - 1) * a.stride;
      d2 wv_ = ld_tile<FULL, true>(wk, i, n), vv = ld_tile<FULL, true>(vk, i, n);
      const double c = cc[0];
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const double wn = batch_nrm<RCP>(wv_[q] - fin[q], s, rs);
        const double vn = batch_nrm<RCP>(vv[q], s, rs);
        wv_[q] = wn;
        vv[q] = COMPACT ? vn - wn : vn;
        x[q] = COMPACT ? x[q] + c * vv[q] : comb1<COMB>(x[q], c, wv_[q], vv[q]);
      }
      st_tile<FULL, true>(wk, i, n, wv_);
      st_tile<FULL, true>(vk, i, n, vv);
      j0 = 1;
    }
    constexpr int U = 4;      // pairs whose loads are in flight together (beyond the plan: the last pair again, not applied)
    for (int j = j0; j < ncomb; j += U) {
      d2 wv_[U], vv[U];
      double c[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int jj = j + u < ncomb ? j + u : ncomb - 1;
        const size_t off = (size_t)(cs[jj] - 1) * a.stride;
        c[u] = cc[jj];
        vv[u] = ld_tile<FULL, true>(V + off, i, n);
        if (!COMPACT) wv_[u] = ld_tile<FULL, true>(W + off, i, n); else wv_[u] = vv[u];
      }
#pragma unroll
      for (int u = 0; u < U; u++)
        if (j + u < ncomb) {
#pragma unroll
          for (int q = 0; q < 2; q++) x[q] = COMPACT ? x[q] + c[u] * vv[u][q] : comb1<COMB>(x[q], c[u], wv_[u][q], vv[u][q]);
        }
    }
    st_tile<FULL, true>(wnew, i, n, fin);
    st_tile<FULL, true>(vnew, i, n, x);
    if (ncomb > 0) st_tile<FULL, FV>(f, i, n, x);      // (nothing to combine: f stays as it is)
    if constexpr (STEP)
      if (xrow != nullptr) {
        xit[0] = xit[0] - x[0];
        xit[1] = xit[1] - x[1];
        if (xvec) st_tile<FULL, true>(xrow, i, n, xit); else st_tile<FULL, false>(xrow, i, n, xit);
      }
  });
}

// THE LAUNCH LADDER: flavour -> weighted? -> lengths? -> launch.  (Whether a call is weighted, in which form, and whether it has
// lengths travels in the launch: the instance, the two buffers' addresses and the row stride are fixed when the call is enqueued
// -- or captured --, the buffers' VALUES are read when it runs.)
// ... -> the scalar step: a batch of nka_hip_batch_create_waves_rows whose setting is NKA_HIP_BATCH_SCALAR_WAVEFRONT launches the
// instance with a WavesRows<NLMAX> behind the pack and asks for the LDS of waves_rows_lds; every other call is the launch it was
template <int COMB, int NLMAX, class... Pack>
void launch_waves_rows_nl(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Pack... pack) {
  const size_t lds = (size_t)nka_host::waves_rows_lds(b->k.mvec).bytes();
  hipLaunchKernelGGL((k_waves_update<COMB, Pack..., WavesRows<NLMAX>>), dim3((unsigned)nka_host::waves_ngroup(b->k.nsys)), dim3(kWavesThreads),
                     lds, b->stream, b->k, f, ld, active, pack..., WavesRows<NLMAX>{});
}
template <int COMB, class... Pack>
void launch_waves_as(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Pack... pack) {
  if (b->waves_rows && b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT) {
    switch (nka_host::waves_rows_nlmax(b->k.mvec)) {
      case 6: launch_waves_rows_nl<COMB, 6, Pack...>(b, f, ld, active, pack...); break;
      case 11: launch_waves_rows_nl<COMB, 11, Pack...>(b, f, ld, active, pack...); break;
      case 21: launch_waves_rows_nl<COMB, 21, Pack...>(b, f, ld, active, pack...); break;
      default: launch_waves_rows_nl<COMB, nka_host::waves_rows_max_mvec() + 1, Pack...>(b, f, ld, active, pack...);
    }
    return;
  }
  const size_t lds = (size_t)nka_host::waves_lds(b->k.mvec).bytes();
  hipLaunchKernelGGL((k_waves_update<COMB, Pack...>), dim3((unsigned)nka_host::waves_ngroup(b->k.nsys)), dim3(kWavesThreads), lds,
                     b->stream, b->k, f, ld, active, pack...);
}
template <int COMB, class... Pack>
void launch_waves_len(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Pack... pack) {
  if (b->waves_ext && b->has_len) launch_waves_as<COMB, Pack..., LenArgs>(b, f, ld, active, pack..., LenArgs{b->len});
  else launch_waves_as<COMB, Pack...>(b, f, ld, active, pack...);
}
template <int COMB, class... Step>
void launch_waves_wgt(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (b->waves_ext && b->weighted)      // (the pack is named throughout: deduction would drop the __restrict__ of WgtRows)
    launch_waves_len<COMB, WgtRows, WgtStride, Step...>(b, f, ld, active, b->wgt, WgtStride(b->wgt_stride), step...);
  else launch_waves_len<COMB, Step...>(b, f, ld, active, step...);
}
// `step`: nothing for the update, one StepArgs for the solve step
template <class... Step>
void launch_waves(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  switch (b->flavor) {
    case NKA_HIP_FLAVOR_F08_VECTOR: launch_waves_wgt<1>(b, f, ld, active, step...); break;
    case NKA_HIP_FLAVOR_C: launch_waves_wgt<2>(b, f, ld, active, step...); break;
    default: launch_waves_wgt<0>(b, f, ld, active, step...);
  }
}

}  // namespace

void nka_batch_waves_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active) { launch_waves(b, f, ld, active); }

void nka_batch_waves_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                          double *fnorm) {
  launch_waves(b, f, ld, active, StepArgs{x, x ? ldx : 0, tol, fnorm});
}

extern "C" int nka_hip_batch_waves_rows_limits(int32_t *max_mvec, int32_t mvec, int64_t *lds_bytes) {
  constexpr int cap = nka_host::waves_rows_max_mvec();
  if (mvec < 1 || mvec > cap)
    return fail(NKA_HIP_EINVAL, "nka_hip_batch_waves_rows_limits: mvec must be 1 ... " + std::to_string(cap) +
                                    " (four working copies and four matrices in 64 KiB of LDS)");
  if (max_mvec) *max_mvec = cap;
  if (lds_bytes) *lds_bytes = nka_host::waves_rows_lds(mvec).bytes();
  return 0;
}

extern "C" int nka_hip_batch_waves_limits(int32_t *systems_per_group, int64_t *max_vlen) {
  if (systems_per_group) *systems_per_group = kWavesGroup;
  if (max_vlen) *max_vlen = NKA_HIP_BATCH_WAVES_MAX_VLEN;
  return 0;
}
