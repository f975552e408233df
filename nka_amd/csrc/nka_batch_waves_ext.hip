// nka_batch_waves_ext.hip -- the WAVE batch WITH PER-SYSTEM LENGTHS AND DIAGONAL DOT WEIGHTS (nka_hip_batch_create_waves_ext of
// include/nka_hip_batch.h).  The kernel of nka_batch_waves.hip restated, statement for statement where the two overlap, with the
// two arguments that kernel does not take; nka_batch_waves.hip itself is held to its text and its machine code and is not touched.
// A batch of the new entry with neither lengths nor weights set runs nka_batch_waves_update / _step; this unit holds only the
// instances with at least one of the two: 3 flavours x {weights, lengths, both} x {update, step} = 18.
//   LENGTHS  A trailing LenArgs makes n = len[sys] -- one uniform load behind the `active` test -- the length of EVERY phase: the
//            sweeps, the step's <f,f> and x -= f_out, the weight loads.  Lane l owns the pair 2l, 2l + 1 of every 128-element tile
//            and meets its pairs in increasing order whatever n is, and the butterfly does not depend on n: the system carries the
//            bits of a wave batch created with vlen = len[sys], and nothing at an index >= len[sys] of f, x, the weight row or a
//            slot is read or written.
//   WEIGHTS  WGT = true: row `sys` of the batch's weight buffer -- wgt_all + sys * wgt_stride, 0 for the form all systems share --
//            is read like a stored vector (16-byte aligned rows at the slot stride) in phases 2 and 3, and fl(w_i a_i) is the
//            FIRST operand of every product, the narrow batch's table: red[0] fma(fl(w d), d, .), red[1] fma(fl(w f), w1', .),
//            red[2+p] fma(fl(w w1'), w_p, .), red[2+m+p] fma(fl(w f), w_p, .), the step's <f,f> fma(fl(w f), f, .); fl(w f) is
//            formed once per element and sweep.  Phase 6 does not read the weights.  The chain of roundings behind the first
//            operand is the unweighted one: waves_k(n) stands.
// Everything else is the wave batch's: no __syncthreads(), no flags, no spinning, no cooperative launch; a masked, retired or
// absent wavefront returns on its own; every element of f, x and the slots belongs to one lane in all phases.
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

// what a solve step takes beside the update's arguments (the StepArgs of nka_batch_waves.hip); each pointer may be NULL
struct StepArgs {
  double *x;
  int64_t ldx;
  const double *tol;
  double *fnorm;
};
// the batch's buffer of nsys validated lengths, 1 <= len[sys] <= vlen (the LenArgs of nka_batch.hip): the LAST member of the pack
struct LenArgs {
  const int32_t *len;
};
__device__ __forceinline__ const StepArgs &step_args(const StepArgs &st) { return st; }
__device__ __forceinline__ const StepArgs &step_args(const StepArgs &st, const LenArgs &) { return st; }
__device__ __forceinline__ const int32_t *len_args(const LenArgs &l) { return l.len; }
__device__ __forceinline__ const int32_t *len_args(const StepArgs &, const LenArgs &l) { return l.len; }

// one lane's LDS traffic ordered against the other lanes' of the SAME wavefront (nka_batch_waves.hip, SYNCHRONISATION)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum over the wavefront, in every lane (wave_sum leaves it in lane 0)
__device__ __forceinline__ double wave_sum_all(double x) { return readlane_f64(wave_sum(x), 0); }

// One sweep over a system's elements at wavefront width: body(FULL, FVEC, i) for this lane's pair i = 2l, 2l + 128, ... -- the full
// tiles first, then the ragged one with guards (waves_sweep of nka_batch_waves.hip).
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

// Pack...: [StepArgs][, LenArgs], the order of k_batch_update (nka_batch.hip).  wgt_all / wgt_stride are read by WGT = true only.
template <int COMB, bool WGT, class... Pack>
__global__ __launch_bounds__(kWavesThreads) void k_waves_ext_update(BatchArgs a, double *__restrict__ f_all, int64_t ld,
                                                                    const int32_t *__restrict__ active,
                                                                    const double *__restrict__ wgt_all, int64_t wgt_stride, Pack... pack) {
#pragma clang fp contract(off)      // elementwise statements round like the reference; fma is explicit
  constexpr bool STEP = (std::is_same<Pack, StepArgs>::value || ...);
  constexpr bool LEN = (std::is_same<Pack, LenArgs>::value || ...);
  static_assert(sizeof...(Pack) == (STEP ? 1 : 0) + (LEN ? 1 : 0), "at most one StepArgs, then at most one LenArgs");
  static_assert(WGT || LEN, "neither: k_waves_update of nka_batch_waves.hip");
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
    if constexpr (LEN) return len_args(pack...)[sys]; else return a.n;      // (validated when it was set: 1 <= len[sys] <= a.n)
  }();
  const Ctl ctl = batch_ctl(a, (int)sys);
  double *const f = f_all + (size_t)sys * (size_t)ld;
  double *const W = a.w + (size_t)sys * (size_t)a.sys_stride, *const V = a.v + (size_t)sys * (size_t)a.sys_stride;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;      // (stored vectors: always 16-byte aligned)
  [[maybe_unused]] const double *wg = nullptr;                       // this system's weights (rows: 16-byte aligned)
  if constexpr (WGT) wg = wgt_all + (size_t)sys * (size_t)wgt_stride;

  const nka_host::WavesLds wl = nka_host::waves_lds(mvec);
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
    const StepArgs &st = step_args(pack...);
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

  // ---- phase 4: the scalar step on this wavefront's working copy (red, ps: written by lane 0 itself) ----
  if (lane == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);
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

// (whether a call is weighted, in which form, and whether it has lengths travels in the launch: the instance, the two buffers'
// addresses and the row stride are fixed when the call is enqueued -- or captured --, the buffers' VALUES are read when it runs)
template <int COMB, bool WGT, class... Pack>
void launch_waves_ext_as(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Pack... pack) {
  const size_t lds = (size_t)nka_host::waves_lds(b->k.mvec).bytes();
  hipLaunchKernelGGL((k_waves_ext_update<COMB, WGT, Pack...>), dim3((unsigned)nka_host::waves_ngroup(b->k.nsys)), dim3(kWavesThreads), lds,
                     b->stream, b->k, f, ld, active, WGT ? (const double *)b->wgt : (const double *)nullptr,
                     WGT ? b->wgt_stride : (int64_t)0, pack...);
}
template <int COMB, class... Step>
void launch_waves_ext_form(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (b->weighted) {
    if (b->has_len) launch_waves_ext_as<COMB, true>(b, f, ld, active, step..., LenArgs{b->len});
    else launch_waves_ext_as<COMB, true>(b, f, ld, active, step...);
  } else {
    launch_waves_ext_as<COMB, false>(b, f, ld, active, step..., LenArgs{b->len});      // (the caller saw has_len)
  }
}
template <class... Step>
void launch_waves_ext(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  switch (b->flavor) {
    case NKA_HIP_FLAVOR_F08_VECTOR: launch_waves_ext_form<1>(b, f, ld, active, step...); break;
    case NKA_HIP_FLAVOR_C: launch_waves_ext_form<2>(b, f, ld, active, step...); break;
    default: launch_waves_ext_form<0>(b, f, ld, active, step...);
  }
}

}  // namespace

// (both: b->waves_ext && (b->weighted || b->has_len), which accel_update and accel_step of nka_batch.hip test)
void nka_batch_waves_ext_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active) { launch_waves_ext(b, f, ld, active); }

void nka_batch_waves_ext_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                              double *fnorm) {
  launch_waves_ext(b, f, ld, active, StepArgs{x, x ? ldx : 0, tol, fnorm});
}
