// nka_batch_lanes.hip -- the LANE batch of include/nka_hip_batch.h (nka_hip_batch_create_lanes): ONE LANE PER SYSTEM, for very
// short systems (vlen <= 64).  A workgroup is one wavefront and advances G = nka_host::lanes_group(mvec) systems; lane l of
// workgroup g owns system g * G + l through every phase, and the scalar steps of up to 64 systems run side by side on the
// lanes that the narrow batch (nka_batch.hip: a workgroup of 256 threads per system) leaves idle.
//
// A sum formed by one lane, element after element, is the reference's order: every sum below is one chain a = a + x * y with
// one rounding per product and per addition (contraction off), its operands in the order of k_batch_update<*, true>, so a
// system carries the bits of the narrow batch in NKA_HIP_SUMS_REFERENCE_ORDER -- and of the reference -- by construction.
//   1 load      the control blocks of the group's live systems into the lanes' working copies in LDS, system after system with
//               all lanes (source: h, c, next, prev of system g * G + s; destination: the copy of lane s)
//   2 norm      per lane: [dp(f, f),] dp(d, d), d = fl(w1 - f); s = sqrt          -- a step may retire the system here
//   3 sums      per lane: <f,w1'>, <w1',w_p>, <f,w_p> on the rounded w1', four older vectors per pass over the elements
//   4 scalar    per lane: batch_scalar_step on its own working copy
//   5 combine   per lane: normalise the pending pair, combine in list order, w_new = f_in, v_new = f_out, f [, x -= f_out]
//   6 store     the working copies of the live systems back, system after system with all lanes (source: the copy of lane s;
//               destination: h, c, next, prev, red of system g * G + s)
// Masked, retired and absent systems are PREDICATED LANES: every thread reaches both barriers, a lane whose system sits out
// reads and writes no byte of it, and the cooperative copies skip it (hdr[kLanesHdrLive] of its copy).  No workgroup reads what
// another writes, and outside the two cooperative copies no lane reads what another lane's system owns: no flags, no spinning,
// no atomics, no cooperative launch.  Per-lane arrays live in LDS (host_logic.hpp: LanesLds and THE BANK RULE), never in private
// arrays: no scratch.  The slots are interleaved across the systems of a group (lanes_slot_offset), so a wavefront's load of
// element i of a stored vector is one contiguous run; the caller's rows of f and x stay where they are, one row per lane.
#include "nka_batch_dev.hpp"

#include <algorithm>
#include <cstdint>
#include <string>

using namespace nka;

namespace {

using nka_host::kLanesHdrLive;
using nka_host::kLanesThreads;

// what a solve step takes beside the update's arguments (the StepArgs of nka_batch.hip); each pointer may be NULL
struct StepArgs {
  double *x;
  int64_t ldx;
  const double *tol;
  double *fnorm;
};

static_assert(nka_host::kLanesMaxVlen == kOrdAutoMax && NKA_HIP_BATCH_LANES_MAX_VLEN == kOrdAutoMax,
              "the cap is the range in which the narrow batch's default is the reference order");
static_assert(nka_host::lanes_group(NKA_HIP_BATCH_MAX_MVEC) >= 1, "a workgroup advances at least one system");
static_assert(nka_host::kLanesLdsBudget <= 160 * 1024, "the LDS of a CU");

// Step...: nothing (the update) or one StepArgs (the solve step).  G: systems per workgroup, = lanes_group(a.mvec).
template <int COMB, class... Step>
__global__ __launch_bounds__(kLanesThreads) void k_lanes_update(BatchArgs a, int32_t G, double *f_all, int64_t ld,
                                                                const int32_t *__restrict__ active, Step... step) {
#pragma clang fp contract(off)      // every sum is a chain of separately rounded products and additions, like the reference
  constexpr bool STEP = sizeof...(Step) == 1;
  static_assert(sizeof...(Step) <= 1, "nothing, or one StepArgs");
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nh = (m1 + 1) * (m1 + 1);
  const int n = (int)a.n;      // (1 ... 64)
  const nka_host::LanesLds lds = nka_host::lanes_lds(mvec);
  const int64_t sys0 = (int64_t)blockIdx.x * G;
  const int64_t sys = sys0 + t;
  // the lane has a system and the system takes part (lanes at or beyond G, and beyond nsys in the last group, do nothing)
  bool live = t < G && sys < a.nsys && (active == nullptr || active[sys] != 0);

  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + (size_t)G * lds.dstride);
  const int tl = t < G ? t : 0;      // (a lane without a copy forms the addresses of copy 0 and never uses them)
  double *const myd = shd + lds.dbase(tl);
  int32_t *const myi = shi + lds.ibase(tl);
  Lst L;
  L.h = myd + lds.h;
  L.c = myd + lds.c;
  double *const red = myd + lds.red;
  double *const cc = myd + lds.cc;           // combine plan: coefficients in list order (slots: cs)
  L.next = myi + lds.next;
  L.prev = myi + lds.prev;
  int32_t *const ps = myi + lds.ps;          // older list entries at entry, in list order
  int32_t *const cs = myi + lds.cs;
  int32_t *const hdr = myi + lds.hdr;
  L.m1 = m1;
  L.mvec = mvec;
  L.subspace = L.pending = L.first = L.last = L.free_ = 0;
  L.vtol = 0.0;

  // ---- phase 1: the working copies.  Cooperative copy: source the control block of system sys0 + s, destination the copy of
  // lane s; a system that sits out is neither read nor given a copy ----
  if (t < G) hdr[kLanesHdrLive] = live ? 1 : 0;
  __syncthreads();
  for (int e = t; e < G * nh; e += kLanesThreads) {
    const int s = e / nh, i = e - s * nh;
    if (shi[lds.ibase(s) + lds.hdr + kLanesHdrLive]) shd[lds.dbase(s) + lds.h + i] = batch_ctl(a, (int)(sys0 + s)).h()[i];
  }
  for (int e = t; e < G * (m1 + 1); e += kLanesThreads) {
    const int s = e / (m1 + 1), i = e - s * (m1 + 1);
    if (shi[lds.ibase(s) + lds.hdr + kLanesHdrLive]) {
      const Ctl cs_ = batch_ctl(a, (int)(sys0 + s));
      shd[lds.dbase(s) + lds.c + i] = cs_.c()[i];
      shi[lds.ibase(s) + lds.next + i] = cs_.next()[i];
      shi[lds.ibase(s) + lds.prev + i] = cs_.prev()[i];
    }
  }
  __syncthreads();

  // ---- phases 2 to 5: the lane's own system, no barrier inside ----
  if (live) {
    const Ctl ctl = batch_ctl(a, (int)sys);
    double *const f = f_all + sys * ld;
    // this lane's column of the group's interleaved slots: element i of slot k at ((k - 1) n + i) G
    const int64_t gbase = (int64_t)blockIdx.x * nka_host::lanes_group_stride(n, mvec, G) + t;
    double *const W = a.w + gbase, *const V = a.v + gbase;
    const int eg = G;                        // doubles between two elements of a stored vector
    const int sg = n * G;                    // ... and between two slots
    for (int i = 0; i < 2 + 2 * mvec; i++) red[i] = 0.0;      // an update rewrites every entry
    lst_load_scalars(L, ctl);
    L.vtol = ctl.dc[DC_VTOL];
    int nolder = 0;
    for (int k = L.pending ? L.next[L.first] : L.first; k != 0 && nolder < m1; k = L.next[k]) ps[nolder++] = k;
    const int pending = L.pending;
    const double *const w1 = W + (pending ? (L.first - 1) * sg : 0);      // (no pending pair: never read)

    // ---- phase 2: the norm (F08:266-267), and the step's residual norm and stop rule ----
    double s = 0.0;
    if constexpr (STEP) {
      const StepArgs &st = (step, ...);
      double ff = 0.0;
      for (int i = 0; i < n; i++) ff = ff + f[i] * f[i];
      const double r = sqrt(ff);
      if (st.fnorm != nullptr) st.fnorm[sys] = r;
      if (st.tol != nullptr && r <= st.tol[sys]) {      // (a NaN on either side: false, the system goes on)
        const_cast<int32_t *>(active)[sys] = 0;         // the system retires: nothing else of it is written
        hdr[kLanesHdrLive] = 0;
        live = false;
      }
    }
    if (live) {
      if (pending) {
        double dd = 0.0;
        for (int i = 0; i < n; i++) {
          const double d = w1[i * eg] - f[i];
          dd = dd + d * d;
        }
        red[0] = dd;
        s = sqrt(dd);
      }
      const bool normed = pending && s != 0.0;      // (s == 0: the scalar step relaxes, F08:275; NaN: goes on, like the reference)
      const double rs = 1.0 / s;

      // ---- phase 3: every other sum, on the rounded w1' (F08:286-290, 371), kBatchGroup older vectors per pass ----
      const int ngroup = (nolder + kBatchGroup - 1) / kBatchGroup;
      for (int g = 0; g < (ngroup > 0 ? ngroup : (normed ? 1 : 0)); g++) {
        const double *wk[kBatchGroup];
#pragma unroll
        for (int j = 0; j < kBatchGroup; j++) {
          const int p = g * kBatchGroup + j;      // (beyond the list: the last entry again, discarded)
          wk[j] = nolder > 0 ? W + (ps[p < nolder ? p : nolder - 1] - 1) * sg : W;
        }
        double acc[kBatchAcc];
#pragma unroll
        for (int q = 0; q < kBatchAcc; q++) acc[q] = 0.0;
        for (int i = 0; i < n; i++) {
          const double fq = f[i];
          double y[kBatchGroup];
#pragma unroll
          for (int j = 0; j < kBatchGroup; j++) y[j] = wk[j][i * eg];
          if (normed) {
            const double wn = batch_nrm<RCP>(w1[i * eg] - fq, s, rs);
            if (g == 0) acc[2 * kBatchGroup] = acc[2 * kBatchGroup] + wn * fq;      // dp(f, w1')
#pragma unroll
            for (int j = 0; j < kBatchGroup; j++) acc[j] = acc[j] + wn * y[j];       // dp(w1', w_p)
          }
#pragma unroll
          for (int j = 0; j < kBatchGroup; j++) acc[kBatchGroup + j] = acc[kBatchGroup + j] + fq * y[j];      // dp(f, w_p)
        }
#pragma unroll
        for (int j = 0; j < kBatchGroup; j++) {
          const int p = g * kBatchGroup + j;
          if (p < nolder) {
            if (normed) red[2 + p] = acc[j];
            red[2 + mvec + p] = acc[kBatchGroup + j];
          }
        }
        if (g == 0 && normed) red[1] = acc[2 * kBatchGroup];
      }

      // ---- phase 4: the scalar step on this lane's working copy ----
      batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);

      // ---- phase 5: normalise the pending pair, combine, ring stores (F08:282-283, 361, 395-404) ----
      const int ncomb = hdr[HDR_NCOMB];
      const bool norm0 = hdr[HDR_NORMED] != 0;      // pair 0 of the plan is the pending pair, still raw
      double *const wnew = W + (hdr[HDR_NEW] - 1) * sg, *const vnew = V + (hdr[HDR_NEW] - 1) * sg;
      double *const w0 = W + (norm0 ? (cs[0] - 1) * sg : 0), *const v0 = V + (norm0 ? (cs[0] - 1) * sg : 0);
      const double c0 = norm0 ? cc[0] : 0.0;
      [[maybe_unused]] double *xrow = nullptr;      // this system's row of the iterate, if there is one
      if constexpr (STEP) {
        const StepArgs &st = (step, ...);
        if (st.x != nullptr) xrow = st.x + sys * st.ldx;
      }
      for (int i = 0; i < n; i++) {
        const double fin = f[i];
        double x = fin;
        int j = 0;
        if (norm0) {      // (F08:282-283)
          const double wn = batch_nrm<RCP>(w0[i * eg] - fin, s, rs);
          const double vn = batch_nrm<RCP>(v0[i * eg], s, rs);
          const double vv = COMPACT ? vn - wn : vn;
          x = COMPACT ? x + c0 * vv : comb1<COMB>(x, c0, wn, vv);
          w0[i * eg] = wn;
          v0[i * eg] = vv;
          j = 1;
        }
        for (; j < ncomb; j++) {
          const int off = (cs[j] - 1) * sg + i * eg;
          const double c = cc[j];
          const double vv = V[off];
          if constexpr (COMPACT) x = x + c * vv; else x = comb1<COMB>(x, c, W[off], vv);
        }
        wnew[i * eg] = fin;
        vnew[i * eg] = x;
        if (ncomb > 0) f[i] = x;      // (nothing to combine: f stays as it is)
        if constexpr (STEP)
          if (xrow != nullptr) xrow[i] = xrow[i] - x;
      }
    }
  }
  __syncthreads();

  // ---- phase 6: the working copies back.  Cooperative copy: source the copy of lane s, destination the control block of system
  // sys0 + s; a system that sat out or retired in this call is not written ----
  for (int e = t; e < G * nh; e += kLanesThreads) {
    const int s = e / nh, i = e - s * nh;
    if (shi[lds.ibase(s) + lds.hdr + kLanesHdrLive]) batch_ctl(a, (int)(sys0 + s)).h()[i] = shd[lds.dbase(s) + lds.h + i];
  }
  for (int e = t; e < G * (m1 + 1); e += kLanesThreads) {
    const int s = e / (m1 + 1), i = e - s * (m1 + 1);
    if (shi[lds.ibase(s) + lds.hdr + kLanesHdrLive]) {
      const Ctl cs_ = batch_ctl(a, (int)(sys0 + s));
      cs_.c()[i] = shd[lds.dbase(s) + lds.c + i];
      cs_.next()[i] = shi[lds.ibase(s) + lds.next + i];
      cs_.prev()[i] = shi[lds.ibase(s) + lds.prev + i];
    }
  }
  for (int e = t; e < G * (2 + 2 * mvec); e += kLanesThreads) {
    const int s = e / (2 + 2 * mvec), i = e - s * (2 + 2 * mvec);
    if (shi[lds.ibase(s) + lds.hdr + kLanesHdrLive]) batch_ctl(a, (int)(sys0 + s)).red()[i] = shd[lds.dbase(s) + lds.red + i];
  }
}

template <int COMB, class... Step>
void launch_lanes_as(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  const int G = b->lanes_group;
  const size_t lds = (size_t)nka_host::lanes_lds(b->k.mvec).bytes(G);
  hipLaunchKernelGGL((k_lanes_update<COMB, Step...>), dim3((unsigned)nka_host::lanes_ngroup(b->k.nsys, G)), dim3(kLanesThreads), lds,
                     b->stream, b->k, (int32_t)G, f, ld, active, step...);
}
template <class... Step>
void launch_lanes(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  switch (b->flavor) {
    case NKA_HIP_FLAVOR_F08_VECTOR: launch_lanes_as<1>(b, f, ld, active, step...); break;
    case NKA_HIP_FLAVOR_C: launch_lanes_as<2>(b, f, ld, active, step...); break;
    default: launch_lanes_as<0>(b, f, ld, active, step...);
  }
}

}  // namespace

int nka_batch_lanes_alloc(nka_hip_batch_t b) {
  const int G = nka_host::lanes_group(b->k.mvec);
  b->lanes_group = G;
  const int64_t elems = nka_host::lanes_slot_alloc_elems(b->k.n, b->k.mvec, G, b->k.nsys);
  if ((double)elems * 8.0 > 1.0e13) return fail(NKA_HIP_ENOMEM, "nka_hip_batch_create_lanes: the batch needs more device memory than any device has");
  const size_t bytes = sizeof(double) * (size_t)elems;
  for (double **p : {&b->k.w, &b->k.v}) {
    const hipError_t e = hipMalloc((void **)p, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(NKA_HIP_ENOMEM, std::string("hipMalloc(") + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    }
    HIP_TRY(hipMemsetAsync(*p, 0, bytes, b->stream));
  }
  b->vector_bytes = nka_host::lanes_vector_bytes(b->k.n, b->k.mvec, G, b->k.nsys);
  return 0;
}

void nka_batch_lanes_free(nka_hip_batch_t) {}      // (k.w and k.v are freed with every batch's)

void nka_batch_lanes_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active) { launch_lanes(b, f, ld, active); }

void nka_batch_lanes_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                          double *fnorm) {
  launch_lanes(b, f, ld, active, StepArgs{x, x ? ldx : 0, tol, fnorm});
}

// element i of the slot lies lanes_group doubles from element i - 1: a strided copy of vlen single doubles
int nka_batch_lanes_get_slot(nka_hip_batch_t b, bool v, int32_t sys, int32_t slot, double *host_out) {
  const int G = b->lanes_group;
  const double *src = (v ? b->k.v : b->k.w) + nka_host::lanes_slot_offset(b->k.n, b->k.mvec, G, sys, slot, 0);
  HIP_TRY(hipMemcpy2DAsync(host_out, sizeof(double), src, sizeof(double) * (size_t)G, sizeof(double), (size_t)b->k.n, hipMemcpyDeviceToHost,
                           b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int nka_hip_batch_lanes_limits(int32_t mvec, int32_t *systems_per_group, int64_t *max_vlen) {
  if (mvec < 1 || mvec > NKA_HIP_BATCH_MAX_MVEC)
    return fail(NKA_HIP_EINVAL, "nka_hip_batch_lanes_limits: mvec must be 1 ... " + std::to_string((int)NKA_HIP_BATCH_MAX_MVEC));
  if (systems_per_group) *systems_per_group = nka_host::lanes_group(mvec);
  if (max_vlen) *max_vlen = NKA_HIP_BATCH_LANES_MAX_VLEN;
  return 0;
}
