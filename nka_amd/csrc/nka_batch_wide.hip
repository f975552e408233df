// nka_batch_wide.hip -- the WIDE batched accelerator (nka_hip_batch_create_wide, include/nka_hip_batch.h): nsys independent NKA
// states of equal shape, each split into nchunk chunks of NKA_HIP_BATCH_WIDE_CHUNK elements with ONE WORKGROUP PER CHUNK
// (blockIdx.x = chunk, blockIdx.y = system).  The phases of k_batch_update (nka_batch.hip) that need a sum over the whole
// system are separated by KERNEL BOUNDARIES instead of workgroup barriers -- an update is four launches in a line:
//   k_wide_norm      phase 2 on a chunk: sum d^2 of the chunk -> part[sys][0][chunk]
//   k_wide_sums      s = sqrt(part[sys][0][0] + part[sys][0][1] + ...), the same bits in every workgroup of the system; phase 3
//                    on a chunk -> part[sys][1 ...][chunk]
//   k_wide_scalar    one workgroup per system: red[j] = the chunk-order sum of entry j's partials; phases 4 and 5; the plan
//   k_wide_combine   phase 6 on a chunk
// Within a launch no workgroup reads what another writes: no flags, no spinning, no atomics, no cooperative launch.  A chunk
// is whole tiles of 512 elements, so inside a chunk the element -> thread map, the per-thread order, the 16-byte alignment of
// the stored vectors and the parity of a row of f are those of the narrow kernel: a wide batch of ONE chunk returns the
// narrow batch's bits.  Which partials a kernel reads is decided from the list (pending, normed, nolder), never from what the
// buffer holds: a partial that this update did not write is not read.
// With diagonal dot weights (a batch of nka_hip_batch_create_wide_ext) the first two launches are k_wide_norm_wgt and
// k_wide_sums_wgt, further down; the last two do not read weights and stay the kernels above.
#include "nka_batch_dev.hpp"

#include <string>

using namespace nka;

namespace {

using nka_host::kWideChunk;
#ifndef NKA_BATCH_WIDE_CANDIDATE      // (a candidate build of another chunk: tools/batch_throughput.py --wide, never the product)
static_assert(kWideChunk == NKA_HIP_BATCH_WIDE_CHUNK, "host_logic.hpp and nka_hip_batch.h disagree on the chunk");
#endif
static_assert((int64_t)NKA_HIP_BATCH_WIDE_MAX_VLEN <= nka_host::kWideMaxChunks * (int64_t)NKA_HIP_BATCH_WIDE_CHUNK, "the cap is at most 1024 chunks");
static_assert(nka_host::wide_scalar_lds(NKA_HIP_BATCH_MAX_MVEC, nka_host::kWideMaxChunks).b.bytes() <= 40 * 1024, "LDS of the scalar kernel");

struct WideArgs {
  double *part;         // nka_host::wide_part_index
  double *plan_c;       // combine plan of system sys: plan_c + sys * (mvec + 1), plan_s likewise
  int32_t *plan_s;
  int32_t nchunk;
};

// pending, first and the links of the system into LDS with one coalesced load; thread 0 lists the older entries (the walk
// runs in LDS).  hdr[HDR_PENDING, HDR_FIRST, HDR_NOLDER] and ps[] are valid after the trailing barrier.
__device__ __forceinline__ void wide_list(const Ctl &ctl, int m1, int32_t *next, int32_t *ps, int32_t *hdr) {
  const int t = threadIdx.x;
  if (t < m1 + 1) next[t] = ctl.next()[t];
  if (t == 64) hdr[HDR_PENDING] = ctl.ic[IC_PENDING];
  if (t == 65) hdr[HDR_FIRST] = ctl.ic[IC_FIRST];
  __syncthreads();
  if (t == 0) {
    const int pending = hdr[HDR_PENDING], first = hdr[HDR_FIRST];
    int no = 0;
    for (int k = pending ? next[first] : first; k != 0 && no < m1; k = next[k]) ps[no++] = k;
    hdr[HDR_NOLDER] = no;
  }
  __syncthreads();
}

// <d,d> of a system: its nchunk partials in CHUNK ORDER, starting from part[0] -- staged into LDS by the whole workgroup, added by
// one thread.  Every workgroup that calls this for a system forms the same bits.  *out is valid after the trailing barrier.
__device__ __forceinline__ void wide_norm_sum(const double *__restrict__ part0, int nchunk, double *stage, double *out) {
  for (int c = threadIdx.x; c < nchunk; c += kBatchThreads) stage[c] = part0[c];
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = stage[0];
    for (int c = 1; c < nchunk; c++) r += stage[c];
    *out = r;
  }
  __syncthreads();
}

// ---- 1: the norm (F08:266-267) of a chunk ----
__global__ __launch_bounds__(kBatchThreads) void k_wide_norm(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                                             const int32_t *__restrict__ active) {
#pragma clang fp contract(off)
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  const Ctl ctl = batch_ctl(a, sys);
  if (ctl.ic[IC_PENDING] == 0) return;      // (uniform: no pending pair, no norm -- and nobody reads this partial)
  __shared__ double sm[kBatchWaves], res[2];
  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_chunk_len(a.n, blockIdx.x);
  const double *const f = f_all + (size_t)sys * ld + lo;
  const double *const w1 = a.w + (size_t)sys * a.sys_stride + (size_t)(ctl.ic[IC_FIRST] - 1) * a.stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double acc[1] = {};
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    const d2 fv = ld_tile<FULL, FV>(f, i, n), wv = ld_tile<FULL, true>(w1, i, n);
#pragma unroll
    for (int q = 0; q < 2; q++)
      if (FULL || i + q < n) {
        const double d = wv[q] - fv[q];
        acc[0] = fma(d, d, acc[0]);
      }
  });
  batch_block_sum<1>(acc, sm, res);
  if (threadIdx.x == 0) wa.part[nka_host::wide_part_index(sys, 0, blockIdx.x, a.mvec, wa.nchunk)] = res[0];
}

// ---- 2: every other sum of a chunk, on the rounded w1' (F08:286-290, 371) ----
template <int COMB>
__global__ __launch_bounds__(kBatchThreads) void k_wide_sums(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                                             const int32_t *__restrict__ active) {
#pragma clang fp contract(off)
  constexpr bool RCP = (COMB == 1);
  const int sys = blockIdx.y, chunk = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nchunk = wa.nchunk;
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideLds lds = nka_host::wide_sums_lds(mvec, nchunk);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  double *const stage = shd + lds.stage, *const sm = shd + lds.sm, *const res = shd + lds.res;
  int32_t *const next = shi + lds.next, *const ps = shi + lds.ps, *const hdr = shi + lds.hdr;

  wide_list(ctl, m1, next, ps, hdr);
  const int pending = hdr[HDR_PENDING], nolder = hdr[HDR_NOLDER];
  double s = 0.0;
  if (pending) {
    wide_norm_sum(wa.part + nka_host::wide_part_index(sys, 0, 0, mvec, nchunk), nchunk, stage, res + kBatchAcc);
    s = sqrt(res[kBatchAcc]);
  }
  const bool normed = pending && s != 0.0;
  const double rs = 1.0 / s;

  const int64_t lo = (int64_t)chunk * kWideChunk, n = nka_host::wide_chunk_len(a.n, chunk);
  const double *const f = f_all + (size_t)sys * ld + lo;
  const double *const W = a.w + (size_t)sys * a.sys_stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  const double *const w1s = pending ? W + (size_t)(hdr[HDR_FIRST] - 1) * a.stride : W;      // always a stored vector
  auto out = [&](int entry) -> double & { return wa.part[nka_host::wide_part_index(sys, entry, chunk, mvec, nchunk)]; };

  const int ngroup = (nolder + kBatchGroup - 1) / kBatchGroup;
  for (int g = 0; g < (ngroup > 0 ? ngroup : (normed ? 1 : 0)); g++) {
    const double *wk[kBatchGroup];
#pragma unroll
    for (int j = 0; j < kBatchGroup; j++) {
      const int p = g * kBatchGroup + j;
      wk[j] = nolder > 0 ? W + (size_t)(ps[p < nolder ? p : nolder - 1] - 1) * a.stride : w1s;   // (beyond the list: a re-read, discarded)
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
      for (int j = 0; j < kBatchGroup; j++) wv[j] = ld_tile<FULL, true>(wk[j], i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double fq = fv[q];
          if (normed) {
            const double wn = batch_nrm<RCP>(dv[q] - fq, s, rs);
            if (g == 0) acc[2 * kBatchGroup] = fma(fq, wn, acc[2 * kBatchGroup]);
#pragma unroll
            for (int j = 0; j < kBatchGroup; j++) acc[j] = fma(wn, wv[j][q], acc[j]);
          }
#pragma unroll
          for (int j = 0; j < kBatchGroup; j++) acc[kBatchGroup + j] = fma(fq, wv[j][q], acc[kBatchGroup + j]);
        }
    });
    batch_block_sum<kBatchAcc>(acc, sm, res);
    if (t < kBatchGroup && g * kBatchGroup + t < nolder) {
      if (normed) out(2 + g * kBatchGroup + t) = res[t];
      out(2 + mvec + g * kBatchGroup + t) = res[kBatchGroup + t];
    }
    if (t == 0 && g == 0 && normed) out(1) = res[2 * kBatchGroup];
    // (res is rewritten only behind the two barriers of the next batch_block_sum)
  }
}

// ---- 3: the sums of the system from its partials, the scalar step, the plan; one workgroup per system ----
__global__ __launch_bounds__(kBatchThreads) void k_wide_scalar(BatchArgs a, WideArgs wa, const int32_t *__restrict__ active) {
#pragma clang fp contract(off)
  const int sys = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nh = (m1 + 1) * (m1 + 1), nchunk = wa.nchunk;
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideScalarLds wl = nka_host::wide_scalar_lds(mvec, nchunk);
  const nka_host::BatchLds &lds = wl.b;
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  Lst L;
  L.h = shd + lds.h;
  L.c = shd + lds.c;
  double *const red = shd + lds.red;
  double *const cc = shd + lds.cc;
  double *const res = shd + lds.res;
  double *const stage = shd + wl.stage;
  L.next = shi + lds.next;
  L.prev = shi + lds.prev;
  int32_t *const ps = shi + lds.ps;
  int32_t *const cs = shi + lds.cs;
  int32_t *const hdr = shi + lds.hdr;
  L.m1 = m1;
  L.mvec = mvec;

  // the working copy (phase 1 of k_batch_update)
  for (int i = t; i < nh; i += kBatchThreads) L.h[i] = ctl.h()[i];
  for (int i = t; i < m1 + 1; i += kBatchThreads) {
    L.c[i] = ctl.c()[i];
    L.next[i] = ctl.next()[i];
    L.prev[i] = ctl.prev()[i];
  }
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
  double s = 0.0;
  if (pending) {      // the same chunk-order sum as k_wide_sums
    wide_norm_sum(wa.part + nka_host::wide_part_index(sys, 0, 0, mvec, nchunk), nchunk, stage, res + kBatchAcc);
    s = sqrt(res[kBatchAcc]);
  }
  const bool normed = pending && s != 0.0;
  // red[j], one thread per entry: the chunk-order sum of the partials k_wide_sums wrote in this update, zero everywhere else
  if (t < 2 + 2 * mvec) {
    double r = 0.0;
    if (t == 0) {
      if (pending) r = res[kBatchAcc];
    } else {
      const bool formed = t == 1 ? normed : t < 2 + mvec ? (normed && t - 2 < nolder) : (t - 2 - mvec < nolder);
      if (formed) {
        const double *const p = wa.part + nka_host::wide_part_index(sys, t, 0, mvec, nchunk);
        r = p[0];
        int c = 1;
        for (; c + 8 <= nchunk; c += 8) {      // (eight loads in flight; the additions stay one chain, in chunk order)
          double x[8];
#pragma unroll
          for (int u = 0; u < 8; u++) x[u] = p[c + u];
#pragma unroll
          for (int u = 0; u < 8; u++) r += x[u];
        }
        for (; c < nchunk; c++) r += p[c];
      }
    }
    red[t] = r;
  }
  __syncthreads();

  // phase 4: the scalar step on the working copy
  if (t == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);
  __syncthreads();

  // phase 5: the working copy back; the plan to the combine
  for (int i = t; i < nh; i += kBatchThreads) ctl.h()[i] = L.h[i];
  for (int i = t; i < m1 + 1; i += kBatchThreads) {
    ctl.c()[i] = L.c[i];
    ctl.next()[i] = L.next[i];
    ctl.prev()[i] = L.prev[i];
  }
  for (int i = t; i < 2 + 2 * mvec; i += kBatchThreads) ctl.red()[i] = red[i];
  if (t < hdr[HDR_NCOMB]) {
    wa.plan_c[(size_t)sys * m1 + t] = cc[t];
    wa.plan_s[(size_t)sys * m1 + t] = cs[t];
  }
}

// ---- 4: normalise the pending pair, combine, ring stores (F08:282-283, 361, 395-404) on a chunk ----
template <int COMB>
__global__ __launch_bounds__(kBatchThreads) void k_wide_combine(BatchArgs a, WideArgs wa, double *__restrict__ f_all, int64_t ld,
                                                                const int32_t *__restrict__ active) {
#pragma clang fp contract(off)
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int m1 = a.mvec + 1;
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideLds lds = nka_host::wide_combine_lds(a.mvec);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  double *const cc = shd + lds.cc;
  int32_t *const cs = shi + lds.cs, *const hdr = shi + lds.hdr;
  // the plan into LDS
  if (t == 64) hdr[HDR_NCOMB] = ctl.ic[IC_NCOMB];
  if (t == 65) hdr[HDR_NEW] = ctl.ic[IC_NEW];
  if (t == 66) hdr[HDR_NORMED] = ctl.ic[IC_NORMED];
  if (t < m1) {      // (entries beyond the plan are never applied)
    cc[t] = wa.plan_c[(size_t)sys * m1 + t];
    cs[t] = wa.plan_s[(size_t)sys * m1 + t];
  }
  __syncthreads();
  const int ncomb = hdr[HDR_NCOMB];
  const bool norm0 = hdr[HDR_NORMED] != 0;      // pair 0 of the plan is the pending pair, still raw
  const double s = norm0 ? ctl.dc[DC_S] : 0.0;
  const double rs = 1.0 / s;

  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_chunk_len(a.n, blockIdx.x);
  double *const f = f_all + (size_t)sys * ld + lo;
  double *const W = a.w + (size_t)sys * a.sys_stride + lo, *const V = a.v + (size_t)sys * a.sys_stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double *const wnew = W + (size_t)(hdr[HDR_NEW] - 1) * a.stride, *const vnew = V + (size_t)(hdr[HDR_NEW] - 1) * a.stride;
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    if (!FULL && i >= n) return;
    const d2 fin = ld_tile<FULL, FV>(f, i, n);
    d2 x = fin;
    int j0 = 0;
    if (norm0) {      // pair 0 of the plan: the pending pair, still raw (F08:282-283)
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
        vv[u] = ld_tile<FULL, true>(V + off, i, n);
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
  });
}

// ---- THE SAME FOUR KERNELS WITH PER-SYSTEM LENGTHS (nka_hip_batch_set_lengths) ----
// The system is len[sys] elements long -- one uniform scalar load behind the `active` test, a value that was validated when it was
// set: 1 <= len[sys] <= a.n --, it owns the first wide_len_nchunk(len[sys]) chunks, and a workgroup of another chunk returns
// before it reads anything else.  The partials keep the batch's nchunk as stride (wide_part_index does not change); only the
// system's own are added, in chunk order from chunk 0.  The grid stays nchunk x nsys.  Every other statement is the one of the
// kernel above: the text is WRITTEN OUT a second time because sharing it -- the four bodies as functions of a bool, called by
// both kernels -- changed the machine code of the kernels above, which are held to it (docs/design/12_batched_systems.md).
// A change to a phase is made in both places.

// ---- 1 ----
__global__ __launch_bounds__(kBatchThreads) void k_wide_norm_len(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                          const int32_t *__restrict__ active, const int32_t *__restrict__ len) {
#pragma clang fp contract(off)
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  const int64_t sn = len[sys];
  if (!nka_host::wide_len_owns(sn, blockIdx.x)) return;      // (uniform: a chunk beyond the system's own; nothing was read)
  const Ctl ctl = batch_ctl(a, sys);
  if (ctl.ic[IC_PENDING] == 0) return;      // (uniform: no pending pair, no norm -- and nobody reads this partial)
  __shared__ double sm[kBatchWaves], res[2];
  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_len_chunk_len(sn, blockIdx.x);
  const double *const f = f_all + (size_t)sys * ld + lo;
  const double *const w1 = a.w + (size_t)sys * a.sys_stride + (size_t)(ctl.ic[IC_FIRST] - 1) * a.stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double acc[1] = {};
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    const d2 fv = ld_tile<FULL, FV>(f, i, n), wv = ld_tile<FULL, true>(w1, i, n);
#pragma unroll
    for (int q = 0; q < 2; q++)
      if (FULL || i + q < n) {
        const double d = wv[q] - fv[q];
        acc[0] = fma(d, d, acc[0]);
      }
  });
  batch_block_sum<1>(acc, sm, res);
  if (threadIdx.x == 0) wa.part[nka_host::wide_part_index(sys, 0, blockIdx.x, a.mvec, wa.nchunk)] = res[0];
}

// ---- 2 ----
template <int COMB>
__global__ __launch_bounds__(kBatchThreads) void k_wide_sums_len(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                          const int32_t *__restrict__ active, const int32_t *__restrict__ len) {
#pragma clang fp contract(off)
  constexpr bool RCP = (COMB == 1);
  const int sys = blockIdx.y, chunk = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  const int64_t sn = len[sys];
  if (!nka_host::wide_len_owns(sn, chunk)) return;      // (uniform, before the first barrier)
  const int nown = (int)nka_host::wide_len_nchunk(sn);      // the partials of <d,d> that are added
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nchunk = wa.nchunk;
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideLds lds = nka_host::wide_sums_lds(mvec, nchunk);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  double *const stage = shd + lds.stage, *const sm = shd + lds.sm, *const res = shd + lds.res;
  int32_t *const next = shi + lds.next, *const ps = shi + lds.ps, *const hdr = shi + lds.hdr;

  wide_list(ctl, m1, next, ps, hdr);
  const int pending = hdr[HDR_PENDING], nolder = hdr[HDR_NOLDER];
  double s = 0.0;
  if (pending) {
    wide_norm_sum(wa.part + nka_host::wide_part_index(sys, 0, 0, mvec, nchunk), nown, stage, res + kBatchAcc);
    s = sqrt(res[kBatchAcc]);
  }
  const bool normed = pending && s != 0.0;
  const double rs = 1.0 / s;

  const int64_t lo = (int64_t)chunk * kWideChunk, n = nka_host::wide_len_chunk_len(sn, chunk);
  const double *const f = f_all + (size_t)sys * ld + lo;
  const double *const W = a.w + (size_t)sys * a.sys_stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  const double *const w1s = pending ? W + (size_t)(hdr[HDR_FIRST] - 1) * a.stride : W;      // always a stored vector
  auto out = [&](int entry) -> double & { return wa.part[nka_host::wide_part_index(sys, entry, chunk, mvec, nchunk)]; };

  const int ngroup = (nolder + kBatchGroup - 1) / kBatchGroup;
  for (int g = 0; g < (ngroup > 0 ? ngroup : (normed ? 1 : 0)); g++) {
    const double *wk[kBatchGroup];
#pragma unroll
    for (int j = 0; j < kBatchGroup; j++) {
      const int p = g * kBatchGroup + j;
      wk[j] = nolder > 0 ? W + (size_t)(ps[p < nolder ? p : nolder - 1] - 1) * a.stride : w1s;   // (beyond the list: a re-read, discarded)
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
      for (int j = 0; j < kBatchGroup; j++) wv[j] = ld_tile<FULL, true>(wk[j], i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double fq = fv[q];
          if (normed) {
            const double wn = batch_nrm<RCP>(dv[q] - fq, s, rs);
            if (g == 0) acc[2 * kBatchGroup] = fma(fq, wn, acc[2 * kBatchGroup]);
#pragma unroll
            for (int j = 0; j < kBatchGroup; j++) acc[j] = fma(wn, wv[j][q], acc[j]);
          }
#pragma unroll
          for (int j = 0; j < kBatchGroup; j++) acc[kBatchGroup + j] = fma(fq, wv[j][q], acc[kBatchGroup + j]);
        }
    });
    batch_block_sum<kBatchAcc>(acc, sm, res);
    if (t < kBatchGroup && g * kBatchGroup + t < nolder) {
      if (normed) out(2 + g * kBatchGroup + t) = res[t];
      out(2 + mvec + g * kBatchGroup + t) = res[kBatchGroup + t];
    }
    if (t == 0 && g == 0 && normed) out(1) = res[2 * kBatchGroup];
    // (res is rewritten only behind the two barriers of the next batch_block_sum)
  }
}

// ---- 3 ----
__global__ __launch_bounds__(kBatchThreads) void k_wide_scalar_len(BatchArgs a, WideArgs wa, const int32_t *__restrict__ active,
                                            const int32_t *__restrict__ len) {
#pragma clang fp contract(off)
  const int sys = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  const int nown = (int)nka_host::wide_len_nchunk(len[sys]);      // the partials that are added
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nh = (m1 + 1) * (m1 + 1), nchunk = wa.nchunk;
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideScalarLds wl = nka_host::wide_scalar_lds(mvec, nchunk);
  const nka_host::BatchLds &lds = wl.b;
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  Lst L;
  L.h = shd + lds.h;
  L.c = shd + lds.c;
  double *const red = shd + lds.red;
  double *const cc = shd + lds.cc;
  double *const res = shd + lds.res;
  double *const stage = shd + wl.stage;
  L.next = shi + lds.next;
  L.prev = shi + lds.prev;
  int32_t *const ps = shi + lds.ps;
  int32_t *const cs = shi + lds.cs;
  int32_t *const hdr = shi + lds.hdr;
  L.m1 = m1;
  L.mvec = mvec;

  // the working copy (phase 1 of k_batch_update)
  for (int i = t; i < nh; i += kBatchThreads) L.h[i] = ctl.h()[i];
  for (int i = t; i < m1 + 1; i += kBatchThreads) {
    L.c[i] = ctl.c()[i];
    L.next[i] = ctl.next()[i];
    L.prev[i] = ctl.prev()[i];
  }
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
  double s = 0.0;
  if (pending) {      // the same chunk-order sum as k_wide_sums
    wide_norm_sum(wa.part + nka_host::wide_part_index(sys, 0, 0, mvec, nchunk), nown, stage, res + kBatchAcc);
    s = sqrt(res[kBatchAcc]);
  }
  const bool normed = pending && s != 0.0;
  // red[j], one thread per entry: the chunk-order sum of the partials k_wide_sums wrote in this update, zero everywhere else
  if (t < 2 + 2 * mvec) {
    double r = 0.0;
    if (t == 0) {
      if (pending) r = res[kBatchAcc];
    } else {
      const bool formed = t == 1 ? normed : t < 2 + mvec ? (normed && t - 2 < nolder) : (t - 2 - mvec < nolder);
      if (formed) {
        const double *const p = wa.part + nka_host::wide_part_index(sys, t, 0, mvec, nchunk);
        r = p[0];
        int c = 1;
        for (; c + 8 <= nown; c += 8) {      // (eight loads in flight; the additions stay one chain, in chunk order)
          double x[8];
#pragma unroll
          for (int u = 0; u < 8; u++) x[u] = p[c + u];
#pragma unroll
          for (int u = 0; u < 8; u++) r += x[u];
        }
        for (; c < nown; c++) r += p[c];
      }
    }
    red[t] = r;
  }
  __syncthreads();

  // phase 4: the scalar step on the working copy
  if (t == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);
  __syncthreads();

  // phase 5: the working copy back; the plan to the combine
  for (int i = t; i < nh; i += kBatchThreads) ctl.h()[i] = L.h[i];
  for (int i = t; i < m1 + 1; i += kBatchThreads) {
    ctl.c()[i] = L.c[i];
    ctl.next()[i] = L.next[i];
    ctl.prev()[i] = L.prev[i];
  }
  for (int i = t; i < 2 + 2 * mvec; i += kBatchThreads) ctl.red()[i] = red[i];
  if (t < hdr[HDR_NCOMB]) {
    wa.plan_c[(size_t)sys * m1 + t] = cc[t];
    wa.plan_s[(size_t)sys * m1 + t] = cs[t];
  }
}

// ---- 4 ----
template <int COMB>
__global__ __launch_bounds__(kBatchThreads) void k_wide_combine_len(BatchArgs a, WideArgs wa, double *__restrict__ f_all, int64_t ld,
                                             const int32_t *__restrict__ active, const int32_t *__restrict__ len) {
#pragma clang fp contract(off)
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  const int64_t sn = len[sys];
  if (!nka_host::wide_len_owns(sn, blockIdx.x)) return;      // (uniform, before the first barrier)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int m1 = a.mvec + 1;
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideLds lds = nka_host::wide_combine_lds(a.mvec);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  double *const cc = shd + lds.cc;
  int32_t *const cs = shi + lds.cs, *const hdr = shi + lds.hdr;
  // the plan into LDS
  if (t == 64) hdr[HDR_NCOMB] = ctl.ic[IC_NCOMB];
  if (t == 65) hdr[HDR_NEW] = ctl.ic[IC_NEW];
  if (t == 66) hdr[HDR_NORMED] = ctl.ic[IC_NORMED];
  if (t < m1) {      // (entries beyond the plan are never applied)
    cc[t] = wa.plan_c[(size_t)sys * m1 + t];
    cs[t] = wa.plan_s[(size_t)sys * m1 + t];
  }
  __syncthreads();
  const int ncomb = hdr[HDR_NCOMB];
  const bool norm0 = hdr[HDR_NORMED] != 0;      // pair 0 of the plan is the pending pair, still raw
  const double s = norm0 ? ctl.dc[DC_S] : 0.0;
  const double rs = 1.0 / s;

  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_len_chunk_len(sn, blockIdx.x);
  double *const f = f_all + (size_t)sys * ld + lo;
  double *const W = a.w + (size_t)sys * a.sys_stride + lo, *const V = a.v + (size_t)sys * a.sys_stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double *const wnew = W + (size_t)(hdr[HDR_NEW] - 1) * a.stride, *const vnew = V + (size_t)(hdr[HDR_NEW] - 1) * a.stride;
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    if (!FULL && i >= n) return;
    const d2 fin = ld_tile<FULL, FV>(f, i, n);
    d2 x = fin;
    int j0 = 0;
    if (norm0) {      // pair 0 of the plan: the pending pair, still raw (F08:282-283)
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
        vv[u] = ld_tile<FULL, true>(V + off, i, n);
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
  });
}

// ---- THE FIRST TWO KERNELS WITH DIAGONAL DOT WEIGHTS (nka_hip_batch_create_wide_ext, nka_hip_batch_set_dot_weights) ----
// Row `sys` of the batch's weight buffer -- wgt + sys * wgt_stride, wgt_stride = 0 for the form all systems share -- is read like a
// stored vector: rows lie at the slot stride and a chunk starts on a multiple of 2048 elements, so every chunk of a weight row is
// 16-byte aligned.  fl(w_i a_i) is the FIRST operand of every product, the table of k_batch_update<..., WGT = true> (nka_batch.hip):
// <d,d> = sum fma(fl(w d), d, .), <f,w1'> = sum fma(fl(w f), w1', .), <w1',w_p> = sum fma(fl(w w1'), w_p, .), <f,w_p> = sum
// fma(fl(w f), w_p, .).  The thread -> element map, the per-thread order, batch_block_sum, the chunk-order chains and which
// partials are written are those of the kernels above.  The scalar step and the combine do not read weights: a weighted update
// launches k_wide_scalar[_len] and k_wide_combine[_len].  Each body is written ONCE, as a template on LEN -- these kernels have no
// earlier instruction stream to keep --; `len` is not read where LEN is false.  With LEN nothing at or beyond len[sys] of the weight
// row is read: the weight pair is loaded under the guards of the pair of f.

// ---- 1, weighted ----
template <bool LEN>
__global__ __launch_bounds__(kBatchThreads) void k_wide_norm_wgt(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                                                 const int32_t *__restrict__ active, const int32_t *__restrict__ len,
                                                                 const double *__restrict__ wgt, int64_t wgt_stride) {
#pragma clang fp contract(off)
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  int64_t sn = a.n;
  if constexpr (LEN) {
    sn = len[sys];
    if (!nka_host::wide_len_owns(sn, blockIdx.x)) return;      // (uniform: a chunk beyond the system's own; nothing was read)
  }
  const Ctl ctl = batch_ctl(a, sys);
  if (ctl.ic[IC_PENDING] == 0) return;      // (uniform: no pending pair, no norm -- and nobody reads this partial)
  __shared__ double sm[kBatchWaves], res[2];
  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_chunk_len(sn, blockIdx.x);
  const double *const f = f_all + (size_t)sys * (size_t)ld + lo;
  const double *const w1 = a.w + (size_t)sys * a.sys_stride + (size_t)(ctl.ic[IC_FIRST] - 1) * a.stride + lo;
  const double *const wg = wgt + (size_t)nka_host::wide_wgt_offset(sys, wgt_stride, blockIdx.x);
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double acc[1] = {};
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    const d2 fv = ld_tile<FULL, FV>(f, i, n), wv = ld_tile<FULL, true>(w1, i, n);
    const d2 gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
    for (int q = 0; q < 2; q++)
      if (FULL || i + q < n) {
        const double d = wv[q] - fv[q];
        acc[0] = fma(gv[q] * d, d, acc[0]);
      }
  });
  batch_block_sum<1>(acc, sm, res);
  if (threadIdx.x == 0) wa.part[nka_host::wide_part_index(sys, 0, blockIdx.x, a.mvec, wa.nchunk)] = res[0];
}

// ---- 2, weighted ----
template <int COMB, bool LEN>
__global__ __launch_bounds__(kBatchThreads) void k_wide_sums_wgt(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                                                 const int32_t *__restrict__ active, const int32_t *__restrict__ len,
                                                                 const double *__restrict__ wgt, int64_t wgt_stride) {
#pragma clang fp contract(off)
  constexpr bool RCP = (COMB == 1);
  const int sys = blockIdx.y, chunk = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  int64_t sn = a.n;
  if constexpr (LEN) {
    sn = len[sys];
    if (!nka_host::wide_len_owns(sn, chunk)) return;      // (uniform, before the first barrier)
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nchunk = wa.nchunk;
  const int nown = LEN ? (int)nka_host::wide_len_nchunk(sn) : nchunk;      // the partials of <d,d> that are added
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideLds lds = nka_host::wide_sums_lds(mvec, nchunk);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  double *const stage = shd + lds.stage, *const sm = shd + lds.sm, *const res = shd + lds.res;
  int32_t *const next = shi + lds.next, *const ps = shi + lds.ps, *const hdr = shi + lds.hdr;

  wide_list(ctl, m1, next, ps, hdr);
  const int pending = hdr[HDR_PENDING], nolder = hdr[HDR_NOLDER];
  double s = 0.0;
  if (pending) {
    wide_norm_sum(wa.part + nka_host::wide_part_index(sys, 0, 0, mvec, nchunk), nown, stage, res + kBatchAcc);
    s = sqrt(res[kBatchAcc]);
  }
  const bool normed = pending && s != 0.0;
  const double rs = 1.0 / s;

  const int64_t lo = (int64_t)chunk * kWideChunk, n = nka_host::wide_chunk_len(sn, chunk);
  const double *const f = f_all + (size_t)sys * (size_t)ld + lo;
  const double *const W = a.w + (size_t)sys * a.sys_stride + lo;
  const double *const wg = wgt + (size_t)nka_host::wide_wgt_offset(sys, wgt_stride, blockIdx.x);
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  const double *const w1s = pending ? W + (size_t)(hdr[HDR_FIRST] - 1) * a.stride : W;      // always a stored vector
  auto out = [&](int entry) -> double & { return wa.part[nka_host::wide_part_index(sys, entry, chunk, mvec, nchunk)]; };

  const int ngroup = (nolder + kBatchGroup - 1) / kBatchGroup;
  for (int g = 0; g < (ngroup > 0 ? ngroup : (normed ? 1 : 0)); g++) {
    const double *wk[kBatchGroup];
#pragma unroll
    for (int j = 0; j < kBatchGroup; j++) {
      const int p = g * kBatchGroup + j;
      wk[j] = nolder > 0 ? W + (size_t)(ps[p < nolder ? p : nolder - 1] - 1) * a.stride : w1s;   // (beyond the list: a re-read, discarded)
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
      for (int j = 0; j < kBatchGroup; j++) wv[j] = ld_tile<FULL, true>(wk[j], i, n);
      const d2 gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double fq = fv[q];
          const double fa = gv[q] * fq;                      // first operand of the products on f: fl(w f), formed once
          if (normed) {
            const double wn = batch_nrm<RCP>(dv[q] - fq, s, rs);
            const double wa_ = gv[q] * wn;                   // first operand of the Gram row: fl(w w1')
            if (g == 0) acc[2 * kBatchGroup] = fma(fa, wn, acc[2 * kBatchGroup]);
#pragma unroll
            for (int j = 0; j < kBatchGroup; j++) acc[j] = fma(wa_, wv[j][q], acc[j]);
          }
#pragma unroll
          for (int j = 0; j < kBatchGroup; j++) acc[kBatchGroup + j] = fma(fa, wv[j][q], acc[kBatchGroup + j]);
        }
    });
    batch_block_sum<kBatchAcc>(acc, sm, res);
    if (t < kBatchGroup && g * kBatchGroup + t < nolder) {
      if (normed) out(2 + g * kBatchGroup + t) = res[t];
      out(2 + mvec + g * kBatchGroup + t) = res[kBatchGroup + t];
    }
    if (t == 0 && g == 0 && normed) out(1) = res[2 * kBatchGroup];
    // (res is rewritten only behind the two barriers of the next batch_block_sum)
  }
}

// (whether an update runs with per-system lengths or weights, in which form, and the buffers' addresses are fixed when it is
// enqueued or captured; the values are read when it runs.  The grid is nchunk x nsys either way, so the host needs no length to
// launch)
template <int COMB>
void launch_wide(nka_hip_batch_t b, const WideArgs &wa, double *f, int64_t ld, const int32_t *active) {
  const int mvec = b->k.mvec, nchunk = b->nchunk;
  const dim3 grid((unsigned)nchunk, (unsigned)b->k.nsys), block(kBatchThreads);
  if (b->weighted) {      // (only a batch of nka_hip_batch_create_wide_ext can be: every other wide batch refuses the setters)
    const int32_t *const len = b->has_len ? b->len : nullptr;
    const double *const wgt = b->wgt;
    const int64_t ws = b->wgt_stride;
    const size_t lsums = nka_host::wide_sums_lds(mvec, nchunk).bytes(), lscal = nka_host::wide_scalar_lds(mvec, nchunk).b.bytes(),
                 lcomb = nka_host::wide_combine_lds(mvec).bytes();
    if (len) {
      hipLaunchKernelGGL(k_wide_norm_wgt<true>, grid, block, 0, b->stream, b->k, wa, (const double *)f, ld, active, len, wgt, ws);
      hipLaunchKernelGGL((k_wide_sums_wgt<COMB, true>), grid, block, lsums, b->stream, b->k, wa, (const double *)f, ld, active, len, wgt, ws);
      hipLaunchKernelGGL(k_wide_scalar_len, dim3((unsigned)b->k.nsys), block, lscal, b->stream, b->k, wa, active, len);
      hipLaunchKernelGGL((k_wide_combine_len<COMB>), grid, block, lcomb, b->stream, b->k, wa, f, ld, active, len);
    } else {
      hipLaunchKernelGGL(k_wide_norm_wgt<false>, grid, block, 0, b->stream, b->k, wa, (const double *)f, ld, active, len, wgt, ws);
      hipLaunchKernelGGL((k_wide_sums_wgt<COMB, false>), grid, block, lsums, b->stream, b->k, wa, (const double *)f, ld, active, len, wgt, ws);
      hipLaunchKernelGGL(k_wide_scalar, dim3((unsigned)b->k.nsys), block, lscal, b->stream, b->k, wa, active);
      hipLaunchKernelGGL((k_wide_combine<COMB>), grid, block, lcomb, b->stream, b->k, wa, f, ld, active);
    }
    return;
  }
  if (b->has_len) {
    const int32_t *const len = b->len;
    hipLaunchKernelGGL(k_wide_norm_len, grid, block, 0, b->stream, b->k, wa, (const double *)f, ld, active, len);
    hipLaunchKernelGGL((k_wide_sums_len<COMB>), grid, block, nka_host::wide_sums_lds(mvec, nchunk).bytes(), b->stream, b->k, wa,
                       (const double *)f, ld, active, len);
    hipLaunchKernelGGL(k_wide_scalar_len, dim3((unsigned)b->k.nsys), block, nka_host::wide_scalar_lds(mvec, nchunk).b.bytes(), b->stream,
                       b->k, wa, active, len);
    hipLaunchKernelGGL((k_wide_combine_len<COMB>), grid, block, nka_host::wide_combine_lds(mvec).bytes(), b->stream, b->k, wa, f, ld, active,
                       len);
    return;
  }
  hipLaunchKernelGGL(k_wide_norm, grid, block, 0, b->stream, b->k, wa, (const double *)f, ld, active);
  hipLaunchKernelGGL((k_wide_sums<COMB>), grid, block, nka_host::wide_sums_lds(mvec, nchunk).bytes(), b->stream, b->k, wa, (const double *)f,
                     ld, active);
  hipLaunchKernelGGL(k_wide_scalar, dim3((unsigned)b->k.nsys), block, nka_host::wide_scalar_lds(mvec, nchunk).b.bytes(), b->stream, b->k, wa,
                     active);
  hipLaunchKernelGGL((k_wide_combine<COMB>), grid, block, nka_host::wide_combine_lds(mvec).bytes(), b->stream, b->k, wa, f, ld, active);
}

}  // namespace

int nka_batch_wide_alloc(nka_hip_batch_t b) {
  const int m1 = b->k.mvec + 1;
  b->nchunk = (int32_t)nka_host::wide_nchunk(b->k.n);
  const size_t npart = (size_t)nka_host::wide_part_count(b->k.nsys, b->k.mvec, b->nchunk), nplan = (size_t)b->k.nsys * m1;
  HIP_TRY(hipMalloc((void **)&b->part, sizeof(double) * npart));
  HIP_TRY(hipMalloc((void **)&b->plan_c, sizeof(double) * nplan));
  HIP_TRY(hipMalloc((void **)&b->plan_s, sizeof(int32_t) * nplan));
  HIP_TRY(hipMemsetAsync(b->part, 0, sizeof(double) * npart, b->stream));
  HIP_TRY(hipMemsetAsync(b->plan_c, 0, sizeof(double) * nplan, b->stream));
  HIP_TRY(hipMemsetAsync(b->plan_s, 0, sizeof(int32_t) * nplan, b->stream));
  return 0;
}

void nka_batch_wide_free(nka_hip_batch_t b) {
  hipFree(b->part);
  hipFree(b->plan_c);
  hipFree(b->plan_s);
  b->part = b->plan_c = nullptr;
  b->plan_s = nullptr;
}

void nka_batch_wide_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active) {
  const WideArgs wa{b->part, b->plan_c, b->plan_s, b->nchunk};
  switch (b->flavor) {
    case NKA_HIP_FLAVOR_F08_VECTOR: launch_wide<1>(b, wa, f, ld, active); break;
    case NKA_HIP_FLAVOR_C: launch_wide<2>(b, wa, f, ld, active); break;
    default: launch_wide<0>(b, wa, f, ld, active);
  }
}

extern "C" int nka_hip_batch_wide_limits(int64_t *chunk, int64_t *max_vlen) {
  if (chunk) *chunk = kWideChunk;
  if (max_vlen) *max_vlen = std::min<int64_t>(NKA_HIP_BATCH_WIDE_MAX_VLEN, nka_host::kWideMaxChunks * kWideChunk);
  return 0;
}
