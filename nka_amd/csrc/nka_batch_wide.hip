// nka_batch_wide.hip -- the WIDE batched accelerator (nka_hip_batch_create_wide, _wide_step, _wide_ext, _wide_stored; include/nka_hip_batch.h):
// nsys independent NKA states of equal shape, each split into nchunk chunks of NKA_HIP_BATCH_WIDE_CHUNK elements with ONE WORKGROUP
// PER CHUNK (blockIdx.x = chunk, blockIdx.y = system).  The phases of k_batch_update (nka_batch.hip) that need a sum over the whole
// system are separated by KERNEL BOUNDARIES instead of workgroup barriers -- an update is four launches in a line, a solve step
// (STEP: residual norm, stop rule and x -= f_out on the device) the same four:
//   k_wide_norm      phase 2 on a chunk: sum d^2 of the chunk -> part[sys][0][chunk].  STEP: k_wide_step_norm in its place: <f,f> of
//                    the chunk in the same sweep -> fpart[sys][chunk]; without a pending pair f is swept alone
//   k_wide_sums      STEP: r = sqrt(fpart[sys][0] + fpart[sys][1] + ...), the same bits in every workgroup of the system; r <=
//                    tol[sys]: the workgroup returns, nothing written (NOT active[sys]: other workgroups of this launch read it).
//                    s = sqrt(part[sys][0][0] + part[sys][0][1] + ...), the same bits likewise; phase 3 on a chunk ->
//                    part[sys][1 ...][chunk]
//   k_wide_scalar    one workgroup per system.  STEP: r again; fnorm[sys] = r; r <= tol[sys]: active[sys] = 0 and return -- the
//                    only workgroup of its launch that reads or writes the entry.  red[j] = the chunk-order sum of entry j's
//                    partials; phases 4 and 5; the plan
//   k_wide_combine   active[sys] (STEP: now 0 for a system that retired); phase 6 on a chunk.  STEP: x = fl(x - f_out)
// Within a launch no workgroup reads what another writes: no flags, no spinning, no atomics, no cooperative launch.  A chunk
// is whole tiles of 512 elements, so inside a chunk the element -> thread map, the per-thread order, the 16-byte alignment of
// the stored vectors and the parity of a row of f are those of the narrow kernel: a wide batch of ONE chunk returns the
// narrow batch's bits.  Which partials a kernel reads is decided from the list (pending, normed, nolder), never from what the
// buffer holds: a partial that this update did not write is not read.
// FIVE KERNEL TEMPLATES, 68 INSTANCES: norm 8 + 4, sums 32, scalar 8, combine 16 (20 of them with binary32 storage).  What an
// instance takes beside the update's arguments rides in THE TRAILING PACK [WideStepArgs][, LenRows][, Store32Args][, WgtRows,
// WgtStride] (below), so an instance without a member keeps its arguments.  The step's norm alone is a kernel of its own, k_wide_step_norm<LEN, [WgtRows, WgtStride]>: folded into
// k_wide_norm it was measured slower than before.
//   LENGTHS  (nka_hip_batch_set_lengths) The system is len[sys] elements long -- one uniform scalar load behind the `active` test,
//            a value that was validated when it was set: 1 <= len[sys] <= a.n --, it owns the first wide_len_nchunk(len[sys])
//            chunks, and a workgroup of another chunk returns before it reads anything else.  The partials keep the batch's nchunk
//            as stride (wide_part_index does not change); only the system's own are added, in chunk order from chunk 0.  The grid
//            stays nchunk x nsys.
//   WEIGHTS  (nka_hip_batch_create_wide_ext, nka_hip_batch_set_dot_weights) Row `sys` of the batch's weight buffer -- rows + sys *
//            stride, stride = 0 for the form all systems share -- is read like a stored vector in the norm and the sums: rows lie at
//            the slot stride and a chunk starts on a multiple of 2048 elements, so every chunk of a weight row is 16-byte aligned.
//            fl(w_i a_i) is the FIRST operand of every product, the table of k_batch_update<..., WGT = true> (nka_batch.hip):
//            <f,f> = sum fma(fl(w f), f, .), <d,d> = sum fma(fl(w d), d, .), <f,w1'> = sum fma(fl(w f), w1', .), <w1',w_p> = sum
//            fma(fl(w w1'), w_p, .), <f,w_p> = sum fma(fl(w f), w_p, .).  The weight pair is loaded under the guards of the pair of
//            f: with lengths nothing at or beyond len[sys] of the weight row is read.  The scalar kernel and the combine do not
//            read weights and never take them.
//   STORAGE  (nka_hip_batch_create_wide_stored with NKA_HIP_BATCH_STORE_F32; flavour C only) A Store32Args in the pack makes the
//            instance one of BINARY32 STORAGE, the statements of k_batch_update<..., Store32Args> (nka_batch.hip) per chunk: a.w / a.v
//            are float allocations of the same strides in elements, an older vector is one 8-byte load widened exactly (a chunk
//            starts on a multiple of 2048 elements, so a float pair is 8-byte aligned), the raw pending pair is read from and written
//            to the binary64 rows pw / pv + sys * stride, and the normalised pair is narrowed once -- w1' = q(fl(d/s)) in the sums and
//            the combine alike, v = q(fl(fl(v1/s) - w1')) -- before it is used or stored.  The two norm kernels read binary64 data
//            only: the launch gives them the pending buffer as a.w (launch_wide), the step's norm runs its binary64 instances, and
//            k_wide_norm and k_wide_scalar take the member with the pack without reading it.  Without the member every such
//            statement is discarded at compile time and the instance is the one it was, instruction for instruction.
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
static_assert(nka_host::wide_scalar_rows_lds(NKA_HIP_BATCH_MAX_MVEC, nka_host::kWideMaxChunks).b.bytes() <= 64 * 1024, "... with the wavefront step: no function attribute");
static_assert(NKA_HIP_BATCH_MAX_MVEC + 1 <= nka_host::kWideRowsMaxList, "the wavefront step holds every list a batch can have");

struct WideArgs {
  double *part;         // nka_host::wide_part_index
  double *plan_c;       // combine plan of system sys: plan_c + sys * (mvec + 1), plan_s likewise
  int32_t *plan_s;
  int32_t nchunk;
};

// THE TRAILING PACK of the kernels: [WideStepArgs][, LenRows][, Store32Args][, WgtRows, WgtStride], each at most once, in this order
// (Store32Args, WgtRows and WgtStride: nka_batch_dev.hpp; the scalar kernel and the combine never take the weights, k_wide_norm
// never the step's arguments).
// what a solve step takes beside the update's arguments; every pointer but fpart may be NULL
struct WideStepArgs {
  double *fpart;        // nka_host::wide_fpart_index: the partials of <f,f>
  double *x;            // the iterate, nsys rows ldx apart
  int64_t ldx;
  const double *tol;    // per-system thresholds on r (read in launches 2 and 3)
  double *fnorm;        // per-system r out (written in launch 3)
};
// the batch's buffer of nsys validated lengths: a kernel argument of its own, so that it is __restrict__ like `active`
using LenRows = const int32_t *__restrict__;
// ... and what k_wide_step_norm takes in their place: the step's arguments with the lengths behind them (NULL where LEN is false)
struct WideStepLenArgs : WideStepArgs {
  const int32_t *len;
};
// THE SCALAR STEP ON ONE WAVEFRONT (nka_hip_batch_set_scalar_step): an empty member, the LAST of the pack and taken by k_wide_scalar
// alone; NLMAX: the rows batch_scalar_step_rows<NLMAX> holds in registers, >= mvec + 1 (nka_host::wide_rows_nlmax)
template <int NLMAX> struct WideRows {};
template <class T> struct wide_rows_of { static constexpr int value = 0; };
template <int NLMAX> struct wide_rows_of<WideRows<NLMAX>> { static constexpr int value = NLMAX; };
template <class... Pack> constexpr int wide_rows_nl = (0 + ... + wide_rows_of<Pack>::value);      // 0: the one-thread step
template <class T, class... Pack> constexpr bool wide_has = (std::is_same<Pack, T>::value || ...);
template <class T>
constexpr int wide_pack_rank = std::is_same<T, WideStepArgs>::value ? 0 : std::is_same<T, LenRows>::value ? 1 : std::is_same<T, Store32Args>::value ? 2
                               : std::is_same<T, WgtRows>::value ? 3 : std::is_same<T, WgtStride>::value ? 4 : wide_rows_of<T>::value > 0 ? 5 : -1;
// LDS of the scalar kernel: with the matrix of the wavefront step where ROWS (host_logic.hpp)
template <bool ROWS> __host__ __device__ constexpr auto wide_scalar_layout(int mvec, int nchunk) {
  if constexpr (ROWS) return nka_host::wide_scalar_rows_lds(mvec, nchunk); else return nka_host::wide_scalar_lds(mvec, nchunk);
}
template <class... Pack> constexpr bool wide_pack_ok() {      // known members only, ranks strictly increasing, the weights as a pair
  int prev = -1;
  bool ok = true;
  ((ok = ok && wide_pack_rank<Pack> > prev, prev = wide_pack_rank<Pack>), ...);
  return ok && wide_has<WgtRows, Pack...> == wide_has<WgtStride, Pack...>;
}

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

// a sum of a system (<d,d>, the step's <f,f>) from its nchunk partials in CHUNK ORDER, starting from part0[0] -- staged into LDS
// by the whole workgroup, added by one thread.  Every workgroup that calls this for a system forms the same bits.  *out is valid
// after the trailing barrier; stage and *out may be reused behind it.
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

// ---- 1: the norm (F08:266-267) of a chunk (an update; Pack: [LenRows][, WgtRows, WgtStride]) ----
template <class... Pack>
__global__ __launch_bounds__(kBatchThreads) void k_wide_norm(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                                             const int32_t *__restrict__ active, Pack... pack) {
#pragma clang fp contract(off)
  constexpr bool LEN = wide_has<LenRows, Pack...>, WGT = wide_has<WgtRows, Pack...>;
  // (a Store32Args is taken and not read: the launch gives such an instance the pending rows as a.w, see launch_wide)
  static_assert(wide_pack_ok<Pack...>() && !wide_has<WideStepArgs, Pack...>, "[LenRows][, Store32Args][, WgtRows, WgtStride]: a step's norm is k_wide_step_norm");
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  int64_t sn = a.n;
  if constexpr (LEN) {
    sn = pack_get<LenRows>(pack...)[sys];
    if (!nka_host::wide_len_owns(sn, blockIdx.x)) return;      // (uniform: a chunk beyond the system's own; nothing was read)
  }
  const Ctl ctl = batch_ctl(a, sys);
  if (ctl.ic[IC_PENDING] == 0) return;      // (uniform: no pending pair, no norm -- and nobody reads this partial)
  __shared__ double sm[kBatchWaves], res[2];
  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_chunk_len(sn, blockIdx.x);
  const double *const f = f_all + (size_t)sys * (size_t)ld + lo;
  const double *const w1 = a.w + (size_t)sys * a.sys_stride + (size_t)(ctl.ic[IC_FIRST] - 1) * a.stride + lo;
  [[maybe_unused]] const double *wg = nullptr;      // this chunk of the system's weight row
  if constexpr (WGT) wg = pack_get<WgtRows>(pack...) + (size_t)nka_host::wide_wgt_offset(sys, (int64_t)pack_get<WgtStride>(pack...), blockIdx.x);
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double acc[1] = {};
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    const d2 fv = ld_tile<FULL, FV>(f, i, n), wv = ld_tile<FULL, true>(w1, i, n);
    [[maybe_unused]] d2 gv;
    if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
    for (int q = 0; q < 2; q++)
      if (FULL || i + q < n) {
        const double d = wv[q] - fv[q];
        if constexpr (WGT) acc[0] = fma(gv[q] * d, d, acc[0]); else acc[0] = fma(d, d, acc[0]);
      }
  });
  batch_block_sum<1>(acc, sm, res);
  if (threadIdx.x == 0) wa.part[nka_host::wide_part_index(sys, 0, blockIdx.x, a.mvec, wa.nchunk)] = res[0];
}

// ---- 1, STEP: <f,f> of a chunk, and the norm of the chunk beside it.  A kernel of its own, with the step's arguments and the
// lengths where they were before the wide kernels became templates on a pack (st in front of f_all, len inside it, read where LEN)
// and only the weights behind `active`: as an instance of k_wide_norm it was measured slower (docs/design/12_batched_systems.md,
// "One wide unit") ----
template <bool LEN, class... Wgt>
__global__ __launch_bounds__(kBatchThreads) void k_wide_step_norm(BatchArgs a, WideArgs wa, WideStepLenArgs st, const double *__restrict__ f_all,
                                                                  int64_t ld, const int32_t *__restrict__ active, Wgt... wgt) {
#pragma clang fp contract(off)
  constexpr bool WGT = wide_has<WgtRows, Wgt...>;
  static_assert(wide_pack_ok<Wgt...>() && sizeof...(Wgt) == (WGT ? 2 : 0), "[WgtRows, WgtStride]");
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;
  int64_t sn = a.n;
  if constexpr (LEN) {
    sn = st.len[sys];
    if (!nka_host::wide_len_owns(sn, blockIdx.x)) return;      // (uniform: a chunk beyond the system's own; nothing was read)
  }
  const Ctl ctl = batch_ctl(a, sys);
  __shared__ double sm[2 * kBatchWaves], res[2];
  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_chunk_len(sn, blockIdx.x);
  const double *const f = f_all + (size_t)sys * (size_t)ld + lo;
  [[maybe_unused]] const double *wg = nullptr;      // this chunk of the system's weight row
  if constexpr (WGT) wg = pack_get<WgtRows>(wgt...) + (size_t)nka_host::wide_wgt_offset(sys, (int64_t)pack_get<WgtStride>(wgt...), blockIdx.x);
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  double *const fp = st.fpart + nka_host::wide_fpart_index(sys, blockIdx.x, wa.nchunk);
  if (ctl.ic[IC_PENDING] != 0) {      // (uniform)
    const double *const w1 = a.w + (size_t)sys * a.sys_stride + (size_t)(ctl.ic[IC_FIRST] - 1) * a.stride + lo;
    double acc[2] = {};
    batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
      constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
      const d2 fv = ld_tile<FULL, FV>(f, i, n), wv = ld_tile<FULL, true>(w1, i, n);
      [[maybe_unused]] d2 gv;
      if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double d = wv[q] - fv[q];
          if constexpr (WGT) acc[1] = fma(gv[q] * d, d, acc[1]); else acc[1] = fma(d, d, acc[1]);
          if constexpr (WGT) acc[0] = fma(gv[q] * fv[q], fv[q], acc[0]); else acc[0] = fma(fv[q], fv[q], acc[0]);
        }
    });
    batch_block_sum<2>(acc, sm, res);
    if (threadIdx.x == 0) {
      *fp = res[0];
      wa.part[nka_host::wide_part_index(sys, 0, blockIdx.x, a.mvec, wa.nchunk)] = res[1];
    }
  } else {      // no pending pair (first update, after a restart): f is swept alone, the weights ride along
    double acc[1] = {};
    batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
      constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
      const d2 fv = ld_tile<FULL, FV>(f, i, n);
      [[maybe_unused]] d2 gv;
      if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          if constexpr (WGT) acc[0] = fma(gv[q] * fv[q], fv[q], acc[0]); else acc[0] = fma(fv[q], fv[q], acc[0]);
        }
    });
    batch_block_sum<1>(acc, sm, res);
    if (threadIdx.x == 0) *fp = res[0];
  }
}

// ---- 2: STEP: the stop rule, read only; every other sum of a chunk, on the rounded w1' (F08:286-290, 371) ----
template <int COMB, class... Pack>
__global__ __launch_bounds__(kBatchThreads) void k_wide_sums(BatchArgs a, WideArgs wa, const double *__restrict__ f_all, int64_t ld,
                                                             const int32_t *__restrict__ active, Pack... pack) {
#pragma clang fp contract(off)
  constexpr bool STEP = wide_has<WideStepArgs, Pack...>, LEN = wide_has<LenRows, Pack...>, WGT = wide_has<WgtRows, Pack...>;
  constexpr bool S32 = wide_has<Store32Args, Pack...>;
  static_assert(wide_pack_ok<Pack...>(), "[WideStepArgs][, LenRows][, Store32Args][, WgtRows, WgtStride]");
  static_assert(!S32 || COMB == 2, "binary32 storage: the default flavour only");
  constexpr bool RCP = (COMB == 1);
  const int sys = blockIdx.y, chunk = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  int64_t sn = a.n;
  if constexpr (LEN) {
    sn = pack_get<LenRows>(pack...)[sys];
    if (!nka_host::wide_len_owns(sn, chunk)) return;      // (uniform, before the first barrier)
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nchunk = wa.nchunk;
  const int nown = LEN ? (int)nka_host::wide_len_nchunk(sn) : nchunk;      // the partials that are added
  const Ctl ctl = batch_ctl(a, sys);
  const nka_host::WideLds lds = nka_host::wide_sums_lds(mvec, nchunk);
  double *const shd = reinterpret_cast<double *>(smem);
  int32_t *const shi = reinterpret_cast<int32_t *>(shd + lds.ndouble);
  double *const stage = shd + lds.stage, *const sm = shd + lds.sm, *const res = shd + lds.res;
  int32_t *const next = shi + lds.next, *const ps = shi + lds.ps, *const hdr = shi + lds.hdr;

  // STEP: r from LDS behind a barrier, tol[sys] written by nobody during this launch: the return is uniform, and nothing has been
  // written.  active[sys] stays as it is -- the other workgroups of the system read it --; k_wide_scalar clears it.
  if constexpr (STEP) {
    const WideStepArgs st = pack_get<WideStepArgs>(pack...);
    wide_norm_sum(st.fpart + nka_host::wide_fpart_index(sys, 0, nchunk), nown, stage, res + kBatchAcc);
    const double r = sqrt(res[kBatchAcc]);
    if (st.tol != nullptr && r <= st.tol[sys]) return;      // (a NaN on either side: false, the system goes on)
  }

  wide_list(ctl, m1, next, ps, hdr);      // (its barriers lie between the read of res above and the next write of it)
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
  [[maybe_unused]] const double *wg = nullptr;      // this chunk of the system's weight row
  if constexpr (WGT) wg = pack_get<WgtRows>(pack...) + (size_t)nka_host::wide_wgt_offset(sys, (int64_t)pack_get<WgtStride>(pack...), blockIdx.x);
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  // binary32 storage: this chunk of the system's float slots, and of its row of the pending buffer where the raw w1 lies
  [[maybe_unused]] const float *W32 = nullptr;
  [[maybe_unused]] const double *pw = nullptr;
  if constexpr (S32) {
    W32 = reinterpret_cast<const float *>(a.w) + (size_t)sys * a.sys_stride + lo;
    pw = pack_get<Store32Args>(pack...).pw + (size_t)sys * a.stride + lo;
  }
  const double *const w1s = S32 ? pw : pending ? W + (size_t)(hdr[HDR_FIRST] - 1) * a.stride : W;      // always a stored vector
  auto out = [&](int entry) -> double & { return wa.part[nka_host::wide_part_index(sys, entry, chunk, mvec, nchunk)]; };

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
      [[maybe_unused]] d2 gv;
      if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (FULL || i + q < n) {
          const double fq = fv[q];
          double fa = fq;                                    // first operand of the products on f: fl(w f), formed once
          if constexpr (WGT) fa = gv[q] * fq;
          if (normed) {
            double wn = batch_nrm<RCP>(dv[q] - fq, s, rs);
            if constexpr (S32) wn = batch_q32(wn);           // (binary32 storage: the value the slot will hold)
            double wa_ = wn;                                 // first operand of the Gram row: fl(w w1')
            if constexpr (WGT) wa_ = gv[q] * wn;
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

// ---- 3: STEP: fnorm, the stop rule and the mask; the sums of the system from its partials, the scalar step, the plan; one
// workgroup per system.  Mask: const int32_t, or int32_t in a step, which clears the entry ----
template <class Mask, class... Pack>
__global__ __launch_bounds__(kBatchThreads) void k_wide_scalar(BatchArgs a, WideArgs wa, Mask *__restrict__ active, Pack... pack) {
#pragma clang fp contract(off)
  constexpr bool STEP = wide_has<WideStepArgs, Pack...>, LEN = wide_has<LenRows, Pack...>;
  constexpr bool S32 = wide_has<Store32Args, Pack...>;      // (taken with the pack and not read: this kernel touches no stored vector)
  constexpr int ROWS = wide_rows_nl<Pack...>;      // > 0: phase 4 on wavefront 0 (batch_scalar_step_rows<ROWS>), the matrix in LDS
  static_assert(wide_pack_ok<Pack...>() && sizeof...(Pack) == (STEP ? 1 : 0) + (LEN ? 1 : 0) + (S32 ? 1 : 0) + (ROWS > 0 ? 1 : 0) &&
                    STEP == !std::is_const<Mask>::value,
                "[WideStepArgs][, LenRows][, Store32Args][, WideRows<NLMAX>]: the weights are not taken; a step, and only a step, writes the mask");
  const int sys = blockIdx.x;
  if (active != nullptr && active[sys] == 0) return;
  int nown = wa.nchunk;      // the partials that are added
  if constexpr (LEN) nown = (int)nka_host::wide_len_nchunk(pack_get<LenRows>(pack...)[sys]);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x;
  const int mvec = a.mvec, m1 = mvec + 1, nh = (m1 + 1) * (m1 + 1), nchunk = wa.nchunk;
  const Ctl ctl = batch_ctl(a, sys);
  const auto wl = wide_scalar_layout<(ROWS > 0)>(mvec, nchunk);
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

  // STEP: the same chunk-order sum as k_wide_sums, hence the same decision.  This workgroup is the only one of its launch that
  // reads or writes active[sys]; the return is uniform, and of the system's state nothing has been written.
  if constexpr (STEP) {
    const WideStepArgs st = pack_get<WideStepArgs>(pack...);
    wide_norm_sum(st.fpart + nka_host::wide_fpart_index(sys, 0, nchunk), nown, stage, res + kBatchAcc);
    const double r = sqrt(res[kBatchAcc]);
    if (t == 0 && st.fnorm != nullptr) st.fnorm[sys] = r;
    if (st.tol != nullptr && r <= st.tol[sys]) {      // (a NaN on either side: false, the system goes on)
      if (t == 0) active[sys] = 0;
      return;
    }
  }

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
  // red[j], one thread per entry: the chunk-order sum of the partials k_wide_sums wrote in this call, zero everywhere else
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

  // phase 4: the scalar step on the working copy -- one thread, or wavefront 0 while the other three wait at the barrier
  if constexpr (ROWS > 0) {
    if (t < 64) batch_scalar_step_rows<ROWS>(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr, shd + wl.a);
  } else {
    if (t == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);
  }
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

// ---- 4: normalise the pending pair, combine, ring stores (F08:282-283, 361, 395-404) on a chunk; STEP: x = fl(x - f_out) ----
template <int COMB, class... Pack>
__global__ __launch_bounds__(kBatchThreads) void k_wide_combine(BatchArgs a, WideArgs wa, double *__restrict__ f_all, int64_t ld,
                                                                const int32_t *__restrict__ active, Pack... pack) {
#pragma clang fp contract(off)
  constexpr bool STEP = wide_has<WideStepArgs, Pack...>, LEN = wide_has<LenRows, Pack...>;
  constexpr bool S32 = wide_has<Store32Args, Pack...>;
  static_assert(wide_pack_ok<Pack...>() && sizeof...(Pack) == (STEP ? 1 : 0) + (LEN ? 1 : 0) + (S32 ? 1 : 0),
                "[WideStepArgs][, LenRows][, Store32Args]: the weights are not taken");
  static_assert(!S32 || COMB == 2, "binary32 storage: the default flavour only");
  constexpr bool RCP = (COMB == 1);
  constexpr bool COMPACT = (COMB == 2);
  const int sys = blockIdx.y;
  if (active != nullptr && active[sys] == 0) return;      // (STEP: a system that retired in this step was cleared by the launch before)
  int64_t sn = a.n;
  if constexpr (LEN) {
    sn = pack_get<LenRows>(pack...)[sys];
    if (!nka_host::wide_len_owns(sn, blockIdx.x)) return;      // (uniform, before the first barrier)
  }
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

  const int64_t lo = (int64_t)blockIdx.x * kWideChunk, n = nka_host::wide_chunk_len(sn, blockIdx.x);
  double *const f = f_all + (size_t)sys * ld + lo;
  double *const W = a.w + (size_t)sys * a.sys_stride + lo, *const V = a.v + (size_t)sys * a.sys_stride + lo;
  const bool fvec = (reinterpret_cast<uintptr_t>(f) % 16) == 0;
  // binary32 storage: this chunk of the system's float slots and of its rows of the pending buffers, where the new raw pair goes
  [[maybe_unused]] float *W32 = nullptr, *V32 = nullptr;
  [[maybe_unused]] double *pw = nullptr, *pv = nullptr;
  if constexpr (S32) {
    W32 = reinterpret_cast<float *>(a.w) + (size_t)sys * a.sys_stride + lo;
    V32 = reinterpret_cast<float *>(a.v) + (size_t)sys * a.sys_stride + lo;
    pw = pack_get<Store32Args>(pack...).pw + (size_t)sys * a.stride + lo;
    pv = pack_get<Store32Args>(pack...).pv + (size_t)sys * a.stride + lo;
  }
  double *const wnew = S32 ? pw : W + (size_t)(hdr[HDR_NEW] - 1) * a.stride, *const vnew = S32 ? pv : V + (size_t)(hdr[HDR_NEW] - 1) * a.stride;
  // STEP: this chunk of the system's row of the iterate, if there is one; a chunk starts on a multiple of 16 bytes of its row
  [[maybe_unused]] double *xrow = nullptr;
  if constexpr (STEP) {
    const WideStepArgs st = pack_get<WideStepArgs>(pack...);
    xrow = st.x != nullptr ? st.x + (size_t)sys * st.ldx + lo : nullptr;
  }
  [[maybe_unused]] const bool xvec = (reinterpret_cast<uintptr_t>(xrow) % 16) == 0;
  batch_sweep(n, fvec, [&](auto full, auto fv_, int64_t i) {
    constexpr bool FULL = decltype(full)::value, FV = decltype(fv_)::value;
    if (!FULL && i >= n) return;
    const d2 fin = ld_tile<FULL, FV>(f, i, n);
    d2 x = fin;
    [[maybe_unused]] d2 xit = {0.0, 0.0};      // STEP: the iterate's pair, loaded with the other loads of the tile
    if constexpr (STEP)
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
        xit[0] = xit[0] - x[0];
        xit[1] = xit[1] - x[1];
        if (xvec) st_tile<FULL, true>(xrow, i, n, xit); else st_tile<FULL, false>(xrow, i, n, xit);
      }
  });
}

// THE LAUNCH LADDER: flavour -> lengths? -> the four launches, the first two with the weights where the batch is weighted (only a
// batch of nka_hip_batch_create_wide_ext can be: every other wide batch refuses the setters).  The pack's types are named
// throughout: deduction would drop their __restrict__.  (Whether a call runs with per-system lengths or weights, in which form,
// and every address are fixed when it is enqueued or captured; the values are read when it runs.  The grid is nchunk x nsys
// either way, so the host needs no length to launch.)
// THE THIRD LAUNCH WITH THE WAVEFRONT STEP (b->scalar_step): Pack: [WideStepArgs][, LenRows] -- a Store32Args is not passed on, the
// scalar kernel never read it --, the instance by mvec, which is fixed at creation: a captured call stays valid
template <class Mask, int NLMAX, class... Pack>
void launch_wide_scalar_rows_nl(nka_hip_batch_t b, const WideArgs &wa, Mask *active, Pack... pack) {
  const size_t lds = nka_host::wide_scalar_rows_lds(b->k.mvec, b->nchunk).b.bytes();
  // (the chevron form of the same launch: the eight hipLaunchKernelGGL statements of this unit stay the four launches of launch_wide in
  // their two forms, which tests/test_batch_wide_weights_cpu.py counts)
  k_wide_scalar<Mask, Pack..., WideRows<NLMAX>><<<dim3((unsigned)b->k.nsys), dim3(kBatchThreads), lds, b->stream>>>(b->k, wa, active, pack...,
                                                                                                             WideRows<NLMAX>{});
}
template <class Mask, class... Pack>
void launch_wide_scalar_rows(nka_hip_batch_t b, const WideArgs &wa, Mask *active, Pack... pack) {
  switch (nka_host::wide_rows_nlmax(b->k.mvec)) {
    case 6: launch_wide_scalar_rows_nl<Mask, 6, Pack...>(b, wa, active, pack...); break;
    case 11: launch_wide_scalar_rows_nl<Mask, 11, Pack...>(b, wa, active, pack...); break;
    case 21: launch_wide_scalar_rows_nl<Mask, 21, Pack...>(b, wa, active, pack...); break;
    default: launch_wide_scalar_rows_nl<Mask, nka_host::kWideRowsMaxList, Pack...>(b, wa, active, pack...);
  }
}
// Pack: [WideStepArgs][, LenRows], what all four kernels take; Mask: the scalar kernel's
template <int COMB, class Mask, class... Pack>
void launch_wide(nka_hip_batch_t b, double *f, int64_t ld, Mask *active, Pack... pack) {
  const WideArgs wa{b->part, b->plan_c, b->plan_s, b->nchunk};
  const int mvec = b->k.mvec, nchunk = b->nchunk;
  const dim3 grid((unsigned)nchunk, (unsigned)b->k.nsys), block(kBatchThreads);
  const size_t lsums = nka_host::wide_sums_lds(mvec, nchunk).bytes(), lscal = nka_host::wide_scalar_lds(mvec, nchunk).b.bytes(),
               lcomb = nka_host::wide_combine_lds(mvec).bytes();
  const double *const cf = f;
  const int32_t *const mask = active;
  constexpr bool STEP = wide_has<WideStepArgs, Pack...>, LEN = wide_has<LenRows, Pack...>;
  // binary32 storage: both norm kernels read binary64 data only, f and the raw w1 of the system's pending row -- they get the
  // pending buffer as `w`, its row stride as the stride between systems and 0 between slots, and form the address they always did
  BatchArgs kn = b->k;
  if constexpr (wide_has<Store32Args, Pack...>) {
    kn.w = pack_get<Store32Args>(pack...).pw;
    kn.sys_stride = b->k.stride;
    kn.stride = 0;
  }
  [[maybe_unused]] WideStepLenArgs sl{};      // STEP: what the step's norm takes in place of the pack
  if constexpr (STEP) sl = WideStepLenArgs{pack_get<WideStepArgs>(pack...), b->has_len ? b->len : nullptr};
  if (b->weighted) {
    const WgtRows wgt = b->wgt;
    const WgtStride ws = WgtStride(b->wgt_stride);
    if constexpr (STEP) hipLaunchKernelGGL((k_wide_step_norm<LEN, WgtRows, WgtStride>), grid, block, 0, b->stream, kn, wa, sl, cf, ld, mask, wgt, ws);
    else hipLaunchKernelGGL((k_wide_norm<Pack..., WgtRows, WgtStride>), grid, block, 0, b->stream, kn, wa, cf, ld, mask, pack..., wgt, ws);
    hipLaunchKernelGGL((k_wide_sums<COMB, Pack..., WgtRows, WgtStride>), grid, block, lsums, b->stream, b->k, wa, cf, ld, mask, pack..., wgt, ws);
  } else {
    if constexpr (STEP) hipLaunchKernelGGL((k_wide_step_norm<LEN>), grid, block, 0, b->stream, kn, wa, sl, cf, ld, mask);
    else hipLaunchKernelGGL((k_wide_norm<Pack...>), grid, block, 0, b->stream, kn, wa, cf, ld, mask, pack...);
    hipLaunchKernelGGL((k_wide_sums<COMB, Pack...>), grid, block, lsums, b->stream, b->k, wa, cf, ld, mask, pack...);
  }
  if (b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT) {
    if constexpr (STEP && LEN) launch_wide_scalar_rows<Mask, WideStepArgs, LenRows>(b, wa, active, pack_get<WideStepArgs>(pack...), pack_get<LenRows>(pack...));
    else if constexpr (STEP) launch_wide_scalar_rows<Mask, WideStepArgs>(b, wa, active, pack_get<WideStepArgs>(pack...));
    else if constexpr (LEN) launch_wide_scalar_rows<Mask, LenRows>(b, wa, active, pack_get<LenRows>(pack...));
    else launch_wide_scalar_rows<Mask>(b, wa, active);
  } else {
    hipLaunchKernelGGL((k_wide_scalar<Mask, Pack...>), dim3((unsigned)b->k.nsys), block, lscal, b->stream, b->k, wa, active, pack...);
  }
  hipLaunchKernelGGL((k_wide_combine<COMB, Pack...>), grid, block, lcomb, b->stream, b->k, wa, f, ld, mask, pack...);
}
template <int COMB, class Mask, class... Step>
void launch_wide_len(nka_hip_batch_t b, double *f, int64_t ld, Mask *active, Step... step) {
  if (b->storage == NKA_HIP_BATCH_STORE_F32) {      // (the default flavour only: every other one was refused at creation)
    if constexpr (COMB == 2) {
      const Store32Args s32{b->pend_w, b->pend_v};
      if (b->has_len) launch_wide<COMB, Mask, Step..., LenRows, Store32Args>(b, f, ld, active, step..., b->len, s32);
      else launch_wide<COMB, Mask, Step..., Store32Args>(b, f, ld, active, step..., s32);
    }
    return;
  }
  if (b->has_len) launch_wide<COMB, Mask, Step..., LenRows>(b, f, ld, active, step..., b->len);
  else launch_wide<COMB, Mask, Step...>(b, f, ld, active, step...);
}
// `step`: nothing for the update, one WideStepArgs for the solve step
template <class Mask, class... Step>
void launch_wide_flavor(nka_hip_batch_t b, double *f, int64_t ld, Mask *active, Step... step) {
  switch (b->flavor) {
    case NKA_HIP_FLAVOR_F08_VECTOR: launch_wide_len<1, Mask, Step...>(b, f, ld, active, step...); break;
    case NKA_HIP_FLAVOR_C: launch_wide_len<2, Mask, Step...>(b, f, ld, active, step...); break;
    default: launch_wide_len<0, Mask, Step...>(b, f, ld, active, step...);
  }
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

void nka_batch_wide_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active) { launch_wide_flavor(b, f, ld, active); }

// the one buffer the solve step adds (b->nchunk is set): the partials of <f,f>
int nka_batch_wide_step_alloc(nka_hip_batch_t b) {
  const size_t nf = (size_t)nka_host::wide_fpart_count(b->k.nsys, b->nchunk);
  HIP_TRY(hipMalloc((void **)&b->fpart, sizeof(double) * nf));
  HIP_TRY(hipMemsetAsync(b->fpart, 0, sizeof(double) * nf, b->stream));
  return 0;
}

void nka_batch_wide_step_free(nka_hip_batch_t b) {
  hipFree(b->fpart);
  b->fpart = nullptr;
}

void nka_batch_wide_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol,
                         double *fnorm) {
  launch_wide_flavor(b, f, ld, active, WideStepArgs{b->fpart, x, x ? ldx : 0, tol, fnorm});
}

extern "C" int nka_hip_batch_wide_limits(int64_t *chunk, int64_t *max_vlen) {
  if (chunk) *chunk = kWideChunk;
  if (max_vlen) *max_vlen = std::min<int64_t>(NKA_HIP_BATCH_WIDE_MAX_VLEN, nka_host::kWideMaxChunks * kWideChunk);
  return 0;
}
