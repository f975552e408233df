// nka_batch.hip -- the batched accelerator of include/nka_hip_batch.h: nsys independent NKA states of equal shape, one
// kernel launch per update of the whole batch, ONE WORKGROUP PER SYSTEM (blockIdx.x = system).
//
// Inside a workgroup the phases of an update (nka_kernels.hpp: PA / scalar step / PB of a lone handle, three to six
// kernels) are separated by __syncthreads():
//   0 skip      active[sys] == 0: return before any memory of the system is touched
//   1 load      h, c and the links into LDS; thread 0 lists the older entries (the list length is read HERE, on the device)
//   2 norm      sum d^2, d = fl(w1 - f), per-thread strided fma, fixed-order reduction; s = sqrt
//   3 sums      on the ROUNDED w1' = fl(d/s) (fl(fl(1/s)*d) in the F08-vector flavour): <f,w1'>, <w1',w_p>, <f,w_p> while the
//               older w stream past once, kBatchGroup of them per sweep (f and w1 are re-read from cache per sweep)
//   4 scalar    thread 0, on the working copy in LDS: the lst_* functions of nka_device.hpp, i.e. the statements of k_solve:
//               decisions given the sums are the reference's by construction -- or, in the instances with a BatchRows member (a
//               batch of nka_hip_batch_create_rows with NKA_HIP_BATCH_SCALAR_WAVEFRONT), the 64 lanes of wavefront 0:
//               batch_scalar_step_rows (nka_batch_dev.hpp), the same bits in about mvec sequential steps
//   5 store    the working copy back to the system's control block
//   6 combine   normalise the pending pair, combine in list order with the flavour's association, w_new = f_in,
//               v_new = f_out, f
// No workgroup waits for another one: no flags, no spinning, no cooperative launch, no atomics.  The element -> thread
// mapping (pairs 2t, 2t+1 of every 512) and every accumulation order are the same whether a row of f is 16-byte aligned
// (16-byte loads) or not (two 8-byte loads), so results do not depend on ld, on nsys, or on a system's position.
// ORDERED = true is the reference-order sibling: every sum element after element, unfused, one thread per sum.
// WGT = true forms the weighted sums of nka_hip_batch_set_dot_weights in phases 2 and 3 (either order); phase 6 never reads
// the weights.
// A trailing StepArgs argument makes the instance a SOLVE STEP (nka_hip_batch_accel_step): <f,f> rides along in phase 2 (or is
// swept alone where there is no pending pair), the system may retire itself between phases 2 and 3 -- up to there a workgroup
// has written LDS only --, and phase 6 also forms x = fl(x - f_out).  Without it every step statement is discarded at compile
// time and the instance is the plain update, instruction for instruction.
// A WIDE batch (nka_hip_batch_create_wide) shares the handle, the storage and every host entry of this file; its update and
// its solve step -- a system split across workgroups, four launches each -- are nka_batch_wide.hip, what the units share nka_batch_dev.hpp.
// The kernel template itself is nka_batch_kernel.hpp: this unit holds the instances every narrow batch launches and the host
// entries, nka_batch_rows.hip the instances with the scalar step on wavefront 0 (nka_hip_batch_create_rows).
#include "nka_batch_dev.hpp"      // BatchArgs, the tile loads and stores, batch_sweep, batch_block_sum, the scalar step, the handle
#include "nka_batch_kernel.hpp"   // StepArgs, LenArgs, BatchRows<NLMAX>, k_batch_update

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace nka;

namespace {

// restart / relax (F08:422-457) of the active systems, one thread per system, on the control block in global memory
enum { kBatchOpRestart = 0, kBatchOpRelax = 1 };
__global__ __launch_bounds__(64) void k_batch_list_op(BatchArgs a, int op, const int32_t *__restrict__ active) {
  const int sys = blockIdx.x * 64 + threadIdx.x;
  if (sys >= a.nsys) return;
  if (active != nullptr && active[sys] == 0) return;
  const Ctl ctl = batch_ctl(a, sys);
  Lst L;
  lst_on_ctl(L, ctl);
  lst_load_scalars(L, ctl);      // (neither operation reads vtol)
  if (op == kBatchOpRestart) lst_restart(L); else lst_relax(L);
  lst_store_scalars(L, ctl);
}

__global__ __launch_bounds__(64) void k_batch_set_vtol(BatchArgs a, double vtol) {
  const int sys = blockIdx.x * 64 + threadIdx.x;
  if (sys < a.nsys) batch_ctl(a, sys).dc[DC_VTOL] = vtol;
}

// Set-time check of `rows` weight rows of n doubles, `ldw` apart (the strided sibling of k_check_weights, nka_kernels.hpp;
// the elements between two rows are never read): out[0] += entries that are not finite or below zero, out[1] = min over
// row * n + column of them (starts at ~0).  Grid-stride; runs once per set, not in an update.
__global__ __launch_bounds__(kBatchThreads) void k_batch_check_weights(const double *__restrict__ w, int64_t n, int64_t ldw,
                                                                       int64_t rows, unsigned long long *out) {
  unsigned long long bad = 0, first = ~0ull;
  for (int64_t e = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; e < rows * n; e += (int64_t)gridDim.x * kBatchThreads) {
    const double x = w[(e / n) * ldw + e % n];
    if (!(x >= 0.0 && x <= __DBL_MAX__)) {      // NaN, -Inf, +Inf, negative (-0.0 is >= 0)
      bad++;
      if ((unsigned long long)e < first) first = (unsigned long long)e;
    }
  }
  if (bad) {
    atomicAdd(out, bad);
    atomicMin(out + 1, first);
  }
}
// ... and the copy of the checked rows into the batch's buffer (rows `dld` apart)
__global__ __launch_bounds__(kBatchThreads) void k_batch_copy_weights(double *__restrict__ dst, int64_t dld,
                                                                      const double *__restrict__ w, int64_t n, int64_t ldw,
                                                                      int64_t rows) {
  for (int64_t e = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x; e < rows * n; e += (int64_t)gridDim.x * kBatchThreads)
    dst[(e / n) * dld + e % n] = w[(e / n) * ldw + e % n];
}

}  // namespace

namespace {

bool batch_ordered(const nka_hip_batch_state *b) {
  if (b->storage == NKA_HIP_BATCH_STORE_F32) return false;      // (AUTO: the rounded fast sums at every vlen)
  return b->sum_order == NKA_HIP_SUMS_REFERENCE_ORDER || (b->sum_order == NKA_HIP_SUMS_AUTO && b->k.n <= kOrdAutoMax);
}

int check_mask(const nka_hip_batch_state *b, const int32_t *active, const char *what) {
  if (!active) return 0;
  return nka_detail::check_device_span_i32(active, b->k.nsys, what);
}

int check_sys(const nka_hip_batch_state *b, int32_t sys, const char *who) {
  if (!b) return fail(NKA_HIP_EINVAL, std::string(who) + ": null handle");
  if (sys < 0 || sys >= b->k.nsys) return fail(NKA_HIP_EINVAL, std::string(who) + ": system out of range");
  return 0;
}

// control block of one system as it stands on the device (synchronises)
int fetch_sys(nka_hip_batch_t b, int32_t sys, std::vector<int32_t> &ic, std::vector<double> &dc) {
  HIP_TRY(hipSetDevice(b->device));
  const Ctl c = batch_ctl(b->k, sys);
  ic.resize((size_t)c.ic_count());
  dc.resize((size_t)c.dc_count());
  HIP_TRY(hipMemcpyAsync(ic.data(), c.ic, sizeof(int32_t) * ic.size(), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(dc.data(), c.dc, sizeof(double) * dc.size(), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int list_op(nka_hip_batch_t b, int op, const int32_t *active, const char *who) {
  if (!b) return fail(NKA_HIP_EINVAL, std::string(who) + ": null handle");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = check_mask(b, active, who)) return rc;
  hipLaunchKernelGGL(k_batch_list_op, dim3((unsigned)((b->k.nsys + 63) / 64)), dim3(64), 0, b->stream, b->k, op, active);
  HIP_TRY(hipGetLastError());
  return 0;
}

// (whether an update is weighted, and in which form, travels in the launch: the kernel instance, the weight pointer and the
// row stride are fixed when the update is enqueued -- or captured -- and only the buffer's VALUES are read when it runs)
// `step`: nothing for the update, one StepArgs for the solve step
template <int COMB, bool ORDERED, bool WGT, class... Step>
void launch_update_as(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  const size_t lds = nka_host::batch_lds(b->k.mvec).bytes();
  hipLaunchKernelGGL((k_batch_update<COMB, ORDERED, WGT, Step...>), dim3((unsigned)b->k.nsys), dim3(kBatchThreads), lds, b->stream, b->k, f,
                     ld, active, WGT ? (const double *)b->wgt : (const double *)nullptr, WGT ? b->wgt_stride : (int64_t)0, step...);
}
template <int COMB, class... Step>
void launch_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (batch_ordered(b)) {
    if (b->weighted) launch_update_as<COMB, true, true>(b, f, ld, active, step...);
    else launch_update_as<COMB, true, false>(b, f, ld, active, step...);
  } else {
    if (b->weighted) launch_update_as<COMB, false, true>(b, f, ld, active, step...);
    else launch_update_as<COMB, false, false>(b, f, ld, active, step...);
  }
}
template <class... Step>
void launch_flavor_as(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  switch (b->flavor) {
    case NKA_HIP_FLAVOR_F08_VECTOR: launch_update<1>(b, f, ld, active, step...); break;
    case NKA_HIP_FLAVOR_C: launch_update<2>(b, f, ld, active, step...); break;
    default: launch_update<0>(b, f, ld, active, step...);
  }
}
// (per-system lengths travel like the weights: the instance and the buffer's address are fixed when the update is enqueued or
// captured, the buffer's VALUES are read when it runs)
// binary32 storage: the default flavour and the fast sums only (refused otherwise at creation and in set_sum_order) -- eight
// instances, x weights x step x lengths; the pending buffers' addresses travel in the launch like the weights'
template <class... Step>
void launch_store32(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (b->weighted) launch_update_as<2, false, true>(b, f, ld, active, step...);
  else launch_update_as<2, false, false>(b, f, ld, active, step...);
}
template <class... Step>
void launch_flavor(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (b->storage == NKA_HIP_BATCH_STORE_F32) {
    const Store32Args s32{b->pend_w, b->pend_v};
    if (b->has_len) launch_store32(b, f, ld, active, step..., LenArgs{b->len}, s32); else launch_store32(b, f, ld, active, step..., s32);
    return;
  }
  if (b->has_len) launch_flavor_as(b, f, ld, active, step..., LenArgs{b->len}); else launch_flavor_as(b, f, ld, active, step...);
}
// what accel_update and accel_step check of f
int check_rows(nka_hip_batch_t b, const double *p, int64_t ld, const std::string &who, const char *name, const char *ldname) {
  if (ld < b->k.n) return fail(NKA_HIP_EINVAL, who + ": " + ldname + " must be >= vlen");
  if (ld > (INT64_MAX / (int64_t)sizeof(double) - b->k.n) / (int64_t)b->k.nsys)      // (the span below, in bytes, stays inside 64 bits)
    return fail(NKA_HIP_EINVAL, who + ": " + ldname + " is larger than any allocation");
  return nka_detail::check_device_span(p, (int64_t)(b->k.nsys - 1) * ld + b->k.n, (who + ": " + name).c_str());
}

// what both weight setters check first
int weights_settable(nka_hip_batch_t b, const char *what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(b->stream, &cs) != hipSuccess) (void)hipGetLastError();
  if (cs != hipStreamCaptureStatusNone) return fail(NKA_HIP_ESTATE, std::string(what) + ": the batch's stream is capturing");
  return 0;
}
int weights_ldw(nka_hip_batch_t b, int64_t ldw, const char *what) {
  if (ldw != 0 && ldw < b->k.n) return fail(NKA_HIP_EINVAL, std::string(what) + ": ldw must be >= vlen (one row per system) or 0 (one row for all)");
  if (ldw > (INT64_MAX / (int64_t)sizeof(double) - b->k.n) / (int64_t)b->k.nsys)
    return fail(NKA_HIP_EINVAL, std::string(what) + ": ldw is larger than any allocation");
  return 0;
}
int weights_alloc(nka_hip_batch_t b, double **buf) {
  if (!b->wgt_chk) HIP_TRY(hipMalloc((void **)&b->wgt_chk, 2 * sizeof(unsigned long long)));
  if (!*buf) HIP_TRY(hipMalloc((void **)buf, sizeof(double) * (size_t)b->k.stride * (size_t)b->k.nsys));
  return 0;
}
// `src`: device memory, nsys rows `ldw` apart, or one row with ldw == 0.  Checked where it lies, row by row, and only then
// copied into the batch's buffer: invalid weights leave the previous weighting in force.  Synchronises.
int set_weights_from_device(nka_hip_batch_t b, const double *src, int64_t ldw, const char *what) {
  hipStream_t s = b->stream;
  const int64_t n = b->k.n, rows = ldw == 0 ? 1 : b->k.nsys;
  if (int rc = weights_alloc(b, &b->wgt)) return rc;
  unsigned long long res[2] = {0ull, ~0ull};
  HIP_TRY(hipMemcpyAsync(b->wgt_chk, res, sizeof res, hipMemcpyHostToDevice, s));
  const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (rows * n + kBatchThreads - 1) / kBatchThreads));
  hipLaunchKernelGGL(k_batch_check_weights, dim3(g), dim3(kBatchThreads), 0, s, src, n, ldw, rows, b->wgt_chk);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(res, b->wgt_chk, sizeof res, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (res[0] != 0)
    return fail(NKA_HIP_EINVAL, std::string(what) + ": " + std::to_string(res[0]) + " weight(s) negative or not finite, the first in row " +
                                    std::to_string(res[1] / (unsigned long long)n) + " at index " + std::to_string(res[1] % (unsigned long long)n) +
                                    " (the previous weighting stays in force)");
  hipLaunchKernelGGL(k_batch_copy_weights, dim3(g), dim3(kBatchThreads), 0, s, b->wgt, b->k.stride, src, n, ldw, rows);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  b->weighted = true;
  b->wgt_stride = ldw == 0 ? 0 : b->k.stride;
  return 0;
}

}  // namespace

extern "C" {

// the three kinds of batch: `wide` = a system split across workgroups (nka_batch_wide.hip), `lanes` = one lane per system
// (nka_batch_lanes.hip), `waves` = one wavefront per system on the storage of this file (nka_batch_waves.hip), none = one workgroup
// per system (this file)
static int batch_create(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor, int32_t device,
                        void *stream, bool wide, int32_t storage = NKA_HIP_BATCH_STORE_F64, const char *entry = nullptr,
                        bool lanes = false, bool waves = false, bool wide_step = false, bool waves_ext = false, bool wide_ext = false,
                        bool waves_rows = false, bool narrow_rows = false) {
  const std::string who = entry ? entry : wide ? "nka_hip_batch_create_wide" : "nka_hip_batch_create";
  const bool s32 = storage == NKA_HIP_BATCH_STORE_F32;
  if (!out) return fail(NKA_HIP_EINVAL, who + ": out is NULL");
  *out = nullptr;
  if (nsys < 1) return fail(NKA_HIP_EINVAL, who + ": nsys must be >= 1");
  if (storage != NKA_HIP_BATCH_STORE_F64 && !s32) return fail(NKA_HIP_EINVAL, who + ": unknown storage (NKA_HIP_BATCH_STORE_F64 or _F32)");
  if (wide) {
    int64_t chunk = 0, cap = 0;
    nka_hip_batch_wide_limits(&chunk, &cap);
    if (nsys > 65535) return fail(NKA_HIP_EINVAL, who + ": nsys must be <= 65535 (the system is the second grid index)");
    if (vlen < 1 || vlen > cap)
      return fail(NKA_HIP_EINVAL, who + ": vlen must be 1 ... " + std::to_string((long long)cap) + " (longer systems: lone handles, nka_hip_create)");
  } else if (lanes) {
    if (vlen < 1 || vlen > NKA_HIP_BATCH_LANES_MAX_VLEN)
      return fail(NKA_HIP_EINVAL, who + ": vlen must be 1 ... " + std::to_string((int)NKA_HIP_BATCH_LANES_MAX_VLEN) +
                                      " (one lane forms every sum of a system; longer systems: nka_hip_batch_create)");
  } else if (waves) {
    if (vlen < 1 || vlen > NKA_HIP_BATCH_WAVES_MAX_VLEN)
      return fail(NKA_HIP_EINVAL, who + ": vlen must be 1 ... " + std::to_string((int)NKA_HIP_BATCH_WAVES_MAX_VLEN) +
                                      " (one wavefront sweeps a system; longer systems: nka_hip_batch_create)");
  } else if (vlen < 1 || vlen > NKA_HIP_BATCH_MAX_VLEN)
    return fail(NKA_HIP_EINVAL, (narrow_rows ? who : std::string("nka_hip_batch_create")) + ": vlen must be 1 ... " + std::to_string((int)NKA_HIP_BATCH_MAX_VLEN) +
                                    " (longer systems: nka_hip_batch_create_wide, or lone handles, nka_hip_create)");
  if (mvec < 1 || mvec > NKA_HIP_BATCH_MAX_MVEC)
    return fail(NKA_HIP_EINVAL, who + ": mvec must be 1 ... " + std::to_string((int)NKA_HIP_BATCH_MAX_MVEC));
  if (waves && waves_rows && mvec > nka_host::waves_rows_max_mvec())      // (derived: four working copies and four matrices in 64 KiB)
    return fail(NKA_HIP_EINVAL, who + ": mvec must be 1 ... " + std::to_string(nka_host::waves_rows_max_mvec()) +
                                    " (the wavefront step keeps a matrix of (mvec + 2)^2 doubles per system in LDS beside the working copy; "
                                    "longer lists: nka_hip_batch_create_waves, which keeps the one-lane step)");
  if (!(vtol > 0.0)) return fail(NKA_HIP_EINVAL, who + ": vtol must be > 0");
  if (int rc = nka_detail::resolve_flavor(&flavor, who.c_str())) return rc;
  if (s32 && flavor != NKA_HIP_FLAVOR_C)
    return fail(NKA_HIP_EINVAL, who + ": binary32 storage runs the default flavour only (NKA_HIP_FLAVOR_C); the F08 flavours are there "
                                      "for the reference's bits, which this storage gives up");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(NKA_HIP_EINVAL, who + ": no such HIP device");
  HIP_TRY(hipSetDevice(device));

  auto *b = new nka_hip_batch_state();
  b->wide = wide;
  b->lanes = lanes;
  b->waves = waves;
  b->waves_ext = waves && waves_ext;
  b->waves_rows = waves && waves_rows;
  b->wide_ext = wide && wide_ext;
  b->narrow_rows = narrow_rows && !wide && !lanes && !waves;
  b->device = device;
  b->stream = (hipStream_t)stream;
  b->flavor = flavor;
  b->vtol = vtol;
  b->storage = storage;
  BatchArgs &k = b->k;
  k.n = vlen;
  k.mvec = mvec;
  k.nsys = nsys;
  const nka_host::BatchLayout lay = nka_host::batch_layout(vlen, mvec);
  k.stride = lay.stride;
  k.sys_stride = lay.sys_stride;
  k.ic_stride = lay.ic_stride;
  k.dc_stride = lay.dc_stride;
  const double slot_bytes = lanes ? 0.0 : (double)k.sys_stride * 8.0 * (double)nsys;      // (a lane batch: checked where it allocates)
  if (slot_bytes > 1.0e13) {      // (beyond any device: also keeps the size arithmetic below inside 64 bits)
    delete b;
    return fail(NKA_HIP_ENOMEM, who + ": the batch needs more device memory than any device has");
  }
  int rc = 0;
  auto alloc = [&](void **p, size_t bytes) {
    if (rc) return;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(NKA_HIP_ENOMEM, std::string("hipMalloc(") + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    }
  };
  // (binary32 storage: float allocations of the same strides in elements behind k.w / k.v, and the two pending buffers)
  // (a lane batch: its own interleaved slots, allocated and zeroed by nka_batch_lanes_alloc)
  const size_t slot_bytes_each = lanes ? (size_t)0 : (size_t)nka_host::batch_slot_alloc_bytes(lay, nsys, storage);
  const size_t pend_bytes_each = (size_t)nka_host::batch_pending_alloc_bytes(lay, nsys, storage);
  if (lanes) {
    rc = nka_batch_lanes_alloc(b);
  } else {
    alloc((void **)&k.w, slot_bytes_each);
    alloc((void **)&k.v, slot_bytes_each);
  }
  if (s32) {
    alloc((void **)&b->pend_w, pend_bytes_each);
    alloc((void **)&b->pend_v, pend_bytes_each);
  }
  if (!lanes) b->vector_bytes = nka_host::batch_vector_bytes(lay, nsys, storage);
  alloc((void **)&k.ic, sizeof(int32_t) * (size_t)k.ic_stride * (size_t)nsys);
  alloc((void **)&k.dc, sizeof(double) * (size_t)k.dc_stride * (size_t)nsys);
  if (!rc && (hipMemsetAsync(k.ic, 0, sizeof(int32_t) * (size_t)k.ic_stride * (size_t)nsys, b->stream) != hipSuccess ||
              hipMemsetAsync(k.dc, 0, sizeof(double) * (size_t)k.dc_stride * (size_t)nsys, b->stream) != hipSuccess ||
              (!lanes && (hipMemsetAsync(k.w, 0, slot_bytes_each, b->stream) != hipSuccess ||
                          hipMemsetAsync(k.v, 0, slot_bytes_each, b->stream) != hipSuccess)) ||
              (s32 && (hipMemsetAsync(b->pend_w, 0, pend_bytes_each, b->stream) != hipSuccess ||
                       hipMemsetAsync(b->pend_v, 0, pend_bytes_each, b->stream) != hipSuccess)))) {
    (void)hipGetLastError();
    rc = fail(NKA_HIP_EHIP, who + ": initialising the batch failed");
  }
  if (!rc && wide) rc = nka_batch_wide_alloc(b);
  if (!rc && wide_step) {      // (one more buffer than a batch of nka_hip_batch_create_wide holds; nothing else differs)
    b->wide_step = true;
    rc = nka_batch_wide_step_alloc(b);
  }
  if (!rc) {
    hipLaunchKernelGGL(k_batch_set_vtol, dim3((unsigned)((nsys + 63) / 64)), dim3(64), 0, b->stream, k, vtol);
    hipLaunchKernelGGL(k_batch_list_op, dim3((unsigned)((nsys + 63) / 64)), dim3(64), 0, b->stream, k, (int)kBatchOpRestart,
                       (const int32_t *)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) rc = fail(NKA_HIP_EHIP, who + ": " + hipGetErrorString(e));
  }
  if (rc) {
    nka_hip_batch_destroy(b);
    return rc;
  }
  *out = b;
  return 0;
}

int nka_hip_batch_create(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                         int32_t device, void *stream) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false);
}
int nka_hip_batch_create_wide(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                              int32_t device, void *stream) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, true);
}
int nka_hip_batch_create_wide_step(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                                   int32_t device, void *stream) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, true, NKA_HIP_BATCH_STORE_F64, "nka_hip_batch_create_wide_step", false,
                      false, true);
}
int nka_hip_batch_create_wide_ext(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                                  int32_t device, void *stream, int32_t step) {
  if (step != 0 && step != 1) {
    if (out) *out = nullptr;
    return fail(NKA_HIP_EINVAL, "nka_hip_batch_create_wide_ext: step must be 0 (nka_hip_batch_create_wide) or 1 (nka_hip_batch_create_wide_step)");
  }
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, true, NKA_HIP_BATCH_STORE_F64, "nka_hip_batch_create_wide_ext", false,
                      false, step == 1, false, true);
}
// (a wide batch with binary32 storage: the allocations of batch_create for that storage at the wide batch's stride, the binary32
// instances of nka_batch_wide.hip; with binary64 storage every argument of the call above)
int nka_hip_batch_create_wide_stored(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                                     int32_t device, void *stream, int32_t step, int32_t storage) {
  if (step != 0 && step != 1) {
    if (out) *out = nullptr;
    return fail(NKA_HIP_EINVAL, "nka_hip_batch_create_wide_stored: step must be 0 (no solve step) or 1 (nka_hip_batch_accel_step is offered)");
  }
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, true, storage, "nka_hip_batch_create_wide_stored", false, false,
                      step == 1, false, true);
}
int nka_hip_batch_create_stored(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                                int32_t device, void *stream, int32_t storage) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false, storage, "nka_hip_batch_create_stored");
}
int nka_hip_batch_create_lanes(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                               int32_t device, void *stream) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false, NKA_HIP_BATCH_STORE_F64, "nka_hip_batch_create_lanes", true);
}
int nka_hip_batch_create_waves(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                               int32_t device, void *stream) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false, NKA_HIP_BATCH_STORE_F64, "nka_hip_batch_create_waves", false,
                      true);
}
int nka_hip_batch_create_waves_ext(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                                   int32_t device, void *stream) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false, NKA_HIP_BATCH_STORE_F64, "nka_hip_batch_create_waves_ext",
                      false, true, false, true);
}
// (a wave batch that offers the scalar step on the wavefront: the batch of one of the two entries above, with the cap on mvec)
int nka_hip_batch_create_waves_rows(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                                    int32_t device, void *stream, int32_t ext) {
  if (ext != 0 && ext != 1) {
    if (out) *out = nullptr;
    return fail(NKA_HIP_EINVAL, "nka_hip_batch_create_waves_rows: ext must be 0 (nka_hip_batch_create_waves) or 1 (nka_hip_batch_create_waves_ext)");
  }
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false, NKA_HIP_BATCH_STORE_F64, "nka_hip_batch_create_waves_rows",
                      false, true, false, ext == 1, false, true);
}
// (a narrow batch that offers the scalar step on wavefront 0 of a system's workgroup: the batch of nka_hip_batch_create, or with
// binary32 storage that of nka_hip_batch_create_stored, and one host flag)
int nka_hip_batch_create_rows(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol, int32_t flavor,
                              int32_t device, void *stream, int32_t storage) {
  return batch_create(out, nsys, vlen, mvec, vtol, flavor, device, stream, false, storage, "nka_hip_batch_create_rows", false, false, false,
                      false, false, false, true);
}
int nka_hip_batch_rows_limits(int32_t mvec, int64_t *lds_bytes) {
  if (mvec < 1 || mvec > NKA_HIP_BATCH_MAX_MVEC)
    return fail(NKA_HIP_EINVAL, "nka_hip_batch_rows_limits: mvec must be 1 ... " + std::to_string((int)NKA_HIP_BATCH_MAX_MVEC));
  if (lds_bytes) *lds_bytes = nka_host::batch_rows_lds(mvec).bytes();
  return 0;
}
int nka_hip_batch_kind(nka_hip_batch_t b) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_kind: null handle");
  if (b->waves) return NKA_HIP_BATCH_KIND_WAVES;
  return b->lanes ? NKA_HIP_BATCH_KIND_LANES : b->wide ? NKA_HIP_BATCH_KIND_WIDE : NKA_HIP_BATCH_KIND_NARROW;
}
int nka_hip_batch_storage(nka_hip_batch_t b) { return b ? b->storage : fail(NKA_HIP_EINVAL, "batch_storage: null handle"); }
int64_t nka_hip_batch_vector_bytes(nka_hip_batch_t b) { return b ? b->vector_bytes : (int64_t)fail(NKA_HIP_EINVAL, "batch_vector_bytes: null handle"); }
int nka_hip_batch_is_wide(nka_hip_batch_t b) { return b ? (b->wide ? 1 : 0) : fail(NKA_HIP_EINVAL, "batch_is_wide: null handle"); }
int nka_hip_batch_offers_step(nka_hip_batch_t b) {
  return b ? (b->wide && !b->wide_step ? 0 : 1) : fail(NKA_HIP_EINVAL, "batch_offers_step: null handle");
}

int nka_hip_batch_offers_lengths(nka_hip_batch_t b) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_offers_lengths: null handle");
  return b->lanes || (b->waves && !b->waves_ext) ? 0 : 1;
}
int nka_hip_batch_offers_weights(nka_hip_batch_t b) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_offers_weights: null handle");
  return (b->wide && !b->wide_ext) || b->lanes || (b->waves && !b->waves_ext) ? 0 : 1;
}

int nka_hip_batch_destroy(nka_hip_batch_t b) {
  if (!b) return 0;
  nka_detail::invalidate_span_cache();
  hipSetDevice(b->device);
  hipStreamSynchronize(b->stream);
  hipFree(b->k.w);
  hipFree(b->k.v);
  hipFree(b->k.ic);
  hipFree(b->k.dc);
  hipFree(b->wgt);
  hipFree(b->wgt_stage);
  hipFree(b->wgt_chk);
  hipFree(b->len);
  hipFree(b->pend_w);
  hipFree(b->pend_v);
  nka_batch_wide_free(b);
  nka_batch_wide_step_free(b);
  nka_batch_lanes_free(b);
  delete b;
  return 0;
}

int nka_hip_batch_accel_update(nka_hip_batch_t b, double *f_dev, int64_t ld, const int32_t *active_dev) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_accel_update: null handle");
  if (!f_dev) return fail(NKA_HIP_EINVAL, "batch_accel_update: f is NULL");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = check_rows(b, f_dev, ld, "batch_accel_update", "f", "ld")) return rc;
  if (int rc = check_mask(b, active_dev, "batch_accel_update: active")) return rc;
  if (b->wide) nka_batch_wide_update(b, f_dev, ld, active_dev);
  else if (b->lanes) nka_batch_lanes_update(b, f_dev, ld, active_dev);
  else if (b->waves) nka_batch_waves_update(b, f_dev, ld, active_dev);
  else if (b->narrow_rows && b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT) nka_batch_rows_update(b, f_dev, ld, active_dev);
  else launch_flavor(b, f_dev, ld, active_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

int nka_hip_batch_accel_step(nka_hip_batch_t b, double *f_dev, int64_t ld, double *x_dev, int64_t ldx, int32_t *active_dev,
                             const double *tol_dev, double *fnorm_dev) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_accel_step: null handle");
  if (b->wide && !b->wide_step)
    return fail(NKA_HIP_EINVAL, "batch_accel_step: not offered by a wide batch (nka_hip_batch_create_wide): accel_update, or a batch of "
                                "nka_hip_batch_create_wide_step");
  if (!f_dev) return fail(NKA_HIP_EINVAL, "batch_accel_step: f is NULL");
  if (tol_dev && !active_dev) return fail(NKA_HIP_EINVAL, "batch_accel_step: tol needs a mask (a system retires by clearing its entry)");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = check_rows(b, f_dev, ld, "batch_accel_step", "f", "ld")) return rc;
  if (x_dev) {
    if (int rc = check_rows(b, x_dev, ldx, "batch_accel_step", "x", "ldx")) return rc;
    const int64_t nf = (int64_t)(b->k.nsys - 1) * ld + b->k.n, nx = (int64_t)(b->k.nsys - 1) * ldx + b->k.n;
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(f_dev), x0 = reinterpret_cast<uintptr_t>(x_dev);
    if (f0 < x0 + sizeof(double) * (uintptr_t)nx && x0 < f0 + sizeof(double) * (uintptr_t)nf)
      return fail(NKA_HIP_EINVAL, "batch_accel_step: the span of x overlaps the span of f");
  }
  if (int rc = check_mask(b, active_dev, "batch_accel_step: active")) return rc;
  if (tol_dev)
    if (int rc = nka_detail::check_device_span(tol_dev, b->k.nsys, "batch_accel_step: tol")) return rc;
  if (fnorm_dev)
    if (int rc = nka_detail::check_device_span(fnorm_dev, b->k.nsys, "batch_accel_step: fnorm")) return rc;
  if (tol_dev && fnorm_dev) {
    const uintptr_t t0 = reinterpret_cast<uintptr_t>(tol_dev), n0 = reinterpret_cast<uintptr_t>(fnorm_dev), len = sizeof(double) * (uintptr_t)b->k.nsys;
    if (t0 < n0 + len && n0 < t0 + len) return fail(NKA_HIP_EINVAL, "batch_accel_step: fnorm overlaps tol (a threshold would be overwritten while it is read)");
  }
  if (b->wide) nka_batch_wide_step(b, f_dev, ld, x_dev, ldx, active_dev, tol_dev, fnorm_dev);
  else if (b->lanes) nka_batch_lanes_step(b, f_dev, ld, x_dev, ldx, active_dev, tol_dev, fnorm_dev);
  else if (b->waves) nka_batch_waves_step(b, f_dev, ld, x_dev, ldx, active_dev, tol_dev, fnorm_dev);
  else if (b->narrow_rows && b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT) nka_batch_rows_step(b, f_dev, ld, x_dev, ldx, active_dev, tol_dev, fnorm_dev);
  else launch_flavor(b, f_dev, ld, active_dev, StepArgs{x_dev, x_dev ? ldx : 0, tol_dev, fnorm_dev});
  HIP_TRY(hipGetLastError());
  return 0;
}

int nka_hip_batch_restart(nka_hip_batch_t b, const int32_t *active_dev) { return list_op(b, kBatchOpRestart, active_dev, "batch_restart"); }
int nka_hip_batch_relax(nka_hip_batch_t b, const int32_t *active_dev) { return list_op(b, kBatchOpRelax, active_dev, "batch_relax"); }

int nka_hip_batch_set_vec_tol(nka_hip_batch_t b, double vtol) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_vec_tol: null handle");
  if (!(vtol > 0.0)) return fail(NKA_HIP_EINVAL, "batch_set_vec_tol: vtol must be > 0");      // F08:205
  HIP_TRY(hipSetDevice(b->device));
  b->vtol = vtol;
  hipLaunchKernelGGL(k_batch_set_vtol, dim3((unsigned)((b->k.nsys + 63) / 64)), dim3(64), 0, b->stream, b->k, vtol);
  HIP_TRY(hipGetLastError());
  return 0;
}

int nka_hip_batch_set_sum_order(nka_hip_batch_t b, int32_t order) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_sum_order: null handle");
  if (b->wide && order != NKA_HIP_SUMS_AUTO && order != NKA_HIP_SUMS_BLOCKED_ROUNDED)
    return fail(NKA_HIP_EINVAL, "batch_set_sum_order: a wide batch forms the rounded fast sums only: NKA_HIP_SUMS_BLOCKED_ROUNDED or _AUTO");
  if (b->storage == NKA_HIP_BATCH_STORE_F32 && order == NKA_HIP_SUMS_REFERENCE_ORDER)
    return fail(NKA_HIP_EINVAL, "batch_set_sum_order: a batch with binary32 storage forms the rounded fast sums only (the reference order is "
                                "there for the reference's bits, which this storage gives up): NKA_HIP_SUMS_BLOCKED_ROUNDED or _AUTO");
  if (b->lanes && (order == NKA_HIP_SUMS_BLOCKED || order == NKA_HIP_SUMS_BLOCKED_ROUNDED))
    return fail(NKA_HIP_EINVAL, "batch_set_sum_order: a lane batch forms every sum in the reference's order (one lane, element after "
                                "element): NKA_HIP_SUMS_REFERENCE_ORDER or _AUTO; the fast sums: nka_hip_batch_create");
  if (b->waves && order != NKA_HIP_SUMS_AUTO && order != NKA_HIP_SUMS_BLOCKED_ROUNDED)
    return fail(NKA_HIP_EINVAL, "batch_set_sum_order: a wave batch forms the rounded fast sums only (one wavefront per system): "
                                "NKA_HIP_SUMS_BLOCKED_ROUNDED or _AUTO; the reference order: nka_hip_batch_create");
  if (order == NKA_HIP_SUMS_BLOCKED)
    return fail(NKA_HIP_EINVAL, "batch_set_sum_order: NKA_HIP_SUMS_BLOCKED is not offered by a batch (it has no exchange to save): "
                                "NKA_HIP_SUMS_BLOCKED_ROUNDED, _REFERENCE_ORDER or _AUTO");
  if (order != NKA_HIP_SUMS_AUTO && order != NKA_HIP_SUMS_REFERENCE_ORDER && order != NKA_HIP_SUMS_BLOCKED_ROUNDED)
    return fail(NKA_HIP_EINVAL, "batch_set_sum_order: unknown sum order");
  // (a narrow batch of nka_hip_batch_create_rows: the wavefront step has fast-sum instances only, and nothing is downgraded)
  if (b->narrow_rows && b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT && b->storage != NKA_HIP_BATCH_STORE_F32 &&
      (order == NKA_HIP_SUMS_REFERENCE_ORDER || (order == NKA_HIP_SUMS_AUTO && b->k.n <= kOrdAutoMax)))
    return fail(NKA_HIP_ESTATE, "batch_set_sum_order: this order means the reference order here (explicitly, or NKA_HIP_SUMS_AUTO at vlen <= 64), and "
                                "NKA_HIP_BATCH_SCALAR_WAVEFRONT is set, which runs with the fast sums only: call nka_hip_batch_set_scalar_step(b, "
                                "NKA_HIP_BATCH_SCALAR_ONE_THREAD) first; systems of at most 1024 elements have the wavefront step in "
                                "nka_hip_batch_create_waves_rows");
  b->sum_order = order;
  return 0;
}

// SCALAR STEP: enqueue-side state of a wide batch, read by launch_wide (nka_batch_wide.hip) when a call is enqueued, of a wave
// batch of nka_hip_batch_create_waves_rows, read by launch_waves_as (nka_batch_waves.hip), and of a narrow batch of
// nka_hip_batch_create_rows, read by nka_hip_batch_accel_update / _accel_step (above), which then call nka_batch_rows.hip
int nka_hip_batch_offers_scalar_step(nka_hip_batch_t b) {
  return b ? (b->wide || b->waves_rows || b->narrow_rows ? 1 : 0) : fail(NKA_HIP_EINVAL, "batch_offers_scalar_step: null handle");
}
int nka_hip_batch_scalar_step(nka_hip_batch_t b) { return b ? b->scalar_step : fail(NKA_HIP_EINVAL, "batch_scalar_step: null handle"); }
int nka_hip_batch_set_scalar_step(nka_hip_batch_t b, int32_t how) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_scalar_step: null handle");
  if (how != NKA_HIP_BATCH_SCALAR_ONE_THREAD && how != NKA_HIP_BATCH_SCALAR_WAVEFRONT)
    return fail(NKA_HIP_EINVAL, "batch_set_scalar_step: NKA_HIP_BATCH_SCALAR_ONE_THREAD or NKA_HIP_BATCH_SCALAR_WAVEFRONT");
  if (how == NKA_HIP_BATCH_SCALAR_WAVEFRONT && !b->wide && !b->waves_rows && !b->narrow_rows)
    return fail(NKA_HIP_EINVAL, "batch_set_scalar_step: NKA_HIP_BATCH_SCALAR_WAVEFRONT is offered by a wide batch (nka_hip_batch_create_wide "
                                "and its four siblings), by a wave batch of nka_hip_batch_create_waves_rows and by a narrow batch of "
                                "nka_hip_batch_create_rows only: this batch keeps NKA_HIP_BATCH_SCALAR_ONE_THREAD");
  // (a narrow batch of nka_hip_batch_create_rows: the wavefront step has fast-sum instances only, and nothing is downgraded)
  if (how == NKA_HIP_BATCH_SCALAR_WAVEFRONT && b->narrow_rows && batch_ordered(b))
    return fail(NKA_HIP_ESTATE, "batch_set_scalar_step: NKA_HIP_BATCH_SCALAR_WAVEFRONT runs with the fast sums only, and this batch forms its "
                                "sums in the reference order (explicitly, or NKA_HIP_SUMS_AUTO at vlen <= 64): call nka_hip_batch_set_sum_order(b, "
                                "NKA_HIP_SUMS_BLOCKED_ROUNDED) first; systems of at most 1024 elements have the wavefront step in "
                                "nka_hip_batch_create_waves_rows");
  b->scalar_step = how;
  return 0;
}

int nka_hip_batch_set_dot_weights(nka_hip_batch_t b, const double *w_dev, int64_t ldw) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights: null handle");
  if (b->wide && !b->wide_ext) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights: not offered by a wide batch (nka_hip_batch_create_wide)");
  if (b->lanes) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights: not offered by a lane batch (nka_hip_batch_create_lanes): nka_hip_batch_create");
  if (b->waves && !b->waves_ext) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights: not offered by a wave batch (nka_hip_batch_create_waves): nka_hip_batch_create");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = weights_settable(b, "batch_set_dot_weights")) return rc;
  if (!w_dev) {
    b->weighted = false;      // (the buffer stays: a captured update may hold its address)
    return 0;
  }
  if (int rc = weights_ldw(b, ldw, "batch_set_dot_weights")) return rc;
  const int64_t span = ldw == 0 ? b->k.n : (int64_t)(b->k.nsys - 1) * ldw + b->k.n;
  if (int rc = nka_detail::check_device_span(w_dev, span, "batch_set_dot_weights: w")) return rc;
  return set_weights_from_device(b, w_dev, ldw, "batch_set_dot_weights");
}

int nka_hip_batch_set_dot_weights_host(nka_hip_batch_t b, const double *w_host, int64_t ldw) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights_host: null handle");
  if (b->wide && !b->wide_ext) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights_host: not offered by a wide batch (nka_hip_batch_create_wide)");
  if (b->lanes) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights_host: not offered by a lane batch (nka_hip_batch_create_lanes): nka_hip_batch_create");
  if (b->waves && !b->waves_ext) return fail(NKA_HIP_EINVAL, "batch_set_dot_weights_host: not offered by a wave batch (nka_hip_batch_create_waves): nka_hip_batch_create");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = weights_settable(b, "batch_set_dot_weights_host")) return rc;
  if (!w_host) {
    b->weighted = false;
    return 0;
  }
  if (int rc = weights_ldw(b, ldw, "batch_set_dot_weights_host")) return rc;
  // the caller's rows, without the padding between them, into a staging buffer of the batch's own row stride; checked there
  if (int rc = weights_alloc(b, &b->wgt_stage)) return rc;
  const int64_t rows = ldw == 0 ? 1 : b->k.nsys;
  for (int64_t r = 0; r < rows; r++)
    HIP_TRY(hipMemcpyAsync(b->wgt_stage + (size_t)r * b->k.stride, w_host + (size_t)r * ldw, sizeof(double) * (size_t)b->k.n,
                           hipMemcpyHostToDevice, b->stream));
  return set_weights_from_device(b, b->wgt_stage, ldw == 0 ? 0 : b->k.stride, "batch_set_dot_weights_host");
}

int nka_hip_batch_dot_weighted(nka_hip_batch_t b) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_dot_weighted: null handle");
  return b->weighted ? 1 : 0;
}

// PER-SYSTEM LENGTHS (nka_hip_batch.h, LENGTHS).  Both setters end in set_lengths_checked: the values are on the HOST by then
// -- the device entry stages its checked span there --, every one is held to 1 <= len <= vlen, and only then are they copied
// into the batch's buffer, which therefore never holds a length that an update kernel may not use as a bound.
static int lengths_alloc(nka_hip_batch_t b) {
  if (b->len) return 0;
  int32_t *p = nullptr;
  HIP_TRY(hipMalloc((void **)&p, sizeof(int32_t) * (size_t)b->k.nsys));
  const std::vector<int32_t> full((size_t)b->k.nsys, (int32_t)b->k.n);      // (vlen everywhere until a set succeeds)
  hipError_t e = hipMemcpyAsync(p, full.data(), sizeof(int32_t) * full.size(), hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    hipFree(p);
    return fail(NKA_HIP_EHIP, std::string("batch_set_lengths: ") + hipGetErrorString(e));
  }
  b->len = p;
  return 0;
}
static int set_lengths_checked(nka_hip_batch_t b, const int32_t *len_host, const char *what) {
  for (int32_t sys = 0; sys < b->k.nsys; sys++)
    if (!nka_host::batch_len_valid(len_host[sys], b->k.n))
      return fail(NKA_HIP_EINVAL, std::string(what) + ": length " + std::to_string(len_host[sys]) + " of system " + std::to_string(sys) +
                                      " is outside 1 ... vlen = " + std::to_string((long long)b->k.n) +
                                      " (the previous lengths stay in force; a system that should sit out: the mask)");
  if (int rc = lengths_alloc(b)) return rc;
  HIP_TRY(hipMemcpyAsync(b->len, len_host, sizeof(int32_t) * (size_t)b->k.nsys, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->has_len = true;
  return 0;
}
// NULL: every system vlen long again.  The buffer stays -- a captured update may hold its address -- and is filled with vlen.
static int clear_lengths(nka_hip_batch_t b) {
  b->has_len = false;
  if (!b->len) return 0;
  const std::vector<int32_t> full((size_t)b->k.nsys, (int32_t)b->k.n);
  HIP_TRY(hipMemcpyAsync(b->len, full.data(), sizeof(int32_t) * full.size(), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int nka_hip_batch_set_lengths(nka_hip_batch_t b, const int32_t *len_dev) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_lengths: null handle");
  if (b->lanes) return fail(NKA_HIP_EINVAL, "batch_set_lengths: not offered by a lane batch (nka_hip_batch_create_lanes): nka_hip_batch_create");
  if (b->waves && !b->waves_ext) return fail(NKA_HIP_EINVAL, "batch_set_lengths: not offered by a wave batch (nka_hip_batch_create_waves): nka_hip_batch_create");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = weights_settable(b, "batch_set_lengths")) return rc;
  if (!len_dev) return clear_lengths(b);
  if (int rc = nka_detail::check_device_span_i32(len_dev, b->k.nsys, "batch_set_lengths: len")) return rc;
  std::vector<int32_t> stage((size_t)b->k.nsys);
  HIP_TRY(hipMemcpyAsync(stage.data(), len_dev, sizeof(int32_t) * stage.size(), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return set_lengths_checked(b, stage.data(), "batch_set_lengths");
}

int nka_hip_batch_set_lengths_host(nka_hip_batch_t b, const int32_t *len_host) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_lengths_host: null handle");
  if (b->lanes) return fail(NKA_HIP_EINVAL, "batch_set_lengths_host: not offered by a lane batch (nka_hip_batch_create_lanes): nka_hip_batch_create");
  if (b->waves && !b->waves_ext) return fail(NKA_HIP_EINVAL, "batch_set_lengths_host: not offered by a wave batch (nka_hip_batch_create_waves): nka_hip_batch_create");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = weights_settable(b, "batch_set_lengths_host")) return rc;
  if (!len_host) return clear_lengths(b);
  const std::vector<int32_t> stage(len_host, len_host + b->k.nsys);      // (pageable memory of the caller's is free again at once)
  return set_lengths_checked(b, stage.data(), "batch_set_lengths_host");
}

int nka_hip_batch_get_lengths(nka_hip_batch_t b, int32_t *len_host) {
  if (!b || !len_host) return fail(NKA_HIP_EINVAL, "batch_get_lengths: null argument");
  if (!b->has_len) {
    std::fill(len_host, len_host + b->k.nsys, (int32_t)b->k.n);
    return 0;
  }
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipMemcpyAsync(len_host, b->len, sizeof(int32_t) * (size_t)b->k.nsys, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int nka_hip_batch_has_lengths(nka_hip_batch_t b) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_has_lengths: null handle");
  return b->has_len ? 1 : 0;
}

int nka_hip_batch_set_stream(nka_hip_batch_t b, void *stream) {
  if (!b) return fail(NKA_HIP_EINVAL, "batch_set_stream: null handle");
  hipStream_t ns = (hipStream_t)stream;
  if (ns == b->stream) return 0;
  HIP_TRY(hipSetDevice(b->device));
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e1 = hipEventRecord(ev, b->stream);
  hipError_t e2 = (e1 == hipSuccess) ? hipStreamWaitEvent(ns, ev, 0) : e1;
  hipEventDestroy(ev);
  if (e2 != hipSuccess) return fail(NKA_HIP_EHIP, std::string("batch_set_stream: ") + hipGetErrorString(e2));
  b->stream = ns;
  return 0;
}

int nka_hip_batch_flavor(nka_hip_batch_t b) { return b ? b->flavor : fail(NKA_HIP_EINVAL, "batch_flavor: null handle"); }

int nka_hip_batch_num_vec(nka_hip_batch_t b, int32_t *num_vec_host) {
  if (!b || !num_vec_host) return fail(NKA_HIP_EINVAL, "batch_num_vec: null argument");
  HIP_TRY(hipSetDevice(b->device));
  std::vector<int32_t> ic((size_t)b->k.ic_stride * (size_t)b->k.nsys);
  HIP_TRY(hipMemcpyAsync(ic.data(), b->k.ic, sizeof(int32_t) * ic.size(), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int sys = 0; sys < b->k.nsys; sys++)
    num_vec_host[sys] = nka_host::snapshot_num_vec(ic.data() + (size_t)sys * b->k.ic_stride, b->k.mvec);
  return 0;
}

int nka_hip_batch_get_state(nka_hip_batch_t b, int32_t sys, int32_t *subspace, int32_t *pending, int32_t *first, int32_t *last,
                            int32_t *free_, int32_t *next, int32_t *prev, double *h, double *c) {
  if (int rc = check_sys(b, sys, "batch_get_state")) return rc;
  std::vector<int32_t> ic;
  std::vector<double> dc;
  if (int rc = fetch_sys(b, sys, ic, dc)) return rc;
  nka_host::snapshot_unpack(ic.data(), dc.data(), b->k.mvec, subspace, pending, first, last, free_, next, prev, h, c);
  return 0;
}

int nka_hip_batch_get_reductions(nka_hip_batch_t b, int32_t sys, double *red_out) {
  if (int rc = check_sys(b, sys, "batch_get_reductions")) return rc;
  if (!red_out) return fail(NKA_HIP_EINVAL, "batch_get_reductions: null argument");
  HIP_TRY(hipSetDevice(b->device));
  const Ctl c = batch_ctl(b->k, sys);
  HIP_TRY(hipMemcpyAsync(red_out, c.red(), sizeof(double) * (size_t)c.red_count(), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

static int batch_get_slot(nka_hip_batch_t b, bool v, int32_t sys, int32_t slot, double *host_out) {
  if (int rc = check_sys(b, sys, v ? "batch_get_v" : "batch_get_w")) return rc;
  if (slot < 1 || slot > b->k.mvec + 1) return fail(NKA_HIP_EINVAL, "batch_get_w/v: slot out of range");
  if (!host_out) return fail(NKA_HIP_EINVAL, "batch_get_w/v: null argument");
  HIP_TRY(hipSetDevice(b->device));
  if (b->lanes) return nka_batch_lanes_get_slot(b, v, sys, slot, host_out);      // (gathered from the interleaved slots)
  if (b->storage == NKA_HIP_BATCH_STORE_F32) {
    // the slot of the pending pair: its binary64 row of the pending buffers; any other slot: the stored floats, widened
    std::vector<int32_t> ic;
    std::vector<double> dc;
    if (int rc = fetch_sys(b, sys, ic, dc)) return rc;
    int32_t pending = 0, first = 0;
    nka_host::snapshot_unpack(ic.data(), dc.data(), b->k.mvec, nullptr, &pending, &first, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (pending && first == slot) {
      const double *src = (v ? b->pend_v : b->pend_w) + (size_t)sys * b->k.stride;
      HIP_TRY(hipMemcpyAsync(host_out, src, sizeof(double) * (size_t)b->k.n, hipMemcpyDeviceToHost, b->stream));
      HIP_TRY(hipStreamSynchronize(b->stream));
      return 0;
    }
    const float *src = reinterpret_cast<const float *>(v ? b->k.v : b->k.w) + (size_t)sys * b->k.sys_stride + (size_t)(slot - 1) * b->k.stride;
    std::vector<float> stage((size_t)b->k.n);
    HIP_TRY(hipMemcpyAsync(stage.data(), src, sizeof(float) * stage.size(), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t i = 0; i < stage.size(); i++) host_out[i] = (double)stage[i];
    return 0;
  }
  const double *src = (v ? b->k.v : b->k.w) + (size_t)sys * b->k.sys_stride + (size_t)(slot - 1) * b->k.stride;
  HIP_TRY(hipMemcpyAsync(host_out, src, sizeof(double) * (size_t)b->k.n, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}
int nka_hip_batch_get_w(nka_hip_batch_t b, int32_t sys, int32_t slot, double *host_out) { return batch_get_slot(b, false, sys, slot, host_out); }
int nka_hip_batch_get_v(nka_hip_batch_t b, int32_t sys, int32_t slot, double *host_out) { return batch_get_slot(b, true, sys, slot, host_out); }

// FNV-1a over the system's two control blocks, as nka_hip_state_digest
int nka_hip_batch_state_digest(nka_hip_batch_t b, int32_t sys, uint64_t *digest) {
  if (int rc = check_sys(b, sys, "batch_state_digest")) return rc;
  if (!digest) return fail(NKA_HIP_EINVAL, "batch_state_digest: null argument");
  std::vector<int32_t> ic;
  std::vector<double> dc;
  if (int rc = fetch_sys(b, sys, ic, dc)) return rc;
  *digest = nka_host::snapshot_digest(ic, dc);
  return 0;
}

}  // extern "C"
