// nka_batch_rows.hip -- THE SCALAR STEP ON WAVEFRONT 0 of a narrow batch (nka_hip_batch_create_rows with
// nka_hip_batch_set_scalar_step(b, NKA_HIP_BATCH_SCALAR_WAVEFRONT); include/nka_hip_batch.h, NARROW ROWS): the instances of
// k_batch_update (nka_batch_kernel.hpp, the one kernel body of the narrow batch) whose trailing pack ends in a BatchRows<NLMAX>.
// Phase 4 of such an instance is batch_scalar_step_rows<NLMAX> (nka_batch_dev.hpp) on the 64 lanes of wavefront 0, between the
// two barriers that stand around the one-thread statements in every other instance; wavefronts 1-3 go on to the second barrier.
// Every other phase is the text every instance compiles.  No flags, no spinning, no atomics, no cooperative launch, no function
// attribute: the matrix of the step lies in dynamic LDS behind the working copy (nka_host::batch_rows_lds: 9.2 KB at mvec = 20,
// 20.5 KB at 32, four workgroups per CU by LDS).
//   A unit of its own for the build's sake only: with these 96 instances (32 fast packs -- three flavours x weights x step x
// lengths in binary64, weights x step x lengths in binary32 -- x 11 / 21 / 33 rows) nka_batch.hip would be the longest unit of
// the library.  The host entries, the setters and their refusals stay in nka_batch.hip, which calls the two functions below when
// a call is enqueued: the instance and the LDS size it asks for are chosen together, here, so a captured call keeps both.
//   FAST SUMS ONLY (ORDERED = false): nka_hip_batch_set_scalar_step and nka_hip_batch_set_sum_order refuse every state in which
// a reference-order launch would meet the wavefront step, so nothing is downgraded here.
#include "nka_batch_dev.hpp"      // BatchArgs, the sweeps, batch_scalar_step_rows, the handle
#include "nka_batch_kernel.hpp"   // StepArgs, LenArgs, BatchRows<NLMAX>, k_batch_update

#include <cstdint>

using namespace nka;

namespace {

template <int COMB, bool WGT, int NLMAX, class... Step>
void launch_rows_nl(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  const size_t lds = (size_t)nka_host::batch_rows_lds(b->k.mvec).bytes();
  hipLaunchKernelGGL((k_batch_update<COMB, false, WGT, Step..., BatchRows<NLMAX>>), dim3((unsigned)b->k.nsys), dim3(kBatchThreads), lds, b->stream,
                     b->k, f, ld, active, WGT ? (const double *)b->wgt : (const double *)nullptr, WGT ? b->wgt_stride : (int64_t)0, step...,
                     BatchRows<NLMAX>{});
}
// NLMAX from mvec, which is fixed at creation: 11 / 21 / 33 rows (nka_host::batch_rows_nlmax)
template <int COMB, bool WGT, class... Step>
void launch_rows_as(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  switch (nka_host::batch_rows_nlmax(b->k.mvec)) {
    case 11: launch_rows_nl<COMB, WGT, 11>(b, f, ld, active, step...); break;
    case 21: launch_rows_nl<COMB, WGT, 21>(b, f, ld, active, step...); break;
    default: launch_rows_nl<COMB, WGT, nka_host::kWideRowsMaxList>(b, f, ld, active, step...);
  }
}
template <int COMB, class... Step>
void launch_rows_wgt(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (b->weighted) launch_rows_as<COMB, true>(b, f, ld, active, step...); else launch_rows_as<COMB, false>(b, f, ld, active, step...);
}
// the ladder of launch_flavor (nka_batch.hip): binary32 storage runs the default flavour only; the lengths stand behind the step,
// the pending buffers behind the lengths
template <class... Step>
void launch_rows(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active, Step... step) {
  if (b->storage == NKA_HIP_BATCH_STORE_F32) {
    const Store32Args s32{b->pend_w, b->pend_v};
    if (b->has_len) launch_rows_wgt<2>(b, f, ld, active, step..., LenArgs{b->len}, s32); else launch_rows_wgt<2>(b, f, ld, active, step..., s32);
    return;
  }
  auto flavor = [&](auto... pack) {
    switch (b->flavor) {
      case NKA_HIP_FLAVOR_F08_VECTOR: launch_rows_wgt<1>(b, f, ld, active, pack...); break;
      case NKA_HIP_FLAVOR_C: launch_rows_wgt<2>(b, f, ld, active, pack...); break;
      default: launch_rows_wgt<0>(b, f, ld, active, pack...);
    }
  };
  if (b->has_len) flavor(step..., LenArgs{b->len}); else flavor(step...);
}

}  // namespace

void nka_batch_rows_update(nka_hip_batch_t b, double *f, int64_t ld, const int32_t *active) { launch_rows(b, f, ld, active); }

void nka_batch_rows_step(nka_hip_batch_t b, double *f, int64_t ld, double *x, int64_t ldx, int32_t *active, const double *tol, double *fnorm) {
  launch_rows(b, f, ld, active, StepArgs{x, x ? ldx : 0, tol, fnorm});
}
