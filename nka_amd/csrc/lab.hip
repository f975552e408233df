// lab.hip -- the builder's lab: the entry points of include/nka_hip_diag.h, linked into libnka_hip_diag.so beside the
// product's own objects (nka_amd/csrc/Makefile).  Host code only: it defines and launches no kernel; what it enqueues goes
// through the product's functions (handles.hpp), so the lab library runs the product's kernels and nothing else.
#include "handles.hpp"
#include "nka_chain.hpp"
#include "../../include/nka_hip_diag.h"

#include <algorithm>
#include <string>

using namespace nka;
using namespace nka_detail;

extern "C" {

// The s_memtime stamps of the last scalar step (written only by a -DNKA_SOLVE_STAMPS build, `make stamps`).
int nka_hip_get_stamps(nka_hip_t a, double *out16) {
  if (!a || !out16) return fail(NKA_HIP_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(a->device));
  HIP_TRY(hipMemcpyAsync(out16, a->ctl.stamps(), sizeof(double) * kStamps, hipMemcpyDeviceToHost, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  return 0;
}

// The skip of the last vector as the device sees it: plan flag, hysteresis countdown, pending repair, repairs so far.
int nka_hip_get_skip_state(nka_hip_t a, int32_t out4[4]) {
  if (!a || !out4) return fail(NKA_HIP_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(a->device));
  HIP_TRY(hipMemcpyAsync(out4, a->ctl.ic + IC_PLAN_SKIP, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  return 0;
}

// The deferred v of the pending pair as the device sees it: the word, and how many entries the last PB replayed (0: none).
int nka_hip_get_defer_state(nka_hip_t a, int32_t out2[2]) {
  if (!a || !out2) return fail(NKA_HIP_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(a->device));
  long long w[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(w, a->ctl.pc + PC_VDEFER, sizeof w, hipMemcpyDeviceToHost, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  out2[0] = (int32_t)w[0];
  out2[1] = (int32_t)w[1];
  return 0;
}

int nka_hip_set_grid(nka_hip_t a, int32_t pa, int32_t pb) {
  if (!a) return fail(NKA_HIP_EINVAL, "null handle");
  const int32_t v[2] = {pa, pb};
  for (int i = 0; i < 2; i++) {
    if (v[i] < 0 || v[i] * a->num_cu > kMaxGrid) return fail(NKA_HIP_EINVAL, "blocks per CU out of range");
    a->bpc[i] = v[i];   // 0 = automatic
  }
  return 0;
}

// start + x[0]*y[0] + x[1]*y[1] + ... as the per-sum reference-order kernel forms it (k_chain_sums on one workgroup),
// over ANY two device arrays: the test bench of chain_block_summary / _apply (walk = 1: every block element after element).
int nka_hip_debug_chain_sum(nka_hip_t a, const double *x, const double *y, int64_t n, double start, int32_t walk, double *sum,
                            float *ms) {
  if (!a || !sum || n < 0 || (n > 0 && (!x || !y))) return fail(NKA_HIP_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(a->device));
  double *slot = a->ctl.red() + 2 + a->mvec;
  struct Events {          // (destroyed on EVERY exit)
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); }
  } ev;
  hipEvent_t &e0 = ev.e[0], &e1 = ev.e[1];
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipMemcpyAsync(slot, &start, sizeof(double), hipMemcpyHostToDevice, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  const bool many = (walk & 2) != 0;                    // (bit 1: through k_chain_blocks / _predict / _apply)
  if (many) {
    const int keep = a->chain_many;
    a->chain_many = 1;
    const bool ready = chain_many_ready(a, 1, n);
    a->chain_many = keep;
    if (!ready) return fail(NKA_HIP_EINVAL, "debug_chain_sum: no full block, or no memory for the block arrays");
  }
  HIP_TRY(hipEventRecord(e0, a->stream));
  if (many) {
    const int keepw = a->chain_walk;
    a->chain_walk = walk & 1;
    const int rc = chain_many_stage(a, x, 0, (int)kChainProbe, 1, 0, 1, y, n);
    a->chain_walk = keepw;
    if (rc) return rc;
  } else {
    chain_sum_probe(a, x, y, n, walk & 1);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, a->stream));
  HIP_TRY(hipMemcpyAsync(sum, slot, sizeof(double), hipMemcpyDeviceToHost, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  if (ms) HIP_TRY(hipEventElapsedTime(ms, e0, e1));
  return 0;
}

// Measurement aid: the PA launches of the NEXT update, `reps` times back to back on the
// handle's stream, timed with HIP events (mean ms per repetition).  PA only writes
// scratch (partials, red[]), so the state is unchanged.
int nka_hip_debug_time_pa(nka_hip_t a, const double *f, int32_t reps, float *ms_mean) {
  if (!a || !f || !ms_mean || reps < 1) return fail(NKA_HIP_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(a->device));
  if (int rc = check_device_span(f, a->n, "debug_time_pa: f")) return rc;
  const int vec = (reinterpret_cast<uintptr_t>(f) % 16) == 0 ? 2 : 1;
  const int older_ub = a->pending ? std::max(a->list_ub - 1, 0) : a->list_ub;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  enqueue_pa(a, f, vec, older_ub);   // warm
  HIP_TRY(hipEventRecord(e0, a->stream));
  for (int r = 0; r < reps; r++) enqueue_pa(a, f, vec, older_ub);
  HIP_TRY(hipEventRecord(e1, a->stream));
  HIP_TRY(hipStreamSynchronize(a->stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  *ms_mean = ms / reps;
  return 0;
}

int nka_hip_set_tuning(nka_hip_t a, const char *key, int32_t value) {
  if (!a || !key) return fail(NKA_HIP_EINVAL, "null argument");
  const std::string k(key);
  if (k == "pb_pipe") {
    if (value != -1 && value != 0 && !(value > 200 && value <= 204))
      return fail(NKA_HIP_EINVAL, "pb_pipe: -1 (auto), 0 (every load of a tile in flight), 201..204 (rolling window, 1..4 blocks per CU)");
    a->pb_pipe = value;
  } else if (k == "pa_pipe") {
    if (value != -1 && value != 0 && !(value > 200 && value <= 204))
      return fail(NKA_HIP_EINVAL, "pa_pipe: -1 (auto), 0 (every load of a tile in flight), 201..204 (rolling window, 1..4 blocks per CU)");
    a->pa_pipe = value;
  } else if (k == "pb_tile") {
    if (value != -1 && value != 1 && value != 2) return fail(NKA_HIP_EINVAL, "pb_tile: -1 (auto), 1, 2");
    a->pb_tile = value;
  } else if (k == "pb_tickets") {
    if (value != -1 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(NKA_HIP_EINVAL, "pb_tickets: -1 (auto), 0 (static tile mapping), 1, 2, 4, 8 (ticket counters)");
    a->pb_tickets = value;
  } else if (k == "fail_after_solve") {   // 1: the NEXT update returns NKA_HIP_EHIP right behind its enqueued scalar step
    a->fail_after_solve = value != 0;
  } else if (k == "prime_pad") {      // -1 automatic = 1: list lengths 23 / 29 / 31 run the next width (one dead ring slot); 0: exact widths
    if (value < -1 || value > 1) return fail(NKA_HIP_EINVAL, "prime_pad: -1, 0, 1");
    a->prime_pad = value;
  } else if (k == "skip_last") {      // -1 automatic (from a vector length on), 0 never, 1 wherever the launch allows it, at any n
    if (value < -1 || value > 1) return fail(NKA_HIP_EINVAL, "skip_last: -1, 0, 1");
    a->skip_last = value;
  } else if (k == "defer_v") {        // -1 automatic (from a vector length on), 0 never, 1 wherever the launch allows it, at any n
    if (value < -1 || value > 1) return fail(NKA_HIP_EINVAL, "defer_v: -1, 0, 1");
    a->defer_v = value;
  } else if (k == "chain_many") {    // -1 automatic, 0: one compute unit per reference-order sum at every length, 1: many wherever blocks exist
    if (value < -1 || value > 1) return fail(NKA_HIP_EINVAL, "chain_many: -1, 0, 1");
    a->chain_many = value;
  } else if (k == "chain_walk") {     // 1: the per-sum reference-order kernel walks every block (no summaries): same bits, for A/B
    a->chain_walk = value != 0;
  } else if (k == "serial_solve") {
    a->serial_solve = value != 0;
  } else if (k == "list_word") {       // 0: the host's own bound only (the behaviour before round 4), for A/B runs
    a->word_off = value == 0;
  } else {
    return fail(NKA_HIP_EINVAL, "unknown tuning key: " + k);
  }
  return 0;
}

int nka_hip_vec_set_tuning(nka_hip_vec_ws_t ws, const char *key, int32_t value) {
  if (!ws || !key) return fail(NKA_HIP_EINVAL, "null argument");
  if (std::string(key) == "tickets") {
    if (value != -1 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(NKA_HIP_EINVAL, "tickets: -1 (auto), 0 (static tile mapping), 1, 2, 4, 8 (ticket counters)");
    ws->ticket_groups = value;
    return 0;
  }
  return fail(NKA_HIP_EINVAL, std::string("unknown tuning key: ") + key);
}

}  // extern "C"
