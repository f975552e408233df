// handles.hpp -- the two handle types of the C ABI and the host functions the library's translation units share.
// Private to nka_amd/csrc: nka_hip.hip (the accelerator), vec_ops.hip (the abstract-vector hooks), nka_batch.hip (the batched
// accelerator) and lab.hip (the entry points of include/nka_hip_diag.h, linked into libnka_hip_diag.so only) include it.
// Declarations only: every function below is defined in nka_hip.hip.  Of the device side only the layout of the control block
// (nka_ctl.hpp) comes with it: a unit that launches kernels includes nka_device.hpp / nka_chain.hpp / nka_kernels.hpp itself.
#pragma once

#include "../../include/nka_hip.h"
#include "../../include/nka_hip_ext.h"
#include "../../include/nka_hip_vec.h"
#include "nka_ctl.hpp"
#include "host_logic.hpp"
#include "rccl_dl.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace nka_detail {
// one thread-local error string per library (nka_hip_last_error)
int set_error(int code, const std::string &msg);
std::string last_error();
bool &span_check_failed();   // (thread-local) set by a failing check_device_span
int check_device_span(const void *p, int64_t n, const char *what);
int check_device_span_i32(const void *p, int64_t n, const char *what);
void invalidate_span_cache();
void register_allocation(const void *p, size_t bytes, const void *owner);
void unregister_owner(const void *owner);
void unregister_allocation(const void *p);
int resolve_flavor(int32_t *flavor_io, const char *who);   // NKA_HIP_FLAVOR_DEFAULT / NKA_HIP_FLAVOR (include/nka_hip.h)

// pieces of an update, for the lab (lab.hip)
void enqueue_pa(nka_hip_t a, const double *f, int vec, int older_ub);
bool chain_many_ready(nka_hip_t a, int nsum_max, long long n = -1);
int chain_many_stage(nka_hip_t a, const double *f, int rcp, int set, int with_f, int ub, int nsum, const double *probe = nullptr,
                     long long n_probe = -1);
// start + x[0]*y[0] + ... + x[n-1]*y[n-1] by k_chain_sums on one workgroup, into the probe slot of red[] (walk: chain_walk)
void chain_sum_probe(nka_hip_t a, const double *x, const double *y, long long n, int walk);
}  // namespace nka_detail

static inline int fail(int code, const std::string &msg) { return nka_detail::set_error(code, msg); }

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      (void)hipGetLastError(); /* reported here: do not leave it for a later hipGetLastError() to find */ \
      return fail(e_ == hipErrorOutOfMemory ? NKA_HIP_ENOMEM : NKA_HIP_EHIP,                \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    }                                                                                       \
  } while (0)

struct nka_hip_state {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t n = 0;
  int32_t mvec = 0;
  double vtol = 0.01;
  int flavor = NKA_HIP_FLAVOR_F08;
  nka::Vecs vs{};
  nka::Ctl ctl{};
  double *partials = nullptr;
  unsigned *tickets = nullptr; // tile-ticket counters of the rolling-window PB (kTicketWords, zero between launches)
  double *f_stage = nullptr;  // device staging for the host-array entry point
  double *hd_scratch = nullptr;  // device vector for the operands of a user host dot product (set_host_dot)
  // what the host knows without reading the device back
  bool pending = false;
  int list_ub = 0;            // upper bound on the list length
  // ... and what the device tells it without being asked: the list word (Ctl::hw, nka_ctl.hpp), one 64-bit word
  // in pinned host memory that PB of update number u overwrites with (u, list length at its exit).
  unsigned long long *list_word = nullptr;
  int64_t seq = 0;            // updates enqueued so far; the next one is number seq + 1
  int64_t word_valid_after = 0;      // words of updates numbered <= this are stale (restart; a word of 0 = none yet)
  std::vector<int64_t> relaxed_after;  // relax() calls that dropped a pending pair, by the number of the update before them
  bool word_off = false;      // the handle's stream was seen capturing (replays change the list behind the word), or
                              // the diagnostic switch "list_word" = 0
  // out-of-place updates (nka_hip_accel_update_swap): the slot -> buffer tables live on the device (Ctl::pc); the host
  // knows only the two buffers it can hand out next
  bool swapped = false;       // a table entry may differ from base + (slot-1)*stride: host-side accessors read the tables
  double *spare_w = nullptr, *spare_v = nullptr;   // free buffers the host knows of (given away by the next swap update)
  bool swap_pending = false;  // the buffers the last swap update displaced have not been collected yet (record word 3)
  int64_t swap_seq = 0;       // number of that update
  const double *last_acc = nullptr;   // the accelerated f lent by the last out-of-place update (read only for the caller)
  std::vector<void *> extra_allocs;   // the two spare buffers allocated at the first swap update (freed at destroy)
  // Who holds which buffer, as far as the HOST can know it: `taken` = every buffer outside the two slot-major
  // allocations that a table entry may name (callers' buffers handed in, the two extra allocations); `lent` = the free
  // buffers handed to the caller for its NEXT input (they may lie anywhere, the slot-major allocations included).  A
  // buffer may enter an update only if the library does not hold it: it is lent, or it is foreign to both.
  nka_host::BufferBook book;          // .taken / .lent (host_logic.hpp)
  bool captured = false;      // the handle's stream was seen capturing: replays re-issue the scalar step with the ARGUMENTS of
                              // the capture, so from then on it loads the slot -> buffer tables instead of computing them
  bool solve63_raised = false;   // k_solve_rows<63> has its dynamic-LDS limit raised on this handle's device
  bool poisoned = false;      // a HIP call failed AFTER the scalar step of an update was enqueued: the lists on the device
                              // are ahead of the vectors; every later call but destroy returns NKA_HIP_ESTATE
  // launch geometry
  int num_cu = 256;
  int bpc[2] = {0, 0};        // blocks per CU of PA, PB; 0 = automatic (see grid_for)
  char devname[64] = {0};
  int pa_pipe = -1;           // form of PA: 0 = k_dots (every load of a tile in flight; any list length), 201..204 = k_dots_win
                              // (rolling window) with 1..4 blocks per CU, -1 = automatic (see enqueue_pa)
  int pb_pipe = -1;           // form of PB: 0 = k_combine, 201..204 = k_combine_win, -1 = automatic (see enqueue_pb)
  int pb_flags = 0;           // kPbNoStoreW | kPbNoStoreF while an out-of-place update is being enqueued, else 0
  int pb_tile = -1;           // tile width of the rolling-window PB for short lists: -1 automatic (double-width tiles
                              // when the tickets apply), 1 = 512 elements, 2 = 1024 elements
  int pb_tickets = -1;        // tile tickets of the rolling-window PB: -1 automatic, 0 static tile mapping,
                              // 1, 2, 4, 8 = that many ticket counters (see k_combine_win)
  double *chain_pred = nullptr;   // reference-order sums of the longest vectors (k_chain_blocks ...): per sum and block of 1024, the block
  void *chain_summ = nullptr;     // sum / the predicted running sum, and the block's summary; allocated at the first such update
  long long chain_cap = 0;        // (sums x blocks the two arrays hold)
  int chain_many = -1;            // diagnostic switch "chain_many": -1 automatic (from kChainManyMin elements on), 0 never, 1 whenever blocks exist
  int chain_walk = 0;         // diagnostic switch "chain_walk": k_chain_sums walks every block element after element (A/B of chain_block_summary / _apply)
  int fail_after_solve = 0;   // lab switch "fail_after_solve": the next update fails as if a HIP call behind its scalar step had
                              // (the test of the poisoned-handle path: the failure itself cannot be provoked from outside)
  int prime_pad = -1;         // list lengths 23, 29, 31 (primes: the only ring of their window kernels is the whole width -- up to 311
                              // VGPRs and scratch in PA, every load of a tile in flight in PB) run the next width with ONE dead ring
                              // slot: -1 / 1 on (automatic), 0 off.  In-process A/B at n = 1e7 (profiles/r05/multipass.txt): update
                              // -12.7 % at m = 31, -3.4 % at 29, -0.3 % at 23 (compact); -11 / -4.4 / -2.9 % in the src-F08 rounding
  int skip_last = -1;         // PA leaves out the vector a full list drops for capacity (nka_hip.hip, skip_last_applies): -1 automatic
                              // (from a vector length on), 0 never, 1 wherever the launch allows it (diagnostic switch "skip_last")
  int defer_v = -1;           // PB leaves the pending pair's v unstored and the next PB replays it (nka_hip.hip, defer_v_applies;
                              // k_combine_win, DEFER): -1 automatic (from a vector length on), 0 never, 1 wherever the launch
                              // allows it (diagnostic switch "defer_v")
  bool v_deferred = false;    // an update of this handle passed "may defer" and nothing has materialised the slot since: the
                              // device may hold PC_VDEFER (the host never reads the word: ensure_v launches guarded kernels)
  bool pb_defer = false;      // the update being enqueued is one that may defer: its scalar step writes the replay plan, its
                              // PB is the DEFER instantiation
  int pa_skip = 0;            // the PA / final sums being enqueued: kSkipMay, kSkipRepair (nka_device.hpp) or 0
  bool state_in_global = false;  // mvec > 140: h, c and the links no longer fit the LDS of one CU; the one-lane
                                 // scalar kernels then work on the control block in global memory (slow, unlimited)
  bool serial_solve = false;  // NKA_HIP_SERIAL_SOLVE=1: reference loops verbatim on one lane
  int sum_order = NKA_HIP_SUMS_AUTO;   // nka_hip_set_sum_order: reference-order sums (k_dots_ordered) within one tile / always / never
  bool debug = false;         // NKA_HIP_DEBUG=1: check defined() on entry of every update, like the
                              // reference built without -DNDEBUG (F08:257); synchronises
  // distribution hook
  nka_hip_allreduce_fn allreduce = nullptr;
  void *allreduce_ctx = nullptr;
  ncclComm_t comm = nullptr;
  // peer-to-peer exchange (nka_hip_p2p_export / _attach; nka_ctl.hpp: struct P2P)
  nka::P2P p2p{};                          // base == nullptr: none
  void *p2p_mail = nullptr;           // this rank's mailbox (fine-grained device memory, exported through hipIpc)
  std::vector<void *> p2p_opened;     // the peers' mailboxes as mapped here (hipIpcCloseMemHandle at detach)
  void *p2p_dev = nullptr;            // offsets table, exchange counter, status word
  int p2p_ranks = 0;                  // ranks the mailbox was sized for
  bool p2p_fused = false;             // the PA being enqueued sends its sums itself (update_impl)
  int pa_normed = 0;                  // the PA being enqueued sums on the ROUNDED w1' (NKA_HIP_SUMS_BLOCKED_ROUNDED): 0 no, 1 d/s, 3 (1/s)*d
  int shard_rank = -1, shard_n = 0;   // position of this rank's slice in the global vector (nka_hip_set_shard; set by
                                      // nka_hip_comm_init_rank too): only the sharded reference-order sums need it
  bool needs_comm = false;    // a deep copy of an accelerator that reduced through the built-in RCCL communicator: the
                              // communicator belongs to the original, and rank-local sums would be silently wrong
  nka_hip_host_dot_fn host_dot = nullptr;   // user dot product on host copies (compatibility path)
  void *host_dot_ctx = nullptr;
  double *wgt = nullptr;      // diagonal dot-product weights (nka_hip_set_dot_weights): n doubles, allocated at the first set,
                              // freed at destroy only (a captured update holds the address)
  unsigned long long *wgt_chk = nullptr;   // two words for the set-time check of the weights (k_check_weights), freed at destroy
  bool weighted = false;      // the passes that form sums run their WGT = true instantiations (k_norm_diff, k_dots, k_dots_win)
  // instrumentation
  // kTimingEvents events per update, in a ring of timing_cap updates
  int timing_cap = 0;
  int64_t timing_count = 0;   // updates recorded since set_timing
  int timing_stride = 1;      // record the events of every stride-th update only (tuning key "timing_stride"):
  int64_t update_seq = 0;     // four event records widen the kernel boundaries of an update by ~15 us
  bool timing_this = false;   // the update in progress is a recorded one
  std::vector<hipEvent_t> ev;
};

struct nka_hip_vec_ws {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cu = 256;
  double *partials = nullptr;  // kMaxGrid
  unsigned *tickets = nullptr; // tile-ticket counters of k_update_many_keep_win (kTicketWords, zero between launches)
  int ticket_groups = -1;      // -1 automatic, 0 static tile mapping, 1/2/4/8 counters (nka_hip_vec_set_tuning "tickets")
  double *host_results = nullptr; // pinned, 2*kManyMax+2 doubles
  double *host_results_dev = nullptr;  // its device-side address: the final-sum kernel writes straight into host
                                       // memory (no copy kernel, no staging)
  // parallel-aware reductions ("the vector base class reduction methods will necessarily be
  // parallel-aware", src-F08-vector/README.md:16-22): every sum a reduction returns to the host is first
  // summed over the ranks -- on the device by `allreduce` (stream-ordered; built-in: RCCL), and/or on the
  // host by `host_allreduce` after the stream has been synchronised
  nka_hip_allreduce_fn allreduce = nullptr;
  void *allreduce_ctx = nullptr;
  nka_hip_host_allreduce_fn host_allreduce = nullptr;
  void *host_allreduce_ctx = nullptr;
  ncclComm_t comm = nullptr;
  double *red_dev = nullptr;      // 2*kManyMax+2 doubles: the sums of one reduction in canonical layout
  int sum_order = 0;              // nka_hip_vec_set_sum_order: 1 = dot() sums element after element, unfused (k_dot_ordered)
};
