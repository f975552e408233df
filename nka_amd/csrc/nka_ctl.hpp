// nka_ctl.hpp -- the layout of the device-resident control block: the indices of its three arrays, Ctl, Vecs and the record
// of the peer-to-peer exchange.  Plain C++17, no HIP needed: the kernels, the host code of the library and host_logic.hpp
// (which tests/c compiles with g++ under sanitizers) all read the layout from here and from nowhere else.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NKA_HOST_DEVICE __host__ __device__
#else
#define NKA_HOST_DEVICE
#endif

namespace nka {

// ---- indices into the small device-resident control arrays -----------------
// int32 control block
enum {
  IC_SUBSPACE = 0,
  IC_PENDING = 1,
  IC_FIRST = 2,
  IC_LAST = 3,
  IC_FREE = 4,
  IC_NEW = 5,          // slot that receives (f_in, f_out) in the current update
  IC_NCOMB = 6,        // number of (slot, coefficient) pairs in the combine plan
  IC_PLAN_PENDING = 7, // plan for PA of the NEXT update: `pending` at its entry
  IC_PLAN_FIRST = 8,   //   slot holding the pending pair
  IC_PLAN_NOLDER = 9,  //   number of list entries to dot against
  IC_NRELAX = 10,      // count of s == 0 events (diagnostic)
  IC_NORMED = 11,      // this update normalises the pending pair (pending && s != 0)
  // SKIP OF THE LAST VECTOR (k_dots_win): with the list full, PA of the NEXT update may leave out the oldest w -- the capacity
  // drop F08:301-309 ends the list before its sums are looked at -- when the launch allows it too (argument `skip`).
  IC_PLAN_SKIP = 12,   //   plan for PA of the NEXT update: 1 = may skip (written by the scalar step: IC_SKIP_HOLD == 0)
  IC_SKIP_HOLD = 13,   //   updates still to run WITHOUT the skip after a repair (hysteresis, counts down)
  IC_REDO = 14,        //   the scalar step needed the skipped sums after all: the guarded repair launches behind it run
  IC_NREDO = 15,       //   count of such repairs (diagnostic)
  IC_HEADER = 16
};
// double control block
enum { DC_VTOL = 0, DC_S = 1, DC_HEADER = 2 };
// pointer control block (Ctl::pc)
enum {
  PC_FIRST_W = 0,  // w of the pending pair at the entry of the NEXT update (PA)
  PC_NEW_W = 1,    // w, v buffers of the slot that receives (f_in, f_out) in the current update (PB)
  PC_NEW_V = 2,
  PC_OLD_W = 3,    // what an out-of-place update displaced from that slot: handed to the caller /
  PC_OLD_V = 4,    //   kept as the library's next spare
  PC_WGT = 5,      // the diagonal dot-product weights of nka_hip_set_dot_weights (read by the WGT = true passes only)
  // DEFERRED v OF THE PENDING PAIR (k_combine_win<.., DEFER = true>, nka_kernels.hpp).  The two words live here and not in the
  // int32 header: that header is full, its length is part of the batch layouts, and a word in ic / dc would show in the state
  // digest, which a deferring handle must share with one that never defers.
  PC_VDEFER = 6,   // != 0: the v buffer of the pending pair does NOT hold f_out yet; f_out = w + sum c_k u_k over the combine plan
                   //   as it stands (comb_v / comb_c / IC_NCOMB: nothing rewrites them before the next scalar step)
  PC_VREPLAY = 7,  // written by the scalar step for ITS PB: 0 = v of the pending pair is in memory, np > 0 = form it from the np
                   //   entries of the replay plan below
  PC_HEADER = 8
};

constexpr int kMaxPerPass = 32;  // largest MAXL / MAXK instantiated
constexpr int kMaxGrid = 4096;   // upper bound on persistent grid size (partials buffer)

constexpr int kStamps = 16;      // s_memtime stamps of the scalar step, written only when NKA_SOLVE_STAMPS is defined

struct Ctl {
  int32_t *ic;         // header, then next[M1+1], prev[M1+1], plan_slots[M1+pad], comb_slots[M1+pad]
  double *dc;          // header, then h[(M1+1)^2], c[M1+1], comb_c[M1+pad], red[2+2*mvec]
  int32_t mvec;
  // LIST WORD: one 64-bit word in pinned host memory (nullptr: none) that block 0 of PB overwrites with
  // (number of this update << kListWordLenBits | list length at its exit), see list_word_publish (nka_device.hpp); `seq` = the
  // number the host gave this update.  The host reads it WITHOUT synchronising to learn that dependence drops
  // (F08:326-345) have made the list shorter than its own bookkeeping says (nka_hip.hip: list_bound_now).
  unsigned long long *hw;
  unsigned long long seq;
  // ADDRESS CONTROL BLOCK.  The streaming passes take the ADDRESSES of the stored vectors from here, not slot numbers:
  // wtab / vtab map slot -> buffer (at creation slot k -> (k-1)*stride of the two slot-major allocations; the out-of-place
  // entry nka_hip_accel_update_swap exchanges entries with buffers of the caller), and the scalar kernels, which alone know
  // the slots, resolve them when they write the plans.  Every entry is an OFFSET IN DOUBLES FROM Vecs::w (any buffer of the
  // device, the caller's included, is some 64-bit offset from it): a pointer read from memory carries no address space and
  // the compiler would reach it with FLAT loads -- one counter for LDS and memory, every wait a wait for everything (the
  // first version of this block did: PB -13 %) -- while vs.w + offset is a global address like any kernel argument.
  long long *pc;
  NKA_HOST_DEVICE long long *plan_w() const { return pc + PC_HEADER; }          // w of PA's older entries [m1p]
  NKA_HOST_DEVICE long long *comb_w() const { return plan_w() + m1p(); }        // w of PB's pairs [m1p]
  NKA_HOST_DEVICE long long *comb_v() const { return comb_w() + m1p(); }        // v of PB's pairs [m1p]
  NKA_HOST_DEVICE long long *wtab() const { return comb_v() + m1p(); }          // slot -> w buffer [m1+1], 1-based
  NKA_HOST_DEVICE long long *vtab() const { return wtab() + (m1() + 1); }       // slot -> v buffer [m1+1]
  // REPLAY PLAN (PC_VREPLAY): the combine plan of the update that deferred, in its list order -- entry j: the buffer of u_j, the
  // coefficient it had THEN, the coefficient it has NOW -- and one word whose bit j says that entry j is still on the list.  The
  // new plan minus the pending pair is a subsequence of the old one (drops keep the order), so this is all PB needs; a dropped
  // entry is skipped, never multiplied by zero (-0 and non-finite values would change).
  NKA_HOST_DEVICE long long *rp_v() const { return vtab() + (m1() + 1); }                                   // [m1p]
  NKA_HOST_DEVICE double *rp_cprev() const { return reinterpret_cast<double *>(rp_v() + m1p()); }           // [m1p]
  NKA_HOST_DEVICE double *rp_cnew() const { return rp_cprev() + m1p(); }                                    // [m1p]
  NKA_HOST_DEVICE long long *rp_keep() const { return rp_v() + 3 * m1p(); }                                 // [1]
  NKA_HOST_DEVICE constexpr int pc_count() const { return PC_HEADER + 3 * m1p() + 2 * (m1() + 1) + 3 * m1p() + 1; }
  // plan_slots / comb_slots / comb_c are padded by one pass width: the unrolled
  // kernels read (and ignore) entries up to the end of their last pass.
  NKA_HOST_DEVICE constexpr int m1() const { return mvec + 1; }
  NKA_HOST_DEVICE constexpr int m1p() const { return mvec + 1 + kMaxPerPass; }
  NKA_HOST_DEVICE int32_t *next() const { return ic + IC_HEADER; }
  NKA_HOST_DEVICE int32_t *prev() const { return next() + (m1() + 1); }
  NKA_HOST_DEVICE int32_t *plan_slots() const { return prev() + (m1() + 1); }
  NKA_HOST_DEVICE int32_t *comb_slots() const { return plan_slots() + m1p(); }
  NKA_HOST_DEVICE constexpr int ic_count() const { return IC_HEADER + 2 * (m1() + 1) + 2 * m1p(); }
  NKA_HOST_DEVICE double *h() const { return dc + DC_HEADER; }
  NKA_HOST_DEVICE double *c() const { return h() + (m1() + 1) * (m1() + 1); }
  NKA_HOST_DEVICE double *comb_c() const { return c() + (m1() + 1); }
  NKA_HOST_DEVICE double *red() const { return comb_c() + m1p(); }
  NKA_HOST_DEVICE constexpr int red_count() const { return 2 + 2 * mvec; }
  NKA_HOST_DEVICE double *stamps() const { return red() + red_count(); }   // kStamps cycle stamps (diagnostic builds)
  NKA_HOST_DEVICE constexpr int dc_count() const {
    return DC_HEADER + (m1() + 1) * (m1() + 1) + (m1() + 1) + m1p() + red_count() + kStamps;
  }
};
constexpr long long kNoBuffer = (long long)0x8000000000000000ull;      // "no buffer" among the offsets of Ctl::pc
constexpr int kListWordLenBits = 20;        // mvec + 1 <= 2^17 + 1 (nka_hip_create)

// red[] layout (raw sums of PA, d = w1 - f NOT yet divided by s):
//   [0] sum d^2, [1] <f,d>, [2+p] <d,w_older(p)>, [2+mvec+p] <f,w_older(p)>

struct Vecs {
  double *v, *w;       // slot k (1-based) at base + (k-1)*stride
  int64_t stride;      // in doubles, multiple of 32 (256 B)
  int64_t n;           // local vector length
};

// ---- PEER-TO-PEER EXCHANGE of the 2 + 2 mvec sums (round 5, opt-in: nka_hip_p2p_attach) -----------------------------------
// The one exchange of a sharded update is an all-reduce of 336 bytes: latency, not bandwidth.  Through RCCL it is a kernel of
// its own between the final sums and the scalar step.  Here every rank owns a MAILBOX in fine-grained device memory that its
// peers map through hipIpc: the final-sums kernel of rank p writes each sum it forms straight into row p of EVERY rank's
// mailbox (value, then -- released at system scope -- the number of the exchange as that entry's flag), and the scalar step of
// rank q starts by waiting, entry by entry, for the N flags and adding the N rows IN RANK ORDER: the same additions in the same
// order on every rank, hence the same bits -- no communication kernel, two kernel boundaries fewer.
//   mailbox of one rank: val[2][N][cap] doubles, then flag[2][N][cap] 64-bit words; slot = exchange number & 1.  Two slots
//   suffice: a rank can start exchange x+2 only after its scalar step of x+1 has seen EVERY peer's row of x+1, and a peer sends
//   x+1 only after its own scalar step has consumed x (stream order).
//   `xseq` (device memory of this rank): number of the NEXT exchange, advanced by whoever gathers; device-resident so that a
//   captured update replays correctly.  Peers' mailboxes are reached as BYTE OFFSETS from this rank's own (`off[q]`): a pointer
//   read from memory has no address space and would be accessed with FLAT instructions (see Ctl::pc).
//   A wait is bounded (`timeout_ticks` of the 100 MHz wall clock): a peer that never sends makes the gather store NaNs, raise
//   `status` and go on, so that the grid always drains; the host reports NKA_HIP_ECOMM at its next synchronising call.
struct P2P {
  char *base;                    // this rank's mailbox (nullptr: no peer-to-peer exchange)
  const long long *off;          // [n] byte offset of rank q's mailbox from `base` (device memory)
  unsigned long long *xseq;      // number of the next exchange (device memory, starts at 1)
  int *status;                   // != 0: a wait timed out
  int n, me, cap;
  long long timeout_ticks;
};
NKA_HOST_DEVICE constexpr size_t p2p_mailbox_bytes(int n, int cap) { return (size_t)2 * n * cap * 16; }

}  // namespace nka
