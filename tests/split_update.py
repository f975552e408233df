"""One update of the lone array handle (nka_amd.nka(), product or diagnostic build), split as
tests/test_batch_sums_exact_gpu.py splits an update of the batch kernel, with all three parts held exactly here -- and with the
way the update is made chosen PER UPDATE, so that one checker follows a handle through every change the headers allow between
updates (include/nka_hip.h: the sum order "can be changed between updates", new weights apply "from the next update on",
fn = NULL "restores the device sums", the hook can be installed and removed; include/nka_hip_ext.h: the two entries "can be
mixed", an f that is not 16-byte aligned gives "the same bits").

A Config names one update:
  sums   R  NKA_HIP_SUMS_BLOCKED_ROUNDED        B  NKA_HIP_SUMS_BLOCKED        O  NKA_HIP_SUMS_REFERENCE_ORDER
         H  the user's dot product on host copies (nka_hip_set_host_dot)       Rw, Bw  R and B with diagonal weights, two
         weight vectors in turn (every weighted update sets the other one, by the device and by the host entry in turn)
         A, Aw  NKA_HIP_SUMS_AUTO, plain and weighted: the reference-order kernel up to 64 elements on a handle without hook
         and weights, the rounded passes otherwise
  entry  a  in place, 16-byte aligned     u  in place, 8 bytes off     s  accel_update_swap     h  a numpy array
  hook   an identity all-reduce hook that records `count`; with O it needs set_shard(0, 1) (one "rank": the chain over the ranks
         is the single-rank order)
legal(): no s with H, no weights with O or H, no hook on top of H.

SplitRun keeps a host mirror of the stored w AND v by slot and one OracleNKA that is driven ONLY through scalar_step, relax,
restart and set_vec_tol: whatever the device decides from its own sums is the expected answer, close calls included.  It moves
the handle from one configuration to the next with the public calls only; where the header refuses an order of calls it tries
the refused order first and asserts the error code (weights while O is selected, O while weighted: -1; H while weighted,
weights under H, s under H: -5; s with an unaligned buffer: -1; O under a hook without set_shard: -5) -- the update that
follows shows that the handle was left as it was.  After every update(x, cfg) it reads state(), reductions(), the output and
only the slots this update wrote, and asserts:

  1 THE SUMS   d = fl(w1 - f), s = sqrt(red[0]), w1' = fl(d/s) (fl(fl(1/s)*d) in flavour 1), operands from the mirror.
               R, B, Rw, Bw: every live red[] entry within exact_sums.gamma(K) * abs_dot of exact_sums.exact_dot, K =
               exact_sums.device_k(n, ncu, aligned) (aligned for s and h: the library's own buffers).  The operands are the
               table's of include/nka_hip.h: R red[1] = <f,w1'>, red[2+p] = <w1',w_p>; B red[1] = <f,d>, red[2+p] = <d,w_p>;
               red[0] = <d,d>, red[2+m+p] = <f,w_p> in both; weighted, the first operand is fl(w*a); with s == 0 R's red[1]
               and Gram row are exactly 0.
               O: every live entry equals, bit for bit, numpy's sequential add.accumulate of the rounded products from 0.0:
               the norm on d, red[1] and red[2+p] on w1', red[2+m+p] on f; dead Gram entries (s == 0) are 0.
               H: the recorded dp calls are, operands compared by their bits, (d,d); if s != 0 (w1', w_k) in list order;
               then, after the drops, (f, w_j) from first to last (w1' for the normalised pair): the docstring of
               nka_hip_set_host_dot.  red[0] and the Gram row carry what dp returned.
               Entries past the list are exactly 0 (R, B, O).  On an update that skipped the last vector (skip_last, the
               diagnostic build) its two entries read 0 and are left out.
    THE HOOK   the recorded counts: R [1, 2 mvec + 1] with a pending pair, [2 mvec + 1] without; B [2 + 2 mvec]; O what
               ordered_chain (nka_hip.hip) exchanges on one rank, N = 1: one norm round on red[0] alone if a pair is
               pending, then one rows round on everything behind it -- [1, 2 mvec + 1], R's counts; none on an update that
               forms no sum, none under H.
  2 THE SCALAR STEP   s = sqrt(red[0]) (IEEE sqrt; NaN, Inf and 0 included; 0 without a pending pair).  The Gram row and the
               right-hand side by slot, from red[] exactly as the device's solve_nrm forms them for the update's way:
               R, O and H the entries as they are (H: the right-hand side is what dp returned); B red / s in the flavours 0
               and 2, fl(1/s) * red in flavour 1; the Gram row and the pending pair's entry all zero when s == 0 or nothing
               is pending.  These go to the oracle's scalar_step; then, with == (NaN as NaN): first, last, free, subspace,
               pending, next; prev, c and h on the live entries; the free-list order; the new slot scalar_step returns.
  3 THE ELEMENTWISE STATEMENTS   with numpy (IEEE, no fma), the device's s, the device's c and operands from the mirror, bit
               for bit (NaN payloads as NaN only):
               - the normalised pair as stored: d = w1 - f; w1' = d/s (fl(1/s)*d in flavour 1); v1' = v1/s (fl(1/s)*v1);
                 flavour 2 keeps fl(v1' - w1') in the v array; with s == 0 the pending pair is gone from the list;
               - the combine in list order with the flavour's association: 0 (f - c*w) + c*v; 1 ((-c)*w + c*v) + f;
                 2 f + c*u; the output carries those bits, f_in itself if nothing was combined;
               - the ring stores: w_new == f_in and v_new == f_out;
               - out of place (accel_update_swap): the caller's buffer keeps f_in, v_new holds f_out and the buffer of the
                 accelerated f that is handed back carries the bits f would carry;
               - finish(), once at the end of a sequence: every slot of the list still carries the mirror's bits (a store
                 to the wrong slot of an entry that was live before and after and was not written).

What a run met is recorded for the tests to assert: ncomb {(len(comb), normed)}; nolder_pending / nolder_no_pending (older
counts with / without a pending pair at entry); dropped_at_once {1, 2, 3 = three or more}; dropped_newest / dropped_mid (the
newest older entry / an entry with live older ones behind it went); zero_s; after_relax / after_restart (an update right
after a relax that took a pending pair / after a restart); full_at_entry and capacity_drop (mvec older entries at entry; the
last of them, and only it, dropped); outcomes [(call, positions of the older entries the update dropped)]; widest (the
longest older list at entry); pairs {(previous Config, this Config)}; ways {way: {"capacity_drop", "dependence_drop",
"zero_s", "after_relax", "after_restart"} met under it} (way: R, B, O, H, Rw, Bw as the update really ran); hooked (updates
whose sums went through the hook); skipped / redone (updates that skipped the last vector / repaired a skip); fast_not_ordered
{"A" | "A+hook" | "Aw": some fast red[0] under that configuration of SUMS_AUTO was NOT the bits of the sequential sum of the same
rounded products, fl(w d) d when weighted}: what tells the rounded passes from the reference-order kernel, whose sums of 65
products lie well inside the fast bound (assert_auto_boundary).
WORST[way] = [worst |red - exact| / (u sum|xy|), the K it was held to, where], over every run of the process.

In place, f lies in a buffer with a guard element behind it (and one in front of it if f is not 16-byte aligned): the guards
must stay 0, so a store of the vector or the scalar path just outside f fails the update.

tests/test_split_update_cpu.py runs the checker on the CPU over a stand-in accelerator written in numpy and shows that each
fault planted in it makes the assertion meant for it fail."""
import math
from collections import namedtuple

import numpy as np

import exact_sums as X

SUMS_AUTO, SUMS_REFERENCE_ORDER, SUMS_BLOCKED, SUMS_BLOCKED_ROUNDED = 0, 1, 2, 3      # nka_amd.SUMS_* (include/nka_hip.h)
EINVAL, ESTATE = -1, -5                                                                 # NKA_HIP_EINVAL, NKA_HIP_ESTATE
ORD_AUTO_MAX = 64                                   # kOrdAutoMax: SUMS_AUTO sums in the reference's order up to here

Config = namedtuple("Config", "sums entry hook", defaults=(False,))
SUMS = ("R", "B", "O", "H", "Rw", "Bw")
ENTRIES = ("a", "u", "s", "h")
ORDER_OF = {"R": SUMS_BLOCKED_ROUNDED, "Rw": SUMS_BLOCKED_ROUNDED, "B": SUMS_BLOCKED, "Bw": SUMS_BLOCKED,
            "O": SUMS_REFERENCE_ORDER, "A": SUMS_AUTO, "Aw": SUMS_AUTO}
WORST = {}                                          # way -> [ratio, K, where]


def legal(cfg):
    """The combinations the headers allow."""
    if cfg.sums == "H":
        return cfg.entry != "s" and not cfg.hook
    return True


def configs(sums=SUMS, entries=ENTRIES):
    """The legal (sums, entry) pairs, the transport kept apart: 23 of the full axes."""
    return [Config(s, e) for s in sums for e in entries if legal(Config(s, e))]


def circuit(k):
    """A closed walk over the complete directed graph on k nodes, self-loops included, that takes every one of the k * k arcs
    once (Hierholzer): k * k + 1 nodes, so every ordered pair of nodes occurs as two consecutive entries."""
    nxt = [0] * k                                    # the next arc to leave node i by
    stack, walk = [0], []
    while stack:
        i = stack[-1]
        if nxt[i] < k:
            stack.append((i + 1 + nxt[i]) % k)       # (the self-loop last)
            nxt[i] += 1
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == k * k + 1 and len(set(zip(walk, walk[1:]))) == k * k
    return walk


def _bits_equal(a, b):
    """Bit for bit, but NaN payloads (which the host and the device need not agree on) only as NaN."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def _same_bits(a, b):
    """Two doubles, bit for bit (NaN as NaN)."""
    return _bits_equal(np.array([a], dtype=np.float64), np.array([b], dtype=np.float64))


def combine(flavor, f, c, w, v):
    """One pair of the combine, the flavour's association (v: what the v array stores, the difference v' - w' in flavour 2)."""
    if flavor == 0:
        return (f - c * w) + c * v                                  # F08:397
    if flavor == 1:
        return ((-c) * w + c * v) + f                               # F08V: update3_(-c, w, c, v)
    return f + c * v


def normalise(flavor, s, x):
    """x / s, or fl(1/s) * x in the F08-vector flavour (F08:282-283, F08V:255-256)."""
    return (np.float64(1.0) / s) * x if flavor == 1 else x / s


def ordered_dot(x, y):
    """0.0 + x[0]*y[0] + x[1]*y[1] + ... in that order, one rounding per product and per addition: the reference's sum."""
    with np.errstate(all="ignore"):
        return float(np.add.accumulate(np.concatenate((np.zeros(1), x * y)))[-1])


def host_dot(x, y):
    """The user's dot product of the H updates: any function of the operands will do; this one does not depend on where
    the operands lie in memory."""
    return math.fsum((x * y).tolist())


def gram_and_rhs(mode, flavor, mvec, red, s, normed, olders, first0, rhs_by_slot=None):
    """(Gram row, right-hand side) by slot with a leading unused entry, from red[] as solve_nrm takes it in `mode` (a
    SUMS_* number: every way but SUMS_BLOCKED takes the entries as they are).  rhs_by_slot: the right-hand side where it
    does not pass through red[] (the user's dot product)."""
    hrow, rhs = np.zeros(mvec + 2), np.zeros(mvec + 2)
    k = len(olders)
    with np.errstate(all="ignore"):
        if normed:
            row = np.concatenate((red[1:2], red[2:2 + k]))
            if mode == SUMS_BLOCKED:                                 # raw sums <f,d>, <d,w_p>: one operation by s each
                row = normalise(flavor, s, row)
            rhs[first0] = row[0]
            hrow[olders] = row[1:]
        rhs[olders] = red[2 + mvec:2 + mvec + k]
    if rhs_by_slot is not None:
        rhs[:] = 0.0
        for slot, val in rhs_by_slot.items():
            rhs[slot] = val
    return hrow, rhs


def array_at(x, off8):
    """A copy of x in host memory that starts on a 16-byte boundary (off8 = 0) or 8 bytes behind one (off8 = 1)."""
    raw = np.zeros(x.size + 2)
    lead = 0 if raw.ctypes.data % 16 == 8 * off8 else 1
    out = raw[lead:lead + x.size]
    out[:] = x
    assert x.size == 0 or out.ctypes.data % 16 == 8 * off8
    return out


class _Dots:
    """The recording user dot product: calls [(x, y, value)]; `pure` is the same function without the record."""

    pure = staticmethod(host_dot)

    def __init__(self):
        self.calls = []

    def __call__(self, x, y):
        val = host_dot(x, y)
        self.calls.append((np.array(x, dtype=np.float64), np.array(y, dtype=np.float64), val))
        return val


class SplitRun:
    """`acc`: an initialised handle of nka_amd.nka() (torch: the torch module) or a StandIn (torch None).  `mode`, `aligned`
    and `swap` choose the configuration of the updates that name none (a handle in one fast mode for life, as the earlier
    tests drive it); update(x, cfg) runs one update in cfg.  check_sums=False leaves part 1 out (long vectors with long
    lists: the exact sums cost more host time than everything else).  skip_last: the handle (diagnostic build) skips the
    last vector wherever the launch allows."""

    def __init__(self, torch, oracle, acc, flavor, n, mvec, mode=SUMS_BLOCKED_ROUNDED, aligned=True, swap=False, check_sums=True,
                 skip_last=False, seed=0):
        self.torch, self.acc, self.flavor, self.n, self.m, self.swap = torch, acc, flavor, n, mvec, swap
        assert acc.flavor() == flavor and mode in (SUMS_AUTO, SUMS_BLOCKED, SUMS_BLOCKED_ROUNDED)
        assert mode != SUMS_AUTO or n > ORD_AUTO_MAX, "SUMS_AUTO sums in the reference's order up to 64 elements"
        self.default = Config("B" if mode == SUMS_BLOCKED else "R", "a" if aligned else "u")
        self.mode = SUMS_BLOCKED_ROUNDED if mode == SUMS_AUTO else mode
        acc.set_sum_order(mode)
        self.check_sums, self.skip_last = check_sums, skip_last
        self.ncu = acc.device_info()[1] if check_sums else 0
        self.ora = oracle.OracleNKA(n, mvec, flavor)
        self.W, self.V = {}, {}                              # slot -> stored w / v (host mirror)
        self.calls, self._after = 0, None
        # the handle as the public calls have left it
        self.order, self.weighted, self.hosted, self.hook, self.sharded = mode, False, False, False, False
        self.dots, self.counts = _Dots(), []
        rng = np.random.default_rng(seed + 7919 * n + mvec)
        self.weights = [rng.uniform(0.875, 1.125, n), rng.uniform(0.75, 1.25, n)]      # > 0 (s == 0 only where d == 0) and near
        #                                    1: the subspace mixes the metrics of its updates, and a long list must still fill
        self.nweighted, self.wvec = 0, None                  # weighted updates so far; the weights in force
        if torch is not None:
            self.bufs = {"a": torch.zeros(n + 1, dtype=torch.float64, device="cuda"),            # (a guard behind f,
                         "u": torch.zeros(n + 2, dtype=torch.float64, device="cuda")}            #  and one in front)
            assert n == 0 or (self.bufs["a"].data_ptr() % 16 == 0 and self.bufs["u"][1:].data_ptr() % 16 == 8)
            self.lent = torch.zeros(n, dtype=torch.float64, device="cuda")      # the caller's buffer of an out-of-place call
        # what the run met (asserted by the tests)
        self.ncomb, self.nolder_pending, self.nolder_no_pending, self.dropped_at_once = set(), set(), set(), set()
        self.dropped_newest = self.dropped_mid = self.zero_s = self.after_relax = self.after_restart = False
        self.full_at_entry = self.capacity_drop = False
        self.fast_not_ordered = {}
        self.outcomes, self.widest, self.pairs, self.ways, self._prev_cfg = [], 0, set(), {}, None
        self.hooked = self.skipped = self.redone = 0

    # -- from one configuration to the next: the public calls, the refused orders first -------------------------------------
    def _refused(self, code, call, *args):
        try:
            call(*args)
        except Exception as exc:                             # (nka_amd.NKAError; the stand-in's own)
            refused = f"({code})" in str(exc)
            text = str(exc)
        else:
            refused, text = False, "the call went through"
        assert refused, ("a refused order of calls", getattr(call, "__name__", call), code, text)

    def _move_to(self, cfg):
        acc = self.acc
        assert legal(cfg), cfg
        want_w = cfg.sums.endswith("w")
        # the hook first: it is independent of everything else (H ignores it; it comes off there, H applies none on top)
        if cfg.hook != self.hook:
            acc.set_dot_prod((lambda ptr, count, stream: self.counts.append(count)) if cfg.hook else None)
            self.hook = cfg.hook
        if cfg.sums == "H":
            if not self.hosted:
                if self.weighted:
                    self._refused(ESTATE, acc.set_host_dot, self.dots)               # H while weighted
                    acc.set_dot_weights(None)
                    self.weighted = False
                acc.set_host_dot(self.dots)
                self.hosted = True
            return
        order = ORDER_OF[cfg.sums]
        if self.hosted:
            if want_w:
                self._refused(ESTATE, acc.set_dot_weights, self.weights[0])         # weights under H
            acc.set_host_dot(None)
            self.hosted = False
        if order == SUMS_REFERENCE_ORDER and self.weighted:
            self._refused(EINVAL, acc.set_sum_order, order)                          # O while weighted
        if self.weighted and not want_w:
            acc.set_dot_weights(None)
            self.weighted = False
        if want_w and self.order == SUMS_REFERENCE_ORDER:
            self._refused(EINVAL, acc.set_dot_weights, self.weights[0])             # weights while O is selected
        if order != self.order:
            acc.set_sum_order(order)
            self.order = order
        if want_w:                                           # the other weight vector, by the two entries in turn
            w = self.weights[self.nweighted % 2]
            if self.torch is not None and self.nweighted % 4 < 2:
                acc.set_dot_weights(self.torch.from_numpy(w).cuda())
            else:
                acc.set_dot_weights(w.copy())
            self.nweighted += 1
            self.weighted, self.wvec = True, w

    def _way(self, cfg):
        """How the update really runs: AUTO resolved."""
        if cfg.sums == "A":
            return "O" if self.n <= ORD_AUTO_MAX and not cfg.hook else "R"
        return "Rw" if cfg.sums == "Aw" else cfg.sums

    # -- the calls ------------------------------------------------------------------------------------------------------
    def _run(self, x, cfg, where):
        """-> (f_out, what the caller's buffer holds after an out-of-place call or None)."""
        acc, entry = self.acc, cfg.entry
        if self.torch is None:
            f = array_at(x, 1 if entry == "u" else 0)
            if entry == "u" and cfg.sums != "H":
                self._refused(EINVAL, acc.accel_update_swap, f)                      # s with an unaligned buffer
            if cfg.sums == "H":
                self._refused(ESTATE, acc.accel_update_swap, array_at(x, 0))         # s under H
            if cfg.sums == "O" and cfg.hook and not self.sharded:
                self._refused(ESTATE, acc.accel_update, f)                           # the chain needs the slice's position
                acc.set_shard(0, 1)
                self.sharded = True
            if entry != "s":
                acc.accel_update(f)
                return f.copy(), None
            _, out = acc.accel_update_swap(f)
            return out.copy(), f
        src = self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        if entry == "u" and cfg.sums != "H":
            self._refused(EINVAL, acc.accel_update_swap, self.bufs["u"][1:1 + self.n])
        if cfg.sums == "H":
            self._refused(ESTATE, acc.accel_update_swap, self.lent)
        if cfg.sums == "O" and cfg.hook and not self.sharded:
            self._refused(ESTATE, acc.accel_update, self.bufs["a"][:self.n])
            acc.set_shard(0, 1)
            self.sharded = True
        if entry == "h":
            f = x.copy()
            acc.accel_update(f)
            return f, None
        if entry != "s":
            lead = 1 if entry == "u" else 0
            buf = self.bufs[entry]
            view = buf[lead:lead + self.n]
            view.copy_(src)
            acc.accel_update(view)
            whole = buf.cpu().numpy()
            guards = np.concatenate((whole[:lead], whole[lead + self.n:]))
            assert not guards.any() and not np.signbit(guards).any(), (where, "a store outside f", guards)
            return whole[lead:lead + self.n].copy(), None
        mine = self.lent
        mine.copy_(src)
        nxt, out = acc.accel_update_swap(mine)
        assert len({nxt.data_ptr(), out.data_ptr(), mine.data_ptr()}) == 3 or self.n == 0, (where, "the buffers coincide")
        self.lent = nxt
        return out.cpu().numpy(), mine.cpu().numpy()

    def update(self, x, cfg=None, swap=None):
        """One update on x in the configuration cfg (without one: the run's default, out of place with swap) and every check
        of the module docstring -> f_out."""
        acc, m, fl = self.acc, self.m, self.flavor
        if cfg is None:
            cfg = self.default._replace(entry="s") if (self.swap if swap is None else swap) else self.default
            way = cfg.sums
        else:
            self._move_to(cfg)
            way = self._way(cfg)
        x = np.asarray(x, dtype=np.float64)
        where = (fl, self.n, m, cfg.sums + cfg.entry + ("+hook" if cfg.hook else ""), "call", self.calls)
        W, V = self.W, self.V
        st0 = acc.state()
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        assert sorted(W) == sorted(order0) == sorted(V), (where, "the mirror lost track of the list")
        skip0 = acc.skip_state() if self.skip_last else None
        del self.dots.calls[:], self.counts[:]
        out, kept = self._run(x, cfg, where)
        red, st = acc.reductions(), acc.state()
        order = st.list_order()
        new, comb = order[0], order[1:]

        # 1: the sums, as the update's way forms them
        with np.errstate(all="ignore"):
            s = np.sqrt(np.float64(red[0])) if pending else np.float64(0.0)
            normed = pending and not s == 0.0                             # (NaN goes on, like the reference)
            d = W[first0] - x if pending else None                        # F08:266
            w1n = normalise(fl, s, d) if normed else None
        dead = self._skipped(skip0, order0, comb, cfg, way, where)
        rhs_by_slot = None
        if way == "H":
            rhs_by_slot = self._check_dots(x, d, w1n, red, pending, normed, olders, first0, comb, where)
        elif self.check_sums and way == "O":
            self._check_ordered(x, d, w1n, red, pending, normed, olders, where)
        elif self.check_sums:
            self._check_fast(way, cfg, x, d, w1n, s, red, pending, normed, olders, dead, where)
        self._check_hook(way, cfg, pending, olders, where)

        # 2: the scalar step on the device's own sums
        mode = SUMS_BLOCKED if way in ("B", "Bw") else SUMS_BLOCKED_ROUNDED
        hrow, rhs = gram_and_rhs(mode, fl, m, red, s, normed, olders, first0, rhs_by_slot)
        got = self.ora.scalar_step(float(s), hrow, rhs)
        sn = self.ora.state()
        self._same_lists(st, sn, where)
        assert st.first == got, (where, "the scalar step", "the new slot", st.first, got)
        live = [i - 1 for i in comb]
        assert np.array_equal(st.c[live], sn.c[live], equal_nan=True), (where, "the scalar step", "c", st.c[live], sn.c[live])
        assert np.array_equal(st.h[np.ix_(live, live)], sn.h[np.ix_(live, live)], equal_nan=True), (where, "the scalar step", "h")
        self._record(cfg, way, pending, normed, olders, comb, where)

        # 3: the elementwise statements with the device's s and c; the mirror takes the slots this update wrote
        Wn, Vn = {slot: W[slot] for slot in comb}, {slot: V[slot] for slot in comb}
        if normed:
            assert comb and comb[0] == first0, (where, "the normalised pair does not lead the list")
            with np.errstate(all="ignore"):
                v1n = normalise(fl, s, V[first0])
                v1s = v1n - w1n if fl == 2 else v1n                       # compact storage keeps v' - w'
            w1, v1 = acc.w(first0), acc.v(first0)
            assert _bits_equal(w1, w1n), (where, "stored w1' is not fl(d/s)", int(np.sum(w1 != w1n)))
            assert _bits_equal(v1, v1s), (where, "stored v1' is not fl(v1/s)", int(np.sum(v1 != v1s)))
            Wn[first0], Vn[first0] = w1, v1
        elif pending:
            assert first0 not in comb, (where, "s == 0 did not drop the pending pair")
        f = x.copy()
        with np.errstate(all="ignore"):
            for slot in comb:
                f = combine(fl, f, st.c[slot - 1], Wn[slot], Vn[slot])
        assert _bits_equal(out, f), (where, "f_out", len(comb), int(np.sum(out != f)))      # (nothing combined: f_in itself)
        if kept is not None:
            assert _bits_equal(kept, x), (where, "the caller's buffer of an out-of-place update lost f_in")
        w_new, v_new = acc.w(new), acc.v(new)
        assert _bits_equal(w_new, x), (where, "the new pair's w is not the input")       # F08:361
        assert _bits_equal(v_new, f), (where, "the new pair's v is not f_out")           # F08:404
        Wn[new], Vn[new] = w_new, v_new
        self.W, self.V = Wn, Vn
        self.calls += 1
        return out

    def _list_op(self, op):
        so = self.ora.state()
        where = (self.flavor, self.n, self.m, op, "before call", self.calls)
        if op == "restart":
            self.W, self.V = {}, {}
            self._after = "restart"
        elif so.pending:                                     # relax drops the pending pair (F08:441-457)
            self.W.pop(so.first)
            self.V.pop(so.first)
            self._after = "relax"
        getattr(self.acc, op)()
        getattr(self.ora, op)()
        self._same_lists(self.acc.state(), self.ora.state(), where)

    def relax(self):
        self._list_op("relax")

    def restart(self):
        self._list_op("restart")

    def set_vec_tol(self, vtol):
        self.acc.set_vec_tol(vtol)
        self.ora.set_vec_tol(vtol)

    def finish(self):
        """Once, at the end of a sequence: every slot of the list still carries the mirror's bits."""
        where = (self.flavor, self.n, self.m, "after call", self.calls)
        order = self.acc.state().list_order()
        assert sorted(order) == sorted(self.W) == sorted(self.V), (where, "the mirror lost track of the list")
        for slot in order:
            assert _bits_equal(self.acc.w(slot), self.W[slot]), (where, "w of a slot no update wrote has changed", slot)
            assert _bits_equal(self.acc.v(slot), self.V[slot]), (where, "v of a slot no update wrote has changed", slot)
        return self

    # -- the checks -----------------------------------------------------------------------------------------------------
    def _hold(self, way, what, red, x, y, k, where):
        """One fast sum against the correctly rounded one, within gamma(k) * sum|x y|."""
        ex = X.exact_dot(x, y)
        if math.isnan(ex):
            assert math.isnan(red), (where, "a fast sum is not NaN where the exact sum is", what, red)
            return
        if math.isinf(ex):
            assert red == ex, (where, "a fast sum is not the infinity of the exact sum", what, red, ex)
            return
        tot = X.abs_dot(x, y)
        err = abs(red - ex)
        assert err <= X.gamma(k) * tot, (where, "a fast sum beyond gamma(K) of the exact sum", what, red, ex, err / (X.U * tot) if tot else err, k)
        if tot > 0:
            r = WORST.setdefault(way, [0.0, 0, ""])
            ratio = err / (X.U * tot)
            if ratio >= r[0]:
                r[:] = [ratio, k, f"{what} {where}"]

    def _check_fast(self, way, cfg, x, d, w1n, s, red, pending, normed, olders, dead, where):
        m, W = self.m, self.W
        k = X.device_k(self.n, self.ncu, cfg.entry != "u")
        rounded = way in ("R", "Rw")
        wgt = (lambda a: self.wvec * a) if way.endswith("w") else (lambda a: a)          # fl(w*a): the FIRST operand
        if pending:
            with np.errstate(all="ignore"):
                self._hold(way, "<d,d>", red[0], wgt(d), d, k, where)
                if cfg.sums in ("A", "Aw"):                 # the same operands summed in sequence: other bits, sooner or later
                    key = cfg.sums + ("+hook" if cfg.hook else "")
                    self.fast_not_ordered[key] = self.fast_not_ordered.get(key, False) or \
                        not _same_bits(red[0], ordered_dot(wgt(d), d))
                if rounded:
                    op = w1n if normed else np.zeros(self.n)        # (s == 0: the scalar step relaxes, these are 0)
                    if not normed and not np.isnan(s):
                        assert red[1] == 0.0 and all(red[2 + p] == 0.0 for p in range(len(olders))), \
                            (where, "s == 0 but the sums on w1' are not 0", red)
                else:
                    op = d
                self._hold(way, "<f,w1'>" if rounded else "<f,d>", red[1], wgt(x), op, k, where)
                for p, slot in enumerate(olders):
                    if 2 + p not in dead:
                        self._hold(way, f"<w1',w_{p}>" if rounded else f"<d,w_{p}>", red[2 + p], wgt(op), W[slot], k, where)
        if pending or olders:
            with np.errstate(all="ignore"):
                for p, slot in enumerate(olders):
                    if 2 + m + p not in dead:
                        self._hold(way, f"<f,w_{p}>", red[2 + m + p], wgt(x), W[slot], k, where)
            self._past_the_list(red, len(olders), where)
        for i in dead:
            assert red[i] == 0.0, (where, "an entry of the skipped vector is not 0", i, red[i])

    def _past_the_list(self, red, k, where):
        m = self.m
        for p in range(k, m):
            assert red[2 + p] == 0.0 and red[2 + m + p] == 0.0, (where, "past the list: not exactly 0", p, red[2 + p],
                                                                  red[2 + m + p])

    def _check_ordered(self, x, d, w1n, red, pending, normed, olders, where):
        m, W = self.m, self.W

        def same(what, got, a, b):
            want = ordered_dot(a, b)
            assert _same_bits(got, want), (where, "not the sequential sum's bits", what, got, want)

        if pending:
            same("<d,d>", red[0], d, d)
            if normed:
                same("<f,w1'>", red[1], x, w1n)
                for p, slot in enumerate(olders):
                    same(f"<w1',w_{p}>", red[2 + p], w1n, W[slot])
            else:
                assert red[1] == 0.0 and all(red[2 + p] == 0.0 for p in range(len(olders))), \
                    (where, "s == 0 but the sums on w1' are not 0", red)
        if pending or olders:
            for p, slot in enumerate(olders):
                same(f"<f,w_{p}>", red[2 + m + p], x, W[slot])
            self._past_the_list(red, len(olders), where)

    def _check_dots(self, x, d, w1n, red, pending, normed, olders, first0, comb, where):
        """The dp calls of the update against the reference's sequence -> the right-hand side by slot as dp returned it."""
        W = self.W
        want = []
        if pending:
            want.append(("(d,d)", d, d))
        if normed:
            want += [(f"(w1',w_{p})", w1n, W[slot]) for p, slot in enumerate(olders)]
        for slot in comb:                                    # after the drops, first ... last (F08:371)
            want.append((f"(f,w[{slot}])", x, w1n if normed and slot == first0 else W[slot]))
        calls = self.dots.calls
        assert len(calls) == len(want), (where, "dp operand", "the number of dp calls", len(calls), [w[0] for w in want])
        for (what, a, b), (ga, gb, _) in zip(want, calls):
            assert _bits_equal(ga, a) and _bits_equal(gb, b), (where, "dp operand", what, int(np.sum(ga != a)), int(np.sum(gb != b)))
        vals = [c[2] for c in calls]
        if pending:
            assert _same_bits(red[0], vals[0]), (where, "red[0] is not what dp returned", red[0], vals[0])
        if normed:
            for p in range(len(olders)):
                assert _same_bits(red[2 + p], vals[1 + p]), (where, "the Gram row is not what dp returned", p)
        return dict(zip(comb, vals[len(vals) - len(comb):]))

    def _check_hook(self, way, cfg, pending, olders, where):
        """The exchanges of the update, as the recorded counts."""
        m = self.m
        if not cfg.hook or way == "H":
            want = []
        elif not (pending or olders):
            want = []                                        # no sum is formed: nothing is exchanged
        elif way in ("B", "Bw"):
            want = [2 + 2 * m]                               # sums_blocked: ONE exchange
        else:
            # sums_rounded: the norm, then the rows.  ordered_chain on one rank (N = 1): a norm round that exchanges red[0]
            # alone if a pair is pending, then one rows round that exchanges everything behind it -- the same counts
            want = ([1] if pending else []) + [2 * m + 1]
        assert self.counts == want, (where, "the hook's counts", self.counts, want)
        self.hooked += bool(want)

    def _skipped(self, skip0, order0, comb, cfg, way, where):
        """The skip of the last vector (tests/test_skip_last_gpu.py recognises it the same way) -> the dead entries of red[]."""
        if skip0 is None:
            return ()
        m = self.m
        may, hold, pending_redo, nredo = skip0
        may2, hold2, pending2, nredo2 = self.acc.skip_state()
        assert pending_redo == 0 and pending2 == 0, (where, "a repair is left pending")
        full = len(order0) == m + 1                          # (mvec + 1 entries: the first of them is a pending pair)
        removed = [p for p, slot in enumerate(order0) if slot not in comb]
        possible = way in ("R", "B", "Rw", "Bw") and not cfg.hook and cfg.entry != "u" and 2 <= m <= 32
        needs = full and removed != [m] and may == 1 and possible
        if nredo2 != nredo:
            assert nredo2 == nredo + 1 and needs, (where, "a repair nothing asked for", nredo, nredo2, removed)
            self.redone += 1
            return ()
        assert not needs, (where, "the repair was not taken", removed)
        if full and may == 1 and possible:
            self.skipped += 1
            return (2 + m - 1, 2 + 2 * m - 1)
        return ()

    @staticmethod
    def _same_lists(sd, sn, where):
        assert (sd.first, sd.last, sd.free, sd.subspace, sd.pending) == (sn.first, sn.last, sn.free, sn.subspace, sn.pending), \
            (where, "the scalar step", "first, last, free, subspace, pending")
        assert np.array_equal(sd.next, sn.next), (where, "the scalar step", "next", sd.next, sn.next)
        assert all(sd.prev[i - 1] == sn.prev[i - 1] for i in sn.list_order()), (where, "the scalar step", "prev")
        assert sd.free_order() == sn.free_order(), (where, "the scalar step", "the free list")

    def _record(self, cfg, way, pending, normed, olders, comb, where):
        gone = [p for p, slot in enumerate(olders) if slot not in comb]
        self.outcomes.append((self.calls, gone))
        self.widest = max(self.widest, len(olders))
        (self.nolder_pending if pending else self.nolder_no_pending).add(len(olders))
        self.ncomb.add((len(comb), normed))
        met = self.ways.setdefault(way, set())
        self.pairs.add((self._prev_cfg, cfg))
        self._prev_cfg = cfg
        self.zero_s |= pending and not normed
        self.after_relax |= self._after == "relax"
        self.after_restart |= self._after == "restart"
        if pending and not normed:
            met.add("zero_s")
        if self._after:
            met.add("after_" + self._after)
        self._after = None
        if len(olders) == self.m:
            self.full_at_entry = True
            self.capacity_drop |= normed and gone == [self.m - 1]
            if normed and gone == [self.m - 1]:
                met.add("capacity_drop")
        if gone:
            assert normed, (where, "an update without a normalised pair dropped an older entry")
            self.dropped_at_once.add(min(len(gone), 3))
            self.dropped_newest |= 0 in gone
            self.dropped_mid |= any(set(range(p + 1, len(olders))) - set(gone) for p in gone if p > 0)
            if gone != [self.m - 1] or len(olders) < self.m:
                met.add("dependence_drop")


def assert_auto_boundary(run):
    """What a run over SUMS_AUTO must show of the kernel that ran: under the hook and with weights the rounded passes at every n,
    on the plain handle the rounded passes beyond ORD_AUTO_MAX elements (up to there _check_ordered has held every plain
    update to the sequential sum's bits, which the blocked fma sums do not keep up over a run)."""
    want = {"A+hook", "Aw"} | ({"A"} if run.n > ORD_AUTO_MAX else set())
    assert set(run.fast_not_ordered) == want, (run.n, "the configurations of SUMS_AUTO that took the fast check", run.fast_not_ordered)
    for key in sorted(want):
        assert run.fast_not_ordered[key], (run.n, key, "the rounded passes did not run: every red[0] is the sequential sum's bits")


EVERY_RECORD = {"capacity_drop", "dependence_drop", "zero_s", "after_relax", "after_restart"}
