"""One update of the lone array handle (nka_amd.nka(), product or diagnostic build) in a fast sum mode, split as
tests/test_batch_sums_exact_gpu.py splits an update of the batch kernel, with parts 2 and 3 held exactly here.  Part 1, the
sums against the correctly rounded sums, stays in tests/test_sums_exact_gpu.py.

SplitRun keeps a host mirror of the stored w AND v by slot and one OracleNKA that is driven ONLY through scalar_step, relax,
restart and set_vec_tol: whatever the device decides from its own sums is the expected answer, close calls included.  After
every update(x) it reads state(), reductions(), the output and only the slots this update wrote, and asserts:

  2 THE SCALAR STEP   s = sqrt(red[0]) (IEEE sqrt; NaN, Inf and 0 included; 0 without a pending pair).  The Gram row and the
               right-hand side by slot, from red[] exactly as the device's solve_nrm forms them for the handle's mode:
               SUMS_BLOCKED_ROUNDED the entries as they are; SUMS_BLOCKED red / s in the flavours 0 and 2, fl(1/s) * red in
               flavour 1; the Gram row and the pending pair's entry all zero when s == 0 or nothing is pending.  These go to
               the oracle's scalar_step; then, with == (NaN as NaN): first, last, free, subspace, pending, next; prev, c and
               h on the live entries; the free-list order; the new slot scalar_step returns.
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
last of them, and only it, dropped); outcomes [(call, positions of the older entries the update dropped)].

In place, f lies in a buffer with a guard element behind it (and one in front of it if f is not 16-byte aligned): the guards
must stay 0, so a store of the vector or the scalar path just outside f fails the update.

tests/test_split_update_cpu.py runs the checker on the CPU over a stand-in accelerator written in numpy and shows that each
fault planted in it makes the assertion meant for it fail."""
import numpy as np

SUMS_AUTO, SUMS_BLOCKED, SUMS_BLOCKED_ROUNDED = 0, 2, 3          # nka_amd.SUMS_* (include/nka_hip.h)


def _bits_equal(a, b):
    """Bit for bit, but NaN payloads (which the host and the device need not agree on) only as NaN."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


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


def gram_and_rhs(mode, flavor, mvec, red, s, normed, olders, first0):
    """(Gram row, right-hand side) by slot with a leading unused entry, from red[] as solve_nrm takes it in `mode`."""
    hrow, rhs = np.zeros(mvec + 2), np.zeros(mvec + 2)
    k = len(olders)
    with np.errstate(all="ignore"):
        if normed:
            row = np.concatenate((red[1:2], red[2:2 + k]))
            if mode != SUMS_BLOCKED_ROUNDED:                         # raw sums <f,d>, <d,w_p>: one operation by s each
                row = normalise(flavor, s, row)
            rhs[first0] = row[0]
            hrow[olders] = row[1:]
        rhs[olders] = red[2 + mvec:2 + mvec + k]
    return hrow, rhs


class SplitRun:
    """`acc`: an initialised handle of nka_amd.nka() (torch: the torch module) or a StandIn (torch None)."""

    def __init__(self, torch, oracle, acc, flavor, n, mvec, mode, aligned=True, swap=False):
        self.torch, self.acc, self.flavor, self.n, self.m, self.swap = torch, acc, flavor, n, mvec, swap
        assert acc.flavor() == flavor and mode in (SUMS_AUTO, SUMS_BLOCKED, SUMS_BLOCKED_ROUNDED)
        assert mode != SUMS_AUTO or n > 64, "SUMS_AUTO sums in the reference's order up to 64 elements"
        acc.set_sum_order(mode)
        self.mode = SUMS_BLOCKED_ROUNDED if mode == SUMS_AUTO else mode
        self.ora = oracle.OracleNKA(n, mvec, flavor)
        self.W, self.V = {}, {}                              # slot -> stored w / v (host mirror)
        self.calls, self._after = 0, None
        if torch is not None:
            self.lead = 0 if aligned else 1                              # 8-byte but not 16-byte aligned
            self.buf = torch.zeros(self.lead + n + 1, dtype=torch.float64, device="cuda")     # (a guard behind f, and in front)
            self.view = self.buf[self.lead:self.lead + n]
            assert n == 0 or self.view.data_ptr() % 16 == (0 if aligned else 8)
            self.lent = torch.zeros(n, dtype=torch.float64, device="cuda")      # the caller's buffer of an out-of-place call
        else:
            assert aligned
        # what the run met (asserted by the tests)
        self.ncomb, self.nolder_pending, self.nolder_no_pending, self.dropped_at_once = set(), set(), set(), set()
        self.dropped_newest = self.dropped_mid = self.zero_s = self.after_relax = self.after_restart = False
        self.full_at_entry = self.capacity_drop = False
        self.outcomes = []

    # -- the calls ------------------------------------------------------------------------------------------------------
    def _run(self, x, swap, where):
        """-> (f_out, what the caller's buffer holds after an out-of-place call or None)."""
        if self.torch is None:
            f = x.copy()
            if not swap:
                self.acc.accel_update(f)
                return f, None
            _, out = self.acc.accel_update_swap(f)
            return out.copy(), f
        src = self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        if not swap:
            self.view.copy_(src)
            self.acc.accel_update(self.view)
            whole = self.buf.cpu().numpy()
            guards = np.concatenate((whole[:self.lead], whole[self.lead + self.n:]))
            assert not guards.any() and not np.signbit(guards).any(), (where, "a store outside f", guards)
            return whole[self.lead:self.lead + self.n].copy(), None
        mine = self.lent
        mine.copy_(src)
        nxt, out = self.acc.accel_update_swap(mine)
        assert len({nxt.data_ptr(), out.data_ptr(), mine.data_ptr()}) == 3 or self.n == 0, (where, "the buffers coincide")
        self.lent = nxt
        return out.cpu().numpy(), mine.cpu().numpy()

    def update(self, x, swap=None):
        """One update on x (in place, or out of place with swap) and every check of the module docstring -> f_out."""
        acc, m, fl = self.acc, self.m, self.flavor
        swap = self.swap if swap is None else swap
        x = np.asarray(x, dtype=np.float64)
        where = (fl, self.n, m, self.mode, "swap" if swap else "in place", "call", self.calls)
        W, V = self.W, self.V
        st0 = acc.state()
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        assert sorted(W) == sorted(order0) == sorted(V), (where, "the mirror lost track of the list")
        out, kept = self._run(x, swap, where)
        red, st = acc.reductions(), acc.state()

        # 2: the scalar step on the device's own sums
        with np.errstate(all="ignore"):
            s = np.sqrt(np.float64(red[0])) if pending else np.float64(0.0)
        normed = pending and not s == 0.0                                 # (NaN goes on, like the reference)
        hrow, rhs = gram_and_rhs(self.mode, fl, m, red, s, normed, olders, first0)
        new = self.ora.scalar_step(float(s), hrow, rhs)
        sn = self.ora.state()
        self._same_lists(st, sn, where)
        assert st.first == new, (where, "the new slot", st.first, new)
        order = st.list_order()
        new, comb = order[0], order[1:]
        live = [i - 1 for i in comb]
        assert np.array_equal(st.c[live], sn.c[live], equal_nan=True), (where, "c", st.c[live], sn.c[live])
        assert np.array_equal(st.h[np.ix_(live, live)], sn.h[np.ix_(live, live)], equal_nan=True), (where, "h")
        self._record(pending, normed, olders, comb, where)

        # 3: the elementwise statements with the device's s and c; the mirror takes the slots this update wrote
        Wn, Vn = {slot: W[slot] for slot in comb}, {slot: V[slot] for slot in comb}
        if normed:
            assert comb and comb[0] == first0, (where, "the normalised pair does not lead the list")
            with np.errstate(all="ignore"):
                d = W[first0] - x                                         # F08:266
                w1n, v1n = normalise(fl, s, d), normalise(fl, s, V[first0])
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
        where = (self.flavor, self.n, self.m, self.mode, op, "before call", self.calls)
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
        where = (self.flavor, self.n, self.m, self.mode, "after call", self.calls)
        order = self.acc.state().list_order()
        assert sorted(order) == sorted(self.W) == sorted(self.V), (where, "the mirror lost track of the list")
        for slot in order:
            assert _bits_equal(self.acc.w(slot), self.W[slot]), (where, "w of a slot no update wrote has changed", slot)
            assert _bits_equal(self.acc.v(slot), self.V[slot]), (where, "v of a slot no update wrote has changed", slot)
        return self

    # -- the checks -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _same_lists(sd, sn, where):
        assert (sd.first, sd.last, sd.free, sd.subspace, sd.pending) == (sn.first, sn.last, sn.free, sn.subspace, sn.pending), \
            (where, "first, last, free, subspace, pending")
        assert np.array_equal(sd.next, sn.next), (where, "next", sd.next, sn.next)
        assert all(sd.prev[i - 1] == sn.prev[i - 1] for i in sn.list_order()), (where, "prev")
        assert sd.free_order() == sn.free_order(), (where, "the free list")

    def _record(self, pending, normed, olders, comb, where):
        gone = [p for p, slot in enumerate(olders) if slot not in comb]
        self.outcomes.append((self.calls, gone))
        (self.nolder_pending if pending else self.nolder_no_pending).add(len(olders))
        self.ncomb.add((len(comb), normed))
        self.zero_s |= pending and not normed
        self.after_relax |= self._after == "relax"
        self.after_restart |= self._after == "restart"
        self._after = None
        if len(olders) == self.m:
            self.full_at_entry = True
            self.capacity_drop |= normed and gone == [self.m - 1]
        if gone:
            assert normed, (where, "an update without a normalised pair dropped an older entry")
            self.dropped_at_once.add(min(len(gone), 3))
            self.dropped_newest |= 0 in gone
            self.dropped_mid |= any(set(range(p + 1, len(olders))) - set(gone) for p in gone if p > 0)
