"""The checker of tests/split_update.py on the CPU: a stand-in accelerator written in numpy (StandIn below: the accessors and
the mode calls of the handle, its decisions from an OracleNKA.scalar_step of its own on its own sums) passes it in all three
flavours, in both fast sum modes and over mixed schedules whose configuration changes with every update, and every planted
fault makes the assertion meant for it fail -- so the assertions tests/test_update_parts_exact_gpu.py,
tests/test_sums_exact_gpu.py and tests/test_mode_changes_exact_gpu.py make on the GPU can fail.  The last test runs the stand-in
over the very schedules of tests/test_mode_changes_exact_gpu.py and holds it to the coverage records those tests assert.

The stand-in writes its statements out by itself; of the checker it uses only _bits_equal (to tell whether a fault changed a
bit) and the mode numbers."""
import math
from fractions import Fraction

import numpy as np
import pytest

import batch_seq as B
import exact_sums as X
import mode_schedules as M
import split_update as U

MODES = pytest.mark.parametrize("mode", [U.SUMS_BLOCKED_ROUNDED, U.SUMS_BLOCKED], ids=["rounded", "blocked"])
N, MVEC, CALLS = 65, 5, 40                     # (CALLS of the sequence, MVEC + 2 more behind it)
NCU = 256                                      # the stand-in's "device": what exact_sums.device_k takes the grids from


# ---- the same update in numpy, behind the accessors the checker uses ------------------------------------------------------------
def fma(a, b, c):
    """fl(a*b + c), one rounding."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# fault -> the text of the assertion of the checker it has to trip
FAULTS = {"fma": "f_out",
          "coefficient_of_the_next_pair": "f_out",
          "rcp_for_div": "stored w1' is not",
          "div_for_rcp": "stored w1' is not",
          "no_compact": "stored v1' is not",
          "tail_element": r"f_out', \d+, 1\)",                      # (exactly one element differs)
          "gram_divided": "'c'",
          "h_transposed": "'h'",
          "w_new_in_the_next_free_slot": "the new pair's w is not the input"}
# ... and the faults that only a handle whose configuration changes can have
MIXED_FAULTS = {"stale_mode": "the scalar step",
                "stale_weights": "a fast sum beyond gamma",
                "tail_after_realign": "a fast sum beyond gamma",
                "hostdot_identity_tables": "dp operand",
                "stale_red_past_list": "past the list: not exactly 0"}


# ... and one that no single update shows: SUMS_AUTO sums in the reference's order up to 65 elements instead of 64.  A sequential
# sum of 65 products is inside the fast bound; split_update.assert_auto_boundary sees that no red[0] of the plain handle ever
# left the sequential sum's bits
AUTO_FAULT = "auto_threshold_65"


class Refused(RuntimeError):
    """A refused call: the text carries the library's code like nka_amd.NKAError's, "(-1)" or "(-5)"."""

    def __init__(self, code, what):
        super().__init__(f"{what} failed ({code})")


class StandIn:
    """A stand-in accelerator in numpy: state, reductions, w, v, accel_update, accel_update_swap, relax, restart, set_vec_tol and
    the calls that change how an update is made (set_sum_order, set_dot_weights, set_host_dot, set_dot_prod, set_shard) with
    the refusals of include/nka_hip.h.  It takes its decisions from an OracleNKA.scalar_step of its own on its own sums:
    np.dot for the fast ways, a loop for the reference's order, the caller's function for the user dot product.  Whether f is
    16-byte aligned it reads off the array's address.  `fault`: one of FAULTS or MIXED_FAULTS, planted in the statement of that
    name (None: the update as the reference states it)."""

    def __init__(self, oracle, n, mvec, flavor, fault=None):
        assert fault is None or fault in FAULTS or fault in MIXED_FAULTS or fault == AUTO_FAULT
        self.n, self.m, self.fl, self.fault = n, mvec, flavor, fault
        self.ora = oracle.OracleNKA(n, mvec, flavor)
        self.mode = U.SUMS_AUTO
        self.wgt = self.dot = self.hook = None
        self.shard = False
        self.W, self.V = np.zeros((mvec + 2, n)), np.zeros((mvec + 2, n))
        self.Wmajor, self.foreign = np.zeros((mvec + 2, n)), set()   # the slot-major array; the slots whose w lies elsewhere
        self.red = np.zeros(2 + 2 * mvec)
        self.fired = False                                   # the planted fault changed at least one bit
        self._was_raw = self._old_wgt = self._aligned = None  # what the faults of a changed configuration remember
        self._new_mode = self._new_wgt = self._relaxed = False

    def flavor(self):
        return self.fl

    def device_info(self):
        return "numpy", NCU

    # -- how the next update is made --
    def set_sum_order(self, mode):
        if mode == U.SUMS_REFERENCE_ORDER and self.wgt is not None:
            raise Refused(U.EINVAL, "set_sum_order")
        if mode != self.mode:
            self._was_raw, self._new_mode = self.mode == U.SUMS_BLOCKED, True
        self.mode = mode
        return self

    def set_dot_weights(self, w):
        if w is None:
            self.wgt = None
            return self
        if self.dot is not None:
            raise Refused(U.ESTATE, "set_dot_weights")
        if self.mode == U.SUMS_REFERENCE_ORDER:
            raise Refused(U.EINVAL, "set_dot_weights")
        self._old_wgt, self._new_wgt = self.wgt, True
        self.wgt = np.array(w, dtype=np.float64)
        return self

    def set_host_dot(self, dot):
        if dot is not None and self.wgt is not None:
            raise Refused(U.ESTATE, "set_host_dot")
        self.dot = dot

    def set_dot_prod(self, hook):
        self.hook = hook

    def set_shard(self, rank, nranks):
        self.shard = True
        return self

    def set_vec_tol(self, vtol):
        self.ora.set_vec_tol(vtol)

    def relax(self):
        self._relaxed = self.ora.state().pending
        self.ora.relax()

    def restart(self):
        self.ora.restart()

    def state(self):
        st = self.ora.state()
        live = st.list_order()[1:]
        if self.fault == "h_transposed" and len(live) >= 3:          # (the newest live entry's pivot is 1: its two entries agree)
            i, j = live[1] - 1, live[2] - 1
            self.fired |= st.h[i, j] != st.h[j, i]
            st.h[i, j], st.h[j, i] = st.h[j, i], st.h[i, j]
        return st

    def reductions(self):
        return self.red.copy()

    def w(self, slot):
        return self.W[slot].copy()

    def v(self, slot):
        return self.V[slot].copy()

    @staticmethod
    def _scaled(reciprocal, s, x):
        return (np.float64(1.0) / s) * x if reciprocal else x / s

    def _norm(self, x, s):
        """The pair by s: by its reciprocal in the F08-vector flavour -- the other way round if that is the fault."""
        right = self._scaled(self.fl == 1, s, x)
        if self.fault in ("rcp_for_div", "div_for_rcp"):
            wrong = self._scaled(self.fl != 1, s, x)
            self.fired |= not U._bits_equal(wrong, right)
            return wrong
        return right

    def _way(self):
        """(R | B | O | H, weighted): pick_sums_stage of nka_hip.hip."""
        if self.dot is not None:
            return "H", False
        if self.mode == U.SUMS_REFERENCE_ORDER and self.hook is not None:
            if not self.shard:
                raise Refused(U.ESTATE, "accel_update")
            return "O", False
        plain = self.hook is None and self.wgt is None
        auto_max = U.ORD_AUTO_MAX + (self.fault == AUTO_FAULT)
        if plain and (self.mode == U.SUMS_REFERENCE_ORDER or (self.mode == U.SUMS_AUTO and self.n <= auto_max)):
            self.fired |= self.fault == AUTO_FAULT and self.mode == U.SUMS_AUTO and self.n == auto_max
            return "O", False
        return ("B" if self.mode == U.SUMS_BLOCKED else "R"), self.wgt is not None

    def _store_w(self, slot, x):
        self.W[slot] = x
        if slot not in self.foreign:
            self.Wmajor[slot] = x

    def accel_update_swap(self, f):
        if self.dot is not None:
            raise Refused(U.ESTATE, "accel_update_swap")
        if f.ctypes.data % 16:
            raise Refused(U.EINVAL, "accel_update_swap")
        out = f.copy()
        self.accel_update(out, swap=True)
        return np.zeros(self.n), out

    def accel_update(self, f, swap=False):
        m, fl, W, V, fault = self.m, self.fl, self.W, self.V, self.fault
        way, weighted = self._way()
        st0 = self.ora.state()
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        x = f.copy()
        # -- the faults of a handle whose configuration has just changed
        aligned = swap or f.ctypes.data % 16 == 0
        cut = (fault == "tail_after_realign" and self._aligned is not None and aligned != self._aligned and self.n > 1
               and way in ("R", "B"))
        self._aligned = aligned
        wgt = self.wgt
        if fault == "stale_weights" and self._new_wgt and weighted and self._old_wgt is not None:
            wgt = self._old_wgt
        self._new_wgt = False
        Wop = W
        if fault == "hostdot_identity_tables" and way == "H":
            Wop = self.Wmajor                                # as if the slot -> buffer tables were the identity

        def total(a, b):
            """One inner product, the update's way."""
            if way == "H":
                return self.dot(a, b)
            if way == "O":
                acc = 0.0
                for p in (a * b).tolist():
                    acc += p
                return acc
            if weighted:
                a = wgt * a
            if cut:
                a, b = a[:-1], b[:-1]
            return np.dot(a, b)

        red = np.zeros(2 + 2 * m)
        hrow, rhs = np.zeros(m + 2), np.zeros(m + 2)
        s, normed = np.float64(0.0), False
        raw = way == "B"
        with np.errstate(all="ignore"):
            if pending:
                d = W[first0] - x
                red[0] = total(d, d)
                if self.hook is not None and way in ("R", "O"):
                    self.hook(0, 1, 0)
                s = np.sqrt(np.float64(red[0]))
                normed = not s == 0.0
            if normed:
                w1n, v1n = self._norm(d, s), self._norm(V[first0], s)
                lhs = d if raw else w1n                      # the blocked mode sums d, every other way the normalised pair
                if way != "H":
                    red[1] = total(x, lhs)
                for p, slot in enumerate(olders):
                    red[2 + p] = total(lhs, Wop[slot])
                    self.fired |= Wop is not W and not U._bits_equal(Wop[slot], W[slot])
                scale = raw                                  # ... and takes each sum by s in one operation
                if fault == "stale_mode" and self._new_mode and way != "H" and self._was_raw != raw:
                    scale = self._was_raw                    # the Gram row as the previous mode formed it
                    self.fired = True
                for p, slot in enumerate([first0] + olders):
                    row = red[1 + p]
                    if scale:
                        row = self._scaled(fl == 1, s, row)
                    elif fault == "gram_divided" and p > 0 and way == "R":
                        row = row / s
                        self.fired = True
                    if p == 0:
                        rhs[slot] = row
                    else:
                        hrow[slot] = row
            self._new_mode = False
            dp = getattr(self.dot, "pure", self.dot) if way == "H" else None      # (the projections dp is asked for later)
            for p, slot in enumerate(olders):
                rhs[slot] = dp(x, Wop[slot]) if way == "H" else total(x, Wop[slot])
                if way != "H":
                    red[2 + m + p] = rhs[slot]
            if way == "H" and normed:
                rhs[first0] = dp(x, w1n)
            if self.hook is not None and way != "H" and (pending or olders):
                self.hook(0, 2 + 2 * m if raw else 2 * m + 1, 0)
            if fault == "stale_red_past_list" and self._relaxed:
                for p in range(len(olders), m):              # what the update before the relax left there
                    for i in (2 + p, 2 + m + p):
                        self.fired |= self.red[i] != 0.0
                        red[i] = self.red[i]
            self._relaxed = False
            self.fired |= cut and (pending or bool(olders))
            self.fired |= wgt is not self.wgt and (pending or bool(olders))
            self.red = red
            new = self.ora.scalar_step(float(s), hrow, rhs)
            st = self.ora.state()
            comb = st.list_order()[1:]
            if way == "H":                                   # F08:371, after the drops, first ... last
                for slot in comb:
                    self.dot(x, w1n if normed and slot == first0 else Wop[slot])
                    self.fired |= Wop is not W and not U._bits_equal(Wop[slot], W[slot])
            if normed:
                self._store_w(first0, w1n)
                V[first0] = v1n - w1n if fl == 2 and fault != "no_compact" else v1n
                self.fired |= fault == "no_compact" and fl == 2
            c = [st.c[slot - 1] for slot in comb]
            if fault == "coefficient_of_the_next_pair" and len(comb) >= 2:
                c = c[1:] + c[-1:]
                self.fired = True
            out = x.copy()
            for ck, slot in zip(c, comb):
                if fl == 0:
                    nxt = (out - ck * W[slot]) + ck * V[slot]
                elif fl == 1:
                    nxt = ((-ck) * W[slot] + ck * V[slot]) + out
                else:
                    nxt = out + ck * V[slot]
                if fault == "fma":                           # the last product and sum of the statement contracted, a few elements
                    for i in range(min(self.n, 8)):
                        if fl == 0:
                            e = fma(ck, V[slot][i], out[i] - ck * W[slot][i])
                        elif fl == 1:
                            e = fma(ck, V[slot][i], (-ck) * W[slot][i]) + out[i]
                        else:
                            e = fma(ck, V[slot][i], out[i])
                        self.fired |= e != nxt[i] and not (math.isnan(e) and math.isnan(nxt[i]))
                        nxt[i] = e
                out = nxt
            if fault == "tail_element" and comb and self.n:
                self.fired |= out[-1] != x[-1]
                out[-1] = x[-1]
        if swap:
            self.foreign.add(new)                            # the caller's buffer becomes the slot's: the slot-major row is stale
        if fault == "w_new_in_the_next_free_slot" and st.free != 0:
            W[st.free] = x
            self.fired = True
        else:
            self._store_w(new, x)
        V[new] = out
        f[:] = out


# ---- the tests --------------------------------------------------------------------------------------------------------------------
def _drive(oracle, flavor, mode, fault=None, swap=False, seed=65005):
    acc = StandIn(oracle, N, MVEC, flavor, fault)
    run = U.SplitRun(None, oracle, acc, flavor, N, MVEC, mode, swap=swap)
    seq = B.Sequence(N, seed)
    for t in range(CALLS):
        run.update(seq.next(), swap=swap and t % 3 != 2)
        if t == 20:
            run.relax()
        if t == 30:
            run.restart()
    rng = np.random.default_rng(seed)               # a raised tolerance on a grown list: several entries go at once
    for t in range(MVEC + 2):
        if t == MVEC:
            run.set_vec_tol(0.95)
        run.update(rng.standard_normal(N))
    run.finish()
    return run, acc


@MODES
@pytest.mark.parametrize("swap", [False, True], ids=["in-place", "out-of-place"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_the_stand_in_passes_the_checker(oracle, flavor, mode, swap):
    """... on a batch_seq.Sequence (fresh, dependent, repeated and zero inputs) with a relax and a restart, and the run meets
    what the coverage record is there for."""
    run, _ = _drive(oracle, flavor, mode, swap=swap)
    assert run.calls == CALLS + MVEC + 2 and run.full_at_entry and run.capacity_drop and run.zero_s
    assert run.after_relax and run.after_restart and run.dropped_newest and run.dropped_mid
    assert 1 in run.dropped_at_once and run.dropped_at_once & {2, 3}, run.dropped_at_once
    assert {c for c, _ in run.ncomb} == set(range(MVEC + 1)), run.ncomb
    assert {r for _, r in run.ncomb} == {True, False}
    assert 0 in run.nolder_no_pending and max(run.nolder_no_pending) > 0 and max(run.nolder_pending) == MVEC


FAULT_CASES = [(fault, flavor, mode)
               for fault in FAULTS for flavor in (0, 1, 2) for mode in (U.SUMS_BLOCKED_ROUNDED, U.SUMS_BLOCKED)
               if not (fault == "rcp_for_div" and flavor == 1) and not (fault == "div_for_rcp" and flavor != 1)
               and not (fault == "no_compact" and flavor != 2) and not (fault == "gram_divided" and mode == U.SUMS_BLOCKED)]


@pytest.mark.parametrize("fault,flavor,mode", FAULT_CASES,
                         ids=[f"{f}-{fl}-{'rounded' if m == U.SUMS_BLOCKED_ROUNDED else 'blocked'}" for f, fl, m in FAULT_CASES])
def test_every_planted_fault_fails_the_checker(oracle, fault, flavor, mode):
    """The combine contracted to an fma; the coefficient of pair j+1 on pair j; fl(1/s)*d for d/s and the reverse; v1' stored
    without the compact subtraction; one tail element left at f_in; the Gram row divided by s in the rounded mode; one entry
    of h transposed; w_new written to the free list's next slot.  Each trips the assertion on the statement it was planted in
    (FAULTS), not one of the checker's own bookkeeping."""
    acc = StandIn(oracle, N, MVEC, flavor, fault)
    run = U.SplitRun(None, oracle, acc, flavor, N, MVEC, mode)
    seq = B.Sequence(N, 65005)
    with pytest.raises(AssertionError, match=FAULTS[fault]):
        for _ in range(CALLS):
            run.update(seq.next())
        run.finish()
    assert acc.fired, "the planted fault changed no bit"
    assert run.calls < CALLS                        # (an update failed, not only the read-back at the end)


# ---- a handle whose configuration changes with every update ----------------------------------------------------------------------
def _mixed(oracle, flavor, ops, n=N, mvec=MVEC, fault=None, seed=3):
    acc = StandIn(oracle, n, mvec, flavor, fault)
    run = U.SplitRun(None, oracle, acc, flavor, n, mvec)
    return M.play(run, ops, NCU, seed, background=M.background_for(mvec)), acc


@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_the_stand_in_passes_the_checker_over_every_change_of_configuration(oracle, flavor):
    """The 23 legal configurations, every ordered pair of them, with the hook on and off, dependent and repeated inputs,
    relax, restart and a raised tolerance laid over it: sums, hook counts, dp calls, scalar step, statements."""
    ops = M.all_legal()
    run, _ = _mixed(oracle, flavor, ops)
    assert run.calls == len(M.updates(ops)) == 23 * 23 + 1
    assert M.pairs_met(run) == M.all_pairs(U.configs())
    assert run.hooked > 100 and set(run.ways) == set(U.SUMS)
    met = {c for _, c in M.pairs_met(run, keep_hook=True)}
    assert {M.strip(c) for c in met if c.hook} == {c for c in U.configs() if c.sums != "H"}
    assert run.sharded and {c.entry for c in met if c.hook and c.sums == "O"} == set(U.ENTRIES)
    for way in U.SUMS:
        assert run.ways[way] == U.EVERY_RECORD, (way, U.EVERY_RECORD - run.ways[way])


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("fault", list(MIXED_FAULTS))
def test_every_fault_of_a_changed_configuration_fails_the_checker(oracle, fault, flavor):
    """The first update after set_sum_order forms the Gram row as the previous mode did; the first update after new weights
    sums with the old ones; the first update after the alignment of f changed leaves the last element (a sentinel) out of the
    sums; after an out-of-place update the dp operands come from the slot-major rows; after a relax an entry past the list
    keeps its old value.  Each trips its own assertion (MIXED_FAULTS)."""
    ops = M.all_legal()
    acc = StandIn(oracle, N, MVEC, flavor, fault)
    run = U.SplitRun(None, oracle, acc, flavor, N, MVEC)
    with pytest.raises(AssertionError, match=MIXED_FAULTS[fault]):
        M.play(run, ops, NCU, 3)
    assert acc.fired, "the planted fault changed no bit"
    assert run.calls < len(M.updates(ops))


def test_the_sentinel_at_the_last_element_is_what_the_sums_check_sees():
    """tail_after_realign leaves out x[n - 1]: exact_sums.planted_input puts a sentinel there, far above the bound."""
    rng = np.random.default_rng(1)
    x, y = X.planted_input(N, NCU, rng), X.planted_input(N, NCU, rng)
    k = X.device_k(N, NCU, False)
    assert abs(x[-1]) >= 1.0 and abs(y[-1]) >= 1.0
    assert X.detectable(x[-1] * y[-1], X.gamma(k), X.abs_dot(x, y))


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_stand_in_meets_every_record_on_the_schedules_of_the_gpu_tests(oracle, name):
    """tests/test_mode_changes_exact_gpu.py asserts, from the run's own record, every ordered pair of configurations and per way
    of forming the sums a capacity drop, a dependence drop, s == 0, an update right after relax and one right after restart.
    The periods of mode_schedules are chosen so that the numpy stand-in alone meets all of it on the same schedules, at the
    same shapes."""
    n, mvec, flavors, schedule, ways = M.CASES[name]
    ops = schedule()
    for flavor in flavors:
        run, _ = _mixed(oracle, flavor, ops, n=n, mvec=mvec, seed=n + mvec)
        if name.startswith("auto"):
            assert M.pairs_met(run, keep_hook=True) == M.all_pairs(M.AUTO_NODES)
            U.assert_auto_boundary(run)
        elif name == "all-legal":
            assert M.pairs_met(run) == M.all_pairs(U.configs())
        else:
            assert {(p.sums, c.sums) for p, c in M.pairs_met(run)} == {(p, c) for p in U.SUMS for c in U.SUMS}
        assert set(run.ways) == set(ways), run.ways.keys()
        for way in ways:
            assert run.ways[way] == U.EVERY_RECORD, (name, flavor, way, U.EVERY_RECORD - run.ways[way])


def test_an_auto_threshold_off_by_one_fails_the_auto_boundary_check(oracle):
    """At n = 65 a stand-in whose SUMS_AUTO still sums in the reference's order passes every update of the auto-65 schedule -- its
    sums are inside the fast bound -- and meets every record; assert_auto_boundary is what fails."""
    n, mvec, _, schedule, ways = M.CASES["auto-65"]
    acc = StandIn(oracle, n, mvec, 2, AUTO_FAULT)
    run = M.play(U.SplitRun(None, oracle, acc, 2, n, mvec), schedule(), NCU, n + mvec)
    assert acc.fired and all(run.ways[way] == U.EVERY_RECORD for way in ways)
    with pytest.raises(AssertionError, match="the rounded passes did not run"):
        U.assert_auto_boundary(run)
    assert run.fast_not_ordered == {"A": False, "A+hook": True, "Aw": True}


def test_circuit_takes_every_arc_once():
    for k in (1, 2, 6, 9, 23):
        walk = U.circuit(k)
        assert walk[0] == walk[-1] and len(walk) == k * k + 1
        assert set(zip(walk, walk[1:])) == {(i, j) for i in range(k) for j in range(k)}


def test_bits_equal_tells_signed_zeros_apart_and_nan_payloads_not():
    a = np.array([0.0, 1.0, np.nan])
    assert U._bits_equal(a, a.copy()) and not U._bits_equal(a, np.array([-0.0, 1.0, np.nan]))
    b = a.copy()
    b.view(np.int64)[2] ^= 1                        # another NaN payload
    assert np.isnan(b[2]) and U._bits_equal(a, b) and not U._bits_equal(a, np.array([0.0, 1.0, 2.0]))
