"""The checker of tests/split_update.py on the CPU: a stand-in accelerator written in numpy (StandIn below: the accessors of the
handle, its decisions from an OracleNKA.scalar_step of its own on its own sums) passes it in all three flavours and both fast
sum modes, and every planted fault makes the assertion meant for it fail -- so the assertions
tests/test_update_parts_exact_gpu.py makes on the GPU can fail.

The stand-in writes its statements out by itself; of the checker it uses only _bits_equal (to tell whether a fault changed a
bit) and the mode numbers."""
import math
from fractions import Fraction

import numpy as np
import pytest

import batch_seq as B
import split_update as U

MODES = pytest.mark.parametrize("mode", [U.SUMS_BLOCKED_ROUNDED, U.SUMS_BLOCKED], ids=["rounded", "blocked"])
N, MVEC, CALLS = 65, 5, 40                     # (CALLS of the sequence, MVEC + 2 more behind it)


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


class StandIn:
    """A stand-in accelerator in numpy: state, reductions, w, v, accel_update, accel_update_swap, relax, restart, set_vec_tol.  It
    takes its decisions from an OracleNKA.scalar_step of its own on its own sums (np.dot).  `fault`: one of FAULTS, planted
    in the statement of that name (None: the update as the reference states it)."""

    def __init__(self, oracle, n, mvec, flavor, fault=None):
        assert fault is None or fault in FAULTS
        self.n, self.m, self.fl, self.fault = n, mvec, flavor, fault
        self.ora = oracle.OracleNKA(n, mvec, flavor)
        self.mode = U.SUMS_BLOCKED_ROUNDED
        self.W, self.V = np.zeros((mvec + 2, n)), np.zeros((mvec + 2, n))
        self.red = np.zeros(2 + 2 * mvec)
        self.fired = False                                   # the planted fault changed at least one bit

    def flavor(self):
        return self.fl

    def set_sum_order(self, mode):
        self.mode = mode
        return self

    def set_vec_tol(self, vtol):
        self.ora.set_vec_tol(vtol)

    def relax(self):
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

    def accel_update_swap(self, f):
        out = f.copy()
        self.accel_update(out)
        return np.zeros(self.n), out

    def accel_update(self, f):
        m, fl, W, V, fault = self.m, self.fl, self.W, self.V, self.fault
        st0 = self.ora.state()
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        x = f.copy()
        red = np.zeros(2 + 2 * m)
        hrow, rhs = np.zeros(m + 2), np.zeros(m + 2)
        s, normed = np.float64(0.0), False
        with np.errstate(all="ignore"):
            if pending:
                d = W[first0] - x
                red[0] = np.dot(d, d)
                s = np.sqrt(np.float64(red[0]))
                normed = not s == 0.0
            if normed:
                w1n, v1n = self._norm(d, s), self._norm(V[first0], s)
                rounded = self.mode == U.SUMS_BLOCKED_ROUNDED
                lhs = w1n if rounded else d                  # the rounded mode sums the normalised pair, the blocked one d
                red[1] = np.dot(x, lhs)
                for p, slot in enumerate(olders):
                    red[2 + p] = np.dot(lhs, W[slot])
                for p, slot in enumerate([first0] + olders):
                    row = red[1 + p]
                    if not rounded:                          # ... and takes each sum by s in one operation
                        row = self._scaled(fl == 1, s, row)
                    elif fault == "gram_divided" and p > 0:
                        row = row / s
                        self.fired = True
                    if p == 0:
                        rhs[slot] = row
                    else:
                        hrow[slot] = row
            for p, slot in enumerate(olders):
                red[2 + m + p] = rhs[slot] = np.dot(x, W[slot])
            self.red = red
            new = self.ora.scalar_step(float(s), hrow, rhs)
            st = self.ora.state()
            comb = st.list_order()[1:]
            if normed:
                W[first0] = w1n
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
        if fault == "w_new_in_the_next_free_slot" and st.free != 0:
            W[st.free] = x
            self.fired = True
        else:
            W[new] = x
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


def test_bits_equal_tells_signed_zeros_apart_and_nan_payloads_not():
    a = np.array([0.0, 1.0, np.nan])
    assert U._bits_equal(a, a.copy()) and not U._bits_equal(a, np.array([-0.0, 1.0, np.nan]))
    b = a.copy()
    b.view(np.int64)[2] ^= 1                        # another NaN payload
    assert np.isnan(b[2]) and U._bits_equal(a, b) and not U._bits_equal(a, np.array([0.0, 1.0, 2.0]))
