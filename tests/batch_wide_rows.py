"""Helpers of the tests of the wide batch's scalar step on one wavefront (nka_hip_batch_set_scalar_step; include/nka_hip_batch.h,
SCALAR STEP): tests/test_batch_wide_rows_cpu.py and tests/test_batch_wide_rows_gpu.py.

  model_step      a numpy model of batch_scalar_step_rows (nka_amd/csrc/nka_batch_dev.hpp): the right-looking factorisation with
                  drops, the right-hand side riding along as one more row, the column-oriented back-substitution -- one rounding per
                  operation, in the order of the device function.  Its target is the oracle's scalar_step.
  script          the sequences of the twin tests: eight systems with staggered starts, built to reach every branch of the drop logic
  census_of       what one update did to one system, read off the states before and after it
"""
import numpy as np

NSYS = 8
MVECS = (1, 2, 5, 10, 11, 20, 21, 32)      # both sides of every NLMAX boundary (6 / 11 / 21 / 33 rows) and the largest
TINY_VTOL, VTOL = 1e-12, 0.01
EPS = 1e-4                                 # a `near` direction is e + EPS r: kept under TINY_VTOL, dependent under VTOL
CENSUS = ("two_dep", "dep_first", "dep_last", "capacity", "last_evaluated", "relax_s0", "no_new_pair")
MUTATIONS = ("dropped_row_not_stored", "dropped_diagonal_written", "dropped_rhs_left", "ascending_back_substitution")


# ---- the model ---------------------------------------------------------------------------------------------------------------------

class Work:
    """A working copy in the Fortran numbering (slot 0 = end of list), from a State of oracle_py / nka_amd."""

    def __init__(self, st, mvec, vtol):
        n = mvec + 1
        self.mvec, self.vtol = mvec, np.float64(vtol)
        self.h = np.zeros((n + 1, n + 1))
        self.h[1:, 1:] = st.h
        self.c = np.zeros(n + 1)
        self.c[1:] = st.c
        self.next = np.zeros(n + 1, np.int64)
        self.prev = np.zeros(n + 1, np.int64)
        self.next[1:], self.prev[1:] = st.next, st.prev
        self.first, self.last, self.free = st.first, st.last, st.free
        self.subspace, self.pending = int(st.subspace), int(st.pending)

    def order(self):
        out, k = [], self.first
        while k != 0:
            out.append(k)
            k = int(self.next[k])
        return out


def _relax(L):
    dropped = L.first
    L.first = int(L.next[dropped])
    if L.first == 0:
        L.last = 0
    else:
        L.prev[L.first] = 0
    L.next[dropped] = L.free
    L.free = dropped
    L.pending = 0


def _prepend(L, slot):
    L.prev[slot] = 0
    L.next[slot] = L.first
    if L.first == 0:
        L.last = slot
    else:
        L.prev[L.first] = slot
    L.first = slot
    L.pending = 1


def _solve_on_one_lane(L):
    """lst_solve: the path without a new pair."""
    order = L.order()
    for a, j in enumerate(order):
        cj = L.c[j]
        for i in order[:a]:
            cj = cj - L.h[j, i] * L.c[i]
        L.c[j] = cj / L.h[j, j]
    for a in range(len(order) - 1, -1, -1):
        j = order[a]
        cj = L.c[j]
        for i in reversed(order[a + 1:]):
            cj = cj - L.h[i, j] * L.c[i]
        L.c[j] = cj / L.h[j, j]


def model_step(L, s, hrow, b, mutate=None):
    """One scalar step of batch_scalar_step_rows on the working copy L.  hrow, b: indexed by slot like the oracle's scalar_step
    (hrow[k] = <w1', w_k>, b[j] = <f, w_j>).  -> (new slot, positions dropped by dependence, position dropped by capacity or
    None); L.c of a dropped older entry holds the raw b.  mutate: one of MUTATIONS -- a wrong model, which must not pass."""
    s = np.float64(s)
    with np.errstate(all="ignore"):
        if L.pending and s == 0.0:
            _relax(L)
        if not L.pending:                      # (uniform branch: lane 0 runs the one-thread step)
            slot = L.free
            L.free = int(L.next[slot])
            if L.subspace:
                for j in L.order():
                    L.c[j] = b[j]
                _solve_on_one_lane(L)
            _prepend(L, slot)
            return slot, [], None
        order = L.order()                      # position -> slot: the pending entry, then the older ones
        nl, first, mvec = len(order), L.first, L.mvec
        vtol2 = L.vtol * L.vtol
        # phase 0: the Gram row and the raw right-hand sides, every older entry
        L.h[first, first] = 1.0
        for k in order[1:]:
            L.h[first, k] = hrow[k]
        for k in order:
            L.c[k] = b[k]
        # row p of the position-indexed matrix: a[p][q] = H(slot_q, slot_p), q newer; row nl: the right-hand side
        a = np.zeros((nl + 1, nl))
        for p in range(nl):
            for q in range(nl):
                a[p, q] = L.h[order[q], order[p]]
        for q in range(nl):
            a[nl, q] = L.c[order[q]]
        alive = [True] * nl
        ddr = np.ones(nl)
        Ldr = np.ones(nl)
        capdrop, kept, open_ = None, 0, True
        # phase 1: right-looking, column by column
        for i in range(nl):
            keep, Lii = False, np.float64(1.0)
            if open_:
                if i == 0:
                    keep = True
                elif kept + 1 > mvec:
                    capdrop, open_ = i, False
                else:
                    hkk = ddr[i]
                    keep = bool(hkk > vtol2)
                    if keep:
                        Lii = np.sqrt(hkk)
                if not keep:
                    alive[i] = False
            if keep:
                kept += 1
                Ldr[i] = Lii
                l = a[:, i] / Lii              # every row at once: one division each
                a[:, i] = l
                for p in range(i + 1, nl):
                    ddr[p] = ddr[p] - l[p] * l[p]
                for q in range(i + 1, nl):
                    a[:, q] = a[:, q] - l * l[q]
        # phase 2: the rows back by slot; the drops in list order
        for p in range(1, nl):
            if p == capdrop:
                continue
            if not alive[p] and mutate == "dropped_row_not_stored":
                continue
            for q in range(p):
                if alive[q]:
                    L.h[order[p], order[q]] = a[p, q]
            if alive[p] or mutate == "dropped_diagonal_written":
                L.h[order[p], order[p]] = Ldr[p] if alive[p] else np.sqrt(np.abs(ddr[p]))
        dep = []
        for p in range(1, nl):
            if alive[p]:
                continue
            k = order[p]
            if p == capdrop:
                L.next[L.last] = L.free
                L.free = k
                L.last = int(L.prev[k])
                L.next[L.last] = 0
            else:
                dep.append(p)
                pv, nx = int(L.prev[k]), int(L.next[k])
                L.next[pv] = nx
                if nx == 0:
                    L.last = pv
                else:
                    L.prev[nx] = pv
                L.next[k] = L.free
                L.free = k
        L.subspace, L.pending = 1, 0
        # phase 3: the new slot; the back-substitution by columns
        slot = L.free
        L.free = int(L.next[slot])
        y = a[nl].copy()
        cols = range(nl) if mutate == "ascending_back_substitution" else range(nl - 1, -1, -1)
        for i in cols:
            if not alive[i]:
                continue
            ci = y[i] / Ldr[i]
            y[i] = ci
            for p in range(i):
                if alive[p]:
                    y[p] = y[p] - a[i, p] * ci
        for p in range(nl):
            if alive[p] or mutate == "dropped_rhs_left":
                L.c[order[p]] = y[p]
        _prepend(L, slot)
        return slot, dep, capdrop


# ---- the sequences -------------------------------------------------------------------------------------------------------------------

def switch_call(mvec):
    """The call ahead of which vtol goes from TINY_VTOL to VTOL: systems 0 ... 3 then hold full lists."""
    return mvec + 5


def ncalls(mvec):
    return switch_call(mvec) + 10


def twin_seed(mvec, flavor):
    """The seed of the twin test's sequences at this point of its grid (the CPU census runs the same ones)."""
    return 100 * mvec + flavor


def _unit(rng, n):
    x = rng.standard_normal(n)
    return x / np.linalg.norm(x)


def script(lens, mvec, seed, ill=NSYS - 1):
    """Yields one dict per call: {"vtol": value or None (set ahead of the call, for ALL systems), "relax": [systems], "restart":
    [systems] (masked, ahead of the call), "inputs": {system: the row it is fed}, "retire": [systems] (a step retires them)}.
    System k starts k calls late, so one launch holds older counts from 0 up.  lens[k]: the length of system k.  The stored w of
    an update is the normalised difference of two successive inputs, so a system's directions are chosen freely:
      rand   a fresh random direction                        near   e_k + EPS r: dependent on every other `near` under VTOL
      same   the input again (s == 0: relax, and a solve without a new pair)
    Up to switch_call(mvec) the lists fill under TINY_VTOL with near and rand in a pattern that differs from system to system
    (capacity drops from update mvec + 2 on); then VTOL, and a near input drops every near entry of the list at once -- several
    dependence drops in one update, at the first older position, at the last, and with the last position of a full list
    evaluated behind a drop; then s == 0 on the even systems, a masked relax, a masked restart, and NaN and Inf for system
    `ill`."""
    nsys = len(lens)
    rngs = [np.random.default_rng([seed, mvec, k]) for k in range(nsys)]
    base = [_unit(rngs[k], lens[k]) for k in range(nsys)]
    prev = [rngs[k].standard_normal(lens[k]) for k in range(nsys)]
    P = switch_call(mvec)
    for t in range(ncalls(mvec)):
        ev = {"vtol": None, "relax": [], "restart": [], "inputs": {}, "retire": []}
        if t == 0:
            ev["vtol"] = TINY_VTOL
        if t == P:
            ev["vtol"] = VTOL
        if t == P + 1:
            ev["retire"] = [3]
        if t == P + 4:
            ev["relax"] = [1, 5]
        if t == P + 5:
            ev["restart"] = [2, 6]
        for k in range(nsys):
            j = t - k
            if j < 0:
                continue
            if t < P:
                kind = "rand" if (j + k) % 3 == 0 else "near"
            else:
                kind = ("near", "rand", "near", "same" if k % 2 == 0 else "rand", "rand", "rand", "near", "rand", "near", "rand")[t - P]
            if j == 0:
                x = prev[k]
            elif kind == "same":
                x = prev[k].copy()
            else:
                d = base[k] + EPS * _unit(rngs[k], lens[k]) if kind == "near" else _unit(rngs[k], lens[k])
                x = prev[k] - d
            prev[k] = x
            fed = x
            if k == ill and t == P + 6:
                fed = x.copy()
                fed[lens[k] - 1] = np.nan
            if k == ill and t == P + 7:
                fed = x.copy()
                fed[0] = np.inf
            ev["inputs"][k] = fed
        yield ev


def census_of(before, after, mvec):
    """The tags of CENSUS one update earned on one system, from its states before and after."""
    tags = set()
    lb, la = before.list_order(), after.list_order()
    kept = la[1:]                              # (la[0], the new slot, may be the slot of an entry this update dropped)
    if not before.pending:
        if before.subspace:
            tags.add("no_new_pair")
        return tags
    if lb[0] not in kept:                      # the pending entry itself went: s == 0 relaxed it
        tags.add("relax_s0")
        if before.subspace:
            tags.add("no_new_pair")
        return tags
    older = lb[1:]
    gone = [p for p, k in enumerate(older) if k not in kept]
    full = len(lb) == mvec + 1
    if full and gone == [len(older) - 1]:      # every entry ahead of the last was kept: kept + 1 > mvec at the last
        tags.add("capacity")
        return tags
    if len(gone) >= 2:
        tags.add("two_dep")
    if gone and gone[0] == 0:
        tags.add("dep_first")
    if gone and gone[-1] == len(older) - 1:
        tags.add("dep_last")
    if full and any(p < len(older) - 1 for p in gone):
        tags.add("last_evaluated")
    return tags


def census_short(census):
    """The tags of CENSUS that were never earned."""
    return [tag for tag in CENSUS if census.get(tag, 0) < 1]
