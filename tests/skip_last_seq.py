"""Call sequences for the skip of the last vector (nka_device.hpp, kSkipMay), shared by tests/test_skip_last_cpu.py -- which
holds every mark below against the oracle on the CPU -- and tests/test_skip_last_gpu.py, which runs two handles through them.

A sequence is a list of operations: ("update", x, mark) | ("relax",) | ("restart",) | ("vtol", value).  Every input depends
on the raw inputs before it only, never on a result, so the same list serves the oracle and the device.  `mark` is None or
the list positions (0 = the pending pair, 1 ... mvec = the older entries, newest first) that the update removes from a FULL
list -- mvec + 1 entries at its entry.  [mvec] is the capacity drop alone (F08:301-309), which the skip is built for; every
other mark is an update that needs the sums of the last vector after all and must take the repair.

The stored w of an entry is the normalised difference of two consecutive raw inputs, so the geometry below is that of the
inputs: fresh normal inputs give differences at 120 degrees to their neighbours and at right angles to the rest (pivot^2 =
0.75 +- 0.05 from 400 elements on, as tests/test_update_parts_exact_gpu.py uses it)."""
import numpy as np

CASES = ("capacity", "newest", "mid", "multi", "s0", "relax_restart")


def is_redo(mark, mvec):
    return mark is not None and mark != [mvec]


def sequence(case, n, mvec, seed=0):
    rng = np.random.default_rng(1000 * seed + 17 * mvec + n)
    X, ops = [], []
    cap = [mvec]

    def update(x, mark=None):
        X.append(x)
        ops.append(("update", x, mark))

    def fresh(mark=None):
        update(rng.standard_normal(n), mark)

    for _ in range(mvec + 1):        # the list grows to mvec + 1 entries
        fresh()
    for _ in range(2):
        fresh(cap)
    if case == "capacity":
        for _ in range(2 * mvec):
            fresh(cap)
        return ops
    if case == "newest":
        # the difference from the pending pair's input is parallel to the newest older entry: its pivot vanishes, it goes, and
        # the last entry is evaluated and kept
        update(X[-1] + 0.7 * (X[-1] - X[-2]), [1])
    elif case == "mid":
        # ... lies in the span of the two newest older entries: the second of them goes (a mid-list entry from mvec = 3 on)
        assert mvec >= 3
        update(X[-1] + 0.6 * (X[-1] - X[-2]) + 0.5 * (X[-2] - X[-3]), [2])
    elif case == "multi":
        # the raised tolerance takes the newest older entry and every second one behind it: with an odd mvec the last itself
        assert mvec % 2 == 1 and mvec <= 7
        ops.append(("vtol", 0.95))
        fresh(list(range(1, mvec + 1, 2)))
        ops.append(("vtol", 0.01))
        for _ in range(mvec + 3):    # (the list is short now and grows again: no marks)
            fresh()
        return ops
    elif case == "s0":
        update(X[-1].copy(), [0])    # s == 0: the pending pair is relaxed away inside the update, every older entry stays
    elif case == "relax_restart":
        ops.append(("relax",))
        fresh()                      # no pending pair: mvec entries, all of them needed
        for _ in range(2):
            fresh(cap)
        ops.append(("restart",))
        for _ in range(mvec + 1):
            fresh()
        for _ in range(2):
            fresh(cap)
        return ops
    else:
        raise ValueError(case)
    # behind a single drop (or the relaxed pair) the new pair fills the list again at once: capacity drops from here on,
    # mvec of them with the skip held off, then three with it
    for _ in range(mvec + 3):
        fresh(cap)
    return ops


def weights(n):
    """Diagonal dot-product weights for the weighted cases (nka_hip_set_dot_weights): the geometry above holds in any such
    metric -- a parallel difference stays parallel, a repeated input stays repeated."""
    return 0.5 + np.random.default_rng(n).random(n)


def removed_positions(before, after):
    """The positions of the list `before` an update (slots, first to last) that are no longer behind the new first entry."""
    kept = set(after[1:])
    return [i for i, k in enumerate(before) if k not in kept]
