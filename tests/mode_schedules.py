"""The schedules of tests/test_mode_changes_exact_gpu.py: which configuration (split_update.Config) every update of a run is
made in, and what is laid over it.  They are host code: tests/test_split_update_cpu.py runs every one of them over the numpy
stand-in and asserts there, on the CPU, that the stand-in alone meets every record the GPU tests assert.

A schedule is a list of operations: ("update", Config, kind) with kind "fresh" | "dependent" | "repeat"; ("relax",);
("restart",); ("vtol", value).  Its updates walk split_update.circuit over the nodes in question -- a closed walk through the
complete directed graph, self-loops included --, so every ordered pair (previous configuration, this configuration) occurs.
Laid over it, with periods coprime to one another and to the lengths of the walks (37, 82, 530):
  every DEP-th update takes a dependent input, a combination of the previous two inputs whose difference from the previous
  one is parallel to the stored difference: the newest older entry goes by dependence;
  every REP-th update repeats the previous input (s == 0);
  before every RELAX-th update relax(), before every RESTART-th one restart();
  before every VTOL-th update set_vec_tol(0.95), two updates later the default again (several entries go at once).
play() draws the inputs: exact_sums.planted_input, sentinels where the sum kernels change hands."""
import numpy as np

import exact_sums as X
import split_update as U

PERIODS = (7, 11, 13, 43, 17)                    # DEP, REP, RELAX, RESTART, VTOL of the long walk
VTOL_RAISED, VTOL_DEFAULT = 0.95, 0.01


def overlay(cfgs, restarts=True, start=0, periods=PERIODS):
    """The operations of one walk: `cfgs` in turn, the periodic events counted from update number `start`."""
    DEP, REP, RELAX, RESTART, VTOL = periods
    ops = []
    for i, cfg in enumerate(cfgs):
        t = start + i
        if restarts and t % RESTART == RESTART - 1:
            ops.append(("restart",))
        elif t % RELAX == RELAX - 1:
            ops.append(("relax",))
        if t % VTOL == VTOL - 1:
            ops.append(("vtol", VTOL_RAISED))
        if t % VTOL == 1 and t > 1:
            ops.append(("vtol", VTOL_DEFAULT))
        kind = "dependent" if t % DEP == DEP - 1 else "repeat" if t % REP == REP - 1 else "fresh"
        ops.append(("update", cfg, kind))
    return ops


def updates(ops):
    return [op for op in ops if op[0] == "update"]


def all_legal():
    """The 23 legal (sums, entry) pairs: 530 updates, the hook on for two updates of five wherever it may be."""
    nodes = U.configs()
    assert len(nodes) == 23
    cfgs = [nodes[i] for i in U.circuit(len(nodes))]
    cfgs = [c._replace(hook=(t % 5 in (2, 3)) and c.sums != "H") for t, c in enumerate(cfgs)]
    return overlay(cfgs)


def _entries_rotating(sums_walk, entries=U.ENTRIES):
    out, k = [], 0
    for s in sums_walk:
        while not U.legal(U.Config(s, entries[k % len(entries)])):
            k += 1
        out.append((s, entries[k % len(entries)]))
        k += 1
    return out


AXIS_PERIODS = (3, 5, 7, 17, 19)                 # ... of the 6 x 6 walks: six laps of 37
AUTO_PERIODS = (3, 5, 13, 23, 11)                # ... of the 9 x 9 walk
FULL_PERIODS = (7, 11, 13, 10 ** 6, 10 ** 6)     # ... of a lap on a full long list: no restart, no raised tolerance


def sum_axis(mvec, hook, laps=6, periods=AXIS_PERIODS, full_lap=False):
    """The 6 x 6 circuit over the sum-forming axis, the entry rotating through a, u, s, h: `laps` walks with the periodic
    events running on.  full_lap (a list too long to fill between two restarts): behind them mvec + 1 fresh inputs fill the
    list, and one more walk without restart and raised tolerance lets every way meet the full list."""
    walk = [U.SUMS[i] for i in U.circuit(len(U.SUMS))]

    def lap(first):
        return [U.Config(s, e, hook and s != "H") for s, e in _entries_rotating(walk if first else walk[1:])]

    ops, t = [], 0
    for k in range(laps):
        cfgs = lap(k == 0)
        ops += overlay(cfgs, start=t, periods=periods)
        t += len(cfgs)
    if full_lap:
        fill = [U.Config(s, e, hook and s != "H") for s, e in _entries_rotating((U.SUMS * (mvec + 1))[:mvec + 1])]
        ops += [("vtol", VTOL_DEFAULT)] + [("update", c, "fresh") for c in fill]
        ops += overlay(lap(False), restarts=False, start=1, periods=FULL_PERIODS)
    return ops


AUTO_NODES = [U.Config(s, e, h) for s, h in (("A", False), ("A", True), ("Aw", False)) for e in ("a", "u", "h")]


def auto_boundary(periods=AUTO_PERIODS):
    """{no transport, the hook, weights} x {a, u, h} under SUMS_AUTO: 82 updates."""
    return overlay([AUTO_NODES[i] for i in U.circuit(len(AUTO_NODES))], periods=periods)


def strip(cfg):
    return None if cfg is None else cfg._replace(hook=False)


def pairs_met(run, keep_hook=False):
    """The ordered pairs of configurations a run met (the transport kept apart unless keep_hook)."""
    f = (lambda c: c) if keep_hook else strip
    return {(f(p), f(c)) for p, c in run.pairs if p is not None}


def all_pairs(nodes):
    return {(p, c) for p in nodes for c in nodes}


def play(run, ops, ncu, seed, background=0.125):
    """Run the schedule on a split_update.SplitRun (background: exact_sums.planted_input's; a list of 33 only fills if the
    inputs stay independent beside their few sentinels, so the long list takes 1.0)."""
    rng = np.random.default_rng(seed)
    x1 = x2 = None
    for op in ops:
        if op[0] == "relax":
            run.relax()
        elif op[0] == "restart":
            run.restart()
        elif op[0] == "vtol":
            run.set_vec_tol(op[1])
        else:
            _, cfg, kind = op
            if kind == "repeat" and x1 is not None:
                x = x1.copy()
            elif kind == "dependent" and x2 is not None:
                x = 1.5 * x1 - 0.5 * x2                      # x1 - x = 0.5 (x2 - x1): parallel to the stored difference
            else:
                x = X.planted_input(run.n, ncu, rng, x1, background=background)
            run.update(x, cfg)
            x2, x1 = x1, x
    return run.finish()


def background_for(mvec):
    return 1.0 if mvec > 5 else 0.125


# name -> (n, mvec, flavours, the schedule, the ways whose records are asserted)
CASES = {
    "all-legal": (1031, 5, (2,), all_legal, U.SUMS),
    "sum-axis": (1031, 5, (0, 1), lambda: sum_axis(5, False), U.SUMS),
    "sum-axis-hook": (1031, 5, (0, 1), lambda: sum_axis(5, True), U.SUMS),
    "eight-tiles": (4099, 5, (2,), lambda: sum_axis(5, False), U.SUMS),
    "long-list": (1031, 33, (2,), lambda: sum_axis(33, False, full_lap=True), U.SUMS),
    "auto-64": (64, 3, (2,), auto_boundary, ("O", "R", "Rw")),
    "auto-65": (65, 3, (2,), auto_boundary, ("R", "Rw")),
}
