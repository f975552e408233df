"""A handle whose configuration changes between updates, held to the exact checks of tests/split_update.py after EVERY update:
the sums (exact sums within gamma(K) for the fast passes, the sequential sum's bits for the reference order, the reference's
dp calls for the user dot product), the hook's counts, the scalar step against the oracle on the device's own red[], the
elementwise statements and ring stores against numpy, the guards around an in-place f, finish().

The schedules (tests/mode_schedules.py) walk a circuit through the complete directed graph of configurations, self-loops
included, with dependent and repeated inputs, relax, restart and a raised tolerance laid over it; every test asserts from the
run's own record that every ordered pair (previous configuration, this configuration) occurred and that every way of
forming the sums met a capacity drop, a dependence drop, s == 0, an update right after relax and one right after restart.
tests/test_split_update_cpu.py shows on the CPU that a numpy stand-in meets all of it on the same schedules and that the
assertions fail on planted faults.  These are the smallest shapes at which this can go wrong, not the workload's."""
import json
import os
import time

import pytest

import exact_sums as X
import mode_schedules as M
import split_update as U

pytestmark = pytest.mark.gpu

TIMES = {}                                   # case -> wall seconds


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module", autouse=True)
def _fresh_record():
    U.WORST.clear()
    TIMES.clear()
    yield


def _report_lines():
    lines = [f"mode changes, sums {way}: worst |red - exact| = {r[0]:.3f} u sum|xy| against K = {r[1]} there ({r[2]})"
             for way, r in sorted(U.WORST.items())]
    return lines + [f"mode changes, {case}: {sec:.1f} s" for case, sec in TIMES.items()]


def mixed_run(torch, oracle, case, flavor, diagnostic=False, **tuning):
    """One handle through the schedule of mode_schedules.CASES[case] -> the SplitRun."""
    import nka_amd
    n, mvec, _, schedule, _ = M.CASES[case]
    acc = nka_amd.nka(diagnostic=diagnostic or bool(tuning)).init(n, mvec, flavor=flavor)
    for key, value in tuning.items():
        acc.set_tuning(key, value)
    mode = U.SUMS_BLOCKED_ROUNDED                      # (every update names its own configuration)
    run = U.SplitRun(torch, oracle, acc, flavor, n, mvec, mode, skip_last=tuning.get("skip_last") == 1)
    t0 = time.perf_counter()
    M.play(run, schedule(), run.ncu, n + mvec, background=M.background_for(mvec))
    TIMES[f"{case}-flavour{flavor}"] = time.perf_counter() - t0
    return run


def assert_every_record(run, ways):
    assert set(run.ways) == set(ways), sorted(run.ways)
    for way in ways:
        assert run.ways[way] == U.EVERY_RECORD, (way, "never met", U.EVERY_RECORD - run.ways[way])


def assert_the_sum_axis(run):
    assert {(p.sums, c.sums) for p, c in M.pairs_met(run)} == {(p, c) for p in U.SUMS for c in U.SUMS}
    assert {c.entry for _, c in M.pairs_met(run)} == set(U.ENTRIES)


def test_every_legal_configuration_after_every_other(torch_cuda, oracle):
    """n = 1031 (two tiles and a tail of 7), mvec = 5, flavour 2, the product library: the 23 legal (sums, entry) pairs, 530
    updates, the hook on for two updates of five; k_solve_rows<6>, under the user dot product k_solve."""
    run = mixed_run(torch_cuda, oracle, "all-legal", 2)
    assert run.calls == 23 * 23 + 1
    assert M.pairs_met(run) == M.all_pairs(U.configs())
    assert run.hooked > 100 and run.full_at_entry
    # the transport: every configuration the hook may lie on met it and met the handle without it; the reference order under
    # the hook, which needs set_shard, among them
    met = {c for _, c in M.pairs_met(run, keep_hook=True)}
    hookable = {c for c in U.configs() if c.sums != "H"}
    assert {M.strip(c) for c in met if c.hook} == hookable and {c for c in met if not c.hook} == set(U.configs())
    assert run.sharded and {c.entry for c in met if c.hook and c.sums == "O"} == set(U.ENTRIES)
    assert_every_record(run, U.SUMS)


@pytest.mark.parametrize("hook", [False, True], ids=["no-hook", "hook"])
@pytest.mark.parametrize("flavor", [0, 1])
def test_the_sum_forming_axis_in_the_other_flavours(torch_cuda, oracle, flavor, hook):
    """The 6 x 6 circuit, the entry rotating through a, u, s, h; once without a hook, once with the identity hook."""
    run = mixed_run(torch_cuda, oracle, "sum-axis-hook" if hook else "sum-axis", flavor)
    assert_the_sum_axis(run)
    assert (run.hooked > 100) if hook else run.hooked == 0
    assert_every_record(run, U.SUMS)


def test_eight_tiles_with_the_forced_variants(torch_cuda, oracle):
    """n = 4099 (eight tiles and a tail of 3), mvec = 5, the diagnostic library: chain_many = 1 on the reference-order updates
    (the block arrays are allocated in mid-life, behind out-of-place updates) and skip_last = 1 throughout -- the skipping
    handle held to the exact sums and the oracle directly: on an update that skipped, the two dead entries of red[] read 0
    and are left out of the sums check; an update that needed the last vector's sums raised the repair counter."""
    run = mixed_run(torch_cuda, oracle, "eight-tiles", 2, chain_many=1, skip_last=1)
    assert_the_sum_axis(run)
    assert run.skipped > 0 and run.redone > 0, (run.skipped, run.redone)
    assert_every_record(run, U.SUMS)


@pytest.mark.parametrize("n", [64, 65])
def test_the_auto_boundary(torch_cuda, oracle, n):
    """mvec = 3, SUMS_AUTO over {no transport, the hook, weights} x {a, u, h}: at 64 the reference-order kernel runs on the
    plain handle (the sequential sum's bits are asserted), installing the hook or weights flips AUTO to the rounded passes
    and removing them flips it back; at 65 the rounded passes run throughout.  A reference-order sum of 65 products lies well
    inside the fast bound, so what tells the kernels apart is split_update.assert_auto_boundary: under each of the plain
    handle (at 65), the hook and the weights (at 64 and 65) some red[0] is not the sequential sum's bits."""
    run = mixed_run(torch_cuda, oracle, f"auto-{n}", 2)
    assert M.pairs_met(run, keep_hook=True) == M.all_pairs(M.AUTO_NODES)
    assert_every_record(run, ("O", "R", "Rw") if n == 64 else ("R", "Rw"))
    assert run.hooked > 10
    U.assert_auto_boundary(run)


def test_the_long_list(torch_cuda, oracle):
    """n = 1031, mvec = 33, flavour 2: the balanced passes beyond 32, k_solve_rows<48>, the skip impossible."""
    run = mixed_run(torch_cuda, oracle, "long-list", 2)
    assert_the_sum_axis(run)
    assert run.widest == 33
    assert_every_record(run, U.SUMS)


# ---- the record (keep this test last) ------------------------------------------------------------------------------------------
def test_worst_ratios_and_times_of_the_module_are_printed(capsys):
    """Per way of forming the sums the worst |red - exact| / (u sum|xy|) the tests above saw and the K it was held to, and the
    wall time of every case: printed past the output capture, written beside the other records, and the ratios once more held
    to their K.  Selected on its own it has nothing to report."""
    import parity_util as P
    if not U.WORST:
        return
    with capsys.disabled():
        print("\n" + "\n".join(_report_lines()))
    rows = {way: {"worst_err_over_u_sum_abs": r[0], "k": r[1], "where": r[2]} for way, r in sorted(U.WORST.items())}
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "mode_changes_worst.json"), "w") as fh:
            json.dump({"worst": rows, "seconds": TIMES}, fh, indent=1, sort_keys=True)
    for way, (ratio, k, where) in U.WORST.items():
        assert ratio <= (k + 1) / (1.0 - (k + 1) * X.U), (way, ratio, k, where)      # gamma(k) / u
