"""The scalar step and the elementwise statements of the lone array handle, held exactly in both fast sum modes
(tests/split_update.py: parts 2 and 3 of an update; part 1, the sums, is tests/test_sums_exact_gpu.py).

The scalar step: every k_solve_rows<NLMAX> instance and both one-lane forms of k_solve, the three branches of solve_nrm (the
sums as they are in SUMS_BLOCKED_ROUNDED, red / s and fl(1/s) * red in SUMS_BLOCKED), capacity and dependence drops, close
calls of the drop rule, s == 0, relax, restart, set_vec_tol, the slot tables loaded after an out-of-place update.
The combine against numpy: every width of the automatic choice, in passes of 32 beyond a list of 32, in passes of four from
an unaligned f, more than one tile per block with and without dead ring slots, the window kernel forced for the flavours
that never get it by themselves, tickets and double-width tiles, and out of place.

G = the device's CU count, t = 512 elements (one tile)."""
import numpy as np
import pytest

import batch_seq as B
import scenarios as S
import split_update as U

pytestmark = pytest.mark.gpu

ROUNDED, BLOCKED = U.SUMS_BLOCKED_ROUNDED, U.SUMS_BLOCKED             # (the default first)
MODES = pytest.mark.parametrize("mode", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])
FLAVORS = pytest.mark.parametrize("flavor", [0, 1, 2])
TILE = 512


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ncu(torch_cuda):
    import nka_amd
    acc = nka_amd.nka().init(1, 1)
    _, g = acc.device_info()
    acc.delete()
    assert g >= 1
    return g


def split_run(torch, oracle, flavor, n, mvec, mode, aligned=True, swap=False, **tuning):
    """A fresh handle (the diagnostic build's if a kernel form is forced: it is built from the product's objects) in a SplitRun."""
    import nka_amd
    acc = nka_amd.nka(diagnostic=bool(tuning)).init(n, mvec, flavor=flavor)
    for key, value in tuning.items():
        acc.set_tuning(key, value)
    return U.SplitRun(torch, oracle, acc, flavor, n, mvec, mode, aligned=aligned, swap=swap, check_sums=False)


def affine_of_stored(inputs):
    """A combination of three stored inputs whose coefficients sum to 1: its difference from the newest input lies in the span
    of the stored differences, so the update drops the oldest of the four entries involved (a mid-list entry)."""
    return 0.5 * inputs[-1] + 0.3 * inputs[-3] + 0.2 * inputs[-5]


# ---- every k_solve_rows instance and both one-lane forms -------------------------------------------------------------------
TURN = 8                                     # the updates of grow_and_turn behind the fresh ones


def in_the_span_of_two_stored(run):
    """An input whose difference from the pending pair's lies in the span of the two newest older entries (the mirror's w, equal
    parts of each): the update keeps the newer of the two (pivot^2 = 1/2) and drops the older one at the default tolerance,
    with whatever is stored behind it staying -- a mid-list entry."""
    pending, newer, older = run.acc.state().list_order()[:3]
    return run.W[pending] - np.sqrt(run.n) * (run.W[newer] + run.W[older])


def grow_and_turn(run, seed, fresh):
    """`fresh` fresh inputs (mvec + 1 fill the list, two more drop by capacity); a repeated input (s == 0); relax and an update;
    then the dependence drops on the widest list: a further fresh input, so that the stored differences are again those of
    consecutive inputs, each at 120 degrees to its neighbours and at a right angle to the rest (pivot^2 = 0.75 +- 0.05 in 400
    dimensions and more); the tolerance raised to 0.95 (0.9025 squared) and two fresh inputs, the first of which drops the
    newest older entry and every second one behind it (three and more from five older entries on), the second the newest
    alone; the default tolerance again and in_the_span_of_two_stored; at last restart and two updates."""
    rng = np.random.default_rng(seed)
    vtol = run.ora.vec_tol()
    for _ in range(fresh):
        x = rng.standard_normal(run.n)
        run.update(x)
    run.update(x.copy())
    run.relax()
    run.update(rng.standard_normal(run.n))
    run.update(rng.standard_normal(run.n))
    run.set_vec_tol(0.95)
    for _ in range(2):
        run.update(rng.standard_normal(run.n))
    run.set_vec_tol(vtol)
    run.update(in_the_span_of_two_stored(run))
    run.restart()
    for _ in range(2):
        run.update(rng.standard_normal(run.n))
    assert run.calls == fresh + TURN
    return run.finish()


def assert_grown_and_turned(run, fresh):
    """What grow_and_turn is there to meet.  `top`, `widest`: the older counts at the entry of the repeated input and of the
    first update under the raised tolerance: mvec both, or fresh - 1 and fresh where the run is cut short of a full list."""
    top, widest = min(run.m, fresh - 1), min(run.m, fresh)
    assert run.zero_s and run.after_relax and run.after_restart
    assert {c for c, _ in run.ncomb} == set(range(widest + 1)), run.ncomb
    assert run.nolder_pending == set(range(widest + 1)), run.nolder_pending
    assert run.nolder_no_pending == {0, top}, run.nolder_no_pending             # after init / restart; after relax
    assert {(0, False), (1, True), (widest, True), (top, False)} <= run.ncomb, run.ncomb
    # the dependence drops.  The raised tolerance takes the newest older entry and every second one behind it (far down a long
    # list at n = 400 the small angles to the many kept entries add up and more go: the head of the list is asserted) ...
    gone = dict(run.outcomes)
    raised = fresh + 3
    assert gone[raised][:3] == [0, 2, 4] and 1 not in gone[raised] and 3 not in gone[raised], (raised, gone[raised])
    assert gone[raised + 1][:1] == [0], (raised + 1, gone[raised + 1])         # ... then the newest alone
    assert gone[raised + 2] == [1], (raised + 2, gone[raised + 2])             # in_the_span_of_two_stored: the older of the two
    assert run.dropped_mid and run.dropped_newest and run.dropped_at_once >= {1, 3}, run.dropped_at_once
    capacity = [call for call, went in run.outcomes if went == [run.m - 1]]
    if widest == run.m:
        assert top == run.m and run.full_at_entry and run.capacity_drop
        assert capacity == [run.m + 1, run.m + 2, fresh + 2], capacity          # the inputs beyond the full list
    else:
        assert not run.full_at_entry and not capacity


@MODES
@pytest.mark.parametrize("mvec", [5, 6, 10, 11, 20, 21, 32, 33, 47, 48, 62, 63])
def test_scalar_step_and_statements_in_every_solve_instance(torch_cuda, oracle, mvec, mode):
    """mvec + 1 = 6 | 7, 11 | 12, 21 | 22, 33 | 34, 48 | 49 straddle the k_solve_rows instances 6, 11, 21, 33, 48 and 63; mvec = 63
    is the first subspace of the one-lane k_solve in LDS; from mvec = 21 on the matrix is loaded in the old loop beyond the
    first 8 * 64 entries."""
    for flavor in (0, 1, 2):
        run = grow_and_turn(split_run(torch_cuda, oracle, flavor, 700, mvec, mode), 700 + mvec, fresh=mvec + 3)
        assert_grown_and_turned(run, mvec + 3)


@MODES
@FLAVORS
@pytest.mark.parametrize("mvec", [140, 141])
def test_scalar_step_and_statements_in_the_one_lane_solves(torch_cuda, oracle, mvec, flavor, mode):
    """mvec = 140: the last subspace of k_solve in LDS; 141: the first in global memory, cut to 34 updates (it is slow): its
    list reaches 26 older entries, of which the raised tolerance drops every second one."""
    fresh = mvec + 3 if mvec == 140 else 34 - TURN
    run = grow_and_turn(split_run(torch_cuda, oracle, flavor, 400, mvec, mode), 400 + mvec, fresh=fresh)
    assert_grown_and_turned(run, fresh)


@MODES
def test_scalar_step_and_statements_with_the_serial_solve_forced(torch_cuda, oracle, mode):
    """k_solve on one lane where the automatic choice takes k_solve_rows<21>."""
    for flavor in (0, 1, 2):
        run = grow_and_turn(split_run(torch_cuda, oracle, flavor, 700, 20, mode, serial_solve=1), 720, fresh=23)
        assert_grown_and_turned(run, 23)


# ---- drops and close calls ----------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("mvec", [1, 10, 32])
def test_drops_by_capacity_and_by_dependence(torch_cuda, oracle, mvec, mode):
    """batch_seq.Sequence: fresh, dependent, repeated and zero inputs; mvec = 1 drops by capacity in every update."""
    n = 65
    for flavor in (0, 1, 2):
        run = split_run(torch_cuda, oracle, flavor, n, mvec, mode)
        seq = B.Sequence(n, 65001 + 37 * mvec)
        for _ in range(2 * mvec + 16):
            run.update(seq.next())
        run.finish()
        assert run.full_at_entry and run.capacity_drop and run.zero_s and 1 in run.dropped_at_once
        assert run.dropped_newest if mvec == 1 else run.dropped_mid


@MODES
def test_several_entries_dropped_at_once(torch_cuda, oracle, mode):
    """A tolerance raised on a grown list.  Stored differences of consecutive fresh inputs make an angle of 120 degrees with
    their neighbours (pivot^2 = 0.75 against vtol^2 = 0.9025, +- 0.04 in 700 dimensions) and a right angle with the rest: the
    next update drops the newest older entry and every second one behind it."""
    n, mvec = 700, 10
    for flavor in (0, 1, 2):
        run = split_run(torch_cuda, oracle, flavor, n, mvec, mode)
        rng = np.random.default_rng(7)
        for t in range(mvec + 2):
            if t == mvec:
                run.set_vec_tol(0.95)
            run.update(rng.standard_normal(n))
        run.finish()
        assert 3 in run.dropped_at_once and run.dropped_newest and run.dropped_mid, run.outcomes


@MODES
@pytest.mark.parametrize("mvec", B.NEAR_MVECS)
@pytest.mark.parametrize("vlen", B.NEAR_VLENS)
def test_close_calls_of_the_drop_rule(torch_cuda, oracle, vlen, mvec, mode):
    """batch_seq.NearThreshold puts the newest older pair at an angle of about vtol to the normalised one: whichever way the
    device's sums decide, the oracle's scalar step on those sums decides the same; over the seeds of the shape (guarded on
    the CPU by tests/test_exact_sums_cpu.py) at least one close call drops the pair in question and one keeps it."""
    for flavor in (0, 1, 2):
        dropped = kept = 0
        for seed in B.near_seeds(vlen, mvec):
            run = split_run(torch_cuda, oracle, flavor, vlen, mvec, mode)
            seq = B.NearThreshold(vlen, seed)
            near_calls = set()
            for t in range(B.NEAR_CALLS):
                x, near = seq.next()
                if near:
                    near_calls.add(t)
                run.update(x)
            run.finish()
            went = {t for t, gone in run.outcomes if gone and gone[0] == 0}        # the newest older entry went
            dropped += len(near_calls & went)
            kept += len(near_calls - went)
        assert dropped and kept, (flavor, dropped, kept)


@MODES
@pytest.mark.parametrize("name", S.scenario_names())
def test_golden_scenarios(torch_cuda, oracle, name, mode):
    """The state machines of the fixtures, their relax, restart and set_vec_tol included (n = 64 and 7: the fast sums are set
    explicitly)."""
    g = S.load(name)
    n, m = int(g["n"]), int(g["mvec"])
    for flavor in (0, 1, 2):
        run = split_run(torch_cuda, oracle, flavor, n, m, mode)
        for op, idx, val in g["ops"]:
            op = int(op)
            if op == S.OP_UPDATE:
                run.update(g["inputs"][int(idx)].copy())
            elif op == S.OP_RESTART:
                run.restart()
            elif op == S.OP_RELAX:
                run.relax()
            elif op == S.OP_SET_VEC_TOL:
                run.set_vec_tol(float(val))
            assert run.acc.num_vec() == run.ora.num_vec()
        run.finish()


# ---- every PB width against numpy ---------------------------------------------------------------------------------------------
def every_width_then_a_dependent_input(run, seed):
    """mvec + 2 fresh inputs (len(comb) = 0..mvec, then the capacity drop), then a combination of three stored inputs: an update
    with dead ring slots."""
    rng = np.random.default_rng(seed)
    inputs = []
    for _ in range(run.m + 2):
        inputs.append(rng.standard_normal(run.n))
        run.update(inputs[-1])
    assert {c for c, _ in run.ncomb} == set(range(run.m + 1)) and run.capacity_drop, run.ncomb
    assert not run.dropped_mid
    run.update(affine_of_stored(inputs))
    assert run.dropped_mid and run.outcomes[-1][1] == [3], run.outcomes[-1]
    return run.finish()


def two_or_three_tiles(ncu):
    return 2 * ncu * TILE + TILE + 77


@MODES
@FLAVORS
@pytest.mark.parametrize("mvec,aligned", [(32, True), (64, True), (10, False)], ids=["m32", "m64", "m10-unaligned"])
def test_every_combine_width_of_the_automatic_choice(torch_cuda, oracle, mvec, aligned, flavor, mode):
    """n = 4099.  mvec = 32: every list width of one pass; 64: the passes of a list longer than 32, in place; 10 from a buffer
    8 bytes off a 16-byte boundary: the scalar path, one to three passes of four."""
    run = split_run(torch_cuda, oracle, flavor, 4099, mvec, mode, aligned=aligned)
    every_width_then_a_dependent_input(run, 4099 + mvec)


@MODES
@FLAVORS
def test_every_combine_width_with_several_tiles_a_block(torch_cuda, oracle, ncu, flavor, mode):
    """n = 2 G t + t + 77: blocks own two or three tiles plus the tail block, so the ring refills across tiles."""
    run = split_run(torch_cuda, oracle, flavor, two_or_three_tiles(ncu), 32, mode)
    every_width_then_a_dependent_input(run, 32)


# ---- the forced forms -----------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("flavor", [0, 1])
@pytest.mark.parametrize("large", [False, True], ids=["4099", "2Gt+t+77"])
def test_every_combine_width_of_the_window_kernel_forced(torch_cuda, oracle, ncu, large, flavor, mode):
    """The automatic rule never picks the window kernel for the flavours 0 and 1 at a size a test can run."""
    n = two_or_three_tiles(ncu) if large else 4099
    run = split_run(torch_cuda, oracle, flavor, n, 32, mode, pb_pipe=201)
    every_width_then_a_dependent_input(run, 201)


@MODES
def test_every_combine_width_of_the_window_kernel_two_blocks_a_cu(torch_cuda, oracle, ncu, mode):
    """pb_pipe = 202: the window kernel with two blocks a CU."""
    run = split_run(torch_cuda, oracle, 1, two_or_three_tiles(ncu), 32, mode, pb_pipe=202)
    every_width_then_a_dependent_input(run, 202)


@MODES
@FLAVORS
@pytest.mark.parametrize("tickets,tile", [(1, 1), (2, 1), (1, 2), (2, 2), (-1, -1)])
def test_tickets_and_double_width_tiles(torch_cuda, oracle, ncu, tickets, tile, flavor, mode):
    """n = 5 G t + 77, mvec = 6: the window kernel with its tiles handed out by tickets and with T = 2, through the growth, a
    dependent input, a repeated input, relax and restart.

    What the switches reach (launch_combine_win_k, launch_combine_win_1): pb_tile = 2 gives T = 2 only where a tile carries at
    most 14 words per element, that is for lists of 1 to 4 pairs in the flavours 0 and 1 (2 K + 6 words) and for all of 1
    to 6 in flavour 2 (K + 7 words); the wider lists of this sweep run T = 1 under the same setting.  pb_tickets = 2 takes
    two counters only if the grid divides by 2, otherwise the static mapping without a word: the grid here is G blocks
    (one a CU, 5 G tiles of t, or 2.5 G of 2 t, to share), so G has to be even, which is asserted.  (-1, -1) is the automatic
    choice: static mapping and T = 1 below 64 G tiles."""
    n, mvec = 5 * ncu * TILE + 77, 6
    assert tickets != 2 or ncu % 2 == 0, "two ticket counters need an even number of blocks"
    run = split_run(torch_cuda, oracle, flavor, n, mvec, mode, pb_pipe=201, pb_tickets=tickets, pb_tile=tile)
    rng = np.random.default_rng(77)
    inputs = []
    for _ in range(mvec + 2):
        inputs.append(rng.standard_normal(n))
        run.update(inputs[-1])
    x = affine_of_stored(inputs)
    run.update(x)
    run.update(x.copy())
    run.relax()
    run.update(rng.standard_normal(n))
    run.restart()
    for _ in range(2):
        run.update(rng.standard_normal(n))
    run.finish()
    assert run.capacity_drop and run.dropped_mid and run.zero_s and run.after_relax and run.after_restart
    assert {c for c, _ in run.ncomb} == set(range(mvec + 1)), run.ncomb


# ---- out of place -----------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("flavor", [0, 2])
@pytest.mark.parametrize("n,mvec", [(513, 3), (4099, 20), (4099, 40)])
def test_out_of_place_updates(torch_cuda, oracle, n, mvec, flavor, mode):
    """accel_update_swap: the caller's buffer keeps f_in, v_new holds f_out, the buffer handed back carries f's bits, and the
    scalar step runs with loaded slot tables.  mvec = 40: the passes of 32 with the running value in v_new.  Once the list is
    full, in-place and out-of-place calls alternate, and a dependent input leaves dead slots."""
    run = split_run(torch_cuda, oracle, flavor, n, mvec, mode, swap=True)
    rng = np.random.default_rng(n + mvec)
    inputs = []
    for _ in range(mvec + 2):
        inputs.append(rng.standard_normal(n))
        run.update(inputs[-1])
    assert {c for c, _ in run.ncomb} == set(range(mvec + 1)) and run.capacity_drop, run.ncomb
    for t in range(6):
        inputs.append(rng.standard_normal(n))
        run.update(inputs[-1], swap=bool(t % 2))
    if mvec >= 5:
        run.update(affine_of_stored(inputs))
        assert run.dropped_mid
    run.finish()


# ---- NaN / Inf ----------------------------------------------------------------------------------------------------------------------
@MODES
@FLAVORS
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_input(torch_cuda, oracle, bad, flavor, mode):
    """A NaN / an Inf in one element: parts 2 and 3 on the update that sees it and the three after it."""
    n, mvec = 1000, 3
    run = split_run(torch_cuda, oracle, flavor, n, mvec, mode)
    rng = np.random.default_rng(11)
    for t in range(7):
        x = rng.standard_normal(n)
        if t == 3:
            x[5] = bad
        out = run.update(x)
    run.finish()
    assert np.isnan(out).any()
