"""The call sequences of tests/skip_last_seq.py against the oracle, on the CPU: every marked update must find the list at
mvec + 1 entries and remove exactly the positions its mark names -- otherwise tests/test_skip_last_gpu.py could pass without
ever entering the repair path (or without ever skipping)."""
import numpy as np
import pytest

import skip_last_seq as Q

# (case, mvec) as the GPU tests use them; every flavour
GRID = ([("capacity", m) for m in (2, 3, 5, 20, 32)] + [("newest", m) for m in (2, 3, 5, 20)] +
        [("mid", m) for m in (3, 5, 20)] + [("multi", m) for m in (3, 5)] + [("s0", m) for m in (2, 5, 20)] +
        [("relax_restart", m) for m in (3, 20)] + [("capacity", 33)])


def walk(oracle, case, n, mvec, flavor, weighted=False):
    """The oracle through the sequence; per marked update (full at entry?, positions removed)."""
    ora = oracle.OracleNKA(n, mvec, flavor)
    if weighted:
        w = Q.weights(n)
        ora.set_dot_prod(lambda x, y: float(np.dot(w * x, y)))
    seen = []
    for op in Q.sequence(case, n, mvec):
        if op[0] == "relax":
            ora.relax()
        elif op[0] == "restart":
            ora.restart()
        elif op[0] == "vtol":
            ora.set_vec_tol(op[1])
        else:
            before = ora.state().list_order()
            ora.accel_update(op[1].copy())
            after = ora.state().list_order()
            if op[2] is not None:
                seen.append((op[2], len(before), Q.removed_positions(before, after)))
    return seen


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("case,mvec", GRID)
def test_marked_updates_find_a_full_list_and_take_the_named_drops(oracle, case, mvec, flavor):
    for n in (1031, 4099):
        seen = walk(oracle, case, n, mvec, flavor)
        assert seen, (case, mvec)
        for mark, length, removed in seen:
            assert length == mvec + 1, (case, mvec, n, mark, length)
            assert removed == mark, (case, mvec, n, mark, removed)
        redo = [mark for mark, _, _ in seen if Q.is_redo(mark, mvec)]
        assert len(redo) == (0 if case in ("capacity", "relax_restart") else 1), (case, mvec, redo)
        assert sum(1 for mark, _, _ in seen if mark == [mvec]) >= 2, (case, mvec)


@pytest.mark.parametrize("case", ["newest", "s0"])
def test_marked_updates_in_a_weighted_metric(oracle, case):
    """(the weighted cases of the GPU test: n = 4099, mvec = 5, compact flavour)"""
    seen = walk(oracle, case, 4099, 5, 2, weighted=True)
    assert all(length == 6 and removed == mark for mark, length, removed in seen), seen
    assert sum(1 for mark, _, _ in seen if Q.is_redo(mark, 5)) == 1 and len(seen) == 2 + 1 + 8


def test_the_marks_say_what_they_are_meant_to():
    assert not Q.is_redo([5], 5) and not Q.is_redo(None, 5)
    assert Q.is_redo([1], 5) and Q.is_redo([0], 5) and Q.is_redo([1, 3, 5], 5) and Q.is_redo([2], 3)
    assert Q.removed_positions([7, 3, 4, 1], [2, 7, 4]) == [1, 3]
    assert np.array_equal(Q.sequence("s0", 64, 3)[5][1], Q.sequence("s0", 64, 3)[6][1])
