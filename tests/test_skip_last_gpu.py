"""The skip of the last vector (nka_device.hpp, kSkipMay; diagnostic switch "skip_last"): two handles of the diagnostic build
in lock step on the same inputs, one with skip_last = 1 (skip wherever the launch allows it, at any length) and one with
skip_last = 0.  After every call they must agree to the bit in everything an update defines -- the returned f, the list and
the free list, h between listed slots, c of listed slots, the stored w and v of listed slots, num_vec, the host's bound on
the list -- and in red[] but for the two entries of a skipped vector, which read 0.

The sequences and their marks are tests/skip_last_seq.py's; tests/test_skip_last_cpu.py holds the marks against the oracle.
Here every update marked as a repair must raise the repair counter of the skipping handle, no other update may, and the mvec
updates behind a repair must run without the skip."""
import numpy as np
import pytest

import skip_last_seq as Q

pytestmark = pytest.mark.gpu

ROUNDED, BLOCKED = 3, 2              # nka_amd.SUMS_BLOCKED_ROUNDED (the default beyond 64 elements), nka_amd.SUMS_BLOCKED
SUMS = pytest.mark.parametrize("sums", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def size_for(mvec):
    """4099 = eight tiles and a ragged tail of three, 1031 = two tiles and a tail of seven (the longer lists: every listed slot
    is read back after every update)."""
    return 4099 if mvec <= 5 else 1031


class Pair:
    """The two handles and what they are held to."""

    def __init__(self, torch, n, mvec, flavor, sums, offset=0, prepare=None):
        import nka_amd
        assert nka_amd.SUMS_BLOCKED_ROUNDED == ROUNDED and nka_amd.SUMS_BLOCKED == BLOCKED
        self.torch, self.n, self.m = torch, n, mvec
        self.accs = []
        for skip in (1, 0):
            acc = nka_amd.nka(diagnostic=True).init(n, mvec, flavor=flavor).set_sum_order(sums)
            acc.set_tuning("skip_last", skip)
            if prepare:
                prepare(acc)
            self.accs.append(acc)
        # (offset = 1: an f that is 8 but not 16 bytes aligned)
        self.buf = [torch.empty(n + 2, dtype=torch.float64, device="cuda")[offset:offset + n] for _ in self.accs]
        self.calls = 0
        self.skipped = 0              # updates whose red[] showed the skip
        self.redo_at = []             # calls that raised the repair counter
        self.plain_after_redo = 0     # full-list updates that ran without the skip because a repair was recent

    def lists(self, acc):
        st = acc.state()
        return st, st.list_order(), st.free_order()

    def same_state(self, where, vectors=True, bound=True):
        a, b = self.accs
        (sa, la, fa), (sb, lb, fb) = self.lists(a), self.lists(b)
        assert la == lb and fa == fb, (where, la, lb, fa, fb)
        assert (sa.subspace, sa.pending) == (sb.subspace, sb.pending), where
        assert a.num_vec() == b.num_vec(), where
        assert not bound or a.list_bound() == b.list_bound(), where
        # h and c between listed slots: after an update the pending pair (la[0]) has no row yet
        ix = [k - 1 for k in la[1:]]
        assert np.array_equal(sa.h[np.ix_(ix, ix)], sb.h[np.ix_(ix, ix)]), where
        assert np.array_equal(sa.c[ix], sb.c[ix]), where
        if vectors:
            for k in la:
                assert np.array_equal(a.w(k), b.w(k)), (where, "w", k)
                assert np.array_equal(a.v(k), b.v(k)), (where, "v", k)

    def update(self, x, mark=None, check=True):
        torch, m = self.torch, self.m
        a, b = self.accs
        self.calls += 1
        where = (self.calls, mark)
        may, hold, pending_redo, nredo = a.skip_state()
        assert pending_redo == 0, where
        before = a.state().list_order() if check else None
        outs = []
        for acc, buf in zip(self.accs, self.buf):
            buf.copy_(torch.from_numpy(x))
            acc.accel_update(buf)
            if check:
                outs.append(buf.cpu().numpy())
        if not check:
            return
        assert np.array_equal(outs[0], outs[1]), (where, np.abs(outs[0] - outs[1]).max())
        self.same_state(where)
        after = a.state().list_order()
        removed = Q.removed_positions(before, after)
        if mark is not None:
            assert len(before) == m + 1 and removed == mark, (where, before, after)
        may2, hold2, pending2, nredo2 = a.skip_state()
        assert pending2 == 0 and b.skip_state()[3] == 0, where
        # the repair: taken exactly where the last vector's sums were needed at a full list with the skip planned
        full = len(before) == m + 1                             # (mvec + 1 entries: the first of them is a pending pair)
        needs = full and removed != [m]
        if nredo2 != nredo:
            assert nredo2 == nredo + 1 and needs and may == 1, (where, nredo, nredo2, removed)
            self.redo_at.append(self.calls)
            assert (may2, hold2) == (0, m), (where, may2, hold2)
        else:
            assert not (needs and may == 1 and self.skip_possible), (where, "the repair was not taken", removed)
            assert hold2 == max(hold - 1, 0) and may2 == (1 if hold2 == 0 else 0), (where, hold, hold2, may2)
        if Q.is_redo(mark, m) and self.skip_possible:
            assert nredo2 == nredo + 1, (where, "a marked update did not take the repair")
        # red[]: zero in the two entries of a skipped vector, the other handle's bits everywhere else
        if not before:                # (the first update after init / restart forms no sum: red[] is the previous update's)
            return
        ra, rb = a.reductions(), b.reductions()
        skipped = full and may == 1 and nredo2 == nredo and self.skip_possible
        if skipped:
            dead = [2 + m - 1, 2 + 2 * m - 1]
            assert ra[dead[0]] == 0.0 and ra[dead[1]] == 0.0, (where, ra[dead])
            assert rb[dead[1]] != 0.0, where
            live = np.ones(ra.size, bool)
            live[dead] = False
            assert np.array_equal(ra[live], rb[live]), where
            self.skipped += 1
        else:
            assert np.array_equal(ra, rb), (where, ra, rb)
            if full and may == 0:
                self.plain_after_redo += 1

    skip_possible = True              # (False: mvec = 33, a hook, an unaligned f -- the skipping handle must never skip)

    def run(self, ops):
        for op in ops:
            if op[0] == "update":
                self.update(op[1], op[2])
                continue
            for acc in self.accs:
                if op[0] == "relax":
                    acc.relax()
                elif op[0] == "restart":
                    acc.restart()
                else:
                    acc.set_vec_tol(op[1])
            self.same_state(op)
        return self


@SUMS
@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("mvec", [2, 3, 5, 20, 32])
def test_growth_then_capacity_drops(torch_cuda, mvec, flavor, sums):
    """Growth to the full list, then 2 mvec + 2 updates that drop for capacity: every one of them skips."""
    p = Pair(torch_cuda, size_for(mvec), mvec, flavor, sums).run(Q.sequence("capacity", size_for(mvec), mvec))
    assert p.skipped == 2 * mvec + 2 and not p.redo_at, (p.skipped, p.redo_at)


REDO = ([("newest", m, f) for m, f in ((2, 0), (3, 1), (5, 2), (20, 0))] + [("mid", m, f) for m, f in ((3, 2), (5, 0), (20, 1))] +
        [("multi", m, f) for m, f in ((3, 0), (5, 1), (5, 2))] + [("s0", m, f) for m, f in ((2, 1), (5, 0), (20, 2))])


@SUMS
@pytest.mark.parametrize("case,mvec,flavor", REDO)
def test_updates_that_need_the_last_vector_take_the_repair(torch_cuda, case, mvec, flavor, sums):
    """At a full list: the newest older entry dropped as dependent (the last vector kept), a mid-list entry dropped, several
    dropped with the last among them, s == 0.  One repair each, at the marked call, and the skip held off for the mvec
    updates behind it."""
    n = size_for(mvec)
    ops = Q.sequence(case, n, mvec)
    marked = [i for i, op in enumerate(o for o in ops if o[0] == "update") if Q.is_redo(op[2], mvec)]
    p = Pair(torch_cuda, n, mvec, flavor, sums).run(ops)
    assert p.redo_at == [marked[0] + 1] and len(marked) == 1, (p.redo_at, marked)
    assert p.accs[0].skip_state()[3] == 1
    if case != "multi":               # (full again at once: mvec capacity drops without the skip, then three with it)
        assert p.plain_after_redo == mvec and p.skipped == 2 + 3, (p.plain_after_redo, p.skipped)
    else:                             # (the list grows again while the skip is held off)
        assert p.plain_after_redo >= 1 and p.skipped > 2, (p.plain_after_redo, p.skipped)


@SUMS
@pytest.mark.parametrize("case", ["newest", "s0"])
def test_the_repair_in_a_weighted_metric(torch_cuda, case, sums):
    """Diagonal dot-product weights keep the skip: the repair launch is then the weighted form of the one-vector pass."""
    n, mvec = 4099, 5
    w = Q.weights(n)
    p = Pair(torch_cuda, n, mvec, 2, sums, prepare=lambda acc: acc.set_dot_weights(w)).run(Q.sequence(case, n, mvec))
    assert all(acc.dot_weighted() for acc in p.accs)
    assert p.redo_at == [mvec + 4] and p.plain_after_redo == mvec and p.skipped == 2 + 3, (p.redo_at, p.plain_after_redo, p.skipped)


@SUMS
@pytest.mark.parametrize("mvec", [3, 20])
def test_relax_and_restart_at_a_full_list(torch_cuda, mvec, sums):
    p = Pair(torch_cuda, size_for(mvec), mvec, 2, sums).run(Q.sequence("relax_restart", size_for(mvec), mvec))
    assert not p.redo_at and p.skipped == 6, (p.redo_at, p.skipped)


@SUMS
def test_a_host_that_never_synchronises(torch_cuda, sums):
    """No read-back between the updates: the host's bound on the list stays one too high behind the dependence drop, the
    launches stay as wide as the list can be, and the device alone decides where the skip holds."""
    torch, n, mvec = torch_cuda, 4099, 5
    ops = [op for op in Q.sequence("newest", n, mvec) if op[0] == "update"]
    p = Pair(torch, n, mvec, 0, sums)
    keep = [[torch.from_numpy(x).cuda() for _, x, _ in ops] for _ in p.accs]      # (every input is on the device beforehand)
    torch.cuda.synchronize()
    for t in range(len(ops)):
        for i, acc in enumerate(p.accs):
            acc.accel_update(keep[i][t])
    torch.cuda.synchronize()
    for t, (fa, fb) in enumerate(zip(*keep)):
        assert np.array_equal(fa.cpu().numpy(), fb.cpu().numpy()), t
    p.same_state("at the end")
    assert p.accs[0].skip_state()[3] == 1 and p.accs[1].skip_state()[3] == 0


def never_skips(torch, mvec, sums, n=1031, offset=0, prepare=None):
    p = Pair(torch, n, mvec, 2, sums, offset=offset, prepare=prepare)
    p.skip_possible = False
    p.run(Q.sequence("capacity", n, mvec)[:mvec + 5])
    assert p.skipped == 0 and not p.redo_at and p.calls == mvec + 5
    return p


@SUMS
def test_off_beyond_one_launch(torch_cuda, sums):
    never_skips(torch_cuda, 33, sums)


@SUMS
def test_off_with_an_allreduce_hook(torch_cuda, sums):
    """(a single-rank hook that leaves the sums as they are: the repair would need a conditional exchange)"""
    never_skips(torch_cuda, 5, sums, prepare=lambda acc: acc.set_dot_prod(lambda ptr, count, stream: None))


@SUMS
def test_off_with_an_unaligned_f(torch_cuda, sums):
    never_skips(torch_cuda, 5, sums, n=4099, offset=1)


@SUMS
@pytest.mark.parametrize("flavor", [0, 2])
def test_out_of_place_mixed_with_in_place(torch_cuda, flavor, sums):
    """Every other update hands its buffer over (nka_hip_accel_update_swap), the repair among them."""
    torch, n, mvec = torch_cuda, 4099, 5
    p = Pair(torch, n, mvec, flavor, sums)
    cur = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in p.accs]
    ops = [op for op in Q.sequence("mid", n, mvec) if op[0] == "update"]
    for t, (_, x, mark) in enumerate(ops):
        outs = []
        for i, acc in enumerate(p.accs):
            if t % 2 == 0:
                cur[i].copy_(torch.from_numpy(x))
                cur[i], out = acc.accel_update_swap(cur[i])
                outs.append(out.cpu().numpy())
            else:
                p.buf[i].copy_(torch.from_numpy(x))
                acc.accel_update(p.buf[i])
                outs.append(p.buf[i].cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), t
        p.same_state(t)
    marked = [t for t, op in enumerate(ops) if Q.is_redo(op[2], mvec)]
    assert len(marked) == 1 and marked[0] % 2 == 0          # (the repair falls on an out-of-place update)
    assert p.accs[0].skip_state()[3] == 1 and p.accs[1].skip_state()[3] == 0


@SUMS
def test_a_captured_update_carries_the_repair(torch_cuda, sums):
    """A steady-state update captured into a graph and replayed: three replays that skip, one whose input forces the repair,
    and the capacity drops behind it -- against the eager handle that never skips."""
    torch, n, mvec = torch_cuda, 4099, 5
    rng = np.random.default_rng(5)
    eager_until = mvec + 3            # (the list is full from update mvec + 2 on)
    X = list(rng.standard_normal((eager_until + 3, n)))      # ... and three replays that drop for capacity
    X.append(X[-1] + 0.7 * (X[-1] - X[-2]))                  # the recipe of "newest" (tests/skip_last_seq.py): the repair
    X += list(rng.standard_normal((mvec + 2, n)))
    p = Pair(torch, n, mvec, 0, sums)
    skipper, plain = p.accs
    want = []
    for x in X:
        p.buf[1].copy_(torch.from_numpy(x))
        plain.accel_update(p.buf[1])
        want.append(p.buf[1].cpu().numpy())
    side = torch.cuda.Stream()
    static = p.buf[0]
    got = []
    with torch.cuda.stream(side):
        for x in X[:eager_until]:
            static.copy_(torch.from_numpy(x))
            skipper.accel_update(static)
            got.append(static.cpu().numpy())
    torch.cuda.synchronize()
    assert skipper.capture_safe() and skipper.skip_state()[0] == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        skipper.accel_update(static)
    for t, x in enumerate(X[eager_until:]):
        static.copy_(torch.from_numpy(x))
        g.replay()
        torch.cuda.synchronize()
        got.append(static.cpu().numpy())
        assert skipper.skip_state()[3] == (0 if t < 3 else 1), t
    for t, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a, b), t
    p.same_state("behind the replays", bound=False)      # (a captured handle stops reading the list word)
