"""The deferred v of the pending pair (k_combine_win, DEFER; diagnostic switch "defer_v"): two handles of the diagnostic build in
lock step on the same inputs, one with defer_v = 1 (PB leaves the accelerated f unstored in the new pair's v wherever the launch
allows it, the next PB forms it again from the vectors it streams) and its twin with defer_v = 0.  After every call they must
agree to the bit in the returned f, in state() -- every word of it, and the digest -- and in the stored w and v.

Reading the v of the pending pair writes it (k_materialise_v) and the next combine then finds it in memory, so every sequence
runs in two ways: peek = "all" reads w and v of every listed slot after every update -- each update defers, each look
materialises -- and peek = "lazy" leaves the pending pair's v alone until the end: each combine replays it, and what it formed
is checked one update later, in the u' = v' - w' it stored for that pair, and through every f it is combined into.

n = 1031 = two tiles of 512 and a ragged tail of seven with the ticketed rolling-window PB forced at that length (pb_pipe = 201,
pb_tickets = 1); the short lists also with the tile of 1024 they take at long vectors (pb_tile = 2, n = 2055).  The sequences
are tests/skip_last_seq.py's: growth to the full list and capacity drops, dependence drops at a full list (with the skip of the
last vector on, so that the repair's second scalar step writes the replay plan), a repeated input, relax and restart."""
import numpy as np
import pytest

import parity_util as P
import scenarios as S
import skip_last_seq as Q

pytestmark = pytest.mark.gpu

ROUNDED, BLOCKED = 3, 2              # nka_amd.SUMS_BLOCKED_ROUNDED (the default), nka_amd.SUMS_BLOCKED
C_FLAVOR = 2                         # compact storage: the only flavour that defers
SHAPES = [(2, 1), (2, 2), (5, 1), (5, 2), (20, 1)]      # (mvec, pb_tile)
PEEK = pytest.mark.parametrize("peek", ["all", "lazy"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def size_for(tile):
    return 1031 if tile == 1 else 2055


def tuned(acc, defer, tile=1, skip_last=0):
    acc.set_tuning("pb_pipe", 201)
    acc.set_tuning("pb_tickets", 1)
    acc.set_tuning("pb_tile", tile)
    acc.set_tuning("skip_last", skip_last)
    acc.set_tuning("defer_v", defer)
    return acc


def bits(x):
    return np.ascontiguousarray(x).tobytes()


class Twins:
    def __init__(self, torch, n, mvec, tile=1, sums=ROUNDED, peek="lazy", skip_last=0, prepare=None, flavor=C_FLAVOR):
        import nka_amd
        assert nka_amd.SUMS_BLOCKED_ROUNDED == ROUNDED and nka_amd.SUMS_BLOCKED == BLOCKED
        self.torch, self.n, self.m, self.peek = torch, n, mvec, peek
        self.accs = []
        for defer in (1, 0):
            acc = tuned(nka_amd.nka(diagnostic=True).init(n, mvec, flavor=flavor).set_sum_order(sums), defer, tile, skip_last)
            if prepare:
                prepare(acc)
            self.accs.append(acc)
        self.buf = [torch.empty(n + 2, dtype=torch.float64, device="cuda") for _ in self.accs]
        self.calls = 0
        self.deferred = 0             # updates that left the word raised
        self.replayed = []            # entries replayed, per update that did
        self.may_defer = True         # (False: the deferring handle must never defer)

    def same_state(self, where, pending_v=None, bound=True):
        a, b = self.accs
        sa, sb = a.state(), b.state()
        assert (sa.subspace, sa.pending, sa.first, sa.last, sa.free) == (sb.subspace, sb.pending, sb.first, sb.last, sb.free), where
        for name in ("next", "prev", "h", "c"):
            assert bits(getattr(sa, name)) == bits(getattr(sb, name)), (where, name)
        assert a.state_digest() == b.state_digest(), where
        assert a.num_vec() == b.num_vec(), where
        assert not bound or a.list_bound() == b.list_bound(), where
        assert bits(a.reductions()) == bits(b.reductions()), where
        order = sa.list_order()
        if pending_v is None:
            pending_v = self.peek == "all"
        for k in order:
            assert bits(a.w(k)) == bits(b.w(k)), (where, "w", k)
            if pending_v or not (sa.pending and k == sa.first):
                assert bits(a.v(k)) == bits(b.v(k)), (where, "v", k)
        return sa

    def update(self, x, offset=0, check=True):
        torch = self.torch
        a, b = self.accs
        self.calls += 1
        where = self.calls
        before = a.state()
        word_before = a.defer_state()[0]
        outs = []
        for acc, buf in zip(self.accs, self.buf):
            view = buf[offset:offset + self.n]
            view.copy_(torch.from_numpy(x))
            acc.accel_update(view)
            outs.append(view.cpu().numpy())
        assert bits(outs[0]) == bits(outs[1]), (where, np.abs(outs[0] - outs[1]).max())
        word, nrep = a.defer_state()
        assert b.defer_state()[0] == 0, where
        if not self.may_defer or offset:
            assert word == 0, where
        else:
            # the device defers wherever a combine happened, and replays wherever it finds the word and a pair to normalise
            combined = a.state().subspace
            assert word == (1 if combined else 0), (where, word)
            s0 = before.pending and a.reductions()[0] == 0.0
            want = len(before.list_order()) - 1 if (word_before and before.pending and not s0) else 0
            assert nrep == want, (where, nrep, want)
            if nrep:
                self.replayed.append(nrep)
        self.deferred += word
        if check:
            self.same_state(where)
        return outs[0]

    def run(self, ops):
        for op in ops:
            if op[0] == "update":
                self.update(op[1])
                continue
            for acc in self.accs:
                if op[0] == "relax":
                    acc.relax()
                elif op[0] == "restart":
                    acc.restart()
                else:
                    acc.set_vec_tol(op[1])
            assert self.accs[0].defer_state()[0] == 0 or op[0] == "vtol", op[0]
            self.same_state(op[0])
        self.same_state("at the end", pending_v=True)
        assert self.accs[0].defer_state()[0] == 0            # (that look has written the v and cleared the word)
        return self


@PEEK
@pytest.mark.parametrize("sums", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])
@pytest.mark.parametrize("mvec,tile", SHAPES)
def test_a_list_that_fills_and_a_full_one(torch_cuda, mvec, tile, sums, peek):
    """Growth to mvec + 1 entries (each replay one entry longer, one dead ring slot), then 2 mvec + 2 capacity drops (the
    replay reads the dropped vector in place of v)."""
    n = size_for(tile)
    p = Twins(torch_cuda, n, mvec, tile, sums, peek).run(Q.sequence("capacity", n, mvec))
    assert p.deferred == p.calls - 1                           # every update but the first combines
    if peek == "lazy":
        assert p.replayed == list(range(1, mvec)) + [mvec] * (p.calls - mvec - 1), p.replayed
    else:
        assert p.replayed == []


DROPS = [("newest", 2, 1), ("newest", 5, 2), ("newest", 20, 1), ("mid", 5, 1), ("mid", 20, 1), ("multi", 5, 1), ("multi", 5, 2),
         ("s0", 2, 2), ("s0", 5, 1), ("s0", 20, 1)]


@PEEK
@pytest.mark.parametrize("case,mvec,tile", DROPS)
def test_dependence_drops_and_a_repeated_input_at_a_full_list(torch_cuda, case, mvec, tile, peek):
    """A dropped entry is replayed into v and skipped in f; with the skip of the last vector on, the update that drops takes the
    repair and its second scalar step writes the plan; s == 0 drops the pair whose v was deferred and clears the word."""
    n = size_for(tile)
    p = Twins(torch_cuda, n, mvec, tile, ROUNDED, peek, skip_last=1).run(Q.sequence(case, n, mvec))
    assert all(acc.skip_state()[3] == 1 for acc in p.accs)     # (one repair each)
    assert p.deferred == p.calls - 1


@PEEK
@pytest.mark.parametrize("mvec", [5, 20])
def test_inputs_confined_to_a_low_dimensional_span(torch_cuda, mvec, peek):
    """Every input lies in a span of three vectors: dependence drops while the list is still filling, in update after update."""
    n = 1031
    rng = np.random.default_rng(mvec)
    basis = rng.standard_normal((3, n))
    p = Twins(torch_cuda, n, mvec, 1, ROUNDED, peek)
    p.run([("update", rng.standard_normal(3) @ basis, None) for _ in range(mvec + 4)])
    assert p.accs[0].num_vec() < mvec and p.deferred == p.calls - 1


@PEEK
@pytest.mark.parametrize("mvec", [2, 5, 20])
def test_relax_and_restart_between_updates(torch_cuda, mvec, peek):
    Twins(torch_cuda, 1031, mvec, 1, BLOCKED, peek).run(Q.sequence("relax_restart", 1031, mvec))


@pytest.mark.parametrize("mvec", [2, 5, 20])
def test_get_v_of_the_pending_slot_mid_sequence(torch_cuda, mvec):
    """v of the pending pair is the accelerated f, whenever it is asked for; the update behind the look reads it from memory."""
    n = 1031
    p = Twins(torch_cuda, n, mvec)
    for t, op in enumerate(Q.sequence("capacity", n, mvec)[:mvec + 6]):
        out = p.update(op[1])
        if t % 3 == 2:
            a = p.accs[0]
            assert a.defer_state()[0] == 1
            assert bits(a.v(a.state().first)) == bits(out), t
            assert a.defer_state()[0] == 0
            assert bits(a.v(a.state().first)) == bits(out), t
    p.same_state("at the end", pending_v=True)
    assert len(p.replayed) == p.calls - 2 - (p.calls - 1) // 3


@pytest.mark.parametrize("mvec", [5, 20])
def test_clone_mid_sequence_and_both_copies_continue(torch_cuda, mvec):
    torch, n = torch_cuda, 1031
    ops = Q.sequence("capacity", n, mvec)
    p = Twins(torch, n, mvec)
    for op in ops[:mvec + 3]:
        p.update(op[1])
    assert p.accs[0].defer_state()[0] == 1
    q = Twins(torch, n, mvec)
    for acc in q.accs:
        acc.delete()
    q.accs = [acc.copy() for acc in p.accs]                    # (the copy takes the vectors as they lie: the word is cleared)
    q.calls = p.calls
    assert p.accs[0].defer_state()[0] == 0 and q.accs[0].defer_state()[0] == 0
    for pair in (p, q):
        pair.same_state("behind the copy", pending_v=True)
    outs = []
    for pair in (p, q):
        outs.append([pair.update(op[1]) for op in ops[mvec + 3:mvec + 8]])
        pair.same_state("at the end", pending_v=True)
    assert all(bits(x) == bits(y) for x, y in zip(*outs))
    assert len(q.replayed) == 4                                # (the copy defers like the original)


def test_the_out_of_place_entry_and_back(torch_cuda):
    """Every third update hands its buffer over (nka_hip_accel_update_swap): it materialises first and never defers."""
    torch, n, mvec = torch_cuda, 1031, 5
    p = Twins(torch, n, mvec)
    cur = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in p.accs]
    for t, op in enumerate(Q.sequence("capacity", n, mvec)[:mvec + 8]):
        if t % 3 != 2:
            p.update(op[1])
            continue
        outs = []
        for i, acc in enumerate(p.accs):
            cur[i].copy_(torch.from_numpy(op[1]))
            cur[i], out = acc.accel_update_swap(cur[i])
            outs.append(out.cpu().numpy())
        assert bits(outs[0]) == bits(outs[1]), t
        assert p.accs[0].defer_state()[0] == 0, t
        p.same_state(t, pending_v=True)
    p.same_state("at the end", pending_v=True)
    assert p.replayed and p.deferred


def test_one_unaligned_f(torch_cuda):
    """An f that is 8 but not 16 bytes aligned takes the scalar PB: it materialises first, does not defer, and the aligned
    update behind it defers again."""
    n, mvec = 1031, 5
    p = Twins(torch_cuda, n, mvec)
    for t, op in enumerate(Q.sequence("capacity", n, mvec)[:mvec + 6]):
        p.update(op[1], offset=1 if t == mvec + 2 else 0)
    p.same_state("at the end", pending_v=True)
    assert p.deferred == p.calls - 2 and len(p.replayed) == p.calls - 4


@PEEK
@pytest.mark.parametrize("sums", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])
def test_diagonal_dot_weights(torch_cuda, sums, peek):
    n, mvec = 1031, 5
    w = Q.weights(n)
    p = Twins(torch_cuda, n, mvec, 1, sums, peek, skip_last=1, prepare=lambda acc: acc.set_dot_weights(w))
    p.run(Q.sequence("newest", n, mvec))
    assert all(acc.dot_weighted() for acc in p.accs) and p.deferred == p.calls - 1


def test_a_captured_update_does_not_defer(torch_cuda):
    """The eager updates defer; the captured one starts with the guarded launches that write a deferred v, and neither it nor
    anything behind it on that handle defers again."""
    torch, n, mvec = torch_cuda, 1031, 5
    rng = np.random.default_rng(11)
    X = list(rng.standard_normal((mvec + 9, n)))
    p = Twins(torch, n, mvec)
    deferring, plain = p.accs
    want = []
    for x in X:
        p.buf[1][:n].copy_(torch.from_numpy(x))
        plain.accel_update(p.buf[1][:n])
        want.append(p.buf[1][:n].cpu().numpy())
    side = torch.cuda.Stream()
    static = p.buf[0][:n]
    got = []
    with torch.cuda.stream(side):
        for x in X[:mvec + 3]:
            static.copy_(torch.from_numpy(x))
            deferring.accel_update(static)
            got.append(static.cpu().numpy())
    torch.cuda.synchronize()
    assert deferring.capture_safe() and deferring.defer_state()[0] == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        deferring.accel_update(static)
    for x in X[mvec + 3:mvec + 6]:
        static.copy_(torch.from_numpy(x))
        g.replay()
        torch.cuda.synchronize()
        got.append(static.cpu().numpy())
        assert deferring.defer_state()[0] == 0
    with torch.cuda.stream(side):
        for x in X[mvec + 6:]:
            static.copy_(torch.from_numpy(x))
            deferring.accel_update(static)
            got.append(static.cpu().numpy())
            assert deferring.defer_state()[0] == 0
    for t, (a, b) in enumerate(zip(want, got)):
        assert bits(a) == bits(b), t
    p.same_state("behind the replays", pending_v=True, bound=False)


def test_flavours_and_lists_that_cannot_defer(torch_cuda):
    """The two-vector flavours and a list beyond one launch never raise the word."""
    for flavor, mvec in ((0, 5), (1, 5), (C_FLAVOR, 33)):
        p = Twins(torch_cuda, 1031, mvec, flavor=flavor)
        p.may_defer = False
        p.run(Q.sequence("capacity", 1031, mvec)[:mvec + 4])
        assert p.deferred == 0 and not p.replayed


@pytest.mark.parametrize("sums", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])
def test_a_deferring_handle_against_the_oracle(torch_cuda, oracle, sums):
    """As tests/test_hip_parity.py holds the plain handle: decisions exact, the returned f within the bar of the condition."""
    import nka_amd
    torch, n, m = torch_cuda, 1031, 5
    rng = np.random.default_rng(n * 131 + m)
    acc = tuned(nka_amd.nka(diagnostic=True).init(n, m, flavor=C_FLAVOR).set_sum_order(sums), 1)
    ora = oracle.OracleNKA(n, m, C_FLAVOR)
    spread = P.Spread(oracle, n, m)
    basis = rng.standard_normal((3, n))
    replays = 0
    for t in range(3 * m):
        x = rng.standard_normal(n) if (t % 5) else rng.standard_normal(3) @ basis
        f = x.copy()
        ora.accel_update(f)
        spread.update(x)
        ft = torch.from_numpy(x.copy()).cuda()
        acc.accel_update(ft)
        out = ft.cpu().numpy()
        replays += acc.defer_state()[1] > 0
        assert acc.num_vec() == ora.num_vec(), t
        assert acc.state().list_order() == ora.state().list_order()
        assert acc.state().free_order() == ora.state().free_order()
        P.check(S.rel_err(out, f, x), acc.state(), f"deferred v n={n} m={m} [{sums}]", where=t, spread=spread.value,
                truth=spread.truth(out, x))
    assert replays >= 3 * m - 3 and acc.defined()
