"""Binary32 storage of a batch's normalised subspace vectors (nka_hip_batch_create_stored, nka_batch().init(..., storage=
STORE_F32); include/nka_hip_batch.h, STORAGE).  q(x) = astype(float32).astype(float64) (tests/batch_store32.py).

  1 the three layers of tests/test_batch_sums_exact_gpu.py under the contract, exactly: the sums against exact_dot of the operands
    the contract names (d from the binary64 pending mirror, w1' = q(fl(d/s)) with the device's s, older w_p from a host mirror of
    the widened stored values) within gamma(batch_k(n)) sum|xy| -- K is unchanged: widening is exact and the narrowing precedes
    the product --; the oracle's scalar_step on the device's sums with ==; the stored w1' = q(fl(d/s)), the stored
    v = q(fl(fl(v1/s) - w1')), f_out = x + sum c v_p formed sequentially in binary64 from the mirror, get_w(new) = f_in and
    get_v(new) = f_out, bit for bit; systems that sat out unchanged
  2 weights, step and lengths, each against what already holds them
  3 a value beyond the binary32 range stays inside its own system
  4 capture before the first update
  5 a whole solve inside the budget the host model fixed (tests/test_batch_store32_cpu.py)
  6 refusals and lifecycle
  7 one batch whose float allocations pass 2^31 elements and 2^32 bytes

Tolerances are derived (gamma(batch_k(n)), batch_step.norm_bound); nothing is fitted."""
import json
import math
import os

import numpy as np
import pytest

import batch_large as G
import batch_lengths as BL
import batch_seq as B
import batch_step as T
import batch_store32 as S32
import exact_sums as X
from split_update import _bits_equal
from test_batch_large_gpu import Large, _fill_the_lists, _sequences
from test_batch_sums_exact_gpu import PLAN, SHAPE_CALLS, SHAPE_MVEC, BatchRun, _assert_planned_coverage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
F32_MIN_NORMAL = 2.0 ** -126
WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|xy|) seen, the K it was held to, where


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(f"batch sums, binary32 storage: worst |red - exact| = {ratio:.3f} u sum|xy| against K = {k} there ({where})")
    out = P.dump_dir(ROOT)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_store32_exact_worst.json"), "w") as fh:
            json.dump({"rounded": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.asarray(a, np.float64)).cuda()


def _batch32(nsys, n, mvec, **kw):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, n, mvec, storage=nka_amd.STORE_F32, **kw)
    assert b.storage() == nka_amd.STORE_F32 and b.flavor() == nka_amd.FLAVOR_C
    return b


def _hold(what, red, x, y, k, where):
    ex = X.exact_dot(x, y)
    if math.isnan(ex):
        assert math.isnan(red), (what, where, red)
        return
    if math.isinf(ex):
        assert red == ex, (what, where, red, ex)
        return
    tot = X.abs_dot(x, y)
    err = abs(red - ex)
    assert err <= X.gamma(k) * tot, (what, where, red, ex, err / (X.U * tot) if tot else err, k)
    if tot > 0 and err / (X.U * tot) >= WORST[0]:
        WORST[:] = [err / (X.U * tot), k, f"{what} {where}"]


# ---- 1. the three layers ---------------------------------------------------------------------------------------------------------

class Run32(BatchRun):
    """BatchRun for a batch with binary32 storage, left at SUMS_AUTO: its own mirror (W, V: the widened stored values of the
    normalised pairs; PW, PV: the raw pending pair, binary64) and its own _check under the contract.  A second binary32 batch
    set to SUMS_BLOCKED_ROUNDED explicitly takes every call too and must return the same bits: AUTO resolved to the rounded fast
    sums, at vlen <= 64 as well."""

    def __init__(self, torch, oracle, n, mvec, nsys, odd_ld=False):
        super().__init__(torch, oracle, 2, n, mvec, nsys, odd_ld)
        self.PW, self.PV = [None] * nsys, [None] * nsys
        self.subnormal = self.flushed = 0      # stored w1' elements in the binary32 subnormal range / +-0 from a nonzero d

    def _device(self, odd_ld):
        import nka_amd
        super()._device(odd_ld)
        self.b.delete()
        self.b = _batch32(self.nsys, self.n, self.m)
        self.explicit = _batch32(self.nsys, self.n, self.m).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        self.Fx = self.torch.zeros_like(self.raw).view(self.nsys, self.ld)[:, :self.n]
        self.order = nka_amd.SUMS_BLOCKED_ROUNDED      # (what the checks judge by: never the reference order)

    def update(self, inputs, order=None):
        assert order is None
        host = self.rows.copy()
        for k in inputs:
            host[k] = inputs[k]
        self.Fx.copy_(self.torch.from_numpy(host))
        super().update(inputs)
        self.explicit.accel_update(self.Fx, self._mask(sorted(inputs)))
        assert self.torch.equal(self.Fx, self.F), (self.n, self.calls, "SUMS_AUTO is not the rounded fast sums")
        for k in inputs:
            assert _bits_equal(self.explicit.reductions(k), self.b.reductions(k)) and self.explicit.state_digest(k) == self.dig[k]

    def _list_op(self, ks, op):
        ks = sorted(ks)
        getattr(self.b, op)(self._mask(ks))
        getattr(self.explicit, op)(self._mask(ks))
        for k in range(self.nsys):
            where = (self.n, self.m, op, "before call", self.calls, "system", k)
            if k not in ks:
                self._unchanged(k, where)
                continue
            if op == "restart":
                self.W[k], self.V[k] = {}, {}
                self.saw_after_restart = True
            self.PW[k] = self.PV[k] = None              # (relax drops the pending pair, F08:441-457)
            getattr(self.ora[k], op)()
            self._same_lists(self.b.state(k), self.ora[k].state(), where)
            assert _bits_equal(self.b.reductions(k), self.red[k]), (where, "red[] changed")
            self.dig[k] = self.b.state_digest(k)

    def _sum(self, what, red, x, y, where):
        _hold(what, red, x, y, self.k, where)

    def _check(self, k, st0, x, out, where):
        b, m = self.b, self.m
        W, V = self.W[k], self.V[k]
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        assert sorted(W) == sorted(olders) == sorted(V) and (self.PW[k] is not None) == bool(pending), (where, "the mirror lost track")
        red, st = b.reductions(k), b.state(k)
        self.widest = max(self.widest, len(olders))

        # 1: the sums
        s, normed, w1n, v1s = 0.0, False, None, None
        if pending:
            d = self.PW[k] - x
            self._sum("<d,d>", red[0], d, d, where)
            s = np.sqrt(np.float64(red[0]))
            normed = not s == 0.0
        if normed:
            with np.errstate(all="ignore"):
                w1n = S32.q(d / s)                                        # contract 3
                v1s = S32.q(self.PV[k] / s - w1n)                         # contract 4
            self._sum("<f,w1'>", red[1], x, w1n, where)
            for p, slot in enumerate(olders):
                self._sum(f"<w1',w_{p}>", red[2 + p], w1n, W[slot], where)
            self.nolder_normed.add(len(olders))
            self.subnormal += int(np.sum((w1n != 0) & (np.abs(w1n) < F32_MIN_NORMAL)))
            self.flushed += int(np.sum((w1n == 0) & (d != 0)))
        else:
            assert red[1] == 0.0 and not red[2:2 + m].any(), (where, "sums on w1' without a normalised pair", red[1:2 + m])
            if not pending:
                assert red[0] == 0.0, (where, red[0])
                self.nolder_no_pending.add(len(olders))
            else:
                self.saw_zero_s = True
        for p, slot in enumerate(olders):
            self._sum(f"<f,w_{p}>", red[2 + m + p], x, W[slot], where)
        for p in range(len(olders), m):
            assert red[2 + p] == 0.0 and red[2 + m + p] == 0.0, (where, p, red[2 + p], red[2 + m + p])

        # 2: the scalar step on the device's own sums
        hrow, rhs = np.zeros(m + 2), np.zeros(m + 2)
        for p, slot in enumerate(olders):
            hrow[slot], rhs[slot] = red[2 + p], red[2 + m + p]
        if pending:
            rhs[first0] = red[1]
        new = self.ora[k].scalar_step(float(s), hrow, rhs)
        sn = self.ora[k].state()
        self._same_lists(st, sn, where)
        assert st.first == new, where
        order = st.list_order()
        live = [i - 1 for i in order[1:]]
        assert np.array_equal(st.c[live], sn.c[live], equal_nan=True), (where, "c", st.c[live], sn.c[live])
        assert np.array_equal(st.h[np.ix_(live, live)], sn.h[np.ix_(live, live)], equal_nan=True), (where, "h")
        self.outcomes.append((k, self.calls, [p for p, slot in enumerate(olders) if slot not in order[1:]]))

        # 3: bit for bit
        new, comb = order[0], order[1:]
        Wn, Vn = {slot: W[slot] for slot in comb if slot in W}, {slot: V[slot] for slot in comb if slot in V}
        if normed:
            assert comb[0] == first0, (where, "the normalised pair does not lead the list")
            w1, v1 = b.w(k, first0), b.v(k, first0)
            assert _bits_equal(w1, w1n), (where, "stored w1' is not q(fl(d/s))", int(np.sum(w1 != w1n)))
            assert _bits_equal(v1, v1s), (where, "stored v is not q(fl(fl(v1/s) - w1'))", int(np.sum(v1 != v1s)))
            assert _bits_equal(S32.q(w1), w1) and _bits_equal(S32.q(v1), v1)      # (what a binary32 slot can hold)
            Wn[first0], Vn[first0] = w1, v1
        elif pending:
            assert first0 not in comb, (where, "s == 0 did not drop the pending pair")
        f = x.copy()
        with np.errstate(all="ignore"):
            for slot in comb:
                f = f + st.c[slot - 1] * Vn[slot]
        assert _bits_equal(out, f), (where, "f_out", len(comb), int(np.sum(out != f)))
        assert _bits_equal(b.w(k, new), x), (where, "get_w of the pending slot is not f_in")
        assert _bits_equal(b.v(k, new), out), (where, "get_v of the pending slot is not f_out")
        self.PW[k], self.PV[k] = x.copy(), out.copy()
        self.W[k], self.V[k] = Wn, Vn
        self.ncomb.add((len(comb), normed))
        self.red[k], self.dig[k] = red, b.state_digest(k)


def _input32(n, rng, prev):
    """exact_sums.batch_planted_input with two components off the sentinels scaled by 1e-42 and 1e-50: their share of the
    normalised difference lands in the binary32 subnormal range and at +-0."""
    x = X.batch_planted_input(n, rng, prev)
    free = np.setdiff1d(np.arange(n), X.batch_all_sentinels(n))
    if free.size >= 2:
        x[free[free.size // 3]] *= 1e-42
        x[free[2 * free.size // 3]] *= 1e-50
    return x


def _planned_run32(run, seed):
    rngs, prev = [np.random.default_rng([seed, k]) for k in range(run.nsys)], [None] * run.nsys
    for t in range(SHAPE_CALLS):
        steps = {k: t - PLAN[k][0] for k in range(run.nsys) if t >= PLAN[k][0]}
        relax = [k for k, j in steps.items() if j == PLAN[k][1]]
        restart = [k for k, j in steps.items() if j == PLAN[k][3]]
        if relax:
            run.relax(relax)
        if restart:
            run.restart(restart)
        inputs = {}
        for k, j in steps.items():
            inputs[k] = prev[k].copy() if j == PLAN[k][2] else _input32(run.n, rngs[k], prev[k])
            prev[k] = inputs[k]
        run.update(inputs)
    return run


@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 511, 512, 513, 1025, 4099])
def test_every_part_of_an_update_at_the_boundary_shapes(torch_cuda, oracle, n, odd_ld):
    """The planned six-system staggered run of tests/test_batch_sums_exact_gpu.py (masked relax, restart, a repeated input for
    s == 0, mvec = 10).  n <= 64 would have been reference order under SUMS_AUTO with binary64 storage."""
    run = _planned_run32(Run32(torch_cuda, oracle, n, SHAPE_MVEC, len(PLAN), odd_ld), seed=n)
    assert run.lengths_differed and run.saw_zero_s and run.saw_after_restart and 0 in run.nolder_no_pending
    if n >= 63:
        _assert_planned_coverage(run)
        assert run.subnormal > 0 and run.flushed > 0, (n, run.subnormal, run.flushed)


def test_every_older_count_up_to_the_largest_subspace(torch_cuda, oracle):
    n, mvec = X.BATCH_WIDTH_SHAPE, 32
    run = Run32(torch_cuda, oracle, n, mvec, 2, odd_ld=True)
    rngs, prev = [np.random.default_rng([n, k]) for k in range(2)], [None, None]
    for t in range(mvec + 2):
        inputs = {}
        for k in range(2):
            if t >= k:
                inputs[k] = prev[k] = _input32(n, rngs[k], prev[k])
        run.update(inputs)
    assert run.widest == mvec == 32 and run.nolder_normed == set(range(mvec + 1)), run.nolder_normed
    assert run.lengths_differed and run.subnormal > 0 and run.flushed > 0


@pytest.mark.parametrize("n", X.BATCH_CAP_SHAPES, ids=["16383", "16384"])
def test_every_part_of_an_update_at_the_longest_system(torch_cuda, oracle, n):
    assert X.batch_k(n) == 73
    run = Run32(torch_cuda, oracle, n, 3, 2, odd_ld=bool(n % 2))
    rngs, prev = [np.random.default_rng([n, k]) for k in range(2)], [None, None]
    for t in range(5):
        inputs = {}
        for k in range(2):
            if t >= k:
                inputs[k] = prev[k] = _input32(n, rngs[k], prev[k])
        run.update(inputs)
    assert run.widest == 3 and run.lengths_differed and run.subnormal > 0 and run.flushed > 0


# ---- 2. weights, step, lengths -------------------------------------------------------------------------------------------------

def _same_state(a, b, nsys, where):
    assert np.array_equal(a.num_vec(), b.num_vec()), (where, "num_vec")
    for k in range(nsys):
        assert a.state_digest(k) == b.state_digest(k), (where, k, "digest")
        assert _bits_equal(a.reductions(k), b.reductions(k)), (where, k, "red")


@pytest.mark.parametrize("n", [65, 513, 1025])
def test_unit_weights_are_the_unweighted_batch(torch_cuda, n):
    torch = torch_cuda
    nsys, mvec = 4, 5
    plain, unit = _batch32(nsys, n, mvec), _batch32(nsys, n, mvec)
    unit.set_dot_weights(np.ones((nsys, n)))
    assert unit.dot_weighted() and not plain.dot_weighted()
    seqs = [B.Sequence(n, 3200 + 7 * k + n) for k in range(nsys)]
    for t in range(12):
        xh = np.stack([s.next() for s in seqs])
        Fa, Fb = _f64(torch, xh), _f64(torch, xh)
        plain.accel_update(Fa)
        unit.accel_update(Fb)
        assert torch.equal(Fa, Fb), (n, t)
        _same_state(plain, unit, nsys, (n, t))
    plain.delete()
    unit.delete()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n", [1, 65, 513, 1025])
def test_a_step_is_the_update(torch_cuda, n, weighted):
    """accel_step of a binary32 batch against a binary32 twin that runs accel_update under the mask the host predicts from the
    device's fnorm: F, X, the mask, red[], the digests with ==; fnorm within batch_step.norm_bound(n) of the exact norm."""
    import batch_weights as BW
    torch = torch_cuda
    nsys, mvec, calls = 6, 5, 12
    ld, ldx = n + 1 - n % 2, n + n % 2                       # an odd and an even row stride
    wts = BW.system_weights(n, nsys) if weighted else None
    step, twin = _batch32(nsys, n, mvec), _batch32(nsys, n, mvec)
    if weighted:
        step.set_dot_weights(wts)
        twin.set_dot_weights(wts)
    rng = np.random.default_rng([32, n, int(weighted)])
    seqs = [B.Sequence(n, 3300 * n + 10 * k) for k in range(nsys)]
    fs_raw, ft_raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda"), torch.zeros(nsys * ld, dtype=torch.float64, device="cuda")
    Fs, Ft = fs_raw.view(nsys, ld)[:, :n], ft_raw.view(nsys, ld)[:, :n]
    xhost = rng.standard_normal((nsys, ldx))
    x_raw = _f64(torch, xhost.ravel())
    Xd = x_raw.view(nsys, ldx)[:, :n]
    fhost, alive = np.zeros((nsys, ld)), np.ones(nsys, bool)
    mask, tol, fnorm = _i32(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    retired = 0
    for t in range(calls):
        where = (n, weighted, t)
        for op, at, who in (("relax", 5, [1, 4]), ("restart", 8, [2, 5])):
            if t == at:
                m = _i32(torch, [int(k in who) for k in range(nsys)])
                getattr(step, op)(m)
                getattr(twin, op)(m)
        entry = alive & (t >= np.arange(nsys) % 3)
        for k in np.flatnonzero(entry):
            fhost[k, :n] = seqs[k].next()
        tolh = np.full(nsys, -1.0)
        if t in (4, 9) and entry.sum() >= 3:
            a = fhost[:, :n] * (wts if weighted else 1.0)
            tolh[:] = np.sort(np.sqrt((a * fhost[:, :n]).sum(axis=1))[entry])[1] * (1.0 + 1e-9)
        for raw in (fs_raw, ft_raw):
            raw.copy_(torch.from_numpy(fhost.ravel()))
        mask.copy_(_i32(torch, entry))
        tol.copy_(_f64(torch, tolh))
        fnorm.fill_(-7.0)
        step.accel_step(Fs, Xd, mask, tol, fnorm)
        fn, got = fnorm.cpu().numpy(), mask.cpu().numpy().astype(bool)
        assert (fn[~entry] == -7.0).all(), (where, "fnorm of a system inactive on entry")
        for k in np.flatnonzero(entry):
            f = fhost[k, :n]
            ok, ratio = T.norm_inside(fn[k], f * wts[k] if weighted else f, f, n)
            assert ok, (where, k, fn[k], ratio)
        with np.errstate(invalid="ignore"):
            want = entry & ~(fn <= tolh)
        assert np.array_equal(got, want), (where, "mask", got, want)
        twin.accel_update(Ft, _i32(torch, want))
        assert torch.equal(fs_raw, ft_raw), (where, "F")
        _same_state(step, twin, nsys, where)
        fhost = fs_raw.cpu().numpy().reshape(nsys, ld)
        xwant = xhost.copy()
        xwant[want, :n] = xhost[want, :n] - fhost[want, :n]
        xgot = x_raw.cpu().numpy().reshape(nsys, ldx)
        assert _bits_equal(xgot, xwant), (where, "X")
        xhost = xgot
        retired += int((entry & ~want).sum())
        alive &= ~(entry & ~want)
    assert retired >= 1 and alive.any() and step.num_vec().max() >= 1
    step.delete()
    twin.delete()


def _live_state_equal(sa, sb):
    """The lists and, on their live entries, h and c (a batch that ran before its restart keeps stale entries elsewhere)."""
    if (sa.first, sa.last, sa.free, sa.subspace, sa.pending) != (sb.first, sb.last, sb.free, sb.subspace, sb.pending):
        return False
    if sa.list_order() != sb.list_order() or sa.free_order() != sb.free_order():
        return False
    live = [i - 1 for i in sa.list_order()[1:]]
    return _bits_equal(sa.c[live], sb.c[live]) and _bits_equal(sa.h[np.ix_(live, live)], sb.h[np.ix_(live, live)])


@pytest.mark.parametrize("paint_slots", [False, True], ids=["fresh", "slots-painted"])
def test_lengths_against_twins_of_that_length(torch_cuda, paint_slots):
    """Lengths {1, 65, 513, 1025} in one binary32 batch of vlen = 1100 against binary32 twins created at vlen = len[sys], with ==;
    the tails of F and X hold NaNs of distinct payloads and are compared byte for byte after every call.
    fresh: the lengths are set on a new batch, and the digests are compared too.
    slots-painted: seven full-length updates first write every ring slot and the pending rows over their whole length; after a
    restart every ring slot is read (no pending pair: get_w / get_v return the stored floats) and the pending rows' tails are
    known on the host (the last input and output).  After the run every tail of the pending rows (get_w / get_v of the pending
    slot) and, after a relax, of every ring slot is compared byte for byte with that paint.  (The control block of such a batch
    keeps stale entries from before its restart, so the state is compared on its live entries instead of by digest.)"""
    torch = torch_cuda
    vlen, lens, mvec = 1100, [1, 65, 513, 1025], 3
    nsys = len(lens)
    b = _batch32(nsys, vlen, mvec)
    rng = np.random.default_rng(3232)
    if paint_slots:
        for t in range(7):
            fin = rng.standard_normal((nsys, vlen))
            F = _f64(torch, fin)
            b.accel_update(F)
        pend_tail = [(fin[k, L:].copy(), F.cpu().numpy()[k, L:].copy()) for k, L in enumerate(lens)]
        b.restart()
        ring = {(k, s): (b.w(k, s), b.v(k, s)) for k in range(nsys) for s in range(1, mvec + 2)}
        assert all(w[lens[k]:].any() and v[lens[k]:].any() for (k, s), (w, v) in ring.items()), "a ring slot holds no paint"
    b.set_lengths(np.array(lens, np.int32))
    twins = [_batch32(1, L, mvec) for L in lens]
    fpaint, xpaint = BL.nan_paint(nsys, vlen, 1), BL.nan_paint(nsys, vlen, 2)
    xh = xpaint.copy()
    for k, L in enumerate(lens):
        xh[k, :L] = rng.standard_normal(L)
    Xd = _f64(torch, xh)
    Xt = [_f64(torch, xh[k:k + 1, :L]) for k, L in enumerate(lens)]
    seqs = BL.sequences(lens, 3270)
    for t in range(9):
        if t == 5:
            m = _i32(torch, [1, 0, 1, 0])
            b.relax(m)
            for k in (0, 2):
                twins[k].relax()
        fh = fpaint.copy()
        for k, L in enumerate(lens):
            fh[k, :L] = seqs[k].next()
        F = _f64(torch, fh)
        b.accel_step(F, Xd)
        got, xg = F.cpu().numpy(), Xd.cpu().numpy()
        assert BL.tails_intact(got, fpaint, lens) == [] and BL.tails_intact(xg, xpaint, lens) == [], t
        for k, L in enumerate(lens):
            Fk = _f64(torch, fh[k:k + 1, :L])
            twins[k].accel_step(Fk, Xt[k])
            where = (t, k, L)
            assert BL.same_bytes(got[k, :L], Fk.cpu().numpy()[0]) and BL.same_bytes(xg[k, :L], Xt[k].cpu().numpy()[0]), where
            assert _bits_equal(b.reductions(k), twins[k].reductions(0)) and _live_state_equal(b.state(k), twins[k].state(0)), where
            if not paint_slots:
                assert b.state_digest(k) == twins[k].state_digest(0), where
            for s in b.state(k).list_order():
                assert BL.same_bytes(b.w(k, s)[:L], twins[k].w(0, s)) and BL.same_bytes(b.v(k, s)[:L], twins[k].v(0, s)), (where, s)
    assert b.num_vec().tolist() == [int(t_.num_vec()[0]) for t_ in twins]
    if paint_slots:
        for k, L in enumerate(lens):                         # the pending rows beyond L: still the last full-length pair
            st = b.state(k)
            assert st.pending and BL.same_bytes(b.w(k, st.first)[L:], pend_tail[k][0]) and BL.same_bytes(b.v(k, st.first)[L:], pend_tail[k][1]), k
        b.relax()
        for (k, s), (w, v) in ring.items():                  # every ring slot beyond L: still the paint
            assert BL.same_bytes(b.w(k, s)[lens[k]:], w[lens[k]:]) and BL.same_bytes(b.v(k, s)[lens[k]:], v[lens[k]:]), (k, s)
    else:
        for k, L in enumerate(lens):                         # nothing beyond L was ever written: zeros
            for s in range(1, mvec + 2):
                assert not b.w(k, s)[L:].any() and not b.v(k, s)[L:].any(), (k, s)
    b.delete()
    for t_ in twins:
        t_.delete()


# ---- 3. overflow stays home -----------------------------------------------------------------------------------------------------

def test_a_value_beyond_the_binary32_range_stays_in_its_system(torch_cuda):
    """System 2 of five has a frozen entry at 1e10 and a moving entry of about 1e-30: s is about 1e-30, fl(v1/s) about 1e40 at the
    frozen entry, and the stored v holds +-Inf exactly where q() says.  Every other system is == a twin batch in which system 2
    sits every call out."""
    torch = torch_cuda
    nsys, n, mvec, ill = 5, 130, 4, 2
    b, twin = _batch32(nsys, n, mvec), _batch32(nsys, n, mvec)
    rng = np.random.default_rng(3203)
    others = [k for k in range(nsys) if k != ill]
    tmask = _i32(torch, [int(k != ill) for k in range(nsys)])
    pw = pv = None
    met_inf = False
    for t in range(5):
        xh = rng.standard_normal((nsys, n))
        xh[ill] = 0.0
        xh[ill, 0], xh[ill, 7] = 1e10, 1e-30 * (t + 1)
        Fa, Fb = _f64(torch, xh), _f64(torch, xh)
        st0 = b.state(ill)
        b.accel_update(Fa)
        twin.accel_update(Fb, tmask)
        out = Fa.cpu().numpy()
        assert _bits_equal(out[others], Fb.cpu().numpy()[others]), t
        for k in others:
            assert b.state_digest(k) == twin.state_digest(k) and _bits_equal(b.reductions(k), twin.reductions(k)), (t, k)
        if t == 1:                                           # the first normalised pair of the ill system
            s = np.sqrt(np.float64(b.reductions(ill)[0]))
            with np.errstate(all="ignore"):
                w1n = S32.q((pw - xh[ill]) / s)
                v1s = S32.q(pv / s - w1n)
            got = b.v(ill, st0.first)
            assert np.isinf(v1s[0]) and np.isfinite(v1s[1:]).all() and _bits_equal(got, v1s), (got[:8], v1s[:8])
            assert _bits_equal(b.w(ill, st0.first), w1n)
            met_inf = True
        pw, pv = xh[ill].copy(), out[ill].copy()
    assert met_inf and not np.isfinite(out[ill]).all() and np.isfinite(out[others]).all()
    b.delete()
    twin.delete()


# ---- 4. capture before the first update ----------------------------------------------------------------------------------------

def test_captured_before_the_first_update_and_replayed(torch_cuda):
    """8 systems, mvec = 3: the update captured ONCE before any has run and replayed through growth to a full list, the capacity
    drop and a masked relax; an eager binary32 twin takes the same calls."""
    torch = torch_cuda
    nsys, n, mvec = 8, 513, 3
    rng = np.random.default_rng(3204)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _batch32(nsys, n, mvec)
        Fs = torch.zeros(nsys, n, dtype=torch.float64, device="cuda")
    eager = _batch32(nsys, n, mvec)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.accel_update(Fs)
    assert b.num_vec().max() == 0
    relax = _i32(torch, [k % 2 for k in range(nsys)])
    for t in range(9):
        if t == 6:
            with torch.cuda.stream(side):
                b.relax(relax)
            eager.relax(relax)
        xh = rng.standard_normal((nsys, n))
        with torch.cuda.stream(side):
            Fs.copy_(_f64(torch, xh))
            g.replay()
        side.synchronize()
        Fe = _f64(torch, xh)
        eager.accel_update(Fe)
        assert torch.equal(Fs, Fe), t
        _same_state(b, eager, nsys, t)
    assert b.num_vec().max() == mvec
    b.delete()
    eager.delete()


# ---- 5. a whole solve ---------------------------------------------------------------------------------------------------------

def _solve(torch, storage):
    import nka_amd
    nsys, vlen, mvec = T.SOLVE_NSYS, T.SOLVE_VLEN, T.SOLVE_MVEC
    d, eps, bb, x = (_f64(torch, a) for a in T.solve_problem())
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, storage=storage)
    mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    retired = np.full(nsys, -1)
    for it in range(T.SOLVE_REPLAYS):
        F = T.solve_residual(torch, x, d, eps, bb)
        before = mask.cpu().numpy().astype(bool)
        b.accel_step(F, x, mask, tol, fnorm)
        if it == 0:
            torch.mul(fnorm, T.SOLVE_TOL, out=tol)           # device-formed relative thresholds
        retired[before & ~mask.cpu().numpy().astype(bool)] = it
    b.delete()
    return retired


def test_a_whole_solve_inside_the_budget_of_the_host_model(torch_cuda):
    """batch_step.solve_problem(), flavour C, mvec = 6, accel_step with device-formed relative thresholds: every system of the
    binary32 batch retires within SOLVE_REPLAYS - SOLVE_SLACK steps, the budget the host model fixed on the CPU.  The binary64
    batch runs beside it; both sets of iterations go to batch_store32_solve.json.  Only the budget is asserted."""
    import nka_amd
    import parity_util as P
    it32, it64 = _solve(torch_cuda, nka_amd.STORE_F32), _solve(torch_cuda, nka_amd.STORE_F64)
    print("binary32 retirements", it32.tolist(), "binary64", it64.tolist())
    out = P.dump_dir(ROOT)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_store32_solve.json"), "w") as fh:
            json.dump({"binary32": it32.tolist(), "binary64": it64.tolist(), "differ": int((it32 != it64).sum()),
                       "tol": T.SOLVE_TOL, "mvec": T.SOLVE_MVEC}, fh, indent=1, sort_keys=True)
    assert (it32 >= 0).all() and it32.max() <= T.SOLVE_REPLAYS - T.SOLVE_SLACK, it32


# ---- 6. refusals and lifecycle ----------------------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(torch_cuda):
    import ctypes as C

    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    L = nka_amd.nka_batch()._L
    nsys, n, mvec = 48, 16384, 20
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    h = C.c_void_p()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for flavor in (nka_amd.FLAVOR_F08, nka_amd.FLAVOR_F08_VECTOR):
        assert L.nka_hip_batch_create_stored(C.byref(h), nsys, n, mvec, 0.01, flavor, 0, stream, nka_amd.STORE_F32) == EINVAL
        assert h.value is None and b"flavour" in L.nka_hip_last_error()
        with pytest.raises(NKAError):
            nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor, storage=nka_amd.STORE_F32)
    assert L.nka_hip_batch_create_stored(C.byref(h), nsys, n, mvec, 0.01, nka_amd.FLAVOR_C, 0, stream, 2) == EINVAL and h.value is None
    with pytest.raises(NKAError, match="wide"):
        nka_amd.nka_batch().init(nsys, n, mvec, wide=True, storage=nka_amd.STORE_F32)
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "a refused creation left something allocated"
    # the allocation: the library's own accounting equals the formula, and the device's free memory moved by about that much
    want32, want64 = S32.vector_bytes(nsys, n, mvec, S32.STORE_F32), S32.vector_bytes(nsys, n, mvec, S32.STORE_F64)
    b = _batch32(nsys, n, mvec)
    assert b.vector_bytes() == want32
    grown = free0 - torch.cuda.mem_get_info()[0]
    assert want32 <= grown + (64 << 20) and grown <= want32 + (96 << 20), (grown, want32)
    with pytest.raises(NKAError, match="binary32"):
        b.set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    b.set_sum_order(nka_amd.SUMS_AUTO).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    rng = np.random.default_rng(3206)
    for s in range(1, mvec + 2):                             # never-written slots read zeros
        assert not b.w(5, s).any() and not b.v(5, s).any()
    x0, x1 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    F = _f64(torch, x0)
    b.accel_update(F)
    st = b.state(5)
    assert st.pending and _bits_equal(b.w(5, st.first), x0[5]) and _bits_equal(b.v(5, st.first), x0[5])      # binary64-exact
    assert (S32.q(x0[5]) != x0[5]).any()
    F = _f64(torch, x1)
    b.accel_update(F)
    w = b.w(5, st.first)
    assert _bits_equal(S32.q(w), w) and abs(np.linalg.norm(w) - 1.0) < 1e-6                                   # now a stored float row
    b.delete()
    b64 = nka_amd.nka_batch().init(nsys, n, mvec, flavor=nka_amd.FLAVOR_C)
    assert b64.storage() == nka_amd.STORE_F64 and b64.vector_bytes() == want64
    b64.delete()
    b = _batch32(nsys, n, mvec)                               # destroy and re-create
    assert b.num_vec().max() == 0 and b.vector_bytes() == want32
    b.delete()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "destroy left something allocated"


# ---- 7. one large case -----------------------------------------------------------------------------------------------------------

class Large32(Large):
    """tests/test_batch_large_gpu.py's large batch beside its twin, both with binary32 storage; the systems that run and the
    witnesses are those of tests/batch_store32.py (a float's byte offset passes 2^32 at 2^30 elements)."""

    def __init__(self, torch):
        self.torch, self.sh = torch, S32.LARGE
        self.active = S32.large_active()
        self.na = len(self.active)
        self.b = self.t = self.mask = self.tmask = self.idx = None
        self.raw, self.rows, self.trows, self.host, self.misc = {}, {}, {}, {}, {}
        try:
            self._create("slots, binary32")
        except BaseException:
            self.close()
            raise

    def _create(self, sid):
        import time
        torch, sh = self.torch, self.sh
        need = S32.large_bytes()
        free, total = torch.cuda.mem_get_info()
        if free < need + (8 << 30):
            pytest.skip(f"{sid}: {free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 8 GiB")
        self.t0 = time.perf_counter()
        self.b, self.t = _batch32(sh.nsys, sh.vlen, sh.mvec), _batch32(self.na, sh.vlen, sh.mvec)
        assert self.b.vector_bytes() == S32.vector_bytes(sh.nsys, sh.vlen, sh.mvec, S32.STORE_F32) > 2 ** 34
        self.fresh_digest = self.b.state_digest(S32.large_witnesses()[0])
        self.raw["F"] = torch.full((G.span(sh, "F"),), G.PAD, dtype=torch.float64, device="cuda")
        self.rows["F"] = torch.as_strided(self.raw["F"], (sh.nsys, sh.vlen), (sh.ld, 1))
        self.trows["F"] = torch.zeros(self.na, sh.vlen, dtype=torch.float64, device="cuda")
        self.host["F"] = [None] * self.na
        self.mask = torch.zeros(sh.nsys, dtype=torch.int32, device="cuda")
        self.tmask = torch.ones(self.na, dtype=torch.int32, device="cuda")
        self.idx = torch.tensor(self.active, dtype=torch.int64, device="cuda")
        self.mask[self.idx] = 1
        self.lens = [sh.vlen] * self.na
        self.ran = np.zeros(self.na, np.int64)

    def finish(self, where):
        sh = self.sh
        self.compare(where + ("every slot",), "all")
        nv = self.b.num_vec()
        idle = np.ones(sh.nsys, bool)
        idle[self.active] = False
        assert (nv[idle] == 0).all(), (where, "a system that never ran holds vectors", np.flatnonzero(idle & (nv != 0))[:8])
        for k in S32.large_witnesses():
            assert self.b.state_digest(k) == self.fresh_digest, (where, "witness", k, "digest")
            for s in range(1, sh.mvec + 2):
                assert not self.b.w(k, s).any() and not self.b.v(k, s).any(), (where, "witness", k, "slot", s)
        for k in self.active:
            self.rows["F"][k].fill_(G.PAD)
        assert bool((self.raw["F"] == G.PAD).all().item()), (where, "an element of F of no running system was written")


def test_float_slots_beyond_2_to_the_31_elements_and_2_to_the_32_bytes(torch_cuda):
    """3976 systems of 16 384, mvec = 32, binary32 storage: each of the w and the v allocation holds 2.15e9 floats, 8.6 GB.  System
    3971 straddles 2^31 elements, system 1985 2^30 elements = 2^32 bytes; they, their neighbours, system 0 and the last one run,
    all others are masked.  36 updates on fresh inputs fill the lists to 32 and write every slot, then mixed inputs and a masked
    restart; every running system == its system in a small binary32 twin after every call, the witnesses at the wrapped offsets
    are untouched."""
    L = Large32(torch_cuda)
    try:
        k30 = G.on_boundary(S32.LARGE, "w", S32.BYTES_4G_FLOATS)
        assert k30 in L.active and G.on_boundary(S32.LARGE, "w", G.ELEMS_2G) in L.active
        _fill_the_lists(L, np.random.default_rng(3207), ("slots32",))
        seqs = _sequences(L, 3207)
        for c in range(3):
            L.update(("slots32", "mixed", c), [s.next() for s in seqs])
        L.restart([0, 2, 5])
        for c in range(3):
            L.update(("slots32", "after the restart", c), [s.next() for s in seqs])
        L.finish(("slots32",))
    finally:
        L.close()
