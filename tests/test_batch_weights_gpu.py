"""Diagonal dot-product weights of the batched accelerator (nka_hip_batch_set_dot_weights, nka_amd.nka_batch.set_dot_weights):
<x,y>_w = sum_i w_i x_i y_i per system inside the one launch, fl(w_i a_i) the first operand of every product.

  1 w == 1 gives the plain batch's bits, in both forms (one row for all, one row per system), and so does clearing the weights
  2 powers of four are an exact rescaling, per system
  3 in reference order a system carries the bits of the reference run with the same dp
  4 the fast sums, the scalar step and the elementwise statements, each held exactly (BatchRun of
    tests/test_batch_sums_exact_gpu.py with the first operand of every sum replaced by fl(w x); tests/test_batch_weights_cpu.py
    shows that the check has teeth at these shapes)
  5 a zero-weight tail is a shorter system (ragged batches)
  6 masked entries stay out of every sum and decision
  7 graph capture
  8 refusals and lifecycle"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import batch_seq as B
import batch_weights as BW
import exact_sums as X
from split_update import _bits_equal, ordered_dot
from test_batch_sums_exact_gpu import PLAN, SHAPE_MVEC, BatchRun, _planned_run

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|fl(w x) y|) seen, the K it was held to, where


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _orders():
    import nka_amd
    return {"reference": nka_amd.SUMS_REFERENCE_ORDER, "rounded": nka_amd.SUMS_BLOCKED_ROUNDED}


def _ld(n, odd):
    return n + (1 - n % 2 if odd else n % 2)                 # the smallest odd / even row stride that holds a row


def _rows(torch, nsys, n, ld, fill=0.0):
    """nsys rows of n doubles, ld apart, inside one allocation: (the whole buffer, the view a batch takes)."""
    raw = torch.full((nsys * ld,), fill, dtype=torch.float64, device="cuda")
    return raw, raw.view(nsys, ld)[:, :n]


def _mask(torch, nsys, ks):
    if len(ks) == nsys:
        return None
    m = np.zeros(nsys, np.int32)
    m[list(ks)] = 1
    return torch.from_numpy(m).cuda()


def _decisions(st):
    return st.list_order(), st.free_order(), (st.subspace, st.pending)


def _same_system(a, ka, b, kb, where):
    """red[], h, c and the decisions of system ka of batch a and system kb of batch b, bit for bit."""
    assert _bits_equal(a.reductions(ka), b.reductions(kb)), (where, "red")
    sa, sb = a.state(ka), b.state(kb)
    assert _decisions(sa) == _decisions(sb), (where, "lists")
    assert _bits_equal(sa.h, sb.h) and _bits_equal(sa.c, sb.c), (where, "h / c")
    return sa


# ---- 1. w == 1 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 511, 512, 513, 1025, 4099, 16384])
def test_unit_weights_give_the_bits_of_the_plain_batch(torch_cuda, n):
    """Three flavours, both sum orders, even and odd ld; mvec = 10, mvec + 4 updates of 5 systems with staggered starts.  Beside
    the plain batch: unit weights in the shared form, unit weights per row (rows ld apart, like f), and a batch whose general
    weights were cleared again.  After every update the rows of f, every red[] and every digest are the plain batch's."""
    import nka_amd
    torch = torch_cuda
    mvec, nsys = 10, 5
    for flavor in (0, 1, 2):
        for oname, order in _orders().items():
            for odd in (False, True):
                ld = _ld(n, odd)
                new = lambda: nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(order)      # noqa: E731
                _, ones = _rows(torch, nsys, n, ld, fill=1.0)
                general = torch.from_numpy(BW.system_weights(n, nsys)).cuda()
                batches = {"plain": new(), "shared": new().set_dot_weights(ones[0]), "rows": new().set_dot_weights(ones),
                           "cleared": new().set_dot_weights(general).set_dot_weights(None)}
                assert [b.dot_weighted() for b in batches.values()] == [False, True, True, False]
                bufs = {name: _rows(torch, nsys, n, ld)[1] for name in batches}
                seqs = [B.Sequence(n, 1000 * n + 10 * k + flavor) for k in range(nsys)]
                host = np.zeros((nsys, n))
                for t in range(mvec + 4):
                    ks = [k for k in range(nsys) if t >= k]
                    for k in ks:
                        host[k] = seqs[k].next()
                    mask = _mask(torch, nsys, ks)
                    for name, b in batches.items():
                        bufs[name].copy_(torch.from_numpy(host))
                        b.accel_update(bufs[name], mask)
                    host = bufs["plain"].cpu().numpy()
                    for name in ("shared", "rows", "cleared"):
                        where = (n, flavor, oname, ld, t, name)
                        assert torch.equal(bufs[name], bufs["plain"]), where
                        for k in range(nsys):
                            assert _bits_equal(batches[name].reductions(k), batches["plain"].reductions(k)), (where, k)
                            assert batches[name].state_digest(k) == batches["plain"].state_digest(k), (where, k)
                for b in batches.values():
                    b.delete()


# ---- 2. powers of four ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mvec", [1, 5, 20, 32])
@pytest.mark.parametrize("n", [7, 129, 513, 4099])
@pytest.mark.parametrize("oname", ["reference", "rounded"])
def test_powers_of_four_are_an_exact_rescaling_per_system(torch_cuda, oname, n, mvec):
    """w[sys, i] = 4^k, k in [-6, 6] drawn per system and element: fl(w a) b = (2^k a)(2^k b) exactly, so the weighted batch on
    F equals 2^-k o (a plain batch on 2^k o F), bit for bit: rows, red[], h, c, list and free order, stored w and v."""
    import nka_amd
    torch = torch_cuda
    order, nsys = _orders()[oname], 3
    for flavor in (0, 1, 2):
        rng = np.random.default_rng([4, n, mvec, flavor])
        k4 = rng.integers(-6, 7, (nsys, n))
        scale = np.ldexp(1.0, k4)
        bw = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(order)
        bw.set_dot_weights(torch.from_numpy(np.ldexp(1.0, 2 * k4)).cuda())
        bp = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(order)
        seqs = [B.Sequence(n, 4000 * n + 100 * mvec + 10 * k + flavor) for k in range(nsys)]
        for t in range(mvec + 4):
            Xh = np.stack([s.next() for s in seqs])
            Fw, Fp = torch.from_numpy(Xh.copy()).cuda(), torch.from_numpy(scale * Xh).cuda()
            bw.accel_update(Fw)
            bp.accel_update(Fp)
            where = (oname, n, mvec, flavor, t)
            assert _bits_equal(scale * Fw.cpu().numpy(), Fp.cpu().numpy()), where
            for k in range(nsys):
                st = _same_system(bw, k, bp, k, (where, k))
                for slot in st.list_order():
                    assert _bits_equal(scale[k] * bw.w(k, slot), bp.w(k, slot)), (where, k, slot, "w")
                    assert _bits_equal(scale[k] * bw.v(k, slot), bp.v(k, slot)), (where, k, slot, "v")
        assert bw.num_vec().max() >= 1
        bw.delete()
        bp.delete()


# ---- 3. reference order: the reference's bits with the same dp ---------------------------------------------------------------

def _general_weights(n, rng):
    """2^U(-3, 3), not powers of two, with 10 % zeros."""
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0
    return w


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 7, 64, 65, 513, 1537])
def test_reference_order_carries_the_reference_bits_with_the_same_dp(torch_cuda, oracle, n, flavor):
    """One oracle per system with dp(x, y) = the sequential sum of fl(fl(w x) y); 6 systems, mvec + 6 calls, some systems sit
    calls out, a masked relax and a masked restart on the way.  Up to 64 elements the order is SUMS_AUTO (which must resolve to
    the reference's with weights too), beyond it SUMS_REFERENCE_ORDER."""
    import nka_amd
    torch = torch_cuda
    mvec, nsys = 5, 6
    rng = np.random.default_rng([3, n, flavor])
    W = np.stack([_general_weights(n, rng) for _ in range(nsys)])
    b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor)
    b.set_sum_order(nka_amd.SUMS_AUTO if n <= 64 else nka_amd.SUMS_REFERENCE_ORDER).set_dot_weights(torch.from_numpy(W).cuda())
    oras = [oracle.OracleNKA(n, mvec, flavor) for _ in range(nsys)]
    for k, o in enumerate(oras):
        o.set_dot_prod(lambda x, y, w=W[k]: ordered_dot(w * x, y))
    seqs = [B.Sequence(n, 3000 * n + 10 * k + flavor) for k in range(nsys)]
    F = torch.zeros(nsys, n, dtype=torch.float64, device="cuda")
    for t in range(mvec + 6):
        for op, at, who in (("relax", 5, [1, 4]), ("restart", 8, [2, 5])):
            if t == at:
                getattr(b, op)(_mask(torch, nsys, who))
                for k in who:
                    getattr(oras[k], op)()
        ks = [k for k in range(nsys) if (t + k) % 4 != 3]
        before = F.cpu().numpy()
        red0 = [b.reductions(k) for k in range(nsys)]
        dig0 = [b.state_digest(k) for k in range(nsys)]
        host, want = before.copy(), before.copy()
        for k in ks:
            host[k] = seqs[k].next()
            want[k] = host[k]
            oras[k].accel_update(want[k])
        F.copy_(torch.from_numpy(host))
        b.accel_update(F, _mask(torch, nsys, ks))
        got, nv = F.cpu().numpy(), b.num_vec()
        for k in range(nsys):
            where = (n, flavor, t, k)
            if k not in ks:
                assert _bits_equal(got[k], before[k]) and _bits_equal(b.reductions(k), red0[k]), (where, "sat out")
                assert b.state_digest(k) == dig0[k], (where, "sat out")
                continue
            assert _bits_equal(got[k], want[k]), (where, "f")
            sb, so = b.state(k), oras[k].state()
            assert nv[k] == oras[k].num_vec() and _decisions(sb) == _decisions(so), where
            live = [s - 1 for s in (so.list_order()[1:] if so.pending else so.list_order())]
            ix = np.ix_(live, live)
            assert np.array_equal(sb.h[ix], so.h[ix]), (where, "h")
            assert np.array_equal(sb.c[live], so.c[live]), (where, "c")
    assert b.dot_weighted() and (n < 64 or b.num_vec().max() >= 3)


# ---- 4. fast sums, every part held exactly --------------------------------------------------------------------------------------

def _worst_line():
    ratio, k, where = WORST
    return f"batch sums (rounded, weighted): worst |red - exact| = {ratio:.3f} u sum|fl(w x) y| against K = {k} there ({where})"


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """At the end of the module: the worst ratio of the weighted sums and the K it was held to, written to
    batch_weights_exact_worst.json beside batch_sums_exact_worst.json."""
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(_worst_line())
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_weights_exact_worst.json"), "w") as fh:
            json.dump({"rounded_weighted": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


class WeightedRun(BatchRun):
    """BatchRun with per-system general weights (batch_weights.system_weights: nonzero and at least a factor 2 from 1 at every
    sentinel, so that a dropped weight cannot hide inside the bound).  Part 1 holds every sum with its FIRST operand x replaced
    by fl(w_sys o x): within gamma(batch_k(n)) * sum|fl(w x) y| of the exact sum in the fast order -- K unchanged, the product's
    first operand is the already rounded fl(w x) -- and to the sequential sum's bits in reference order.  Parts 2 and 3 are
    inherited unchanged."""

    def _device(self, odd_ld):
        super()._device(odd_ld)
        self.wts = BW.system_weights(self.n, self.nsys)
        _, wdev = _rows(self.torch, self.nsys, self.n, self.ld)      # rows as far apart as those of f
        wdev.copy_(self.torch.from_numpy(self.wts))
        self.b.set_dot_weights(wdev)
        assert self.b.dot_weighted()
        self._sys = None

    def _check(self, k, *args):
        self._sys = k
        super()._check(k, *args)

    def _sum(self, what, red, x, y, where):
        a = self.wts[self._sys] * x
        if self.order == self.reference or (self.order == 0 and self.n <= 64):
            want = ordered_dot(a, y)
            assert _bits_equal(np.array([red]), np.array([want])), (what, where, "not the sequential sum's bits", red, want)
            self.ordered_sums += 1
            return
        ex = X.exact_dot(a, y)
        assert math.isfinite(ex), (what, where)
        tot, k = X.abs_dot(a, y), self.k
        err = abs(red - ex)
        assert err <= X.gamma(k) * tot, (what, where, red, ex, err / (X.U * tot) if tot else err, k)
        if tot > 0 and err / (X.U * tot) >= WORST[0]:
            WORST[:] = [err / (X.U * tot), k, f"{what} {where}"]


@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("n", [1, 3, 63, 65, 129, 512, 513, 1025, 4099])
def test_every_part_of_a_weighted_fast_update(torch_cuda, oracle, n, odd_ld):
    for flavor in (0, 1, 2):
        run = _planned_run(WeightedRun(torch_cuda, oracle, flavor, n, SHAPE_MVEC, len(PLAN), odd_ld), seed=n)
        assert run.lengths_differed and run.saw_zero_s and run.saw_after_restart and 0 in run.nolder_no_pending
        if n >= 63:
            assert run.nolder_normed >= set(range(SHAPE_MVEC + 1)), run.nolder_normed      # every sweep count, the full list


@pytest.mark.parametrize("n,flavor", [(X.BATCH_CAP_SHAPES[0], 2), (X.BATCH_CAP_SHAPES[1], 1)], ids=["16383", "16384"])
def test_every_part_of_a_weighted_fast_update_at_the_longest_system(torch_cuda, oracle, n, flavor):
    run = WeightedRun(torch_cuda, oracle, flavor, n, 3, 2, odd_ld=bool(n % 2))
    rngs, prev = [np.random.default_rng([n, k]) for k in range(2)], [None, None]
    for t in range(5):
        inputs = {}
        for k in range(2):
            if t >= k:
                inputs[k] = prev[k] = X.batch_planted_input(n, rngs[k], prev[k])
        run.update(inputs)
    assert run.widest == 3 and run.lengths_differed


@pytest.mark.parametrize("n", [65, 513])
def test_weighted_updates_in_alternating_sum_orders(torch_cuda, oracle, n):
    """The same run with the order changed on the live batch: reference-order updates carry the sequential sums' bits."""
    import nka_amd
    for flavor in (0, 1, 2):
        run = WeightedRun(torch_cuda, oracle, flavor, n, 5, 3, odd_ld=True)
        rngs, prev = [np.random.default_rng([n, k]) for k in range(3)], [None] * 3
        for t in range(9):
            inputs = {}
            for k in range(3):
                inputs[k] = prev[k] = X.batch_planted_input(n, rngs[k], prev[k])
            run.update(inputs, order=nka_amd.SUMS_REFERENCE_ORDER if t % 2 else nka_amd.SUMS_BLOCKED_ROUNDED)
        assert run.ordered_sums > 30 and run.widest == 5


# ---- 5. a zero-weight tail is a shorter system ------------------------------------------------------------------------------

@pytest.mark.parametrize("oname", ["reference", "rounded"])
def test_a_zero_weight_tail_is_a_shorter_system(torch_cuda, oname):
    """vlen = 1025, lengths 1, 64, 511, 513, 1025; w = 1 below the length and 0 from there on, finite garbage of magnitude 1e3 in
    the tail of every input.  Derived, not fitted: fma(+-0, b, acc) = acc for finite b (acc + +-0 = acc in the reference's
    order), and a thread meets its elements in the same order at either length."""
    import nka_amd
    torch = torch_cuda
    order, vlen, mvec = _orders()[oname], 1025, 5
    lengths = [1, 64, 511, 513, 1025]
    nsys = len(lengths)
    W = np.zeros((nsys, vlen))
    for k, ln in enumerate(lengths):
        W[k, :ln] = 1.0
    for flavor in (0, 1, 2):
        rng = np.random.default_rng([5, flavor])
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(order).set_dot_weights(W)      # (host entry)
        short = [nka_amd.nka_batch().init(1, ln, mvec, flavor=flavor).set_sum_order(order) for ln in lengths]
        seqs = [B.Sequence(ln, 500 + 10 * k + flavor) for k, ln in enumerate(lengths)]
        for t in range(mvec + 4):
            host = 1.0e3 * rng.standard_normal((nsys, vlen))
            heads = [s.next() for s in seqs]
            for k, ln in enumerate(lengths):
                host[k, :ln] = heads[k]
            F = torch.from_numpy(host).cuda()
            b.accel_update(F)
            got = F.cpu().numpy()
            assert np.isfinite(got).all()
            for k, ln in enumerate(lengths):
                Fs = torch.from_numpy(heads[k].copy()).cuda().view(1, ln)
                short[k].accel_update(Fs)
                where = (oname, flavor, t, ln)
                _same_system(b, k, short[k], 0, where)
                assert _bits_equal(got[k, :ln], Fs.cpu().numpy()[0]), (where, "f")


# ---- 6. masked entries and s == 0 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oname", ["reference", "rounded"])
def test_masked_entries_stay_out_of_every_sum_and_decision(torch_cuda, oname):
    import nka_amd
    torch = torch_cuda
    order, nsys, n, mvec = _orders()[oname], 4, 700, 8
    for flavor in (0, 1, 2):
        rng = np.random.default_rng([6, flavor])
        W = (rng.random((nsys, n)) >= 0.3).astype(np.float64)
        keep = W != 0
        a, b = [nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(order).set_dot_weights(torch.from_numpy(W).cuda())
                for _ in range(2)]
        last = None
        for t in range(6):
            Xa = rng.standard_normal((nsys, n)) if t < 5 else last.copy()      # the last input: the one before it ...
            Xb = Xa.copy()
            Xa[~keep] = rng.standard_normal(int((~keep).sum()))                # ... up to the masked entries
            Xb[~keep] = 10.0 * rng.standard_normal(int((~keep).sum()))
            last = Xa
            before = [len(a.state(k).list_order()) for k in range(nsys)]
            Fa, Fb = torch.from_numpy(Xa.copy()).cuda(), torch.from_numpy(Xb.copy()).cuda()
            a.accel_update(Fa)
            b.accel_update(Fb)
            ga, gb = Fa.cpu().numpy(), Fb.cpu().numpy()
            assert _bits_equal(ga[keep], gb[keep]), (oname, flavor, t)
            for k in range(nsys):
                st = _same_system(a, k, b, k, (oname, flavor, t, k))
                red = a.reductions(k)
                if t == 5:      # differs from the previous input ONLY at masked entries: s == 0, the system relaxes
                    assert red[0] == 0.0 and not red[1:2 + mvec].any(), (oname, flavor, k, red[:2 + mvec])
                    assert st.pending and len(st.list_order()) == before[k], (oname, flavor, k)
                elif t > 0:
                    assert red[0] > 0.0 and len(st.list_order()) == before[k] + 1, (oname, flavor, t, k)


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["shared", "rows"])
def test_a_weighted_update_is_capturable_from_the_first_call(torch_cuda, form):
    """Captured before the first update, replayed against an eager twin; new values of the same form set between replays reach
    the next replay; setting weights while the stream captures returns NKA_HIP_ESTATE and changes nothing."""
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = 24, 300, 6
    rng = np.random.default_rng(7)
    pick = (lambda w: w[0]) if form == "shared" else (lambda w: w)
    w1, w2 = (torch.from_numpy(np.stack([_general_weights(vlen, rng) for _ in range(nsys)])).cuda() for _ in range(2))
    seqs = [B.Sequence(vlen, 700 + k) for k in range(nsys)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec).set_dot_weights(pick(w1))
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec).set_dot_weights(pick(w1))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        b.accel_update(static)
        rc = b._L.nka_hip_batch_set_dot_weights(b._handle(), C.c_void_p(pick(w2).data_ptr()), 0 if form == "shared" else vlen)
        rc_none = b._L.nka_hip_batch_set_dot_weights(b._handle(), None, 0)
    assert rc == ESTATE and rc_none == ESTATE and b.dot_weighted()
    for t in range(mvec + 6):
        if t == 5:                                           # new values: the next replays run with them
            with torch.cuda.stream(side):
                b.set_dot_weights(pick(w2))
            eager.set_dot_weights(pick(w2))
        Xh = np.stack([s.next() for s in seqs])
        static.copy_(torch.from_numpy(Xh))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = torch.from_numpy(Xh.copy()).cuda()
        eager.accel_update(F)
        assert torch.equal(F, static), (form, t)
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], (form, t)
    plain = nka_amd.nka_batch().init(nsys, vlen, mvec)       # (and the weights did something)
    F = torch.from_numpy(Xh.copy()).cuda()
    plain.accel_update(F)
    assert plain.state_digest(0) != b.state_digest(0)


# ---- 8. refusals and lifecycle -------------------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(torch_cuda):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    nsys, vlen, mvec = 5, 33, 3
    rng = np.random.default_rng(8)
    W0 = np.stack([_general_weights(vlen, rng) for _ in range(nsys)])
    b = nka_amd.nka_batch().init(nsys, vlen, mvec)
    twin = nka_amd.nka_batch().init(nsys, vlen, mvec).set_dot_weights(W0)
    assert not b.dot_weighted() and b.set_dot_weights(torch.from_numpy(W0).cuda()) is b and b.dot_weighted()
    L, h = b._L, b._handle()

    def still_the_twins(calls=2, digests=True):
        for _ in range(calls):
            Xh = rng.standard_normal((nsys, vlen))
            Fa, Fb = torch.from_numpy(Xh.copy()).cuda(), torch.from_numpy(Xh.copy()).cuda()
            b.accel_update(Fa)
            twin.accel_update(Fb)
            assert torch.equal(Fa, Fb)
            for k in range(nsys):
                assert _bits_equal(b.reductions(k), twin.reductions(k))
                assert not digests or b.state_digest(k) == twin.state_digest(k)

    still_the_twins()
    # an entry in the LAST row only: negative, NaN, Inf -- through both entries
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        Wb = np.ones((nsys, vlen))
        Wb[nsys - 1, 7] = bad
        with pytest.raises(NKAError, match=r"\(-1\).*first in row %d at index 7" % (nsys - 1)):
            b.set_dot_weights(Wb)
        with pytest.raises(NKAError, match=r"\(-1\)"):
            b.set_dot_weights(torch.from_numpy(Wb).cuda())
        assert b.dot_weighted()
    ok = torch.ones(nsys * vlen, dtype=torch.float64, device="cuda")
    for ldw in (1, vlen - 1, -1, -vlen):
        assert L.nka_hip_batch_set_dot_weights(h, C.c_void_p(ok.data_ptr()), ldw) == EINVAL, ldw
        assert L.nka_hip_batch_set_dot_weights_host(h, np.ones(nsys * vlen).ctypes.data_as(C.c_void_p), ldw) == EINVAL, ldw
    assert L.nka_hip_batch_set_dot_weights(h, C.c_void_p(ok.data_ptr()), 2 ** 62) == EINVAL      # (no overflow on the way)
    # a device buffer one element too short, in both forms (a buffer of exactly known size: the library's own allocator)
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    ldw = vlen + 3
    for count, form in (((nsys - 1) * ldw + vlen - 1, ldw), (vlen - 1, 0)):
        assert L.nka_hip_vec_alloc(ws, count, C.byref(short)) == 0
        torch.cuda.synchronize()
        assert L.nka_hip_batch_set_dot_weights(h, short, form) == EINVAL, form
        assert b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_vec_free(ws, short) == 0
    assert L.nka_hip_vec_workspace_destroy(ws) == 0
    assert b.dot_weighted()
    still_the_twins()                                        # the previous weighting stayed in force

    # garbage in the padding between rows is never read: accepted, through both entries, and the weights are W1
    W1 = np.stack([_general_weights(vlen, rng) for _ in range(nsys)])
    pad = np.full((nsys, vlen + 3), np.nan)
    pad[:, :vlen] = W1
    twin.set_dot_weights(torch.from_numpy(W1).cuda())
    b.set_dot_weights(torch.from_numpy(pad).cuda()[:, :vlen])
    still_the_twins()
    twin.set_dot_weights(W0)
    b.set_dot_weights(W0)
    b.set_dot_weights(pad[:, :vlen])
    twin.set_dot_weights(W1)
    still_the_twins()
    # the shared form after the per-row form, on a live batch
    b.set_dot_weights(W1[2])
    twin.set_dot_weights(torch.from_numpy(np.tile(W1[2], (nsys, 1))).cuda())
    still_the_twins()

    # what the Python layer refuses before the library is called
    Wt = torch.from_numpy(W0).cuda()
    for wrong in (Wt.float(), Wt.cpu(), Wt[:, :-1], Wt[:-1], Wt[None], torch.ones(nsys, 2 * vlen, dtype=torch.float64, device="cuda")[:, ::2],
                  torch.ones(2 * vlen, dtype=torch.float64, device="cuda")[::2], W0.astype(np.float32), W0[:, :-1], W0[None],
                  np.ones((nsys, 2 * vlen))[:, ::2], W0.tolist(), 1.0):
        with pytest.raises(NKAError, match="batch set_dot_weights:"):
            b.set_dot_weights(wrong)
    assert b.dot_weighted()
    still_the_twins()

    # cleared and restarted: a fresh plain batch
    assert b.set_dot_weights(None) is b and not b.dot_weighted()
    b.restart()
    twin.delete()
    twin = nka_amd.nka_batch().init(nsys, vlen, mvec)
    still_the_twins(3, digests=False)                        # (a restarted block keeps stale entries a fresh one never had)
    # destroy after set, and after set and clear; a NULL handle
    b.set_dot_weights(W0)
    b.delete()
    twin.delete()
    assert L.nka_hip_batch_dot_weighted(None) == EINVAL and L.nka_hip_batch_set_dot_weights(None, None, 0) == EINVAL
