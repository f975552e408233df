"""The solve step of the batched accelerator (nka_hip_batch_accel_step, nka_amd.nka_batch.accel_step): residual norm, stop
rule, update and correction of every system in the one launch of accel_update.

  1 a step is the update: F, state and red[] of a twin that runs accel_update under the mask the host predicts; the mask; X
  2 the norm is the batch's dot product, exactly held (bound: batch_step.norm_bound; teeth: tests/test_batch_step_cpu.py)
  3 the stop rule at its edges
  4 a whole solve captured once and replayed with no host in the loop, against an eager twin
  5 refusals, the step with every optional pointer NULL, independence of nsys / position / alignment of the row of X"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import batch_seq as B
import batch_step as S
import batch_weights as BW
import exact_sums as X
from split_update import _bits_equal, ordered_dot

pytestmark = pytest.mark.gpu

EINVAL = -1
PLANTED = -7.0                     # what fnorm holds before a call: kept by every system inactive on entry
WORST = [0.0, 0, ""]               # worst |fnorm - sqrt(E)| / (u sqrt(E)) seen, the K it was held to, where


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


def _rows(torch, nsys, n, ld, host=None):
    """nsys rows of n doubles, ld apart, inside one allocation: (the whole buffer, the view a batch takes)."""
    raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda") if host is None else torch.from_numpy(host.ravel().copy()).cuda()
    return raw, raw.view(nsys, ld)[:, :n]


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.asarray(a, np.float64)).cuda()


def _pair(nsys, n, mvec, flavor, order, weights=None):
    import nka_amd
    out = []
    for _ in range(2):
        b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(order)
        if weights is not None:
            b.set_dot_weights(weights)
        out.append(b)
    return out


def _same_state(a, b, nsys, where):
    assert np.array_equal(a.num_vec(), b.num_vec()), (where, "num_vec")
    for k in range(nsys):
        assert a.state_digest(k) == b.state_digest(k), (where, k, "digest")
        assert _bits_equal(a.reductions(k), b.reductions(k)), (where, k, "red")


# ---- 1. a step is the update -----------------------------------------------------------------------------------------------------

def _step_against_twin(torch, n, flavor, order, weighted, odd_ld, odd_ldx):
    nsys, mvec, calls = 6, 5, 12
    ld, ldx = _ld(n, odd_ld), _ld(n, odd_ldx)
    wts = BW.system_weights(n, nsys) if weighted else None
    step, twin = _pair(nsys, n, mvec, flavor, order, wts)
    rng = np.random.default_rng([1, n, flavor, int(weighted), ld])
    seqs = [B.Sequence(n, 5000 * n + 10 * k + flavor) for k in range(nsys)]
    (fs_raw, Fs), (ft_raw, Ft) = _rows(torch, nsys, n, ld), _rows(torch, nsys, n, ld)
    xhost = rng.standard_normal((nsys, ldx))                 # (the padding between rows too: it must stay as it is)
    x_raw, Xd = _rows(torch, nsys, n, ldx, xhost)
    fhost = np.zeros((nsys, ld))
    alive = np.ones(nsys, bool)
    mask, tol, fnorm = _i32(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    retired_at = set()
    for t in range(calls):
        where = (n, flavor, order, weighted, ld, ldx, t)
        for op, at, who in (("relax", 5, [1, 4]), ("restart", 8, [2, 5])):      # no pending pair mid-sequence
            if t == at:
                m = _i32(torch, [int(k in who) for k in range(nsys)])
                getattr(step, op)(m)
                getattr(twin, op)(m)
        entry = alive & (t >= np.arange(nsys) % 3)           # staggered starts: with and without a pending pair in one launch
        for k in np.flatnonzero(entry):
            fhost[k, :n] = seqs[k].next()
        # thresholds: none (-1: no norm is below it; the sequences hold zero inputs) but at calls 4 and 9, where the second
        # smallest norm of the entering systems -- formed on the host, so only roughly the device's -- retires about two
        tolh = np.full(nsys, -1.0)
        if t in (4, 9) and entry.sum() >= 3:
            a = fhost[:, :n] * (wts if weighted else 1.0)
            tolh[:] = np.sort(np.sqrt((a * fhost[:, :n]).sum(axis=1))[entry])[1] * (1.0 + 1e-9)
        for raw in (fs_raw, ft_raw):
            raw.copy_(torch.from_numpy(fhost.ravel()))
        mask.copy_(_i32(torch, entry))
        tol.copy_(_f64(torch, tolh))
        fnorm.fill_(PLANTED)
        assert step.accel_step(Fs, Xd, mask, tol, fnorm) is Fs
        fn, got = fnorm.cpu().numpy(), mask.cpu().numpy().astype(bool)
        assert (fn[~entry] == PLANTED).all(), (where, "fnorm of a system inactive on entry")
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
        retired_at |= {t for k in np.flatnonzero(entry & ~want)}
        alive &= ~(entry & ~want)
    assert len(retired_at) >= 1 and alive.any(), (n, flavor, order, weighted, retired_at, alive)
    assert step.num_vec().max() >= 1
    step.delete()
    twin.delete()


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 257, 511, 512, 513, 514, 1025, 4099])
def test_a_step_is_the_update(torch_cuda, n):
    """6 systems, mvec = 5, 12 calls; three flavours, both sum orders, plain and weighted; ld even with ldx odd and ld odd with
    ldx even (either parity of each; with an odd stride the rows alternate between 16-byte aligned and not)."""
    for flavor in (0, 1, 2):
        for order in _orders().values():
            for weighted in (False, True):
                for odd_ld, odd_ldx in ((False, True), (True, False)):
                    _step_against_twin(torch_cuda, n, flavor, order, weighted, odd_ld, odd_ldx)


# ---- 2. the norm ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """At the end of the module: the worst ratio of the norm and the K it was held to, beside batch_sums_exact_worst.json."""
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(f"batch step norm (rounded): worst |fnorm - sqrt(E)| = {ratio:.3f} u sqrt(E) against gamma({k}) + 4u there ({where})")
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_step_exact_worst.json"), "w") as fh:
            json.dump({"rounded": {"worst_err_over_u_sqrt_e": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n", [1, 3, 65, 511, 513, 514, 1025, 4099])
def test_the_norm_is_the_dot_product_of_the_batch(torch_cuda, n, weighted):
    """Planted inputs; 3 systems, 7 calls: the first (no pending pair), later ones, and the calls after a masked relax (system
    1) and a masked restart (system 2).  Fast sums: inside the derived bound.  Reference order: the sequential sum's bits."""
    import nka_amd
    torch = torch_cuda
    nsys, mvec = 3, 3
    wts = BW.system_weights(n, nsys) if weighted else np.ones((nsys, n))
    for oname, order in _orders().items():
        b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=n % 3).set_sum_order(order)
        if weighted:
            b.set_dot_weights(wts)
        rngs, prev = [np.random.default_rng([2, n, k]) for k in range(nsys)], [None] * nsys
        fnorm = _f64(torch, np.zeros(nsys))
        for t in range(7):
            if t == 3:
                b.relax(_i32(torch, [0, 1, 0]))
            if t == 5:
                b.restart(_i32(torch, [0, 0, 1]))
            for k in range(nsys):
                prev[k] = X.batch_planted_input(n, rngs[k], prev[k])
            F = _f64(torch, np.stack(prev))
            pend = [b.state(k).pending for k in range(nsys)]
            b.accel_step(F, fnorm=fnorm)
            fn = fnorm.cpu().numpy()
            for k in range(nsys):
                where = (n, weighted, oname, t, k)
                assert pend[k] == (0 if t == 0 or (t, k) in ((3, 1), (5, 2)) else 1), where
                a = wts[k] * prev[k]
                if oname == "reference":
                    want = np.sqrt(ordered_dot(a, prev[k]))
                    assert _bits_equal(fn[k:k + 1], np.array([want])), (where, fn[k], want)
                    continue
                ok, ratio = S.norm_inside(fn[k], a, prev[k], n)
                print(f"norm {where}: {ratio:.3f} u sqrt(E), bound {S.norm_bound(n) / X.U:.1f} u")
                assert ok, (where, fn[k], ratio, S.norm_bound(n) / X.U)
                if ratio >= WORST[0]:
                    WORST[:] = [ratio, X.batch_k(n), str(where)]
        b.delete()


# ---- 3. the stop rule at its edges ---------------------------------------------------------------------------------------------

def _snapshot(b, nsys):
    return [(b.state_digest(k), b.reductions(k)) for k in range(nsys)]


def _unchanged(b, snap, ks, where):
    for k in ks:
        assert b.state_digest(k) == snap[k][0] and _bits_equal(b.reductions(k), snap[k][1]), (where, k)


@pytest.mark.parametrize("oname", ["reference", "rounded"])
def test_the_stop_rule_at_its_edges(torch_cuda, oname):
    torch = torch_cuda
    nsys, n, mvec, order = 5, 130, 4, _orders()[oname]
    rng = np.random.default_rng(3)
    a, twin = _pair(nsys, n, mvec, 2, order)
    for _ in range(2):                                       # (both with a pending pair)
        Xh = rng.standard_normal((nsys, n))
        a.accel_step(_f64(torch, Xh))
        twin.accel_update(_f64(torch, Xh))
    f0, x0 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    f0[4] = 0.0                                              # a zero row: retires at tol = 0
    r = _f64(torch, np.zeros(nsys))
    Ft = _f64(torch, f0)
    twin.accel_step(Ft, fnorm=r)                             # the probing call: tol = None
    r = r.cpu().numpy()
    assert r[4] == 0.0 and (r[:4] > 0).all()
    snap = _snapshot(a, nsys)
    tol = np.array([r[0], np.nextafter(r[1], 0.0), np.nan, np.inf, 0.0])
    want = np.array([0, 1, 1, 0, 0], np.int32)
    F, Xd, mask, fnorm = _f64(torch, f0), _f64(torch, x0), _i32(torch, np.ones(nsys)), _f64(torch, np.full(nsys, PLANTED))
    a.accel_step(F, Xd, mask, _f64(torch, tol), fnorm)
    assert np.array_equal(mask.cpu().numpy(), want), (oname, mask.cpu().numpy())
    assert _bits_equal(fnorm.cpu().numpy(), r), oname
    got, xg, ft = F.cpu().numpy(), Xd.cpu().numpy(), Ft.cpu().numpy()
    out = want == 0
    assert _bits_equal(got[out], f0[out]) and _bits_equal(xg[out], x0[out]), (oname, "a retired system's rows")
    _unchanged(a, snap, np.flatnonzero(out), (oname, "a retired system's state"))
    assert _bits_equal(got[~out], ft[~out]) and _bits_equal(xg[~out], x0[~out] - ft[~out]), (oname, "the systems that went on")
    for k in np.flatnonzero(~out):
        assert a.state_digest(k) == twin.state_digest(k), (oname, k)
    # tol = +inf retires every ACTIVE system; the one inactive on entry stays as it is, fnorm included
    snap = _snapshot(a, nsys)
    f1 = rng.standard_normal((nsys, n))
    F, mask, fnorm = _f64(torch, f1), _i32(torch, [1, 1, 0, 1, 1]), _f64(torch, np.full(nsys, PLANTED))
    a.accel_step(F, Xd, mask, _f64(torch, np.full(nsys, np.inf)), fnorm)
    assert not mask.cpu().numpy().any() and _bits_equal(F.cpu().numpy(), f1) and _bits_equal(Xd.cpu().numpy(), xg)
    fn = fnorm.cpu().numpy()
    assert fn[2] == PLANTED and (fn[[0, 1, 3, 4]] > 0).all()
    _unchanged(a, snap, range(nsys), (oname, "+inf"))
    a.delete()
    twin.delete()
    # a NaN in one system's f: that system goes on (even under tol = +inf), every other one carries the bits of a clean run
    c, d = _pair(nsys, n, mvec, 2, order)
    for t in range(3):
        Xh = rng.standard_normal((nsys, n))
        Xn = Xh.copy()
        if t == 1:
            Xn[1, 77] = np.nan
        tolh = np.zeros(nsys)
        tolh[1] = np.inf
        Fc, Fd, mc, md = _f64(torch, Xn), _f64(torch, Xh), _i32(torch, np.ones(nsys)), _i32(torch, np.ones(nsys))
        fnorm = _f64(torch, np.zeros(nsys))
        c.accel_step(Fc, None, mc, _f64(torch, tolh if t == 1 else np.zeros(nsys)), fnorm)
        d.accel_step(Fd, None, md, _f64(torch, np.zeros(nsys)))
        assert mc.cpu().numpy().all() and md.cpu().numpy().all(), (oname, t)
        if t == 1:
            assert np.isnan(fnorm.cpu().numpy()[1]) and np.isnan(c.reductions(1)[0])
        others = [0, 2, 3, 4]
        assert _bits_equal(Fc.cpu().numpy()[others], Fd.cpu().numpy()[others]), (oname, t)
        for k in others:
            assert c.state_digest(k) == d.state_digest(k), (oname, t, k)
    c.delete()
    d.delete()


# ---- 4. a whole solve with no host in the loop --------------------------------------------------------------------------------

def test_a_whole_solve_replays_with_no_host_in_the_loop(torch_cuda):
    """[residual; accel_step] captured ONCE, before any update, and replayed SOLVE_REPLAYS times without a synchronise; the
    relative thresholds are formed on the device after the first replay (tol = 0 until then: nothing retires on the way).
    The eager twin runs accel_update under masks the host forms from torch.linalg.vector_norm.  Its norms are not the
    device's bits, so the two runs take the same decisions only where no norm is a close call: both norms are within
    ~1e-15 of the true one (batch_step.norm_bound), and the twin asserts that none of its own lies within SOLVE_GUARD =
    1e-10 of its threshold -- five orders of magnitude more."""
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = S.SOLVE_NSYS, S.SOLVE_VLEN, S.SOLVE_MVEC
    d, eps, bb, x0 = (_f64(torch, a) for a in S.solve_problem())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=S.SOLVE_FLAVOR)
        Xs, Fs = x0.clone(), torch.zeros_like(x0)
        mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        Fs.copy_(S.solve_residual(torch, Xs, d, eps, bb))
        b.accel_step(Fs, Xs, mask, tol, fnorm)
    with torch.cuda.stream(side):
        g.replay()
        torch.mul(fnorm, S.SOLVE_TOL, out=tol)               # the recipe for relative tolerances: a device operation
        for _ in range(S.SOLVE_REPLAYS - 1):
            g.replay()
    torch.cuda.synchronize()

    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=S.SOLVE_FLAVOR)
    Xe, alive, tolh = x0.clone(), np.ones(nsys, bool), np.zeros(nsys)
    retired = np.full(nsys, -1)
    for it in range(S.SOLVE_REPLAYS):
        Fe = S.solve_residual(torch, Xe, d, eps, bb)
        r = torch.linalg.vector_norm(Fe, dim=1).cpu().numpy()
        if it == 1:
            tolh = S.SOLVE_TOL * r0
        assert (np.abs(r - tolh)[alive] > S.SOLVE_GUARD * tolh[alive]).all(), (it, "a close call: the twin cannot judge it")
        stop = alive & (r <= tolh)
        retired[stop] = it
        alive &= ~stop
        m = _i32(torch, alive)
        eager.accel_update(Fe, m)
        Xe = torch.where(m.bool()[:, None], Xe - Fe, Xe)
        if it == 0:
            r0 = r
    assert not alive.any() and len(set(retired.tolist())) >= 3, retired
    assert not mask.cpu().numpy().any(), "every system has retired"
    assert torch.equal(Xs, Xe)
    assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)]
    res = S.solve_residual(np, Xs.cpu().numpy(), *(a.cpu().numpy() for a in (d, eps, bb)))
    assert (np.linalg.norm(res, axis=1) <= 1e-7).all()       # (and it is a solution)


# ---- 5. surface -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_usable(torch_cuda):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    nsys, n, mvec = 5, 33, 3
    rng = np.random.default_rng(5)
    b, twin = _pair(nsys, n, mvec, 0, 0)

    def still_the_twins():
        for _ in range(2):
            Xh = rng.standard_normal((nsys, n))
            Fa, Fb = _f64(torch, Xh), _f64(torch, Xh)
            b.accel_step(Fa)                                 # every optional pointer NULL: the update
            twin.accel_update(Fb)
            assert torch.equal(Fa, Fb)
            _same_state(b, twin, nsys, "twins")

    still_the_twins()
    L, h = b._L, b._handle()
    ld = n + 3
    span = (nsys - 1) * ld + n
    big = _f64(torch, rng.standard_normal(3 * span))
    ok_i, ok_d, ok_n = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(2 * nsys)), _f64(torch, np.zeros(nsys))      # (tol = 0: nothing retires)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)      # noqa: E731
    rows = lambda off: big[off:off + span].as_strided((nsys, n), (ld, 1))      # noqa: E731
    step = L.nka_hip_batch_accel_step

    def accepted(foff, xoff):
        Fc, Xc = rows(foff).clone(), rows(xoff).clone()
        assert step(h, P(big, foff), ld, P(big, xoff), ld, P(ok_i), P(ok_d), P(ok_n)) == 0
        twin.accel_update(Fc)
        assert torch.equal(rows(foff), Fc) and torch.equal(rows(xoff), Xc - Fc) and ok_i.cpu().numpy().all()
        _same_state(b, twin, nsys, "accepted")

    accepted(0, span)                                        # (the arguments below are wrong in ONE respect each)
    f, x = P(big), P(big, span)
    dig = [b.state_digest(k) for k in range(nsys)]
    assert step(h, f, ld, x, ld, None, P(ok_d), P(ok_n)) == EINVAL and b"mask" in L.nka_hip_last_error()
    for off in (0, nsys - 1):                                # fnorm over tol: a threshold would be overwritten while it is read
        assert step(h, f, ld, x, ld, P(ok_i), P(ok_d, off), P(ok_d, nsys - 1)) == EINVAL and b"overlaps" in L.nka_hip_last_error()
    assert step(h, f, ld, x, n - 1, P(ok_i), P(ok_d), P(ok_n)) == EINVAL and b"ldx" in L.nka_hip_last_error()
    assert step(h, f, n - 1, x, ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL
    assert step(h, None, ld, x, ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL
    assert step(None, f, ld, x, ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL
    assert step(h, f, ld, x, 2 ** 62, P(ok_i), P(ok_d), P(ok_n)) == EINVAL
    for off in (0, 1, span - 1, -(span - 1)):                # x over f: the same rows, one element in, the last element either way
        assert step(h, P(big, span), ld, P(big, span + off), ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL, off
        assert b"overlaps" in L.nka_hip_last_error()
    assert dig == [b.state_digest(k) for k in range(nsys)]
    accepted(span, 2 * span)                                 # (adjacent spans do not overlap)
    accepted(span, 0)
    dig = [b.state_digest(k) for k in range(nsys)]
    # each of x, fnorm, tol, active one element short of its span (buffers of exactly known size: the library's allocator)
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    assert nsys % 2 == 1                                     # (the allocator counts doubles: nsys // 2 of them are one int32 short)
    for what, count in (("x", span - 1), ("fnorm", nsys - 1), ("tol", nsys - 1), ("active", nsys // 2)):
        assert L.nka_hip_vec_alloc(ws, count, C.byref(short)) == 0
        torch.cuda.synchronize()
        args = {"x": x, "fnorm": P(ok_n), "tol": P(ok_d), "active": P(ok_i)}
        args[what] = short
        assert step(h, f, ld, args["x"], ld, args["active"], args["tol"], args["fnorm"]) == EINVAL, what
        assert b"shorter" in L.nka_hip_last_error(), (what, L.nka_hip_last_error())
        assert L.nka_hip_vec_free(ws, short) == 0
    assert L.nka_hip_vec_workspace_destroy(ws) == 0
    assert dig == [b.state_digest(k) for k in range(nsys)]
    # what the Python layer refuses before the library is called
    F, Xd = _f64(torch, rng.standard_normal((nsys, n))), _f64(torch, rng.standard_normal((nsys, n)))
    ok_d = ok_d[:nsys]
    for kw in (dict(tol=ok_d), dict(X=Xd.float()), dict(X=Xd[:, :-1]), dict(X=Xd.cpu()), dict(active=ok_i, tol=ok_d[:-1]),
               dict(active=ok_i, tol=ok_d.float()), dict(fnorm=ok_d.cpu()), dict(fnorm=torch.zeros(2 * nsys, dtype=torch.float64, device="cuda")[::2]),
               dict(active=ok_i[:-1]), dict(active=ok_i.long())):
        with pytest.raises(NKAError, match="batch accel_step"):
            b.accel_step(F, **kw)
    with pytest.raises(NKAError, match=r"\(-1\).*overlaps"):
        b.accel_step(F, F)
    assert dig == [b.state_digest(k) for k in range(nsys)]
    still_the_twins()
    b.delete()
    twin.delete()


@pytest.mark.parametrize("oname", ["reference", "rounded"])
def test_results_do_not_depend_on_the_batch_around_a_system(torch_cuda, oname):
    """System 3 of a batch of five against a batch of ONE that runs its inputs, its row of X one element off the alignment of
    the other's: F, X, fnorm, the retirement and the state, bit for bit."""
    import nka_amd
    torch = torch_cuda
    nsys, n, mvec, k, order = 5, 515, 4, 3, _orders()[oname]
    rng = np.random.default_rng(55)
    big = nka_amd.nka_batch().init(nsys, n, mvec, flavor=1).set_sum_order(order)
    one = nka_amd.nka_batch().init(1, n, mvec, flavor=1).set_sum_order(order)
    Xb = _f64(torch, rng.standard_normal((nsys, n + 1)))[:, :n]      # (row stride n + 1 = 516: every row 16-byte aligned)
    x1_raw = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    X1 = x1_raw[1:].view(1, n)                                       # 8 bytes off
    X1.copy_(Xb[k:k + 1])
    assert Xb[k].data_ptr() % 16 == 0 and X1.data_ptr() % 16 == 8
    mb, m1 = _i32(torch, np.ones(nsys)), _i32(torch, [1])
    for t in range(8):
        Xh = rng.standard_normal((nsys, n))
        Fb, F1 = _f64(torch, Xh), _f64(torch, Xh[k:k + 1])
        tb = np.zeros(nsys)
        if t == 6:
            tb[k] = 1e300
        nb, n1 = _f64(torch, np.zeros(nsys)), _f64(torch, [0.0])
        big.accel_step(Fb, Xb, mb, _f64(torch, tb), nb)
        one.accel_step(F1, X1, m1, _f64(torch, tb[k:k + 1]), n1)
        where = (oname, t)
        assert torch.equal(Fb[k], F1[0]) and torch.equal(Xb[k], X1[0]) and torch.equal(nb[k], n1[0]), where
        assert int(mb[k]) == int(m1[0]) == (0 if t >= 6 else 1), where
        assert big.state_digest(k) == one.state_digest(0) and _bits_equal(big.reductions(k), one.reductions(0)), where
    big.delete()
    one.delete()
