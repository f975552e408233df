"""The lane batch (include/nka_hip_batch.h, LANES; nka_amd.nka_batch().init(..., lanes=True)): one lane per system.  Its
contract is equality of BITS with a narrow batch of the same flavour in SUMS_REFERENCE_ORDER -- and hence with the reference --,
so every comparison below is ==.  G = batch_lanes_limits(mvec)[0] places the edges: nsys = 1, G - 1, G, G + 1, 2 G + 3.
  1 bits against the twin       2 bits against the oracle      3 the solve step       4 independence of lane, group and neighbours
  5 graphs from the first call  6 refusals and lifecycle       7 many groups, and slot allocations beyond 2^32 bytes"""
import ctypes as C

import numpy as np
import pytest

import batch_lanes as BL
import batch_step as S
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

EINVAL = -1
PLANTED = -7.0
VLENS = [1, 2, 7, 33, 63, 64]
MVECS = [1, 3, 10, 20, 32]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.asarray(a, np.float64)).cuda()


def _rows(torch, host, ld):
    """nsys rows of vlen doubles, ld apart, inside one allocation padded with PAD: (the whole buffer, the view a batch takes)."""
    nsys, n = host.shape
    full = np.full((nsys, ld), BL.PAD)
    full[:, :n] = host
    raw = torch.from_numpy(full.ravel().copy()).cuda()
    return raw, raw.view(nsys, ld)[:, :n]


def _pair(nsys, vlen, mvec, flavor):
    import nka_amd
    lane = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, lanes=True)
    twin = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    assert lane.kind() == nka_amd.KIND_LANES and twin.kind() == nka_amd.KIND_NARROW and lane.flavor() == twin.flavor() == flavor
    return lane, twin


def _group(mvec):
    import nka_amd
    G, cap = nka_amd.batch_lanes_limits(mvec)
    assert cap == 64 and G == BL.lanes_group(mvec)
    return G


def _same_slots(a, b, k, slots, where):
    for s in slots:
        assert _bits_equal(a.w(k, s), b.w(k, s)), (where, k, s, "w")
        assert _bits_equal(a.v(k, s), b.v(k, s)), (where, k, s, "v")


def _same_everything(a, b, ks, mvec, where):
    assert np.array_equal(a.num_vec(), b.num_vec()), (where, "num_vec")
    for k in ks:
        assert a.state_digest(k) == b.state_digest(k), (where, k, "digest")
        assert _bits_equal(a.reductions(k), b.reductions(k)), (where, k, "red")
        _same_slots(a, b, k, range(1, mvec + 2), where)


def _apply(torch, batch, op, arg, mask, ld):
    """One entry of a script on one batch -> (raw buffer, view) of an update, else (None, None)."""
    m = _i32(torch, mask)
    if op == "update":
        raw, F = _rows(torch, arg, ld)
        batch.accel_update(F, m)
        return raw, F
    (batch.relax if op == "relax" else batch.restart)(m)
    return None, None


# ---- 1. bits against the twin ---------------------------------------------------------------------------------------------

def _run_against_twin(torch, vlen, mvec, flavor, nsys, ld, G, seen):
    lane, twin = _pair(nsys, vlen, mvec, flavor)
    where0 = (vlen, mvec, flavor, nsys, ld)
    pend = np.zeros(nsys, bool)                       # a pending pair at the entry of the next update (host bookkeeping)
    first = [0] * nsys                                # slot of the newest pair
    g0 = range(min(G, nsys))                          # the systems of group 0
    for step, (op, arg, mask) in enumerate(BL.script(vlen, nsys, mvec, 17 * vlen + mvec)):
        where = where0 + (step, op)
        nv0 = lane.num_vec()
        rawl, _ = _apply(torch, lane, op, arg, mask, ld)
        rawt, _ = _apply(torch, twin, op, arg, mask, ld)
        on = mask != 0
        if op != "update":
            pend[on] = False
            if op == "restart":
                for k in np.flatnonzero(on):
                    first[k] = 0
            for k in range(nsys):
                assert lane.state_digest(k) == twin.state_digest(k), (where, k)
            continue
        assert torch.equal(rawl, rawt), (where, "F and its padding")
        nv = lane.num_vec()
        assert np.array_equal(nv, twin.num_vec()), (where, "num_vec")
        for k in range(nsys):
            assert lane.state_digest(k) == twin.state_digest(k), (where, k, "digest")      # (the digest covers red[])
            if on[k]:
                st = lane.state(k)
                _same_slots(lane, twin, k, {st.first} | ({first[k]} if first[k] else set()), where)
                first[k] = st.first
        # what the sequence was built to meet, seen on group 0
        red0 = np.array([lane.reductions(k)[0] for k in g0])
        ran = np.array([on[k] and pend[k] for k in g0])                    # updates that had a pending pair
        relaxed = ran & (red0 == 0.0)
        grew = ran & (red0 != 0.0) & (nv[list(g0)] == nv0[list(g0)] + 1)
        dropped = ran & (red0 != 0.0) & (nv0[list(g0)] < mvec) & (nv[list(g0)] <= nv0[list(g0)])
        full = ran & (nv0[list(g0)] == mvec)
        if len(set(nv[list(g0)].tolist())) > 1:
            seen.add("lengths")
        if relaxed.any() and grew.any():
            seen.add("relax")
        if dropped.any() and grew.any():
            seen.add("drop")
        if full.any():
            seen.add("capacity")
        pend[on] = True
    _same_everything(lane, twin, range(nsys), mvec, where0 + ("end",))
    lane.delete()
    twin.delete()


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("mvec", MVECS)
@pytest.mark.parametrize("vlen", VLENS)
def test_bits_of_the_narrow_twin_in_reference_order(torch_cuda, vlen, mvec, flavor):
    """F with its padding, red[], state, num_vec and digest after every call, the slots a call wrote after that call and every
    slot at the end; nsys at the edges of a group, both row strides."""
    G = _group(mvec)
    seen = set()
    for j, nsys in enumerate(sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 3})):
        _run_against_twin(torch_cuda, vlen, mvec, flavor, nsys, vlen + (j + flavor) % 2, G, seen)
    if vlen >= 7:      # (shorter systems: every difference is dependent, nothing to tell apart)
        assert "lengths" in seen and "relax" in seen, (seen, "the lanes of one group never differed")
        if mvec >= 3:
            assert "drop" in seen, (seen, "no dependence drop beside a lane that had none")
        if vlen > mvec + 1:
            assert "capacity" in seen, (seen, "no list ever filled")


@pytest.mark.parametrize("vlen", [1, 64])
def test_both_row_strides_at_every_group_edge(torch_cuda, vlen):
    """ld = vlen and vlen + 1 at EVERY nsys of test 1 (there the stride alternates from one nsys to the next)."""
    mvec = 10
    G = _group(mvec)
    for nsys in sorted({1, G - 1, G, G + 1, 2 * G + 3}):
        for ld in (vlen, vlen + 1):
            _run_against_twin(torch_cuda, vlen, mvec, 2, nsys, ld, G, set())


# ---- 2. bits against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("mvec", [3, 10])
@pytest.mark.parametrize("vlen", [7, 64])
def test_bits_of_the_oracle(torch_cuda, oracle, vlen, mvec, flavor):
    import nka_amd
    torch = torch_cuda
    nsys = _group(mvec) + 1
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, lanes=True)
    oras = [oracle.OracleNKA(vlen, mvec, flavor) for _ in range(nsys)]
    for step, (op, arg, mask) in enumerate(BL.script(vlen, nsys, mvec, 5 * vlen + mvec)):
        where = (vlen, mvec, flavor, step, op)
        _, F = _apply(torch, b, op, arg, mask, vlen)
        want = None if arg is None else arg.copy()
        for k in np.flatnonzero(mask):
            if op == "update":
                oras[k].accel_update(want[k])
            else:
                (oras[k].relax if op == "relax" else oras[k].restart)()
        if op == "update":
            assert np.array_equal(F.cpu().numpy(), want), where
        nv = b.num_vec()
        for k in range(nsys):
            sb, so = b.state(k), oras[k].state()
            assert nv[k] == oras[k].num_vec() and sb.list_order() == so.list_order() and sb.free_order() == so.free_order(), (where, k)
            assert (sb.subspace, sb.pending) == (so.subspace, so.pending), (where, k)
            live = so.list_order()[1:] if so.pending else so.list_order()
            for slot in so.list_order():
                wo, vo = oras[k].w(slot), oras[k].v(slot)
                if flavor == 2 and slot in live:
                    vo = vo - wo                      # compact storage: v holds fl(v' - w') of a normalised pair
                assert np.array_equal(b.w(k, slot), wo) and np.array_equal(b.v(k, slot), vo), (where, k, slot)
    b.delete()


# ---- 3. the solve step --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("use_x, use_tol, use_fnorm", [(x, t, f) for x in (0, 1) for t in (0, 1) for f in (0, 1)])
def test_a_step_is_the_twins_step(torch_cuda, flavor, use_x, use_tol, use_fnorm):
    """Every combination of X / tol / fnorm the narrow batch accepts (tol needs the mask; without tol the mask is None in
    every other call), residuals that shrink at a rate of their own per system so that the systems of one group retire at
    different calls."""
    torch = torch_cuda
    vlen, mvec = 33, 3
    G = _group(mvec)
    nsys, ld, ldx = G + 1, vlen + 1, vlen + 2
    lane, twin = _pair(nsys, vlen, mvec, flavor)
    rng = np.random.default_rng(11 + flavor)
    rate = 0.2 + 0.7 * rng.random(nsys)
    tolh = np.full(nsys, 1e-3)
    x0 = rng.standard_normal((nsys, vlen))
    state = []
    for b in (lane, twin):
        rawx, Xd = _rows(torch, x0, ldx)
        state.append({"rawx": rawx, "X": Xd, "mask": _i32(torch, np.ones(nsys)), "fnorm": _f64(torch, np.full(nsys, PLANTED))})
    retired_at = np.full(nsys, -1)
    for t in range(14):
        fh = rng.standard_normal((nsys, vlen)) * (rate ** t)[:, None]
        raws = []
        for b, st in zip((lane, twin), state):
            raw, F = _rows(torch, fh, ld)
            masked = use_tol or t % 2 == 0
            b.accel_step(F, st["X"] if use_x else None, st["mask"] if masked else None, _f64(torch, tolh) if use_tol else None,
                         st["fnorm"] if use_fnorm else None)
            raws.append(raw)
        where = (flavor, use_x, use_tol, use_fnorm, t)
        assert torch.equal(raws[0], raws[1]), (where, "F and its padding")
        assert torch.equal(state[0]["rawx"], state[1]["rawx"]), (where, "X and its padding")
        assert torch.equal(state[0]["mask"], state[1]["mask"]), (where, "the mask")
        assert _bits_equal(state[0]["fnorm"].cpu().numpy(), state[1]["fnorm"].cpu().numpy()), (where, "fnorm")
        for k in range(nsys):
            assert lane.state_digest(k) == twin.state_digest(k), (where, k)
        m = state[0]["mask"].cpu().numpy()
        retired_at[(m == 0) & (retired_at < 0)] = t
        if not use_x:
            assert (state[0]["rawx"].view(nsys, ldx)[:, :vlen].cpu().numpy() == x0).all(), (where, "x was written")
        if not use_fnorm:
            assert (state[0]["fnorm"].cpu().numpy() == PLANTED).all()
    if use_tol:
        assert len(set(retired_at[:G].tolist()) - {-1}) >= 3, (retired_at, "the systems of group 0 retired together")
        if use_fnorm:      # a system inactive on entry keeps the norm it retired with
            fn = state[0]["fnorm"].cpu().numpy()
            assert (fn[retired_at >= 0] <= tolh[retired_at >= 0]).all() and (fn > 0).all()
    _same_everything(lane, twin, range(nsys), mvec, ("step", "end"))
    lane.delete()
    twin.delete()


def test_the_stop_rule_at_its_edges(torch_cuda):
    """tol = r, nextafter(r, 0), NaN, +inf and 0 on a zero row, in neighbouring lanes; a retired system keeps every byte."""
    torch = torch_cuda
    nsys, n, mvec = 5, 33, 4
    rng = np.random.default_rng(3)
    a, twin = _pair(nsys, n, mvec, 2)
    for _ in range(2):
        Xh = rng.standard_normal((nsys, n))
        a.accel_step(_f64(torch, Xh))
        twin.accel_update(_f64(torch, Xh))
    f0, x0 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    f0[4] = 0.0
    r = _f64(torch, np.zeros(nsys))
    Ft = _f64(torch, f0)
    twin.accel_step(Ft, fnorm=r)                             # the probing call: tol = None
    r = r.cpu().numpy()
    assert r[4] == 0.0 and (r[:4] > 0).all()
    snap = [(a.state_digest(k), a.reductions(k), [a.w(k, s) for s in range(1, mvec + 2)], [a.v(k, s) for s in range(1, mvec + 2)])
            for k in range(nsys)]
    tol = np.array([r[0], np.nextafter(r[1], 0.0), np.nan, np.inf, 0.0])
    want = np.array([0, 1, 1, 0, 0], np.int32)
    F, Xd, mask, fnorm = _f64(torch, f0), _f64(torch, x0), _i32(torch, np.ones(nsys)), _f64(torch, np.full(nsys, PLANTED))
    a.accel_step(F, Xd, mask, _f64(torch, tol), fnorm)
    assert np.array_equal(mask.cpu().numpy(), want), mask.cpu().numpy()
    assert _bits_equal(fnorm.cpu().numpy(), r)
    got, xg, ft = F.cpu().numpy(), Xd.cpu().numpy(), Ft.cpu().numpy()
    out = want == 0
    assert _bits_equal(got[out], f0[out]) and _bits_equal(xg[out], x0[out]), "a retired system's rows"
    for k in np.flatnonzero(out):
        assert a.state_digest(k) == snap[k][0] and _bits_equal(a.reductions(k), snap[k][1]), k
        for s in range(1, mvec + 2):
            assert _bits_equal(a.w(k, s), snap[k][2][s - 1]) and _bits_equal(a.v(k, s), snap[k][3][s - 1]), (k, s)
    assert _bits_equal(got[~out], ft[~out]) and _bits_equal(xg[~out], x0[~out] - ft[~out]), "the systems that went on"
    for k in np.flatnonzero(~out):
        assert a.state_digest(k) == twin.state_digest(k), k
    # tol = +inf retires every ACTIVE system; the one inactive on entry stays as it is, fnorm included
    f1 = rng.standard_normal((nsys, n))
    digests = [a.state_digest(k) for k in range(nsys)]
    F, mask, fnorm = _f64(torch, f1), _i32(torch, [1, 1, 0, 1, 1]), _f64(torch, np.full(nsys, PLANTED))
    a.accel_step(F, Xd, mask, _f64(torch, np.full(nsys, np.inf)), fnorm)
    assert not mask.cpu().numpy().any() and _bits_equal(F.cpu().numpy(), f1) and _bits_equal(Xd.cpu().numpy(), xg)
    fn = fnorm.cpu().numpy()
    assert fn[2] == PLANTED and (fn[[0, 1, 3, 4]] > 0).all()
    assert digests == [a.state_digest(k) for k in range(nsys)]
    a.delete()
    twin.delete()


def test_a_whole_solve_replays_with_no_host_in_the_loop(torch_cuda):
    """The solve of tests/batch_step.py on its first 64 unknowns (a lane batch holds no longer system; the stencil wraps
    around, so the slice is a problem of the same family): [residual; accel_step] captured ONCE, before any update, replayed
    SOLVE_REPLAYS times; the eager twin is a narrow batch in reference order running the same steps.  Its norms ARE the lane
    batch's bits, so no guard band is needed: every iterate, the mask and every digest are compared with ==."""
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = S.SOLVE_NSYS, 64, S.SOLVE_MVEC
    d, eps, bb, x0 = (_f64(torch, a[:, :vlen] if a.shape[1] > 1 else a) for a in S.solve_problem())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=S.SOLVE_FLAVOR, lanes=True)
        Xs, Fs = x0.clone(), torch.zeros_like(x0)
        mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        Fs.copy_(S.solve_residual(torch, Xs, d, eps, bb))
        b.accel_step(Fs, Xs, mask, tol, fnorm)
    with torch.cuda.stream(side):
        g.replay()
        torch.mul(fnorm, S.SOLVE_TOL, out=tol)
        for _ in range(S.SOLVE_REPLAYS - 1):
            g.replay()
    torch.cuda.synchronize()

    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=S.SOLVE_FLAVOR).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    Xe, me, te, fe = x0.clone(), _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    retired = np.full(nsys, -1)
    for it in range(S.SOLVE_REPLAYS):
        Fe = S.solve_residual(torch, Xe, d, eps, bb).contiguous()
        eager.accel_step(Fe, Xe, me, te, fe)
        if it == 0:
            torch.mul(fe, S.SOLVE_TOL, out=te)
        m = me.cpu().numpy()
        retired[(m == 0) & (retired < 0)] = it
    assert not me.cpu().numpy().any() and len(set(retired.tolist())) >= 3, retired
    assert torch.equal(mask, me) and torch.equal(Xs, Xe) and torch.equal(fnorm, fe) and torch.equal(tol, te)
    assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)]
    res = S.solve_residual(np, Xs.cpu().numpy(), *(a.cpu().numpy() for a in (d, eps, bb)))
    assert (np.linalg.norm(res, axis=1) <= 1e-7).all()       # (and it is a solution)
    b.delete()
    eager.delete()


# ---- 4. independence ----------------------------------------------------------------------------------------------------------

def _snapshot(b, k, mvec):
    return (b.state_digest(k), b.reductions(k).tobytes(), [b.w(k, s).tobytes() for s in range(1, mvec + 2)],
            [b.v(k, s).tobytes() for s in range(1, mvec + 2)])


@pytest.mark.parametrize("mvec", [3, 20])
def test_the_bits_do_not_depend_on_lane_group_or_batch_size(torch_cuda, mvec):
    import nka_amd
    torch = torch_cuda
    vlen, flavor = 33, 2
    G = _group(mvec)
    nsys = 2 * G + 1                                       # system 2 G is the only one of the last group
    spots = sorted({0, G - 1, 2 * G})
    big = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, lanes=True)
    one = nka_amd.nka_batch().init(1, vlen, mvec, flavor=flavor, lanes=True)
    ops = BL.script(vlen, 3, mvec, 99)                     # system 2 of it: a relax inside an update on the way
    rng = np.random.default_rng(5)
    for step, (op, arg, mask3) in enumerate(ops):
        if not mask3[2]:
            continue
        if op == "update":
            X = rng.standard_normal((nsys, vlen))
            X[spots] = arg[2]
            Fb, Fo = _f64(torch, X), _f64(torch, arg[2:3])
            big.accel_update(Fb)
            one.accel_update(Fo)
            for k in spots:
                assert torch.equal(Fb[k], Fo[0]), (mvec, step, k)
        else:
            (big.relax if op == "relax" else big.restart)()
            (one.relax if op == "relax" else one.restart)()
        want = _snapshot(one, 0, mvec)
        for k in spots:
            assert _snapshot(big, k, mvec) == want, (mvec, step, k)
    big.delete()
    one.delete()


def test_inactive_groups_and_neighbours_keep_every_byte(torch_cuda):
    import nka_amd
    torch = torch_cuda
    vlen, mvec = 7, 10
    G = _group(mvec)
    nsys = 3 * G
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
    rng = np.random.default_rng(8)
    for _ in range(4):
        b.accel_update(_f64(torch, rng.standard_normal((nsys, vlen))))
    snap = [_snapshot(b, k, mvec) for k in range(nsys)]
    only = G + 3                                          # group 0 all inactive, group 1 one active system, group 2 all active
    mask = np.zeros(nsys, np.int32)
    mask[only] = 1
    mask[2 * G:] = 1
    Xh = rng.standard_normal((nsys, vlen))
    F, Xd, fnorm = _f64(torch, Xh), _f64(torch, Xh + 1.0), _f64(torch, np.full(nsys, PLANTED))
    b.accel_step(F, Xd, _i32(torch, mask), None, fnorm)
    got, xg, fn = F.cpu().numpy(), Xd.cpu().numpy(), fnorm.cpu().numpy()
    for k in range(nsys):
        if mask[k]:
            assert _snapshot(b, k, mvec) != snap[k] and fn[k] > 0 and not np.array_equal(got[k], Xh[k]), k
        else:
            assert _snapshot(b, k, mvec) == snap[k] and fn[k] == PLANTED, k
            assert np.array_equal(got[k], Xh[k]) and np.array_equal(xg[k], Xh[k] + 1.0), k
    b.delete()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_stays_inside_its_system(torch_cuda, bad):
    """NaN / Inf fed to one system: its lane neighbours on both sides equal their twins of a clean run, and after a restart the
    system carries nothing of what it saw."""
    import nka_amd
    torch = torch_cuda
    vlen, mvec, nsys, k = 33, 3, 7, 3
    dirty, clean = _pair(nsys, vlen, mvec, 2)
    rng = np.random.default_rng(21)
    for t in range(5):
        Xh = rng.standard_normal((nsys, vlen))
        Xn = Xh.copy()
        if t == 2:
            Xn[k, 11] = bad
        Fd, Fc = _f64(torch, Xn), _f64(torch, Xh)
        dirty.accel_update(Fd)
        clean.accel_update(Fc)
        others = [j for j in range(nsys) if j != k]
        assert torch.equal(Fd[others], Fc[others]), (bad, t)
        for j in others:
            assert _snapshot(dirty, j, mvec) == _snapshot(clean, j, mvec), (bad, t, j)
    assert not np.isfinite(dirty.reductions(k)).all()
    mask = np.zeros(nsys, np.int32)
    mask[k] = 1
    dirty.restart(_i32(torch, mask))
    fresh = nka_amd.nka_batch().init(1, vlen, mvec, flavor=2, lanes=True)
    for t in range(mvec + 3):
        Xh = rng.standard_normal((nsys, vlen))
        Fd, Ff = _f64(torch, Xh), _f64(torch, Xh[k:k + 1])
        dirty.accel_update(Fd, _i32(torch, mask))
        fresh.accel_update(Ff)
        assert torch.equal(Fd[k], Ff[0]) and np.isfinite(Fd.cpu().numpy()).all(), (bad, t)
        # (not the digest: a restart leaves the dead entries of h and c as they were, as in the reference)
        sd, sf = dirty.state(k), fresh.state(0)
        assert sd.list_order() == sf.list_order() and sd.free_order() == sf.free_order(), (bad, t)
        assert np.isfinite(dirty.reductions(k)).all() and _bits_equal(dirty.reductions(k), fresh.reductions(0)), (bad, t)
        live = [s - 1 for s in sd.list_order()[1:]]
        assert np.array_equal(sd.h[np.ix_(live, live)], sf.h[np.ix_(live, live)]), (bad, t)
        for s in sd.list_order():
            assert _bits_equal(dirty.w(k, s), fresh.w(0, s)) and _bits_equal(dirty.v(k, s), fresh.v(0, s)), (bad, t, s)
    for b in (dirty, clean, fresh):
        b.delete()


# ---- 5. graphs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["update", "step"])
def test_a_graph_captured_before_the_first_update_replays_through_growth_and_drops(torch_cuda, entry):
    import nka_amd
    torch = torch_cuda
    vlen, mvec = 7, 10                                     # (7 unknowns: dependence drops from the eighth update on)
    nsys = _group(mvec) + 1
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
        Fs, Xs = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda"), torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        ms, fns = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys))
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
    Xe, fne = torch.zeros_like(Xs), torch.zeros_like(fns)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        if entry == "update":
            b.accel_update(Fs, ms)
        else:
            b.accel_step(Fs, Xs, ms, None, fns)
    rng = np.random.default_rng(13)
    nvs = []
    for t in range(mvec + 6):
        Xh = rng.standard_normal((nsys, vlen))
        mh = (rng.random(nsys) < 0.8).astype(np.int32)
        if t == 6:
            with torch.cuda.stream(side):
                b.set_vec_tol(0.5)                           # applies to the replays that follow
            eager.set_vec_tol(0.5)
        with torch.cuda.stream(side):
            Fs.copy_(_f64(torch, Xh))
            ms.copy_(_i32(torch, mh))
            g.replay()
        torch.cuda.synchronize()
        Fe, me = _f64(torch, Xh), _i32(torch, mh)
        if entry == "update":
            eager.accel_update(Fe, me)
        else:
            eager.accel_step(Fe, Xe, me, None, fne)
        assert torch.equal(Fs, Fe) and torch.equal(Xs, Xe) and torch.equal(fns, fne), (entry, t)
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], (entry, t)
        nvs.append(b.num_vec().copy())
    nvs = np.array(nvs)
    assert nvs.max() >= 4 and (np.diff(nvs, axis=0) < 0).any(), "the replays saw neither growth nor a drop"
    plain = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)      # ... and set_vec_tol did apply: without it the lists differ
    rng = np.random.default_rng(13)
    for t in range(mvec + 6):
        Xh = rng.standard_normal((nsys, vlen))
        mh = (rng.random(nsys) < 0.8).astype(np.int32)
        plain.accel_update(_f64(torch, Xh), _i32(torch, mh))
    assert not np.array_equal(plain.num_vec(), b.num_vec())
    for x in (b, eager, plain):
        x.delete()


# ---- 6. refusals and lifecycle ------------------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(torch_cuda):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    L = nka_amd.nka_batch()._L
    for warm in _pair(70, 33, 10, 2):      # (code objects loaded and torch's pool grown BEFORE free memory is read, also when run alone)
        warm.accel_update(_f64(torch, np.ones((70, 33))))
        warm.w(0, 1)
        warm.delete()
    held = [_f64(torch, np.ones((70, 33))) for _ in range(8)] + [_i32(torch, np.ones(70))]
    del held
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    h = C.c_void_p()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nsys, vlen, mvec in ((8, 65, 5), (8, 64, 33), (0, 64, 5), (8, 0, 5), (8, 64, 0)):
        assert L.nka_hip_batch_create_lanes(C.byref(h), nsys, vlen, mvec, 0.01, nka_amd.FLAVOR_DEFAULT, 0, stream) == EINVAL, (nsys, vlen, mvec)
        assert h.value is None and L.nka_hip_last_error()
        with pytest.raises(NKAError):
            nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
    assert L.nka_hip_batch_create_lanes(C.byref(h), 8, 65, 5, 0.01, nka_amd.FLAVOR_DEFAULT, 0, stream) == EINVAL
    assert b"nka_hip_batch_create)" in L.nka_hip_last_error(), "the refusal names the entry to use instead"
    with pytest.raises(NKAError, match="wide"):
        nka_amd.nka_batch().init(8, 64, 5, lanes=True, wide=True)
    with pytest.raises(NKAError, match="binary32"):
        nka_amd.nka_batch().init(8, 64, 5, lanes=True, storage=nka_amd.STORE_F32)
    assert L.nka_hip_batch_lanes_limits(0, None, None) == EINVAL and L.nka_hip_batch_lanes_limits(33, None, None) == EINVAL
    assert L.nka_hip_batch_kind(None) < 0
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "a refused creation left something allocated"

    nsys, vlen, mvec = 70, 33, 10
    a, twin = _pair(nsys, vlen, mvec, 2)
    never = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=2, lanes=True)      # one that never refused anything
    assert a.kind() == nka_amd.KIND_LANES and not a.is_wide() and a.storage() == nka_amd.STORE_F64
    assert L.nka_hip_batch_kind(a._h) == 2 and L.nka_hip_batch_is_wide(a._h) == 0
    wide = nka_amd.nka_batch().init(2, 64, 3, wide=True)
    assert wide.kind() == nka_amd.KIND_WIDE and twin.kind() == nka_amd.KIND_NARROW
    wide.delete()
    assert a.vector_bytes() == BL.vector_bytes(vlen, mvec, nsys) == 16 * (mvec + 1) * vlen * _group(mvec) * -(-nsys // _group(mvec))
    rng = np.random.default_rng(2)
    w = _f64(torch, np.ones((nsys, vlen)))
    lens = _i32(torch, np.full(nsys, vlen))
    hostw, hostl = np.ones((nsys, vlen)), np.full(nsys, vlen, np.int32)

    def refusals():
        assert L.nka_hip_batch_set_dot_weights(a._h, C.c_void_p(w.data_ptr()), vlen) == EINVAL and b"nka_hip_batch_create" in L.nka_hip_last_error()
        assert L.nka_hip_batch_set_dot_weights_host(a._h, C.c_void_p(hostw.ctypes.data), vlen) == EINVAL
        assert L.nka_hip_batch_set_lengths(a._h, C.c_void_p(lens.data_ptr())) == EINVAL and b"nka_hip_batch_create" in L.nka_hip_last_error()
        assert L.nka_hip_batch_set_lengths_host(a._h, hostl.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL
        for order in (nka_amd.SUMS_BLOCKED, nka_amd.SUMS_BLOCKED_ROUNDED):
            assert L.nka_hip_batch_set_sum_order(a._h, order) == EINVAL and b"REFERENCE_ORDER" in L.nka_hip_last_error()
            with pytest.raises(NKAError):
                a.set_sum_order(order)
        for call in (lambda: a.set_dot_weights(w), lambda: a.set_dot_weights(hostw), lambda: a.set_lengths(lens), lambda: a.set_lengths(hostl)):
            with pytest.raises(NKAError):
                call()
        assert not a.dot_weighted() and not a.has_lengths()
        # spans one element short, for f and for x; tol without a mask; x overlapping f
        # (a buffer of exactly known size: the library's allocator)
        good = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        ws, short = C.c_void_p(), C.c_void_p()
        assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
        assert L.nka_hip_vec_alloc(ws, nsys * vlen - 1, C.byref(short)) == 0
        torch.cuda.synchronize()
        assert L.nka_hip_batch_accel_update(a._h, short, vlen, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_batch_accel_step(a._h, short, vlen, None, 0, None, None, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_batch_accel_step(a._h, C.c_void_p(good.data_ptr()), vlen, short, vlen, None, None, None) == EINVAL
        assert b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_vec_free(ws, short) == 0 and L.nka_hip_vec_workspace_destroy(ws) == 0
        assert L.nka_hip_batch_accel_step(a._h, C.c_void_p(good.data_ptr()), vlen, None, 0, None, C.c_void_p(w.data_ptr()), None) == EINVAL
        assert L.nka_hip_batch_accel_step(a._h, C.c_void_p(good.data_ptr()), vlen, C.c_void_p(good.data_ptr()), vlen, None, None, None) == EINVAL
        assert L.nka_hip_batch_accel_update(a._h, C.c_void_p(good.data_ptr()), vlen - 1, None) == EINVAL
        a.set_sum_order(nka_amd.SUMS_REFERENCE_ORDER).set_sum_order(nka_amd.SUMS_AUTO)      # both mean the reference order

    for t in range(6):
        refusals()
        Xh = rng.standard_normal((nsys, vlen))
        Fa, Ft, Fn = _f64(torch, Xh), _f64(torch, Xh), _f64(torch, Xh)
        a.accel_update(Fa)
        twin.accel_update(Ft)
        never.accel_update(Fn)
        assert torch.equal(Fa, Ft) and torch.equal(Fa, Fn), t
    _same_everything(a, twin, range(nsys), mvec, "after refusals")
    _same_everything(a, never, range(nsys), mvec, "after refusals, against a batch that never refused")
    a.set_stream(torch.cuda.current_stream().cuda_stream)
    for b in (a, twin, never):
        b.delete()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "destroy left something allocated"


# ---- 7. many groups, and slot allocations beyond 2^32 bytes -------------------------------------------------------------------

def test_a_grid_of_more_than_a_thousand_groups_with_a_ragged_last_one(torch_cuda):
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = 70001, 8, 3
    G = _group(mvec)
    assert -(-nsys // G) > 1000 and nsys % G != 0
    sample = sorted({0, nsys - 1} | {g * G + d for g in np.linspace(1, nsys // G, 10).astype(int) for d in (-1, 0)})
    big = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
    twin = nka_amd.nka_batch().init(len(sample), vlen, mvec).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    idx = torch.tensor(sample, dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(4)
    for t in range(mvec + 4):
        F = torch.randn(nsys, vlen, dtype=torch.float64, device="cuda", generator=g)
        Ft = F[idx].clone()
        big.accel_update(F)
        twin.accel_update(Ft)
        assert torch.equal(F[idx], Ft), t
        nv = big.num_vec()
        assert np.array_equal(nv[sample], twin.num_vec()) and (nv == nv[0]).all(), t
    for j, k in enumerate(sample):
        assert _snapshot(big, k, mvec) == _snapshot(twin, j, mvec), k
    big.delete()
    twin.delete()


def test_slot_allocations_beyond_4_gib(torch_cuda):
    """w and v each pass 2^32 bytes (tests/batch_lanes.py: large_shape, held by the CPU test): nine systems run -- system 0, the
    last one, the group on the boundary and its neighbours --, every other one is masked; the nine equal a nine-system twin
    after every call, and the masked witnesses where a byte offset that lost its upper half would land stay fresh."""
    import nka_amd
    torch = torch_cuda
    sh = BL.large_shape()
    nsys, vlen, mvec, act = sh["nsys"], sh["vlen"], sh["mvec"], sh["active"]
    assert sh["G"] == _group(mvec) and len(act) <= BL.MAX_ACTIVE
    need = sum(BL.large_bytes(sh).values())
    free, total = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip(f"{free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 8 GiB")
    big = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
    assert big.vector_bytes() == BL.vector_bytes(vlen, mvec, nsys) and big.vector_bytes() // 2 > 2 ** 32
    twin = nka_amd.nka_batch().init(len(act), vlen, mvec).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    fresh = nka_amd.nka_batch().init(1, vlen, mvec, lanes=True).state_digest(0)
    mask = torch.zeros(nsys, dtype=torch.int32, device="cuda")
    idx = torch.tensor(act, dtype=torch.int64, device="cuda")
    mask[idx] = 1
    F = torch.full((nsys, vlen), BL.PAD, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(6)
    for t in range(mvec + 3):
        Xh = rng.standard_normal((len(act), vlen))
        F[idx] = _f64(torch, Xh)
        Ft = _f64(torch, Xh)
        big.accel_update(F, mask)
        twin.accel_update(Ft)
        assert torch.equal(F[idx], Ft), t
        for j, k in enumerate(act):
            assert big.state_digest(k) == twin.state_digest(j), (t, k)
            s = big.state(k).first
            assert _bits_equal(big.w(k, s), twin.w(j, s)) and _bits_equal(big.v(k, s), twin.v(j, s)), (t, k)
    for j, k in enumerate(act):
        assert _snapshot(big, k, mvec) == _snapshot(twin, j, mvec), k
    F[idx] = BL.PAD
    assert bool((F == BL.PAD).all()), "a row of a masked system was written"
    nv = big.num_vec()
    zero = np.zeros(vlen).tobytes()
    for k in sh["witnesses"]:
        assert nv[k] == 0 and big.state_digest(k) == fresh, k
        for s in range(1, mvec + 2):
            assert big.w(k, s).tobytes() == zero and big.v(k, s).tobytes() == zero, (k, s)
    big.delete()
    twin.delete()
