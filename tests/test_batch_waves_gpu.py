"""The wave batch (include/nka_hip_batch.h, WAVES; nka_amd.nka_batch().init(..., waves=True)): one wavefront per system, four
systems per workgroup, on the narrow batch's storage.  Its sums carry bits of their own -- two fma per lane and 128-element
tile, then a six-level butterfly: K = batch_waves.waves_k(n) = 2 ceil(n / 128) + 6 -- so the contract is the numerical one of
SUMS_BLOCKED_ROUNDED, held in three layers, and everything that is not a sum is held with ==.
  1 three layers after every update (test_batch_sums_exact_gpu.BatchRun with this kind's K): the sums against exact sums, the
    scalar step on the device's own sums against the oracle, the elementwise statements against numpy
  2 independence of nsys, position, wavefront, neighbours and row alignment     3 the solve step against a twin under host masks
  4 a whole solve captured before the first update                                5 limits, refusals, lifecycle
  6 slot allocations beyond 2^32 bytes"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import batch_seq as B
import batch_step as S
import batch_waves as BWV
import exact_sums as X
import test_batch_sums_exact_gpu as T
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

EINVAL = -1
PLANTED = -7.0
WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|xy|) seen, the K it was held to, where


def _worst_line():
    ratio, k, where = WORST
    return f"wave batch sums: worst |red - exact| = {ratio:.3f} u sum|xy| against K = {k} there ({where})"


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """At the end of the module: the worst ratio of the wave sums and the K it was held to -> batch_waves_exact_worst.json."""
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(_worst_line())
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_waves_exact_worst.json"), "w") as fh:
            json.dump({"waves": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def CAP():
    group, cap = BWV.limits()
    assert group == BWV.GROUP and cap >= 128 and cap & (cap - 1) == 0
    return cap


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.asarray(a, np.float64)).cuda()


def _rows(torch, host, ld):
    """nsys rows of vlen doubles, ld apart, inside one allocation padded with PAD: (the whole buffer, the view a batch takes)."""
    nsys, n = host.shape
    full = np.full((nsys, ld), BWV.PAD)
    full[:, :n] = host
    raw = torch.from_numpy(full.ravel().copy()).cuda()
    return raw, raw.view(nsys, ld)[:, :n]


def _ld(n, odd):
    return n + (1 - n % 2 if odd else n % 2)      # the smallest odd / even row stride that holds a row


def _waves(nsys, vlen, mvec, flavor=2):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, waves=True)
    assert b.kind() == nka_amd.KIND_WAVES == 3 and not b.is_wide() and b.flavor() == flavor
    return b


def _snapshot(b, k, mvec):
    return (b.state_digest(k), b.reductions(k).tobytes(), [b.w(k, s).tobytes() for s in range(1, mvec + 2)],
            [b.v(k, s).tobytes() for s in range(1, mvec + 2)])


# ---- 1. the three layers ------------------------------------------------------------------------------------------------------------

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
    ratio = err / (X.U * tot) if tot else err
    print(f"  {what} {where}: |red - exact| = {ratio:.3f} u sum|xy|, K = {k}")
    assert err <= X.gamma(k) * tot, (what, where, red, ex, ratio, k)
    if tot > 0 and ratio >= WORST[0]:
        WORST[:] = [ratio, k, f"{what} {where}"]


class WavesRun(T.BatchRun):
    """BatchRun on a wave batch: the sums are held to waves_k(n); layers 2 and 3 are inherited unchanged."""

    def __init__(self, torch, oracle, flavor, n, mvec, nsys, odd_ld=False):
        super().__init__(torch, oracle, flavor, n, mvec, nsys, odd_ld)
        self.k = BWV.waves_k(n)

    def _device(self, odd_ld):
        import nka_amd
        torch, n, nsys, ld = self.torch, self.n, self.nsys, self.ld
        self.b = _waves(nsys, n, self.m, self.flavor)
        self.order, self.orders_met = nka_amd.SUMS_BLOCKED_ROUNDED, set()
        self.reference = nka_amd.SUMS_REFERENCE_ORDER
        self.raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda")
        self.F = self.raw.view(nsys, ld)[:, :n]
        align = [(self.raw.data_ptr() + 8 * k * ld) % 16 for k in range(nsys)]
        if odd_ld:
            assert ld % 2 == 1 and align == [8 * (k % 2) for k in range(nsys)], align      # odd rows: 8-byte aligned only
        else:
            assert ld % 2 == 0 and not any(align), align                                    # every row 16-byte aligned

    def _sum(self, what, red, x, y, where):
        _hold(what, red, x, y, self.k, where)


def _planned_run(run, seed):
    """test_batch_sums_exact_gpu._planned_run with this kind's sentinels; system k follows PLAN[k % 6]: six different starting
    delays in one launch, a repeated input (s == 0), a masked relax and a masked restart each."""
    n, rngs, prev = run.n, [np.random.default_rng([seed, k]) for k in range(run.nsys)], [None] * run.nsys
    plan = [T.PLAN[k % len(T.PLAN)] for k in range(run.nsys)]
    for t in range(T.SHAPE_CALLS):
        steps = {k: t - plan[k][0] for k in range(run.nsys) if t >= plan[k][0]}
        relax = [k for k, j in steps.items() if j == plan[k][1]]
        restart = [k for k, j in steps.items() if j == plan[k][3]]
        if relax:
            run.relax(relax)
        if restart:
            run.restart(restart)
        inputs = {}
        for k, j in steps.items():
            inputs[k] = prev[k].copy() if j == plan[k][2] else BWV.planted_input(n, rngs[k], prev[k])
            prev[k] = inputs[k]
        run.update(inputs)
    return run


def _shape_ids():
    return ["1", "2", "3", "127", "128", "129", "255", "257", "1027", "cap-1", "cap"]


def _vlen(which, cap):
    """1027 is eight tiles and a pair and a half; where the measured cap lies below it, the same shape one tile short of the cap."""
    return {"cap-1": cap - 1, "cap": cap, "1027": BWV.several_tiles(cap)}.get(which) or int(which)


@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("mvec", BWV.MVECS)
@pytest.mark.parametrize("which", _shape_ids())
def test_every_part_of_a_wave_update(torch_cuda, oracle, CAP, which, mvec, flavor, odd_ld):
    """Eleven systems (the last workgroup has one absent wavefront), six starting delays in one launch."""
    n = _vlen(which, CAP)
    run = _planned_run(WavesRun(torch_cuda, oracle, flavor, n, mvec, BWV.NSYS, odd_ld), seed=1000 * mvec + n)
    assert run.lengths_differed and run.saw_zero_s and run.saw_after_restart and 0 in run.nolder_no_pending
    if n >= 63:                                              # (shorter systems cannot hold that many independent differences)
        assert run.widest == mvec, run.widest
        if mvec == T.SHAPE_MVEC:
            T._assert_planned_coverage(run)


@pytest.mark.parametrize("flavor", [0, 2])
def test_every_older_count_up_to_the_largest_subspace(torch_cuda, oracle, flavor):
    """Fresh planted inputs in 129 dimensions stay independent: the older count visits 0..32, i.e. every group count of the sweep
    of four and the re-read beyond the list at every residue; system k starts k % 3 calls late, odd rows are 8-byte aligned."""
    n, mvec = BWV.WIDTH_SHAPE
    run = WavesRun(torch_cuda, oracle, flavor, n, mvec, BWV.NSYS, odd_ld=True)
    rngs, prev = [np.random.default_rng([n, k]) for k in range(run.nsys)], [None] * run.nsys
    for t in range(mvec + 4):
        inputs = {}
        for k in range(run.nsys):
            if t >= k % 3:
                inputs[k] = prev[k] = BWV.planted_input(n, rngs[k], prev[k])
        run.update(inputs)
    assert run.widest == mvec == 32 and run.nolder_normed == set(range(mvec + 1)), run.nolder_normed
    assert run.lengths_differed


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_non_finite_input_in_one_system(torch_cuda, oracle, bad, flavor):
    """A NaN / an Inf in one system's f: its sums are NaN / Inf exactly where the exact sums are, its scalar step and its
    elementwise statements are the reference's on those sums; the other systems -- its three neighbours in the workgroup
    among them -- are held as always."""
    n, m, nsys, ill = 257, 3, 6, 1
    run = WavesRun(torch_cuda, oracle, flavor, n, m, nsys, odd_ld=False)
    rngs, prev = [np.random.default_rng([11, k]) for k in range(nsys)], [None] * nsys
    for t in range(7):
        inputs = {}
        for k in range(nsys):
            inputs[k] = prev[k] = BWV.planted_input(n, rngs[k], prev[k])
        if t == 3:
            inputs[ill][5] = bad
        run.update(inputs)
    assert np.isnan(run.rows[ill]).any() and np.isfinite(np.delete(run.rows, ill, axis=0)).all()


def test_scalar_step_through_capacity_drops_and_dependence(torch_cuda, oracle):
    """batch_seq.Sequence (fresh, dependent, repeated and zero inputs) at mvec = 3: dependence drops and capacity drops."""
    vlen, nsys, mvec = 129, 5, 3
    run = WavesRun(torch_cuda, oracle, 2, vlen, mvec, nsys, odd_ld=True)
    seqs = [B.Sequence(vlen, 129001 + k) for k in range(nsys)]
    for t in range(2 * mvec + 16):
        run.update({k: seq.next() for k, seq in enumerate(seqs)})
    assert run.widest == mvec and any(gone for _, _, gone in run.outcomes)


# ---- 2. independence --------------------------------------------------------------------------------------------------------------

IND_VLEN, IND_MVEC, IND_CALLS = 257, 3, 7


def _ind_inputs():
    rng, prev, out = np.random.default_rng(77), None, []
    for t in range(IND_CALLS):
        prev = prev.copy() if t == 4 else BWV.planted_input(IND_VLEN, rng, prev)      # (call 4 repeats call 3: s == 0)
        out.append(prev)
    return out


def _ind_run(torch, nsys, pos, odd_ld, others):
    """The system at `pos` of a batch of nsys runs _ind_inputs(); the others are masked, run inputs of their own, or are fed NaN /
    Inf -> per call: the system's row, red[], digest and every slot."""
    b = _waves(nsys, IND_VLEN, IND_MVEC)
    ld = _ld(IND_VLEN, odd_ld)
    rng = np.random.default_rng([5, nsys, pos])
    trace = []
    for t, x in enumerate(_ind_inputs()):
        host = rng.standard_normal((nsys, IND_VLEN))
        if others in ("nan", "inf") and t >= 2:
            host[:, 7] = np.nan if others == "nan" else np.inf
        host[pos] = x
        mask = np.ones(nsys, np.int32)
        if others == "masked":
            mask[:] = 0
            mask[pos] = 1
        raw, F = _rows(torch, host, ld)
        b.accel_update(F, _i32(torch, mask))
        got = raw.view(nsys, ld).cpu().numpy()
        assert (got[:, IND_VLEN:] == BWV.PAD).all(), "the padding between two rows was written"
        if others == "masked":
            keep = np.arange(nsys) != pos
            assert _bits_equal(got[keep, :IND_VLEN], host[keep]), "a masked neighbour's row was written"
        trace.append((got[pos, :IND_VLEN].tobytes(),) + _snapshot(b, pos, IND_MVEC))
    if others in ("nan", "inf"):
        assert np.isfinite(got[pos, :IND_VLEN]).all() and np.isfinite(b.reductions(pos)).all()
        assert not np.isfinite(np.delete(got[:, :IND_VLEN], pos, axis=0)).all() or nsys == 1
    b.delete()
    return trace


@pytest.fixture(scope="module")
def ind_reference(torch_cuda):
    return _ind_run(torch_cuda, 1, 0, False, "active")


@pytest.mark.parametrize("others", ["active", "masked", "nan", "inf"])
@pytest.mark.parametrize("nsys", [1, 4, 5, 9])
def test_the_bits_do_not_depend_on_the_batch_around_a_system(torch_cuda, ind_reference, nsys, others):
    """Every position 0 ... nsys - 1 (every wavefront of a full, a ragged and a lone workgroup), both row alignments."""
    for pos in range(nsys):
        for odd_ld in (False, True):
            assert _ind_run(torch_cuda, nsys, pos, odd_ld, others) == ind_reference, (nsys, pos, odd_ld, others)


# ---- 3. the solve step ------------------------------------------------------------------------------------------------------------

STEP_NSYS, STEP_MVEC, STEP_CALLS, STEP_TOL = 7, 3, 12, 1.0e-3


def _step_inputs(n, flavor):
    """-> per call the rows of f: system k's residual shrinks at a rate of its own, so thresholds retire systems mid-sequence."""
    rng = np.random.default_rng([31, n, flavor])
    rate = 0.15 + 0.1 * np.arange(STEP_NSYS)
    return [rng.standard_normal((STEP_NSYS, n)) * (rate ** t)[:, None] for t in range(STEP_CALLS)], rng.standard_normal((STEP_NSYS, n))


def step_retirements(n, flavor):
    """Host prediction (numpy norms; no call here is close) of the call at which each system retires, -1: never."""
    fs, _ = _step_inputs(n, flavor)
    out = np.full(STEP_NSYS, -1)
    for t, f in enumerate(fs):
        r = np.sqrt((f * f).sum(axis=1))
        out[(r <= STEP_TOL) & (out < 0)] = t
    return out


@pytest.mark.parametrize("odd_ldx", [False, True], ids=["ldx-even", "ldx-odd"])
@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("n", BWV.STEP_LENGTHS)
def test_a_step_is_the_update_under_the_mask_its_own_norm_predicts(torch_cuda, CAP, n, flavor, odd_ld, odd_ldx):
    torch = torch_cuda
    n = min(n, BWV.several_tiles(CAP))                      # (1027 where the cap allows it)
    nsys, mvec, ld, ldx = STEP_NSYS, STEP_MVEC, _ld(n, odd_ld), _ld(n, odd_ldx)
    a, twin = _waves(nsys, n, mvec, flavor), _waves(nsys, n, mvec, flavor)
    fs, x0 = _step_inputs(n, flavor)
    tolh = np.full(nsys, STEP_TOL)
    rawx, Xd = _rows(torch, x0, ldx)
    xh = np.full((nsys, ldx), BWV.PAD)
    xh[:, :n] = x0
    mask, tol = _i32(torch, np.ones(nsys)), _f64(torch, tolh)
    fnorm = _f64(torch, np.full(nsys, PLANTED))
    alive, fn_prev, retired_at = np.ones(nsys, bool), np.full(nsys, PLANTED), np.full(nsys, -1)
    bound = X.gamma(BWV.waves_k(n)) + 4.0 * X.U
    for t, fh in enumerate(fs):
        where = (n, flavor, ld, ldx, "call", t)
        rawa, Fa = _rows(torch, fh, ld)
        a.accel_step(Fa, Xd, mask, tol, fnorm)
        fn = fnorm.cpu().numpy()
        assert _bits_equal(fn[~alive], fn_prev[~alive]), (where, "fnorm of a system inactive on entry")
        for k in np.flatnonzero(alive):                      # the narrow step test's argument with this kind's K
            want = math.sqrt(X.exact_dot(fh[k], fh[k]))
            print(f"  fnorm {where} system {k}: {abs(fn[k] - want) / (X.U * want) if want else 0.0:.3f} u")
            assert abs(fn[k] - want) <= bound * want, (where, k, fn[k], want)
        stop = alive & (fn <= tolh)                          # the mask the host predicts from the step's own fnorm and tol
        retired_at[stop] = t
        alive = alive & ~stop
        assert np.array_equal(mask.cpu().numpy(), alive.astype(np.int32)), (where, "the mask")
        rawt, Ft = _rows(torch, fh, ld)
        twin.accel_update(Ft, _i32(torch, alive))
        assert torch.equal(rawa, rawt), (where, "F and its padding")
        out = Ft.cpu().numpy()
        with np.errstate(all="ignore"):
            xh[alive, :n] = xh[alive, :n] - out[alive]
        assert _bits_equal(rawx.view(nsys, ldx).cpu().numpy(), xh), (where, "X and its padding")
        assert np.array_equal(a.num_vec(), twin.num_vec()), where
        for k in range(nsys):
            assert a.state_digest(k) == twin.state_digest(k), (where, k)
            assert _bits_equal(a.reductions(k), twin.reductions(k)), (where, k)
        fn_prev = fn
    assert np.array_equal(retired_at, step_retirements(n, flavor)), (retired_at, "not the retirements the CPU test looked at")
    for k in range(nsys):
        assert _snapshot(a, k, mvec) == _snapshot(twin, k, mvec), k
    a.delete()
    twin.delete()


def test_the_stop_rule_at_its_edges_and_the_all_null_step(torch_cuda):
    """tol = r, nextafter(r, 0), NaN, +inf and 0 on a zero row, in the wavefronts of two workgroups; a retired system keeps every
    byte.  Before that: accel_step(F) with nothing else is accel_update(F)."""
    torch = torch_cuda
    nsys, n, mvec = 5, 129, 4
    rng = np.random.default_rng(3)
    a, twin = _waves(nsys, n, mvec), _waves(nsys, n, mvec)
    for _ in range(2):
        Xh = rng.standard_normal((nsys, n))
        Fa, Ft = _f64(torch, Xh), _f64(torch, Xh)
        a.accel_step(Fa)                                     # the all-NULL step
        twin.accel_update(Ft)
        assert torch.equal(Fa, Ft)
    for k in range(nsys):
        assert _snapshot(a, k, mvec) == _snapshot(twin, k, mvec), k
    f0, x0 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    f0[4] = 0.0
    r = _f64(torch, np.zeros(nsys))
    Ft = _f64(torch, f0)
    twin.accel_step(Ft, fnorm=r)                             # the probing call: tol = None
    r = r.cpu().numpy()
    assert r[4] == 0.0 and (r[:4] > 0).all()
    snap = [_snapshot(a, k, mvec) for k in range(nsys)]
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
        assert _snapshot(a, k, mvec) == snap[k], k
    assert _bits_equal(got[~out], ft[~out]) and _bits_equal(xg[~out], x0[~out] - ft[~out]), "the systems that went on"
    for k in np.flatnonzero(~out):
        assert _snapshot(a, k, mvec) == _snapshot(twin, k, mvec), k
    # tol = +inf retires every ACTIVE system; the one inactive on entry stays as it is, fnorm included
    f1 = rng.standard_normal((nsys, n))
    snap = [_snapshot(a, k, mvec) for k in range(nsys)]
    F, mask, fnorm = _f64(torch, f1), _i32(torch, [1, 1, 0, 1, 1]), _f64(torch, np.full(nsys, PLANTED))
    a.accel_step(F, Xd, mask, _f64(torch, np.full(nsys, np.inf)), fnorm)
    assert not mask.cpu().numpy().any() and _bits_equal(F.cpu().numpy(), f1) and _bits_equal(Xd.cpu().numpy(), xg)
    fn = fnorm.cpu().numpy()
    assert fn[2] == PLANTED and (fn[[0, 1, 3, 4]] > 0).all()
    assert snap == [_snapshot(a, k, mvec) for k in range(nsys)]
    a.delete()
    twin.delete()


# ---- 4. graphs --------------------------------------------------------------------------------------------------------------------

def test_a_whole_solve_replays_with_no_host_in_the_loop(torch_cuda):
    """The solve of tests/batch_step.py, 64 systems of 96 unknowns: [residual; accel_step] captured ONCE, before any update, and
    replayed SOLVE_REPLAYS times (the budget of tests/test_batch_step_cpu.py: the oracle retires every system eight steps inside
    it) with thresholds formed on the device after the first replay.  The eager twin is a wave batch running accel_update under
    masks the host forms from the twin's own accel_step norms -- this kind's bits, so no guard band is needed: all of it ==."""
    torch = torch_cuda
    nsys, vlen, mvec = S.SOLVE_NSYS, S.SOLVE_VLEN, S.SOLVE_MVEC
    d, eps, bb, x0 = (_f64(torch, a) for a in S.solve_problem())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _waves(nsys, vlen, mvec, S.SOLVE_FLAVOR)
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

    eager, probe = _waves(nsys, vlen, mvec, S.SOLVE_FLAVOR), _waves(nsys, vlen, mvec, S.SOLVE_FLAVOR)
    Xe, alive, tolh = x0.clone(), np.ones(nsys, bool), np.zeros(nsys)
    retired = np.full(nsys, -1)
    rdev = _f64(torch, np.zeros(nsys))
    for it in range(S.SOLVE_REPLAYS):
        Fe = S.solve_residual(torch, Xe, d, eps, bb).contiguous()
        probe.restart()                                      # the norm alone, in this kind's order: a step on a scratch batch
        probe.accel_step(Fe.clone(), fnorm=rdev)
        r = rdev.cpu().numpy()
        if it == 1:
            tolh = S.SOLVE_TOL * r0
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
    assert _bits_equal(tol.cpu().numpy(), tolh)
    assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)]
    assert np.array_equal(b.num_vec(), eager.num_vec())
    res = S.solve_residual(np, Xs.cpu().numpy(), *(a.cpu().numpy() for a in (d, eps, bb)))
    assert (np.linalg.norm(res, axis=1) <= 1e-7).all()       # (and it is a solution)
    for x in (b, eager, probe):
        x.delete()


# ---- 5. limits, refusals, lifecycle -----------------------------------------------------------------------------------------------

def test_limits_refusals_and_lifecycle(torch_cuda, CAP):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    L = nka_amd.nka_batch()._L
    warm = _waves(9, 129, 10)      # (code objects loaded and torch's pool grown BEFORE free memory is read, also when run alone)
    warm.accel_update(_f64(torch, np.ones((9, 129))))
    warm.w(0, 1)
    warm.delete()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    g, cap = C.c_int32(), C.c_int64()
    assert L.nka_hip_batch_waves_limits(C.byref(g), C.byref(cap)) == 0 and (g.value, cap.value) == (4, CAP)
    assert L.nka_hip_batch_waves_limits(None, None) == 0 and nka_amd.batch_waves_limits() == (4, CAP)
    h = C.c_void_p()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nsys, vlen, mvec, vtol in ((8, CAP + 1, 5, 0.01), (8, 129, 33, 0.01), (8, 129, 0, 0.01), (0, 129, 5, 0.01), (-1, 129, 5, 0.01),
                                   (8, 0, 5, 0.01), (8, 129, 5, 0.0), (8, 129, 5, -1.0)):
        assert L.nka_hip_batch_create_waves(C.byref(h), nsys, vlen, mvec, vtol, nka_amd.FLAVOR_DEFAULT, 0, stream) == EINVAL, (nsys, vlen, mvec, vtol)
        assert h.value is None and L.nka_hip_last_error()
    for nsys, vlen, mvec in ((8, CAP + 1, 5), (8, 129, 33), (0, 129, 5), (8, 0, 5)):
        with pytest.raises(NKAError):
            nka_amd.nka_batch().init(nsys, vlen, mvec, waves=True)
    assert L.nka_hip_batch_create_waves(C.byref(h), 8, CAP + 1, 5, 0.01, nka_amd.FLAVOR_DEFAULT, 0, stream) == EINVAL
    assert b"nka_hip_batch_create)" in L.nka_hip_last_error(), "the refusal names the entry to use instead"
    with pytest.raises(NKAError, match="wide"):
        nka_amd.nka_batch().init(8, 129, 5, waves=True, wide=True)
    with pytest.raises(NKAError, match="lanes"):
        nka_amd.nka_batch().init(8, 64, 5, waves=True, lanes=True)
    with pytest.raises(NKAError, match="binary32"):
        nka_amd.nka_batch().init(8, 129, 5, waves=True, storage=nka_amd.STORE_F32)
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "a refused creation left something allocated"

    nsys, vlen, mvec = 9, 129, 10
    a, never = _waves(nsys, vlen, mvec), _waves(nsys, vlen, mvec)      # `never`: one that never refused anything
    assert L.nka_hip_batch_kind(a._h) == 3 and L.nka_hip_batch_is_wide(a._h) == 0 and a.storage() == nka_amd.STORE_F64
    narrow = nka_amd.nka_batch().init(nsys, vlen, mvec)
    assert a.vector_bytes() == narrow.vector_bytes() == BWV.vector_bytes(vlen, mvec, nsys) == 2 * 8 * 160 * 11 * 9
    narrow.delete()
    rng = np.random.default_rng(2)
    w = _f64(torch, np.ones((nsys, vlen)))
    lens = _i32(torch, np.full(nsys, vlen))
    hostw, hostl = np.ones((nsys, vlen)), np.full(nsys, vlen, np.int32)

    def refusals():
        assert L.nka_hip_batch_set_dot_weights(a._h, C.c_void_p(w.data_ptr()), vlen) == EINVAL and b"nka_hip_batch_create" in L.nka_hip_last_error()
        assert L.nka_hip_batch_set_dot_weights_host(a._h, C.c_void_p(hostw.ctypes.data), vlen) == EINVAL
        assert L.nka_hip_batch_set_lengths(a._h, C.c_void_p(lens.data_ptr())) == EINVAL and b"nka_hip_batch_create" in L.nka_hip_last_error()
        assert L.nka_hip_batch_set_lengths_host(a._h, hostl.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL
        for order in (nka_amd.SUMS_REFERENCE_ORDER, nka_amd.SUMS_BLOCKED):
            assert L.nka_hip_batch_set_sum_order(a._h, order) == EINVAL and b"BLOCKED_ROUNDED" in L.nka_hip_last_error()
            with pytest.raises(NKAError):
                a.set_sum_order(order)
        for call in (lambda: a.set_dot_weights(w), lambda: a.set_dot_weights(hostw), lambda: a.set_lengths(lens), lambda: a.set_lengths(hostl)):
            with pytest.raises(NKAError):
                call()
        assert not a.dot_weighted() and not a.has_lengths()
        # a too-short allocation of F and of x (a buffer of exactly known size: the library's allocator); the step's refusals
        good = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        other = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        per = torch.zeros(2 * nsys, dtype=torch.float64, device="cuda")
        ws, short = C.c_void_p(), C.c_void_p()
        assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
        assert L.nka_hip_vec_alloc(ws, nsys * vlen - 1, C.byref(short)) == 0
        torch.cuda.synchronize()
        gp, op = C.c_void_p(good.data_ptr()), C.c_void_p(other.data_ptr())
        assert L.nka_hip_batch_accel_update(a._h, short, vlen, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_batch_accel_step(a._h, short, vlen, None, 0, None, None, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_batch_accel_step(a._h, gp, vlen, short, vlen, None, None, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_vec_free(ws, short) == 0 and L.nka_hip_vec_workspace_destroy(ws) == 0
        assert L.nka_hip_batch_accel_step(a._h, gp, vlen, None, 0, None, C.c_void_p(per.data_ptr()), None) == EINVAL      # tol without active
        assert L.nka_hip_batch_accel_step(a._h, gp, vlen, op, vlen - 1, None, None, None) == EINVAL                        # ldx < vlen
        assert L.nka_hip_batch_accel_step(a._h, gp, vlen, gp, vlen, None, None, None) == EINVAL                            # x overlapping f
        assert L.nka_hip_batch_accel_step(a._h, gp, vlen, None, 0, C.c_void_p(lens.data_ptr()), C.c_void_p(per.data_ptr()),
                                          C.c_void_p(per.data_ptr() + 8)) == EINVAL                                       # fnorm overlapping tol
        assert L.nka_hip_batch_accel_update(a._h, gp, vlen - 1, None) == EINVAL
        a.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED).set_sum_order(nka_amd.SUMS_AUTO)      # both mean the rounded fast sums

    for t in range(6):
        refusals()
        Xh = rng.standard_normal((nsys, vlen))
        Fa, Fn = _f64(torch, Xh), _f64(torch, Xh)
        a.accel_update(Fa)
        never.accel_update(Fn)
        assert torch.equal(Fa, Fn), t
    assert np.array_equal(a.num_vec(), never.num_vec())
    for k in range(nsys):
        assert _snapshot(a, k, mvec) == _snapshot(never, k, mvec), k
    a.set_stream(torch.cuda.current_stream().cuda_stream)
    a.set_vec_tol(0.5)
    a.delete()
    never.delete()
    again = _waves(nsys, vlen, mvec)                        # destroy / recreate: a fresh batch, the first call's bits
    first = _waves(nsys, vlen, mvec)
    Xh = rng.standard_normal((nsys, vlen))
    Fa, Fn = _f64(torch, Xh), _f64(torch, Xh)
    again.accel_update(Fa)
    first.accel_update(Fn)
    assert torch.equal(Fa, Fn) and np.array_equal(again.num_vec(), first.num_vec())
    assert _snapshot(again, 0, mvec) == _snapshot(first, 0, mvec) and again.state(0).pending == 1
    again.delete()
    first.delete()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "destroy left something allocated"


# ---- 6. slot allocations beyond 2^32 bytes ----------------------------------------------------------------------------------------

def test_slot_allocations_beyond_4_gib(torch_cuda, CAP):
    """w and v each pass 2^32 bytes at vlen = cap (tests/batch_waves.py: large_shape, held by the CPU test): at most nine systems
    run -- the first, the last, the ones on and beside the boundary --, every other one is masked; those that run equal a small
    twin after every call, and the masked witnesses where a byte offset that lost its upper half would land stay fresh."""
    torch = torch_cuda
    sh = BWV.large_shape(CAP)
    nsys, vlen, mvec, act = sh["nsys"], sh["vlen"], sh["mvec"], sh["active"]
    assert len(act) <= BWV.MAX_ACTIVE
    need = sum(BWV.large_bytes(sh).values())
    free, total = torch.cuda.mem_get_info()
    assert free >= need + (4 << 30), f"{free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 4 GiB"
    big = _waves(nsys, vlen, mvec)
    assert big.vector_bytes() == BWV.vector_bytes(vlen, mvec, nsys) and big.vector_bytes() // 2 > 2 ** 32
    twin = _waves(len(act), vlen, mvec)
    fresh = _waves(1, vlen, mvec).state_digest(0)
    mask = torch.zeros(nsys, dtype=torch.int32, device="cuda")
    idx = torch.tensor(act, dtype=torch.int64, device="cuda")
    mask[idx] = 1
    F = torch.full((nsys, vlen), BWV.PAD, dtype=torch.float64, device="cuda")
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
    for j, k in enumerate(act):
        assert _snapshot(big, k, mvec) == _snapshot(twin, j, mvec), k
    F[idx] = BWV.PAD
    assert bool((F == BWV.PAD).all()), "a row of a masked system was written"
    nv = big.num_vec()
    zero = np.zeros(vlen).tobytes()
    for k in sh["witnesses"]:
        assert nv[k] == 0 and big.state_digest(k) == fresh, k
        for s in range(1, mvec + 2):
            assert big.w(k, s).tobytes() == zero and big.v(k, s).tobytes() == zero, (k, s)
    big.delete()
    twin.delete()


# ---- the record (keep this test last) ----------------------------------------------------------------------------------------------
def test_worst_ratio_of_the_wave_sums_is_printed_and_inside_its_bound(capsys):
    """The worst |red - exact| / (u sum|xy|) the tests above saw, printed past the output capture, and once more held to the K it
    was judged by.  Selected on its own it has nothing to report."""
    ratio, k, where = WORST
    if not where:
        return
    with capsys.disabled():
        print("\n" + _worst_line())
    assert ratio <= (k + 1) / (1.0 - (k + 1) * X.U), (ratio, k, where)      # gamma(k) / u
