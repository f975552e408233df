"""The solve step of a WIDE batch (nka_hip_batch_create_wide_step, nka_batch().init(..., wide=True, step=True); the step instances of
nka_amd/csrc/nka_batch_wide.hip): residual norm, stop rule, update and x -= f of every system in four launches, no host in the loop.

  1 a step is the update: rows of F, state, red[], slots of a plain wide twin that runs accel_update under the mask the host
    predicts from the step's own fnorm and tol; the mask; X; 1 ... 17 chunks
  2 one chunk is the narrow step, bit for bit
  3 the order of the norm's chain in bits: fnorm == sqrt(red[0]) where d = f exactly, 3 ... 257 chunks
  4 the norm against the exact sum (bound: batch_wide_step.norm_bound; teeth: tests/test_batch_wide_step_cpu.py)
  5 the stop rule at its edges
  6 per-system lengths against step batches of the systems' own lengths
  7 a whole solve captured once and replayed, against an eager twin
  8 independence, lifecycle, refusals"""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import batch_lengths as BL
import batch_seq as B
import batch_wide as BW
import batch_wide_step as WS
import exact_sums as X
from split_update import _bits_equal

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


@pytest.fixture(scope="module")
def CH():
    """(C, max_vlen) as the library was built."""
    return BW.limits()


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """At the end of the module: the worst ratio of the norm and the K it was held to, beside batch_wide_exact_worst.json."""
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(f"wide batch step norm: worst |fnorm - sqrt(E)| = {ratio:.3f} u sqrt(E) against gamma({k}) + 4u there ({where})")
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_wide_step_exact_worst.json"), "w") as fh:
            json.dump({"wide_step": {"worst_err_over_u_sqrt_e": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


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


def _step_batch(nsys, n, mvec, flavor=2):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor, wide=True, step=True)
    assert b.is_wide() and b.offers_step() and b.kind() == 1
    return b


def _plain_wide(nsys, n, mvec, flavor=2):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor, wide=True)
    assert b.is_wide() and not b.offers_step()
    return b


def _same_state(a, b, nsys, where):
    assert np.array_equal(a.num_vec(), b.num_vec()), (where, "num_vec")
    for k in range(nsys):
        assert a.state_digest(k) == b.state_digest(k), (where, k, "digest")
        assert _bits_equal(a.reductions(k), b.reductions(k)), (where, k, "red")
        assert a.state(k).list_order() == b.state(k).list_order(), (where, k, "list")


def _same_slots(a, b, nsys, where):
    for k in range(nsys):
        for s in range(1, a.max_vec() + 2):
            assert _bits_equal(a.w(k, s), b.w(k, s)), (where, k, "w", s)
            assert _bits_equal(a.v(k, s), b.v(k, s)), (where, k, "v", s)


# ---- 1 and 2: a step is the update; one chunk is the narrow step -------------------------------------------------------------------

def _step_against_twin(torch, n, flavor, mvec, odd_ld, odd_ldx, narrow_twin=False):
    """5 systems, 11 calls: staggered starts, a masked relax and a masked restart mid-sequence, thresholds that retire about two
    systems at calls 4 and 9.  narrow_twin: the twin is a narrow batch at SUMS_BLOCKED_ROUNDED that runs the same accel_step;
    otherwise a plain wide batch that runs accel_update under the mask the host predicts from the step's fnorm and tol."""
    import nka_amd
    nsys, calls = 5, 11
    ld, ldx = _ld(n, odd_ld), _ld(n, odd_ldx)
    step = _step_batch(nsys, n, mvec, flavor)
    if narrow_twin:
        twin = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    else:
        twin = _plain_wide(nsys, n, mvec, flavor)
    rng = np.random.default_rng([1, n, flavor, mvec, ld])
    seqs = [B.Sequence(n, 7000 * n + 10 * k + flavor) for k in range(nsys)]
    (fs_raw, Fs), (ft_raw, Ft) = _rows(torch, nsys, n, ld), _rows(torch, nsys, n, ld)
    xhost = rng.standard_normal((nsys, ldx))                 # (the padding between rows too: it must stay as it is)
    x_raw, Xd = _rows(torch, nsys, n, ldx, xhost)
    xt_raw, Xt = _rows(torch, nsys, n, ldx, xhost)
    fhost = rng.standard_normal((nsys, ld))                  # (likewise)
    alive = np.ones(nsys, bool)
    mask, tol, fnorm = _i32(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    mask_t, fnorm_t = _i32(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    retired_at = set()
    for t in range(calls):
        where = (n, flavor, mvec, ld, ldx, narrow_twin, t)
        for op, at, who in (("relax", 5, [1, 4]), ("restart", 8, [2, 3])):      # no pending pair mid-sequence
            if t == at:
                m = _i32(torch, [int(k in who) for k in range(nsys)])
                getattr(step, op)(m)
                getattr(twin, op)(m)
        entry = alive & (t >= np.arange(nsys) % 3)           # staggered starts: with and without a pending pair in one launch
        for k in np.flatnonzero(entry):
            fhost[k, :n] = seqs[k].next()
        tolh = np.full(nsys, -1.0)                           # no norm is below it
        if t in (4, 9) and entry.sum() >= 3:                 # the second smallest norm of the entering systems, roughly
            tolh[:] = np.sort(np.sqrt((fhost[:, :n] * fhost[:, :n]).sum(axis=1))[entry])[1] * (1.0 + 1e-9)
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
        if narrow_twin:
            mask_t.copy_(_i32(torch, entry))
            fnorm_t.fill_(PLANTED)
            twin.accel_step(Ft, Xt, mask_t, tol, fnorm_t)
            assert torch.equal(mask, mask_t) and _bits_equal(fn, fnorm_t.cpu().numpy()), (where, "mask and fnorm of the narrow step")
            assert torch.equal(x_raw, xt_raw), (where, "X of the narrow step")
        else:
            twin.accel_update(Ft, _i32(torch, want))
        assert torch.equal(fs_raw, ft_raw), (where, "rows of F and their padding")
        _same_state(step, twin, nsys, where)
        fhost = fs_raw.cpu().numpy().reshape(nsys, ld)
        xwant = xhost.copy()
        xwant[want, :n] = xhost[want, :n] - fhost[want, :n]
        xgot = x_raw.cpu().numpy().reshape(nsys, ldx)
        assert _bits_equal(xgot, xwant), (where, "X and its padding")
        xhost = xgot
        retired_at |= {t for k in np.flatnonzero(entry & ~want)}
        alive &= ~(entry & ~want)
    assert len(retired_at) >= 1 and alive.any(), (n, flavor, mvec, retired_at, alive)
    assert step.num_vec().max() >= 1
    _same_slots(step, twin, nsys, (n, flavor, mvec, "slots at the end"))
    step.delete()
    twin.delete()


@pytest.mark.parametrize("which", ["1", "513", "C", "C+1", "2C+513", "8C+1", "9C+1", "16C+1"])
def test_a_wide_step_is_the_wide_update(torch_cuda, CH, which):
    """1, 1, 1, 2, 3, 9, 10 and 17 chunks: both trips of the eight-way chain of the scalar kernel and its remainders 0, 1 and 7.
    Three flavours x both parities of ld and ldx (with an odd stride the rows alternate between 16-byte aligned and not); mvec
    1, 3 and 10 in turn, and 32 once at 8C + 1."""
    c = CH[0]
    n = {"1": 1, "513": 513, "C": c, "C+1": c + 1, "2C+513": 2 * c + 513, "8C+1": 8 * c + 1, "9C+1": 9 * c + 1, "16C+1": 16 * c + 1}[which]
    assert BW.nchunk(n, c) == {"1": 1, "513": 1, "C": 1, "C+1": 2, "2C+513": 3, "8C+1": 9, "9C+1": 10, "16C+1": 17}[which]
    for i, (flavor, (odd_ld, odd_ldx)) in enumerate(itertools.product((0, 1, 2), ((False, True), (True, False)))):
        _step_against_twin(torch_cuda, n, flavor, (1, 3, 10)[i % 3], odd_ld, odd_ldx)
    if which == "8C+1":
        _step_against_twin(torch_cuda, n, 2, 32, False, False)


@pytest.mark.parametrize("which", ["1", "513", "2047", "C"])
def test_one_chunk_is_the_narrow_step(torch_cuda, CH, which):
    """Against a narrow batch at SUMS_BLOCKED_ROUNDED running the same accel_step: F, X, fnorm, mask, red[] and digest with ==."""
    n = CH[0] if which == "C" else int(which)
    assert BW.nchunk(n, CH[0]) == 1
    for flavor, mvec, odd in ((0, 3, False), (1, 10, True), (2, 3, True)):
        _step_against_twin(torch_cuda, n, flavor, mvec, odd, not odd, narrow_twin=True)


# ---- 3. the order of the norm's chain, in bits ------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["2C+513", "9C+1", "16C+1", "256C", "256C+1"])
def test_the_norm_is_red0_in_bits_where_d_equals_f(torch_cuda, CH, which):
    """Fresh systems; call 1 takes F1, call 2 takes F2 = F1 / 2 (exact).  Then d = fl(F1 - F2) = F2 exactly, so the partials of
    <f,f> are those of <d,d> and fnorm == sqrt(red[0]) bit for bit if and only if both chains add the same partials in the
    same order.  red[0] of the same call is the plain twin's.  3, 10, 17, 256 and 257 chunks (one and two trips of the staging)."""
    torch = torch_cuda
    c = CH[0]
    n = {"2C+513": 2 * c + 513, "9C+1": 9 * c + 1, "16C+1": 16 * c + 1, "256C": 256 * c, "256C+1": 256 * c + 1}[which]
    assert BW.nchunk(n, c) == {"2C+513": 3, "9C+1": 10, "16C+1": 17, "256C": 256, "256C+1": 257}[which]
    nsys, mvec = 2, 3
    step, twin = _step_batch(nsys, n, mvec), _plain_wide(nsys, n, mvec)
    f1 = np.random.default_rng([3, n]).standard_normal((nsys, n))
    f2 = f1 / 2
    assert np.array_equal(f1 - f2, f2)
    fnorm = _f64(torch, np.zeros(nsys))
    for f in (f1, f2):
        Fs, Ft = _f64(torch, f), _f64(torch, f)
        step.accel_step(Fs, fnorm=fnorm)
        twin.accel_update(Ft)
        assert torch.equal(Fs, Ft)
    fn = fnorm.cpu().numpy()
    for k in range(nsys):
        red0 = step.reductions(k)[0]
        assert red0 > 0 and red0 == twin.reductions(k)[0], (which, k, "red[0] against the plain twin")
        assert fn[k] == np.sqrt(red0), (which, k, fn[k], np.sqrt(red0))
    _same_state(step, twin, nsys, which)
    step.delete()
    twin.delete()


# ---- 4. the norm against the exact sum -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["C+1", "2C+513", "9C+1", "16C+1", "256C+1"])
def test_the_norm_against_the_exact_sum(torch_cuda, CH, which):
    """Planted inputs (sentinels at every place where the kernels change hands), each first held to
    batch_wide.undetectable_chunks == []: no lost or doubled partial can hide inside the bound.  Two calls: without a pending
    pair (f swept alone) and with one (<d,d> beside it), the rows exchanged between the systems."""
    torch = torch_cuda
    c = CH[0]
    n = dict(zip(["C+1", "2C+513", "9C+1", "16C+1", "256C+1"], WS.exact_shapes(c)))[which]
    k_sum = BW.wide_k(n, c)
    rows = WS.exact_inputs(n, c)
    exact = []
    for f in rows:
        assert BW.undetectable_chunks(f, f, k_sum, c) == [], (which, "the precondition on the input")
        exact.append(X.exact_dot(f, f))
    nsys = len(rows)
    b = _step_batch(nsys, n, 3, flavor=n % 3)
    fnorm = _f64(torch, np.zeros(nsys))
    for t, order in enumerate((list(range(nsys)), list(range(nsys))[::-1])):
        assert [b.state(k).pending for k in range(nsys)] == [t] * nsys
        b.accel_step(_f64(torch, np.stack([rows[j] for j in order])), fnorm=fnorm)
        fn = fnorm.cpu().numpy()
        for k, j in enumerate(order):
            ok, ratio = WS.norm_inside(fn[k], rows[j], n, c, exact=exact[j])
            print(f"wide step norm {(which, t, k)}: {ratio:.3f} u sqrt(E), bound {WS.norm_bound(n, c) / X.U:.1f} u")
            assert ok, (which, t, k, fn[k], ratio, WS.norm_bound(n, c) / X.U)
            if ratio >= WORST[0]:
                WORST[:] = [ratio, k_sum, str((which, t, k))]
    b.delete()


# ---- 5. the stop rule at its edges ---------------------------------------------------------------------------------------------

def _x_is(got, want):
    """Bit for bit where the expected value is a number; a NaN where it is one (its payload is the device's business)."""
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all()) and _bits_equal(got[~nan], want[~nan])


def _snapshot(b, nsys):
    return [(b.state_digest(k), b.reductions(k), [(b.w(k, s), b.v(k, s)) for s in range(1, b.max_vec() + 2)]) for k in range(nsys)]


def _unchanged(b, snap, ks, where):
    for k in ks:
        assert b.state_digest(k) == snap[k][0] and _bits_equal(b.reductions(k), snap[k][1]), (where, k)
        for s, (w, v) in enumerate(snap[k][2], start=1):
            assert _bits_equal(b.w(k, s), w) and _bits_equal(b.v(k, s), v), (where, k, "slot", s)


def test_the_stop_rule_of_a_wide_step_at_its_edges(torch_cuda, CH):
    torch = torch_cuda
    n, nsys, mvec = 2 * CH[0] + 513, 6, 3
    rng = np.random.default_rng(5)
    a, probe, twin = _step_batch(nsys, n, mvec), _step_batch(nsys, n, mvec), _plain_wide(nsys, n, mvec)
    for _ in range(2):                                       # (all with a pending pair)
        Xh = rng.standard_normal((nsys, n))
        a.accel_step(_f64(torch, Xh))                        # the all-NULL step: the update
        probe.accel_step(_f64(torch, Xh))
        twin.accel_update(_f64(torch, Xh))
    _same_state(a, twin, nsys, "all-NULL")
    f0, x0 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    f0[3, n // 2] = np.nan                                   # a NaN in f: r is NaN, the system goes on
    f0[5] = 0.0                                              # a zero row: retires at tol = 0
    r = _f64(torch, np.zeros(nsys))
    probe.accel_step(_f64(torch, f0), fnorm=r)               # the probing call: fnorm alone
    r = r.cpu().numpy()
    assert r[5] == 0.0 and np.isnan(r[3]) and (r[[0, 1, 2, 4]] > 0).all()
    snap = _snapshot(a, nsys)
    tol = np.array([r[0], np.nextafter(r[1], 0.0), np.nan, 1.0e300, np.inf, 0.0])
    want = np.array([0, 1, 1, 1, 0, 0], np.int32)
    F, Xd, mask, fnorm = _f64(torch, f0), _f64(torch, x0), _i32(torch, np.ones(nsys)), _f64(torch, np.full(nsys, PLANTED))
    Ft = _f64(torch, f0)
    a.accel_step(F, Xd, mask, _f64(torch, tol), fnorm)
    twin.accel_update(Ft, _i32(torch, want))
    assert np.array_equal(mask.cpu().numpy(), want), mask.cpu().numpy()
    assert _bits_equal(fnorm.cpu().numpy(), r)
    got, xg, ft = F.cpu().numpy(), Xd.cpu().numpy(), Ft.cpu().numpy()
    out = want == 0
    assert _bits_equal(got[out], f0[out]) and _bits_equal(xg[out], x0[out]), "a retired system's rows"
    _unchanged(a, snap, np.flatnonzero(out), "a retired system's state and slots")
    assert _bits_equal(got[~out], ft[~out]) and _x_is(xg[~out], x0[~out] - ft[~out]), "the systems that went on"
    _same_state(a, twin, nsys, "after the edges")
    # the partials a retired system wrote are read by nobody: the next update of every system is the twin's.  X alone.
    f1 = rng.standard_normal((nsys, n))
    F, Ft, x1 = _f64(torch, f1), _f64(torch, f1), _f64(torch, xg)
    a.accel_step(F, x1)
    twin.accel_update(Ft)
    assert _bits_equal(F.cpu().numpy(), Ft.cpu().numpy()) and _x_is(x1.cpu().numpy(), xg - Ft.cpu().numpy())
    _same_state(a, twin, nsys, "the update after a retirement")
    _same_slots(a, twin, nsys, "the update after a retirement")
    # tol = +inf retires every ACTIVE system with a norm; the one inactive on entry stays as it is, fnorm included
    snap = _snapshot(a, nsys)
    f2 = rng.standard_normal((nsys, n))
    F, mask, fnorm = _f64(torch, f2), _i32(torch, [1, 1, 0, 1, 1, 1]), _f64(torch, np.full(nsys, PLANTED))
    xb = x1.clone()
    a.accel_step(F, x1, mask, _f64(torch, np.full(nsys, np.inf)), fnorm)
    fn = fnorm.cpu().numpy()
    assert fn[2] == PLANTED and (fn[[0, 1, 3, 4, 5]] > 0).all()      # (system 3: its state carries a NaN, its new f does not)
    assert not mask.cpu().numpy().any()
    assert _bits_equal(F.cpu().numpy(), f2) and _bits_equal(x1.cpu().numpy(), xb.cpu().numpy())
    _unchanged(a, snap, range(nsys), "+inf")
    for b in (a, probe, twin):
        b.delete()


# ---- 6. lengths -------------------------------------------------------------------------------------------------------------------

def test_a_wide_step_with_per_system_lengths_is_the_step_of_each_length(torch_cuda, CH):
    """Systems of 1, C, C + 1, 2C + 513 and 8C + 1 elements in a batch of vlen = 9C + 1 against wide-step batches created with
    vlen = len[sys] (the LENGTHS contract).  The tails of F and X are painted with NaNs of their own payloads and compared byte
    for byte after every call."""
    torch = torch_cuda
    c = CH[0]
    lens = [1, c, c + 1, 2 * c + 513, 8 * c + 1]
    nsys, vlen, mvec, calls = len(lens), 9 * c + 1, 3, 9
    big = _step_batch(nsys, vlen, mvec).set_lengths(lens)
    assert big.has_lengths() and big.offers_step()
    twins = [_step_batch(1, L, mvec) for L in lens]
    seqs = BL.sequences(lens, 611)
    fpaint, xpaint = BL.nan_paint(nsys, vlen, 1), BL.nan_paint(nsys, vlen, 2)
    fhost = fpaint.copy()
    xhost = xpaint.copy()
    rng = np.random.default_rng(6)
    for k, L in enumerate(lens):
        xhost[k, :L] = rng.standard_normal(L)
        fhost[k, :L] = 0.0
    F, Xd = _f64(torch, fhost), _f64(torch, xhost)
    alive = np.ones(nsys, bool)
    for t in range(calls):
        if t == 4:
            big.relax(_i32(torch, [0, 1, 0, 1, 0]))
            twins[1].relax()
            twins[3].relax()
        if t == 6:
            big.restart(_i32(torch, [0, 0, 1, 0, 1]))
            twins[2].restart()
            twins[4].restart()
        entry = alive & (t >= np.arange(nsys) % 3)
        for k in np.flatnonzero(entry):
            fhost[k, :lens[k]] = seqs[k].next()
        tolh = np.full(nsys, -1.0)
        if t == 5:
            tolh[[1, 3]] = np.inf                            # two systems retire mid-sequence
        F.copy_(torch.from_numpy(fhost))
        mask, tol, fnorm = _i32(torch, entry), _f64(torch, tolh), _f64(torch, np.full(nsys, PLANTED))
        big.accel_step(F, Xd, mask, tol, fnorm)
        got, xg, mg, fg = F.cpu().numpy(), Xd.cpu().numpy(), mask.cpu().numpy(), fnorm.cpu().numpy()
        assert BL.tails_intact(got, fpaint, lens) == [] and BL.tails_intact(xg, xpaint, lens) == [], (t, "a tail was written")
        for k, L in enumerate(lens):
            where = (t, k, L)
            if not entry[k]:
                assert fg[k] == PLANTED and mg[k] == 0 and BL.same_bytes(got[k, :L], fhost[k, :L]), where
                continue
            Fk, Xk = _f64(torch, fhost[k:k + 1, :L]), _f64(torch, xhost[k:k + 1, :L])
            mk, fk = _i32(torch, [1]), _f64(torch, [PLANTED])
            twins[k].accel_step(Fk, Xk, mk, _f64(torch, tolh[k:k + 1]), fk)
            assert mg[k] == mk.cpu().numpy()[0] and _bits_equal(fg[k:k + 1], fk.cpu().numpy()), (where, "mask, fnorm")
            assert BL.same_bytes(got[k, :L], Fk.cpu().numpy()[0]) and BL.same_bytes(xg[k, :L], Xk.cpu().numpy()[0]), (where, "rows")
            assert big.state_digest(k) == twins[k].state_digest(0), (where, "digest")
            assert _bits_equal(big.reductions(k), twins[k].reductions(0)), (where, "red")
        alive &= ~(entry & (mg == 0))
        fhost, xhost = got, xg
    assert not alive[1] and not alive[3] and alive[[0, 2, 4]].all()
    for b in [big] + twins:
        b.delete()


# ---- 7. a whole solve with no host in the loop --------------------------------------------------------------------------------

def test_a_whole_wide_solve_replays_with_no_host_in_the_loop(torch_cuda, CH):
    """[residual; accel_step] captured ONCE, before any update, and replayed SOLVE_REPLAYS times without a synchronise; the
    relative thresholds are formed on the device after the first replay (tol = 0 until then).  The eager twin is a plain wide
    batch that runs accel_update under masks the host forms from torch.linalg.vector_norm; it asserts that none of its own
    norms lies within SOLVE_GUARD of its threshold, so the two runs take the same decisions (tests/test_batch_step_gpu.py)."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    nsys, vlen, mvec = WS.SOLVE_NSYS, WS.solve_vlen(c), WS.SOLVE_MVEC
    d, eps, bb, x0 = (_f64(torch, a) for a in WS.solve_problem(c))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=WS.SOLVE_FLAVOR, wide=True, step=True)
        Xs, Fs = x0.clone(), torch.zeros_like(x0)
        mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        Fs.copy_(WS.solve_residual(torch, Xs, d, eps, bb))
        b.accel_step(Fs, Xs, mask, tol, fnorm)
    with torch.cuda.stream(side):
        g.replay()
        torch.mul(fnorm, WS.SOLVE_TOL, out=tol)              # the recipe for relative tolerances: a device operation
        for _ in range(WS.SOLVE_REPLAYS - 1):
            g.replay()
    torch.cuda.synchronize()

    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=WS.SOLVE_FLAVOR, wide=True)
    Xe, alive, tolh = x0.clone(), np.ones(nsys, bool), np.zeros(nsys)
    retired = np.full(nsys, -1)
    for it in range(WS.SOLVE_REPLAYS):
        Fe = WS.solve_residual(torch, Xe, d, eps, bb)
        r = torch.linalg.vector_norm(Fe, dim=1).cpu().numpy()
        if it == 1:
            tolh = WS.SOLVE_TOL * r0
        assert (np.abs(r - tolh)[alive] > WS.SOLVE_GUARD * tolh[alive]).all(), (it, "a close call: the twin cannot judge it")
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
    res = WS.solve_residual(np, Xs.cpu().numpy(), *(a.cpu().numpy() for a in (d, eps, bb)))
    assert (np.linalg.norm(res, axis=1) <= 1e-6).all()       # (and it is a solution)
    b.delete()
    eager.delete()


# ---- 8. independence, lifecycle and refusals ------------------------------------------------------------------------------------

def _run_system(torch, n, mvec, inputs, x0, nsys, pos, others, odd_ldx):
    """The system's inputs at position pos of a batch of nsys; others: "active", "masked" or "nonfinite" neighbours.  The last
    call retires the system (tol = +inf).  -> everything the step leaves of the system."""
    b = _step_batch(nsys, n, mvec)
    ldx = _ld(n, odd_ldx)
    rng = np.random.default_rng([8, nsys, pos])
    xh = rng.standard_normal((nsys, ldx))
    xh[pos, :n] = x0
    x_raw, Xd = _rows(torch, nsys, n, ldx, xh)
    out = []
    for t, f in enumerate(inputs):
        fh = rng.standard_normal((nsys, n))
        if others == "nonfinite":
            fh[:, ::97] = np.inf
            fh[:, 5::101] = np.nan
        fh[pos] = f
        m = np.ones(nsys, np.int32) if others != "masked" else (np.arange(nsys) == pos).astype(np.int32)
        tolh = np.full(nsys, -1.0)
        if t == len(inputs) - 1:
            tolh[pos] = np.inf
        F, mask, fnorm = _f64(torch, fh), _i32(torch, m), _f64(torch, np.full(nsys, PLANTED))
        b.accel_step(F, Xd, mask, _f64(torch, tolh), fnorm)
        out.append((F.cpu().numpy()[pos], x_raw.cpu().numpy().reshape(nsys, ldx)[pos, :n].copy(), fnorm.cpu().numpy()[pos],
                    int(mask.cpu().numpy()[pos]), b.reductions(pos), b.state_digest(pos)))
    b.delete()
    return out


def test_a_system_of_a_wide_step_does_not_depend_on_the_batch_around_it(torch_cuda, CH):
    torch = torch_cuda
    n, mvec = 2 * CH[0] + 513, 3
    seq = B.Sequence(n, 88)
    inputs = [seq.next() for _ in range(6)]
    x0 = np.random.default_rng(80).standard_normal(n)
    base = _run_system(torch, n, mvec, inputs, x0, 1, 0, "active", False)
    assert [o[3] for o in base] == [1] * 5 + [0]
    for nsys, pos, others, odd_ldx in ((3, 1, "active", True), (3, 2, "masked", True), (5, 0, "nonfinite", False), (5, 3, "nonfinite", True),
                                       (5, 4, "masked", False)):
        got = _run_system(torch, n, mvec, inputs, x0, nsys, pos, others, odd_ldx)
        for t, (g, w) in enumerate(zip(got, base)):
            where = (nsys, pos, others, odd_ldx, t)
            assert _bits_equal(g[0], w[0]) and _bits_equal(g[1], w[1]), (where, "rows")
            assert g[2] == w[2] and g[3] == w[3] and _bits_equal(g[4], w[4]) and g[5] == w[5], (where, "fnorm, mask, red, digest")


def test_lifecycle_of_a_wide_step_batch(torch_cuda, CH):
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    L = nka_amd.load()
    assert L.nka_hip_batch_offers_step(None) < 0 and L.nka_hip_last_error()
    made = {"narrow": nka_amd.nka_batch().init(3, 33, 3), "lanes": nka_amd.nka_batch().init(3, 33, 3, lanes=True),
            "waves": nka_amd.nka_batch().init(3, 33, 3, waves=True), "wide": nka_amd.nka_batch().init(3, c + 33, 3, wide=True),
            "wide step": nka_amd.nka_batch().init(3, c + 33, 3, wide=True, step=True)}
    assert {k: b.offers_step() for k, b in made.items()} == {"narrow": True, "lanes": True, "waves": True, "wide": False, "wide step": True}
    assert made["wide step"].kind() == made["wide"].kind() == 1 and made["wide step"].is_wide()
    for b in made.values():
        b.delete()
    # accel_update of a step batch is a plain wide batch's, with and without lengths
    nsys, vlen, mvec = 3, 2 * c + 513, 3
    lens = [c + 1, vlen, 513]
    rng = np.random.default_rng(9)
    for with_len in (False, True):
        a, twin = _step_batch(nsys, vlen, mvec, flavor=1), _plain_wide(nsys, vlen, mvec, flavor=1)
        if with_len:
            a.set_lengths(lens)
            twin.set_lengths(lens)
        for t in range(5):
            f = rng.standard_normal((nsys, vlen))
            Fa, Ft = _f64(torch, f), _f64(torch, f)
            m = None if t != 2 else _i32(torch, [1, 0, 1])
            a.accel_update(Fa, m)
            twin.accel_update(Ft, m)
            assert torch.equal(Fa, Ft), (with_len, t)
            _same_state(a, twin, nsys, (with_len, t))
        _same_slots(a, twin, nsys, with_len)
        a.delete()
        twin.delete()
    # destroy, then create
    b = _step_batch(nsys, vlen, mvec)
    F = _f64(torch, rng.standard_normal((nsys, vlen)))
    b.accel_step(F)
    b.delete()
    b = _step_batch(nsys, vlen, mvec)
    fn = _f64(torch, np.zeros(nsys))
    b.accel_step(F, fnorm=fn)
    assert not b.num_vec().any() and b.state(0).pending and (fn.cpu().numpy() > 0).all()
    b.delete()


def test_what_a_wide_step_batch_refuses_leaves_it_usable(torch_cuda, CH):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    c, cap = CH
    L = nka_amd.load()
    h = C.c_void_p()
    for nsys, vlen, mvec in [(2, cap + 1, 3), (65536, 8, 3), (2, 8, 33), (0, 8, 3), (2, 0, 3)]:      # the limits of create_wide
        assert L.nka_hip_batch_create_wide_step(C.byref(h), nsys, vlen, mvec, 0.01, -1, 0, None) == EINVAL and h.value is None
    for kw in ({}, {"lanes": True}, {"waves": True}):
        with pytest.raises(NKAError):
            nka_amd.nka_batch().init(3, 33, 3, step=True, **kw)
    with pytest.raises(NKAError):
        nka_amd.nka_batch().init(3, c + 33, 3, wide=True, step=True, storage=nka_amd.STORE_F32)
    nsys, n, mvec = 3, c + 33, 3
    rng = np.random.default_rng(10)
    plain = _plain_wide(nsys, n, mvec)
    F, Xs = _f64(torch, rng.standard_normal((nsys, n))), _f64(torch, rng.standard_normal((nsys, n)))
    with pytest.raises(NKAError):                            # a plain wide batch still refuses the step
        plain.accel_step(F, Xs)
    assert L.nka_hip_batch_accel_step(plain._handle(), C.c_void_p(F.data_ptr()), n, None, 0, None, None, None) == EINVAL
    assert b"nka_hip_batch_create_wide" in L.nka_hip_last_error()
    b, twin = _step_batch(nsys, n, mvec), plain

    def still_the_twins():
        for _ in range(2):
            Xh = rng.standard_normal((nsys, n))
            Fa, Fb = _f64(torch, Xh), _f64(torch, Xh)
            b.accel_step(Fa)
            twin.accel_update(Fb)
            assert torch.equal(Fa, Fb)
            _same_state(b, twin, nsys, "twins")

    still_the_twins()
    hb = b._handle()
    ld = n + 3
    span = (nsys - 1) * ld + n
    big = _f64(torch, rng.standard_normal(3 * span))
    ok_i, ok_d, ok_n = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(2 * nsys)), _f64(torch, np.zeros(nsys))      # (tol = 0: nothing retires)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)      # noqa: E731
    step = L.nka_hip_batch_accel_step
    f, x = P(big), P(big, span)
    dig = [b.state_digest(k) for k in range(nsys)]
    before = big.clone()
    assert step(hb, f, ld, x, ld, None, P(ok_d), P(ok_n)) == EINVAL and b"mask" in L.nka_hip_last_error()      # tol without active
    for off in (0, nsys - 1):                                # fnorm over tol
        assert step(hb, f, ld, x, ld, P(ok_i), P(ok_d, off), P(ok_d, nsys - 1)) == EINVAL and b"overlaps" in L.nka_hip_last_error()
    assert step(hb, f, ld, x, n - 1, P(ok_i), P(ok_d), P(ok_n)) == EINVAL and b"ldx" in L.nka_hip_last_error()
    assert step(hb, f, n - 1, x, ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL
    assert step(hb, None, ld, x, ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL
    for off in (0, 1, span - 1, -(span - 1)):                # x over f
        assert step(hb, P(big, span), ld, P(big, span + off), ld, P(ok_i), P(ok_d), P(ok_n)) == EINVAL and b"overlaps" in L.nka_hip_last_error()
    # short spans: allocations of exactly known size from the library's own allocator
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    assert L.nka_hip_vec_alloc(ws, (nsys - 1) * n + n - 1, C.byref(short)) == 0
    torch.cuda.synchronize()
    good = C.c_void_p(F.data_ptr())
    assert step(hb, short, n, None, 0, None, None, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
    assert step(hb, good, n, short, n, None, None, None) == EINVAL and b"shorter" in L.nka_hip_last_error()
    assert L.nka_hip_vec_free(ws, short) == 0 and L.nka_hip_vec_workspace_destroy(ws) == 0
    # weights, the reference order, _BLOCKED: refused on every wide batch
    with pytest.raises(NKAError):
        b.set_dot_weights(torch.ones(n, dtype=torch.float64, device="cuda"))
    with pytest.raises(NKAError):
        b.set_dot_weights(np.ones(n))
    for order in (nka_amd.SUMS_REFERENCE_ORDER, nka_amd.SUMS_BLOCKED, 17):
        with pytest.raises(NKAError):
            b.set_sum_order(order)
    b.set_sum_order(nka_amd.SUMS_AUTO).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    assert not b.dot_weighted()
    torch.cuda.synchronize()
    assert torch.equal(big, before) and [b.state_digest(k) for k in range(nsys)] == dig and ok_i.cpu().numpy().all()
    still_the_twins()
    b.delete()
    twin.delete()
