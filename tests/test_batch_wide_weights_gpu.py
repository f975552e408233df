"""The WIDE batch with diagonal dot weights (nka_hip_batch_create_wide_ext, nka_batch().init(..., wide=True, ext=True[, step=True]);
the weighted instances of k_wide_norm, k_wide_step_norm and k_wide_sums of nka_amd/csrc/nka_batch_wide.hip).  Shapes are given in units of
C = NKA_HIP_BATCH_WIDE_CHUNK, read from the library.

   1 one chunk            a weighted wide batch of at most C elements is the weighted narrow batch in SUMS_BLOCKED_ROUNDED, bit for bit
   2 unit weights         w == 1, in both forms, is the plain wide batch (update) and the plain wide step batch (step), bit for bit
   3 powers of four       w = 4^k is an exact rescaling: a plain wide batch on the rescaled input
   4 several chunks       the three layers of WideRun with fl(w o x) as first operand of every sum
   5 chunk order          red[0] == ((p0 + p1) + p2) + ..., p_c from ONE weighted narrow batch whose rows are the chunks
   6 the step             fnorm against the exact weighted sum; the stop rule at its edges; a retired system writes nothing
   7 a zero-weight tail   against the same batch with per-system lengths
   8 capture              before the first update; new values between replays; a captured shared-form call keeps its form
   9 a whole solve        ragged and weighted, captured once, against an eager twin
  10 independence         of nsys, position, masked or NaN-fed neighbours, ld / ldw parity; painted tails untouched
  11 refusals, lifecycle  what is refused leaves the previous weighting in force; the offers table over all nine creations
  12 large offsets        the weight buffer and the caller's weight rows pass 2^32 bytes inside a running system's row

A bound only proves something where the error it looks for exceeds it: every sum over several chunks that part 4 holds is first
held, from its host operands alone, to batch_wide.undetectable_chunks(fl(w x), y, K, C) == []; tests/test_batch_wide_weights_cpu.py
shows on the host model that a weight ignored, the partner's weight, a lost and a doubled partial then break the bound.

The worst |red - exact| / (u sum|fl(w x) y|) of part 4 and the K it was held to go to batch_wide_weights_exact_worst.json."""
import ctypes as C
import itertools
import json
import math
import os

import numpy as np
import pytest

import batch_lengths as BL
import batch_seq as B
import batch_wide as BW
import batch_wide_step as WS
import batch_wide_weights as WW
import exact_sums as X
import test_batch_sums_exact_gpu as T
from split_update import _bits_equal
from test_batch_wide_gpu import WideRun

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
PLANTED = -7.0                     # what fnorm holds before a call: kept by every system inactive on entry
WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|fl(w x) y|) seen, the K it was held to, where


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


def _worst_line():
    ratio, k, where = WORST
    return f"wide batch sums (weighted): worst |red - exact| = {ratio:.3f} u sum|fl(w x) y| against K = {k} there ({where})"


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(_worst_line())
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_wide_weights_exact_worst.json"), "w") as fh:
            json.dump({"wide_weighted": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


def _ld(n, odd):
    return n + (1 - n % 2 if odd else n % 2)                 # the smallest odd / even row stride that holds a row


def _rows(torch, nsys, n, ld, host=None, fill=0.0):
    """nsys rows of n doubles, ld apart, inside one allocation: (the whole buffer, the view a batch takes)."""
    if host is None:
        raw = torch.full((nsys * ld,), fill, dtype=torch.float64, device="cuda")
    else:
        raw = torch.from_numpy(np.ascontiguousarray(host).ravel().copy()).cuda()
    return raw, raw.view(nsys, ld)[:, :n]


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).cuda()


def _ext(nsys, n, mvec, flavor=2, step=False):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor, wide=True, ext=True, step=step)
    assert b.is_wide() and b.kind() == nka_amd.KIND_WIDE and b.offers_weights() and b.offers_lengths() and b.offers_step() == step
    return b


def _plain(nsys, n, mvec, flavor=2, step=False):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor, wide=True, step=step)
    assert b.is_wide() and not b.offers_weights()
    return b


def _decisions(st):
    return st.list_order(), st.free_order(), (st.subspace, st.pending, st.first, st.last, st.free)


def _same_state(a, b, nsys, where, digest=True, pairs=None):
    """red[], h, c, the lists, num_vec and (digest=True) the digest of every system, bit for bit; pairs: [(ka, kb)]."""
    pairs = [(k, k) for k in range(nsys)] if pairs is None else pairs
    nva, nvb = a.num_vec(), b.num_vec()
    for ka, kb in pairs:
        assert _bits_equal(a.reductions(ka), b.reductions(kb)), (where, ka, "red", a.reductions(ka), b.reductions(kb))
        sa, sb = a.state(ka), b.state(kb)
        assert _decisions(sa) == _decisions(sb), (where, ka, "lists")
        assert _bits_equal(sa.h, sb.h) and _bits_equal(sa.c, sb.c), (where, ka, "h / c")
        assert nva[ka] == nvb[kb], (where, ka, "num_vec")
        assert not digest or a.state_digest(ka) == b.state_digest(kb), (where, ka, "digest")


def _same_slots(a, b, nsys, where, upto=None, pairs=None):
    """EVERY slot of w and v, bit for bit (upto: the first `upto[k]` elements of system k's)."""
    pairs = [(k, k) for k in range(nsys)] if pairs is None else pairs
    for ka, kb in pairs:
        L = None if upto is None else upto[ka]
        for s in range(1, a.max_vec() + 2):
            assert _bits_equal(a.w(ka, s)[:L], b.w(kb, s)[:L]), (where, ka, "w", s)
            assert _bits_equal(a.v(ka, s)[:L], b.v(kb, s)[:L]), (where, ka, "v", s)


def _weights_in_form(torch, W, form, odd_ldw=False):
    """What set_dot_weights takes: the shared row W[0] or the rows of W, ldw apart inside one allocation."""
    nsys, n = W.shape
    if form == "shared":
        return _f64(torch, W[0])
    ldw = _ld(n, odd_ldw)
    host = np.full((nsys, ldw), np.nan)                      # (the padding between two rows is never read)
    host[:, :n] = W
    return _rows(torch, nsys, n, ldw, host)[1]


def _effective(W, form):
    return np.tile(W[0], (W.shape[0], 1)) if form == "shared" else W


# ---- 1. one chunk is the weighted narrow batch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["1", "2", "65", "513", "C-1", "C"])
def test_one_chunk_is_the_weighted_narrow_batch_bit_for_bit(torch_cuda, CH, which):
    """Three systems with staggered starts, general weights in both forms, three flavours, accel_update and accel_step (with X, a
    mask, thresholds that retire a system at call 4, and fnorm), 6 calls each.  The twin is a narrow batch with the same weights in
    SUMS_BLOCKED_ROUNDED (also up to 64 elements, where its AUTO is the reference order).  After every call, with ==: F, X, fnorm,
    the mask, red[], the state, the digest and every slot."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    n = WW.shape(which, c)
    assert BW.nchunk(n, c) == 1 and n <= nka_amd.BATCH_MAX_VLEN
    nsys, mvec, calls = 3, 3, 6
    W = WW.system_weights(n, nsys, c)
    for flavor, form, step in itertools.product((0, 1, 2), ("shared", "rows"), (False, True)):
        odd = bool(flavor % 2)
        ld, ldx = _ld(n, odd), _ld(n, not odd)
        wide = _ext(nsys, n, mvec, flavor, step).set_dot_weights(_weights_in_form(torch, W, form, odd))
        twin = nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        twin.set_dot_weights(_weights_in_form(torch, W, form, not odd))
        assert wide.dot_weighted() and twin.dot_weighted()
        rng = np.random.default_rng([1, n, flavor])
        seqs = [B.Sequence(n, 9000 * n + 10 * k + flavor) for k in range(nsys)]
        (fw_raw, Fw), (ft_raw, Ft) = _rows(torch, nsys, n, ld), _rows(torch, nsys, n, ld)
        xhost = rng.standard_normal((nsys, ldx))
        (xw_raw, Xw), (xt_raw, Xt) = _rows(torch, nsys, n, ldx, xhost), _rows(torch, nsys, n, ldx, xhost)
        fhost = np.zeros((nsys, ld))
        alive = np.ones(nsys, bool)
        for t in range(calls):
            where = (which, flavor, form, "step" if step else "update", t)
            entry = alive & (t >= np.arange(nsys))           # staggered starts: with and without a pending pair in one launch
            for k in np.flatnonzero(entry):
                fhost[k, :n] = seqs[k].next()
            for raw in (fw_raw, ft_raw):
                raw.copy_(torch.from_numpy(fhost.ravel()))
            mw, mt = _i32(torch, entry), _i32(torch, entry)
            if step:
                tolh = np.full(nsys, -1.0)
                if t == 4:
                    tolh[1] = np.inf                         # system 1 retires
                fnw, fnt = _f64(torch, np.full(nsys, PLANTED)), _f64(torch, np.full(nsys, PLANTED))
                wide.accel_step(Fw, Xw, mw, _f64(torch, tolh), fnw)
                twin.accel_step(Ft, Xt, mt, _f64(torch, tolh), fnt)
                assert torch.equal(mw, mt) and _bits_equal(fnw.cpu().numpy(), fnt.cpu().numpy()), (where, "mask, fnorm")
                assert torch.equal(xw_raw, xt_raw), (where, "X and its padding")
                alive &= ~(entry & (mw.cpu().numpy() == 0))
                assert (fnw.cpu().numpy()[entry] >= 0).all() and (fnw.cpu().numpy()[~entry] == PLANTED).all(), where
            else:
                wide.accel_update(Fw, mw)
                twin.accel_update(Ft, mt)
            assert torch.equal(fw_raw, ft_raw), (where, "rows of F and their padding")
            fhost = fw_raw.cpu().numpy().reshape(nsys, ld)
            _same_state(wide, twin, nsys, where)
            _same_slots(wide, twin, nsys, where)
        assert wide.num_vec().max() >= 1 or n < 65, (which, wide.num_vec())
        assert not step or not alive[1]
        wide.delete()
        twin.delete()


# ---- 2. unit weights are the plain wide batch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,lengths", [("C+1", False), ("2C+513", False), ("9C+1", False), ("2C+513", True)],
                         ids=["C+1", "2C+513", "9C+1", "2C+513-lengths"])
def test_unit_weights_are_the_plain_wide_batch(torch_cuda, CH, which, lengths):
    """w == 1 in the shared form and in one row per system, both parities of ld (and of ldw): accel_update against a batch of
    nka_hip_batch_create_wide, accel_step against one of nka_hip_batch_create_wide_step -- F, X, fnorm, the mask, red[], the state,
    the digest, every slot, with ==.  With lengths (1, C, C + 1, 2C + 513 inside 2C + 513) the weight rows hold 2^500 from the length
    on; an ext batch with NOTHING set runs beside them."""
    torch = torch_cuda
    c = CH[0]
    n = WW.shape(which, c)
    nsys, mvec, calls = 4, 3, 6
    lens = [1, c, c + 1, 2 * c + 513] if lengths else [n] * nsys
    ones = np.ones((nsys, n))
    for k, L in enumerate(lens):
        ones[k, L:] = WW.TAIL_WEIGHT
    shared_row = np.ones((1, n))                             # (the shared row serves every length: ones throughout)
    for step, odd in itertools.product((False, True), (False, True)):
        ld = _ld(n, odd)
        batches = {"plain": _plain(nsys, n, mvec, 2, step),
                   "shared": _ext(nsys, n, mvec, 2, step).set_dot_weights(_weights_in_form(torch, shared_row, "shared")),
                   "rows": _ext(nsys, n, mvec, 2, step).set_dot_weights(_weights_in_form(torch, ones, "rows", not odd)),
                   "nothing": _ext(nsys, n, mvec, 2, step)}
        assert [b.dot_weighted() for b in batches.values()] == [False, True, True, False]
        if lengths:
            for b in batches.values():
                b.set_lengths(lens)
        rng = np.random.default_rng([2, n, step, odd])
        paint = BL.nan_paint(nsys, ld, 3)
        fhost = paint.copy()
        xhost = BL.nan_paint(nsys, ld, 4)
        for k, L in enumerate(lens):
            xhost[k, :L] = rng.standard_normal(L)
        F = {name: _rows(torch, nsys, n, ld, fhost) for name in batches}
        Xd = {name: _rows(torch, nsys, n, ld, xhost) for name in batches}
        for t in range(calls):
            where = (which, lengths, "step" if step else "update", odd, t)
            entry = t >= np.arange(nsys) % 3
            for k in np.flatnonzero(entry):
                fhost[k, :lens[k]] = rng.standard_normal(lens[k])
            tolh = np.full(nsys, -1.0)
            if t == 4:
                tolh[2] = np.inf
            out = {}
            for name, b in batches.items():
                raw, view = F[name]
                raw.copy_(torch.from_numpy(fhost.ravel()))
                m = _i32(torch, entry)
                if step:
                    fn = _f64(torch, np.full(nsys, PLANTED))
                    b.accel_step(view, Xd[name][1], m, _f64(torch, tolh), fn)
                    out[name] = (raw.cpu().numpy(), Xd[name][0].cpu().numpy(), m.cpu().numpy(), fn.cpu().numpy())
                else:
                    b.accel_update(view, m)
                    out[name] = (raw.cpu().numpy(),)
            for name in ("shared", "rows", "nothing"):
                for got, want in zip(out[name], out["plain"]):
                    assert BL.same_bytes(got, want), (where, name, "F, X, mask or fnorm")
                _same_state(batches[name], batches["plain"], nsys, where + (name,))
            fhost = out["plain"][0].reshape(nsys, ld)
        for name in ("shared", "rows", "nothing"):
            _same_slots(batches[name], batches["plain"], nsys, (which, lengths, step, odd, name), upto=lens)
        assert batches["rows"].num_vec().max() >= 2
        for b in batches.values():
            b.delete()


# ---- 3. powers of four ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_powers_of_four_are_an_exact_rescaling_of_a_wide_system(torch_cuda, CH, flavor):
    """w[sys, i] = 4^k, k in [-6, 6] drawn per system and element: fl(w a) b = (2^k a)(2^k b) exactly, so the weighted batch on F
    equals 2^-k o (a plain wide batch on 2^k o F), bit for bit: rows, red[], h, c, list and free order, stored w and v; in the step
    also fnorm, the mask and x.  2C + 513 elements, mvec = 5, mvec + 4 calls."""
    torch = torch_cuda
    n, nsys, mvec = 2 * CH[0] + 513, 3, 5
    rng = np.random.default_rng([4, n, flavor])
    k4 = rng.integers(-6, 7, (nsys, n))
    scale = np.ldexp(1.0, k4)
    for step in (False, True):
        bw = _ext(nsys, n, mvec, flavor, step).set_dot_weights(_f64(torch, np.ldexp(1.0, 2 * k4)))
        bp = _plain(nsys, n, mvec, flavor, step)
        seqs = [B.Sequence(n, 4000 + 100 * mvec + 10 * k + flavor) for k in range(nsys)]
        xh = rng.standard_normal((nsys, n))
        Xw, Xp = _f64(torch, xh), _f64(torch, scale * xh)
        for t in range(mvec + 4):
            Xh = np.stack([s.next() for s in seqs])
            Fw, Fp = _f64(torch, Xh), _f64(torch, scale * Xh)
            where = (flavor, step, t)
            if step:
                tolh = np.full(nsys, -1.0)
                if t == 6:
                    tolh[1] = np.inf
                mw, mp = _i32(torch, np.ones(nsys)), _i32(torch, np.ones(nsys))
                fw, fp = _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
                bw.accel_step(Fw, Xw, mw, _f64(torch, tolh), fw)
                bp.accel_step(Fp, Xp, mp, _f64(torch, tolh), fp)
                assert torch.equal(mw, mp) and _bits_equal(fw.cpu().numpy(), fp.cpu().numpy()), (where, "mask, fnorm")
                assert _bits_equal(scale * Xw.cpu().numpy(), Xp.cpu().numpy()), (where, "x")
            else:
                bw.accel_update(Fw)
                bp.accel_update(Fp)
            assert _bits_equal(scale * Fw.cpu().numpy(), Fp.cpu().numpy()), where
            _same_state(bw, bp, nsys, where, digest=False)
            for k in range(nsys):
                for slot in bw.state(k).list_order():
                    assert _bits_equal(scale[k] * bw.w(k, slot), bp.w(k, slot)), (where, k, slot, "w")
                    assert _bits_equal(scale[k] * bw.v(k, slot), bp.v(k, slot)), (where, k, slot, "v")
        assert bw.num_vec().max() >= 3
        bw.delete()
        bp.delete()


# ---- 4. several chunks: the three layers ----------------------------------------------------------------------------------------------

def _hold(what, red, a, y, k, where):
    ex = X.exact_dot(a, y)
    assert math.isfinite(ex), (what, where)
    tot = X.abs_dot(a, y)
    err = abs(red - ex)
    ratio = err / (X.U * tot) if tot else err
    print(f"  {what} {where}: |red - exact| = {ratio:.3f} u sum|fl(w x) y|, K = {k}")
    assert err <= X.gamma(k) * tot, (what, where, red, ex, ratio, k)
    if tot > 0 and ratio >= WORST[0]:
        WORST[:] = [ratio, k, f"{what} {where}"]


class WideWeightedRun(WideRun):
    """WideRun on a batch of nka_hip_batch_create_wide_ext with general weights per system (batch_wide_weights.system_weights:
    the rule of batch_weights at every sentinel of every chunk).  Layer 1 holds every sum with its FIRST operand x replaced by
    fl(w_sys o x) -- K unchanged, the first operand is already rounded --, after the condition on the host operands; layers 2 and 3
    are inherited unchanged."""

    def _device(self, odd_ld):
        import nka_amd
        torch, n, nsys, ld = self.torch, self.n, self.nsys, self.ld
        self.b = _ext(nsys, n, self.m, self.flavor)
        self.order, self.orders_met = nka_amd.SUMS_BLOCKED_ROUNDED, set()
        self.reference = nka_amd.SUMS_REFERENCE_ORDER
        assert self.b.flavor() == self.flavor
        self.raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda")
        self.F = self.raw.view(nsys, ld)[:, :n]
        c = BW.limits()[0]
        self.wts = WW.system_weights(n, nsys, c)
        for k in range(nsys):
            WW.assert_weight_rule(n, self.wts[k], c)
        self.b.set_dot_weights(_weights_in_form(torch, self.wts, "rows", not odd_ld))
        assert self.b.dot_weighted()
        self._sys = None

    def _check(self, k, *args):
        self._sys = k
        super()._check(k, *args)

    def _sum(self, what, red, x, y, where):
        a = self.wts[self._sys] * x                          # fl(w x): rounded once, before the product
        if self.n > self.chunk:
            unseen = BW.undetectable_chunks(a, y, self.k, self.chunk)
            assert not unseen, (what, where, "the bound could not see these chunks' partials lost: another seed", unseen)
            self.cells += BW.nchunk(self.n, self.chunk)
        _hold(what, red, a, y, self.k, where)
        if red != 0.0:
            self.held[what] = self.held.get(what, 0) + 1


def _planned_run(run, seed):
    """test_batch_sums_exact_gpu._planned_run with the sentinels of a wide system."""
    n, rngs, prev = run.n, [np.random.default_rng([seed, k]) for k in range(run.nsys)], [None] * run.nsys
    for t in range(T.SHAPE_CALLS):
        steps = {k: t - T.PLAN[k][0] for k in range(run.nsys) if t >= T.PLAN[k][0]}
        relax = [k for k, j in steps.items() if j == T.PLAN[k][1]]
        restart = [k for k, j in steps.items() if j == T.PLAN[k][3]]
        if relax:
            run.relax(relax)
        if restart:
            run.restart(restart)
        inputs = {}
        for k, j in steps.items():
            inputs[k] = prev[k].copy() if j == T.PLAN[k][2] else BW.wide_planted_input(n, rngs[k], prev[k])
            prev[k] = inputs[k]
        run.update(inputs)
    return run


def _late_second_system(run, calls, seed):
    """Two systems on fresh planted inputs, the second one call late (with odd ld: on a row that is not 16-byte aligned)."""
    rngs, prev = [np.random.default_rng([seed, run.n, k]) for k in range(2)], [None, None]
    for t in range(calls):
        inputs = {}
        for k in range(2):
            if t >= k:
                inputs[k] = prev[k] = BW.wide_planted_input(run.n, rngs[k], prev[k])
        run.update(inputs)
    assert run.lengths_differed and run.cells > 0
    return run


@pytest.mark.parametrize("mvec", [3, 10])
@pytest.mark.parametrize("which", WW.EXACT_SHAPES)
def test_every_part_of_a_weighted_wide_update(torch_cuda, oracle, CH, which, mvec):
    """2, 3, 9, 10 and 17 chunks in the default flavour.  mvec = 10 at 2 and 3 chunks: the plan of six systems of
    test_batch_sums_exact_gpu (older counts 0 ... 10, a repeated input, a masked relax and a masked restart each); mvec = 10 from 9
    chunks on: two systems, the second one call late on an unaligned row, mvec + 2 updates -- every older count 0 ... 10 and the
    capacity drop, a sixth of the host's exact sums; mvec = 3: the same two systems, six updates."""
    c = CH[0]
    n = WW.shape(which, c)
    assert BW.nchunk(n, c) == WW.EXACT_CHUNKS[which] and BW.wide_k(n) == 2 * (c // 512) + 9 + (WW.EXACT_CHUNKS[which] - 1)
    odd = WW.EXACT_CHUNKS[which] % 2 == 1
    if mvec == 10 and WW.EXACT_CHUNKS[which] <= 3:
        run = _planned_run(WideWeightedRun(torch_cuda, oracle, 2, n, T.SHAPE_MVEC, len(T.PLAN), odd), seed=n)
        T._assert_planned_coverage(run)
        assert run.cells > 0
    elif mvec == 10:
        run = _late_second_system(WideWeightedRun(torch_cuda, oracle, 2, n, 10, 2, odd_ld=True), 12, seed=10)
        assert run.widest == 10 and run.nolder_normed == set(range(11)), (run.widest, run.nolder_normed)
    else:
        run = _late_second_system(WideWeightedRun(torch_cuda, oracle, 2, n, 3, 2, odd_ld=True), 6, seed=3)
        assert run.widest == 3 and run.held["<d,d>"] >= 5


@pytest.mark.parametrize("flavor", [0, 1])
def test_every_part_of_a_weighted_wide_update_in_the_other_flavours(torch_cuda, oracle, CH, flavor):
    """... and the two F08 flavours at 2C + 513, the whole plan, odd ld."""
    n = 2 * CH[0] + 513
    run = _planned_run(WideWeightedRun(torch_cuda, oracle, flavor, n, T.SHAPE_MVEC, len(T.PLAN), True), seed=n + flavor)
    T._assert_planned_coverage(run)


def test_every_older_count_of_a_weighted_wide_system_up_to_the_largest_subspace(torch_cuda, oracle, CH):
    """mvec = 32 once at 2C + 513: every group count of the weighted sums kernel, up to eight groups of four."""
    n, mvec = 2 * CH[0] + 513, 32
    run = _late_second_system(WideWeightedRun(torch_cuda, oracle, 2, n, mvec, 2, odd_ld=True), mvec + 2, seed=mvec)
    assert run.widest == mvec and run.nolder_normed == set(range(mvec + 1)), run.nolder_normed
    assert run.held.get("<f,w_30>", 0) >= 1 and run.held.get("<f,w_31>", 0) >= 1, run.held


def test_every_part_of_a_weighted_wide_update_at_257_chunks(torch_cuda, oracle, CH):
    """256C + 1 once: the second trip of the staging loop of wide_norm_sum on weighted partials; mvec = 3, four updates."""
    n = 256 * CH[0] + 1
    assert n <= CH[1] and BW.nchunk(n, CH[0]) == 257
    run = _late_second_system(WideWeightedRun(torch_cuda, oracle, 2, n, 3, 2, odd_ld=True), 4, seed=9)
    assert run.widest == 2 and run.held["<d,d>"] == 5


# ---- 5. the chunk order, in bits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["2C+513", "9C+1"])
def test_red0_is_the_chunk_order_sum_of_one_weighted_narrow_batch_of_the_chunks(torch_cuda, CH, which):
    """red[0] of the second update of a fresh weighted wide system is ((p0 + p1) + p2) + ..., bit for bit, at 3 and 10 chunks.  p_c is
    red[0] of system c of ONE weighted narrow batch (SUMS_BLOCKED_ROUNDED) of nchunk systems whose rows of F AND of weights are the
    chunks; the last chunk through set_lengths, with NaN behind it in F and 2^500 in the weights."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    vlen = WW.shape(which, c)
    chunks = BW.nchunk(vlen, c)
    assert chunks == {"2C+513": 3, "9C+1": 10}[which]
    rng = np.random.default_rng([31, vlen])
    x0 = BW.wide_planted_input(vlen, rng)
    x1 = BW.wide_planted_input(vlen, rng, prev=x0)
    w = WW.draw_weights(vlen, rng, c)
    last = vlen - (chunks - 1) * c
    wide = _ext(1, vlen, 3).set_dot_weights(_f64(torch, w))
    narrow = nka_amd.nka_batch().init(chunks, c, 3).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    narrow.set_lengths(np.array([c] * (chunks - 1) + [last], np.int64))
    wrows = np.full(chunks * c, WW.TAIL_WEIGHT)
    wrows[:vlen] = w
    narrow.set_dot_weights(_f64(torch, wrows.reshape(chunks, c)))
    for x in (x0, x1):          # second update of a fresh system: a pending pair, no older vector
        wide.accel_update(_f64(torch, x).view(1, vlen))
        rows = np.full(chunks * c, np.nan)
        rows[:vlen] = x
        narrow.accel_update(_f64(torch, rows).view(chunks, c))
    got = np.float64(wide.reductions(0)[0])
    p = [np.float64(narrow.reductions(k)[0]) for k in range(chunks)]
    want = p[0]
    for q in p[1:]:
        want = want + q
    assert got > 0 and all(q > 0 for q in p), (got, p)
    assert _bits_equal(np.array([got]), np.array([want])), (which, got, want)
    d = x0 - x1
    plainsum = X.exact_dot(d, d)
    assert abs(got - plainsum) > 1e-3 * plainsum, "the weights did something"


# ---- 6. the step ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["C+1", "9C+1"])
def test_the_weighted_norm_against_the_exact_sum(torch_cuda, CH, which):
    """fnorm within batch_wide_step.norm_bound of sqrt(exact_dot(fl(w f), f)) per system: planted inputs, weights by the rule, each
    operand pair first held to batch_wide.undetectable_chunks == [].  Two calls: without a pending pair (the weights ride along the
    lone sweep of f) and with one (<d,d> beside it), in both forms."""
    torch = torch_cuda
    c = CH[0]
    n = WW.shape(which, c)
    k_sum = BW.wide_k(n, c)
    rows = WS.exact_inputs(n, c)
    nsys = len(rows)
    W = WW.system_weights(n, nsys, c)
    for form in ("rows", "shared"):
        Weff = _effective(W, form)
        b = _ext(nsys, n, 3, flavor=n % 3, step=True).set_dot_weights(_weights_in_form(torch, W, form))
        fnorm = _f64(torch, np.zeros(nsys))
        for t, order in enumerate((list(range(nsys)), list(range(nsys))[::-1])):
            assert [b.state(k).pending for k in range(nsys)] == [t] * nsys
            b.accel_step(_f64(torch, np.stack([rows[j] for j in order])), fnorm=fnorm)
            fn = fnorm.cpu().numpy()
            for k, j in enumerate(order):
                a = Weff[k] * rows[j]
                assert BW.undetectable_chunks(a, rows[j], k_sum, c) == [], (which, form, "the precondition on the input")
                want = math.sqrt(X.exact_dot(a, rows[j]))
                ratio = abs(fn[k] - want) / (X.U * want)
                print(f"weighted wide step norm {(which, form, t, k)}: {ratio:.3f} u sqrt(E), bound {WS.norm_bound(n, c) / X.U:.1f} u")
                assert abs(fn[k] - want) <= WS.norm_bound(n, c) * want, (which, form, t, k, fn[k], want, ratio)
                plain = math.sqrt(X.exact_dot(rows[j], rows[j]))
                assert abs(fn[k] - plain) > 1e-3 * plain, "the weights did something"
        b.delete()


def _snapshot(b, nsys):
    return [(b.state_digest(k), b.reductions(k), [(b.w(k, s), b.v(k, s)) for s in range(1, b.max_vec() + 2)]) for k in range(nsys)]


def _unchanged(b, snap, ks, where):
    for k in ks:
        assert b.state_digest(k) == snap[k][0] and _bits_equal(b.reductions(k), snap[k][1]), (where, k)
        for s, (w, v) in enumerate(snap[k][2], start=1):
            assert _bits_equal(b.w(k, s), w) and _bits_equal(b.v(k, s), v), (where, k, "slot", s)


def _x_is(got, want):
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all()) and _bits_equal(got[~nan], want[~nan])


def test_the_stop_rule_of_a_weighted_wide_step_at_its_edges(torch_cuda, CH):
    """tol = r retires, nextafter(r, 0) does not, a NaN threshold and a NaN norm go on, +inf retires, 0 retires a zero row.  A
    retired system writes nothing but fnorm and its `active` entry: its rows of F and X, red[], digest and every slot stay.  The
    twin is an ext batch with the same weights running accel_update under the expected mask."""
    torch = torch_cuda
    n, nsys, mvec = 2 * CH[0] + 513, 6, 3
    rng = np.random.default_rng(5)
    W = WW.system_weights(n, nsys, CH[0])

    def new(step):
        return _ext(nsys, n, mvec, 2, step).set_dot_weights(_f64(torch, W))

    a, probe, twin = new(True), new(True), new(False)
    for _ in range(2):                                       # (all with a pending pair)
        Xh = rng.standard_normal((nsys, n))
        a.accel_step(_f64(torch, Xh))
        probe.accel_step(_f64(torch, Xh))
        twin.accel_update(_f64(torch, Xh))
    _same_state(a, twin, nsys, "all-NULL")
    f0, x0 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    f0[3, n // 2] = np.nan                                   # a NaN in f under a nonzero weight: r is NaN, the system goes on
    assert W[3, n // 2] >= 0
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
    # the partials a retired system wrote are read by nobody: the next update of every system is the twin's
    f1 = rng.standard_normal((nsys, n))
    F, Ft, x1 = _f64(torch, f1), _f64(torch, f1), _f64(torch, xg)
    a.accel_step(F, x1)
    twin.accel_update(Ft)
    assert _bits_equal(F.cpu().numpy(), Ft.cpu().numpy()) and _x_is(x1.cpu().numpy(), xg - Ft.cpu().numpy())
    _same_state(a, twin, nsys, "the update after a retirement")
    _same_slots(a, twin, nsys, "the update after a retirement")
    for b in (a, probe, twin):
        b.delete()


def test_a_zero_weight_does_not_shield_a_non_finite_value(torch_cuda, CH):
    """fl(0 x NaN) is NaN, as in the narrow batch: a NaN or an Inf under a zero weight reaches the norm and the sums."""
    torch = torch_cuda
    n, nsys = CH[0] + 513, 2
    W = np.ones((nsys, n))
    W[:, CH[0] + 7] = 0.0
    b = _ext(nsys, n, 3, 2, True).set_dot_weights(_f64(torch, W))
    rng = np.random.default_rng(12)
    fn = _f64(torch, np.zeros(nsys))
    b.accel_step(_f64(torch, rng.standard_normal((nsys, n))), fnorm=fn)
    assert np.isfinite(fn.cpu().numpy()).all()
    f = rng.standard_normal((nsys, n))
    f[0, CH[0] + 7] = np.nan
    f[1, CH[0] + 7] = np.inf
    b.accel_step(_f64(torch, f), fnorm=fn)
    assert np.isnan(fn.cpu().numpy()).all(), fn.cpu().numpy()
    assert np.isnan(b.reductions(0)[0]) and np.isnan(b.reductions(1)[0])
    b.delete()


# ---- 7. a zero-weight tail against lengths --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["513", "C+1", "2C+513"])
def test_a_zero_weight_tail_is_the_system_of_that_length(torch_cuda, CH, which):
    """Batch A: vlen = 3C, general positive weights on [0, L) and w = 0 on [L, 3C).  Batch B: the same weights on [0, L), 2^500
    behind, and set_lengths(L).  Finite random data everywhere in A.  Over 5 calls red[], the state, num_vec and F[:, :L] are ==.
    Derived, not fitted: fma(+-0, y, acc) = acc for finite y, a chunk of zero weights adds a partial of +0, and r + 0 = r."""
    torch = torch_cuda
    c = CH[0]
    L = WW.shape(which, c)
    vlen, nsys, mvec = 3 * c, 2, 3
    rng = np.random.default_rng([7, L])
    Wa, Wb = np.zeros((nsys, vlen)), np.full((nsys, vlen), WW.TAIL_WEIGHT)
    Wa[:, :L] = Wb[:, :L] = np.exp2(rng.uniform(-3.0, 3.0, (nsys, L)))
    for step in (False, True):
        A = _ext(nsys, vlen, mvec, 2, step).set_dot_weights(_f64(torch, Wa))
        Bt = _ext(nsys, vlen, mvec, 2, step).set_dot_weights(_f64(torch, Wb)).set_lengths([L] * nsys)
        for t in range(5):
            f = rng.standard_normal((nsys, vlen))
            fb = BL.nan_paint(nsys, vlen, 5)
            fb[:, :L] = f[:, :L]
            Fa, Fb = _f64(torch, f), _f64(torch, fb)
            if step:
                fna, fnb = _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
                A.accel_step(Fa, fnorm=fna)
                Bt.accel_step(Fb, fnorm=fnb)
                assert _bits_equal(fna.cpu().numpy(), fnb.cpu().numpy()), (which, t, "fnorm")
            else:
                A.accel_update(Fa)
                Bt.accel_update(Fb)
            ga, gb = Fa.cpu().numpy(), Fb.cpu().numpy()
            assert np.isfinite(ga).all()
            assert _bits_equal(ga[:, :L], gb[:, :L]), (which, step, t, "F[:, :L]")
            assert BL.same_bytes(gb[:, L:], fb[:, L:]), (which, step, t, "the tail under lengths was written")
            _same_state(A, Bt, nsys, (which, step, t), digest=False)
        assert A.num_vec().max() >= 3
        A.delete()
        Bt.delete()


# ---- 8. capture -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [False, True], ids=["update", "step"])
@pytest.mark.parametrize("form", ["shared", "rows"])
def test_a_weighted_wide_call_is_capturable_before_the_first_update(torch_cuda, CH, form, step):
    """Captured before the first update, replayed against an eager twin; new values of the same form set between replays reach the
    next replay; setting weights while the stream captures returns NKA_HIP_ESTATE and changes nothing.  A captured shared-form
    call keeps its form: after the per-row form is set on the batch, the replay still reads the one row all systems share."""
    torch = torch_cuda
    nsys, vlen, mvec = 6, 2 * CH[0] + 513, 4
    W1, W2, W3 = (WW.system_weights(vlen, nsys, CH[0], seed=s) for s in (81, 82, 83))
    pick = (lambda w: w[0]) if form == "shared" else (lambda w: w)
    seqs = [B.Sequence(vlen, 800 + k) for k in range(nsys)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _ext(nsys, vlen, mvec, 2, step).set_dot_weights(_f64(torch, pick(W1)))
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        xs = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    eager = _ext(nsys, vlen, mvec, 2, step).set_dot_weights(_f64(torch, pick(W1)))
    xe = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    other = _f64(torch, pick(W2))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        if step:
            b.accel_step(static, xs)
        else:
            b.accel_update(static)
        rc = b._L.nka_hip_batch_set_dot_weights(b._handle(), C.c_void_p(other.data_ptr()), 0 if form == "shared" else vlen)
        rc_none = b._L.nka_hip_batch_set_dot_weights(b._handle(), None, 0)
    assert rc == ESTATE and rc_none == ESTATE and b.dot_weighted()
    for t in range(mvec + 6):
        if t == 4:                                           # new values of the same form: the next replays run with them
            with torch.cuda.stream(side):
                b.set_dot_weights(_f64(torch, pick(W2)))
            eager.set_dot_weights(_f64(torch, pick(W2)))
        if t == 7 and form == "shared":                      # the OTHER form on the batch: the captured call keeps its own
            with torch.cuda.stream(side):
                b.set_dot_weights(_f64(torch, W3))
            eager.set_dot_weights(_f64(torch, W3[0]))        # (the shared row lives in row 0 of the batch's buffer)
        Xh = np.stack([s.next() for s in seqs])
        static.copy_(torch.from_numpy(Xh))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = _f64(torch, Xh)
        if step:
            eager.accel_step(F, xe)
            assert torch.equal(xs, xe), (form, t, "x")
        else:
            eager.accel_update(F)
        assert torch.equal(F, static), (form, step, t)
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], (form, step, t)
    plain = _plain(nsys, vlen, mvec)                         # (and the weights did something)
    F = _f64(torch, Xh)
    plain.accel_update(F)
    assert plain.state_digest(0) != b.state_digest(0)
    for x in (b, eager, plain):
        x.delete()


# ---- 9. a whole ragged weighted solve -------------------------------------------------------------------------------------------------

def test_a_ragged_weighted_wide_solve_replays_with_no_host_in_the_loop(torch_cuda, CH):
    """The solve of tests/batch_wide_weights.py -- 16 systems of C/2 ... 3C unknowns, weights zero on every 17th entry and 4^k
    elsewhere --: [residual; accel_step] captured ONCE, before any update, and replayed SOLVE_REPLAYS times (the budget the CPU test
    holds on the oracle), thresholds formed on the device after the first replay.  The eager twin is an ext batch of the same
    lengths and weights running accel_update under masks the host forms from a probe's accel_step norms: all of it ==."""
    torch = torch_cuda
    c = CH[0]
    nsys, vlen, mvec = WW.SOLVE_NSYS, WW.solve_vlen(c), WW.SOLVE_MVEC
    d, eps, bb, x0, left, right = (_f64(torch, a) for a in WW.solve_problem(c))
    lens, W = WW.solve_lengths(c), WW.solve_weights(c)
    inside = torch.from_numpy(np.arange(vlen)[None, :] < lens[:, None]).cuda()

    def new(step):
        return _ext(nsys, vlen, mvec, WW.SOLVE_FLAVOR, step).set_dot_weights(_f64(torch, W)).set_lengths(lens)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = new(True)
        Xs, Fs = x0.clone(), torch.zeros_like(x0)
        mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        Fs.copy_(WW.solve_residual(torch, Xs, d, eps, bb, left, right))
        b.accel_step(Fs, Xs, mask, tol, fnorm)
    with torch.cuda.stream(side):
        g.replay()
        torch.mul(fnorm, WW.SOLVE_TOL, out=tol)
        for _ in range(WW.SOLVE_REPLAYS - 1):
            g.replay()
    torch.cuda.synchronize()

    eager, probe = new(False), new(True)
    Xe, alive, tolh = x0.clone(), np.ones(nsys, bool), np.zeros(nsys)
    retired = np.full(nsys, -1)
    rdev = _f64(torch, np.zeros(nsys))
    for it in range(WW.SOLVE_REPLAYS):
        Fe = WW.solve_residual(torch, Xe, d, eps, bb, left, right).contiguous()
        probe.restart()
        probe.accel_step(Fe.clone(), fnorm=rdev)
        r = rdev.cpu().numpy()
        if it == 1:
            tolh = WW.SOLVE_TOL * r0
        stop = alive & (r <= tolh)
        retired[stop] = it
        alive &= ~stop
        m = _i32(torch, alive)
        eager.accel_update(Fe, m)
        Xe = torch.where(m.bool()[:, None] & inside, Xe - Fe, Xe)
        if it == 0:
            r0 = r
    assert not alive.any() and len(set(retired.tolist())) >= 3, retired
    assert not mask.cpu().numpy().any(), "every system has retired"
    assert torch.equal(Xs, Xe)
    assert not bool(Xs[~inside].any()), "x beyond a system's length was written"
    assert _bits_equal(tol.cpu().numpy(), tolh)
    assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)]
    assert np.array_equal(b.num_vec(), eager.num_vec())
    res = WW.solve_residual(np, Xs.cpu().numpy(), *(a.cpu().numpy() for a in (d, eps, bb, left, right)))
    wres = np.sqrt((np.where(inside.cpu().numpy(), W, 0.0) * res * res).sum(axis=1))
    assert (wres <= 2.0 * tolh).all(), (wres, tolh)          # (and it is a solution in the norm the batch measures)
    for x in (b, eager, probe):
        x.delete()


# ---- 10. independence -----------------------------------------------------------------------------------------------------------------

def _run_system(torch, n, L, mvec, inputs, x0, w, nsys, pos, others, odd):
    """The system's inputs, weights and length at position pos of a weighted ext step batch of nsys with lengths; others:
    "active", "masked" or "nonfinite" neighbours.  The tails of F, X and the weight rows are painted (NaN payloads; weights 2^500)
    and compared byte for byte.  The last call retires the system.  -> everything the step leaves of the system."""
    b = _ext(nsys, n, mvec, 2, True)
    ld = _ld(n, odd)
    rng = np.random.default_rng([10, nsys, pos])
    lens = [int(v) for v in rng.integers(1, n + 1, nsys)]
    lens[pos] = L
    Wh = np.full((nsys, n), WW.TAIL_WEIGHT)
    for k in range(nsys):
        Wh[k, :lens[k]] = np.exp2(rng.uniform(-2.0, 2.0, lens[k]))
    Wh[pos, :L] = w
    b.set_dot_weights(_weights_in_form(torch, Wh, "rows", not odd)).set_lengths(lens)
    xpaint, fpaint = BL.nan_paint(nsys, ld, 6), BL.nan_paint(nsys, ld, 7)
    xh = xpaint.copy()
    for k in range(nsys):
        xh[k, :lens[k]] = rng.standard_normal(lens[k])
    xh[pos, :L] = x0
    x_raw, Xd = _rows(torch, nsys, n, ld, xh)
    out = []
    for t, f in enumerate(inputs):
        fh = fpaint.copy()
        for k in range(nsys):
            fh[k, :lens[k]] = rng.standard_normal(lens[k])
            if others == "nonfinite" and k != pos:
                fh[k, :lens[k]:97] = np.inf
                fh[k, 5:lens[k]:101] = np.nan
        fh[pos, :L] = f
        m = np.ones(nsys, np.int32) if others != "masked" else (np.arange(nsys) == pos).astype(np.int32)
        tolh = np.full(nsys, -1.0)
        if t == len(inputs) - 1:
            tolh[pos] = np.inf
        f_raw, F = _rows(torch, nsys, n, ld, fh)
        mask, fnorm = _i32(torch, m), _f64(torch, np.full(nsys, PLANTED))
        b.accel_step(F, Xd, mask, _f64(torch, tolh), fnorm)
        fg, xg = f_raw.cpu().numpy().reshape(nsys, ld), x_raw.cpu().numpy().reshape(nsys, ld)
        assert BL.tails_intact(fg[:, :n], fpaint[:, :n], lens) == [] and BL.same_bytes(fg[:, n:], fpaint[:, n:]), (t, "a tail of F was written")
        assert BL.tails_intact(xg[:, :n], xpaint[:, :n], lens) == [] and BL.same_bytes(xg[:, n:], xpaint[:, n:]), (t, "a tail of X was written")
        out.append((fg[pos, :L].copy(), xg[pos, :L].copy(), fnorm.cpu().numpy()[pos], int(mask.cpu().numpy()[pos]),
                    b.reductions(pos), b.state_digest(pos)))
    b.delete()
    return out


def test_a_weighted_wide_system_does_not_depend_on_the_batch_around_it(torch_cuda, CH):
    """nsys 1, 3 and 5, every kind of neighbour (active, masked, fed NaN and Inf), both parities of ld and ldw, per-system
    lengths with painted tails: the same bits as the system alone in a batch of one."""
    torch = torch_cuda
    n, L, mvec = 2 * CH[0] + 513, CH[0] + 513, 3
    seq = B.Sequence(L, 98)
    inputs = [seq.next() for _ in range(6)]
    rng = np.random.default_rng(90)
    x0 = rng.standard_normal(L)
    w = WW.draw_weights(L, rng, CH[0])
    base = _run_system(torch, n, L, mvec, inputs, x0, w, 1, 0, "active", False)
    assert [o[3] for o in base] == [1] * 5 + [0]
    for nsys, pos, others, odd in ((1, 0, "active", True), (3, 1, "active", True), (3, 2, "masked", False), (5, 0, "nonfinite", False),
                                   (5, 3, "nonfinite", True), (5, 4, "masked", True)):
        got = _run_system(torch, n, L, mvec, inputs, x0, w, nsys, pos, others, odd)
        for t, (g, want) in enumerate(zip(got, base)):
            where = (nsys, pos, others, odd, t)
            assert _bits_equal(g[0], want[0]) and _bits_equal(g[1], want[1]), (where, "rows")
            assert g[2] == want[2] and g[3] == want[3] and _bits_equal(g[4], want[4]) and g[5] == want[5], (where, "fnorm, mask, red, digest")


# ---- 11. refusals and lifecycle -------------------------------------------------------------------------------------------------------

def test_what_a_weighted_wide_batch_refuses_leaves_the_previous_weighting_in_force(torch_cuda, CH):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    c, cap = CH
    L = nka_amd.load()
    h = C.c_void_p()
    create = L.nka_hip_batch_create_wide_ext
    for step in (-1, 2, 7):                                  # step outside {0, 1}
        assert create(C.byref(h), 2, c + 1, 3, 0.01, -1, 0, None, step) == EINVAL and h.value is None
        assert b"step" in L.nka_hip_last_error()
    for nsys, vlen, mvec in [(2, cap + 1, 3), (65536, 8, 3), (2, 8, 33), (0, 8, 3), (2, 0, 3)]:      # the limits of create_wide
        for step in (0, 1):
            assert create(C.byref(h), nsys, vlen, mvec, 0.01, -1, 0, None, step) == EINVAL and h.value is None
    with pytest.raises(NKAError):
        nka_amd.nka_batch().init(3, c + 33, 3, wide=True, ext=True, storage=nka_amd.STORE_F32)
    with pytest.raises(NKAError):
        nka_amd.nka_batch().init(3, 33, 3, wide=True, ext=True, waves=True)
    with pytest.raises(NKAError, match="waves=True"):
        nka_amd.nka_batch().init(3, 33, 3, ext=True)

    nsys, n, mvec = 3, c + 33, 3
    rng = np.random.default_rng(11)
    W0 = WW.system_weights(n, nsys, c)
    b, twin = _ext(nsys, n, mvec), _ext(nsys, n, mvec).set_dot_weights(W0)
    assert not b.dot_weighted() and b.set_dot_weights(_f64(torch, W0)) is b and b.dot_weighted()
    hb = b._handle()

    def still_the_twins(calls=2):
        for _ in range(calls):
            Xh = rng.standard_normal((nsys, n))
            Fa, Fb = _f64(torch, Xh), _f64(torch, Xh)
            b.accel_update(Fa)
            twin.accel_update(Fb)
            assert torch.equal(Fa, Fb)
            _same_state(b, twin, nsys, "twins")

    still_the_twins()
    # accel_step is refused where step == 0
    with pytest.raises(NKAError):
        b.accel_step(_f64(torch, rng.standard_normal((nsys, n))))
    # an entry in the LAST row only: negative, NaN, Inf -- through both entries
    for bad in (-1.0, np.nan, np.inf):
        Wb = np.ones((nsys, n))
        Wb[nsys - 1, c + 7] = bad
        with pytest.raises(NKAError, match=r"first in row %d at index %d" % (nsys - 1, c + 7)):
            b.set_dot_weights(Wb)
        with pytest.raises(NKAError):
            b.set_dot_weights(_f64(torch, Wb))
        assert b.dot_weighted()
    ok = torch.ones(nsys * n, dtype=torch.float64, device="cuda")
    for ldw in (1, n - 1, -1, -n):                           # 0 < ldw < vlen, and negative
        assert L.nka_hip_batch_set_dot_weights(hb, C.c_void_p(ok.data_ptr()), ldw) == EINVAL, ldw
        assert L.nka_hip_batch_set_dot_weights_host(hb, np.ones(nsys * n).ctypes.data_as(C.c_void_p), ldw) == EINVAL, ldw
    # a device buffer one element too short, in both forms (a buffer of exactly known size: the library's own allocator)
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    ldw = n + 3
    for count, form in (((nsys - 1) * ldw + n - 1, ldw), (n - 1, 0)):
        assert L.nka_hip_vec_alloc(ws, count, C.byref(short)) == 0
        torch.cuda.synchronize()
        assert L.nka_hip_batch_set_dot_weights(hb, short, form) == EINVAL, form
        assert b"shorter" in L.nka_hip_last_error()
        assert L.nka_hip_vec_free(ws, short) == 0
    assert L.nka_hip_vec_workspace_destroy(ws) == 0
    for order in (nka_amd.SUMS_REFERENCE_ORDER, nka_amd.SUMS_BLOCKED, 17):
        with pytest.raises(NKAError):
            b.set_sum_order(order)
    b.set_sum_order(nka_amd.SUMS_AUTO).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    assert b.dot_weighted()
    still_the_twins()                                        # the previous weighting stayed in force
    # NKA_HIP_ESTATE while the stream is capturing
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cb = _ext(nsys, n, mvec).set_dot_weights(W0)
        static = torch.zeros(nsys, n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        cb.accel_update(static)
        rc = L.nka_hip_batch_set_dot_weights(cb._handle(), C.c_void_p(ok.data_ptr()), n)
        rc_host = L.nka_hip_batch_set_dot_weights_host(cb._handle(), np.ones(nsys * n).ctypes.data_as(C.c_void_p), n)
    assert rc == ESTATE and rc_host == ESTATE and cb.dot_weighted()
    cb.delete()
    # the shared form after the per-row form on a live batch; cleared and restarted: a fresh plain wide batch
    b.set_dot_weights(W0[2])
    twin.set_dot_weights(_f64(torch, np.tile(W0[2], (nsys, 1))))
    still_the_twins()
    assert b.set_dot_weights(None) is b and not b.dot_weighted()
    b.restart()
    twin.delete()
    twin = _plain(nsys, n, mvec)
    for _ in range(3):
        Xh = rng.standard_normal((nsys, n))
        Fa, Fb = _f64(torch, Xh), _f64(torch, Xh)
        b.accel_update(Fa)
        twin.accel_update(Fb)
        assert torch.equal(Fa, Fb)
        for k in range(nsys):                                # (h, c and the digest: a restarted block keeps stale entries a fresh one never had)
            assert _bits_equal(b.reductions(k), twin.reductions(k)), ("cleared", k)
            assert _decisions(b.state(k))[0] == _decisions(twin.state(k))[0], ("cleared", k, "list")
    b.set_dot_weights(W0)
    b.delete()                                               # destroy after set
    twin.delete()


def test_the_offers_table_over_all_nine_creations(torch_cuda, CH):
    import nka_amd
    c = CH[0]
    new = nka_amd.nka_batch
    #                                                        kind, is_wide, step, lengths, weights
    table = {"narrow": (new().init(3, 33, 3), 0, False, True, True, True),
             "stored": (new().init(3, 33, 3, storage=nka_amd.STORE_F32), 0, False, True, True, True),
             "lanes": (new().init(3, 33, 3, lanes=True), 2, False, True, False, False),
             "waves": (new().init(3, 33, 3, waves=True), 3, False, True, False, False),
             "waves ext": (new().init(3, 33, 3, waves=True, ext=True), 3, False, True, True, True),
             "wide": (new().init(3, c + 33, 3, wide=True), 1, True, False, True, False),
             "wide step": (new().init(3, c + 33, 3, wide=True, step=True), 1, True, True, True, False),
             "wide ext": (new().init(3, c + 33, 3, wide=True, ext=True), 1, True, False, True, True),
             "wide ext step": (new().init(3, c + 33, 3, wide=True, ext=True, step=True), 1, True, True, True, True)}
    assert len(table) == 9
    for name, (b, kind, wide, step, lengths, weights) in table.items():
        got = (b.kind(), b.is_wide(), b.offers_step(), b.offers_lengths(), b.offers_weights())
        assert got == (kind, wide, step, lengths, weights), (name, got)
        assert not b.dot_weighted()
    for name in ("wide", "wide step"):                       # the two old wide entries keep refusing, with today's message
        with pytest.raises(nka_amd.NKAError, match="not offered by a wide batch"):
            table[name][0].set_dot_weights(np.ones(c + 33))
    for b, *_ in table.values():
        b.delete()


# ---- 12. large offsets ----------------------------------------------------------------------------------------------------------------

def test_weight_rows_of_a_wide_batch_beyond_2_to_the_32_bytes(torch_cuda, CH):
    """520 wide systems of cap - 32 elements, mvec = 1, of which five run and the rest are masked out: byte 2^32 of the batch's
    weight buffer (rows at the slot stride), of the caller's weight rows and of F (ldw = ld = vlen + 1) falls inside row 512, which
    runs with its two neighbours, the first and the last system.  The caller's rows are ones except on the systems that run.
    Compared with == against a twin of five systems, without lengths and with; the witnesses stay fresh."""
    import nka_amd
    torch = torch_cuda
    c, cap = CH
    sh = WW.large_shape(c, cap)
    need = sum(WW.large_bytes(sh).values())
    free, total = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip(f"wide-weights: {free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 8 GiB")
    nsys, vlen, mvec, ld, active = sh["nsys"], sh["vlen"], sh["mvec"], sh["ld"], sh["active"]
    na = len(active)
    assert na <= WW.MAX_ACTIVE and need <= WW.MAX_BYTES
    big = twin = None
    try:
        big, twin = _ext(nsys, vlen, mvec), _ext(na, vlen, mvec)
        fresh = big.state_digest(sh["witnesses"][0])
        i = np.arange(vlen)
        tw = np.stack([np.ldexp(1.0, 1 + j + (i + j) % 3) for j in range(na)])      # powers of two that differ from row to row
        wraw = torch.ones((nsys - 1) * ld + vlen, dtype=torch.float64, device="cuda")
        wrows = torch.as_strided(wraw, (nsys, vlen), (ld, 1))
        for j, k in enumerate(active):
            wrows[k].copy_(_f64(torch, tw[j]))
        big.set_dot_weights(wrows)
        twin.set_dot_weights(_f64(torch, tw))
        del wraw, wrows
        torch.cuda.empty_cache()
        PAD = 7.25
        fraw = torch.full(((nsys - 1) * ld + vlen,), PAD, dtype=torch.float64, device="cuda")
        F = torch.as_strided(fraw, (nsys, vlen), (ld, 1))
        Ft = torch.zeros(na, vlen, dtype=torch.float64, device="cuda")
        mask = torch.zeros(nsys, dtype=torch.int32, device="cuda")
        mask[torch.tensor(active, device="cuda")] = 1
        seqs = [B.Sequence(vlen, 5200 + 31 * j) for j in range(na)]
        lens = [vlen] * na
        for with_len in (False, True):
            if with_len:
                big.restart()
                twin.restart()
                full = [vlen] * nsys
                for k, L in sh["lens"].items():
                    full[k] = L
                lens = [sh["lens"][k] for k in active]
                big.set_lengths(full)
                twin.set_lengths(lens)
            for call in range(3):
                rows = BL.nan_paint(na, vlen, 8) if with_len else np.zeros((na, vlen))
                for j in range(na):
                    rows[j, :lens[j]] = seqs[j].next()[:lens[j]]
                for j, k in enumerate(active):
                    x = _f64(torch, rows[j])
                    F[k].copy_(x)
                    Ft[j].copy_(x)
                big.accel_update(F, mask)
                twin.accel_update(Ft)
                where = ("wide-weights", with_len, call)
                for j, k in enumerate(active):
                    got, want = F[k].cpu().numpy(), Ft[j].cpu().numpy()
                    assert BL.same_bytes(got, want), (where, k, "F")
                    assert BL.same_bytes(got[lens[j]:], rows[j, lens[j]:]), (where, k, "the tail was written")
                _same_state(big, twin, na, where, pairs=list(zip(active, range(na))))
            assert (big.num_vec()[active] >= 1).all()
        _same_slots(big, twin, na, "wide-weights, every slot", upto={k: L for k, L in zip(active, lens)}, pairs=list(zip(active, range(na))))
        nv = big.num_vec()
        idle = np.ones(nsys, bool)
        idle[active] = False
        assert (nv[idle] == 0).all()
        for k in sh["witnesses"]:
            assert big.state_digest(k) == fresh, ("witness", k)
            for s in range(1, mvec + 2):
                assert not big.w(k, s).any() and not big.v(k, s).any(), ("witness", k, "slot", s)
        for k in active:
            F[k].fill_(PAD)
        assert bool((fraw == PAD).all().item()), "an element of F that no running system owns was written"
    finally:
        for x in (big, twin):
            if x is not None:
                x.delete()
        torch.cuda.empty_cache()


# ---- the record (keep this test last) -------------------------------------------------------------------------------------------------
def test_worst_ratio_of_the_weighted_wide_sums_is_printed_and_inside_its_bound(capsys):
    import nka_amd
    assert hasattr(nka_amd.load(), "nka_hip_batch_create_wide_ext"), "the record is of a library that has the entry"
    ratio, k, where = WORST
    if not where:
        return
    with capsys.disabled():
        print("\n" + _worst_line())
    assert ratio <= (k + 1) / (1.0 - (k + 1) * X.U), (ratio, k, where)
