"""The WIDE batch with binary32 storage of its normalised subspace vectors (nka_hip_batch_create_wide_stored, nka_batch().init(...,
wide=True, wide_storage=STORE_F32[, step=True]); the Store32Args instances of nka_amd/csrc/nka_batch_wide.hip; include/
nka_hip_batch.h, WIDE STORED).  Shapes are given in units of C = NKA_HIP_BATCH_WIDE_CHUNK, read from the library; q(x) =
astype(float32).astype(float64) (tests/batch_store32.py).

  1 one chunk            a binary32 wide batch of at most C elements is the binary32 narrow batch, bit for bit
  2 several chunks       the three layers of WideRun on Run32's mirror (the widened stored values and q(w1')); once more weighted,
                         once with lengths, once as a step
  3 chunk order          red[0] == ((p0 + p1) + p2) + ..., p_c from ONE binary32 narrow batch whose rows are the chunks
  4 binary64             nka_hip_batch_create_wide_stored(..., STORE_F64) is nka_hip_batch_create_wide_ext
  5 twins                unit weights; a step against an update under the predicted mask; lengths against twins of that length;
                         independence of nsys, position, neighbours' masks and ld parity; a masked system has no byte written
  6 range                beyond the binary32 range: +-Inf, inside its own system; subnormals and +-0 as numpy narrows them
  7 capture, a solve     the ragged weighted solve captured before the first call, replayed with no host in the loop
  8 refusals, lifecycle
  9 large offsets        float slots beyond 2^31 elements and 2^32 bytes

Tolerances are derived (gamma(wide_k(n)), batch_wide_step.norm_bound); nothing is fitted.  The worst |red - exact| / (u sum|xy|) of
part 2 and the K it was held to go to batch_wide_store32_exact_worst.json, the retirements of part 7 to batch_wide_store32_solve.json."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import batch_large as G
import batch_lengths as BL
import batch_seq as B
import batch_store32 as S32
import batch_wide as BW
import batch_wide_step as WS
import batch_wide_store32 as W32
import batch_wide_weights as WW
import exact_sums as X
import test_batch_sums_exact_gpu as T
from split_update import _bits_equal
from test_batch_large_gpu import _fill_the_lists, _sequences
from test_batch_store32_gpu import F32_MIN_NORMAL, Large32, Run32
from test_batch_wide_weights_gpu import _f64, _i32, _ld, _rows, _same_slots, _same_state, _weights_in_form

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PLANTED = -7.0                     # what fnorm holds before a call: kept by every system inactive on entry
WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|xy|) seen, the K it was held to, where


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
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(f"wide batch sums, binary32 storage: worst |red - exact| = {ratio:.3f} u sum|xy| against K = {k} there ({where})")
    out = P.dump_dir(ROOT)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_wide_store32_exact_worst.json"), "w") as fh:
            json.dump({"wide_store32": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


def _wide32(nsys, n, mvec, step=False, **kw):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, n, mvec, wide=True, wide_storage=nka_amd.STORE_F32, step=step, **kw)
    assert b.storage() == nka_amd.STORE_F32 and b.flavor() == nka_amd.FLAVOR_C and b.is_wide() and b.kind() == nka_amd.KIND_WIDE
    assert b.offers_weights() and b.offers_lengths() and b.offers_step() == step
    assert b.vector_bytes() == W32.vector_bytes(nsys, n, mvec, W32.STORE_F32)
    return b


def _narrow32(nsys, n, mvec):
    import nka_amd
    return nka_amd.nka_batch().init(nsys, n, mvec, storage=nka_amd.STORE_F32)


def _wide64(nsys, n, mvec, step=False):
    import nka_amd
    return nka_amd.nka_batch().init(nsys, n, mvec, flavor=nka_amd.FLAVOR_C, wide=True, ext=True, step=step)


# ---- 1. one chunk is the binary32 narrow batch -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["1", "2", "513", "C-1", "C"])
def test_one_chunk_is_the_binary32_narrow_batch_bit_for_bit(torch_cuda, CH, which):
    """Three systems with staggered starts, mvec 1 / 3 / 10, both parities of ld; accel_update and accel_step (with X, a mask,
    thresholds that retire a system at call 4, and fnorm); no weights, one shared row, one row per system; with and without
    per-system lengths.  The twin is a batch of nka_hip_batch_create_stored with the same weights and lengths.  After every call, with
    ==: F, X and their padding, fnorm, the mask, red[], the state, num_vec, the digest; every slot after every call at mvec <= 3 and
    after the last one at mvec = 10."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    n = WW.shape(which, c)
    assert BW.nchunk(n, c) == 1 and n <= nka_amd.BATCH_MAX_VLEN
    nsys, calls = 3, 6
    W = WW.system_weights(n, nsys, c)
    combos = [(None, False, False), ("rows", True, False), ("shared", False, True), ("rows", True, True), (None, True, True)]
    for mvec in (1, 3, 10):
        for ci, (form, step, lengths) in enumerate(combos):
            odd = bool((ci + mvec) % 2)
            ld, ldx = _ld(n, odd), _ld(n, not odd)
            lens = [n, max(1, n // 2), max(1, n - 1)] if lengths else [n] * nsys
            wide, twin = _wide32(nsys, n, mvec, step), _narrow32(nsys, n, mvec)
            if form:
                wide.set_dot_weights(_weights_in_form(torch, W, form, odd))
                twin.set_dot_weights(_weights_in_form(torch, W, form, not odd))
            if lengths:
                wide.set_lengths(lens)
                twin.set_lengths(lens)
            rng = np.random.default_rng([1, n, mvec, ci])
            seqs = [B.Sequence(n, 9100 * n + 10 * k + ci) for k in range(nsys)]
            paint = BL.nan_paint(nsys, ld, 5) if lengths else np.zeros((nsys, ld))
            fhost = paint.copy()
            xhost = BL.nan_paint(nsys, ldx, 6) if lengths else rng.standard_normal((nsys, ldx))
            for k, L in enumerate(lens):
                xhost[k, :L] = rng.standard_normal(L)
            (fw_raw, Fw), (ft_raw, Ft) = _rows(torch, nsys, n, ld, fhost), _rows(torch, nsys, n, ld, fhost)
            (xw_raw, Xw), (xt_raw, Xt) = _rows(torch, nsys, n, ldx, xhost), _rows(torch, nsys, n, ldx, xhost)
            alive = np.ones(nsys, bool)
            for t in range(calls):
                where = (which, mvec, form, "step" if step else "update", lengths, t)
                entry = alive & (t >= np.arange(nsys))       # staggered starts: with and without a pending pair in one launch
                for k in np.flatnonzero(entry):
                    fhost[k, :lens[k]] = seqs[k].next()[:lens[k]]
                for raw in (fw_raw, ft_raw):
                    raw.copy_(torch.from_numpy(fhost.ravel()))
                mw, mt = _i32(torch, entry), _i32(torch, entry)
                if step:
                    tolh = np.full(nsys, -1.0)
                    if t == 4:
                        tolh[1] = np.inf                     # system 1 retires
                    fnw, fnt = _f64(torch, np.full(nsys, PLANTED)), _f64(torch, np.full(nsys, PLANTED))
                    wide.accel_step(Fw, Xw, mw, _f64(torch, tolh), fnw)
                    twin.accel_step(Ft, Xt, mt, _f64(torch, tolh), fnt)
                    assert torch.equal(mw, mt) and _bits_equal(fnw.cpu().numpy(), fnt.cpu().numpy()), (where, "mask, fnorm")
                    assert BL.same_bytes(xw_raw.cpu().numpy(), xt_raw.cpu().numpy()), (where, "X and its padding")
                    alive &= ~(entry & (mw.cpu().numpy() == 0))
                    assert (fnw.cpu().numpy()[~entry] == PLANTED).all(), where
                else:
                    wide.accel_update(Fw, mw)
                    twin.accel_update(Ft, mt)
                assert BL.same_bytes(fw_raw.cpu().numpy(), ft_raw.cpu().numpy()), (where, "rows of F and their padding")
                fhost = fw_raw.cpu().numpy().reshape(nsys, ld)
                _same_state(wide, twin, nsys, where)
                if mvec <= 3 or t == calls - 1:
                    _same_slots(wide, twin, nsys, where)
            assert wide.num_vec().max() >= 1 or n < 65, (which, wide.num_vec())
            assert not step or not alive[1]
            wide.delete()
            twin.delete()


# ---- 2. several chunks: the three layers -------------------------------------------------------------------------------------------------

def _hold(what, red, x, y, k, where):
    ex = X.exact_dot(x, y)
    assert math.isfinite(ex), (what, where)
    tot = X.abs_dot(x, y)
    err = abs(red - ex)
    ratio = err / (X.U * tot) if tot else err
    print(f"  {what} {where}: |red - exact| = {ratio:.3f} u sum|xy|, K = {k}")
    assert err <= X.gamma(k) * tot, (what, where, red, ex, ratio, k)
    if tot > 0 and ratio >= WORST[0]:
        WORST[:] = [ratio, k, f"{what} {where}"]


class _Proxy:
    """A batch behind the calls BatchRun makes; everything not overridden is the batch's."""

    def __init__(self, b):
        self._b = b

    def __getattr__(self, name):
        return getattr(self._b, name)

    def set_sum_order(self, order):
        self._b.set_sum_order(order)
        return self


class _WithLengths(_Proxy):
    """A binary32 wide batch of vlen = n + extra -- one chunk more than a system owns -- whose systems are all n long: accel_update
    runs on rows of vlen doubles whose tails hold NaNs of distinct payloads and must keep them; get_w / get_v are cut to n."""

    def __init__(self, torch, nsys, n, mvec, extra):
        super().__init__(_wide32(nsys, n + extra, mvec))
        self._b.set_lengths([n] * nsys)
        self._n, self._paint = n, BL.nan_paint(nsys, n + extra, 7)
        self._big = torch.from_numpy(self._paint.copy()).cuda()

    def accel_update(self, F, mask=None):
        n = self._n
        self._big[:, :n].copy_(F)
        self._b.accel_update(self._big, mask)
        F.copy_(self._big[:, :n])
        assert BL.same_bytes(self._big.cpu().numpy()[:, n:], self._paint[:, n:]), "an element at or beyond the length was written"
        return self

    def w(self, k, s):
        return self._b.w(k, s)[:self._n]

    def v(self, k, s):
        return self._b.v(k, s)[:self._n]


class _StepAsUpdate(_Proxy):
    """A binary32 wide STEP batch whose accel_update is accel_step with X, the mask and fnorm (no thresholds: nobody retires).  After
    every call: x = fl(x - f_out) on the systems that ran, bit for bit, every other row of X untouched; fnorm within
    batch_wide_step.norm_bound of sqrt(exact_dot(fl(w f), f)), PLANTED where the system sat out."""

    def __init__(self, torch, b, nsys, n, wts):
        super().__init__(b)
        self._torch, self._n, self._wts = torch, n, wts
        self._xh = np.random.default_rng([77, n]).standard_normal((nsys, n))
        self._X = _f64(torch, self._xh)
        self.steps = 0

    def accel_update(self, F, mask=None):
        nsys, n = self._xh.shape[0], self._n
        fin = F.cpu().numpy().copy()
        fn = _f64(self._torch, np.full(nsys, PLANTED))
        self._b.accel_step(F, self._X, mask, None, fn)
        out, fnh = F.cpu().numpy(), fn.cpu().numpy()
        act = np.ones(nsys, bool) if mask is None else mask.cpu().numpy().astype(bool)
        want = self._xh.copy()
        want[act] = self._xh[act] - out[act]
        xg = self._X.cpu().numpy()
        assert _bits_equal(xg, want), ("X", self.steps)
        self._xh = xg
        c = BW.limits()[0]
        for k in range(nsys):
            if not act[k]:
                assert fnh[k] == PLANTED, ("fnorm of a system that sat out", k)
                continue
            a = self._wts[k] * fin[k] if self._wts is not None else fin[k]
            r = math.sqrt(X.exact_dot(a, fin[k]))
            assert abs(fnh[k] - r) <= WS.norm_bound(n, c) * r, ("fnorm", self.steps, k, fnh[k], r)
        self.steps += 1
        return self


class WideRun32(Run32):
    """Run32 -- the mirror of the widened stored values and of the binary64 pending pair, the three layers under the STORAGE contract --
    on a batch of nka_hip_batch_create_wide_stored, its sums held to wide_k(n) after the condition of WideRun on the operands actually
    used (batch_wide.undetectable_chunks == []).  weighted: general weights per system by the rule of batch_wide_weights, fl(w x) the
    first operand of every sum.  A second such batch set to SUMS_BLOCKED_ROUNDED explicitly takes every call and returns the same bits.
    mode "lengths": both batches are _WithLengths; mode "step": the batch is a step batch behind _StepAsUpdate and the second one
    keeps running accel_update -- a step that retires nobody is the update, bit for bit."""

    def __init__(self, torch, oracle, n, mvec, nsys, odd_ld=False, weighted=False, mode=None):
        self.weighted, self.mode = weighted, mode
        super().__init__(torch, oracle, n, mvec, nsys, odd_ld)
        self.k = BW.wide_k(n)
        self.chunk = BW.limits()[0]
        self.held, self.cells, self._sys = {}, 0, None

    def _device(self, odd_ld):
        import nka_amd
        torch, n, nsys, ld = self.torch, self.n, self.nsys, self.ld
        if self.mode == "lengths":
            extra = BW.limits()[0] + 5
            self.b = _WithLengths(torch, nsys, n, self.m, extra)
            self.explicit = _WithLengths(torch, nsys, n, self.m, extra).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        else:
            self.b = _wide32(nsys, n, self.m, self.mode == "step")
            self.explicit = _wide32(nsys, n, self.m).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        self.order, self.orders_met = nka_amd.SUMS_BLOCKED_ROUNDED, set()
        self.reference = nka_amd.SUMS_REFERENCE_ORDER
        self.raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda")
        self.F = self.raw.view(nsys, ld)[:, :n]
        self.Fx = torch.zeros_like(self.raw).view(nsys, ld)[:, :n]
        align = [(self.raw.data_ptr() + 8 * k * ld) % 16 for k in range(nsys)]
        if odd_ld:
            assert ld % 2 == 1 and align == [8 * (k % 2) for k in range(nsys)], align
        else:
            assert ld % 2 == 0 and not any(align), align
        if self.weighted:
            c = BW.limits()[0]
            self.wts = WW.system_weights(n, nsys, c)
            for x in (self.b, self.explicit):
                x.set_dot_weights(_weights_in_form(torch, self.wts, "rows", not odd_ld))
            assert self.b.dot_weighted()
        if self.mode == "step":
            self.b = _StepAsUpdate(torch, self.b, nsys, n, self.wts if self.weighted else None)

    def _check(self, k, *args):
        self._sys = k
        super()._check(k, *args)

    def _sum(self, what, red, x, y, where):
        a = self.wts[self._sys] * x if self.weighted else x      # fl(w x): rounded once, before the product
        if self.n > self.chunk:
            unseen = BW.undetectable_chunks(a, y, self.k, self.chunk)
            assert not unseen, (what, where, "the bound could not see these chunks' partials lost: another seed", unseen)
            self.cells += BW.nchunk(self.n, self.chunk)
        _hold(what, red, a, y, self.k, where)
        if red != 0.0:
            self.held[what] = self.held.get(what, 0) + 1


def _input32(n, rng, prev):
    """batch_wide.wide_planted_input with two components off the sentinels scaled by 1e-42 and 1e-50: their share of the normalised
    difference lands in the binary32 subnormal range and at +-0."""
    x = BW.wide_planted_input(n, rng, prev)
    free = np.setdiff1d(np.arange(n), BW.wide_sentinel_indices(n))
    x[free[free.size // 3]] *= 1e-42
    x[free[2 * free.size // 3]] *= 1e-50
    return x


def _planned_run32(run, seed):
    """test_batch_sums_exact_gpu._planned_run -- six systems with different starting delays, a masked relax, a masked restart and a
    repeated input (s == 0) each -- with the sentinels of a wide system and the two tiny components."""
    rngs, prev = [np.random.default_rng([seed, k]) for k in range(run.nsys)], [None] * run.nsys
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
            inputs[k] = prev[k].copy() if j == T.PLAN[k][2] else _input32(run.n, rngs[k], prev[k])
            prev[k] = inputs[k]
        run.update(inputs)
    return run


def _late_second_system32(run, calls, seed):
    rngs, prev = [np.random.default_rng([seed, run.n, k]) for k in range(2)], [None, None]
    for t in range(calls):
        inputs = {}
        for k in range(2):
            if t >= k:
                inputs[k] = prev[k] = _input32(run.n, rngs[k], prev[k])
        run.update(inputs)
    assert run.lengths_differed and run.cells > 0
    return run


@pytest.mark.parametrize("mvec", [3, 10])
@pytest.mark.parametrize("which", ["C+1", "2C+513", "8C+1", "9C+1"])
def test_every_part_of_a_binary32_wide_update(torch_cuda, oracle, CH, which, mvec):
    """2, 3, 9 and 10 chunks.  mvec = 10: the plan of six systems (older counts 0 ... 10, a repeated input for s == 0, a masked relax
    and a masked restart each); mvec = 3: two systems, the second one call late on an unaligned row, six updates."""
    c = CH[0]
    n = WW.shape(which, c)
    assert BW.wide_k(n) == 2 * (c // 512) + 9 + (WW.EXACT_CHUNKS[which] - 1)
    odd = WW.EXACT_CHUNKS[which] % 2 == 1
    if mvec == 10:
        run = _planned_run32(WideRun32(torch_cuda, oracle, n, T.SHAPE_MVEC, len(T.PLAN), odd), seed=n)
        T._assert_planned_coverage(run)
        assert run.saw_zero_s and run.saw_after_restart and run.cells > 0
        assert run.subnormal > 0 and run.flushed > 0, (n, run.subnormal, run.flushed)
    else:
        run = _late_second_system32(WideRun32(torch_cuda, oracle, n, 3, 2, odd_ld=True), 6, seed=3)
        assert run.widest == 3 and run.held["<d,d>"] >= 5


def test_every_older_count_of_a_binary32_wide_system_up_to_the_largest_subspace(torch_cuda, oracle, CH):
    """mvec = 32 once at 2C + 513: every group count of the sums kernel, up to eight groups of four float loads."""
    n, mvec = 2 * CH[0] + 513, 32
    run = _late_second_system32(WideRun32(torch_cuda, oracle, n, mvec, 2, odd_ld=True), mvec + 2, seed=mvec)
    assert run.widest == mvec and run.nolder_normed == set(range(mvec + 1)), run.nolder_normed
    assert run.held.get("<f,w_31>", 0) >= 1 and run.subnormal > 0, run.held


def test_every_part_of_a_weighted_binary32_wide_update(torch_cuda, oracle, CH):
    """The same layers once more WEIGHTED, at 2C + 513 with the whole plan: fl(w x) the first operand, fl(w q(w1')) in the Gram row."""
    n = 2 * CH[0] + 513
    run = _planned_run32(WideRun32(torch_cuda, oracle, n, T.SHAPE_MVEC, len(T.PLAN), True, weighted=True), seed=n + 1)
    T._assert_planned_coverage(run)
    assert run.cells > 0 and run.held["<w1',w_0>"] >= 1


def test_every_part_of_a_binary32_wide_update_with_lengths(torch_cuda, oracle, CH):
    """... once with LENGTHS: systems of 2C + 513 unknowns in a batch laid out for 3C + 518 (a fourth chunk whose workgroups return at
    once), the whole plan; the tails of the rows keep their NaNs, and what the layers hold is [0, len) of every row and slot."""
    n = 2 * CH[0] + 513
    run = _planned_run32(WideRun32(torch_cuda, oracle, n, T.SHAPE_MVEC, len(T.PLAN), True, mode="lengths"), seed=n + 2)
    T._assert_planned_coverage(run)
    assert run.cells > 0 and run.b.has_lengths() and run.subnormal > 0


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_every_part_of_a_binary32_wide_step(torch_cuda, oracle, CH, weighted):
    """... and once as a STEP: accel_step with X, the mask and fnorm in place of accel_update, the whole plan at 2C + 513; beside the
    three layers x = fl(x - f_out), fnorm against the exact (weighted) norm, and an update batch that takes the same calls."""
    n = 2 * CH[0] + 513
    run = _planned_run32(WideRun32(torch_cuda, oracle, n, T.SHAPE_MVEC, len(T.PLAN), False, weighted=weighted, mode="step"), seed=n + 3)
    T._assert_planned_coverage(run)
    assert run.cells > 0 and run.b.steps == T.SHAPE_CALLS and run.b.offers_step()


# ---- 3. the chunk order, in bits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["2C+513", "9C+1"])
def test_red0_is_the_chunk_order_sum_of_one_binary32_narrow_batch_of_the_chunks(torch_cuda, CH, which):
    """red[0] of the second update of a fresh binary32 wide system is ((p0 + p1) + p2) + ..., bit for bit, at 3 and 10 chunks.  p_c is
    red[0] of system c of ONE binary32 narrow batch of nchunk systems whose rows of F are the chunks; the last chunk through
    set_lengths, with NaN behind it.  And red[0], formed from the binary64 pending rows, is that of a binary64 wide batch."""
    torch = torch_cuda
    c = CH[0]
    vlen = WW.shape(which, c)
    chunks = BW.nchunk(vlen, c)
    assert chunks == {"2C+513": 3, "9C+1": 10}[which]
    rng = np.random.default_rng([33, vlen])
    x0 = BW.wide_planted_input(vlen, rng)
    x1 = BW.wide_planted_input(vlen, rng, prev=x0)
    last = vlen - (chunks - 1) * c
    wide, wide64 = _wide32(1, vlen, 3), _wide64(1, vlen, 3)
    narrow = _narrow32(chunks, c, 3)
    narrow.set_lengths(np.array([c] * (chunks - 1) + [last], np.int64))
    for x in (x0, x1):          # second update of a fresh system: a pending pair, no older vector
        wide.accel_update(_f64(torch, x).view(1, vlen))
        wide64.accel_update(_f64(torch, x).view(1, vlen))
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
    assert got == wide64.reductions(0)[0], "d, red[0] and s are those of binary64 storage"
    for b in (wide, wide64, narrow):
        b.delete()


# ---- 4. binary64 through the new entry ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [False, True], ids=["update", "step"])
def test_binary64_through_the_new_entry_is_create_wide_ext(torch_cuda, CH, step):
    """20 calls at 2C + 513, weights set at call 7 and lengths at call 13: F, X, fnorm, the mask, red[], the state, the digest with ==
    after every call, every slot at the end; the handle reports what a batch of nka_hip_batch_create_wide_ext reports."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    n, nsys, mvec = 2 * c + 513, 4, 5
    new, old = W32.create_through_the_new_entry(nsys, n, mvec, step, W32.STORE_F64), _wide64(nsys, n, mvec, step)
    for b in (new, old):
        assert b.storage() == nka_amd.STORE_F64 and b.vector_bytes() == W32.vector_bytes(nsys, n, mvec, W32.STORE_F64)
        assert b.is_wide() and b.kind() == nka_amd.KIND_WIDE and b.offers_weights() and b.offers_lengths() and b.offers_step() == step
    W = WW.system_weights(n, nsys, c)
    lens = [n, c, c + 1, 513]
    seqs = [B.Sequence(n, 4400 + k) for k in range(nsys)]
    rng = np.random.default_rng(44)
    xh = rng.standard_normal((nsys, n))
    Xa, Xb = _f64(torch, xh), _f64(torch, xh)
    for t in range(20):
        if t == 7:
            for b in (new, old):
                b.set_dot_weights(_f64(torch, W))
        if t == 13:
            for b in (new, old):
                b.set_lengths(lens)
        fh = np.stack([s.next() for s in seqs])
        Fa, Fb = _f64(torch, fh), _f64(torch, fh)
        entry = (t >= np.arange(nsys)) & (np.arange(nsys) != t % 5)
        ma, mb = _i32(torch, entry), _i32(torch, entry)
        if step:
            tolh = np.full(nsys, -1.0)
            fa, fb = _f64(torch, np.full(nsys, PLANTED)), _f64(torch, np.full(nsys, PLANTED))
            new.accel_step(Fa, Xa, ma, _f64(torch, tolh), fa)
            old.accel_step(Fb, Xb, mb, _f64(torch, tolh), fb)
            assert torch.equal(Xa, Xb) and torch.equal(ma, mb) and _bits_equal(fa.cpu().numpy(), fb.cpu().numpy()), t
        else:
            new.accel_update(Fa, ma)
            old.accel_update(Fb, mb)
        assert torch.equal(Fa, Fb), t
        _same_state(new, old, nsys, (step, t))
    _same_slots(new, old, nsys, (step, "end"))
    assert new.num_vec().max() >= 2
    with pytest.raises(nka_amd.NKAError):
        new.set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    new.delete()
    old.delete()


# ---- 5. twins ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["C+1", "2C+513"])
def test_unit_weights_are_the_unweighted_binary32_wide_batch(torch_cuda, CH, which):
    """w == 1 in the shared form and in one row per system, update and step, both parities of ld: F, X, fnorm, the mask, red[], the
    state, the digest and every slot with ==."""
    torch = torch_cuda
    n = WW.shape(which, CH[0])
    nsys, mvec, calls = 4, 3, 6
    for step, odd in ((False, False), (True, True)):
        ld = _ld(n, odd)
        batches = {"plain": _wide32(nsys, n, mvec, step),
                   "shared": _wide32(nsys, n, mvec, step).set_dot_weights(_f64(torch, np.ones(n))),
                   "rows": _wide32(nsys, n, mvec, step).set_dot_weights(_weights_in_form(torch, np.ones((nsys, n)), "rows", not odd))}
        assert [b.dot_weighted() for b in batches.values()] == [False, True, True]
        rng = np.random.default_rng([5, n, step])
        fhost, xhost = np.zeros((nsys, ld)), rng.standard_normal((nsys, ld))
        F = {name: _rows(torch, nsys, n, ld, fhost) for name in batches}
        Xd = {name: _rows(torch, nsys, n, ld, xhost) for name in batches}
        for t in range(calls):
            entry = t >= np.arange(nsys) % 3
            for k in np.flatnonzero(entry):
                fhost[k, :n] = rng.standard_normal(n)
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
            for name in ("shared", "rows"):
                for got, want in zip(out[name], out["plain"]):
                    assert BL.same_bytes(got, want), (which, step, t, name, "F, X, mask or fnorm")
                _same_state(batches[name], batches["plain"], nsys, (which, step, t, name))
            fhost = out["plain"][0].reshape(nsys, ld)
        for name in ("shared", "rows"):
            _same_slots(batches[name], batches["plain"], nsys, (which, step, name))
        assert batches["rows"].num_vec().max() >= 2
        for b in batches.values():
            b.delete()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("which", ["C+1", "2C+513"])
def test_a_binary32_wide_step_is_the_update_under_the_predicted_mask(torch_cuda, CH, which, weighted):
    """accel_step against a binary32 wide twin that runs accel_update under the mask the host predicts from the step's own fnorm and
    tol: F, X, the mask, red[], the state and the digests with ==; fnorm within batch_wide_step.norm_bound of the exact norm."""
    torch = torch_cuda
    c = CH[0]
    n = WW.shape(which, c)
    nsys, mvec, calls = 6, 4, 11
    ld, ldx = _ld(n, True), _ld(n, False)
    wts = WW.system_weights(n, nsys, c) if weighted else None
    step, twin = _wide32(nsys, n, mvec, True), _wide32(nsys, n, mvec, False)
    if weighted:
        step.set_dot_weights(_f64(torch, wts))
        twin.set_dot_weights(_f64(torch, wts))
    rng = np.random.default_rng([52, n, int(weighted)])
    seqs = [B.Sequence(n, 5200 * 7 + 10 * k + n) for k in range(nsys)]
    (fs_raw, Fs), (ft_raw, Ft) = _rows(torch, nsys, n, ld), _rows(torch, nsys, n, ld)
    xhost = rng.standard_normal((nsys, ldx))
    x_raw, Xd = _rows(torch, nsys, n, ldx, xhost)
    fhost, alive, retired = np.zeros((nsys, ld)), np.ones(nsys, bool), 0
    for t in range(calls):
        where = (which, weighted, t)
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
        mask, fnorm = _i32(torch, entry), _f64(torch, np.full(nsys, PLANTED))
        step.accel_step(Fs, Xd, mask, _f64(torch, tolh), fnorm)
        fn, got = fnorm.cpu().numpy(), mask.cpu().numpy().astype(bool)
        assert (fn[~entry] == PLANTED).all(), (where, "fnorm of a system inactive on entry")
        for k in np.flatnonzero(entry):
            f = fhost[k, :n]
            want = math.sqrt(X.exact_dot(f * wts[k] if weighted else f, f))
            assert abs(fn[k] - want) <= WS.norm_bound(n, c) * want, (where, k, fn[k], want)
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
    _same_slots(step, twin, nsys, (which, weighted, "end"))
    assert retired >= 1 and alive.any() and step.num_vec().max() >= 1
    step.delete()
    twin.delete()


def test_lengths_against_binary32_wide_twins_of_that_length(torch_cuda, CH):
    """Lengths {1, C, C + 1, 2C + 513, 3C - 1} in one weighted binary32 wide step batch of vlen = 3C against twins created at vlen =
    len[sys].  Seven full-length updates first write every float slot and the pending rows over their whole length; the tails of F, X
    and the weight rows then hold NaNs of distinct payloads (the weights: 2^500, they must be finite), and F and X are compared byte
    for byte after every call.  After the run the tails of the pending rows and, after a relax, of every ring slot still hold what
    the full-length updates left."""
    torch = torch_cuda
    c = CH[0]
    vlen, mvec = 3 * c, 3
    lens = [1, c, c + 1, 2 * c + 513, 3 * c - 1]
    nsys = len(lens)
    b = _wide32(nsys, vlen, mvec, True)
    rng = np.random.default_rng(5532)
    for t in range(7):
        fin = rng.standard_normal((nsys, vlen))
        F = _f64(torch, fin)
        b.accel_update(F)
    pend_tail = [(fin[k, L:].copy(), F.cpu().numpy()[k, L:].copy()) for k, L in enumerate(lens)]
    b.restart()
    ring = {(k, s): (b.w(k, s), b.v(k, s)) for k in range(nsys) for s in range(1, mvec + 2)}
    assert all(w[lens[k]:].any() and v[lens[k]:].any() for (k, s), (w, v) in ring.items()), "a ring slot holds no paint"
    W = WW.system_weights(vlen, nsys, c)
    Wp = W.copy()
    for k, L in enumerate(lens):
        Wp[k, L:] = WW.TAIL_WEIGHT
    b.set_dot_weights(_f64(torch, Wp)).set_lengths(np.array(lens, np.int32))
    twins = [_wide32(1, L, mvec, True).set_dot_weights(_f64(torch, W[k, :L])) for k, L in enumerate(lens)]
    fpaint, xpaint = BL.nan_paint(nsys, vlen, 1), BL.nan_paint(nsys, vlen, 2)
    xh = xpaint.copy()
    for k, L in enumerate(lens):
        xh[k, :L] = rng.standard_normal(L)
    Xd = _f64(torch, xh)
    Xt = [_f64(torch, xh[k:k + 1, :L]) for k, L in enumerate(lens)]
    seqs = BL.sequences(lens, 5570)
    for t in range(8):
        if t == 5:
            b.relax(_i32(torch, [1, 0, 1, 0, 1]))
            for k in (0, 2, 4):
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
            assert _bits_equal(b.reductions(k), twins[k].reductions(0)), where
            sa, sb = b.state(k), twins[k].state(0)
            assert sa.list_order() == sb.list_order() and sa.pending == sb.pending, where
            for s in sa.list_order():
                assert BL.same_bytes(b.w(k, s)[:L], twins[k].w(0, s)) and BL.same_bytes(b.v(k, s)[:L], twins[k].v(0, s)), (where, s)
    assert b.num_vec().tolist() == [int(t_.num_vec()[0]) for t_ in twins]
    for k, L in enumerate(lens):                             # the pending rows beyond L: still the last full-length pair
        st = b.state(k)
        assert st.pending and BL.same_bytes(b.w(k, st.first)[L:], pend_tail[k][0]) and BL.same_bytes(b.v(k, st.first)[L:], pend_tail[k][1]), k
    b.relax()
    for (k, s), (w, v) in ring.items():                      # every ring slot beyond L: still the paint
        assert BL.same_bytes(b.w(k, s)[lens[k]:], w[lens[k]:]) and BL.same_bytes(b.v(k, s)[lens[k]:], v[lens[k]:]), (k, s)
    b.delete()
    for t_ in twins:
        t_.delete()


def test_a_binary32_wide_system_does_not_depend_on_the_batch_around_it(torch_cuda, CH):
    """One system of 2C + 513 unknowns, eight updates: alone; as system 3 of 5 beside neighbours that run, sit out or are fed NaN; on a
    row that is not 16-byte aligned.  F, red[], the digest and every slot with ==.  The masked neighbours have no byte written: row
    of F, red[], digest, every slot."""
    torch = torch_cuda
    n, mvec, calls = 2 * CH[0] + 513, 4, 8
    seq = [B.Sequence(n, 5900).next() for _ in range(calls)]
    rng = np.random.default_rng(59)

    def run(nsys, pos, others, odd):
        ld = _ld(n, odd)
        b = _wide32(nsys, n, mvec)
        host = rng.standard_normal((nsys, ld))
        out = []
        for t in range(calls):
            if others == "nan":
                host[:, :] = np.nan
            host[pos, :n] = seq[t]
            raw, F = _rows(torch, nsys, n, ld, host)
            before = raw.cpu().numpy().reshape(nsys, ld).copy()
            entry = np.ones(nsys, bool) if others in ("run", "nan") else np.arange(nsys) == pos
            snap = [(b.state_digest(k), b.reductions(k)) for k in range(nsys)]
            b.accel_update(F, _i32(torch, entry))
            got = raw.cpu().numpy().reshape(nsys, ld)
            for k in np.flatnonzero(~entry):                 # a masked system: no byte written
                assert BL.same_bytes(got[k], before[k]) and b.state_digest(k) == snap[k][0] and _bits_equal(b.reductions(k), snap[k][1])
            assert BL.same_bytes(got[:, n:], before[:, n:]), "the padding between two rows was written"
            out.append((got[pos, :n].copy(), b.reductions(pos), b.state_digest(pos)))
            host = got.copy()
        slots = [(b.w(pos, s), b.v(pos, s)) for s in range(1, mvec + 2)]
        if others == "masked":
            for k in range(nsys):
                if k != pos:
                    assert all(not b.w(k, s).any() and not b.v(k, s).any() for s in range(1, mvec + 2)), k
        b.delete()
        return out, slots

    ref, ref_slots = run(1, 0, "run", False)
    for nsys, pos, others, odd in ((5, 3, "run", False), (5, 3, "masked", True), (5, 3, "nan", True), (2, 1, "masked", True)):
        out, slots = run(nsys, pos, others, odd)
        for t in range(calls):
            assert _bits_equal(out[t][0], ref[t][0]) and _bits_equal(out[t][1], ref[t][1]) and out[t][2] == ref[t][2], (nsys, pos, others, t)
        for (w, v), (rw, rv) in zip(slots, ref_slots):
            assert _bits_equal(w, rw) and _bits_equal(v, rv), (nsys, pos, others)


# ---- 6. range ------------------------------------------------------------------------------------------------------------------------------

def test_a_value_beyond_the_binary32_range_stays_in_its_wide_system(torch_cuda, CH):
    """System 2 of five (2C + 513 unknowns) has a frozen entry at 1e10 in chunk 0 and a moving entry of about 1e-30 in chunk 2: s is about
    1e-30, fl(v1/s) about 1e40 at the frozen entry, and the stored v holds +-Inf exactly where q() says.  Every other system is == a
    twin batch in which system 2 sits every call out."""
    torch = torch_cuda
    c = CH[0]
    nsys, n, mvec, ill = 5, 2 * c + 513, 4, 2
    b, twin = _wide32(nsys, n, mvec), _wide32(nsys, n, mvec)
    rng = np.random.default_rng(6203)
    others = [k for k in range(nsys) if k != ill]
    tmask = _i32(torch, [int(k != ill) for k in range(nsys)])
    pw = pv = None
    met_inf = False
    for t in range(5):
        xh = rng.standard_normal((nsys, n))
        xh[ill] = 0.0
        xh[ill, 0], xh[ill, 2 * c + 7] = 1e10, 1e-30 * (t + 1)
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


def test_binary32_subnormals_and_zeros_are_stored_as_numpy_narrows_them(torch_cuda, CH):
    """Inputs with components of about 1e-42 and 1e-50 in every chunk: the stored w1' holds binary32 subnormals and +-0 there, each
    bit-equal to astype(float32) of fl(d/s) with the device's s; so does the stored v."""
    torch = torch_cuda
    c = CH[0]
    n = 2 * c + 513
    b = _wide32(1, n, 3)
    rng = np.random.default_rng(6242)
    x0, x1 = rng.standard_normal(n), rng.standard_normal(n)
    tiny, gone = np.arange(5, n, 700), np.arange(9, n, 700)
    sign = np.where(np.arange(tiny.size) % 2 == 0, 1.0, -1.0)
    x0[tiny], x1[tiny] = 3e-42 * sign, -2e-42 * sign         # d / s is about 5e-44: a few dozen binary32 subnormal steps
    x0[gone], x1[gone] = 3e-50 * sign, -2e-50 * sign         # ... and about 5e-52: +-0
    F0 = _f64(torch, x0).view(1, n)
    b.accel_update(F0)
    out0 = F0.cpu().numpy()[0]
    first = b.state(0).first
    b.accel_update(_f64(torch, x1).view(1, n))
    s = np.sqrt(np.float64(b.reductions(0)[0]))
    d = x0 - x1
    with np.errstate(all="ignore"):
        w1n = S32.q(d / s)
        v1s = S32.q(out0 / s - w1n)
    w, v = b.w(0, first), b.v(0, first)
    assert _bits_equal(w, w1n) and _bits_equal(v, v1s)
    assert ((w[tiny] != 0) & (np.abs(w[tiny]) < F32_MIN_NORMAL)).all(), "binary32 subnormals were flushed"
    assert (w[gone] == 0).all() and (d[gone] != 0).all() and (np.signbit(w[gone]) == np.signbit(d[gone])).all(), "+-0 keeps its sign"
    assert tiny.size >= 3 and {int(i) // c for i in tiny} == {0, 1, 2}
    b.delete()


# ---- 7. capture before the first call, and a whole solve -----------------------------------------------------------------------------------

def _ragged_solve(torch, c, storage):
    """The ragged weighted solve of tests/batch_wide_weights.py: [residual; accel_step] captured ONCE, before any update, and replayed
    SOLVE_REPLAYS times with no host in the loop, thresholds formed on the device after the first replay -> (the iteration at which
    each system retired, read from a per-replay record of the mask kept on the device; X; the batch's digests)."""
    import nka_amd
    nsys, vlen, mvec = WW.SOLVE_NSYS, WW.solve_vlen(c), WW.SOLVE_MVEC
    d, eps, bb, x0, left, right = (_f64(torch, a) for a in WW.solve_problem(c))
    lens, W = WW.solve_lengths(c), WW.solve_weights(c)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        if storage == nka_amd.STORE_F32:
            b = _wide32(nsys, vlen, mvec, True)
        else:
            b = _wide64(nsys, vlen, mvec, True)
        b.set_dot_weights(_f64(torch, W)).set_lengths(lens)
        Xs, Fs = x0.clone(), torch.zeros_like(x0)
        mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
        alive = torch.zeros(nsys, dtype=torch.int32, device="cuda")      # replays each system was still active after
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        Fs.copy_(WW.solve_residual(torch, Xs, d, eps, bb, left, right))
        b.accel_step(Fs, Xs, mask, tol, fnorm)
        alive.add_(mask)
    assert b.num_vec().max() == 0
    with torch.cuda.stream(side):
        g.replay()
        torch.mul(fnorm, WW.SOLVE_TOL, out=tol)
        for _ in range(WW.SOLVE_REPLAYS - 1):
            g.replay()
    torch.cuda.synchronize()
    retired = alive.cpu().numpy().astype(np.int64)           # active after replays 0 .. r - 1, retired in replay r
    retired[mask.cpu().numpy() != 0] = -1
    inside = torch.from_numpy(np.arange(vlen)[None, :] < lens[:, None]).cuda()
    assert not bool(Xs[~inside].any()), "x beyond a system's length was written"
    x = Xs.cpu().numpy()
    b.delete()
    return retired, x


def test_a_ragged_weighted_binary32_wide_solve_replays_with_no_host_in_the_loop(torch_cuda, CH):
    """16 systems of C/2 ... 3C unknowns, weights zero on every 17th entry and 4^k elsewhere, binary32 storage.  Every system retires
    inside the budget the host model fixed on the CPU (tests/test_batch_wide_store32_cpu.py): SOLVE_REPLAYS - SOLVE_SLACK.  The
    binary64 wide batch runs the same capture beside it; both sets of iterations go to batch_wide_store32_solve.json and are
    printed; the solution is one in the norm the batch measures."""
    import nka_amd
    import parity_util as P
    torch = torch_cuda
    c = CH[0]
    it32, x32 = _ragged_solve(torch, c, nka_amd.STORE_F32)
    it64, x64 = _ragged_solve(torch, c, nka_amd.STORE_F64)
    print("binary32 wide retirements", it32.tolist(), "binary64 wide", it64.tolist())
    out = P.dump_dir(ROOT)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_wide_store32_solve.json"), "w") as fh:
            json.dump({"binary32": it32.tolist(), "binary64": it64.tolist(), "differ": int((it32 != it64).sum()),
                       "tol": WW.SOLVE_TOL, "mvec": WW.SOLVE_MVEC}, fh, indent=1, sort_keys=True)
    assert (it32 >= 0).all() and it32.max() <= WW.SOLVE_REPLAYS - WW.SOLVE_SLACK, it32
    assert (it64 >= 0).all() and len(set(it32.tolist())) >= 3, (it32, it64)
    d, eps, bb, _, left, right = WW.solve_problem(c)
    lens, W = WW.solve_lengths(c), WW.solve_weights(c)
    inside = np.arange(WW.solve_vlen(c))[None, :] < lens[:, None]
    for x in (x32, x64):
        res = WW.solve_residual(np, x, d, eps, bb, left, right)
        r0 = WW.solve_residual(np, np.zeros_like(x), d, eps, bb, left, right)
        wres = np.sqrt((np.where(inside, W, 0.0) * res * res).sum(axis=1))
        w0 = np.sqrt((np.where(inside, W, 0.0) * r0 * r0).sum(axis=1))
        assert (wres <= 2.0 * WW.SOLVE_TOL * w0).all(), (wres, w0)


@pytest.mark.parametrize("step", [False, True], ids=["update", "step"])
def test_a_binary32_wide_call_is_capturable_before_the_first_call(torch_cuda, CH, step):
    """Captured before any call has run -- four kernel nodes --, replayed through growth to a full list, the capacity drop and a masked
    relax; an eager binary32 wide twin takes the same calls."""
    torch = torch_cuda
    nsys, n, mvec = 6, 2 * CH[0] + 513, 3
    rng = np.random.default_rng(7204)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _wide32(nsys, n, mvec, step)
        Fs = torch.zeros(nsys, n, dtype=torch.float64, device="cuda")
        xs = torch.zeros(nsys, n, dtype=torch.float64, device="cuda")
    eager = _wide32(nsys, n, mvec, step)
    xe = torch.zeros(nsys, n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        if step:
            b.accel_step(Fs, xs)
        else:
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
        if step:
            eager.accel_step(Fe, xe)
            assert torch.equal(xs, xe), t
        else:
            eager.accel_update(Fe)
        assert torch.equal(Fs, Fe), t
        _same_state(b, eager, nsys, (step, t))
    assert b.num_vec().max() == mvec
    b.delete()
    eager.delete()


# ---- 8. refusals and lifecycle ---------------------------------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(torch_cuda, CH):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    L = nka_amd.nka_batch()._L
    c, cap = CH
    nsys, n, mvec = 24, 16 * c + 1, 20
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    h = C.c_void_p()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F32, F64 = nka_amd.STORE_F32, nka_amd.STORE_F64

    def create(nsys_=nsys, n_=n, mvec_=mvec, vtol=0.01, flavor=nka_amd.FLAVOR_C, step=0, storage=F32):
        return L.nka_hip_batch_create_wide_stored(C.byref(h), nsys_, n_, mvec_, vtol, flavor, 0, stream, step, storage)

    for flavor in (nka_amd.FLAVOR_F08, nka_amd.FLAVOR_F08_VECTOR):
        assert create(flavor=flavor) == EINVAL and h.value is None and b"flavour" in L.nka_hip_last_error()
        with pytest.raises(NKAError):
            nka_amd.nka_batch().init(nsys, n, mvec, flavor=flavor, wide=True, wide_storage=F32)
    for storage in (2, -1):
        assert create(storage=storage) == EINVAL and h.value is None and b"storage" in L.nka_hip_last_error()
    for step in (-1, 2):
        for storage in (F32, F64):
            assert create(step=step, storage=storage) == EINVAL and h.value is None and b"step" in L.nka_hip_last_error()
    for kw in (dict(nsys_=0), dict(nsys_=65536), dict(n_=0), dict(n_=cap + 1), dict(mvec_=0), dict(mvec_=33), dict(vtol=0.0)):
        for storage in (F32, F64):
            assert create(storage=storage, **kw) == EINVAL and h.value is None, kw
    assert L.nka_hip_batch_create_wide_stored(None, nsys, n, mvec, 0.01, 0, 0, stream, 0, F32) == EINVAL
    # the three pinned spellings keep raising; the new keyword needs wide=True
    for kw in (dict(wide=True), dict(wide=True, step=True), dict(wide=True, ext=True)):
        with pytest.raises(NKAError, match="wide"):
            nka_amd.nka_batch().init(nsys, n, mvec, storage=F32, **kw)
    for kw in (dict(), dict(storage=F32), dict(lanes=True), dict(waves=True)):
        with pytest.raises(NKAError, match="wide_storage"):
            nka_amd.nka_batch().init(4, 64, 3, wide_storage=F32, **kw)
    with pytest.raises(NKAError):
        nka_amd.nka_batch().init(nsys, n, mvec, wide=True, wide_storage=2)
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "a refused creation left something allocated"
    # the four older entries behave as before
    for kw, want in ((dict(wide=True), (0, 0)), (dict(wide=True, step=True), (1, 0)), (dict(wide=True, ext=True), (0, 1)),
                     (dict(wide=True, ext=True, step=True), (1, 1)), (dict(wide=True, wide_storage=F64), (0, 0))):
        b = nka_amd.nka_batch().init(2, c + 1, 3, **kw)
        assert b.storage() == F64 and b.vector_bytes() == W32.vector_bytes(2, c + 1, 3, F64) and b.is_wide()
        assert (int(b.offers_step()), int(b.offers_weights())) == want, kw
        b.delete()
    b = _narrow32(2, 513, 3)
    assert b.storage() == F32 and not b.is_wide() and b.vector_bytes() == W32.vector_bytes(2, 513, 3, F32)
    b.delete()
    # the allocation: the library's own accounting equals the formula, and the device's free memory moved by about that much
    want32, want64 = W32.vector_bytes(nsys, n, mvec, F32), W32.vector_bytes(nsys, n, mvec, F64)
    assert want32 == 2 * nsys * ((n + 31) // 32 * 32) * (4 * (mvec + 1) + 8) and want32 < 0.56 * want64
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    b = _wide32(nsys, n, mvec, True)
    grown = free0 - torch.cuda.mem_get_info()[0]
    assert want32 <= grown + (64 << 20) and grown <= want32 + (96 << 20), (grown, want32)
    for order in (nka_amd.SUMS_REFERENCE_ORDER, nka_amd.SUMS_BLOCKED):
        with pytest.raises(NKAError):
            b.set_sum_order(order)
    b.set_sum_order(nka_amd.SUMS_AUTO).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    rng = np.random.default_rng(8206)
    for s in range(1, mvec + 2):                             # never-written slots read zeros
        assert not b.w(5, s).any() and not b.v(5, s).any()
    x0, x1 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
    F = _f64(torch, x0)
    b.accel_update(F)
    st = b.state(5)
    assert st.pending and _bits_equal(b.w(5, st.first), x0[5]) and _bits_equal(b.v(5, st.first), x0[5])      # binary64-exact
    assert (S32.q(x0[5]) != x0[5]).any()
    side = torch.cuda.Stream()                               # set_stream: the next call waits for what the old stream holds
    b.set_stream(side.cuda_stream)
    with torch.cuda.stream(side):
        F = _f64(torch, x1)
        b.accel_step(F, fnorm=_f64(torch, np.zeros(nsys)))
    side.synchronize()
    w = b.w(5, st.first)
    assert _bits_equal(S32.q(w), w) and abs(np.linalg.norm(w) - 1.0) < 1e-6                                   # now a stored float row
    handle = b._h
    b.delete()
    b.delete()                                               # destroy twice through the class: the second is a no-op
    assert L.nka_hip_batch_destroy(None) == 0 and handle is not None
    b = _wide32(nsys, n, mvec)                               # destroy and re-create
    assert b.num_vec().max() == 0 and b.vector_bytes() == want32
    b.delete()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), "destroy left something allocated"


# ---- 9. one large case ---------------------------------------------------------------------------------------------------------------------

class LargeWide32(Large32):
    """tests/test_batch_store32_gpu.py's large binary32 batch beside its twin, both WIDE; the shape, the systems that run and the
    witnesses are those of tests/batch_wide_store32.py."""

    def __init__(self, torch):
        self.torch, self.sh = torch, W32.LARGE
        self.active = W32.large_active()
        self.na = len(self.active)
        self.b = self.t = self.mask = self.tmask = self.idx = None
        self.raw, self.rows, self.trows, self.host, self.misc = {}, {}, {}, {}, {}
        try:
            self._create("wide slots, binary32")
        except BaseException:
            self.close()
            raise

    def _create(self, sid):
        import time

        import nka_amd
        torch, sh = self.torch, self.sh
        assert nka_amd.batch_wide_limits()[0] == G.WIDE_CHUNK, "the shape was worked out for another chunk"
        need = W32.large_bytes()
        free, total = torch.cuda.mem_get_info()
        assert free >= need + (8 << 30), f"{sid}: {free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 8 GiB"
        self.t0 = time.perf_counter()
        self.b, self.t = _wide32(sh.nsys, sh.vlen, sh.mvec), _wide32(self.na, sh.vlen, sh.mvec)
        assert self.b.vector_bytes() == W32.vector_bytes(sh.nsys, sh.vlen, sh.mvec, W32.STORE_F32) > 2 ** 34
        self.fresh_digest = self.b.state_digest(W32.large_witnesses()[0])
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
        for k in W32.large_witnesses():
            assert self.b.state_digest(k) == self.fresh_digest, (where, "witness", k, "digest")
            for s in range(1, sh.mvec + 2):
                assert not self.b.w(k, s).any() and not self.b.v(k, s).any(), (where, "witness", k, "slot", s)
        for k in self.active:
            self.rows["F"][k].fill_(G.PAD)
        assert bool((self.raw["F"] == G.PAD).all().item()), (where, "an element of F of no running system was written")


def test_float_slots_of_a_wide_batch_beyond_2_to_the_31_elements_and_2_to_the_32_bytes(torch_cuda):
    """14 030 systems of 4609 (three chunks), mvec = 32, binary32 storage: each of the w and the v allocation holds 2.15e9 floats, 8.6 GB;
    18.3 GB with the pending buffers.  The systems on 2^30 elements = 2^32 bytes and on 2^31 elements, their neighbours, system 0 and
    the last one run -- eight --, all others are masked.  36 updates on fresh inputs fill the lists to 32 and write every slot, then
    mixed inputs and a masked restart; every running system == its system in a small binary32 wide twin after every call, the
    witnesses at the wrapped offsets are untouched."""
    L = LargeWide32(torch_cuda)
    try:
        bd = W32.large_boundaries()
        assert all(k in L.active for k in bd.values()) and L.na <= W32.MAX_ACTIVE
        _fill_the_lists(L, np.random.default_rng(9207), ("wide-slots32",))
        seqs = _sequences(L, 9207)
        for c in range(3):
            L.update(("wide-slots32", "mixed", c), [s.next() for s in seqs])
        L.restart([0, 2, 5])
        for c in range(3):
            L.update(("wide-slots32", "after the restart", c), [s.next() for s in seqs])
        L.finish(("wide-slots32",))
    finally:
        L.close()
