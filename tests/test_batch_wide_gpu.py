"""The WIDE batched accelerator (nka_hip_batch_create_wide; nka_amd/csrc/nka_batch_wide.hip): every system split into chunks
of C = NKA_HIP_BATCH_WIDE_CHUNK elements, one workgroup per chunk, four launches per update.  Shapes are given in units of
C, read from the library.

  1 one chunk            a wide batch of at most C elements is the narrow batch in SUMS_BLOCKED_ROUNDED, bit for bit
  2 several chunks       the three layers of tests/test_batch_sums_exact_gpu.py (sums within gamma(wide_k(n)) of the exact sums,
                         the oracle's scalar step on the device's own sums with ==, the elementwise statements bit for bit)
                         at 2 and 3 chunks; at 9, 10, 16 and 17, where the eight-way chain over the partials (k_wide_scalar) runs
                         one trip or two with every kind of remainder; with the longest list, mvec = 32, over 3 and 9 chunks
  3 partition and order  red[0] == ((p0 + p1) + p2) + ..., p_c from narrow batches run on the chunks: 3, 10, 17 and 257 chunks
  4 independence         the same bits at every position, under every mask of the others, at both parities of ld
  5 sitting out          nothing of a masked system is written, nor the padding between rows
  6 no stale partial     a system that saw NaN / Inf and was restarted equals a twin that never saw them
  7 graph                captured before the first update, replayed through growth, drops and a masked relax
  8 refusals, lifecycle  what a wide batch refuses leaves it usable
  9 the long shapes      the three layers of part 2 at 256 and 257 chunks (one and two trips of the staging loop of wide_norm_sum)
                         and at vlen = NKA_HIP_BATCH_WIDE_MAX_VLEN: the last chunk and the largest nchunk

A bound only proves something where the error it looks for exceeds it: every sum over several chunks that WideRun holds is first
held, from its host operands alone, to the condition that each chunk's partial is detectable (batch_wide.undetectable_chunks);
tests/test_batch_wide_cpu.py shows on the host model that a partial lost or added twice then breaks the bound.

The worst |red - exact| / (u sum|xy|) of parts 2 and 9 and the K it was held to go to batch_wide_exact_worst.json, overall and
per chunk count."""
import ctypes as C
import itertools
import json
import math
import os

import numpy as np
import pytest

import batch_seq as B
import batch_wide as BW
import exact_sums as X
import test_batch_sums_exact_gpu as T
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|xy|) seen, the K it was held to, where
WORST_AT = {}                      # K -> [the worst ratio among the sums held to that K, where]


def _worst_line():
    ratio, k, where = WORST
    return f"wide batch sums: worst |red - exact| = {ratio:.3f} u sum|xy| against K = {k} there ({where})"


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
        with open(os.path.join(out, "batch_wide_exact_worst.json"), "w") as fh:
            json.dump({"wide": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where},
                       "wide_by_k": {str(kk): {"worst_err_over_u_sum_abs": r, "where": w} for kk, (r, w) in sorted(WORST_AT.items())}},
                      fh, indent=1, sort_keys=True)


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


def _rows(torch, nsys, vlen, odd_ld, fill=0.0):
    """nsys rows of vlen elements, the smallest odd / even row stride that holds a row -> (raw, view, ld)."""
    ld = vlen + (1 - vlen % 2 if odd_ld else vlen % 2)
    raw = torch.full((nsys * ld,), fill, dtype=torch.float64, device="cuda")
    return raw, raw.view(nsys, ld)[:, :vlen], ld


def _mask(torch, nsys, ks):
    m = np.zeros(nsys, np.int32)
    m[list(ks)] = 1
    return torch.from_numpy(m).cuda()


def _same_system(a, ka, b, kb, where, slots="list"):
    """System ka of batch a and system kb of batch b: red[], the digest, num_vec and the stored vectors of the list, bit for bit."""
    assert _bits_equal(a.reductions(ka), b.reductions(kb)), (where, "red[]", a.reductions(ka), b.reductions(kb))
    assert a.state_digest(ka) == b.state_digest(kb), (where, "digest")
    assert a.num_vec()[ka] == b.num_vec()[kb], (where, "num_vec")
    order = a.state(ka).list_order()
    assert order == b.state(kb).list_order(), where
    for s in (order if slots == "list" else range(1, a.max_vec() + 2)):
        assert _bits_equal(a.w(ka, s), b.w(kb, s)), (where, "w", s)
        assert _bits_equal(a.v(ka, s), b.v(kb, s)), (where, "v", s)


# ---- 1. one chunk is the narrow batch, bit for bit -----------------------------------------------------------------------------

def _one_chunk_inputs(vlen, nsys, calls, seed):
    """Per call {system: input}: system k starts k calls late; every system repeats an input once (s == 0)."""
    rngs, prev, out = [np.random.default_rng([seed, vlen, k]) for k in range(nsys)], [None] * nsys, []
    for t in range(calls):
        step = {}
        for k in range(nsys):
            j = t - k
            if j < 0:
                continue
            x = prev[k].copy() if j == 4 + k % 3 else X.batch_planted_input(vlen, rngs[k], prev[k])
            step[k] = prev[k] = x
        out.append(step)
    return out


@pytest.mark.parametrize("which", ["1", "2", "65", "513", "C-1", "C"])
def test_one_chunk_is_the_narrow_batch_bit_for_bit(torch_cuda, CH, which):
    """Five systems with staggered starts, a masked relax, a masked restart and a repeated input over 15 updates; three flavours,
    mvec 3 and 10, both parities of ld.  The narrow twin runs SUMS_BLOCKED_ROUNDED (also up to 64 elements, where its AUTO is
    the reference order).  After every update: the rows of F, red[], the digest, num_vec and the slots of w and v that the list
    holds; after every fifth, EVERY slot."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    vlen = {"C-1": c - 1, "C": c}.get(which) or int(which)
    assert vlen <= nka_amd.BATCH_MAX_VLEN
    nsys, calls = 5, 15
    for flavor, mvec, odd_ld in itertools.product((0, 1, 2), (3, 10), (False, True)):
        wide = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, wide=True)
        twin = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        assert wide.is_wide() and not twin.is_wide()
        (_, Fw, _), (_, Fn, _) = _rows(torch, nsys, vlen, odd_ld), _rows(torch, nsys, vlen, odd_ld)
        host = np.zeros((nsys, vlen))
        for t, step in enumerate(_one_chunk_inputs(vlen, nsys, calls, 100 * mvec + flavor)):
            where = (vlen, flavor, mvec, odd_ld, "call", t)
            if t == 7:
                for b in (wide, twin):
                    b.relax(_mask(torch, nsys, [1, 3]))
            if t == 10:
                for b in (wide, twin):
                    b.restart(_mask(torch, nsys, [0, 3]))
            for k, x in step.items():
                host[k] = x
            mask = None if len(step) == nsys else _mask(torch, nsys, step)
            for b, F in ((wide, Fw), (twin, Fn)):
                F.copy_(torch.from_numpy(host))
                b.accel_update(F, mask)
            assert torch.equal(Fw, Fn) and _bits_equal(Fw.cpu().numpy(), Fn.cpu().numpy()), (where, "rows of F")
            host = Fw.cpu().numpy()
            for k in range(nsys):
                _same_system(wide, k, twin, k, where + ("system", k), slots="all" if t % 5 == 4 else "list")
        if vlen >= 65 and mvec == 3:
            assert wide.num_vec()[2] == mvec, wide.num_vec()      # a full list: the capacity drop ran


# ---- 2. several chunks: the three layers ------------------------------------------------------------------------------------------

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
    if tot > 0 and ratio >= WORST_AT.get(k, [0.0])[0]:
        WORST_AT[k] = [ratio, f"{what} {where}"]


class WideRun(T.BatchRun):
    """BatchRun on a wide batch: the sums are held to wide_k(n); layers 2 and 3 are inherited unchanged.  Every sum that is held
    is first asked, from its HOST operands alone, whether the bound can see a lost or a doubled partial of each of its chunks
    (batch_wide.undetectable_chunks): no (entry, chunk) cell may fail that."""

    def __init__(self, torch, oracle, flavor, n, mvec, nsys, odd_ld=False):
        super().__init__(torch, oracle, flavor, n, mvec, nsys, odd_ld)
        self.k = BW.wide_k(n)
        self.chunk = BW.limits()[0]
        self.held = {}                 # name of the entry -> how often it was held having been formed non-zero
        self.cells = 0                 # (entry, chunk) cells that passed the condition

    def _device(self, odd_ld):
        import nka_amd
        torch, n, nsys, ld = self.torch, self.n, self.nsys, self.ld
        self.b = nka_amd.nka_batch().init(nsys, n, self.m, flavor=self.flavor, wide=True)
        self.order, self.orders_met = nka_amd.SUMS_BLOCKED_ROUNDED, set()
        self.reference = nka_amd.SUMS_REFERENCE_ORDER
        assert self.b.flavor() == self.flavor and self.b.is_wide()
        self.raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda")
        self.F = self.raw.view(nsys, ld)[:, :n]
        align = [(self.raw.data_ptr() + 8 * k * ld) % 16 for k in range(nsys)]
        if odd_ld:
            assert ld % 2 == 1 and align == [8 * (k % 2) for k in range(nsys)], align
        else:
            assert ld % 2 == 0 and not any(align), align

    def _sum(self, what, red, x, y, where):
        if self.n > self.chunk:
            unseen = BW.undetectable_chunks(x, y, self.k, self.chunk)
            assert not unseen, (what, where, "the bound could not see these chunks' partials lost: another seed", unseen)
            self.cells += BW.nchunk(self.n, self.chunk)
        _hold(what, red, x, y, self.k, where)
        if red != 0.0:
            self.held[what] = self.held.get(what, 0) + 1


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


@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("which", ["C+1", "2C+513"])
def test_every_part_of_a_wide_update_over_several_chunks(torch_cuda, oracle, CH, which, odd_ld):
    """Six systems of different list length in one launch (the PLAN of test_batch_sums_exact_gpu: older counts 0 ... 10, a
    repeated input, a masked relax and a masked restart each), mvec = 10, default flavour."""
    c = CH[0]
    n = c + 1 if which == "C+1" else 2 * c + 513
    assert BW.wide_k(n) == 2 * (c // 512) + 9 + (BW.nchunk(n, c) - 1)
    run = _planned_run(WideRun(torch_cuda, oracle, 2, n, T.SHAPE_MVEC, len(T.PLAN), odd_ld), seed=n)
    T._assert_planned_coverage(run)


@pytest.mark.parametrize("flavor", [0, 1])
def test_every_part_of_a_wide_update_in_the_other_flavours(torch_cuda, oracle, CH, flavor):
    """... and the two other flavours at C + 1 (the chunk of one element), odd ld."""
    n = CH[0] + 1
    run = _planned_run(WideRun(torch_cuda, oracle, flavor, n, T.SHAPE_MVEC, len(T.PLAN), True), seed=n + flavor)
    T._assert_planned_coverage(run)


def _ladder_shape(which, c):
    """n, chunks: the smallest shapes at which the loops over the partials change behaviour -- the eight-way chain of
    k_wide_scalar behind partial 0 and its remainder loop, the staging loop of wide_norm_sum (256 partials a trip), the cap."""
    n, chunks = {"8C+1": (8 * c + 1, 9),          # one trip of eight, empty remainder, a last chunk of one element
                 "9C+1": (9 * c + 1, 10),         # one trip and a remainder of one
                 "15C+513": (15 * c + 513, 16),   # one trip and the longest remainder, seven
                 "16C+1": (16 * c + 1, 17),       # two trips, empty remainder
                 "256C": (256 * c, 256),          # the last single trip of the staging loop
                 "256C+1": (256 * c + 1, 257)}[which]      # its first second trip, a last chunk of one element
    assert BW.nchunk(n, c) == chunks and BW.wide_k(n) == 2 * (c // 512) + 9 + (chunks - 1), (which, c, n)
    return n, chunks


@pytest.mark.parametrize("which", ["8C+1", "9C+1", "15C+513", "16C+1"])
def test_every_part_of_a_wide_update_up_the_ladder_of_chunk_counts(torch_cuda, oracle, CH, which):
    """9, 10, 16 and 17 chunks: every live entry of red[] within gamma(wide_k(n)) of the exact sum where the eight-way unrolled
    chain of k_wide_scalar runs one trip or two, with an empty remainder, one of one and one of seven.  At 9 (odd ld) and 17
    (even ld) chunks the whole plan of six systems in the default flavour; at 10 and 16 two systems, the second one call late on
    an unaligned row, mvec = 3, five updates, flavours 0 and 1."""
    n, chunks = _ladder_shape(which, CH[0])
    if chunks in (9, 17):
        run = _planned_run(WideRun(torch_cuda, oracle, 2, n, T.SHAPE_MVEC, len(T.PLAN), odd_ld=(chunks == 9)), seed=n)
        T._assert_planned_coverage(run)
        assert run.cells > 0
    else:
        for flavor in (0, 1):
            run = _late_second_system(WideRun(torch_cuda, oracle, flavor, n, 3, 2, odd_ld=True), 5, seed=flavor)
            assert run.widest == 3


@pytest.mark.parametrize("which,flavor", [("2C+513", 0), ("8C+1", 2)])
def test_every_older_count_of_a_wide_system_up_to_the_largest_subspace(torch_cuda, oracle, CH, which, flavor):
    """The wide sibling of test_batch_sums_exact_gpu.test_every_older_count_up_to_the_largest_subspace: mvec = 32, fresh planted
    inputs for mvec + 2 updates, system 1 one call late on an unaligned row.  The older count visits 0..32 -- every group count
    of k_wide_sums, up to eight groups of four --, red[] has 66 entries of which 64 and 65 (<f,w_30>, <f,w_31>) are formed by
    the second wavefront of k_wide_scalar, and the LDS of both kernels is carved for the largest working copy.  Over three
    chunks in flavour 0; over nine in flavour 2, where those two threads run the eight-way chain."""
    c = CH[0]
    n = 2 * c + 513 if which == "2C+513" else _ladder_shape(which, c)[0]
    mvec = 32
    run = _late_second_system(WideRun(torch_cuda, oracle, flavor, n, mvec, 2, odd_ld=True), mvec + 2, seed=mvec)
    assert run.widest == mvec == 32 and run.nolder_normed == set(range(mvec + 1)), run.nolder_normed
    assert 2 + mvec + 31 == 65 and run.held.get("<f,w_30>", 0) >= 1 and run.held.get("<f,w_31>", 0) >= 1, run.held


def test_a_wide_system_that_keeps_one_vector(torch_cuda, oracle, CH):
    """mvec = 1 once at C + 1: red[] of four entries, the smallest working copy; ngroup == 0 with a normalised pair at the second
    update, and from the third on one older vector, which every update drops by capacity."""
    n = CH[0] + 1
    run = _late_second_system(WideRun(torch_cuda, oracle, 2, n, 1, 2, odd_ld=True), 6, seed=1)
    assert run.widest == 1 and run.nolder_normed == {0, 1}, (run.widest, run.nolder_normed)
    assert run.held["<w1',w_0>"] >= 1 and run.held["<f,w_0>"] >= 1, run.held
    assert any(gone == [0] for _, _, gone in run.outcomes), run.outcomes


# ---- 3. the partition and the chunk order, in bits ----------------------------------------------------------------------------------

def test_red0_is_the_chunk_order_sum_of_the_narrow_batches_on_the_chunks(torch_cuda, CH):
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    vlen = 2 * c + 513
    rng = np.random.default_rng(31)
    x0 = BW.wide_planted_input(vlen, rng)
    x1 = BW.wide_planted_input(vlen, rng, prev=x0)

    def red0(b, lo, hi):
        for x in (x0, x1):      # second update of a fresh system: a pending pair, no older vector
            F = torch.from_numpy(x[lo:hi].copy()).cuda().view(1, hi - lo)
            b.accel_update(F)
        return np.float64(b.reductions(0)[0])

    got = red0(nka_amd.nka_batch().init(1, vlen, 3, wide=True), 0, vlen)
    p = [red0(nka_amd.nka_batch().init(1, hi - lo, 3).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED), lo, hi)
         for lo, hi in ((0, c), (c, 2 * c), (2 * c, vlen))]
    want = (p[0] + p[1]) + p[2]
    assert got > 0 and _bits_equal(np.array([got]), np.array([want])), (got, want, p)


@pytest.mark.parametrize("which", ["9C+1", "16C+1", "256C+1"])
def test_red0_is_the_chunk_order_sum_of_one_narrow_batch_of_the_chunks(torch_cuda, CH, which):
    """The same at 10, 17 and 257 chunks, where the bound cannot tell the chunk order from a pairwise sum of the partials:
    red[0] of the second update of a fresh wide system is ((p0 + p1) + p2) + ..., bit for bit.  p_c is red[0] of system c of ONE
    narrow batch (SUMS_BLOCKED_ROUNDED) of nchunk systems whose row c is chunk c; the last chunk, of one element, through
    set_lengths with NaN behind it.  (That a narrow system's bits depend neither on its position nor on nsys, and that a length
    gives the bits of a batch of that length, is held in tests/test_batch_gpu.py and tests/test_batch_lengths_gpu.py.)"""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    vlen, chunks = _ladder_shape(which, c)
    rng = np.random.default_rng([31, vlen])
    x0 = BW.wide_planted_input(vlen, rng)
    x1 = BW.wide_planted_input(vlen, rng, prev=x0)
    last = vlen - (chunks - 1) * c
    wide = nka_amd.nka_batch().init(1, vlen, 3, wide=True)
    narrow = nka_amd.nka_batch().init(chunks, c, 3).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    narrow.set_lengths(np.array([c] * (chunks - 1) + [last], np.int64))
    for x in (x0, x1):          # second update of a fresh system: a pending pair, no older vector
        wide.accel_update(torch.from_numpy(x.copy()).cuda().view(1, vlen))
        rows = np.full(chunks * c, np.nan)
        rows[:vlen] = x
        narrow.accel_update(torch.from_numpy(rows).cuda().view(chunks, c))
    got = np.float64(wide.reductions(0)[0])
    p = [np.float64(narrow.reductions(k)[0]) for k in range(chunks)]
    want = p[0]
    for q in p[1:]:
        want = want + q
    assert got > 0 and all(q > 0 for q in p), (got, p)
    assert _bits_equal(np.array([got]), np.array([want])), (which, got, want)
    pairwise = np.float64(np.sum(np.array(p)))      # (numpy's pairwise sum: what the comparison would accept if the order were free)
    print(f"  {which}: red[0] = {got!r}; the pairwise sum of the partials differs: {bool(pairwise != want)}")


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------

def _run_at(torch, nka_amd, vlen, mvec, inputs, nsys, pos, active_others, odd_ld):
    """System `pos` of a wide batch of nsys runs `inputs`; the systems of `active_others` run data of their own, the rest sit out."""
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    rng = np.random.default_rng(5 + 11 * nsys + pos)
    _, F, _ = _rows(torch, nsys, vlen, odd_ld)
    active = sorted(set(active_others) | {pos})
    mask = None if len(active) == nsys else _mask(torch, nsys, active)
    outs = []
    for x in inputs:
        Xh = rng.standard_normal((nsys, vlen))
        Xh[pos] = x
        F.copy_(torch.from_numpy(Xh))
        b.accel_update(F, mask)
        outs.append(F[pos].cpu().numpy())
    vecs = [(b.w(pos, s), b.v(pos, s)) for s in b.state(pos).list_order()]
    return outs, b.state_digest(pos), b.reductions(pos), vecs


@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
def test_results_do_not_depend_on_the_batch_around_a_wide_system(torch_cuda, CH, odd_ld):
    """vlen = C + 513; nsys 1 and 7, every position, every mask of the other six."""
    import nka_amd
    vlen, mvec = CH[0] + 513, 3
    seq = B.Sequence(vlen, 78)
    inputs = [seq.next() for _ in range(mvec + 3)]
    base = _run_at(torch_cuda, nka_amd, vlen, mvec, inputs, 1, 0, [], False)
    runs = [(1, 0, ())] + [(7, pos, tuple(o for o, bit in zip([q for q in range(7) if q != pos], bits) if bit))
                           for pos in range(7) for bits in itertools.product((0, 1), repeat=6)]
    assert len(runs) == 1 + 7 * 64
    for nsys, pos, others in runs:
        outs, dig, red, vecs = _run_at(torch_cuda, nka_amd, vlen, mvec, inputs, nsys, pos, others, odd_ld)
        where = (nsys, pos, others, odd_ld)
        assert dig == base[1] and _bits_equal(red, base[2]), where
        assert all(_bits_equal(a, c) for a, c in zip(outs, base[0])), where
        assert len(vecs) == len(base[3]) and all(_bits_equal(w, w0) and _bits_equal(v, v0) for (w, v), (w0, v0) in zip(vecs, base[3])), where


# ---- 5. sitting out ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavor", [0, 2])
def test_a_masked_system_and_the_padding_are_never_written(torch_cuda, CH, flavor):
    """Three systems of C + 513 elements with three elements of padding behind each row; system 1 holds a pending pair and two
    older vectors when it starts to sit out: across the four kernels of the following updates its row, red[], digest and EVERY
    slot of w and v stay as they were, and so does the padding."""
    import nka_amd
    torch = torch_cuda
    vlen, mvec, nsys, pad = CH[0] + 513, 4, 3, 3
    ld = vlen + pad
    raw = torch.full((nsys * ld,), 7.25, dtype=torch.float64, device="cuda")
    F = raw.view(nsys, ld)[:, :vlen]
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, wide=True)
    rng = np.random.default_rng(55)
    for _ in range(3):
        F.copy_(torch.from_numpy(rng.standard_normal((nsys, vlen))))
        b.accel_update(F)
    keep_row = F[1].cpu().numpy()
    keep = (b.reductions(1), b.state_digest(1), [(b.w(1, s), b.v(1, s)) for s in range(1, mvec + 2)])
    assert b.state(1).pending and b.num_vec()[1] == 2
    mask = _mask(torch, nsys, [0, 2])
    for t in range(mvec + 2):
        Xh = rng.standard_normal((nsys, vlen))
        Xh[1] = keep_row
        F.copy_(torch.from_numpy(Xh))
        b.accel_update(F, mask)
        assert _bits_equal(F[1].cpu().numpy(), keep_row), t
        assert _bits_equal(b.reductions(1), keep[0]) and b.state_digest(1) == keep[1], t
        for s in range(1, mvec + 2):
            assert _bits_equal(b.w(1, s), keep[2][s - 1][0]) and _bits_equal(b.v(1, s), keep[2][s - 1][1]), (t, s)
        assert bool((raw.view(nsys, ld)[:, vlen:] == 7.25).all()), (t, "the padding between two rows was written")
    assert b.num_vec()[0] == mvec and b.num_vec()[2] == mvec


# ---- 6. no stale partial ---------------------------------------------------------------------------------------------------------------------

def test_a_restarted_system_carries_nothing_of_the_nan_and_inf_it_saw(torch_cuda, CH):
    """System 1 of three is fed a NaN, then an Inf, and is then restarted under a mask (its twin in a second batch is restarted
    too, having seen finite inputs): from there on it is bit-equal to the twin -- rows, red[], decisions, stored vectors --
    although every partial of its sums held NaN.  Systems 0 and 2 never differ from their twins."""
    import nka_amd
    torch = torch_cuda
    vlen, mvec, nsys, ill = 2 * CH[0] + 513, 4, 3, 1
    a = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    twin = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    (_, Fa, _), (_, Ft, _) = _rows(torch, nsys, vlen, True), _rows(torch, nsys, vlen, True)
    rng = np.random.default_rng(66)
    for t in range(12):
        Xh = rng.standard_normal((nsys, vlen))
        Xa = Xh.copy()
        if t == 3:
            Xa[ill, vlen - 1] = np.nan
        if t == 4:
            Xa[ill, CH[0]] = np.inf
        if t == 6:
            for b in (a, twin):
                b.restart(_mask(torch, nsys, [ill]))
        Fa.copy_(torch.from_numpy(Xa))
        Ft.copy_(torch.from_numpy(Xh))
        a.accel_update(Fa)
        twin.accel_update(Ft)
        ra, rt = Fa.cpu().numpy(), Ft.cpu().numpy()
        if 3 <= t < 6:
            assert not np.isfinite(ra[ill]).all() and not np.isfinite(a.reductions(ill)).all(), t
        for k in range(nsys):
            if k == ill and t < 6:
                continue
            where = ("call", t, "system", k)
            assert _bits_equal(ra[k], rt[k]), where
            assert _bits_equal(a.reductions(k), twin.reductions(k)), where
            sa, st = a.state(k), twin.state(k)
            assert sa.list_order() == st.list_order() and (sa.pending, sa.subspace, sa.free) == (st.pending, st.subspace, st.free), where
            for s in sa.list_order():
                assert _bits_equal(a.w(k, s), twin.w(k, s)) and _bits_equal(a.v(k, s), twin.v(k, s)), where + (s,)
            if k != ill:
                assert a.state_digest(k) == twin.state_digest(k), where
    assert a.num_vec()[ill] == mvec


# ---- 7. graph -----------------------------------------------------------------------------------------------------------------------------------

def test_wide_update_is_capturable_before_the_first_update(torch_cuda, CH):
    """Eight systems of C + 1 elements, captured BEFORE the first update, replayed 30 times: the lists grow, drop by dependence
    and by capacity (batch_seq.Sequence), systems sit out by mask, and a masked relax runs between two replays."""
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = 8, CH[0] + 1, 5
    seqs = [B.Sequence(vlen, 400 + k) for k in range(nsys)]
    rng = np.random.default_rng(10)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.accel_update(static, mask)
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    full = differed = False
    for t in range(30):
        Xh = np.stack([s.next() for s in seqs])
        m = (rng.random(nsys) < 0.8).astype(np.int32)
        if t in (9, 20):
            rm = _mask(torch, nsys, [1, 4, 6])
            with torch.cuda.stream(side):
                b.relax(rm)
            eager.relax(rm)
        static.copy_(torch.from_numpy(Xh))
        mask.copy_(torch.from_numpy(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = torch.from_numpy(Xh.copy()).cuda()
        eager.accel_update(F, torch.from_numpy(m).cuda())
        assert torch.equal(F, static), t
        assert np.array_equal(b.num_vec(), eager.num_vec()), t
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], t
        full = full or bool((b.num_vec() == mvec).any())
        differed = differed or len(set(b.num_vec().tolist())) > 1
    assert full and differed      # a full list (capacity drops from there on), and lists of different length in one replay


# ---- 8. refusals and lifecycle -------------------------------------------------------------------------------------------------------------------

def test_what_a_wide_batch_refuses_leaves_it_usable(torch_cuda, CH):
    import nka_amd
    from nka_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    c, cap = CH
    EINVAL = -1
    h = C.c_void_p()
    for nsys, vlen, mvec in [(2, cap + 1, 3), (65536, 8, 3), (2, 8, 33), (0, 8, 3), (2, 0, 3)]:
        assert L.nka_hip_batch_create_wide(C.byref(h), nsys, vlen, mvec, 0.01, -1, 0, None) == EINVAL and h.value is None
        with pytest.raises(nka_amd.NKAError):
            nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    nsys, vlen, mvec = 3, c + 33, 3
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    twin = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    narrow = nka_amd.nka_batch().init(nsys, 33, mvec)
    assert b.is_wide() and not narrow.is_wide() and not b.dot_weighted()
    F = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    Xs = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(2)
    inputs = [rng.standard_normal((nsys, vlen)) for _ in range(4)]
    F.copy_(torch.from_numpy(inputs[0]))
    b.accel_update(F)
    with pytest.raises(nka_amd.NKAError):
        b.accel_step(F, Xs)
    with pytest.raises(nka_amd.NKAError):
        b.set_dot_weights(torch.ones(vlen, dtype=torch.float64, device="cuda"))
    with pytest.raises(nka_amd.NKAError):
        b.set_dot_weights(np.ones(vlen))
    for order in (nka_amd.SUMS_REFERENCE_ORDER, nka_amd.SUMS_BLOCKED, 17):
        with pytest.raises(nka_amd.NKAError):
            b.set_sum_order(order)
    b.set_sum_order(nka_amd.SUMS_AUTO).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    assert not b.dot_weighted()
    # a too-short allocation of F is refused before any launch (the library's own allocator: a buffer of exactly known size)
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    assert L.nka_hip_vec_alloc(ws, (nsys - 1) * vlen + vlen - 1, C.byref(short)) == 0
    torch.cuda.synchronize()
    assert L.nka_hip_batch_accel_update(b._handle(), short, vlen, None) == EINVAL
    assert L.nka_hip_vec_free(ws, short) == 0 and L.nka_hip_vec_workspace_destroy(ws) == 0
    assert L.nka_hip_batch_accel_update(b._handle(), C.c_void_p(F.data_ptr()), vlen - 1, None) == EINVAL
    # ... and the next updates are those of a batch that was never refused anything
    Ft = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    Ft.copy_(torch.from_numpy(inputs[0]))
    twin.accel_update(Ft)
    for x in inputs[1:]:
        F.copy_(torch.from_numpy(x))
        Ft.copy_(torch.from_numpy(x))
        b.accel_update(F)
        twin.accel_update(Ft)
        assert torch.equal(F, Ft)
    assert [b.state_digest(k) for k in range(nsys)] == [twin.state_digest(k) for k in range(nsys)]
    assert np.array_equal(b.num_vec(), np.full(nsys, 3, np.int32))
    # destroy, then create
    b.delete()
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    F.copy_(torch.from_numpy(inputs[0]))
    b.accel_update(F)
    assert b.is_wide() and not b.num_vec().any() and b.state(0).pending


# ---- 9. one long shape ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["256C", "256C+1"])
def test_every_part_of_a_wide_update_on_both_sides_of_one_staging_trip(torch_cuda, oracle, CH, which):
    """256 chunks, the last length at which the 256 threads of wide_norm_sum stage the partials of <d,d> in one trip, and 257,
    the first at which a thread stages a second one (a last chunk of one element): the sum that becomes s, formed by every
    workgroup of k_wide_sums and by k_wide_scalar, and every other live entry within gamma(wide_k(n)) of the exact sums.  Two
    systems, the second one call late on an unaligned row where the length is odd, mvec = 3, four updates."""
    n, chunks = _ladder_shape(which, CH[0])
    assert n <= CH[1] and (chunks > X.BATCH_THREADS) == (which == "256C+1")
    run = _late_second_system(WideRun(torch_cuda, oracle, 2, n, 3, 2, odd_ld=bool(n % 2)), 4, seed=9)
    assert run.widest == 2 and run.held["<d,d>"] == 5


def test_the_longest_system_once(torch_cuda, oracle, CH):
    """vlen = NKA_HIP_BATCH_WIDE_MAX_VLEN, two systems (the second on a row that starts one call late), mvec = 3, four updates:
    the last chunk and the largest nchunk; every live entry of red[] within gamma(wide_k(cap)) of the exact sum (K = 528 with
    the chunk of 2048), the elementwise statements bit for bit from the device's s and c."""
    c, cap = CH
    run = WideRun(torch_cuda, oracle, 2, cap, 3, 2, odd_ld=False)
    assert BW.nchunk(cap, c) == cap // c <= 1024 and run.k == 2 * (c // 512) + 9 + (cap // c - 1)
    _late_second_system(run, 4, seed=9)
    assert run.widest == 2 and run.lengths_differed and run.held["<d,d>"] == 5
    assert all(np.isfinite(run.b.reductions(k)).all() for k in range(2))


# ---- the record (keep this test last) ------------------------------------------------------------------------------------------------------------------
def test_worst_ratio_of_the_wide_sums_is_printed_and_inside_its_bound(capsys):
    ratio, k, where = WORST
    if not where:
        return
    with capsys.disabled():
        print("\n" + _worst_line())
    assert ratio <= (k + 1) / (1.0 - (k + 1) * X.U), (ratio, k, where)
