"""The wave batch with per-system lengths and diagonal dot weights (include/nka_hip_batch.h, WAVES EXT;
nka_amd.nka_batch().init(..., waves=True, ext=True); nka_amd/csrc/nka_batch_waves.hip).
  1 lengths: every system == its own plain wave twin of vlen = len, after every call, tails untouched
  2 lengths changed between calls, cleared, and new values between the replays of a graph captured before the first update
  3 weights: unit weights, powers of four, the three layers against exact sums, a zero-weight tail, the weighted fnorm and the stop
    rule, capture, refusals                                   4 weights and lengths together
  5 independence of nsys, position, neighbours, ld / ldw parity      6 a whole ragged weighted solve, captured
  7 offers, kinds, coexistence                                       8 weight buffer, weight rows and F beyond 2^32 bytes
Twins of the old entry (init(..., waves=True)) run the kernel of nka_batch_waves.hip, which this change does not touch."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import batch_lengths as BL
import batch_seq as B
import batch_step as S
import batch_waves as BWV
import batch_waves_ext as E
import exact_sums as X
import test_batch_sums_exact_gpu as T
import test_batch_waves_gpu as G
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
PLANTED = -7.0
WORST = [0.0, 0, ""]               # worst |red - exact| / (u sum|fl(w x) y|) seen, the K it was held to, where


def _worst_line():
    ratio, k, where = WORST
    return f"wave batch sums (weighted): worst |red - exact| = {ratio:.3f} u sum|fl(w x) y| against K = {k} there ({where})"


@pytest.fixture(scope="module", autouse=True)
def _record_worst():
    """At the end of the module: the worst ratio of the weighted wave sums and the K it was held to ->
    batch_waves_ext_exact_worst.json, beside batch_waves_exact_worst.json."""
    yield
    import parity_util as P
    ratio, k, where = WORST
    if not where:
        return
    print(_worst_line())
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_waves_ext_exact_worst.json"), "w") as fh:
            json.dump({"waves_ext": {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}}, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _ld(n, odd):
    return n + (1 - n % 2 if odd else n % 2)      # the smallest odd / even row stride that holds a row


def _ext(nsys, vlen, mvec, flavor=2):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, waves=True, ext=True)
    assert b.kind() == nka_amd.KIND_WAVES == 3 and not b.is_wide() and b.flavor() == flavor
    assert b.offers_lengths() and b.offers_weights() and b.offers_step()
    return b


def _strided(torch, host, ld, pad=BWV.PAD):
    """nsys rows, ld apart, inside one allocation padded with `pad`: (the whole buffer, the view a batch takes)."""
    nsys, n = host.shape
    full = np.full((nsys, ld), pad)
    full[:, :n] = host
    raw = torch.from_numpy(full.ravel().copy()).cuda()
    return raw, raw.view(nsys, ld)[:, :n]


def _same_system(a, ka, b, kb, where):
    """red[], the state, num_vec and the digest of system ka of a against system kb of b, bit for bit."""
    assert _bits_equal(a.reductions(ka), b.reductions(kb)), (where, "red[]", a.reductions(ka), b.reductions(kb))
    sa, sb = a.state(ka), b.state(kb)
    assert sa.list_order() == sb.list_order() and sa.free_order() == sb.free_order(), (where, "list")
    assert (sa.subspace, sa.pending, sa.first, sa.last, sa.free) == (sb.subspace, sb.pending, sb.first, sb.last, sb.free), (where, "state")
    assert _bits_equal(sa.h, sb.h) and _bits_equal(sa.c, sb.c), (where, "h, c")
    assert a.num_vec()[ka] == b.num_vec()[kb], (where, "num_vec")
    assert a.state_digest(ka) == b.state_digest(kb), (where, "digest")


# ---- the twins ----------------------------------------------------------------------------------------------------------------------

class Twins:
    """One ext batch of len(lens) systems of vlen elements with lengths `lens` and weight rows `weights` (None: none) beside one
    twin per system: a batch of ONE system of vlen = its length -- of the old wave entry where there are no weights, an ext batch carrying the same weights (and no lengths) where there are.  Rows of F and X lie
    ld / ldx apart with PAD between them and NaNs of distinct payloads from the system's length on.  Every call runs both sides on
    the same inputs and compares, with ==, everything the contract names; the tails of F, X and of every slot byte for byte."""

    def __init__(self, torch, lens, vlen, mvec, flavor, odd_ld=False, odd_ldx=False, weights=None, odd_ldw=False):
        self.torch, self.vlen, self.mvec, self.flavor = torch, vlen, mvec, flavor
        self.lens = list(lens)
        self.nsys = nsys = len(self.lens)
        self.b = _ext(nsys, vlen, mvec, flavor)
        if weights is None:
            self.twins = [G._waves(1, L, mvec, flavor) for L in self.lens]
            for t in self.twins:
                assert not t.offers_lengths() and not t.offers_weights()
        else:
            assert weights.shape == (nsys, vlen)
            self.twins = [_ext(1, L, mvec, flavor).set_dot_weights(weights[k, :L].copy()) for k, L in enumerate(self.lens)]
            self.wraw, wrows = _strided(torch, weights, _ld(vlen, odd_ldw), pad=np.nan)      # (NaN between two rows: never read)
            self.b.set_dot_weights(wrows)
            assert self.b.dot_weighted() and all(t.dot_weighted() for t in self.twins)
        self.b.set_lengths(np.array(self.lens, np.int32))
        assert self.b.has_lengths() and self.b.lengths().tolist() == self.lens
        self.ld = {"F": _ld(vlen, odd_ld), "X": _ld(vlen, odd_ldx)}
        self.host = {}
        for salt, name in ((1, "F"), (2, "X")):
            self.host[name] = np.full((nsys, self.ld[name]), BWV.PAD)
            self.host[name][:, :vlen] = BL.nan_paint(nsys, vlen, salt)
        self.tw = {name: [torch.zeros(1, L, dtype=torch.float64, device="cuda") for L in self.lens] for name in ("F", "X")}
        self.zero = np.zeros(vlen)
        self.alive = np.ones(nsys, bool)                     # the mask the steps keep, as the host predicts it
        self.mask = _i32(torch, np.ones(nsys))
        self.tmask = [_i32(torch, [1]) for _ in range(nsys)]
        self.fnorm = _f64(torch, np.full(nsys, PLANTED))
        self.tfnorm = [_f64(torch, [PLANTED]) for _ in range(nsys)]
        self.fn_host = np.full(nsys, PLANTED)
        self.retired_at = np.full(nsys, -1)
        self.calls = 0

    def delete(self):
        for a in [self.b] + self.twins:
            a.delete()

    def put(self, name, xs):
        """xs: {system: its first lens[k] elements}."""
        for k, x in xs.items():
            self.host[name][k, :self.lens[k]] = x
            self.tw[name][k].copy_(self.torch.from_numpy(np.asarray(x, np.float64).reshape(1, -1)))

    def _upload(self, name):
        raw = self.torch.from_numpy(self.host[name].ravel().copy()).cuda()
        return raw, raw.view(self.nsys, self.ld[name])[:, :self.vlen]

    def list_op(self, op, ks):
        m = np.zeros(self.nsys, np.int32)
        m[list(ks)] = 1
        getattr(self.b, op)(_i32(self.torch, m))
        for k in ks:
            getattr(self.twins[k], op)()

    def call(self, kind, inputs, tol=None, where=()):
        """kind: "update" | "step" (x, mask, fnorm) | "step-tol" (and tol: nsys thresholds).  inputs: {system: f} -- the systems
        that take part; a system that has retired takes part no more."""
        torch, nsys = self.torch, self.nsys
        where = where + (kind, "call", self.calls)
        part = np.zeros(nsys, bool)
        part[list(inputs)] = True
        self.put("F", inputs)
        rawf, F = self._upload("F")
        want = {n: self.host[n].copy() for n in ("F", "X")}
        run = part & self.alive
        if kind == "update":
            self.b.accel_update(F, _i32(torch, run))
            for k in np.flatnonzero(run):
                self.twins[k].accel_update(self.tw["F"][k])
            names = ("F",)
        else:
            # the mask: alive systems that take part; the others are masked for this call and put back afterwards
            self.mask.copy_(_i32(torch, run))
            rawx, Xd = self._upload("X")
            told = None if tol is None else _f64(torch, tol)
            self.b.accel_step(F, Xd, self.mask, told, self.fnorm)
            got_mask, fn = self.mask.cpu().numpy(), self.fnorm.cpu().numpy()
            stop = np.zeros(nsys, bool)
            for k in np.flatnonzero(run):
                self.tmask[k].fill_(1)
                self.twins[k].accel_step(self.tw["F"][k], self.tw["X"][k], self.tmask[k], None if tol is None else _f64(torch, [tol[k]]),
                                         self.tfnorm[k])
                assert _bits_equal(fn[k:k + 1], self.tfnorm[k].cpu().numpy()), (where, k, "fnorm", fn[k], self.tfnorm[k].item())
                stop[k] = int(self.tmask[k].item()) == 0
            assert np.array_equal(got_mask, (run & ~stop).astype(np.int32)), (where, "the mask", got_mask, run, stop)
            assert _bits_equal(fn[~run], self.fn_host[~run]), (where, "fnorm of a system inactive on entry")
            self.fn_host = fn
            self.retired_at[stop] = self.calls
            self.alive &= ~stop
            run = run & ~stop
            names = ("F", "X")
        for name in names:
            raw = rawf if name == "F" else rawx
            for k in np.flatnonzero(run):
                want[name][k, :self.lens[k]] = self.tw[name][k].cpu().numpy()[0]
            got = raw.cpu().numpy().reshape(nsys, self.ld[name])
            if not BL.same_bytes(got, want[name]):
                bad = np.argwhere(got.view(np.uint64) != want[name].view(np.uint64))[0]
                k, i = int(bad[0]), int(bad[1])
                what = "the padding between two rows" if i >= self.vlen else "the tail" if i >= self.lens[k] else "an element"
                raise AssertionError((where, name, "system", k, "length", self.lens[k], "index", i, what, got[k, i], want[name][k, i]))
            self.host[name] = got
        for k in range(nsys):
            _same_system(self.b, k, self.twins[k], 0, where + ("system", k, "length", self.lens[k]))
        self.slot_tails(where)
        self.calls += 1

    def slot_tails(self, where):
        """From the system's length on every slot still holds the zeros of its creation, byte for byte."""
        for k, L in enumerate(self.lens):
            for s in range(1, self.mvec + 2):
                assert self.b.w(k, s)[L:].tobytes() == self.zero[L:].tobytes(), (where, "w: slot tail", k, s)
                assert self.b.v(k, s)[L:].tobytes() == self.zero[L:].tobytes(), (where, "v: slot tail", k, s)

    def slots(self, where):
        """[0, L) of EVERY slot against the twin."""
        for k, L in enumerate(self.lens):
            for s in range(1, self.mvec + 2):
                assert BL.same_bytes(self.b.w(k, s)[:L], self.twins[k].w(0, s)), (where, "w", k, s)
                assert BL.same_bytes(self.b.v(k, s)[:L], self.twins[k].v(0, s)), (where, "v", k, s)


def _run_plan(r, seed, where):
    """batch_waves_ext.PLAN: staggered starts, a repeated input (s == 0), a masked relax, a masked restart, steps with x and fnorm,
    and thresholds that retire the systems of RETIRE mid-sequence."""
    rngs = [np.random.default_rng([seed, k]) for k in range(r.nsys)]
    prev = [None] * r.nsys
    r.put("X", {k: rngs[k].standard_normal(r.lens[k]) for k in range(r.nsys)})
    tol = np.zeros(r.nsys)
    tol[list(E.RETIRE)] = np.inf
    first_tol = None
    for t, (kind, op) in enumerate(E.PLAN):
        if op is not None:
            r.list_op(op[0], [k for k in op[1] if k < r.nsys])
        inputs = {}
        for k in range(r.nsys):
            if t >= E.delay(k) and r.alive[k]:
                inputs[k] = prev[k].copy() if kind == "repeat" and prev[k] is not None else BWV.planted_input(r.lens[k], rngs[k], prev[k])
                prev[k] = inputs[k]
        if kind == "step-tol" and first_tol is None:
            first_tol = t
        r.call("update" if kind == "repeat" else kind, inputs, tol=tol if kind == "step-tol" else None, where=where)
    assert sorted(np.flatnonzero(r.retired_at >= 0).tolist()) == [k for k in E.RETIRE if k < r.nsys], r.retired_at
    assert (r.retired_at[[k for k in E.RETIRE if k < r.nsys]] == first_tol).all() and 0 < first_tol < E.CALLS - 1
    r.slots(where)
    return r


# ---- 1. lengths against twins -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odd", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("mvec", E.MVECS)
def test_a_length_carries_the_bits_of_a_wave_batch_of_that_length(torch_cuda, mvec, flavor, odd):
    """Nine systems of nine lengths in one ext batch of 385 (three tiles and a pair; the last workgroup has one absent wavefront)
    against nine batches of the OLD wave entry, one system each, over the ten calls of batch_waves_ext.PLAN."""
    r = _run_plan(Twins(torch_cuda, E.LENS, E.VLEN, mvec, flavor, odd_ld=odd, odd_ldx=not odd if mvec == 3 else odd),
                  seed=100 * mvec + flavor, where=("lengths", mvec, flavor, odd))
    assert (r.b.num_vec()[[k for k in range(r.nsys) if k not in E.RETIRE and r.lens[k] > mvec]] >= 1).all()
    r.delete()


def test_a_length_at_the_largest_subspace(torch_cuda):
    r = _run_plan(Twins(torch_cuda, E.LENS, E.VLEN, 32, 2, odd_ld=True), seed=3200, where=("lengths", 32))
    r.delete()


# ---- 2. lengths changed between calls, cleared, and under a graph -------------------------------------------------------------------

def test_lengths_change_between_calls_and_clear(torch_cuda):
    """Three sets of lengths on one live batch (a restart for every system between them, as the header asks), then NULL: every
    system is vlen long again and equals a plain wave twin of vlen."""
    torch = torch_cuda
    vlen, mvec, nsys = 257, 3, 6
    sets = [(257, 1, 129, 128, 3, 200), (2, 257, 127, 255, 256, 64), None]
    b = _ext(nsys, vlen, mvec)
    rng = np.random.default_rng(21)
    for lens in sets:
        full = [vlen] * nsys if lens is None else list(lens)
        b.set_lengths(None if lens is None else np.array(lens, np.int32))
        assert b.has_lengths() == (lens is not None) and b.lengths().tolist() == full
        b.restart()
        twins = [G._waves(1, L, mvec) for L in full]
        for t in range(mvec + 3):
            host = BL.nan_paint(nsys, vlen, 3)
            xs = [rng.standard_normal(L) for L in full]
            for k, L in enumerate(full):
                host[k, :L] = xs[k]
            F = _f64(torch, host)
            b.accel_update(F)
            got = F.cpu().numpy()
            for k, L in enumerate(full):
                Ft = _f64(torch, xs[k].reshape(1, -1))
                twins[k].accel_update(Ft)
                where = (lens, t, k)
                assert BL.same_bytes(got[k, :L], Ft.cpu().numpy()[0]), where
                assert BL.same_bytes(got[k, L:], host[k, L:]), (where, "the tail was written")
                assert _bits_equal(b.reductions(k), twins[k].reductions(0)), where
                assert b.state(k).list_order() == twins[k].state(0).list_order(), where
                for s in b.state(k).list_order():
                    assert BL.same_bytes(b.w(k, s)[:L], twins[k].w(0, s)) and BL.same_bytes(b.v(k, s)[:L], twins[k].v(0, s)), (where, s)
        for t in twins:
            t.delete()
    b.delete()


def test_lengths_under_a_graph_captured_before_the_first_update(torch_cuda):
    """The captured update keeps that it had lengths and reads their VALUES at replay: new lengths between replays (and a restart,
    outside the graph) reach the next replay.  The eager side: plain wave twins of vlen = len."""
    torch = torch_cuda
    vlen, mvec, nsys = 257, 4, 7
    sets = [(257, 1, 129, 128, 3, 200, 255), (2, 257, 127, 255, 256, 64, 1)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _ext(nsys, vlen, mvec).set_lengths(np.array(sets[0], np.int32))
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        b.accel_update(static)
        rc = b._L.nka_hip_batch_set_lengths_host(b._handle(), np.array(sets[1], np.int32).ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == ESTATE and b.lengths().tolist() == list(sets[0])
    rng = np.random.default_rng(22)
    for lens in sets:
        with torch.cuda.stream(side):
            b.set_lengths(np.array(lens, np.int32))
            b.restart()
        twins = [G._waves(1, L, mvec) for L in lens]
        for t in range(mvec + 2):
            host = BL.nan_paint(nsys, vlen, 4)
            xs = [rng.standard_normal(L) for L in lens]
            for k, L in enumerate(lens):
                host[k, :L] = xs[k]
            static.copy_(_f64(torch, host))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = static.cpu().numpy()
            for k, L in enumerate(lens):
                Ft = _f64(torch, xs[k].reshape(1, -1))
                twins[k].accel_update(Ft)
                assert BL.same_bytes(got[k, :L], Ft.cpu().numpy()[0]) and BL.same_bytes(got[k, L:], host[k, L:]), (lens, t, k)
                # (the digest covers h and c, which a restart leaves as they are: a fresh twin's differs after the second set)
                assert _bits_equal(b.reductions(k), twins[k].reductions(0)), (lens, t, k)
                sa, sb = b.state(k), twins[k].state(0)
                assert (sa.list_order(), sa.free_order(), sa.subspace, sa.pending) == (sb.list_order(), sb.free_order(), sb.subspace, sb.pending)
                assert lens is not sets[0] or b.state_digest(k) == twins[k].state_digest(0), (lens, t, k)
        for t in twins:
            t.delete()
    b.delete()


# ---- 3. weights ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", E.UNIT_LENGTHS)
def test_unit_weights_give_the_bits_of_the_plain_wave_batch(torch_cuda, n):
    """Unit weights in the shared form and one row per system (rows ld apart), and a batch whose general weights were cleared
    again, beside a batch of the old wave entry: rows of f, red[] and digests after every update; three flavours, both ld."""
    torch = torch_cuda
    mvec, nsys = 5, 5
    for flavor in (0, 1, 2):
        for odd in (False, True):
            ld = _ld(n, odd)
            _, ones = _strided(torch, np.ones((nsys, n)), ld, pad=np.nan)
            general = _f64(torch, E.system_weights(n, nsys))
            batches = {"plain": G._waves(nsys, n, mvec, flavor), "shared": _ext(nsys, n, mvec, flavor).set_dot_weights(ones[0]),
                       "rows": _ext(nsys, n, mvec, flavor).set_dot_weights(ones),
                       "cleared": _ext(nsys, n, mvec, flavor).set_dot_weights(general).set_dot_weights(None)}
            assert [b.dot_weighted() for b in batches.values()] == [False, True, True, False]
            seqs = [B.Sequence(n, 1000 * n + 10 * k + flavor) for k in range(nsys)]
            host = np.zeros((nsys, n))
            for t in range(mvec + 4):
                ks = [k for k in range(nsys) if t >= k]
                for k in ks:
                    host[k] = seqs[k].next()
                mask = np.zeros(nsys, np.int32)
                mask[ks] = 1
                out = {}
                for name, b in batches.items():
                    raw, F = _strided(torch, host, ld)
                    b.accel_update(F, _i32(torch, mask))
                    out[name] = raw.cpu().numpy()
                for name in ("shared", "rows", "cleared"):
                    where = (n, flavor, ld, t, name)
                    assert BL.same_bytes(out[name], out["plain"]), where
                    for k in range(nsys):
                        _same_system(batches[name], k, batches["plain"], k, where + (k,))
                host = out["plain"].reshape(nsys, ld)[:, :n].copy()
            for b in batches.values():
                b.delete()


@pytest.mark.parametrize("mvec", [1, 5, 32])
@pytest.mark.parametrize("n", [7, 129, 899])
def test_powers_of_four_are_an_exact_rescaling_per_system(torch_cuda, n, mvec):
    """w[sys, i] = 4^k: fl(w a) b = (2^k a)(2^k b) exactly, so the weighted batch on F equals 2^-k o (a plain wave batch on
    2^k o F), bit for bit: rows, red[], h, c, the lists -- the same decisions --, stored w and v."""
    torch = torch_cuda
    nsys = 5
    for flavor in (0, 1, 2):
        rng = np.random.default_rng([4, n, mvec, flavor])
        k4 = rng.integers(-6, 7, (nsys, n))
        scale = np.ldexp(1.0, k4)
        bw = _ext(nsys, n, mvec, flavor).set_dot_weights(_f64(torch, np.ldexp(1.0, 2 * k4)))
        bp = G._waves(nsys, n, mvec, flavor)
        seqs = [B.Sequence(n, 4000 * n + 100 * mvec + 10 * k + flavor) for k in range(nsys)]
        for t in range(min(mvec, 8) + 4):
            Xh = np.stack([s.next() for s in seqs])
            Fw, Fp = _f64(torch, Xh), _f64(torch, scale * Xh)
            bw.accel_update(Fw)
            bp.accel_update(Fp)
            where = (n, mvec, flavor, t)
            assert _bits_equal(scale * Fw.cpu().numpy(), Fp.cpu().numpy()), where
            for k in range(nsys):
                _same_system(bw, k, bp, k, where + (k,))
                for slot in bw.state(k).list_order():
                    assert _bits_equal(scale[k] * bw.w(k, slot), bp.w(k, slot)), (where, k, slot, "w")
                    assert _bits_equal(scale[k] * bw.v(k, slot), bp.v(k, slot)), (where, k, slot, "v")
        assert bw.num_vec().max() >= 1
        bw.delete()
        bp.delete()


class WeightedWavesRun(G.WavesRun):
    """WavesRun on an ext batch with per-system general weights (batch_waves_ext.system_weights: nonzero and at least a factor 2
    from 1 at every sentinel of the wave sum), rows as far apart as those of f.  Layer 1 holds every sum with its FIRST operand x
    replaced by fl(w_sys o x), within gamma(waves_k(n)) * sum|fl(w x) y| of the exact sum -- K unchanged, the product's first
    operand is the already rounded fl(w x); layers 2 and 3 are inherited unchanged."""

    def _device(self, odd_ld):
        import nka_amd
        torch, n, nsys, ld = self.torch, self.n, self.nsys, self.ld
        self.b = _ext(nsys, n, self.m, self.flavor)
        self.order, self.orders_met = nka_amd.SUMS_BLOCKED_ROUNDED, set()
        self.reference = nka_amd.SUMS_REFERENCE_ORDER
        self.raw = torch.zeros(nsys * ld, dtype=torch.float64, device="cuda")
        self.F = self.raw.view(nsys, ld)[:, :n]
        align = [(self.raw.data_ptr() + 8 * k * ld) % 16 for k in range(nsys)]
        assert align == ([8 * (k % 2) for k in range(nsys)] if odd_ld else [0] * nsys), align
        self.wts = E.system_weights(n, nsys)
        self.wraw, wdev = _strided(torch, self.wts, ld, pad=np.nan)
        self.b.set_dot_weights(wdev)
        assert self.b.dot_weighted()
        self._sys = None

    def _check(self, k, *args):
        self._sys = k
        super()._check(k, *args)

    def _sum(self, what, red, x, y, where):
        a = self.wts[self._sys] * x
        ex = X.exact_dot(a, y)
        assert math.isfinite(ex), (what, where)
        tot, k = X.abs_dot(a, y), self.k
        err = abs(red - ex)
        ratio = err / (X.U * tot) if tot else err
        print(f"  {what} {where}: |red - exact| = {ratio:.3f} u sum|fl(w x) y|, K = {k}")
        assert err <= X.gamma(k) * tot, (what, where, red, ex, ratio, k)
        if tot > 0 and ratio >= WORST[0]:
            WORST[:] = [ratio, k, f"{what} {where}"]


def _exact_cases():
    return [(n, m) for n in E.EXACT_LENGTHS for m in (3, 10)] + [(129, 32)]


@pytest.mark.parametrize("odd_ld", [False, True], ids=["ld-even", "ld-odd"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("n,mvec", _exact_cases())
def test_every_part_of_a_weighted_wave_update(torch_cuda, oracle, n, mvec, flavor, odd_ld):
    """The three layers of test_batch_waves_gpu.WavesRun on weighted sums; eleven systems, six starting delays in one launch."""
    if mvec == 32:
        run = WeightedWavesRun(torch_cuda, oracle, flavor, n, mvec, BWV.NSYS, odd_ld)
        rngs, prev = [np.random.default_rng([n, k]) for k in range(run.nsys)], [None] * run.nsys
        for t in range(mvec + 4):
            inputs = {}
            for k in range(run.nsys):
                if t >= k % 3:
                    inputs[k] = prev[k] = BWV.planted_input(n, rngs[k], prev[k])
            run.update(inputs)
        assert run.widest == mvec and run.nolder_normed == set(range(mvec + 1)), run.nolder_normed
        return
    run = G._planned_run(WeightedWavesRun(torch_cuda, oracle, flavor, n, mvec, BWV.NSYS, odd_ld), seed=1000 * mvec + n)
    assert run.lengths_differed and run.saw_zero_s and run.saw_after_restart and 0 in run.nolder_no_pending
    if n >= 63:
        assert run.widest == mvec, run.widest
        if mvec == T.SHAPE_MVEC:
            T._assert_planned_coverage(run)


def test_a_zero_weight_tail_is_a_shorter_system(torch_cuda):
    """vlen = 385, the lengths of test 1; w = 1 below the length and 0 from there on, finite garbage of magnitude 1e3 in the tail
    of every input.  Derived: fma(+-0, b, acc) = acc for finite b, and a lane meets its pairs in the same order at either length."""
    torch = torch_cuda
    vlen, mvec, lens = E.VLEN, 5, E.LENS
    nsys = len(lens)
    W = BL.mask_rows(lens, vlen)
    for flavor in (0, 1, 2):
        rng = np.random.default_rng([5, flavor])
        b = _ext(nsys, vlen, mvec, flavor).set_dot_weights(W)      # (host entry)
        short = [G._waves(1, ln, mvec, flavor) for ln in lens]
        seqs = BL.sequences(lens, 500 + flavor)
        for t in range(mvec + 4):
            host = 1.0e3 * rng.standard_normal((nsys, vlen))
            heads = [s.next() for s in seqs]
            for k, ln in enumerate(lens):
                host[k, :ln] = heads[k]
            F = _f64(torch, host)
            b.accel_update(F)
            got = F.cpu().numpy()
            assert np.isfinite(got).all()
            for k, ln in enumerate(lens):
                Fs = _f64(torch, heads[k].reshape(1, ln))
                short[k].accel_update(Fs)
                _same_system(b, k, short[k], 0, (flavor, t, ln))
                assert _bits_equal(got[k, :ln], Fs.cpu().numpy()[0]), (flavor, t, ln, "f")
        for a in [b] + short:
            a.delete()


@pytest.mark.parametrize("n", E.EXACT_LENGTHS)
def test_the_weighted_norm_and_the_stop_rule_at_its_edges(torch_cuda, n):
    """fnorm against sqrt(exact_dot(fl(w f), f)) within gamma(waves_k(n)) + 4u relative, with and without a pending pair; then
    tol = r, nextafter(r, 0), NaN, +inf and 0 on a zero row: a retired system keeps every byte."""
    torch = torch_cuda
    nsys, mvec = 5, 4
    bound = X.gamma(BWV.waves_k(n)) + 4.0 * X.U
    W = E.system_weights(n, nsys, seed=31)
    rng = np.random.default_rng([3, n])
    for flavor in (0, 1, 2):
        a, twin = (_ext(nsys, n, mvec, flavor).set_dot_weights(W) for _ in range(2))
        fn = _f64(torch, np.full(nsys, PLANTED))
        for t in range(3):                                   # call 0: no pending pair, f swept alone; then the shared sweep
            fh = np.stack([BWV.planted_input(n, rng) for _ in range(nsys)])
            Fa, Ft = _f64(torch, fh), _f64(torch, fh)
            a.accel_step(Fa, fnorm=fn)
            twin.accel_step(Ft, fnorm=fn)
            got = fn.cpu().numpy()
            for k in range(nsys):
                want = math.sqrt(X.exact_dot(W[k] * fh[k], fh[k]))
                print(f"  weighted fnorm n {n} flavour {flavor} call {t} system {k}: {abs(got[k] - want) / (X.U * want) if want else 0.0:.3f} u")
                assert abs(got[k] - want) <= bound * want, (n, flavor, t, k, got[k], want)
        f0, x0 = rng.standard_normal((nsys, n)), rng.standard_normal((nsys, n))
        f0[4] = 0.0
        r = _f64(torch, np.zeros(nsys))
        Ft = _f64(torch, f0)
        twin.accel_step(Ft, fnorm=r)                         # the probing call: tol = None
        r = r.cpu().numpy()
        assert r[4] == 0.0 and (r[:4] > 0).all()                # (the weights are positive at the sentinels, index 0 among them)
        snap = [G._snapshot(a, k, mvec) for k in range(nsys)]
        tol = np.array([r[0], np.nextafter(r[1], 0.0), np.nan, np.inf, 0.0])
        want = np.array([0, 1, 1, 0, 0], np.int32)
        F, Xd, mask, fnorm = _f64(torch, f0), _f64(torch, x0), _i32(torch, np.ones(nsys)), _f64(torch, np.full(nsys, PLANTED))
        a.accel_step(F, Xd, mask, _f64(torch, tol), fnorm)
        assert np.array_equal(mask.cpu().numpy(), want), (n, flavor, mask.cpu().numpy(), r, tol)
        assert _bits_equal(fnorm.cpu().numpy(), r)
        got, xg, ft = F.cpu().numpy(), Xd.cpu().numpy(), Ft.cpu().numpy()
        out = want == 0
        assert _bits_equal(got[out], f0[out]) and _bits_equal(xg[out], x0[out]), "a retired system's rows"
        for k in np.flatnonzero(out):
            assert G._snapshot(a, k, mvec) == snap[k], k
        assert _bits_equal(got[~out], ft[~out]) and _bits_equal(xg[~out], x0[~out] - ft[~out]), "the systems that went on"
        for k in np.flatnonzero(~out):
            assert G._snapshot(a, k, mvec) == G._snapshot(twin, k, mvec), k
        a.delete()
        twin.delete()


@pytest.mark.parametrize("form", ["shared", "rows"])
def test_a_weighted_wave_update_is_capturable_from_the_first_call(torch_cuda, form):
    """Captured before the first update, replayed against an eager twin; new values of the same form set between replays reach the
    next replay; setting weights while the stream captures returns NKA_HIP_ESTATE and changes nothing."""
    torch = torch_cuda
    nsys, vlen, mvec = 23, 300, 6
    pick = (lambda w: w[0]) if form == "shared" else (lambda w: w)
    w1, w2 = (_f64(torch, E.system_weights(vlen, nsys, seed=s)) for s in (71, 72))
    seqs = [B.Sequence(vlen, 700 + k) for k in range(nsys)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _ext(nsys, vlen, mvec).set_dot_weights(pick(w1))
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    eager = _ext(nsys, vlen, mvec).set_dot_weights(pick(w1))
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
        static.copy_(_f64(torch, Xh))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = _f64(torch, Xh)
        eager.accel_update(F)
        assert torch.equal(F, static), (form, t)
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], (form, t)
    plain = G._waves(nsys, vlen, mvec)                       # (and the weights did something)
    F = _f64(torch, Xh)
    plain.accel_update(F)
    assert plain.state_digest(0) != b.state_digest(0)
    for a in (b, eager, plain):
        a.delete()


def test_refusals_leave_the_previous_weights_and_lengths_in_force(torch_cuda):
    """The narrow batch's refusals on an ext batch: a bad entry in the last row only, 0 < ldw < vlen, a span one element short, NaN
    accepted in the padding; invalid lengths; NKA_HIP_ESTATE while capturing; set_sum_order as for a wave batch."""
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    nsys, vlen, mvec = 5, 133, 3
    rng = np.random.default_rng(8)
    W0 = E.system_weights(vlen, nsys, seed=81)
    lens0 = np.array([133, 1, 129, 64, 3], np.int32)
    b, twin = (_ext(nsys, vlen, mvec).set_dot_weights(W0).set_lengths(lens0) for _ in range(2))
    L, h = b._L, b._handle()

    def still_the_twins(calls=2):
        for _ in range(calls):
            Xh = rng.standard_normal((nsys, vlen))
            Fa, Fb = _f64(torch, Xh), _f64(torch, Xh)
            b.accel_update(Fa)
            twin.accel_update(Fb)
            assert torch.equal(Fa, Fb)
            for k in range(nsys):
                _same_system(b, k, twin, k, ("twins", k))

    still_the_twins()
    for bad in (-1.0, np.nan, np.inf, -np.inf):              # an entry in the LAST row only, through both entries
        Wb = np.ones((nsys, vlen))
        Wb[nsys - 1, 7] = bad
        with pytest.raises(NKAError, match=r"\(-1\).*first in row %d at index 7" % (nsys - 1)):
            b.set_dot_weights(Wb)
        with pytest.raises(NKAError, match=r"\(-1\)"):
            b.set_dot_weights(_f64(torch, Wb))
        assert b.dot_weighted()
    ok = torch.ones(nsys * vlen, dtype=torch.float64, device="cuda")
    for ldw in (1, vlen - 1, -1, -vlen):
        assert L.nka_hip_batch_set_dot_weights(h, C.c_void_p(ok.data_ptr()), ldw) == EINVAL, ldw
        assert L.nka_hip_batch_set_dot_weights_host(h, np.ones(nsys * vlen).ctypes.data_as(C.c_void_p), ldw) == EINVAL, ldw
    ws, short = C.c_void_p(), C.c_void_p()                   # a device buffer one element too short, in both forms
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    ldw = vlen + 3
    for count, form in (((nsys - 1) * ldw + vlen - 1, ldw), (vlen - 1, 0)):
        assert L.nka_hip_vec_alloc(ws, count, C.byref(short)) == 0
        torch.cuda.synchronize()
        assert L.nka_hip_batch_set_dot_weights(h, short, form) == EINVAL and b"shorter" in L.nka_hip_last_error(), form
        assert L.nka_hip_vec_free(ws, short) == 0
    assert L.nka_hip_vec_workspace_destroy(ws) == 0
    for bad in ([133, 1, 129, 64, 0], [133, 1, 129, 64, 134], [133, 1, 129, 64, -1]):      # the last entry only
        with pytest.raises(NKAError):
            b.set_lengths(np.array(bad, np.int32))
        with pytest.raises(NKAError):
            b.set_lengths(_i32(torch, bad))
        assert b.has_lengths() and b.lengths().tolist() == lens0.tolist()
    for order in (nka_amd.SUMS_REFERENCE_ORDER, nka_amd.SUMS_BLOCKED):
        assert L.nka_hip_batch_set_sum_order(h, order) == EINVAL and b"BLOCKED_ROUNDED" in L.nka_hip_last_error()
    b.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED).set_sum_order(nka_amd.SUMS_AUTO)
    with pytest.raises(NKAError, match="binary32"):
        nka_amd.nka_batch().init(4, 129, 3, waves=True, ext=True, storage=nka_amd.STORE_F32)
    side = torch.cuda.Stream()                               # NKA_HIP_ESTATE while the batch's stream captures
    with torch.cuda.stream(side):
        c = _ext(nsys, vlen, mvec)
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    lens_dev = _i32(torch, lens0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.accel_update(static)
        rcs = (L.nka_hip_batch_set_dot_weights(c._handle(), C.c_void_p(ok.data_ptr()), vlen),
               L.nka_hip_batch_set_dot_weights_host(c._handle(), W0.ctypes.data_as(C.c_void_p), vlen),
               L.nka_hip_batch_set_lengths(c._handle(), C.c_void_p(lens_dev.data_ptr())),
               L.nka_hip_batch_set_lengths_host(c._handle(), lens0.ctypes.data_as(C.POINTER(C.c_int32))))
    assert rcs == (ESTATE,) * 4 and not c.dot_weighted() and not c.has_lengths()
    still_the_twins()                                        # the previous weights and lengths stayed in force
    # garbage in the padding between rows is never read: accepted, through the device entry, and the weights are W1
    W1 = E.system_weights(vlen, nsys, seed=82)
    _, padded = _strided(torch, W1, vlen + 3, pad=np.nan)
    b.set_dot_weights(padded)
    twin.set_dot_weights(W1)
    still_the_twins()
    for a in (b, twin, c):
        a.delete()


# ---- 4. weights and lengths together --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odd", [False, True], ids=["ld-even", "ld-odd"])
def test_weights_and_lengths_together(torch_cuda, odd):
    """The lengths of test 1 at mvec = 3, flavour C, against ext twins of vlen = len carrying the same weights; the weight rows hold
    2^500 from the system's length on (a tail weight read into a sum overflows against the twin), NaN between two rows."""
    W = E.weight_rows(E.LENS, E.VLEN, seed=41)
    assert all((W[k, L:] == E.TAIL_WEIGHT).all() for k, L in enumerate(E.LENS))
    r = _run_plan(Twins(torch_cuda, E.LENS, E.VLEN, 3, 2, odd_ld=odd, odd_ldx=not odd, weights=W, odd_ldw=odd),
                  seed=41, where=("weights and lengths", odd))
    r.delete()


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------

IND_VLEN, IND_LEN, IND_MVEC, IND_CALLS = 300, 257, 3, 6


def _ind_inputs():
    rng, prev, out = np.random.default_rng(77), None, []
    for t in range(IND_CALLS):
        prev = prev.copy() if t == 4 else BWV.planted_input(IND_LEN, rng, prev)      # (call 4 repeats call 3: s == 0)
        out.append(prev)
    return out, E.draw_weights(IND_LEN, np.random.default_rng(78)), np.random.default_rng(79).standard_normal(IND_LEN)


def _ind_run(torch, nsys, pos, odd, others):
    """The system at `pos` of an ext batch of nsys, IND_LEN long with weights of its own, runs _ind_inputs() as steps with x; the
    others -- other lengths, other weights -- are masked, run inputs of their own, or are fed NaN / Inf -> per call: the system's
    rows of f and x, fnorm, red[], digest and every slot."""
    xs, w, x0 = _ind_inputs()
    rng = np.random.default_rng([5, nsys, pos])
    lens = rng.integers(1, IND_VLEN + 1, nsys).astype(np.int32)
    lens[pos] = IND_LEN
    W = np.exp2(rng.uniform(-2.0, 2.0, (nsys, IND_VLEN)))
    W[pos] = E.TAIL_WEIGHT
    W[pos, :IND_LEN] = w
    ld = _ld(IND_VLEN, odd)
    _, wrows = _strided(torch, W, ld, pad=np.nan)
    b = _ext(nsys, IND_VLEN, IND_MVEC).set_dot_weights(wrows).set_lengths(lens)
    xhost = BL.nan_paint(nsys, IND_VLEN, 6)
    xhost[:, :] = np.where(np.arange(IND_VLEN)[None, :] < lens[:, None], rng.standard_normal((nsys, IND_VLEN)), xhost)
    xhost[pos, :IND_LEN] = x0
    rawx, Xd = _strided(torch, xhost, ld)
    fnorm = _f64(torch, np.full(nsys, PLANTED))
    trace = []
    for t, x in enumerate(xs):
        host = rng.standard_normal((nsys, IND_VLEN))
        if others in ("nan", "inf") and t >= 2:
            host[:, 0] = np.nan if others == "nan" else np.inf
        host[pos] = BL.nan_paint(1, IND_VLEN, 7)[0]
        host[pos, :IND_LEN] = x
        mask = np.ones(nsys, np.int32)
        if others == "masked":
            mask[:] = 0
            mask[pos] = 1
        raw, F = _strided(torch, host, ld)
        b.accel_step(F, Xd, _i32(torch, mask), None, fnorm)
        got, gx = raw.view(nsys, ld).cpu().numpy(), rawx.view(nsys, ld).cpu().numpy()
        assert (got[:, IND_VLEN:] == BWV.PAD).all() and (gx[:, IND_VLEN:] == BWV.PAD).all(), "the padding between two rows was written"
        assert BL.same_bytes(got[pos, IND_LEN:IND_VLEN], host[pos, IND_LEN:]) and BL.same_bytes(gx[pos, IND_LEN:IND_VLEN], xhost[pos, IND_LEN:])
        if others == "masked":
            keep = np.arange(nsys) != pos
            assert BL.same_bytes(got[keep, :IND_VLEN], host[keep]) and BL.same_bytes(gx[keep, :IND_VLEN], xhost[keep]), "a masked neighbour's row"
        trace.append((got[pos, :IND_LEN].tobytes(), gx[pos, :IND_LEN].tobytes(), float(fnorm[pos].item())) + G._snapshot(b, pos, IND_MVEC))
    assert np.isfinite(got[pos, :IND_LEN]).all() and np.isfinite(b.reductions(pos)).all()
    b.delete()
    return trace


@pytest.fixture(scope="module")
def ind_reference(torch_cuda):
    return _ind_run(torch_cuda, 1, 0, False, "active")


@pytest.mark.parametrize("others", ["active", "masked", "nan", "inf"])
@pytest.mark.parametrize("nsys", [1, 4, 5, 9])
def test_the_bits_do_not_depend_on_the_batch_around_a_system(torch_cuda, ind_reference, nsys, others):
    """Every position 0 ... nsys - 1 (every wavefront of a full, a ragged and a lone workgroup), both parities of ld = ldx = ldw."""
    for pos in range(nsys):
        for odd in (False, True):
            assert _ind_run(torch_cuda, nsys, pos, odd, others) == ind_reference, (nsys, pos, odd, others)


# ---- 6. a whole solve ------------------------------------------------------------------------------------------------------------------

def test_a_ragged_weighted_solve_replays_with_no_host_in_the_loop(torch_cuda):
    """The solve of tests/batch_waves_ext.py -- batch_step.solve_problem() with a length and weights per system --: [residual;
    accel_step] captured ONCE, before any update, and replayed SOLVE_REPLAYS times (the budget the CPU test holds on the oracle) with
    thresholds formed on the device after the first replay.  The eager twin is an ext batch of the same lengths and weights running
    accel_update under masks the host forms from a probe's accel_step norms -- this kind's bits: all of it ==."""
    torch = torch_cuda
    nsys, vlen, mvec = S.SOLVE_NSYS, S.SOLVE_VLEN, S.SOLVE_MVEC
    d, eps, bb, x0 = (_f64(torch, a) for a in S.solve_problem())
    left, right = (_f64(torch, a) for a in E.solve_couplings())
    lens, W = E.solve_lengths(), E.solve_weights()
    inside = torch.from_numpy(np.arange(vlen)[None, :] < lens[:, None]).cuda()

    def new():
        return _ext(nsys, vlen, mvec, S.SOLVE_FLAVOR).set_dot_weights(W).set_lengths(lens)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = new()
        Xs, Fs = x0.clone(), torch.zeros_like(x0)
        mask, tol, fnorm = _i32(torch, np.ones(nsys)), _f64(torch, np.zeros(nsys)), _f64(torch, np.zeros(nsys))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        Fs.copy_(E.solve_residual(torch, Xs, d, eps, bb, left, right))
        b.accel_step(Fs, Xs, mask, tol, fnorm)
    with torch.cuda.stream(side):
        g.replay()
        torch.mul(fnorm, S.SOLVE_TOL, out=tol)
        for _ in range(E.SOLVE_REPLAYS - 1):
            g.replay()
    torch.cuda.synchronize()

    eager, probe = new(), new()
    Xe, alive, tolh = x0.clone(), np.ones(nsys, bool), np.zeros(nsys)
    retired = np.full(nsys, -1)
    rdev = _f64(torch, np.zeros(nsys))
    for it in range(E.SOLVE_REPLAYS):
        Fe = E.solve_residual(torch, Xe, d, eps, bb, left, right).contiguous()
        probe.restart()
        probe.accel_step(Fe.clone(), fnorm=rdev)
        r = rdev.cpu().numpy()
        if it == 1:
            tolh = S.SOLVE_TOL * r0
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
    res = E.solve_residual(np, Xs.cpu().numpy(), *(a.cpu().numpy() for a in (d, eps, bb, left, right)))
    res[~inside.cpu().numpy()] = 0.0
    assert (np.linalg.norm(res, axis=1) <= 1e-7).all()       # (and it is a solution)
    for x in (b, eager, probe):
        x.delete()


# ---- 7. offers, kinds, coexistence ------------------------------------------------------------------------------------------------------

def test_offers_kinds_and_coexistence(torch_cuda):
    import nka_amd
    from nka_amd import NKAError
    torch = torch_cuda
    new = nka_amd.nka_batch
    table = {"narrow": (new().init(4, 129, 3), True, True, 0),
             "stored": (new().init(4, 129, 3, storage=nka_amd.STORE_F32), True, True, 0),
             "wide": (new().init(4, 4099, 3, wide=True), True, False, 1),
             "wide_step": (new().init(4, 4099, 3, wide=True, step=True), True, False, 1),
             "lanes": (new().init(4, 33, 3, lanes=True), False, False, 2),
             "waves": (new().init(4, 129, 3, waves=True), False, False, 3),
             "waves_ext": (new().init(4, 129, 3, waves=True, ext=True), True, True, 3)}
    L = new()._L
    for name, (b, lengths, weights, kind) in table.items():
        assert (b.offers_lengths(), b.offers_weights(), b.kind()) == (lengths, weights, kind), name
        assert (L.nka_hip_batch_offers_lengths(b._handle()), L.nka_hip_batch_offers_weights(b._handle())) == (int(lengths), int(weights)), name
        vlen = b.lengths().size and int(b.lengths()[0])
        for offered, call in ((lengths, lambda: b.set_lengths(np.full(4, vlen, np.int32))), (weights, lambda: b.set_dot_weights(np.ones(vlen)))):
            if offered:
                call()
            else:
                with pytest.raises(NKAError):
                    call()
    assert L.nka_hip_batch_offers_lengths(None) < 0 and L.nka_hip_batch_offers_weights(None) < 0
    with pytest.raises(NKAError, match="waves=True"):
        new().init(4, 129, 3, ext=True)
    old = table["waves"][0]                                  # a batch of the old entry still refuses both, with today's message
    h = old._handle()
    w, lens = _f64(torch, np.ones((4, 129))), _i32(torch, np.full(4, 129))
    assert L.nka_hip_batch_set_dot_weights(h, C.c_void_p(w.data_ptr()), 129) == EINVAL
    assert b"not offered by a wave batch (nka_hip_batch_create_waves): nka_hip_batch_create" in L.nka_hip_last_error()
    assert L.nka_hip_batch_set_lengths(h, C.c_void_p(lens.data_ptr())) == EINVAL
    assert b"not offered by a wave batch (nka_hip_batch_create_waves): nka_hip_batch_create" in L.nka_hip_last_error()
    assert not old.dot_weighted() and not old.has_lengths()
    for b, *_ in table.values():
        b.delete()
    # an ext batch with nothing set == a plain wave twin (it runs the same kernels), beside it in one process
    nsys, vlen, mvec = 9, 257, 4
    rng = np.random.default_rng(7)
    for flavor in (0, 1, 2):
        a, plain = _ext(nsys, vlen, mvec, flavor), G._waves(nsys, vlen, mvec, flavor)
        assert a.vector_bytes() == plain.vector_bytes() and not a.dot_weighted() and not a.has_lengths()
        Xa, Xp = (_f64(torch, np.ones((nsys, vlen))) for _ in range(2))
        for t in range(mvec + 3):
            Xh = rng.standard_normal((nsys, vlen))
            Fa, Fp = _f64(torch, Xh), _f64(torch, Xh)
            if t % 2:
                a.accel_step(Fa, Xa)
                plain.accel_step(Fp, Xp)
            else:
                a.accel_update(Fa)
                plain.accel_update(Fp)
            assert torch.equal(Fa, Fp) and torch.equal(Xa, Xp), (flavor, t)
        for k in range(nsys):
            assert G._snapshot(a, k, mvec) == G._snapshot(plain, k, mvec), (flavor, k)
        a.delete()
        plain.delete()


# ---- 8. the weight buffer, the caller's weight rows and F beyond 2^32 bytes ---------------------------------------------------------------

def test_weights_rows_and_f_beyond_4_gib(torch_cuda):
    """batch_waves_ext.large_shape (held by the CPU test): 2^19 + 3 systems of 1024, mvec = 1; row 2^19 of F, of X, of the caller's
    weights and of the batch's weight buffer starts on byte 2^32, the slots pass it at system 2^18.  Seven systems run the weighted
    step with lengths -- the first, the last, both sides of either boundary --, every other one is masked; those that run equal a
    small ext twin after every call, the masked witnesses stay fresh, and no element of F or X that no running system owns moves.
    The rules and the memory guard of tests/test_batch_large_gpu.py."""
    torch = torch_cuda
    sh = E.large_shape()
    nsys, vlen, mvec, act = sh["nsys"], sh["vlen"], sh["mvec"], sh["active"]
    na = len(act)
    assert 5 <= na <= E.MAX_ACTIVE
    need = sum(E.large_bytes(sh).values())
    free, total = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip(f"{free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 8 GiB")
    big = twin = None
    try:
        big, twin = _ext(nsys, vlen, mvec), _ext(na, vlen, mvec)
        fresh = big.state_digest(sh["witnesses"][0])
        idx = torch.tensor(act, dtype=torch.int64, device="cuda")
        lens = np.full(nsys, vlen, np.int32)
        tl = np.array([sh["lens"][k] for k in act], np.int32)
        lens[act] = tl
        wsrc = torch.ones(nsys, vlen, dtype=torch.float64, device="cuda")
        assert wsrc.numel() * 8 > 2 ** 32
        tw = E.weight_rows(tl.tolist(), vlen, seed=91)
        wsrc[idx] = _f64(torch, tw)
        big.set_dot_weights(wsrc).set_lengths(lens)
        twin.set_dot_weights(tw).set_lengths(tl)
        del wsrc                                              # (copied by the set)
        torch.cuda.empty_cache()
        F = torch.full((nsys, vlen), BWV.PAD, dtype=torch.float64, device="cuda")
        Xd = torch.full((nsys, vlen), BWV.PAD, dtype=torch.float64, device="cuda")
        mask = torch.zeros(nsys, dtype=torch.int32, device="cuda")
        mask[idx] = 1
        tmask = _i32(torch, np.ones(na))
        fnorm, tfnorm = torch.full((nsys,), PLANTED, dtype=torch.float64, device="cuda"), _f64(torch, np.full(na, PLANTED))
        tol = ttol = None
        rng = np.random.default_rng(9)
        xpaint = BL.nan_paint(na, vlen, 2)
        for j, L in enumerate(tl):
            xpaint[j, :L] = rng.standard_normal(L)
        Xd[idx] = _f64(torch, xpaint)
        Xt = _f64(torch, xpaint)
        for t in range(6):
            if t == 2:                                       # thresholds from the device's own norms: half of them retire
                tol, ttol = fnorm.clone(), tfnorm.clone()
                tol[idx[::2]] = 0.0
                ttol[::2] = 0.0
            if t == 4:
                m, tm = torch.zeros_like(mask), torch.zeros_like(tmask)
                m[idx[:2]] = 1
                tm[:2] = 1
                big.relax(m)
                twin.relax(tm)
            paint = BL.nan_paint(na, vlen, 1)
            scale = 1.0 if t < 2 else 0.25 if t == 2 else 8.0      # (call 2: a quarter of the norm -- below the threshold)
            for j, L in enumerate(tl):
                paint[j, :L] = scale * rng.standard_normal(L)
            F[idx] = _f64(torch, paint)
            Ft = _f64(torch, paint)
            big.accel_step(F, Xd, mask, tol, fnorm)
            twin.accel_step(Ft, Xt, tmask, ttol, tfnorm)
            assert torch.equal(mask[idx], tmask), (t, "mask")
            assert BL.same_bytes(fnorm[idx].cpu().numpy(), tfnorm.cpu().numpy()), (t, "fnorm")
            assert BL.same_bytes(F[idx].cpu().numpy(), Ft.cpu().numpy()), (t, "F and its tails")
            assert BL.same_bytes(Xd[idx].cpu().numpy(), Xt.cpu().numpy()), (t, "X and its tails")
            for j, L in enumerate(tl):
                assert BL.same_bytes(Ft[j, L:].cpu().numpy(), paint[j, L:]), (t, j, "the twin's own tail")
            for j, k in enumerate(act):
                _same_system(big, k, twin, j, (t, k))
        assert 0 < int(tmask.sum().item()) < na, "some systems retired, some went on"
        for j, k in enumerate(act):
            for s in range(1, mvec + 2):
                assert BL.same_bytes(big.w(k, s), twin.w(j, s)) and BL.same_bytes(big.v(k, s), twin.v(j, s)), (k, s)
        F[idx] = BWV.PAD
        Xd[idx] = BWV.PAD
        assert bool((F == BWV.PAD).all()) and bool((Xd == BWV.PAD).all()), "a row of a masked system was written"
        mask[idx] = 0
        fnorm[idx] = PLANTED
        assert not bool(mask.any()) and bool((fnorm == PLANTED).all()), "the mask or fnorm of a masked system was written"
        nv = big.num_vec()
        idle = np.ones(nsys, bool)
        idle[act] = False
        assert (nv[idle] == 0).all()
        zero = np.zeros(vlen).tobytes()
        for k in sh["witnesses"]:
            assert big.state_digest(k) == fresh, k
            for s in range(1, mvec + 2):
                assert big.w(k, s).tobytes() == zero and big.v(k, s).tobytes() == zero, (k, s)
    finally:
        for a in (big, twin):
            if a is not None:
                a.delete()
        torch.cuda.empty_cache()


# ---- the record (keep this test last) ----------------------------------------------------------------------------------------------------
def test_worst_ratio_of_the_weighted_wave_sums_is_printed_and_inside_its_bound(capsys):
    """The worst |red - exact| / (u sum|fl(w x) y|) the tests above saw, printed past the output capture, and once more held to the
    K it was judged by.  Selected on its own it has nothing to report."""
    ratio, k, where = WORST
    if not where:
        return
    with capsys.disabled():
        print("\n" + _worst_line())
    assert ratio <= (k + 1) / (1.0 - (k + 1) * X.U), (ratio, k, where)      # gamma(k) / u
