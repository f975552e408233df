"""Every reduction of the fast sum modes against the exact sums (tests/exact_sums.py).

After each update every live entry of red[] (nka_hip_get_reductions) is compared with the correctly rounded sum of the
vectors as they were at entry, within K u sum|x y|, K derived from the launch geometry (exact_sums.device_k).  A host
mirror keeps the stored w vectors; only the slots the update wrote are read back, and checked bit for bit on the way:
the new pair's w is the input, the normalised pair's w1' is fl(d/s) (fl(fl(1/s) d) in the vector flavour) with the
device's own s = sqrt(red[0]).

  NKA_HIP_SUMS_BLOCKED_ROUNDED (the default beyond 64 elements): red[0] = <d,d>, d = fl(w1 - f); red[1] = <f,w1'>;
      red[2+p] = <w1',w_p>; red[2+m+p] = <f,w_p>; with s == 0, red[1] and the Gram row are exactly 0.
  NKA_HIP_SUMS_BLOCKED: red[1] = <f,d>, red[2+p] = <d,w_p>, the rest as above.
  Entries past the list's older count are exactly 0.

The inputs carry planted sentinels where the kernels change hands (exact_sums.sentinel_indices); the CPU test
tests/test_exact_sums_cpu.py shows that losing or doubling any one of them breaks the bound at these shapes.
"""
import json
import math
import os

import numpy as np
import pytest

import exact_sums as X
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

ROUNDED, BLOCKED = 3, 2             # nka_amd.SUMS_BLOCKED_ROUNDED, nka_amd.SUMS_BLOCKED (the default first)
MODES = pytest.mark.parametrize("mode", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])
WORST = {}                          # mode -> worst |red - exact| / (u sum|xy|) seen, and the K it was held to


@pytest.fixture(scope="module", autouse=True)
def _report_worst(request):
    """At the end of the module: per mode, the worst |red - exact| / (u sum|xy|) seen and the K it was held to."""
    yield
    import parity_util as P
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    rows = {}
    for mode, (ratio, k, where) in sorted(WORST.items()):
        name = "rounded" if mode == ROUNDED else "blocked"
        rows[name] = {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}
        line = f"sums mode {name}: worst |red - exact| = {ratio:.3f} u sum|xy| against K = {k} there ({where})"
        tr.write_line(line) if tr is not None else print(line)
    out = P.dump_dir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if rows and out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "sums_exact_worst.json"), "w") as fh:
            json.dump(rows, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ncu(torch_cuda):
    import nka_amd
    acc = nka_amd.nka().init(1, 1)
    _, g = acc.device_info()
    acc.delete()
    assert g >= 1
    return g


def _hold(mode, what, red, x, y, k, where):
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
    if tot > 0:
        r = WORST.setdefault(mode, [0.0, 0, ""])
        ratio = err / (X.U * tot)
        if ratio >= r[0]:
            r[:] = [ratio, k, f"{what} {where}"]


class Run:
    """One accelerator in a fast sum mode, its host mirror, and the checks after each update."""

    def __init__(self, torch, ncu, mode, flavor, n, mvec, aligned=True, seed=0):
        import nka_amd
        self.torch, self.mode, self.flavor, self.n, self.m = torch, mode, flavor, n, mvec
        self.acc = nka_amd.nka().init(n, mvec, flavor=flavor).set_sum_order(mode)
        self.G = ncu
        self.k = X.device_k(n, ncu, aligned)
        self.aligned = aligned
        self.rng = np.random.default_rng(seed)
        self.W = {}                  # slot -> stored w (host mirror)
        self.prev = None
        self.widest = 0              # longest list of older vectors seen at the entry of an update
        if aligned:
            self.buf = torch.zeros(n, dtype=torch.float64, device="cuda")
            self.view = self.buf
        else:
            self.buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
            self.view = self.buf[1:]                                 # 8-byte but not 16-byte aligned
            assert self.view.data_ptr() % 16 == 8

    def next_input(self, repeat=False):
        return self.prev.copy() if repeat else X.planted_input(self.n, self.G, self.rng, self.prev)

    def update(self, x, where=""):
        """accel_update(x) on the device, then every check of the module docstring; returns the output f."""
        torch, n, m = self.torch, self.n, self.m
        st0 = self.acc.state()
        order0 = st0.list_order()
        pending = st0.pending
        olders = order0[1:] if pending else order0
        self.widest = max(self.widest, len(olders))
        self.view.copy_(torch.from_numpy(x))
        self.acc.accel_update(self.view)
        out = self.view.cpu().numpy()
        red = self.acc.reductions()
        where = (self.mode, self.flavor, n, m, self.aligned, where)
        w1n = None
        if pending:
            d = self.W[order0[0]] - x                                   # F08:266
            self._hold("<d,d>", red[0], d, d, where)
            s = np.sqrt(np.float64(red[0]))                             # the device's s, IEEE sqrt (NaN, Inf, 0 included)
            with np.errstate(invalid="ignore", divide="ignore"):
                w1n = (np.float64(1.0) / s) * d if self.flavor == 1 else d / s      # F08:283, F08V:256
            if self.mode == ROUNDED:
                op = np.zeros(n) if s == 0.0 else w1n                   # (s == 0: the scalar step relaxes, these are 0)
                if s == 0.0:
                    assert red[1] == 0.0 and all(red[2 + p] == 0.0 for p in range(len(olders))), (where, red)
                self._hold("<f,w1'>", red[1], x, op, where)
                for p, k in enumerate(olders):
                    self._hold(f"<w1',w_{p}>", red[2 + p], op, self.W[k], where)
            else:
                self._hold("<f,d>", red[1], x, d, where)
                for p, k in enumerate(olders):
                    self._hold(f"<d,w_{p}>", red[2 + p], d, self.W[k], where)
        if pending or olders:
            for p, k in enumerate(olders):
                self._hold(f"<f,w_{p}>", red[2 + m + p], x, self.W[k], where)
            for p in range(len(olders), m):                              # past the list: exactly 0
                assert red[2 + p] == 0.0 and red[2 + m + p] == 0.0, (where, p, red[2 + p], red[2 + m + p])
        # the mirror: read back only the slots this update wrote
        order = self.acc.state().list_order()
        new = order[0]
        w_new = self.acc.w(new)
        assert _bits_equal(w_new, x), (where, "the new pair's w is not the input")
        W = {k: self.W[k] for k in order[1:] if k in self.W and k != (order0[0] if pending else None)}
        if pending and order0[0] in order[1:]:
            w1 = self.acc.w(order0[0])
            assert _bits_equal(w1, w1n), (where, "stored w1' is not fl(d/s)", int(np.sum(w1 != w1n)))
            W[order0[0]] = w1
        W[new] = w_new
        self.W = W
        self.prev = x
        return out

    def _hold(self, what, red, x, y, where):
        _hold(self.mode, what, red, x, y, self.k, where)

    def sequence(self, nupd, repeat_at=()):
        for t in range(nupd):
            self.update(self.next_input(repeat=t in repeat_at and self.prev is not None), where=t)
        assert self.acc.defined()
        return self


# ---- every PA width ---------------------------------------------------------------------------------------------------------
# mvec = 32: the list grows through every k_dots_win<MAXL, W> width 1..32 (rings of 4, 5, 6, 3, 7 and the primes, prime_pad 23,
# 29, 31); mvec = 64: the balanced passes 33..64; the second update of each (only the pending pair) runs k_dots<4, 2>.
# Fresh random inputs in 513 / 4099 / 20011 dimensions stay independent: no drops, the list reaches its capacity.
WIDTH_CASES = [(513, 0), (513, 1), (513, 2), (4099, 0), (4099, 1), (4099, 2), (20011, 2)]


@MODES
@pytest.mark.parametrize("n,flavor", WIDTH_CASES)
def test_every_pa_width_against_exact_sums(torch_cuda, ncu, mode, n, flavor):
    for mvec in (32, 64):
        r = Run(torch_cuda, ncu, mode, flavor, n, mvec, seed=n + mvec + flavor)
        r.sequence(mvec + 2, repeat_at=(mvec + 1,))
        assert r.widest == mvec, (mvec, r.widest)              # no drop: every width was visited


# ---- the boundary shapes ----------------------------------------------------------------------------------------------------
# tiny shapes with a list that grows to 6 and a repeated input (s == 0); one tile per block with a list of 4; the
# hand-over of k_norm_diff's ahead loop with a list of 2 (host fsum time, not the GPU, is the cost there)
def _shape_plan(n, G):
    if n <= 4099:
        return 6, 10, (5,)
    if n <= G * 512 + 1:
        return 4, 7, (4,)
    return 2, 4, ()


SHAPE_IDS = ["1", "2", "7", "63", "64", "65", "511", "512", "513", "Gt-1", "Gt", "Gt+1",
             "8Gt-1", "8Gt", "8Gt+1", "8Gt+511", "9Gt+77"]          # t = 512 elements, G = the CU count
# (shape, aligned, mode): every shape in both modes, with f aligned and with f 8-byte but not 16-byte aligned (buf[1:])
SHAPE_CASES = [(i, a, m) for i in range(17) for a in (True, False) for m in (ROUNDED, BLOCKED)]


@pytest.mark.parametrize("which,aligned,mode", SHAPE_CASES,
                         ids=[f"{SHAPE_IDS[i]}-{'aligned' if a else 'unaligned'}-{'rounded' if m == ROUNDED else 'blocked'}"
                              for i, a, m in SHAPE_CASES])
def test_every_sum_at_the_boundary_shapes(torch_cuda, ncu, which, aligned, mode):
    n = X.boundary_shapes(ncu)[which]
    mvec, nupd, rep = _shape_plan(n, ncu)
    for flavor in ((0, 1, 2) if n <= 4099 else ((0, 1, 2)[which % 3],)):       # (the large shapes: one flavour each, in turn)
        Run(torch_cuda, ncu, mode, flavor, n, mvec, aligned=aligned, seed=which).sequence(nupd, repeat_at=rep)


@MODES
def test_sums_when_pb_hands_out_tiles_by_tickets(torch_cuda, ncu, mode):
    """n / 512 >= 64 G: PB takes its tiles by tickets (pb_tickets_apply) in the same updates whose sums are checked here, and
    the next update's sums read what it stored.  Aligned only: the scalar path has no tickets."""
    n = X.pb_ticket_shape(ncu)
    Run(torch_cuda, ncu, mode, 2, n, 1, seed=5).sequence(3)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_non_finite_input_in_the_default_mode(torch_cuda, ncu, oracle, bad, flavor):
    """A NaN / an Inf in f: red[0] and every sum are NaN / Inf exactly where the exact sum is, and the decisions are the
    oracle's, on the update that sees it and the two after it."""
    n, m = 1000, 3
    r = Run(torch_cuda, ncu, ROUNDED, flavor, n, m, seed=11)
    ora = oracle.OracleNKA(n, m, flavor)
    for t in range(7):
        x = r.next_input()
        if t == 3:
            x[5] = bad
        f = x.copy()
        ora.accel_update(f)
        out = r.update(x, where=t)
        assert r.acc.num_vec() == ora.num_vec(), t
        assert r.acc.state().list_order() == ora.state().list_order(), t
        assert np.array_equal(np.isnan(out), np.isnan(f)), t
