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
import os

import numpy as np
import pytest

import exact_sums as X
import split_update as U

pytestmark = pytest.mark.gpu

ROUNDED, BLOCKED = 3, 2             # nka_amd.SUMS_BLOCKED_ROUNDED, nka_amd.SUMS_BLOCKED (the default first)
MODES = pytest.mark.parametrize("mode", [ROUNDED, BLOCKED], ids=["rounded", "blocked"])


@pytest.fixture(scope="module", autouse=True)
def _report_worst(request):
    """At the end of the module: per mode, the worst |red - exact| / (u sum|xy|) seen and the K it was held to."""
    U.WORST.clear()
    yield
    import parity_util as P
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    rows = {}
    for way, (ratio, k, where) in sorted(U.WORST.items()):
        name = "rounded" if way == "R" else "blocked"
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


class Run:
    """One accelerator in a fast sum mode for life: tests/split_update.py's SplitRun -- which holds the sums as described above
    and, on the way, the scalar step and the elementwise statements -- behind the calls of this module."""

    def __init__(self, torch, ncu, mode, flavor, n, mvec, aligned=True, seed=0):
        import nka_amd
        from oracle import oracle_py
        self.mode, self.flavor, self.n, self.m, self.G, self.aligned = mode, flavor, n, mvec, ncu, aligned
        self.acc = nka_amd.nka().init(n, mvec, flavor=flavor)
        self.run = U.SplitRun(torch, oracle_py, self.acc, flavor, n, mvec, mode, aligned=aligned)
        assert self.run.ncu == ncu
        self.rng = np.random.default_rng(seed)
        self.prev = None

    @property
    def widest(self):
        """The longest list of older vectors seen at the entry of an update."""
        return self.run.widest

    def next_input(self, repeat=False):
        return self.prev.copy() if repeat else X.planted_input(self.n, self.G, self.rng, self.prev)

    def update(self, x):
        """accel_update(x) on the device, then every check of the module docstring; returns the output f."""
        out = self.run.update(x)
        self.prev = x
        return out

    def sequence(self, nupd, repeat_at=()):
        for t in range(nupd):
            self.update(self.next_input(repeat=t in repeat_at and self.prev is not None))
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
        out = r.update(x)
        assert r.acc.num_vec() == ora.num_vec(), t
        assert r.acc.state().list_order() == ora.state().list_order(), t
        assert np.array_equal(np.isnan(out), np.isnan(f)), t
