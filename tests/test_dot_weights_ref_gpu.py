"""Diagonal dot-product weights held to INDEPENDENT references (include/nka_hip.h: nka_hip_set_dot_weights):
  4. every live sum of a weighted update against the exact sum of its operands, exact_sums.exact_dot(fl(w o a), b), within
     the blocked-sum bound K u sum|fl(w a) b| of tests/test_sums_exact_gpu.py (same K = device_k);
  5. the compiled src-C reference with the same weights in its user dot product: decisions exact, f within 1e-10;
  9. the Fortran front end (nka_amd/fortran/array/nka_weights_driver.F90): the same per-update digests with no weights,
     w == 1 and w == 4, set from a host array and from device memory, and through a deep copy."""
import math
import os
import subprocess

import numpy as np
import pytest

import exact_sums as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _ncu():
    import nka_amd
    a = nka_amd.nka().init(1, 1)
    return a.device_info()[1]


def _hold(what, red, x, y, k, where):
    ex = X.exact_dot(x, y)
    tot = X.abs_dot(x, y)
    err = abs(red - ex)
    assert err <= X.gamma(k) * tot, (what, where, red, ex, err / (X.U * tot) if tot else err, k)
    if tot > 0:
        WORST[what] = max(WORST.get(what, 0.0), err / (X.U * tot))


@pytest.mark.parametrize("order", [3, 2], ids=["rounded", "blocked"])
@pytest.mark.parametrize("n,m", [(20011, 5), (300_037, 12)])
def test_weighted_sums_hold_the_exact_sums(torch_cuda, order, n, m):
    """4. General weights in [2^-3, 2^3] (not powers of two), 10 % zeros, planted inputs: after every update each live red[]
    entry lies within K u sum|fl(w a) b| of the exact sum of fl(w o a) and b, the operands of the header's table."""
    import nka_amd
    torch = torch_cuda
    ncu = _ncu()
    k = X.device_k(n, ncu, True)
    rng = np.random.default_rng(n + order)
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0
    acc = nka_amd.nka().init(n, m).set_sum_order(order).set_dot_weights(w)      # default flavour: w1' = d / s
    W, prev = {}, None
    view = torch.zeros(n, dtype=torch.float64, device="cuda")
    for t in range(m + 6):
        x = X.planted_input(n, ncu, rng, prev)
        st0 = acc.state()
        order0 = st0.list_order()
        pending = st0.pending
        olders = order0[1:] if pending else order0
        view.copy_(torch.from_numpy(x))
        acc.accel_update(view)
        red = acc.reductions()
        where = (order, n, m, t)
        fw = w * x
        if pending:
            d = W[order0[0]] - x
            dw = w * d
            _hold("<wd,d>", red[0], dw, d, k, where)
            s = np.sqrt(np.float64(red[0]))
            assert s > 0.0
            w1n = d / s
            if order == 3:
                _hold("<wf,w1'>", red[1], fw, w1n, k, where)
                for p, q in enumerate(olders):
                    _hold("<ww1',w_p>", red[2 + p], w * w1n, W[q], k, where)
            else:
                _hold("<wf,d>", red[1], fw, d, k, where)
                for p, q in enumerate(olders):
                    _hold("<wd,w_p>", red[2 + p], dw, W[q], k, where)
        for p, q in enumerate(olders):
            _hold("<wf,w_p>", red[2 + m + p], fw, W[q], k, where)
        for p in range(len(olders), m):
            assert red[2 + p] == 0.0 and red[2 + m + p] == 0.0
        order1 = acc.state().list_order()
        W = {q: acc.w(q) for q in order1}
        prev = x
    print(f"exact sums with weights n={n} m={m} order={order}: worst err / (u sum|ab|) "
          + ", ".join(f"{kk} {v:.2f}" for kk, v in sorted(WORST.items())) + f" (K = {k})")


@pytest.mark.parametrize("order", [3, 2], ids=["rounded", "blocked"])
def test_against_the_compiled_reference_with_a_weighted_dot_product(torch_cuda, order):
    """5. oracle_py.RefC (the reference's src-C accelerator, compiled) with dp(x, y) = sum w x y in its sequential order,
    n = 1e5, m = 10, 30 calls: num_vec and the list order equal after every call, ||f_dev - f_ref|| / ||f_in|| <= 1e-10."""
    import nka_amd
    from oracle import oracle_py
    torch = torch_cuda
    n, m = 100_000, 10
    rng = np.random.default_rng(55 + order)
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0

    def dp(x, y):
        return float(np.sum((w * x) * y))

    ref = oracle_py.RefC(n, m, dp=dp)
    acc = nka_amd.nka().init(n, m, flavor=2).set_sum_order(order).set_dot_weights(w)
    worst = 0.0
    for t in range(30):
        x = rng.standard_normal(n)
        fr = x.copy()
        ref.accel_update(fr)
        ft = torch.from_numpy(x.copy()).cuda()
        acc.accel_update(ft)
        fd = ft.cpu().numpy()
        assert acc.num_vec() == ref.num_vec(), (t, acc.num_vec(), ref.num_vec())
        assert acc.state().list_order() == ref.state().list_order(), t
        e = float(np.linalg.norm(fd - fr) / np.linalg.norm(x))
        worst = max(worst, e)
        assert e <= 1e-10, (t, e)
    print(f"weighted dp against the compiled reference, order {order}: worst ||f_dev - f_ref|| / ||f_in|| = {worst:.3e}")


def test_fortran_front_end_weights():
    """9. The Fortran driver: identical digests per update for no weights, w == 1 and w == 4 (host and device forms, and a
    deep copy); it stops with an error at the first difference."""
    import nka_amd
    if not os.path.exists(nka_amd.lib_path()):
        nka_amd.build()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "nka_amd", "fortran")], check=True)
    exe = os.path.join(ROOT, "nka_amd", "fortran", "build", "nka_weights_driver")
    for flavor in ("0", "1", "2"):
        p = subprocess.run([exe, "100003", "6", "14", flavor], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("digests ")]
        assert len(lines) == 14 and p.stdout.splitlines()[-1] == "OK", p.stdout
        for ln in lines:
            assert len(set(ln[2:])) == 1, ln
        assert len({ln[2] for ln in lines}) == 14            # the state moves on every call
