"""Binary32 storage of a batch's normalised subspace vectors (nka_hip_batch_create_stored; include/nka_hip_batch.h, STORAGE) as
far as a machine without a GPU can see it: the allocation arithmetic against a brute-force layout, the convergence of the host
model that fixes the budget of the GPU solve, and the proof that the bound of the exact-sum layer of
tests/test_batch_store32_gpu.py notices an operand that was not rounded as the contract says."""
import json
import os
import subprocess

import numpy as np
import pytest

import batch_step as T
import batch_store32 as S32
import batch_weights as BW
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: the allocation formula ---------------------------------------------------------------------------------------------

def test_layout_arithmetic_under_sanitizers():
    """tests/c/batch_store32_check.cpp, a stand-alone program built with -fsanitize=address,undefined: slot rows of floats and
    the pending rows of three systems painted byte by byte (no two pieces overlap, rows on 128 bytes, pairs on 8), the formula
    of the header, and every offset and size at the largest legal arguments against __int128."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "store32check"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_store32_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize("nsys,vlen,mvec", [(1, 1, 1), (3, 65, 6), (5, 513, 10), (2, 700, 32), (4, 1025, 20)])
def test_expected_allocation_sizes_against_a_brute_force_layout(nsys, vlen, mvec):
    """The sizes the GPU test expects of the library (batch_store32.vector_bytes) hold every row of the brute-force layout:
    no two rows of an allocation overlap, every row ends inside, pairs of a float row start on 8 bytes."""
    for storage in (S32.STORE_F64, S32.STORE_F32):
        rows = S32.pieces(nsys, vlen, mvec, storage)
        eb = 4 if storage == S32.STORE_F32 else 8
        per_alloc = {}
        for a, lo, hi in rows:
            per_alloc.setdefault(a, []).append((lo, hi))
        total = 0
        for a, spans in per_alloc.items():
            spans.sort()
            assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1)), (a, "rows overlap")
            size = (eb if a in "wv" else 8) * nsys * S32.slot_stride(vlen) * ((mvec + 1) if a in "wv" else 1)
            assert spans[-1][1] <= size and all(lo % (2 * eb) == 0 for lo, _ in spans), a
            total += size
        assert total == S32.vector_bytes(nsys, vlen, mvec, storage)
    r20 = S32.vector_bytes(7, 16384, 20, S32.STORE_F32) / S32.vector_bytes(7, 16384, 20, S32.STORE_F64)
    r10 = S32.vector_bytes(7, 16384, 10, S32.STORE_F32) / S32.vector_bytes(7, 16384, 10, S32.STORE_F64)
    assert abs(r20 - 92 / 168) < 1e-15 and abs(r10 - 52 / 88) < 1e-15          # 0.55 and 0.59 of the header


def test_the_large_case_crosses_what_it_is_there_for():
    import batch_large as G
    sh = S32.LARGE
    assert (sh.vlen, sh.mvec, sh.nsys) == (16384, 32, 3976)
    elems = G.sys_stride(sh) * sh.nsys
    assert elems > 2 ** 31 and 4 * elems > 2 ** 32                             # one float allocation: elements and bytes
    act, wit = S32.large_active(), S32.large_witnesses()
    assert 7 <= len(act) <= 9 and act[0] == 0 and act[-1] == sh.nsys - 1 and wit and not set(act) & set(wit)
    for B in (G.ELEMS_2G, S32.BYTES_4G_FLOATS):
        k = G.on_boundary(sh, "w", B)
        assert k in act and G.straddles(sh, "w", B, k)
        assert any(G.extent(sh, "w", j)[1] <= B for j in act if abs(j - k) <= G.NEAR)
        assert any(G.extent(sh, "w", j)[0] >= B for j in act if abs(j - k) <= G.NEAR)
    assert S32.large_bytes() < 19 * 2 ** 30


# ---- 2: convergence on the host model --------------------------------------------------------------------------------------

def test_the_host_model_retires_every_system_inside_the_budget(oracle):
    """batch_step.solve_problem() through the host model of the contract, flavour C, mvec = 6, relative tolerance SOLVE_TOL: every
    system retires within SOLVE_REPLAYS - SOLVE_SLACK steps -- the budget tests/test_batch_store32_gpu.py holds the device to.
    The binary64 model runs beside it; both sets of iterations go to the dump directory.  Measured with np.dot sums: the last
    system retires at iteration 32 with either storage."""
    import parity_util as P
    it32 = S32.solve_on_the_model(oracle, True, T.SOLVE_MVEC, T.SOLVE_TOL)
    it64 = S32.solve_on_the_model(oracle, False, T.SOLVE_MVEC, T.SOLVE_TOL)
    out = P.dump_dir(ROOT)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_store32_model_solve.json"), "w") as fh:
            json.dump({"binary32": [int(v) for v in it32], "binary64": [int(v) for v in it64], "tol": T.SOLVE_TOL,
                       "mvec": T.SOLVE_MVEC}, fh, indent=1, sort_keys=True)
    budget = T.SOLVE_REPLAYS - T.SOLVE_SLACK
    assert (it64 >= 0).all() and it64.max() <= budget, it64
    assert (it32 >= 0).all() and it32.max() <= budget, it32


# ---- 3: sentinels ----------------------------------------------------------------------------------------------------------

def _operands(n, seed):
    """x: a normalised difference before q() (|x| <= 1); y: a stored older vector (already binary32).  At every sentinel of the
    batch kernel x is 2^-e (1 + 3 * 2^-25), e in 1..3: halfway between two binary32 neighbours plus a quarter of their distance, so
    q(x) rounds UP by 2^-e 2^-25 (to 1 + 2^-23), truncation rounds DOWN by 3 * 2^-e 2^-25 (to 1), and keeping x unrounded is off by
    the former -- each at least 2^-28 |x| against a bound of about 2^-48 sum|xy|; y is +-1/2 there so the product is large."""
    rng = np.random.default_rng([3232, n, seed])
    x = rng.standard_normal(n) * 0.01
    y = S32.q(rng.standard_normal(n) * 0.01)
    idx = X.batch_all_sentinels(n)
    x[idx] = np.ldexp(1.0 + 3.0 * 2.0 ** -25, -rng.integers(1, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    y[idx] = 0.5 * rng.choice([-1.0, 1.0], idx.size)
    return x, y, idx


@pytest.mark.parametrize("n", [65, 513, 4099])
def test_an_operand_not_rounded_as_the_contract_says_breaks_the_bound(n):
    """The exact-sum layer of the GPU test holds red[2 + p] to gamma(batch_k(n)) sum|xy| of exact_dot(q(x), w_p).  On the host
    model of the kernel's sum (batch_weights.thread_sums with unit weights / workgroup_sum): the sum of the contract's operands
    is inside that bound; with ONE planted sentinel taken unrounded, or rounded by truncation, it is outside -- at every
    sentinel.  So the bound alone detects both mistakes at these shapes; the bit-for-bit layer holds them as well."""
    x, y, idx = _operands(n, 0)
    one = np.ones(n)
    xq = S32.q(x)
    assert (xq[idx] != x[idx]).all() and (S32.q_trunc(x)[idx] != xq[idx]).all()
    bound, tot, exact = X.gamma(X.batch_k(n)), X.abs_dot(xq, y), X.exact_dot(xq, y)
    base = BW.thread_sums(one, xq, y)
    assert abs(BW.workgroup_sum(base) - exact) <= bound * tot                    # the contract's sum: inside
    for what, wrong in (("unrounded", x), ("truncated", S32.q_trunc(x))):
        for i in idx:
            mut = xq.copy()
            mut[i] = wrong[i]
            term = (mut[i] - xq[i]) * y[i]
            assert X.detectable(term, bound, tot), (what, n, int(i), term, bound * tot)
            got = BW.workgroup_sum(BW.thread_sums(one, mut, y, base=base, only=BW.owner(int(i))))
            assert abs(got - exact) > bound * tot, (what, n, int(i), "the bound did not notice")
