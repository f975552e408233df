"""Shared by tests/test_batch_wide_step_gpu.py and tests/test_batch_wide_step_cpu.py (the solve step of a wide batch,
nka_hip_batch_create_wide_step): the bound on the step's residual norm, the inputs the GPU test holds to it, and the small
solve both files run -- on the GPU through the library, on the CPU through the oracle -- fixed HERE, without a GPU."""
import math

import numpy as np

import batch_step as S
import batch_wide as BW
import exact_sums as X


# ---- the norm: r = sqrt(sum_c q_c) ------------------------------------------------------------------------------------------

def norm_bound(n, C):
    """|fnorm - sqrt(E)| <= norm_bound * sqrt(E), E = exact_dot(f, f): the derivation of batch_step.norm_bound with the K of a
    wide sum (batch_wide.wide_k: the chain of a chunk, the workgroup's reduction, the chunk-order chain).  Every term is >= 0,
    so the sum carries at most gamma(K) RELATIVE error; the square root halves a relative error upwards and at most keeps it
    downwards; one rounding each for the device's sqrt, the host's sqrt and exact_dot's final rounding."""
    return X.gamma(BW.wide_k(n, C)) + 4.0 * X.U


def norm_inside(got, f, n, C, exact=None):
    want = math.sqrt(X.exact_dot(f, f) if exact is None else exact)
    return abs(got - want) <= norm_bound(n, C) * want, (abs(got - want) / (X.U * want) if want else 0.0)


EXACT_NSYS = 2


def exact_shapes(C):
    """The shapes of GPU test 4: 2, 3, 10, 17 and 257 chunks."""
    return [C + 1, 2 * C + 513, 9 * C + 1, 16 * C + 1, 256 * C + 1]


def exact_inputs(n, C):
    """The rows of GPU test 4 at length n, from batch_wide.wide_planted_input (sentinels), seeded per shape and system."""
    return [BW.wide_planted_input(n, np.random.default_rng([44, n, k]), C=C) for k in range(EXACT_NSYS)]


# ---- the solve of GPU test 7 ------------------------------------------------------------------------------------------------
# batch_step's systems d o x + eps (roll(x, 1) + roll(x, -1)) = b with the Jacobi-preconditioned residual, 5 of them at 2C + 513
# unknowns; eps runs from 0.02 to 0.40, so the systems need different numbers of steps.

SOLVE_NSYS, SOLVE_MVEC, SOLVE_FLAVOR = 5, 6, 0
SOLVE_TOL, SOLVE_REPLAYS, SOLVE_SLACK, SOLVE_GUARD = S.SOLVE_TOL, 40, 8, S.SOLVE_GUARD
solve_residual = S.solve_residual


def solve_vlen(C):
    return 2 * C + 513


def solve_problem(C):
    """-> d, eps, b, x0: float64 arrays (nsys x vlen; eps: nsys x 1), seeded per system."""
    n = solve_vlen(C)
    d = np.empty((SOLVE_NSYS, n))
    b = np.empty_like(d)
    eps = np.empty((SOLVE_NSYS, 1))
    for k in range(SOLVE_NSYS):
        rng = np.random.default_rng([2025, k])
        d[k] = 1.0 + rng.random(n)
        b[k] = rng.standard_normal(n)
        eps[k, 0] = 0.02 + 0.38 * k / (SOLVE_NSYS - 1)
    return d, eps, b, np.zeros_like(d)


def solve_on_the_oracle(oracle, C):
    """batch_step.solve_on_the_oracle on the problem above -> the iteration at which each system retired, -1 where it did not
    within SOLVE_REPLAYS calls."""
    d, eps, b, x = solve_problem(C)
    n = solve_vlen(C)
    accs = [oracle.OracleNKA(n, SOLVE_MVEC, SOLVE_FLAVOR) for _ in range(SOLVE_NSYS)]
    retired = np.full(SOLVE_NSYS, -1)
    tol = np.zeros(SOLVE_NSYS)
    for it in range(SOLVE_REPLAYS):
        f = solve_residual(np, x, d, eps, b)
        r = np.sqrt((f * f).sum(axis=1))
        if it == 1:
            tol = SOLVE_TOL * r0
        for k in range(SOLVE_NSYS):
            if retired[k] >= 0:
                continue
            if r[k] <= tol[k]:
                retired[k] = it
                continue
            fk = f[k].copy()
            accs[k].accel_update(fk)
            x[k] = x[k] - fk
        if it == 0:
            r0 = r
    return retired
