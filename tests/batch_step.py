"""Shared by tests/test_batch_step_gpu.py and tests/test_batch_step_cpu.py (the solve step of the batched accelerator,
nka_hip_batch_accel_step): the bound on the step's residual norm, and the small solve both files run -- on the GPU through
the library, on the CPU through the oracle -- with its seeds, its residual and its budget fixed HERE, without a GPU."""
import math

import numpy as np

import exact_sums as X


# ---- the norm: r = sqrt(dp(f, f)) ------------------------------------------------------------------------------------------

def norm_bound(n):
    """|fnorm - sqrt(E)| <= norm_bound(n) * sqrt(E), E = exact_dot(a, f), a = f or fl(w o f), for the fast sums.  Every term of
    the sum is >= 0, so the sum carries at most gamma(K) RELATIVE error with the K of every other sum of the kernel
    (exact_sums.batch_k; gamma adds exact_dot's own rounding); a square root halves a relative error upwards and at most keeps
    it downwards; then one rounding each for the device's sqrt, the host's sqrt and exact_dot's final rounding."""
    return X.gamma(X.batch_k(n)) + 4.0 * X.U


def norm_inside(got, a, f, n):
    want = math.sqrt(X.exact_dot(a, f))
    return abs(got - want) <= norm_bound(n) * want, (abs(got - want) / (X.U * want) if want else 0.0)


# ---- the solve of GPU test 4 / CPU test 7 ---------------------------------------------------------------------------------
# nsys tridiagonal-plus-corners systems  d o x + eps (roll(x, 1) + roll(x, -1)) = b, Jacobi-preconditioned residual
# f = (d o x + eps (roll(x, 1) + roll(x, -1)) - b) / d, iterate x <- x - accel(f).  d in [1, 2) and eps in [0.02, 0.48] are
# drawn per system, so the contraction of the plain iteration (at most 2 eps / min d) runs from 0.04 to 0.96: the systems
# need very different numbers of steps.

SOLVE_NSYS, SOLVE_VLEN, SOLVE_MVEC, SOLVE_FLAVOR = 64, 96, 6, 0
SOLVE_TOL = 1.0e-9          # relative: a system retires at ||f|| <= SOLVE_TOL * ||f_0||
SOLVE_REPLAYS = 40          # the budget: test 7 shows the oracle retires every system at least SOLVE_SLACK steps before it
SOLVE_SLACK = 8
SOLVE_GUARD = 1.0e-10       # no norm of the eager twin may lie this close (relatively) to its threshold: see test 4


def solve_problem():
    """-> d, eps, b, x0: float64 arrays (nsys x vlen; eps: nsys x 1), seeded per system."""
    d = np.empty((SOLVE_NSYS, SOLVE_VLEN))
    b = np.empty_like(d)
    eps = np.empty((SOLVE_NSYS, 1))
    for k in range(SOLVE_NSYS):
        rng = np.random.default_rng([2024, k])
        d[k] = 1.0 + rng.random(SOLVE_VLEN)
        b[k] = rng.standard_normal(SOLVE_VLEN)
        eps[k, 0] = 0.02 + 0.46 * k / (SOLVE_NSYS - 1)
    return d, eps, b, np.zeros_like(d)


def solve_residual(xp, x, d, eps, b):
    """Elementwise operations only, the same statements for numpy and torch (`xp`): no BLAS inside a capture."""
    return (d * x + eps * (xp.roll(x, 1, 1) + xp.roll(x, -1, 1)) - b) / d


def solve_on_the_oracle(oracle):
    """The loop of nka_example.F90:243-254 per system, with the stop rule of nka_hip_batch_accel_step (<=, relative to the
    first norm) -> the iteration (0-based count of steps taken) at which each system retired, -1 where it did not within
    SOLVE_REPLAYS calls."""
    d, eps, b, x = solve_problem()
    accs = [oracle.OracleNKA(SOLVE_VLEN, SOLVE_MVEC, SOLVE_FLAVOR) for _ in range(SOLVE_NSYS)]
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
