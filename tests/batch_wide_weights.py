"""Shared by tests/test_batch_wide_weights_gpu.py and tests/test_batch_wide_weights_cpu.py (the wide batch with diagonal dot
weights, nka_hip_batch_create_wide_ext): weights that obey the rule of batch_weights at every place where the wide kernels change
hands, the shapes of the GPU tests, the large shape, and the ragged weighted solve both files run -- on the GPU through the
library, on the CPU through the oracle -- fixed HERE, without a GPU.

A weighted wide sum is the wide sum (tests/batch_wide.py) of fl(w o x) and y: the first operand is rounded once, before the
product, so K = batch_wide.wide_k(n) does not change."""
import numpy as np

import batch_weights as BWT
import batch_wide as BW
import batch_wide_step as WS

WEIGHT_SEED = 79
TAIL_WEIGHT = 2.0 ** 500        # what a weight row holds from the system's length on (weights must be finite)


# ---- weights ------------------------------------------------------------------------------------------------------------------------

def draw_weights(n, rng, C):
    """General weights of one wide system: batch_weights.draw_weights -- 2^U(-3, 3) with 10 % zeros -- with the rule of that file
    at the sentinels of EVERY chunk and at both ends of every chunk (batch_wide.wide_sentinel_indices): nonzero, at least a factor
    2 from 1, and different from the pair partner's."""
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0
    idx = BW.wide_sentinel_indices(n, C)
    w[idx] = np.exp2(rng.uniform(1.0, 3.0, idx.size) * rng.choice([-1.0, 1.0], idx.size))
    assert_weight_rule(n, w, C)
    return w


def assert_weight_rule(n, w, C):
    """batch_weights.assert_weight_rule on every chunk (a chunk starts on an even index, so a pair never spans two), and at the two
    ends of every chunk."""
    for lo in range(0, n, C):
        BWT.assert_weight_rule(min(C, n - lo), w[lo:lo + C])
    idx = BW.wide_sentinel_indices(n, C)
    assert ((w[idx] >= 2.0) | ((w[idx] > 0.0) & (w[idx] <= 0.5))).all()
    partner = idx ^ 1
    ok = partner < n
    assert (w[idx[ok]] != w[partner[ok]]).all()


def system_weights(n, nsys, C, seed=WEIGHT_SEED):
    return np.stack([draw_weights(n, np.random.default_rng([seed, n, k]), C) for k in range(nsys)])


# ---- shapes -------------------------------------------------------------------------------------------------------------------------

def shape(which, C):
    """n of a shape given in units of the chunk."""
    return {"1": 1, "2": 2, "65": 65, "513": 513, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+513": 2 * C + 513, "8C+1": 8 * C + 1,
            "9C+1": 9 * C + 1, "16C+1": 16 * C + 1, "256C+1": 256 * C + 1}[which]


EXACT_SHAPES = ("C+1", "2C+513", "8C+1", "9C+1", "16C+1")      # 2, 3, 9, 10 and 17 chunks; 257 once
EXACT_CHUNKS = {"C+1": 2, "2C+513": 3, "8C+1": 9, "9C+1": 10, "16C+1": 17, "256C+1": 257}
CPU_CHUNKS = {"8C+1": 9, "9C+1": 10, "16C+1": 17}


# ---- the large case -----------------------------------------------------------------------------------------------------------------

BYTES_4G = 2 ** 32
MAX_ACTIVE = 9
MAX_BYTES = 36 * 2 ** 30


def slot_stride(vlen):
    return (vlen + 31) // 32 * 32


def large_shape(C, cap):
    """520 systems of cap - 32 elements, mvec = 1: the slot stride -- the row stride of the batch's weight buffer -- is cap - 32
    doubles and the caller's weight rows and the rows of F lie ldw = ld = cap - 31 apart, so byte 2^32 of each falls INSIDE row 512.
    The systems that run: the first, the last, row 512 and its two neighbours; the witnesses: where a byte offset that lost its
    upper half would land, and the inactive neighbours."""
    vlen, mvec, nsys = cap - 32, 1, 520
    stride, ld = slot_stride(vlen), vlen + 1
    kb = BYTES_4G // (8 * stride)
    active = sorted({0, kb - 1, kb, kb + 1, nsys - 1})
    wit = set()
    for k in active:
        for step in (stride, ld, stride * (mvec + 1)):
            wit.add((8 * k * step) % BYTES_4G // (8 * step))
        wit |= {k - 1, k + 1}
    wit = sorted(j for j in wit if 0 <= j < nsys and j not in active)
    lens = {0: vlen, kb - 1: vlen - 1, kb: vlen, kb + 1: 2 * C + 513, nsys - 1: C + 1}
    return {"nsys": nsys, "vlen": vlen, "mvec": mvec, "stride": stride, "ld": ld, "boundary": kb, "active": active, "witnesses": wit,
            "lens": lens}


def large_bytes(sh):
    """{name: bytes} of every device allocation the large case holds at once (the twin of five systems is left out)."""
    nsys, stride, ld, m1 = sh["nsys"], sh["stride"], sh["ld"], sh["mvec"] + 1
    chunks = -(-sh["vlen"] // 2048)
    return {"w": 8 * stride * m1 * nsys, "v": 8 * stride * m1 * nsys, "weight buffer": 8 * stride * nsys,
            "caller's weights": 8 * ld * nsys, "F": 8 * ld * nsys, "part": 8 * nsys * (2 + 2 * sh["mvec"]) * chunks,
            "control": 4096 * nsys}


# ---- a whole solve: ragged, weighted, wide --------------------------------------------------------------------------------------------
# batch_wide_step's systems d o x + eps (left o roll(x, 1) + right o roll(x, -1)) = b with the Jacobi-preconditioned residual: 16 of
# them in a batch of vlen = 3C, system k of length solve_lengths(C)[k] in [C / 2, 3C] with the tridiagonal part of the operator
# inside [0, L).  The weights: zero on every 17th entry (a masked entry: it stays out of every inner product and of the norm),
# 4^k, k in [-3, 3], elsewhere, TAIL_WEIGHT from the length on.  The stop rule is the batch's: the WEIGHTED norm, relative to the
# first one.

SOLVE_NSYS, SOLVE_MVEC, SOLVE_FLAVOR = 16, WS.SOLVE_MVEC, WS.SOLVE_FLAVOR
SOLVE_TOL, SOLVE_SLACK = WS.SOLVE_TOL, 8
SOLVE_REPLAYS = 40              # the budget of the GPU test; the CPU test holds the oracle to SOLVE_SLACK steps inside it


def solve_vlen(C):
    return 3 * C


def solve_lengths(C):
    rng = np.random.default_rng(2027)
    lens = rng.integers(C // 2, 3 * C + 1, SOLVE_NSYS)
    lens[:5] = (3 * C, C // 2, C, C + 1, 2 * C + 513)
    return lens.astype(np.int32)


def solve_weights(C):
    n, lens = solve_vlen(C), solve_lengths(C)
    w = np.full((SOLVE_NSYS, n), TAIL_WEIGHT)
    for k, L in enumerate(lens):
        w[k, :L] = np.ldexp(1.0, 2 * np.random.default_rng([2028, k]).integers(-3, 4, L))
        w[k, k % 17:L:17] = 0.0
    return w


def solve_problem(C):
    """-> d, eps, b, x0, left, right: float64 arrays (nsys x vlen; eps: nsys x 1), seeded per system."""
    n, lens = solve_vlen(C), solve_lengths(C)
    d = np.empty((SOLVE_NSYS, n))
    b = np.empty_like(d)
    eps = np.empty((SOLVE_NSYS, 1))
    for k in range(SOLVE_NSYS):
        rng = np.random.default_rng([2029, k])
        d[k] = 1.0 + rng.random(n)
        b[k] = rng.standard_normal(n)
        eps[k, 0] = 0.02 + 0.38 * k / (SOLVE_NSYS - 1)
    i = np.arange(n)[None, :]
    left = ((i > 0) & (i < lens[:, None])).astype(np.float64)
    right = (i < lens[:, None] - 1).astype(np.float64)
    return d, eps, b, np.zeros_like(d), left, right


def solve_residual(xp, x, d, eps, b, left, right):
    """Elementwise operations only, the same statements for numpy and torch (`xp`): no BLAS inside a capture."""
    return (d * x + eps * (left * xp.roll(x, 1, 1) + right * xp.roll(x, -1, 1)) - b) / d


def solve_on_the_oracle(oracle, C):
    """batch_wide_step.solve_on_the_oracle on the ragged weighted problem: one oracle of length L per system with the weighted dot
    product -> the iteration at which each system retired, -1 where it did not within SOLVE_REPLAYS calls."""
    d, eps, b, x, left, right = solve_problem(C)
    lens, w = solve_lengths(C), solve_weights(C)
    accs = []
    for k, L in enumerate(lens):
        a = oracle.OracleNKA(int(L), SOLVE_MVEC, SOLVE_FLAVOR)
        a.set_dot_prod(lambda p, q, wk=w[k, :L].copy(): float(np.dot(wk * p, q)))
        accs.append(a)
    retired = np.full(SOLVE_NSYS, -1)
    tol = np.zeros(SOLVE_NSYS)
    for it in range(SOLVE_REPLAYS):
        f = solve_residual(np, x, d, eps, b, left, right)
        r = np.array([np.sqrt(np.dot(w[k, :L] * f[k, :L], f[k, :L])) for k, L in enumerate(lens)])
        if it == 1:
            tol = SOLVE_TOL * r0
        for k, L in enumerate(lens):
            if retired[k] >= 0:
                continue
            if r[k] <= tol[k]:
                retired[k] = it
                continue
            fk = f[k, :L].copy()
            accs[k].accel_update(fk)
            x[k, :L] = x[k, :L] - fk
        if it == 0:
            r0 = r
    return retired
