"""The wave batch with per-system lengths and diagonal dot weights (nka_hip_batch_create_waves_ext; include/nka_hip_batch.h,
WAVES EXT; nka_amd/csrc/nka_batch_waves.hip) as far as the host can restate it: the shapes of
tests/test_batch_waves_ext_gpu.py, the weights, the call plan of the twin tests, the large shape, and the ragged weighted solve
with its budget.  No GPU here: tests/test_batch_waves_ext_cpu.py holds all of it."""
import numpy as np

import batch_step as S
import batch_waves as BWV

# ---- lengths against twins ------------------------------------------------------------------------------------------------------
VLEN = 385                      # three tiles and a pair
LENS = (1, 2, 3, 127, 128, 129, 255, 257, 385)
NSYS = len(LENS)                # 9: the last workgroup has one absent wavefront
MVECS = (1, 3, 10)
TAIL_WEIGHT = 2.0 ** 500        # what a weight row holds from the system's length on (weights must be finite)
UNIT_LENGTHS = (1, 3, 127, 128, 129, 257, 899)
EXACT_LENGTHS = (1, 3, 129, 257, 899)
CPU_LENGTHS = (129, 257, 1027)

# the call plan of the twin tests: what happens before call t, and what call t is.  System k joins at call k % 3.
#   kind: "update" | "repeat" (the previous input again: s == 0) | "step" (x and fnorm) | "step-tol" (x, tol and fnorm)
PLAN = (("update", None), ("update", None), ("update", None), ("repeat", None), ("update", ("relax", (0, 3, 6))), ("step", None),
        ("step-tol", ("restart", (1, 4, 7))), ("step-tol", None), ("update", None), ("step-tol", None))
RETIRE = (2, 5)                 # the systems whose threshold (+inf) retires them at the first step with tol; the others' is 0
CALLS = len(PLAN)


def delay(k):
    return k % 3


def tile_cases(lens=LENS):
    """-> {case: lengths}: an empty, a partial and a full last tile; the half pair of an odd length."""
    return {"no ragged tile": [n for n in lens if n % BWV.TILE == 0],
            "ragged tile": [n for n in lens if n % BWV.TILE],
            "a full tile before the ragged one": [n for n in lens if n > BWV.TILE and n % BWV.TILE],
            "half pair": [n for n in lens if n % 2],
            "whole pairs": [n for n in lens if n % 2 == 0]}


# ---- weights --------------------------------------------------------------------------------------------------------------------

def draw_weights(n, rng):
    """General weights of one system: 2^U(-3, 3) -- no powers of two -- with 10 % zeros; at every sentinel of the wave sum
    (batch_waves.all_sentinels) NONZERO, at least a factor 2 from 1 and different from the pair partner's, so that a sum which
    dropped the weight there, or took the partner's, is off by at least half a sentinel product."""
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0
    idx = BWV.all_sentinels(n)
    w[idx] = np.exp2(rng.uniform(1.0, 3.0, idx.size) * rng.choice([-1.0, 1.0], idx.size))
    for i in idx.tolist():
        j = i ^ 1
        if j < n and w[i] == w[j]:
            w[j] = w[j] * 1.5 if w[j] else 3.0
    assert_weight_rule(n, w)
    return w


def assert_weight_rule(n, w):
    idx = BWV.all_sentinels(n)
    assert (w >= 0).all() and np.isfinite(w).all()
    assert ((w[idx] >= 2.0) | ((w[idx] > 0.0) & (w[idx] <= 0.5))).all()
    partner = idx ^ 1
    ok = partner < n
    assert (w[idx[ok]] != w[partner[ok]]).all()


def system_weights(n, nsys, seed=77):
    return np.stack([draw_weights(n, np.random.default_rng([seed, n, k])) for k in range(nsys)])


def weight_rows(lens, vlen, seed):
    """nsys x vlen: draw_weights of the system's own length below L, 2^500 from there on."""
    w = np.full((len(lens), vlen), TAIL_WEIGHT)
    for k, L in enumerate(lens):
        w[k, :L] = draw_weights(L, np.random.default_rng([seed, L, k]))
    return w


# ---- the large case: weight buffer, caller's weight rows and F each pass 2^32 bytes --------------------------------------------------

BYTES_4G = 2 ** 32
MAX_ACTIVE = 9


def large_shape():
    """vlen = 1024 (the slot stride is 1024 too), mvec = 1, ld = ldw = 1024: a row of F, of the caller's weights and of the batch's
    weight buffer is 8192 bytes, so row 2^19 = 524 288 starts on byte 2^32 of each; nsys = 2^19 + 3.  The slots (two per system and
    allocation) pass 2^32 bytes at system 2^18.  The systems that run: the first, the last, both sides of either boundary; the
    witnesses: where a byte offset that lost its upper half would land, and the neighbours."""
    vlen, mvec = 1024, 1
    row = 8 * BWV.slot_stride(vlen)
    kb = BYTES_4G // row
    ks = BYTES_4G // (row * (mvec + 1))
    nsys = kb + 3
    active = sorted({0, ks - 1, ks, kb - 1, kb, kb + 1, nsys - 1})
    lens = {0: 1, ks - 1: 1023, ks: 129, kb - 1: 1024, kb: 899, kb + 1: 257, nsys - 1: 3}
    wit = set()
    for k in active:
        wit |= {(k * row) % BYTES_4G // row, (k * row * (mvec + 1)) % BYTES_4G // (row * (mvec + 1)), k - 1, k + 1}
    wit = sorted(j for j in wit if 0 <= j < nsys and j not in active)
    return {"nsys": nsys, "vlen": vlen, "mvec": mvec, "row_bytes": row, "boundary": kb, "slot_boundary": ks, "active": active,
            "lens": lens, "witnesses": wit}


def large_bytes(sh):
    """{name: bytes} of every device allocation the large case holds at once."""
    base = BWV.large_bytes({"mvec": sh["mvec"], "vlen": sh["vlen"], "nsys": sh["nsys"],
                            "sys_bytes": sh["row_bytes"] * (sh["mvec"] + 1)})
    rows = sh["row_bytes"] * sh["nsys"]
    base.update({"X": rows, "weight buffer": rows, "caller's weights": rows, "len": 4 * sh["nsys"], "tol, fnorm": 16 * sh["nsys"]})
    return base


# ---- a whole solve: ragged, weighted ----------------------------------------------------------------------------------------------
# The problem of tests/batch_step.py -- its d, eps, b and x0 -- with system k of length solve_lengths()[k] and weights of its own:
# inside [0, L) the tridiagonal part of that operator (the corner couplings would reach across L), so a system's residual below L
# depends on its elements below L alone.  The stop rule is the batch's: the WEIGHTED norm, relative to the first one.

SOLVE_REPLAYS = 40              # the budget of the GPU test; the CPU test holds the oracle to SOLVE_SLACK steps inside it
SOLVE_SLACK = 8


def solve_lengths():
    rng = np.random.default_rng(2025)
    lens = rng.integers(S.SOLVE_VLEN // 4, S.SOLVE_VLEN + 1, S.SOLVE_NSYS)
    lens[:4] = (S.SOLVE_VLEN, S.SOLVE_VLEN // 4, 65, 64)
    return lens.astype(np.int32)


def solve_weights():
    """nsys x vlen, 2^U(-1, 1) below the length (positive: the weighted norm is a norm), TAIL_WEIGHT from there on."""
    lens = solve_lengths()
    w = np.full((S.SOLVE_NSYS, S.SOLVE_VLEN), TAIL_WEIGHT)
    for k, L in enumerate(lens):
        w[k, :L] = np.exp2(np.random.default_rng([2026, k]).uniform(-1.0, 1.0, L))
    return w


def solve_couplings():
    """-> (left, right), nsys x vlen of 0 / 1: element i of system k takes x[i - 1] where left is 1 (0 < i < L) and x[i + 1] where
    right is 1 (i < L - 1)."""
    lens = solve_lengths()
    i = np.arange(S.SOLVE_VLEN)[None, :]
    left = ((i > 0) & (i < lens[:, None])).astype(np.float64)
    right = (i < lens[:, None] - 1).astype(np.float64)
    return left, right


def solve_residual(xp, x, d, eps, b, left, right):
    """Elementwise operations only, the same statements for numpy and torch (`xp`): no BLAS inside a capture."""
    return (d * x + eps * (left * xp.roll(x, 1, 1) + right * xp.roll(x, -1, 1)) - b) / d


def solve_on_the_oracle(oracle):
    """batch_step.solve_on_the_oracle on the ragged weighted problem: one oracle of length L per system with the weighted dot
    product -> the iteration at which each system retired, -1 where it did not within SOLVE_REPLAYS calls."""
    d, eps, b, x = S.solve_problem()
    lens, w = solve_lengths(), solve_weights()
    left, right = solve_couplings()
    accs = []
    for k, L in enumerate(lens):
        a = oracle.OracleNKA(int(L), S.SOLVE_MVEC, S.SOLVE_FLAVOR)
        a.set_dot_prod(lambda p, q, wk=w[k, :L].copy(): float(np.dot(wk * p, q)))
        accs.append(a)
    retired = np.full(S.SOLVE_NSYS, -1)
    tol = np.zeros(S.SOLVE_NSYS)
    for it in range(SOLVE_REPLAYS):
        f = solve_residual(np, x, d, eps, b, left, right)
        r = np.array([np.sqrt(np.dot(w[k, :L] * f[k, :L], f[k, :L])) for k, L in enumerate(lens)])
        if it == 1:
            tol = S.SOLVE_TOL * r0
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
