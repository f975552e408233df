"""Weights for the tests of the batched accelerator's diagonal dot-product weights (nka_hip_batch_set_dot_weights), and the
kernel's weighted fast sum restated on the host (no GPU): shared by tests/test_batch_weights_gpu.py and
tests/test_batch_weights_cpu.py."""
from fractions import Fraction

import numpy as np

import exact_sums as X

WEIGHT_SEED = 77


def draw_weights(n, rng):
    """General weights of one system: 2^U(-3, 3) -- not powers of two -- with 10 % zeros.  At every index where the kernel
    changes hands (exact_sums.batch_sentinel_indices) the weight is NONZERO and differs from 1 by at least a factor 2
    (2^+-U(1, 3)), and from its pair partner's: a sum that dropped the weight there, or took the partner's, is off by at least
    half a sentinel product -- far outside the bound."""
    w = np.exp2(rng.uniform(-3.0, 3.0, n))
    w[rng.random(n) < 0.1] = 0.0
    idx = X.batch_all_sentinels(n)
    w[idx] = np.exp2(rng.uniform(1.0, 3.0, idx.size) * rng.choice([-1.0, 1.0], idx.size))
    assert_weight_rule(n, w)
    return w


def assert_weight_rule(n, w):
    idx = X.batch_all_sentinels(n)
    assert (w >= 0).all() and np.isfinite(w).all()
    assert ((w[idx] >= 2.0) | ((w[idx] > 0.0) & (w[idx] <= 0.5))).all()
    partner = idx ^ 1
    ok = partner < n
    assert (w[idx[ok]] != w[partner[ok]]).all()


def system_weights(n, nsys):
    """The weights test 4 of tests/test_batch_weights_gpu.py sets: one draw per system."""
    return np.stack([draw_weights(n, np.random.default_rng([WEIGHT_SEED, n, k])) for k in range(nsys)])


def fma(a, b, c):
    """a*b + c rounded once (Fraction -> float rounds correctly)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def thread_sums(w, x, y, wy=None, base=None, only=None):
    """The 256 per-thread accumulators of one weighted fast sum of k_batch_update<*, false, true>: thread t owns the pairs 2t,
    2t + 1 of every tile of 512 and meets them in increasing order, acc = fma(fl(w_i x_i), y_i, acc).  `wy`: the weight each
    element's product takes, where a mutation makes that another one than w.  `base`, `only`: the accumulators of an earlier
    call and the one thread to form again (a mutation of one element changes one thread's chain)."""
    n = x.size
    a = (w if wy is None else wy) * x                                # fl(w x): rounded once, before the product
    acc = np.zeros(X.BATCH_THREADS) if base is None else base.copy()
    for t in (range(min(X.BATCH_THREADS, (n + 1) // 2)) if only is None else [only]):
        s = 0.0
        for b0 in range(0, n, X.BATCH_TILE):
            for q in range(2):
                i = b0 + 2 * t + q
                if i < n:
                    s = fma(a[i], y[i], s)
        acc[t] = s
    return acc


def workgroup_sum(acc):
    """batch_block_sum: a butterfly over each wavefront (lane i + lane i + 32, 16, 8, 4, 2, 1), then wavefronts 0, 1, 2, 3 in
    turn."""
    waves = []
    for wv in range(X.WAVES):
        v = acc[wv * X.WAVE:(wv + 1) * X.WAVE].copy()
        while v.size > 1:
            v = v[: v.size // 2] + v[v.size // 2:]
        waves.append(v[0])
    r = waves[0]
    for v in waves[1:]:
        r = r + v
    return float(r)


def owner(i):
    """The thread that owns element i."""
    return (i % X.BATCH_TILE) // 2
