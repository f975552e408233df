"""The exact-sum reference of tests/test_sums_exact_gpu.py, held to Fraction arithmetic, and the proof that its planted
inputs make the GPU checks sensitive: at every boundary shape, losing or doubling any one sentinel's product breaks the
error bound.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_sums as X

# CU counts the sentinels are laid out for: an MI355X (256) and a smaller device, so that the layout is not tuned to one
GRIDS = (256, 80)


def fraction_dot(x, y):
    """sum x_i*y_i in rational arithmetic, rounded once (Fraction -> float rounds correctly)."""
    return float(sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y)), Fraction(0)))


@pytest.mark.parametrize("seed", range(6))
def test_exact_dot_is_the_correctly_rounded_sum(seed):
    rng = np.random.default_rng(seed)
    for n in (0, 1, 2, 3, 17, 256, 2000):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        assert X.exact_dot(x, y) == fraction_dot(x, y), n
        p, e = X.two_prod(x, y)
        assert all(Fraction(float(a)) * Fraction(float(b)) == Fraction(float(pp)) + Fraction(float(ee))
                   for a, b, pp, ee in zip(x[:50], y[:50], p[:50], e[:50]))


@pytest.mark.parametrize("seed", range(6))
def test_exact_dot_on_cancelling_sums(seed):
    """Sums whose result is many orders of magnitude below their terms: every rounded intermediate is wrong there."""
    rng = np.random.default_rng(100 + seed)
    n = 1000
    x = rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)
    y = rng.standard_normal(n)
    x2 = np.concatenate([x, x])
    y2 = np.concatenate([y, -y])               # exactly zero ...
    assert X.exact_dot(x2, y2) == 0.0 == fraction_dot(x2, y2)
    y2[rng.integers(0, 2 * n)] *= 1.0 + 2.0 ** -50     # ... but for one product: a result ~1e-15 of the terms
    ex = fraction_dot(x2, y2)
    assert ex != 0.0 and X.exact_dot(x2, y2) == ex


@pytest.mark.parametrize("seed", range(6))
def test_exact_dot_on_wide_exponents(seed):
    rng = np.random.default_rng(200 + seed)
    n = 2000
    x = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-400, 400, n))
    y = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-400, 400, n))
    assert X.exact_dot(x, y) == fraction_dot(x, y)
    # odd significands (53 bits set low and high): the split halves both carry information
    x = (rng.integers(2 ** 52, 2 ** 53, n) | 1).astype(np.float64) * np.ldexp(1.0, rng.integers(-300, 300, n))
    y = -(rng.integers(2 ** 52, 2 ** 53, n) | 1).astype(np.float64) * np.ldexp(1.0, rng.integers(-300, 300, n))
    y[::2] *= -1.0
    assert X.exact_dot(x, y) == fraction_dot(x, y)


def test_exact_dot_range_and_non_finite():
    assert math.isnan(X.exact_dot([1.0, math.nan], [1.0, 1.0]))
    assert math.isnan(X.exact_dot([math.inf, 1.0], [0.0, 1.0]))           # Inf * 0
    assert math.isnan(X.exact_dot([math.inf, math.inf], [1.0, -1.0]))     # +Inf meets -Inf
    assert X.exact_dot([math.inf, 2.0], [-3.0, 1.0]) == -math.inf
    with pytest.raises(ValueError):
        X.exact_dot([2.0 ** 1000], [1.0])
    with pytest.raises(ValueError):
        X.exact_dot([2.0 ** -500], [2.0 ** -500])


def test_k_steps_follows_the_launch_geometry():
    # n = G * 512: every block one tile, two fma per thread; no tail
    assert X.k_steps(256 * 512, 256, 2) == 2 + 9 + (4 + 6)
    # the ragged tail of the last block adds ceil(tail / 256) fma
    assert X.k_steps(256 * 512 + 1, 256, 2) == 2 + 1 + 9 + 10
    assert X.k_steps(256 * 512 + 257, 256, 2) == 2 + 2 + 9 + 10
    # 9 tiles per block (the ahead loop + one plain tile), 77 in the tail
    assert X.k_steps(9 * 256 * 512 + 77, 256, 2) == 18 + 1 + 9 + 10
    # a single block: the final sums add one term per lane
    assert X.k_steps(7, 1, 2) == 1 + 9 + 1 + 6
    # the scalar path: tiles of 256, one fma per tile
    assert X.k_steps(3001, 256, 1) == 1 + 1 + 9 + 10
    # the grids: G never exceeds the tiles, and never the CU count (times 4 for k_dots<4, *>)
    assert X.pass_grids(1, 256, True) == [(1, 2)] * 5
    assert X.pass_grids(10 ** 6, 256, True) == [(256, 2), (256, 2), (512, 2), (768, 2), (1024, 2)]
    assert X.device_k(10 ** 6, 256) == max(X.k_steps(10 ** 6, G, 2) for G in (256, 512, 768, 1024))


def test_the_bound_holds_for_a_simulated_blocked_sum():
    """The device's summation order, restated on the host (fma replaced by a rounded product and a rounded sum, i.e.
    one rounding MORE per step than the device takes), stays within sum_bound on adversarial data."""
    rng = np.random.default_rng(3)
    G, n = 7, 7 * 512 * 3 + 300
    x = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 30, n))
    y = rng.standard_normal(n)
    prod = x * y
    ntile = n // 512
    acc = np.zeros((G, 256))
    for t in range(ntile):                                  # block t % G, thread j takes elements 2j, 2j + 1 of the tile
        b = t % G
        for q in range(2):
            acc[b] = acc[b] + prod[t * 512 + q: (t + 1) * 512: 2]
    for i in range(ntile * 512, n):
        acc[G - 1, (i - ntile * 512) % 256] += prod[i]
    partial = []
    for b in range(G):                                      # butterflies per wavefront, then waves in turn
        waves = []
        for w in range(4):
            v = acc[b, w * 64:(w + 1) * 64].copy()
            while v.size > 1:
                v = v[: v.size // 2] + v[v.size // 2:]
            waves.append(v[0])
        r = waves[0]
        for w in waves[1:]:
            r = r + w
        partial.append(r)
    lanes = [sum(partial[b] for b in range(l, G, 64)) for l in range(64)]
    v = np.array(lanes)
    while v.size > 1:
        v = v[: v.size // 2] + v[v.size // 2:]
    got, ex = float(v[0]), X.exact_dot(x, y)
    assert abs(got - ex) <= (X.sum_bound(n, G, 2) + X.U) * X.abs_dot(x, y)


def _pairs(n, G, rng):
    """The operands of every sum an update forms, built from planted inputs as the GPU tests build them: an older stored
    w (a normalised difference of two earlier inputs), the pending pair's raw w1, the input f; d = w1 - f and w1' = d/s."""
    f_a = X.planted_input(n, G, rng)
    f_b = X.planted_input(n, G, rng, prev=f_a)
    f_c = X.planted_input(n, G, rng, prev=f_b)
    f = X.planted_input(n, G, rng, prev=f_c)
    d_old = f_a - f_b
    w_old = d_old / math.sqrt(float(np.dot(d_old, d_old)))
    d = f_c - f                                                      # w1 = f_c, the raw previous input
    w1n = d / math.sqrt(float(np.dot(d, d)))
    return {"<d,d>": (d, d), "<f,d>": (f, d), "<f,w1'>": (f, w1n), "<d,w_p>": (d, w_old), "<w1',w_p>": (w1n, w_old),
            "<f,w_p>": (f, w_old), "<f,f_prev>": (f, f_c)}


@pytest.mark.parametrize("G", GRIDS)
def test_every_planted_sentinel_is_seen_by_the_bound(G):
    """THE sensitivity argument of tests/test_sums_exact_gpu.py, without a GPU: at every boundary shape and the PB ticket
    shape, for every sum an update forms, each sentinel's product exceeds twice the bound (plus the rounding of the exact
    sum), so a device sum that dropped it or counted it twice fails |red - exact| <= bound; for both alignments."""
    rng = np.random.default_rng(G)
    for n in X.boundary_shapes(G) + [X.pb_ticket_shape(G)]:
        sent = X.sentinel_indices(n, G)
        idx = X.all_sentinels(n, G)
        assert idx.size >= min(n, 2) and idx.min() >= 0 and idx.max() < n
        for name in ("ends", "tail_first", "block_first", "block_last", "plain_first", "tile_last"):
            assert np.isin(sent[name], idx).all()
        if n == 9 * G * 512 + 77:
            assert sent["plain_first"].size == G                     # every block hands over to its plain loop
        bound = max(X.gamma(X.device_k(n, G, True)), X.gamma(X.device_k(n, G, False)))
        for what, (x, y) in _pairs(n, G, rng).items():
            tot = X.abs_dot(x, y)
            terms = x[idx] * y[idx]
            worst = float(np.abs(terms).min())
            assert X.detectable(worst, bound, tot), (n, what, worst / tot, bound)


@pytest.mark.parametrize("G", GRIDS)
def test_dropping_or_doubling_a_sentinel_fails_the_check_end_to_end(G):
    """The same, the long way round at the shapes a reviewer can afford to sum exactly many times: perturb the data (one
    sentinel zeroed, or doubled), sum exactly, and hold the result to the check the GPU tests apply."""
    rng = np.random.default_rng(7 + G)
    for n in [s for s in X.boundary_shapes(G) if s <= G * 512 + 1]:
        bound = max(X.gamma(X.device_k(n, G, True)), X.gamma(X.device_k(n, G, False)))
        sent = X.sentinel_indices(n, G)
        picks = {int(v[0]) for v in sent.values() if v.size} | {int(v[-1]) for v in sent.values() if v.size}
        for what, (x, y) in _pairs(n, G, rng).items():
            ex, tot = X.exact_dot(x, y), X.abs_dot(x, y)
            for i in sorted(picks):
                for factor in (0.0, 2.0):
                    xp = x.copy()
                    xp[i] *= factor
                    assert abs(X.exact_dot(xp, y) - ex) > bound * tot, (n, what, i, factor)


def test_sentinels_sit_where_the_kernels_change_hands():
    G = 4
    t = 512
    s = X.sentinel_indices(9 * G * t + 77, G)
    assert list(s["block_first"]) == [0, t, 2 * t, 3 * t]
    assert list(s["block_last"]) == [(8 * G + b) * t for b in range(G)]
    assert list(s["plain_first"]) == [(8 * G + b) * t for b in range(G)]
    assert list(s["tail_first"]) == [9 * G * t]
    assert s["tile_last"][-1] == 9 * G * t - 1
    # 8 G tiles exactly: the ahead loop serves them all, no plain tile; one tile fewer: the last block has no ahead pass
    assert X.sentinel_indices(8 * G * t, G)["plain_first"].size == 0
    s = X.sentinel_indices(8 * G * t - 1, G)
    assert list(s["plain_first"]) == []
    assert list(s["block_last"]) == [(7 * G + b) * t for b in range(G - 1)] + [(6 * G + G - 1) * t]
    # no full tile
    s = X.sentinel_indices(7, G)
    assert list(s["ends"]) == [0, 6] and list(s["tail_first"]) == [0] and s["tile_last"].size == 0
