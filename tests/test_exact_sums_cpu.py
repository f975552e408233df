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


# ---- the batched accelerator: tests/test_batch_sums_exact_gpu.py -----------------------------------------------------------

BATCH_ALL_SHAPES = X.BATCH_SHAPES + [X.BATCH_WIDTH_SHAPE] + X.BATCH_CAP_SHAPES


def test_batch_k_follows_the_kernel():
    assert [X.batch_k(n) for n in (1, 512, 513, 1025, 16384)] == [11, 11, 13, 15, 73]
    assert X.batch_k(1024) == 13 and X.batch_k(16383) == 73
    assert len(X.BATCH_WAVE_EDGES) == 16 and sorted(X.BATCH_WAVE_EDGES) == [0, 1, 126, 127, 128, 129, 254, 255, 256, 257, 382, 383,
                                                                           384, 385, 510, 511]


def _batch_sum(x, y):
    """The summation order of k_batch_update<*, false> restated on the host, fma replaced by a rounded product and a rounded
    sum (one rounding MORE per element than the device takes): thread t adds the pair 2t, 2t + 1 of every tile of 512 in
    turn, the ragged tile with guards; a butterfly over each wavefront (lane i + lane i + 32, 16, 8, 4, 2, 1); then
    wavefronts 0, 1, 2, 3 in turn."""
    n = x.size
    prod = x * y
    acc = np.zeros(X.BATCH_THREADS)
    for base in range(0, n, X.BATCH_TILE):
        for q in range(2):
            part = prod[base + q: min(base + X.BATCH_TILE, n): 2]
            acc[:part.size] = acc[:part.size] + part
    waves = []
    for w in range(X.WAVES):
        v = acc[w * X.WAVE:(w + 1) * X.WAVE].copy()
        while v.size > 1:
            v = v[: v.size // 2] + v[v.size // 2:]
        waves.append(v[0])
    r = waves[0]
    for w in waves[1:]:
        r = r + w
    return float(r)


@pytest.mark.parametrize("n", [3 * 512 + 300, 7])
def test_the_batch_bound_holds_for_a_simulated_workgroup_sum(n):
    for seed in range(20):
        rng = np.random.default_rng(1000 * n + seed)
        x = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 30, n))      # adversarial exponents
        y = rng.standard_normal(n)
        err = abs(_batch_sum(x, y) - X.exact_dot(x, y))
        assert err <= X.gamma(X.batch_k(n)) * X.abs_dot(x, y), (n, seed, err / (X.U * X.abs_dot(x, y)), X.batch_k(n))


def _batch_pairs(n, rng):
    """_pairs for one system of a batch: the operands of the four sums an update forms, from batch_planted_input."""
    f_a = X.batch_planted_input(n, rng)
    f_b = X.batch_planted_input(n, rng, prev=f_a)
    f_c = X.batch_planted_input(n, rng, prev=f_b)
    f = X.batch_planted_input(n, rng, prev=f_c)
    d_old = f_a - f_b
    w_old = d_old / math.sqrt(float(np.dot(d_old, d_old)))
    d = f_c - f                                                      # w1 = f_c, the raw previous input
    w1n = d / math.sqrt(float(np.dot(d, d)))
    return {"<d,d>": (d, d), "<f,w1'>": (f, w1n), "<w1',w_p>": (w1n, w_old), "<f,w_p>": (f, w_old)}


def test_batch_sentinels_sit_where_the_kernel_changes_hands():
    s = X.batch_sentinel_indices(1537)                               # three full tiles and one element
    assert list(s["ends"]) == [0, 1535, 1536] and list(s["ragged_first"]) == [1536] and list(s["odd_last"]) == [1536]
    assert s["wave_edges"].size == 3 * 16 + 1 and {510, 511, 512, 513, 1024 + 126, 1024 + 385, 1536} <= set(s["wave_edges"])
    s = X.batch_sentinel_indices(514)
    assert list(s["ragged_first"]) == [512] and s["odd_last"].size == 0 and list(s["wave_edges"][-2:]) == [512, 513]
    s = X.batch_sentinel_indices(512)
    assert s["ragged_first"].size == 0 and s["wave_edges"].size == 16
    s = X.batch_sentinel_indices(1)
    assert list(s["ends"]) == [0] and list(s["odd_last"]) == [0] and list(s["ragged_first"]) == [0]
    for n in BATCH_ALL_SHAPES:
        idx = X.batch_all_sentinels(n)
        assert idx.size >= min(n, 2) and idx.min() >= 0 and idx.max() < n and np.unique(idx).size == idx.size
    rng = np.random.default_rng(0)
    a = X.batch_planted_input(700, rng)
    b = X.batch_planted_input(700, rng, prev=a)
    idx = X.batch_all_sentinels(700)
    assert (np.abs(a[idx]) >= 1).all() and (a[idx] != b[idx]).all() and (np.abs(np.delete(a, idx)) < 1).all()


def test_every_batch_sentinel_is_seen_by_the_bound():
    """The sensitivity argument of tests/test_batch_sums_exact_gpu.py without a GPU: at every shape it runs, the cap included,
    and for every sum an update forms, each sentinel's product exceeds twice the bound (plus the rounding of the exact sum)."""
    rng = np.random.default_rng(12)
    for n in BATCH_ALL_SHAPES:
        idx = X.batch_all_sentinels(n)
        bound = X.gamma(X.batch_k(n))
        for what, (x, y) in _batch_pairs(n, rng).items():
            tot = X.abs_dot(x, y)
            worst = float(np.abs(x[idx] * y[idx]).min())
            assert X.detectable(worst, bound, tot), (n, what, worst / tot, bound)


def test_dropping_or_doubling_a_batch_sentinel_fails_the_check_end_to_end():
    """The long way round, up to 1 537 elements: one sentinel zeroed or doubled, the sum taken exactly, held to the check of
    the GPU test -- for EVERY sentinel of the shape."""
    rng = np.random.default_rng(13)
    for n in [s for s in X.BATCH_SHAPES if s <= 1537]:
        bound = X.gamma(X.batch_k(n))
        for what, (x, y) in _batch_pairs(n, rng).items():
            ex, tot = X.exact_dot(x, y), X.abs_dot(x, y)
            for i in X.batch_all_sentinels(n):
                for factor in (0.0, 2.0):
                    xp = x.copy()
                    xp[i] *= factor
                    assert abs(X.exact_dot(xp, y) - ex) > bound * tot, (n, what, int(i), factor)


def test_near_threshold_generator_meets_both_outcomes(oracle):
    """A GUARD FOR THE GPU TEST of the scalar step on close calls (it runs the oracle and tests/batch_seq.py only): at every
    shape and flavour used there, the fixed seed series holds close calls that end with the pair in question dropped and
    close calls that end with it kept.  No system is left out; a series that fails is replaced in batch_seq.near_seeds."""
    import batch_seq as B
    for vlen in B.NEAR_VLENS:
        for mvec in B.NEAR_MVECS:
            for flavor in (0, 1, 2):
                dropped, kept = B.near_outcomes(oracle, vlen, mvec, flavor)
                assert dropped >= 1 and kept >= 1, (vlen, mvec, flavor, dropped, kept)
    a, b = B.NearThreshold(33, 5), B.NearThreshold(33, 5)
    for _ in range(20):
        (xa, na), (xb, nb) = a.next(), b.next()
        assert na == nb and (xa == xb).all()


# ---- the abstract-vector workspace: tests/test_vec_sums_exact_gpu.py --------------------------------------------------------

# the grids of an MI355X (256 CUs): 1 block per CU (the window kernels), 2, 3, 4, 5 (the padded widths) and 8 (k_dot, k_update_norm2)
VEC_GRIDS = (256, 512, 768, 1024, 1280, 2048)
VEC_BIG = 1 << 19               # from here on the GPU tests run at most two vectors ys (the host's fsum is the cost)


def test_vec_grid_and_vec_k_follow_the_kernels():
    # grid_for: 8 blocks per CU for two loads, (22 + nloads - 1) / nloads beyond, one for the window kernels
    assert [X.vec_grid(10 ** 8, 256, 2, nl) for nl in (2, 3, 5, 6, 9, 10, 11, 22, 27)] == [2048, 2048, 1280, 1024, 768, 768, 512, 256, 256]
    assert X.vec_grid(10 ** 8, 1024, 2, 2) == 4096                        # kMaxGrid
    assert X.vec_grid(1, 256, 2, 2) == 1 and X.vec_grid(1023, 256, 2, 2) == 1 and X.vec_grid(1024, 256, 2, 2) == 2
    assert X.vec_grid(1023, 256, 1, 2) == 3
    assert [X.vec_width(c) for c in (0, 1, 4, 5, 12, 13, 24)] == [4, 4, 4, 8, 12, 16, 24]
    assert X.vec_groups(0) == [0] and X.vec_groups(24) == [24] and X.vec_groups(25) == [13, 12] and X.vec_groups(49) == [17, 16, 16]
    # n = G * 512: one tile per block, two fma; block_reduce_store 9; k_finalize_rows one addition per thread + 9
    assert X.vec_k(256 * 512, 256, 2) == 2 + 9 + 1 + 9
    assert X.vec_k(256 * 512 + 1, 256, 2) == 2 + 1 + 9 + 10
    assert X.vec_k(256 * 512 + 257, 256, 2) == 2 + 2 + 9 + 10
    assert X.vec_k(2 * 2048 * 512 + 511, 2048, 2) == 4 + 2 + 9 + 8 + 9  # 8 partials per thread of k_finalize_rows
    assert X.vec_k(7, 1, 2) == 1 + 9 + 1 + 9 and X.vec_k(3001, 11, 1) == 1 + 1 + 9 + 10


def test_vec_sentinels_sit_where_the_kernels_change_hands():
    G, t = 4, 512
    s = X.vec_sentinel_indices(2 * G * t + t + 300, G, 2)                  # 9 tiles on 4 blocks and a tail of 300
    assert list(s["ends"]) == [0, 9 * t + 299]
    assert list(s["tile_last"]) == [k * t - 1 for k in range(1, 10)]
    assert list(s["tail"]) == [9 * t, 9 * t + 255, 9 * t + 256]
    assert list(s["block_first"]) == [0, t, 2 * t, 3 * t]
    assert list(s["block_last"]) == [5 * t, 6 * t, 7 * t, 8 * t]          # sorted: blocks 1, 2, 3 and block 0 (tiles 0, 4, 8)
    assert s["wave_edges"].size == 32 and {0, 1, 126, 127, 128, 129, 510, 511, 8 * t, 8 * t + 511} <= set(s["wave_edges"])
    s = X.vec_sentinel_indices(3 * 256 + 7, 2, 1)                          # the 8-byte path: tiles of 256, one element each
    assert list(s["tile_last"]) == [255, 511, 767] and list(s["tail"]) == [768]
    assert list(s["block_first"]) == [0, 256] and list(s["block_last"]) == [256, 512]
    assert s["wave_edges"].size == 16 and {0, 63, 64, 127, 255, 512, 767} <= set(s["wave_edges"])
    s = X.vec_sentinel_indices(7, 1, 2)                                    # no full tile
    assert list(s["ends"]) == [0, 6] and list(s["tail"]) == [0] and s["tile_last"].size == 0 and s["wave_edges"].size == 0
    assert X.vec_sentinel_indices(0, 1, 2)["ends"].size == 0
    both = X.vec_all_sentinels(9 * t, (4, 3), 2)                           # several grids: the union
    assert set(X.vec_all_sentinels(9 * t, 4, 2)) | set(X.vec_all_sentinels(9 * t, 3, 2)) == set(both)
    for vec in (1, 2):
        for n in X.vec_boundary_shapes(5, vec):
            idx = X.vec_all_sentinels(n, min(5, max(n // (256 * vec), 1)), vec)
            assert idx.size >= min(n, 2) and idx.min() >= 0 and idx.max() < n and np.unique(idx).size == idx.size
    rng = np.random.default_rng(0)
    a = X.vec_planted_input(3000, 3, 2, rng)
    b = X.vec_planted_input(3000, 3, 2, rng, prev=a)
    idx = X.vec_all_sentinels(3000, 3, 2)
    assert (np.abs(a[idx]) >= 1).all() and (a[idx] != b[idx]).all() and (np.abs(np.delete(a, idx)) < 1).all()


def _fma(a, b, c):
    """One fma: a*b + c rounded once (Fraction -> float rounds correctly)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _block_sum(v):
    """block_reduce_store / the end of k_finalize_rows: a butterfly over each wavefront of 64 (lane i + lane i + 32, 16,
    8, 4, 2, 1), then the wave sums 0, 1, 2, 3 in turn."""
    waves = []
    for w in range(X.WAVES):
        u = np.array(v[w * X.WAVE:(w + 1) * X.WAVE], dtype=np.float64)
        while u.size > 1:
            u = u[: u.size // 2] + u[u.size // 2:]
        waves.append(u[0])
    r = waves[0]
    for w in waves[1:]:
        r = r + w
    return float(r)


def _vec_model_sum(x, y, G, vec, tail_from=0, column_shift=None):
    """The workspace's blocked sum restated on the host, every fma rounded once: block b of G takes the tiles b, b + G,
    ..., thread t the elements vec * t ... vec * t + vec - 1 of a tile in turn; the last block walks the tail at stride
    256; block_reduce_store; thread t of k_finalize_rows adds the partials t, t + 256, ... to 0.0; the block sum again.
    `tail_from` = 1 is the MUTATION of a tail loop that starts one element late."""
    n = x.size
    tile = X.BLOCK * vec
    ntile = n // tile
    acc = [[0.0] * X.BLOCK for _ in range(G)]
    for t in range(ntile):
        a = acc[t % G]
        for th in range(X.BLOCK):
            for q in range(vec):
                i = t * tile + th * vec + q
                a[th] = _fma(x[i], y[i], a[th])
    for i in range(ntile * tile + tail_from, n):
        th = (i - ntile * tile - tail_from) % X.BLOCK
        acc[G - 1][th] = _fma(x[i], y[i], acc[G - 1][th])
    partials = [_block_sum(a) for a in acc]
    lanes = np.zeros(X.BLOCK)
    for b in range(G):
        lanes[b % X.BLOCK] = lanes[b % X.BLOCK] + partials[b]
    return _block_sum(lanes)


def _vec_check_passes(got, x, y, k):
    """The check of tests/test_vec_sums_exact_gpu.py: _hold."""
    return abs(got - X.exact_dot(x, y)) <= X.gamma(k) * X.abs_dot(x, y)


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_the_vec_bound_holds_for_the_modelled_blocked_sum(G, vec):
    """The model stays within gamma(vec_k) * abs_dot on planted inputs (three tiles per block and a tail that gives some
    threads two elements; one tile per block and one element) and on adversarial exponents -- and a tail loop that starts
    one element late does not (the first mutation of the issue, on the host-modelled part)."""
    t = X.BLOCK * vec
    rng = np.random.default_rng(10 * G + vec)
    for n in (3 * G * t + 300, G * t + 1):
        k = X.vec_k(n, G, vec)
        o = X.vec_operands(n, G, vec, rng, 1)
        for what, x, y in [p for p in X.vec_sum_pairs(o) if p[0] in ("<x,z>", "<r,r>", "<wn1,y0>")]:
            got = _vec_model_sum(x, y, G, vec)
            assert _vec_check_passes(got, x, y, k), (n, what, abs(got - X.exact_dot(x, y)) / (X.U * X.abs_dot(x, y)), k)
            assert not _vec_check_passes(_vec_model_sum(x, y, G, vec, tail_from=1), x, y, k), (n, what, "late tail")
    n = 2 * G * t + 77
    x = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 30, n))
    y = rng.standard_normal(n)
    assert _vec_check_passes(_vec_model_sum(x, y, G, vec), x, y, X.vec_k(n, G, vec))


def _vec_shape_grid(n, G, vec):
    """The grid grid_for launches at length n when G blocks are the most it may."""
    return min(G, max(n // (X.BLOCK * vec), 1))


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("G", VEC_GRIDS)
def test_every_planted_vec_sentinel_is_seen_by_the_bound(G, vec):
    """The sensitivity argument of tests/test_vec_sums_exact_gpu.py without a GPU: at every shape of vec_boundary_shapes, for
    every sum an entry forms from vec_operands, each sentinel's product exceeds twice the bound (plus the rounding of the
    exact sum), so a device sum that dropped it or counted it twice fails the check."""
    rng = np.random.default_rng(G + vec)
    for n in X.vec_boundary_shapes(G, vec):
        g = _vec_shape_grid(n, G, vec)
        idx = X.vec_all_sentinels(n, g, vec)
        sent = X.vec_sentinel_indices(n, g, vec)
        assert idx.size >= min(n, 2) and idx.min() >= 0 and idx.max() < n
        assert all(np.isin(v, idx).all() for v in sent.values())
        if n >= G * X.BLOCK * vec:
            assert sent["block_first"].size == G
        bound = X.gamma(X.vec_k(n, g, vec))
        for what, x, y in X.vec_sum_pairs(X.vec_operands(n, g, vec, rng, 2 if n >= VEC_BIG else 5)):
            tot = X.abs_dot(x, y)
            worst = float(np.abs(x[idx] * y[idx]).min())
            assert X.detectable(worst, bound, tot), (n, what, worst / tot, bound)


@pytest.mark.parametrize("G,vec", [(3, 1), (3, 2), (8, 2)])
def test_dropping_or_doubling_a_vec_sentinel_fails_the_check_end_to_end(G, vec):
    """The long way round on small grids: one sentinel zeroed or doubled, the sum taken exactly, held to the check of the
    GPU test; the first and the last sentinel of every kind, at every boundary shape."""
    rng = np.random.default_rng(17 * G + vec)
    for n in X.vec_boundary_shapes(G, vec):
        g = _vec_shape_grid(n, G, vec)
        bound = X.gamma(X.vec_k(n, g, vec))
        sent = X.vec_sentinel_indices(n, g, vec)
        picks = sorted({int(v[0]) for v in sent.values() if v.size} | {int(v[-1]) for v in sent.values() if v.size})
        for what, x, y in X.vec_sum_pairs(X.vec_operands(n, g, vec, rng, 1)):
            if what in ("<x,x>", "<r,r>"):
                continue                                                  # (one operand twice: a doubled element counts four times)
            ex, tot = X.exact_dot(x, y), X.abs_dot(x, y)
            for i in picks:
                for factor in (0.0, 2.0):
                    xp = x.copy()
                    xp[i] *= factor
                    assert abs(X.exact_dot(xp, y) - ex) > bound * tot, (n, what, i, factor)


def test_a_wrong_column_of_partials_fails_the_check():
    """The second mutation of the issue on the host model: k_finalize_rows reading column c + 1 returns the NEXT sum of
    the launch; on planted operands no two sums of a launch agree within the bound."""
    G, vec = 3, 2
    n = 3 * G * 512 + 300
    rng = np.random.default_rng(23)
    o = X.vec_operands(n, G, vec, rng, 4)
    k = X.vec_k(n, G, vec)
    sums = [(x, y, _vec_model_sum(x, y, G, vec)) for x, y in [(o["x"], yj) for yj in o["ys"]] + [(o["x"], o["z"])]]
    for c in range(len(sums) - 1):
        x, y, own = sums[c]
        assert _vec_check_passes(own, x, y, k) and not _vec_check_passes(sums[c + 1][2], x, y, k), c


@pytest.mark.parametrize("vec", [1, 2])
@pytest.mark.parametrize("ncu", [256, 80])
def test_the_shared_vec_operands_are_seen_by_every_grid(ncu, vec):
    """The shapes at which the GPU tests share one set of operands among entries and counts (every width 1..24, the long
    lists, the small cases): planted for EVERY grid an entry may launch there, each sentinel detectable under the
    largest bound among them."""
    rng = np.random.default_rng(ncu + vec)
    for n, count in [(X.vec_widths_shape(ncu), X.VEC_MANY_MAX), (X.VEC_LONG_SHAPE, 49)] + [(s, 5) for s in X.VEC_SMALL_SHAPES]:
        grids = X.vec_all_grids(n, ncu, vec)
        idx = X.vec_all_sentinels(n, grids, vec)
        bound = max(X.gamma(X.vec_k(n, g, vec)) for g in grids)
        for what, x, y in X.vec_sum_pairs(X.vec_operands(n, grids, vec, rng, count)):
            tot = X.abs_dot(x, y)
            worst = float(np.abs(x[idx] * y[idx]).min())
            assert X.detectable(worst, bound, tot), (n, what, worst / tot, bound)
