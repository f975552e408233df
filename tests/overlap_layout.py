"""Overlapped (halo / ghost) layouts of a global vector over `world` ranks, for the tests of the diagonal dot-product weights
on sharded handles (tests/test_dot_weights_sharded_cpu.py, tests/_weights_sharded_worker.py).  Pure numpy, no GPU.

A rank's local slice is x_global[src]; w is 1 on the entries the rank OWNS and 0 on its ghosts.  The owned entries of ranks
0, 1, ... in rank order are exactly the global vector in its order (build() asserts it), so a sharded accelerator with these
weights is mathematically the plain accelerator on the global vector (include/nka_hip.h: nka_hip_set_dot_weights)."""
from collections import namedtuple

import numpy as np

TILE = 512          # elements per tile of the aligned sum kernels (nka_amd/csrc/nka_device.hpp: kBlock * 2)

# src: int64 indices into the global vector; w: 0/1 float64; [lo, hi): the owned global range; first: the local index of
# the first owned entry (the owned entries are local [first, first + hi - lo))
Rank = namedtuple("Rank", "src w lo hi first")


def even_split(n_global, world):
    base, rem = divmod(int(n_global), int(world))
    return [base + (1 if r < rem else 0) for r in range(world)]


def build(n_global, world, spec=None):
    """-> [Rank] * world.  spec (a dict, every key optional):
      owned       owned lengths per rank (sum n_global); default: an even split
      halo        ghost entries on BOTH sides of the owned range (clipped at the ends of the global vector): one int, or
                  one (left, right) pair per rank.  A rank that owns nothing gets no halo.
      ghosts      {rank: k}: a rank that owns nothing holds k ghosts, copies of the k global entries from its (empty) range's
                  position on (the last k of the vector where fewer follow)
      tail_tiles  k: every local slice is its owned part -- a multiple of 512 long -- followed by k whole tiles of ghosts,
                  copies of the global entries that follow the owned range (cyclically)"""
    spec = dict(spec or {})
    n_global, world = int(n_global), int(world)
    owned = list(spec.pop("owned", None) or even_split(n_global, world))
    halo = spec.pop("halo", 0)
    ghosts = dict(spec.pop("ghosts", None) or {})
    tail = int(spec.pop("tail_tiles", 0))
    assert not spec, ("unknown layout keys", sorted(spec))
    assert len(owned) == world and sum(owned) == n_global and min(owned) >= 0, (owned, n_global)
    if isinstance(halo, int):
        halo = [(halo, halo)] * world
    assert len(halo) == world
    ranks, lo = [], 0
    for r in range(world):
        hi = lo + owned[r]
        own = np.arange(lo, hi, dtype=np.int64)
        if tail:
            assert owned[r] % TILE == 0 and r not in ghosts, (r, owned[r])
            left, right = np.zeros(0, np.int64), (hi + np.arange(tail * TILE, dtype=np.int64)) % n_global
        elif owned[r] == 0:
            k = int(ghosts.get(r, 0))
            assert k <= n_global
            start = min(lo, n_global - k)
            left, right = np.arange(start, start + k, dtype=np.int64), np.zeros(0, np.int64)
        else:
            assert r not in ghosts, (r, "a rank with ghosts only owns nothing")
            hl, hr = halo[r]
            left = np.arange(max(lo - hl, 0), lo, dtype=np.int64)
            right = np.arange(hi, min(hi + hr, n_global), dtype=np.int64)
        src = np.concatenate([left, own, right])
        w = np.concatenate([np.zeros(left.size), np.ones(own.size), np.zeros(right.size)])
        ranks.append(Rank(src, w, lo, hi, int(left.size)))
        lo = hi
    check(ranks, n_global)
    return ranks


def check(ranks, n_global):
    """The invariants every layout holds: 0/1 weights, the owned entries of the ranks in rank order are arange(n_global),
    and a rank's owned entries are local [first, first + hi - lo)."""
    for k in ranks:
        assert k.src.dtype == np.int64 and k.w.dtype == np.float64 and k.src.shape == k.w.shape
        assert np.isin(k.w, (0.0, 1.0)).all()
        assert k.src.size == 0 or (k.src.min() >= 0 and k.src.max() < n_global)
        own = np.flatnonzero(k.w)
        assert np.array_equal(own, np.arange(k.first, k.first + k.hi - k.lo))
        assert np.array_equal(k.src[own], np.arange(k.lo, k.hi))
    assert np.array_equal(np.concatenate([k.src[k.w != 0] for k in ranks]), np.arange(n_global))
    return ranks


def moved(ranks, shift, n_global):
    """The same local slices (src unchanged) with every inner ownership boundary moved by `shift` entries (within the
    halos): what a caller does who re-balances ownership without moving data."""
    cuts = [0] + [k.hi + shift for k in ranks[:-1]] + [n_global]
    out = []
    for r, k in enumerate(ranks):
        lo, hi = cuts[r], cuts[r + 1]
        w = ((k.src >= lo) & (k.src < hi)).astype(np.float64)
        first = int(np.flatnonzero(w)[0]) if w.any() else 0
        out.append(Rank(k.src, w, lo, hi, first))
    return check(out, n_global)


def without(ranks, r):
    """The layout with rank r (which owns nothing) taken out."""
    assert ranks[r].lo == ranks[r].hi
    return list(ranks[:r]) + list(ranks[r + 1:])


def gather(ranks, local, n_global):
    """The global vector assembled from the owned entries of the local vectors."""
    out = np.empty(n_global)
    for k, x in zip(ranks, local):
        out[k.lo:k.hi] = np.asarray(x)[k.first:k.first + k.hi - k.lo]
    return out


def ahead_length(ncu):
    """A local length beyond the hand-over of k_norm_diff's 8-tiles-ahead loop on a device of ncu compute units."""
    return 8 * int(ncu) * TILE + 1000


def named(name, ncu=256):
    """-> (n_global, world, spec) of the named layouts the tests run.  `ncu` (device_info()) sizes the one slice that must
    pass the hand-over of k_norm_diff's ahead loop, and the trailing-tile layout whose two runs must take the same grids
    (exact_sums.pass_grids: at least 4 ncu tiles of owned entries per rank)."""
    big = ahead_length(ncu)
    g4 = 4 * int(ncu)
    table = {
        "halo1": (200_003, 3, {"halo": 1}),
        "halo3": (262_147, 3, {"halo": 3}),
        "halo512": (300_007, 4, {"halo": 512}),
        "halo700": (400_009, 8, {"halo": 700}),
        "ghost_first": (250_001, 4, {"owned": [0] + even_split(250_001, 3), "ghosts": {0: 17}, "halo": 3}),
        "ghost_mid": (200_003, 3, {"owned": [100_001, 0, 100_002], "ghosts": {1: 17}, "halo": 1}),
        "ghost_last": (320_011, 8, {"owned": even_split(320_011, 7) + [0], "ghosts": {7: 130}, "halo": 130}),
        "empty": (220_009, 4, {"owned": [70_003, 0, 80_003, 70_003], "halo": 1}),
        # one element and no ghosts; a slice within one tile; one beyond the ahead loop's hand-over; the rest
        "shapes": (1 + 300 + big + 100_000, 4, {"owned": [1, 300, big, 100_000], "halo": [(0, 0), (0, 3), (3, 3), (3, 0)]}),
        "tail_tiles": ((2 * g4 + 70) * TILE, 2, {"owned": [(g4 + 60) * TILE, (g4 + 10) * TILE], "tail_tiles": 2}),
    }
    return table[name]


NAMES = ("halo1", "halo3", "halo512", "halo700", "ghost_first", "ghost_mid", "ghost_last", "empty", "shapes", "tail_tiles")


# ---- planted inputs for the exact-sum check of the sharded weighted sums -------------------------------------------------

def sentinel_set(ranks, n_global, G):
    """Global indices that carry a sentinel: where the sum kernels hand elements over inside every LOCAL slice
    (exact_sums.all_sentinels on the local length, mapped through src), and the first and last owned entry of every rank
    with the entries next to them -- the neighbours' ghosts."""
    import exact_sums as X
    idx = [X.all_sentinels(n_global, G)]
    for k in ranks:
        if k.src.size:
            idx.append(k.src[X.all_sentinels(k.src.size, G)])
        if k.hi > k.lo:
            idx.append(np.array([k.lo, k.hi - 1, max(k.lo - 1, 0), min(k.hi, n_global - 1)], dtype=np.int64))
    return np.unique(np.concatenate(idx))


def planted(ranks, n_global, G, rng, prev=None, background=0.125):
    """exact_sums.planted_input on the global vector with the sentinels of sentinel_set: N(0, background^2) everywhere,
    +-2^e (e in 0..3) at every sentinel, never the value the sentinel had in `prev`."""
    x = rng.standard_normal(n_global) * background
    idx = sentinel_set(ranks, n_global, G)
    val = np.ldexp(1.0, rng.integers(0, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    if prev is not None:
        same = val == prev[idx]
        val[same] = -val[same]
    x[idx] = val
    return x
