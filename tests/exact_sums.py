"""Exact inner products and the error bound of the device's blocked sums (host code, no GPU).

exact_dot(x, y) is the reference every fast sum of the library is held to (tests/test_sums_exact_gpu.py);
k_steps / device_k derive how many roundings a product can meet on its way through the kernels that form the sums
(nka_amd/csrc/nka_kernels.hpp: k_norm_diff, k_dots, k_dots_win, k_norm_fin, k_finalize_dots; nka_device.hpp: block_reduce_store) with the
grids the library launches them on (nka_amd/csrc/nka_hip.hip: sums_rounded, launch_dots_win_1, launch_dots_1, grid_for);
planted_input builds the inputs of the GPU tests: a small random background with sentinels at the indices where the
kernels hand elements from one loop, block or launch to the next.  tests/test_exact_sums_cpu.py holds all of it to
Fraction arithmetic and shows that losing or doubling any one sentinel breaks the bound.

The batched accelerator (nka_amd/csrc/nka_batch.hip) forms its sums in one workgroup per system: batch_k,
batch_sentinel_indices and batch_planted_input, at the end of this file, are its counterparts of device_k, sentinel_indices
and planted_input (tests/test_batch_sums_exact_gpu.py).

The abstract-vector workspace (nka_amd/csrc/vec_ops.hip) sums on a persistent grid of its own: vec_grid, vec_k,
vec_sentinel_indices, vec_planted_input and vec_boundary_shapes, behind the batch section, are read off its kernels
(tests/test_vec_sums_exact_gpu.py).
"""
import math

import numpy as np

U = 2.0 ** -53                  # unit roundoff of binary64 (round to nearest)
SPLIT = 2.0 ** 27 + 1.0         # Veltkamp: x = hi + lo, both halves of <= 26 significant bits

# launch geometry of the sum kernels (nka_device.hpp, nka_kernels.hpp)
BLOCK = 256                     # kBlock: threads per block, 4 wavefronts of 64
WAVE = 64
WAVES = BLOCK // WAVE
FIN_THREADS = 64                # kFinThreads (k_finalize_dots) and the one wavefront of k_norm_fin
WAVE_LEVELS = 6                 # exchange-and-add steps of a 64-lane butterfly (wave_sum / block_reduce_store)
DOTS_PER_CU_MAX = 4             # grid_for: (22 + nloads - 1) / nloads blocks per CU for k_dots<4, *> (6 loads per thread)

# exact_dot is exact for |x_i|, |y_i| < 2**995 (the split SPLIT*x and the products stay finite) and nonzero products
# |x_i*y_i| >= 2**-916 (the smallest partial product of the split, ~2**-106 |x_i*y_i|, stays a normal number)
MAX_ABS = 2.0 ** 995
MIN_PRODUCT = 2.0 ** -916


def two_prod(x, y):
    """Error-free products (Dekker / Veltkamp): x*y == p + e exactly, elementwise, inside the range above."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    p = x * y
    c = SPLIT * x
    xh = c - (c - x)
    xl = x - xh
    c = SPLIT * y
    yh = c - (c - y)
    yl = y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def exact_dot(x, y):
    """The correctly rounded value of sum x_i*y_i.

    Finite inputs: every product becomes p + e exactly (two_prod) and math.fsum rounds the sum of all of them once.
    Inputs outside the range where the split is exact (MAX_ABS, MIN_PRODUCT) raise ValueError.  Non-finite inputs follow
    IEEE arithmetic in ANY order of summation: NaN where a product is NaN (NaN, Inf * 0) or where products of both
    infinities meet, else the infinity of the products."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if x.shape != y.shape:
        raise ValueError("exact_dot: lengths differ")
    if x.size == 0:
        return 0.0
    fin = np.isfinite(x) & np.isfinite(y)
    if not fin.all():
        with np.errstate(invalid="ignore", over="ignore"):
            q = x * y
        if np.isnan(q).any() or ((q == np.inf).any() and (q == -np.inf).any()):
            return math.nan
        if np.isinf(q[fin]).any():
            raise ValueError("exact_dot: a product of finite elements overflows")
        return math.inf if (q == np.inf).any() else -math.inf
    if max(float(np.abs(x).max()), float(np.abs(y).max())) >= MAX_ABS:
        raise ValueError("exact_dot: an element beyond the range of the exact split")
    p, e = two_prod(x, y)
    ap = np.abs(p)
    if ((ap > 0) & (ap < MIN_PRODUCT)).any():
        raise ValueError("exact_dot: a product below the range of the exact split")
    return math.fsum(np.concatenate([p, e]))


def abs_dot(x, y):
    """sum |x_i*y_i|, rounded upwards far enough to be an upper bound (the scale of the error bound)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.size == 0:
        return 0.0
    return float(np.abs(x * y).sum()) * (1.0 + (x.size + 2) * U)


def _cdiv(a, b):
    return -(-a // b)


def k_steps(n, G, width):
    """Roundings a product can meet in a blocked fma sum of n elements over G blocks, `width` elements per thread and
    tile (2: the 16-byte path, tiles of 512; 1: the scalar path of an unaligned f, tiles of 256).

      per-thread chain   width * ceil(ntile / G) fma on full tiles (block b takes tiles b, b + G, ...; k_norm_diff's
                         8-tiles-ahead loop visits them in the same order), ntile = n // (BLOCK * width);
      ragged tail        ceil(tail / BLOCK) more fma in the last block (tail < BLOCK * width elements, stride BLOCK);
                         the unaligned k_norm_diff's grid-stride over elements, ceil(n / (G * BLOCK)) fma, is no longer;
      block_reduce_store a 64-lane butterfly of WAVE_LEVELS additions, then waves 1..3 added to wave 0 in turn (3);
      final sum          ceil(G / FIN_THREADS) additions per lane of k_finalize_dots / k_norm_fin, then a butterfly.

    A fma rounds once (the product enters exactly), so a product picks up at most this many factors (1 + delta)."""
    tile = BLOCK * width
    ntile = n // tile
    chain = width * _cdiv(ntile, G) + _cdiv(n - ntile * tile, BLOCK)
    block = WAVE_LEVELS + (WAVES - 1)
    fin = _cdiv(G, FIN_THREADS) + WAVE_LEVELS
    return chain + block + fin


def pass_grids(n, ncu, aligned):
    """(G, width) of every launch that can form a sum of one single-rank update on a device of `ncu` compute units.

    16-byte aligned f: k_norm_diff and k_dots_win run one block per CU, at most one per 512-element tile (sums_rounded,
    launch_dots_win_1); k_dots<4, 2> -- the update whose only stored vector is the pending pair -- takes up to
    DOTS_PER_CU_MAX blocks per CU as its occupancy allows (launch_dots_1, grid_for).  Unaligned f: k_norm_diff's
    grid-stride over elements on the same grid, and k_dots<4, 1> on tiles of 256."""
    t2 = max(n // (BLOCK * 2), 1)
    if aligned:
        return [(min(ncu, t2), 2)] + [(min(ncu * q, t2), 2) for q in range(1, DOTS_PER_CU_MAX + 1)]
    t1 = max(n // BLOCK, 1)
    return [(min(ncu, t2), 1)] + [(min(ncu * q, t1), 1) for q in range(1, DOTS_PER_CU_MAX + 1)]


def device_k(n, ncu, aligned=True):
    """K for every sum of one update: the largest k_steps over the launches that may form it."""
    return max(k_steps(n, G, w) for G, w in pass_grids(n, ncu, aligned))


def sum_bound(n, G, width):
    """Relative error bound of the device's blocked fma sum against the ROUNDED exact sum, per unit of sum |x_i*y_i|:
    gamma(K + 1) = (K + 1) u / (1 - (K + 1) u), K = k_steps(n, G, width); the + 1 is the rounding of exact_dot itself
    (|fl(S) - S| <= u |S| <= u sum |x_i*y_i|)."""
    k = k_steps(n, G, width) + 1
    return k * U / (1.0 - k * U)


def gamma(k):
    """gamma(K + 1) for a K from device_k (see sum_bound)."""
    return (k + 1) * U / (1.0 - (k + 1) * U)


# ---- planted inputs -------------------------------------------------------------------------------------------------------

def sentinel_indices(n, G):
    """Indices where the aligned sum kernels hand elements over, for a grid of G blocks (one per CU) and tiles of 512,
    by name.  Empty arrays where a shape has no such place."""
    tile = BLOCK * 2
    ntile = n // tile
    out = {"ends": np.unique(np.array([0, n - 1] if n else [], dtype=np.int64))}
    out["tile_last"] = np.arange(1, ntile + 1, dtype=np.int64) * tile - 1          # last element of every full tile
    out["tail_first"] = np.array([ntile * tile] if ntile * tile < n else [], dtype=np.int64)
    blocks = np.arange(min(G, ntile), dtype=np.int64)
    last_tile = blocks + G * ((ntile - 1 - blocks) // G)
    out["block_first"] = blocks * tile                                            # first element of each block's first tile
    out["block_last"] = last_tile * tile                                          # ... and of its last tile
    # k_norm_diff's ahead loop serves tiles t, t + G, ..., t + 7G while t + 7G < ntile, stepping 8G; the first tile the
    # plain loop serves after it, where there is one
    ahead = np.where(ntile - 7 * G - blocks - 1 >= 0, (ntile - 7 * G - blocks - 1) // (8 * G) + 1, 0)
    plain = blocks + 8 * G * ahead
    out["plain_first"] = plain[(ahead > 0) & (plain < ntile)] * tile
    return out


def all_sentinels(n, G):
    s = sentinel_indices(n, G)
    return np.unique(np.concatenate([v for v in s.values()] + [np.zeros(0, np.int64)]))


def planted_input(n, G, rng, prev=None, background=0.125):
    """One input f: N(0, background^2) everywhere, +-2^e (e in 0..3, random sign) at every sentinel.  A sentinel never
    repeats the value it had in `prev` (the previous input), so that d = w1 - f is at least 1 in magnitude there: every
    product at a sentinel -- of f, d, the normalised w1' and the stored w -- is far above the error bound."""
    x = rng.standard_normal(n) * background
    idx = all_sentinels(n, G)
    if idx.size == 0:
        return x
    val = np.ldexp(1.0, rng.integers(0, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    if prev is not None:
        same = val == prev[idx]
        val[same] = -val[same]
    x[idx] = val
    return x


def boundary_shapes(G):
    """The vector lengths where the kernels change hands, for G compute units: tiny vectors around one wavefront and one
    tile, every block owning exactly one tile (G * 512 +- 1), and the hand-over of k_norm_diff's 8-tiles-ahead loop to
    its plain loop (8 G * 512 ...)."""
    t = BLOCK * 2
    return [1, 2, 7, 63, 64, 65, 511, 512, 513,
            G * t - 1, G * t, G * t + 1,
            8 * G * t - 1, 8 * G * t, 8 * G * t + 1, 8 * G * t + 511, 9 * G * t + 77]


def pb_ticket_shape(G):
    """A length at which PB hands its tiles out by tickets (pb_tickets_apply: n / 512 >= 64 G), not a multiple of 512."""
    return 64 * G * BLOCK * 2 + 1031


def detectable(term, bound, total_abs):
    """A sum that lost (or doubled) the product `term` is off the exact sum by |term| minus its own error: the check
    |red - exact| <= bound * total_abs cannot pass if |term| > 2 bound total_abs + u total_abs (the last: rounding of the
    exact sum)."""
    return abs(term) > (2.0 * bound + U) * total_abs


# ---- the batched accelerator (nka_amd/csrc/nka_batch.hip: k_batch_update<*, false>) ---------------------------------------
# One workgroup per system forms every sum of that system: there is no grid and no cross-block stage.

BATCH_THREADS = 256             # kBatchThreads: 4 wavefronts of 64
BATCH_TILE = 2 * BATCH_THREADS  # kBatchTile: thread t owns the pair 2t, 2t + 1 of every 512 elements
BATCH_GROUP = 4                 # kBatchGroup: older vectors per sweep of phase 3
BATCH_MAX_VLEN = 16384          # NKA_HIP_BATCH_MAX_VLEN
# offsets inside a tile of the first and the last pair of each wavefront (lanes 0 and 63 of wavefronts 0..3)
BATCH_WAVE_EDGES = tuple(2 * (64 * w + lane) + q for w in range(WAVES) for lane in (0, 63) for q in (0, 1))


def batch_k(n):
    """Roundings a product can meet in a sum of k_batch_update<*, false> over n elements, read off the kernel:

      per-thread chain   batch_sweep gives thread t the pair (2t, 2t + 1) of every tile of 512 elements, the full tiles
                         first, then the ragged one; each element is ONE fma into ONE accumulator per sum (phase 2:
                         acc[0]; phase 3: acc[j], acc[4 + j], acc[8]), so a thread's chain is at most two fma per tile:
                         2 * ceil(n / 512).  (The first fma adds to 0.0 and so rounds the product only: still one.)
      batch_block_sum    wave_sum, a 64-lane butterfly of WAVE_LEVELS = 6 additions (offsets 32, 16, 8, 4, 2, 1), then
                         sm[0] + sm[1] + sm[2] + sm[3]: wavefronts 1..3 added to wavefront 0 in turn, 3 additions.
      nothing else       res[] is copied to red[]; one workgroup owns the whole system.

    A fma rounds once (the product enters it exactly): 2 * ceil(n / 512) + 9 factors (1 + delta) at most; 11 up to one
    tile, 73 at the cap of 16 384 elements.  The bound applied is gamma(batch_k(n)) * abs_dot (gamma adds the rounding
    of exact_dot itself)."""
    return 2 * _cdiv(n, BATCH_TILE) + WAVE_LEVELS + (WAVES - 1)


def batch_sentinel_indices(n):
    """Indices where the batch kernel changes hands in a system of n elements, by name (empty where there is none):

      ends          0, n - 1 and n - 2;
      wave_edges    in every tile, the full ones and the ragged one, the first and the last pair of each wavefront
                    (BATCH_WAVE_EDGES): where the butterfly of one wavefront ends and sm[] takes over;
      ragged_first  the first element of the ragged tile (batch_sweep leaves the straight-line full tiles for the
                    guarded body);
      odd_last      n - 1 for odd n: the first element of a pair whose second lies beyond n (ld_pair falls back from the
                    16-byte load to guarded 8-byte loads and returns a zero that must not be accumulated)."""
    ntile = n // BATCH_TILE
    i = (np.arange(_cdiv(n, BATCH_TILE), dtype=np.int64)[:, None] * BATCH_TILE +
         np.array(BATCH_WAVE_EDGES, dtype=np.int64)[None, :]).ravel()
    return {"ends": np.unique(np.array([k for k in (0, n - 2, n - 1) if k >= 0], dtype=np.int64)),
            "wave_edges": i[i < n],
            "ragged_first": np.array([ntile * BATCH_TILE] if ntile * BATCH_TILE < n else [], dtype=np.int64),
            "odd_last": np.array([n - 1] if n % 2 else [], dtype=np.int64)}


def batch_all_sentinels(n):
    return np.unique(np.concatenate(list(batch_sentinel_indices(n).values())))


def batch_planted_input(n, rng, prev=None, background=0.125):
    """planted_input for one system of a batch: N(0, background^2) everywhere, +-2^e (e in 0..3, random sign) at every
    batch sentinel, never the value `prev` has there."""
    x = rng.standard_normal(n) * background
    idx = batch_all_sentinels(n)
    val = np.ldexp(1.0, rng.integers(0, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    if prev is not None:
        same = val == prev[idx]
        val[same] = -val[same]
    x[idx] = val
    return x


# shapes of tests/test_batch_sums_exact_gpu.py: around one wavefront's pairs (127 .. 129), two (255 .. 257), one tile
# (511 .. 514: the ragged tile of one element, and of one full pair), two tiles, three tiles + 1, eight tiles + 3
BATCH_SHAPES = [1, 2, 3, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 514, 1023, 1024, 1025, 1537, 4099]
BATCH_WIDTH_SHAPE = 700         # every older count up to NKA_HIP_BATCH_MAX_MVEC = 32
BATCH_CAP_SHAPES = [BATCH_MAX_VLEN - 1, BATCH_MAX_VLEN]


# ---- the abstract-vector workspace (nka_amd/csrc/vec_ops.hip) --------------------------------------------------------------
# k_dot, k_dot_many, k_dot_pair_many, k_update_norm2, k_scale_dot_pair_many and k_scale_dot_pair_many_win all sum the same
# way: a persistent grid of G blocks, block b takes the tiles b, b + G, ... of 256 * VEC elements, the last block the
# ragged tail, block_reduce_store leaves one partial per block and column, k_finalize_rows sums a column's partials.

VEC_MAX_GRID = 4096             # kMaxGrid (nka_ctl.hpp)
VEC_PER_CU_MAX = 8              # grid_for (vec_ops.hip): at most 8 blocks per CU
VEC_LOADS_PER_CU = 22           # blocks_per_cu (host_logic.hpp): one block per CU once a thread keeps 22 loads in flight
VEC_MANY_MAX = 24               # kManyMax (host_logic.hpp): vectors per launch
VEC_FIN_THREADS = BLOCK         # k_finalize_rows runs kBlock threads (vec_ops.hip: fetch_sums)


def vec_width(count):
    """width_for (vec_ops.hip): the unroll width 4, 8, ..., 24 of a padded kernel for `count` vectors."""
    return max(4, _cdiv(count, 4) * 4)


def vec_groups(count):
    """The widths of the balanced launch groups of a list of `count` vectors (host_logic.hpp: many_groups,
    many_group_width; 25 = 13 + 12): what dot_pair_many_scaled and diff_norm_dot_pair_many run."""
    ng = 1 if count <= VEC_MANY_MAX else _cdiv(count, VEC_MANY_MAX)
    return [count // ng + (1 if p < count % ng else 0) for p in range(ng)]


def vec_grid(n, ncu, vec, nloads):
    """grid_for (vec_ops.hip) = persistent_grid(ncu, min(8, blocks_per_cu(nloads)), tiles) of host_logic.hpp:
    per_cu = max(1, min(8, (22 + nloads - 1) / nloads)) blocks per CU, at most one
    block per tile of 256 * vec elements (at least one block), at most kMaxGrid.  `nloads` is what the entry passes: 2
    (dot, update_norm2), nv + 1 (dot_many), nv + 2 (dot_pair_many), 22 for the window kernels and
    nv + 3 for the 8-byte k_scale_dot_pair_many; nv = vec_width(count) but for the window kernels, whose width
    is max(count, 1) (scale_dot_pair_many_impl)."""
    per_cu = max(1, min(VEC_PER_CU_MAX, _cdiv(VEC_LOADS_PER_CU, nloads)))
    return min(ncu * per_cu, max(n // (BLOCK * vec), 1), VEC_MAX_GRID)


def vec_k(n, G, vec):
    """Roundings a product can meet in a sum of the workspace over n elements on a grid of G blocks, read off the kernels:

      per-thread chain    block b serves the tiles b, b + G, ... < ntile = n // (256 * vec), one fma per element and sum
                          into ONE accumulator (k_dot :72-78, k_dot_many :197-208, k_dot_pair_many :228-244,
                          k_update_norm2 :336-347, k_scale_dot_pair_many :377-406, the window kernel :564-605 in the same
                          order): vec * ceil(ntile / G) fma;
      ragged tail         the last block walks the tail at stride 256 (:79-80, :209-212, :245-254, :348-353, :407-426,
                          :606-625): ceil(tail / 256) more fma, tail < 256 * vec;
      block_reduce_store  (nka_device.hpp) the 64-lane butterfly of WAVE_LEVELS = 6 additions, then the four wave
                          sums in turn: 3 additions;
      k_finalize_rows     (:877-901) thread t adds the partials t, t + 256, ... of its column -- ceil(G / 256) additions,
                          256 threads, not the 64 of k_finalize_dots --, the butterfly (6) and the four wave sums (3).

    A fma rounds once (the product enters it exactly), so a product meets at most this many factors (1 + delta).  The
    bound applied is gamma(vec_k) * abs_dot (gamma adds the rounding of exact_dot itself)."""
    tile = BLOCK * vec
    ntile = n // tile
    chain = vec * _cdiv(ntile, G) + _cdiv(n - ntile * tile, BLOCK)
    block = WAVE_LEVELS + (WAVES - 1)
    fin = _cdiv(G, VEC_FIN_THREADS) + WAVE_LEVELS + (WAVES - 1)
    return chain + block + fin


def _grids(G):
    return (int(G),) if np.isscalar(G) else tuple(int(g) for g in G)


def vec_sentinel_indices(n, G, vec):
    """Indices where the workspace's sum kernels change hands in a vector of n elements, tiles of 256 * vec, on a grid of
    G blocks (G may be several grids: the union), by name; empty arrays where a shape has no such place:

      ends         0 and n - 1;
      tile_last    the last element of every full tile (the tile loops :72, :197, :228, :336, :377, :564);
      tail         the first element of the tail and the tail elements at offsets 255 and 256: the tail is walked at
                   stride 256 (:80, :210, :246, :349, :408, :607), up to two elements per thread on the 16-byte path;
      block_first  the first element of each block's first tile;
      block_last   ... and of its last tile, where the window kernel prefetches its own tile again (tn == t, :566, :587);
      wave_edges   the first and the last thread's elements of each wavefront in the first and in the last full tile
                   (thread t owns elements vec * t ... of a tile): where a wavefront's butterfly ends and sm[] takes over."""
    tile = BLOCK * vec
    ntile = n // tile
    tail0 = ntile * tile
    out = {"ends": np.unique(np.array([0, n - 1] if n else [], dtype=np.int64)),
           "tile_last": np.arange(1, ntile + 1, dtype=np.int64) * tile - 1,
           "tail": np.array([i for i in (tail0, tail0 + BLOCK - 1, tail0 + BLOCK) if i < n], dtype=np.int64)}
    first, last = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for g in _grids(G):
        blocks = np.arange(min(g, ntile), dtype=np.int64)
        first.append(blocks * tile)
        last.append((blocks + g * ((ntile - 1 - blocks) // g)) * tile)
    out["block_first"] = np.unique(np.concatenate(first))
    out["block_last"] = np.unique(np.concatenate(last))
    edges = np.array([vec * (WAVE * w + lane) + q for w in range(WAVES) for lane in (0, WAVE - 1) for q in range(vec)],
                     dtype=np.int64)
    tiles = np.unique(np.array([0, ntile - 1] if ntile else [], dtype=np.int64))
    out["wave_edges"] = (tiles[:, None] * tile + edges[None, :]).ravel()
    return out


def vec_all_sentinels(n, G, vec):
    return np.unique(np.concatenate(list(vec_sentinel_indices(n, G, vec).values()) + [np.zeros(0, np.int64)]))


def vec_planted_input(n, G, vec, rng, background=0.125, prev=None):
    """planted_input for the workspace: N(0, background^2) everywhere, +-2^e (e in 0..3, random sign) at every sentinel of
    vec_sentinel_indices(n, G, vec), never the value `prev` has there."""
    x = rng.standard_normal(n) * background
    idx = vec_all_sentinels(n, G, vec)
    if idx.size == 0:
        return x
    val = np.ldexp(1.0, rng.integers(0, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    if prev is not None:
        same = val == prev[idx]
        val[same] = -val[same]
    x[idx] = val
    return x


def vec_boundary_shapes(G, vec):
    """The lengths where the workspace's kernels change hands on a grid of up to G blocks (grid_for, vec_ops.hip; persistent_grid, host_logic.hpp:
    one block per tile until G is reached), t = 256 * vec: the fixed small
    ones around one wavefront's stride and one tile, every block's first tile being its last (G t +- 1), one block with a
    second tile ((G + 1) t), and two tiles per block with and without a tail, the longest tail included."""
    t = BLOCK * vec
    return [1, 2, 255, 256, 257, 511, 512, 513,
            G * t - 1, G * t, G * t + 1,
            (G + 1) * t, 2 * G * t - 1, 2 * G * t + 1, 2 * G * t + t - 1]


VEC_SHAPE_IDS = ["1", "2", "255", "256", "257", "511", "512", "513", "Gt-1", "Gt", "Gt+1", "(G+1)t", "2Gt-1", "2Gt+1", "2Gt+t-1"]

# The scalars of the fused stages in the tests.  No power of two: with sentinels of +-2^e in both operands a*x + z and
# pre_a*f + w never cancel at a sentinel (|0.7312 * 2^i +- 2^j| >= 0.2688, |0.75 * 2^i +- 2^j| >= 0.25), so every derived
# operand keeps a sentinel of at least a quarter where its sources have one.
VEC_A = 0.7312                  # r = a*x + z (update_norm2), d = a*x + z (diff_norm_dot_pair_many)
VEC_PRE_A = -0.75               # w0 = pre_a*f + w
VEC_SCALE = 0.3                 # wn = a*w0, vn = a*v


def vec_operands(n, G, vec, rng, count):
    """The host operands of tests/test_vec_sums_exact_gpu.py at one shape, all planted at the same sentinels: x, z, f, w, v
    and `count` vectors ys, and the operands the fused stages derive from them, formed as the kernels form them (numpy:
    IEEE, left to right, no fma):  r = a*x + z;  wn_pre = a*(pre_a*f + w), wn = a*w;  vn = a*v and vn - wn."""
    o = {k: vec_planted_input(n, G, vec, rng) for k in ("x", "z", "f", "w", "v")}
    o["ys"] = [vec_planted_input(n, G, vec, rng) for _ in range(count)]
    o["r"] = VEC_A * o["x"] + o["z"]
    o["wn0"] = VEC_SCALE * o["w"]
    o["wn1"] = VEC_SCALE * (VEC_PRE_A * o["f"] + o["w"])
    return o


def vec_sum_pairs(o):
    """(name, x, y) of every sum the workspace's entries form from vec_operands."""
    pairs = [("<x,z>", o["x"], o["z"]), ("<x,x>", o["x"], o["x"]), ("<r,r>", o["r"], o["r"]), ("<x,r>", o["x"], o["r"]),
             ("<f,wn0>", o["f"], o["wn0"]), ("<f,wn1>", o["f"], o["wn1"])]
    for j, y in enumerate(o["ys"]):
        pairs += [(f"<x,y{j}>", o["x"], y), (f"<z,y{j}>", o["z"], y), (f"<r,y{j}>", o["r"], y), (f"<f,y{j}>", o["f"], y),
                  (f"<wn0,y{j}>", o["wn0"], y), (f"<wn1,y{j}>", o["wn1"], y)]
    return pairs


def vec_all_grids(n, ncu, vec):
    """Every grid some entry of the workspace may launch at length n (nloads 2 ... kManyMax + 3): what operands shared by
    several entries and counts are planted for."""
    return sorted({vec_grid(n, ncu, vec, nl) for nl in range(2, VEC_MANY_MAX + 4)})


def vec_widths_shape(ncu):
    """Every count 1..24 runs here: three 512-tiles per block of the window kernels' grid (one block per CU) and a ragged
    tail that gives some threads two elements."""
    return 3 * ncu * 2 * BLOCK + 301


VEC_LONG_SHAPE = 39 * 512 + 43          # counts 25, 37, 49: lists longer than one launch
VEC_SMALL_SHAPES = [7 * 512 + 300, 3 * 512 + 77]     # the non-finite cases; the refusals in reference order
