"""The wave batch (include/nka_hip_batch.h, WAVES; nka_amd/csrc/nka_batch_waves.hip: one wavefront per system, four systems per
workgroup) restated on the host: the number of roundings on the longest path of one of its sums, a model of the sum in the
kernel's order, the sentinel inputs and the shapes of tests/test_batch_waves_gpu.py.  No GPU here: tests/test_batch_waves_cpu.py
holds the model to exact sums, shows that the bound sees every sentinel, and reads waves_k off the kernel's text."""
import math

import numpy as np

import exact_sums as X

GROUP = 4                       # kWavesGroup: systems (wavefronts) per workgroup
TILE = 128                      # kWavesTile: lane l owns the pair 2l, 2l + 1 of every tile
LANES = 64
LEVELS = 6                      # the butterfly of wave_sum: offsets 32, 16, 8, 4, 2, 1
MAX_MVEC = 32
LDS_LIMIT = 64 * 1024           # dynamic LDS a launch may ask for without an attribute of the function
PAD = 7.25                      # what F and X hold wherever no active system owns the element


def limits():
    """(systems per workgroup, NKA_HIP_BATCH_WAVES_MAX_VLEN) as the loaded library was built."""
    import nka_amd
    return nka_amd.batch_waves_limits()


def waves_k(n):
    """Roundings a product can meet in a sum of k_waves_update over n elements, read off the kernel:

      per-lane chain   waves_sweep gives lane l the pair (2l, 2l + 1) of every tile of 128 elements, the full tiles first, then
                       the ragged one; each element is ONE fma into ONE accumulator per sum, so a lane's chain is at most two
                       fma per tile: 2 * ceil(n / 128);
      wave_sum         a 64-lane butterfly of six additions (offsets 32, 16, 8, 4, 2, 1);
      nothing else     the result goes from lane 0 to red[]; one wavefront owns the whole system.

    A fma rounds once: 2 * ceil(n / 128) + 6.  The bound applied is exact_sums.gamma(waves_k(n)) * abs_dot."""
    return 2 * (-(-n // TILE)) + LEVELS


def copy_bytes(mvec):
    """LDS of one wavefront's working copy: the layout of batch_lds(mvec) (host_logic.hpp), rounded up to 16 bytes."""
    m1 = mvec + 1
    nd = (m1 + 1) ** 2 + (m1 + 1) + (2 + 2 * mvec) + m1 + 4 * 9 + 10
    ni = 2 * (m1 + 1) + 2 * m1 + 8
    return (8 * nd + 4 * ni + 15) // 16 * 16


def ngroup(nsys):
    return -(-nsys // GROUP)


def slot_stride(vlen):
    return (vlen + 31) // 32 * 32


def vector_bytes(vlen, mvec, nsys):
    """nka_hip_batch_vector_bytes: the narrow batch's formula -- w and v, nsys x (mvec + 1) slots at the slot stride."""
    return 2 * 8 * slot_stride(vlen) * (mvec + 1) * nsys


# ---- the sum in the kernel's order ------------------------------------------------------------------------------------------

def fma(a, b, c):
    """fl(a b + c), one rounding: the product split exactly (exact_sums.two_prod), math.fsum rounds once."""
    p, e = X.two_prod(np.float64(a), np.float64(b))
    return math.fsum((float(p), float(e), float(c)))


def lane_accumulators(x, y, take=None):
    """The 64 accumulators before the butterfly: lane l meets its pairs 2l, 2l + 1 of tile 0, 1, ... in increasing order, one fma
    each; elements beyond n are not accumulated.  take(i) -> the (x, y) the sum uses for element i (default: its own): a model
    of a kernel that loses, doubles or misplaces an element."""
    n = len(x)
    acc = [0.0] * LANES
    for lane in range(LANES):
        a = 0.0
        for i0 in range(2 * lane, n, TILE):
            for i in (i0, i0 + 1):
                if i < n:
                    for xi, yi in ([(x[i], y[i])] if take is None else take(i)):
                        a = fma(xi, yi, a)
        acc[lane] = a
    return np.array(acc)


def butterfly(acc):
    """wave_sum: x[l] += x[l + off], off = 32, 16, 8, 4, 2, 1; the value of lane 0."""
    v = np.array(acc, dtype=np.float64)
    off = LANES // 2
    while off >= 1:
        v = v[:off] + v[off:2 * off]
        off //= 2
    return float(v[0])


def model_sum(x, y, take=None):
    return butterfly(lane_accumulators(np.asarray(x, np.float64), np.asarray(y, np.float64), take))


# ---- sentinel inputs --------------------------------------------------------------------------------------------------------

def sentinel_indices(n):
    """Where the kernel changes hands in a system of n elements, by name (empty where there is none):
      ends          0, n - 2, n - 1;
      wave_edges    in every tile, the full ones and the ragged one, both elements of the wavefront's first pair (lane 0) and of
                    its last pair (lane 63): where the butterfly's outermost lanes sit;
      ragged        the first element of the ragged tile (the straight-line full tiles hand over to the guarded body) and the
                    last pair inside n;
      half_pair     n - 1 for odd n: the first element of a pair whose second lies beyond n."""
    ntile = -(-n // TILE)
    edges = (np.arange(ntile, dtype=np.int64)[:, None] * TILE + np.array([0, 1, TILE - 2, TILE - 1], dtype=np.int64)[None, :]).ravel()
    full = n // TILE * TILE
    ragged = [full, (n - 1) // 2 * 2, (n - 1) // 2 * 2 + 1] if full < n else []
    return {"ends": np.unique(np.array([k for k in (0, n - 2, n - 1) if k >= 0], dtype=np.int64)),
            "wave_edges": edges[edges < n],
            "ragged": np.array([k for k in ragged if k < n], dtype=np.int64),
            "half_pair": np.array([n - 1] if n % 2 else [], dtype=np.int64)}


def all_sentinels(n):
    return np.unique(np.concatenate(list(sentinel_indices(n).values())))


def planted_input(n, rng, prev=None, background=0.125):
    """N(0, background^2) everywhere, +-2^e (e in 0..3) at every sentinel -- large beside the background --, the two elements of
    a pair DISTINCT (a sum that takes the partner's element is off by at least 1 times the other operand), never the value `prev`
    has there (d = w1 - f is then at least 1 in magnitude)."""
    x = rng.standard_normal(n) * background
    idx = all_sentinels(n)
    val = np.ldexp(1.0, rng.integers(0, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    if prev is not None:
        same = val == prev[idx]
        val[same] = -val[same]
    x[idx] = val
    planted = set(idx.tolist())
    for i in idx.tolist():                       # partners: distinct, without undoing the condition on prev
        j = i ^ 1
        if i % 2 == 0 and j in planted and x[i] == x[j]:
            x[j] = -x[j] if prev is None or -x[j] != prev[j] else 2.0 * x[j] if 2.0 * x[j] != prev[j] else 4.0 * x[j]
    return x


# ---- the shapes of tests/test_batch_waves_gpu.py ------------------------------------------------------------------------------

def shapes(cap):
    """vlen of the three-layer test: one element, one pair, a pair and a half; one tile -1 / 0 / +1; two tiles -1 / +1; eight
    tiles + 3; the cap and the cap - 1."""
    return sorted({1, 2, 3, 127, 128, 129, 255, 257, several_tiles(cap), cap - 1, cap})


def several_tiles(cap):
    """1027 -- eight full tiles, a pair and the half pair of an odd n -- where the cap allows it; under a smaller cap the same
    shape with the most full tiles that fit: cap - 128 + 3."""
    return 1027 if cap >= 1027 else cap - 128 + 3


MVECS = (1, 3, 10)
WIDTH_SHAPE = (129, 32)         # every group count of the sweep of four
NSYS = 11                       # the last workgroup has one absent wavefront
STEP_LENGTHS = (1, 129, 1027)
CPU_LENGTHS = (129, 257, 1027)


# ---- the large case: the slot allocations pass 2^32 bytes -------------------------------------------------------------------------

BYTES_4G = 2 ** 32
LARGE_MVEC = 3
MAX_ACTIVE = 9


def large_shape(cap):
    """-> dict for vlen = cap: nsys so that each slot allocation passes 2^32 bytes by two systems; the systems that run (the first,
    the last, the one whose slots straddle byte 2^32 or the two beside the boundary, and their neighbours); the masked witnesses
    where a byte offset that lost its upper half would land, and the masked neighbours of the active ones."""
    vlen, mvec = cap, LARGE_MVEC
    sys_bytes = 8 * slot_stride(vlen) * (mvec + 1)
    kb = BYTES_4G // sys_bytes                    # the system that holds byte 2^32 (or starts on it)
    nsys = kb + 3
    active = sorted({0, kb - 1, kb, kb + 1, nsys - 1})
    wit = set()
    for k in active:
        wit |= {(k * sys_bytes) % BYTES_4G // sys_bytes, ((k + 1) * sys_bytes - 1) % BYTES_4G // sys_bytes, k - 1, k + 1}
    wit = sorted(j for j in wit if 0 <= j < nsys and j not in active)
    return {"nsys": nsys, "vlen": vlen, "mvec": mvec, "boundary": kb, "active": active, "witnesses": wit, "sys_bytes": sys_bytes}


def large_bytes(sh):
    """{name: bytes} of every device allocation the large case holds at once (the control blocks: nka_ctl.hpp)."""
    m1 = sh["mvec"] + 1
    m1p = m1 + 32
    ic = 16 + 2 * (m1 + 1) + 2 * m1p
    dc = 2 + (m1 + 1) ** 2 + (m1 + 1) + m1p + (2 + 2 * sh["mvec"]) + 16
    each = sh["sys_bytes"] * sh["nsys"]
    return {"w": each, "v": each, "ic": 4 * ((ic + 31) // 32 * 32) * sh["nsys"], "dc": 8 * ((dc + 31) // 32 * 32) * sh["nsys"],
            "F": 8 * sh["vlen"] * sh["nsys"], "mask": 4 * sh["nsys"]}
