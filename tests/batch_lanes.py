"""The layout arithmetic of the lane batch (include/nka_hip_batch.h, LANES; nka_amd/csrc/host_logic.hpp: lanes_lds,
lanes_group, lanes_slot_offset) restated in Python, and the shape of the large-offset case of tests/test_batch_lanes_gpu.py.
No GPU here: tests/test_batch_lanes_cpu.py holds every function below against the C program's table, and against the
library where it loads."""

LDS_BUDGET = 64 * 1024      # kLanesLdsBudget
MAX_VLEN = 64               # NKA_HIP_BATCH_LANES_MAX_VLEN
MAX_MVEC = 32
BYTES_4G = 2 ** 32
MAX_ACTIVE = 9
MAX_BYTES = 12 * 2 ** 30


def lane_bytes(mvec):
    """LDS of one lane's working copy: h, c, red, cc (doubles, an odd stride) and next, prev, ps, cs, hdr (int32, an odd stride)."""
    m1 = mvec + 1
    nd = (m1 + 1) ** 2 + (m1 + 1) + (2 + 2 * mvec) + m1
    ni = 2 * (m1 + 1) + 2 * m1 + 8
    return 8 * (nd | 1) + 4 * (ni | 1)


def lanes_group(mvec):
    """Systems per workgroup: the most copies the LDS budget holds, at most one wavefront."""
    return min(64, LDS_BUDGET // lane_bytes(mvec))


def ngroup(nsys, G):
    return -(-nsys // G)


def group_stride(vlen, mvec, G):
    """Doubles of one group in each of the two slot allocations."""
    return (mvec + 1) * vlen * G


def slot_offset(vlen, mvec, G, sys, slot, i):
    """Element i of slot `slot` (1-based) of system sys, in doubles from the start of the allocation."""
    return (((sys // G) * (mvec + 1) + (slot - 1)) * vlen + i) * G + sys % G


def alloc_elems(vlen, mvec, nsys, G=None):
    G = lanes_group(mvec) if G is None else G
    return ngroup(nsys, G) * group_stride(vlen, mvec, G)


def vector_bytes(vlen, mvec, nsys, G=None):
    """nka_hip_batch_vector_bytes of a lane batch: both slot allocations, the last group whole."""
    return 16 * alloc_elems(vlen, mvec, nsys, G)


# ---- the large case: both slot allocations pass 2^32 bytes --------------------------------------------------------------------

LARGE_VLEN, LARGE_MVEC = 64, 32


def large_shape(G=None):
    """-> dict: nsys, G, the group whose slots straddle byte 2^32 of w and of v, the systems that run (system 0, the last one,
    every system of the straddling group, the neighbour below it; the last system is the neighbour above), and the masked
    witnesses where a byte offset that lost its upper half would land (the systems of the groups at the wrapped offsets, and
    the masked neighbours of the active ones)."""
    vlen, mvec = LARGE_VLEN, LARGE_MVEC
    G = lanes_group(mvec) if G is None else G
    gs = group_stride(vlen, mvec, G)
    gb = BYTES_4G // (8 * gs)                      # the group that holds byte 2^32
    assert 8 * gs * gb < BYTES_4G < 8 * gs * (gb + 1), "no group straddles the boundary"
    nsys = (gb + 1) * G + min(2, G)                # one group above the boundary, ragged where G allows
    last = nsys - 1
    active = sorted({0, last, gb * G - 1} | set(range(gb * G, (gb + 1) * G)))
    wit = set()
    for k in active:
        wrapped = (8 * (k // G) * gs) % BYTES_4G // (8 * gs)      # the group a 32-bit byte offset of k's group base lands in
        tail = (8 * ((k // G) + 1) * gs - 1) % BYTES_4G // (8 * gs)   # ... and of the last byte of k's group
        for g in (wrapped, tail):
            wit |= set(range(g * G, min((g + 1) * G, nsys)))
        wit |= {k - 1, k + 1}
    wit = sorted(j for j in wit if 0 <= j < nsys and j not in active)
    return {"nsys": nsys, "G": G, "group": gb, "active": active, "witnesses": wit, "vlen": vlen, "mvec": mvec}


def large_bytes(sh):
    """{name: bytes} of every device allocation the large case holds at once (the control blocks: nka_ctl.hpp)."""
    m1 = sh["mvec"] + 1
    m1p = m1 + 32
    ic = 16 + 2 * (m1 + 1) + 2 * m1p
    dc = 2 + (m1 + 1) ** 2 + (m1 + 1) + m1p + (2 + 2 * sh["mvec"]) + 16
    each = 8 * alloc_elems(sh["vlen"], sh["mvec"], sh["nsys"], sh["G"])
    return {"w": each, "v": each, "ic": 4 * ((ic + 31) // 32 * 32) * sh["nsys"], "dc": 8 * ((dc + 31) // 32 * 32) * sh["nsys"],
            "F": 8 * sh["vlen"] * sh["nsys"], "mask": 4 * sh["nsys"]}


# ---- the call sequences of tests/test_batch_lanes_gpu.py --------------------------------------------------------------------

PAD = 7.25      # what F and X hold wherever no active system owns the element


def num_calls(mvec):
    """More than mvec + 2 updates for the systems that start last (three calls late): capacity drops."""
    return mvec + 8


def script(vlen, nsys, mvec, seed):
    """-> [(op, arg, mask)]: ("update", X float64[nsys, vlen], mask int32[nsys]) | ("relax", None, mask) | ("restart", None, mask).
    Every system draws from its own batch_seq.Sequence (fresh, dependent, repeated and zero inputs).  On top of that
      system k sits out the first k % 4 updates          -> the lanes of a wavefront hold lists of different length
      k % 5 == 0: fresh inputs only                      -> its list fills: capacity drops
      k % 5 == 2: its 4th input repeats its 3rd          -> s == 0, a relax inside the update, in some systems only
      k % 5 == 3: its 4th input makes d_4 = 2 d_3        -> a dependence drop, in some systems only
      a masked relax (k % 3 == 0) after call mvec // 2 + 3 and a masked restart (k % 4 == 1) two calls later.
    Rows of systems that sit out hold PAD."""
    import numpy as np

    import batch_seq as B
    seqs = [B.Sequence(vlen, seed + 1000 * k) for k in range(nsys)]
    hist = [[] for _ in range(nsys)]
    ops = []
    for t in range(num_calls(mvec)):
        mask = np.array([1 if t >= k % 4 else 0 for k in range(nsys)], np.int32)
        X = np.full((nsys, vlen), PAD)
        for k in range(nsys):
            if not mask[k]:
                continue
            x = seqs[k].next()
            if k % 5 == 0:
                x = seqs[k].rng.standard_normal(vlen)      # fresh inputs only: the list fills, capacity drops
            elif len(hist[k]) == 3 and k % 5 == 2:
                x = hist[k][-1].copy()
            elif len(hist[k]) == 3 and k % 5 == 3:
                x = hist[k][-1] - 2.0 * (hist[k][-2] - hist[k][-1])
            hist[k].append(x)
            X[k] = x
        ops.append(("update", X, mask))
        if t == mvec // 2 + 3:
            ops.append(("relax", None, np.array([1 if k % 3 == 0 else 0 for k in range(nsys)], np.int32)))
        if t == mvec // 2 + 5:
            ops.append(("restart", None, np.array([1 if k % 4 == 1 else 0 for k in range(nsys)], np.int32)))
    return ops
