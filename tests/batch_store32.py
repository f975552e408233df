"""Shared by tests/test_batch_store32_cpu.py and tests/test_batch_store32_gpu.py (binary32 storage of a batch's normalised
subspace vectors, nka_hip_batch_create_stored; include/nka_hip_batch.h, STORAGE): the rounding q(), the host model of one
update under that contract, the expected allocation sizes and the shape of the large case.  No GPU here."""
import numpy as np

import batch_large as G

STORE_F64, STORE_F32 = 0, 1


def q(x):
    """binary64 -> binary32, round to nearest even (subnormals kept, beyond the range +-Inf), widened back exactly."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def q_trunc(x):
    """The WRONG rounding the sentinels of the CPU test must catch: towards zero (the low 29 bits of the significand cut)."""
    bits = np.asarray(x, dtype=np.float64).view(np.uint64) & np.uint64(0xFFFFFFFFE0000000)
    return bits.view(np.float64)


# ---- the host model of one update ------------------------------------------------------------------------------------------

class HostModel:
    """One system under the contract of the STORAGE paragraph, flavour C (compact storage), the list logic through the oracle's
    scalar_step and the sums by np.dot -- a model of the arithmetic, not of the kernel's sum order.  store32=False: the same
    statements without q(), i.e. binary64 storage."""

    def __init__(self, oracle, n, mvec, store32=True):
        self.ora = oracle.OracleNKA(n, mvec, 2)
        self.n, self.m = n, mvec
        self.rnd = q if store32 else (lambda x: x)
        self.W, self.V = {}, {}          # slot -> stored normalised w', v' - w' (as a later load returns them)
        self.pw = self.pv = None         # the raw pending pair, binary64

    def update(self, f_in):
        m = self.m
        st0 = self.ora.state()
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        hrow, rhs = np.zeros(m + 2), np.zeros(m + 2)
        s, normed = 0.0, False
        if pending:
            d = self.pw - f_in
            s = np.sqrt(np.dot(d, d))
            normed = not s == 0.0
        if normed:
            with np.errstate(all="ignore"):
                w1n = self.rnd(d / s)
                v1n = self.rnd(self.pv / s - w1n)
            rhs[first0] = np.dot(f_in, w1n)
            for slot in olders:
                hrow[slot] = np.dot(w1n, self.W[slot])
        for slot in olders:
            rhs[slot] = np.dot(f_in, self.W[slot])
        self.ora.scalar_step(float(s), hrow, rhs)
        st = self.ora.state()
        comb = st.list_order()[1:]
        if normed:
            self.W[first0], self.V[first0] = w1n, v1n
        x = f_in.copy()
        with np.errstate(all="ignore"):
            for slot in comb:
                x = x + st.c[slot - 1] * self.V[slot]
        self.W = {slot: self.W[slot] for slot in comb}
        self.V = {slot: self.V[slot] for slot in comb}
        self.pw, self.pv = f_in.copy(), x.copy()
        return x


def solve_on_the_model(oracle, store32, mvec, tol):
    """batch_step.solve_problem() through HostModel with the stop rule of nka_hip_batch_accel_step (<=, relative to the first
    norm) -> the iteration at which each system retired, -1 where it did not within SOLVE_REPLAYS calls."""
    import batch_step as T
    d, eps, b, x = T.solve_problem()
    accs = [HostModel(oracle, T.SOLVE_VLEN, mvec, store32) for _ in range(T.SOLVE_NSYS)]
    retired = np.full(T.SOLVE_NSYS, -1)
    thr = np.zeros(T.SOLVE_NSYS)
    r0 = None
    for it in range(T.SOLVE_REPLAYS):
        f = T.solve_residual(np, x, d, eps, b)
        r = np.sqrt((f * f).sum(axis=1))
        if it == 1:
            thr = tol * r0
        for k in range(T.SOLVE_NSYS):
            if retired[k] >= 0:
                continue
            if r[k] <= thr[k]:
                retired[k] = it
                continue
            x[k] = x[k] - accs[k].update(f[k].copy())
        if it == 0:
            r0 = r
    return retired


# ---- allocations -----------------------------------------------------------------------------------------------------------

def slot_stride(vlen):
    return (vlen + 31) // 32 * 32


def vector_bytes(nsys, vlen, mvec, storage):
    """Device memory of the stored vectors: binary64 2 nsys stride 8 (mvec + 1); binary32 2 nsys stride (4 (mvec + 1) + 8)."""
    st = slot_stride(vlen)
    return 2 * nsys * st * (8 * (mvec + 1) if storage == STORE_F64 else 4 * (mvec + 1) + 8)


def pieces(nsys, vlen, mvec, storage):
    """Brute force: [(allocation, first byte, end byte)] of every row the batch owns -- slot rows in `w` and `v`, pending rows in
    `pw` and `pv` -- written out one by one."""
    st, eb = slot_stride(vlen), (4 if storage == STORE_F32 else 8)
    out = []
    for sys in range(nsys):
        for slot in range(1, mvec + 2):
            lo = (sys * (mvec + 1) + (slot - 1)) * st * eb
            for a in ("w", "v"):
                out.append((a, lo, lo + vlen * eb))
        if storage == STORE_F32:
            for a in ("pw", "pv"):
                out.append((a, sys * st * 8, sys * st * 8 + vlen * 8))
    return out


# ---- the large case --------------------------------------------------------------------------------------------------------
# A binary32 batch whose w / v allocation crosses 2^31 ELEMENTS and 2^32 BYTES: the shape "slots" of tests/batch_large.py (16 384
# x mvec 32 x 3976 systems).  Its elements lie where the binary64 batch's do, so the systems on the 2^31-element boundary are
# batch_large's; a float's byte offset is half a double's, so 2^32 bytes are crossed at 2^30 elements.
LARGE = G.SHAPES["slots"]
BYTES_4G_FLOATS = 2 ** 30


def large_active():
    """Systems that run: system 0, the last one, and the system that straddles each boundary of a float allocation -- 2^30
    elements = 2^32 bytes, and 2^31 elements -- with its neighbour below and above.  Sorted; eight systems."""
    have = {0, LARGE.nsys - 1}
    for B in (BYTES_4G_FLOATS, G.ELEMS_2G):
        k = G.on_boundary(LARGE, "w", B)
        have |= {k - 1, k, k + 1}
    return sorted(have)


def large_witnesses():
    """Inactive systems where a slot offset that lost its upper half would land, in elements and in bytes of a float."""
    act = set(large_active())
    ss = G.sys_stride(LARGE)
    out = set()
    for k in act:
        cand = [k - 1, k + 1, (k * ss) % 2 ** 32 // ss, (k * ss * 4) % 2 ** 32 // 4 // ss, (k * ss) % 2 ** 31 // ss]
        out |= {j for j in cand if 0 <= j < LARGE.nsys and j not in act}
    return sorted(out)


def large_bytes():
    """Everything the GPU test of the large case holds at once: the batch's vectors and control blocks, F, the mask."""
    a = G.allocations(LARGE)
    return vector_bytes(LARGE.nsys, LARGE.vlen, LARGE.mvec, STORE_F32) + a["ic"] + a["dc"] + a["F"] + a["per system"]
