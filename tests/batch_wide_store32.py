"""Shared by tests/test_batch_wide_store32_cpu.py and tests/test_batch_wide_store32_gpu.py (the WIDE batch with binary32 storage of
its normalised subspace vectors, nka_hip_batch_create_wide_stored; include/nka_hip_batch.h, WIDE STORED): the allocation formula, the
host model of a chunked sum on the operands the contract names, the solve the GPU test runs, and the shape of the large case.  No GPU
here.

A sum of such a batch is the wide sum (tests/batch_wide.py) of the operands ACTUALLY USED: the widened stored values, which are
binary64 numbers, and q(w1') (tests/batch_store32.py: q).  Widening is exact and the narrowing precedes the product, so K =
batch_wide.wide_k(n) does not change."""
import numpy as np

import batch_large as G
import batch_store32 as S32
import batch_wide as BW
import batch_wide_weights as WW

STORE_F64, STORE_F32 = S32.STORE_F64, S32.STORE_F32


def vector_bytes(nsys, vlen, mvec, storage):
    """The STORAGE formula at the wide batch's slot stride, which is the narrow batch's: vlen rounded up to 32."""
    return S32.vector_bytes(nsys, vlen, mvec, storage)


def create_through_the_new_entry(nsys, vlen, mvec, step, storage, flavor=2):
    """An nka_batch whose handle comes from nka_hip_batch_create_wide_stored with ANY storage (init(..., wide_storage=STORE_F64)
    is the default and goes through the older entries) -- on torch's current stream, followed like init's."""
    import ctypes as C

    import nka_amd
    import torch
    from nka_amd.batch import _check
    b = nka_amd.nka_batch()
    h = C.c_void_p()
    device = torch.cuda.current_device()
    stream = torch.cuda.current_stream(device).cuda_stream
    _check(b._L.nka_hip_batch_create_wide_stored(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                 C.c_void_p(stream), 1 if step else 0, int(storage)),
           "nka_hip_batch_create_wide_stored", b._L)
    b._h, b._device, b._nsys, b._vlen, b._mvec = h, device, int(nsys), int(vlen), int(mvec)
    b._stream, b._follow_torch_stream = int(stream), True
    return b


# ---- the host model of a chunked sum on the contract's operands ---------------------------------------------------------------------

def operands(rng, n, C, weighted=False):
    """(first operand, second operand, the unrounded w1', s) of <w1', w_p> as a binary32 wide batch forms it: w1' = q(fl(d/s)) with d a
    planted difference, w_p a widened stored vector, the first operand fl(w q(w1')) under weights."""
    d = BW.wide_planted_input(n, rng) - BW.wide_planted_input(n, rng)
    s = np.sqrt(np.dot(d, d))
    raw = d / s
    wp = S32.q(BW.wide_planted_input(n, rng) / 37.0)
    first = S32.q(raw)
    if weighted:
        first = WW.draw_weights(n, rng, C) * first
    return first, wp, raw, s


# ---- a whole solve: ragged, weighted, wide, binary32 -----------------------------------------------------------------------------------

def solve_on_the_model(oracle, C, store32=True):
    """The ragged weighted solve of tests/batch_wide_weights.py through batch_store32.HostModel with the weighted dot product (np.dot
    sums; a model of the arithmetic, not of the sum order) -> the iteration at which each system retired, -1 where it did not within
    WW.SOLVE_REPLAYS calls."""
    d, eps, b, x, left, right = WW.solve_problem(C)
    lens, w = WW.solve_lengths(C), WW.solve_weights(C)
    accs = [WeightedModel(oracle, int(L), WW.SOLVE_MVEC, w[k, :L].copy(), store32) for k, L in enumerate(lens)]
    retired = np.full(WW.SOLVE_NSYS, -1)
    tol = np.zeros(WW.SOLVE_NSYS)
    r0 = None
    for it in range(WW.SOLVE_REPLAYS):
        f = WW.solve_residual(np, x, d, eps, b, left, right)
        r = np.array([np.sqrt(np.dot(w[k, :L] * f[k, :L], f[k, :L])) for k, L in enumerate(lens)])
        if it == 1:
            tol = WW.SOLVE_TOL * r0
        for k, L in enumerate(lens):
            if retired[k] >= 0:
                continue
            if r[k] <= tol[k]:
                retired[k] = it
                continue
            x[k, :L] = x[k, :L] - accs[k].update(f[k, :L].copy())
        if it == 0:
            r0 = r
    return retired


class WeightedModel(S32.HostModel):
    """batch_store32.HostModel with fl(w x) as the first operand of every sum (include/nka_hip_batch.h, WEIGHTS)."""

    def __init__(self, oracle, n, mvec, w, store32=True):
        super().__init__(oracle, n, mvec, store32)
        self.w = w

    def update(self, f_in):
        m, w = self.m, self.w
        st0 = self.ora.state()
        order0, pending, first0 = st0.list_order(), st0.pending, st0.first
        olders = order0[1:] if pending else order0
        hrow, rhs = np.zeros(m + 2), np.zeros(m + 2)
        s, normed = 0.0, False
        if pending:
            d = self.pw - f_in
            s = np.sqrt(np.dot(w * d, d))
            normed = not s == 0.0
        if normed:
            with np.errstate(all="ignore"):
                w1n = self.rnd(d / s)
                v1n = self.rnd(self.pv / s - w1n)
            rhs[first0] = np.dot(w * f_in, w1n)
            for slot in olders:
                hrow[slot] = np.dot(w * w1n, self.W[slot])
        for slot in olders:
            rhs[slot] = np.dot(w * f_in, self.W[slot])
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


# ---- the large case --------------------------------------------------------------------------------------------------------------------
# A binary32 wide batch whose w / v allocation crosses 2^31 ELEMENTS and 2^32 BYTES: the shape "wide-slots" of tests/batch_large.py
# (4609 x mvec 32 x 14 030 systems, three chunks each).  A float's byte offset is half a double's: 2^32 bytes are crossed at 2^30
# elements.
LARGE = G.SHAPES["wide-slots"]
BYTES_4G_FLOATS = 2 ** 30
MAX_ACTIVE = 9
MAX_BYTES = 20 * 2 ** 30


def large_boundaries():
    """{boundary in elements: the system whose float slots straddle it}"""
    return {B: G.on_boundary(LARGE, "w", B) for B in (BYTES_4G_FLOATS, G.ELEMS_2G)}


def large_active():
    """Systems that run: system 0, the last one, and the system on each boundary with its neighbour below and above.  Sorted."""
    have = {0, LARGE.nsys - 1}
    for k in large_boundaries().values():
        have |= {k - 1, k, k + 1}
    return sorted(have)


def large_witnesses():
    """Inactive systems where a slot offset that lost its upper half would land -- in elements, in bytes of a float, and in bytes of a
    double of the pending rows --, and the inactive neighbours."""
    act = set(large_active())
    ss, st = G.sys_stride(LARGE), G.slot_stride(LARGE.vlen)
    out = set()
    for k in act:
        cand = [k - 1, k + 1, (k * ss) % 2 ** 32 // ss, (k * ss * 4) % 2 ** 32 // 4 // ss, (k * ss) % 2 ** 31 // ss,
                (k * st * 8) % 2 ** 32 // 8 // st]
        out |= {j for j in cand if 0 <= j < LARGE.nsys and j not in act}
    return sorted(out)


def large_bytes():
    """Everything the GPU test of the large case holds at once: the batch's vectors, control blocks, partial sums and plan, F, the
    mask."""
    a = G.allocations(LARGE)
    return vector_bytes(LARGE.nsys, LARGE.vlen, LARGE.mvec, STORE_F32) + a["ic"] + a["dc"] + a["part"] + a["plan"] + a["F"] + a["per system"]
