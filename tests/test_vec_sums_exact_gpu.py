"""Every reduction of the abstract-vector workspace (nka_amd/csrc/vec_ops.hip) against the exact sums (tests/exact_sums.py).

THE FAST SUMS.  k_dot, k_dot_many, k_dot_pair_many, k_update_norm2, k_scale_dot_pair_many, k_scale_dot_pair_many_win (with
its pure-read and DD forms) and k_finalize_rows, through the C entries that launch them: every value an entry returns is
held to the correctly rounded sum of the operands AS THE KERNEL FORMS THEM (numpy on the host: IEEE, left to right, no
fma) within gamma(K) sum|x y|, K = exact_sums.vec_k for the grid that entry launches at that length and count
(exact_sums.vec_grid) -- derived from the code, not tuned.  The operands carry planted sentinels where the kernels change
hands (exact_sums.vec_sentinel_indices); tests/test_exact_sums_cpu.py shows that losing or doubling any one of them
breaks the bound at these shapes.  Norms are held as sqrt of a sum inside the bound, one ulp either side.  The host result
arrays are four entries longer than the list, with canaries: no padded column reaches the host.  16-byte aligned operands
(the 16-byte kernels, the rolling-window kernels) and every operand 8 bytes off (the VEC = 1 forms).

THE REFERENCE-ORDER dot() (nka_hip_vec_set_sum_order: k_dot_ordered, k_dot_chain) has exactly one right answer per input:
held on the BITS to numpy's strictly sequential sum, at the lengths where the two kernels and the chain's groups and
blocks change hands, under the four alignments of (x, y); the fused reductions refuse in that mode and touch nothing.
"""
import ctypes as C
import json
import math
import os
import re
import struct
import types

import numpy as np
import pytest

import exact_sums as X
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

AUTO, REFERENCE_ORDER, BLOCKED, BLOCKED_ROUNDED = 0, 1, 2, 3        # include/nka_hip.h: NKA_HIP_SUMS_*
EINVAL, ESTATE = -1, -5                                             # include/nka_hip.h: NKA_HIP_EINVAL, NKA_HIP_ESTATE
CANARY = -7.25e77
EXTRA = 4                           # the host result arrays are this much longer than the list; all of it stays CANARY
BIG = 1 << 19                       # from this length on at most two vectors ys: the host's fsum is the cost there
COUNTS = (0, 1, 2, 3, 4, 5)         # the issue's 0, 1, 3, 4, 5, and 2 for the lengths beyond BIG
WORST = {}                          # entry -> [worst |got - exact| / (u sum|xy|), the K it was held to, where]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """At the end of the module: per entry, the worst |got - exact| / (u sum|xy|) seen and the K it was held to."""
    yield
    import parity_util as P
    rows = {}
    for entry, (ratio, k, where) in sorted(WORST.items()):
        rows[entry] = {"worst_err_over_u_sum_abs": ratio, "k": k, "where": where}
        line = f"vec sums {entry}: worst |got - exact| = {ratio:.3f} u sum|xy| against K = {k} there ({where})"
        print(line)
    out = P.dump_dir(ROOT)
    if rows and out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "vec_sums_exact_worst.json"), "w") as fh:
            json.dump(rows, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def env():
    import torch
    import nka_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    acc = nka_amd.nka().init(1, 1)
    _, ncu = acc.device_info()
    acc.delete()
    assert ncu >= 1
    L = nka_amd.load()
    h = C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(h), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    yield types.SimpleNamespace(L=L, h=h, torch=torch, ncu=ncu, pools={})
    L.nka_hip_vec_workspace_destroy(h)


def P(t):
    return C.c_void_p(t.data_ptr())


def _record(entry, ratio, k, where):
    r = WORST.setdefault(entry, [0.0, 0, ""])
    if ratio >= r[0]:
        r[:] = [ratio, k, where]


def _hold(entry, what, got, ex, tot, k, where):
    """|got - exact| <= gamma(K) sum|xy|; NaN and Inf exactly where the exact sum has them."""
    if math.isnan(ex):
        assert math.isnan(got), (entry, what, where, got)
        return
    if math.isinf(ex):
        assert got == ex, (entry, what, where, got, ex)
        return
    err = abs(got - ex)
    assert err <= X.gamma(k) * tot, (entry, what, where, got, ex, err / (X.U * tot) if tot else err, k)
    if tot > 0:
        _record(entry, err / (X.U * tot), k, f"{what} {where}")


def _hold_norm(entry, what, norm, ex, tot, k, where):
    """norm == sqrt(s) for some s within the bound of the exact sum: between the square roots of the two ends of the
    interval, widened by one ulp.  (The recorded ratio is that of norm * norm: it carries the rounding of the root.)"""
    if math.isnan(ex):
        assert math.isnan(norm), (entry, what, where, norm)
        return
    if math.isinf(ex):
        assert norm == ex, (entry, what, where, norm, ex)
        return
    lo, hi = max(ex - X.gamma(k) * tot, 0.0), ex + X.gamma(k) * tot
    assert np.nextafter(math.sqrt(lo), -math.inf) <= norm <= np.nextafter(math.sqrt(hi), math.inf), \
        (entry, what, where, norm, math.sqrt(ex), k)
    if tot > 0:
        _record(entry, abs(norm * norm - ex) / (X.U * tot), k, f"{what} {where} (norm squared)")


class Ops:
    """The operands of one shape on the host (exact_sums.vec_operands: never changed) and on the device, with every
    exact sum computed once."""

    def __init__(self, env, n, grids, vec, count, seed):
        self.env, self.n, self.vec = env, n, vec
        self.o = X.vec_operands(n, grids, vec, np.random.default_rng(seed), count)
        self.off = 0 if vec == 2 else 1          # vec == 1: every operand 8 bytes off a 16-byte boundary
        self.memo, self.cache = {}, {}

    def arr(self, key):
        return self.o["ys"][int(key[1:])] if key[0] == "y" else self.o[key]

    def up(self, a):
        """A fresh device copy, 16-byte aligned or 8 bytes off."""
        torch = self.env.torch
        t = torch.empty(a.size + 2, dtype=torch.float64, device="cuda")
        v = t[self.off:self.off + a.size]
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 8 * self.off
        return v

    def ro(self, key):
        """The device copy of an operand that no entry under test writes."""
        if key not in self.cache:
            self.cache[key] = self.up(self.arr(key))
        return self.cache[key]

    def untouched(self, *keys):
        for key in keys:
            assert _bits_equal(self.cache[key].cpu().numpy(), self.arr(key)), (key, "a pure-read entry wrote an operand")

    def ys_ptrs(self, count, base=0):
        return (C.c_void_p * max(count, 1))(*[self.ro(f"y{base + j}").data_ptr() for j in range(count)])

    def exact(self, a, b):
        if (a, b) not in self.memo:
            x, y = self.arr(a), self.arr(b)
            ex = X.exact_dot(x, y)
            self.memo[a, b] = (ex, X.abs_dot(x, y) if math.isfinite(ex) else math.inf)
        return self.memo[a, b]

    def hold(self, entry, got, a, b, k, where):
        ex, tot = self.exact(a, b)
        _hold(entry, f"<{a},{b}>", got, ex, tot, k, (self.n, self.vec, where))

    def hold_norm(self, entry, norm, a, k, where):
        ex, tot = self.exact(a, a)
        _hold_norm(entry, f"<{a},{a}>", norm, ex, tot, k, (self.n, self.vec, where))


def _out(count):
    return np.full(count + EXTRA, CANARY)


def _canaries(count, *arrs):
    for a in arrs:
        assert (a[count:] == CANARY).all(), ("a padded column reached the host", count, a[count:])


# ---- the grid of every launch an entry makes, as (first vector, vectors, G) per launch --------------------------------------

def _win_nloads(width, vec):
    """scale_dot_pair_many_impl (vec_ops.hip): the window kernel (22) for aligned operands, else nv + 3."""
    return X.VEC_LOADS_PER_CU if vec == 2 else X.vec_width(width) + 3


def _fixed_groups(count, at_least_one):
    """Launch groups of kManyMax (dot_many :1112, dot_pair_many :1164-1197: 24 + the rest)."""
    out = [(b, min(X.VEC_MANY_MAX, count - b)) for b in range(0, count, X.VEC_MANY_MAX)]
    return out or ([(0, 0)] if at_least_one else [])


def launches(entry, n, ncu, vec, count):
    if entry in ("dot", "update_norm2"):
        return [(0, 0, X.vec_grid(n, ncu, vec, 2))]
    if entry == "dot_many":
        return [(b, m, X.vec_grid(n, ncu, vec, X.vec_width(m) + 1)) for b, m in _fixed_groups(count, False)]
    if entry == "dot_pair_many":
        return [(b, m, X.vec_grid(n, ncu, vec, X.vec_width(m) + 2)) for b, m in _fixed_groups(count, True)]
    if entry == "scale_dot_pair_many":      # one fused launch for the first 24, dot_pair_many(w, f) for the rest (:1487)
        m = min(X.VEC_MANY_MAX, count)
        rest = [(X.VEC_MANY_MAX + b, r, g) for b, r, g in launches("dot_pair_many", n, ncu, vec, count - m)] if count > m else []
        return [(0, m, X.vec_grid(n, ncu, vec, _win_nloads(m, vec)))] + rest
    assert entry in ("dot_pair_many_scaled", "diff_norm_dot_pair_many")     # balanced groups (:1346, :1378)
    out, base = [], 0
    for wdt in X.vec_groups(count):
        out.append((base, wdt, X.vec_grid(n, ncu, vec, _win_nloads(wdt, vec))))
        base += wdt
    return out


def _ks(entry, n, ncu, vec, count):
    """K of the scalar sums (the first launch) and of each listed vector's sums."""
    ls = launches(entry, n, ncu, vec, count)
    per = {}
    for base, m, g in ls:
        for j in range(base, base + m):
            per[j] = X.vec_k(n, g, vec)
    return X.vec_k(n, ls[0][2], vec) if ls else 0, per


# ---- the entries ----------------------------------------------------------------------------------------------------------------

def run_dot(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    k0, _ = _ks("dot", n, env.ncu, ops.vec, 0)
    r = C.c_double(CANARY)
    assert L.nka_hip_vec_dot(h, n, P(ops.ro("x")), P(ops.ro("z")), C.byref(r)) == 0
    ops.hold("dot", r.value, "x", "z", k0, tag)
    assert L.nka_hip_vec_norm2(h, n, P(ops.ro("x")), C.byref(r)) == 0
    ops.hold_norm("norm2", r.value, "x", k0, tag)
    ops.untouched("x", "z")


def run_dot_many(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    _, kj = _ks("dot_many", n, env.ncu, ops.vec, count)
    vals = _out(count)
    assert L.nka_hip_vec_dot_many(h, n, P(ops.ro("x")), ops.ys_ptrs(count), count, vals.ctypes.data_as(dp)) == 0
    _canaries(count, vals)
    for j in range(count):
        ops.hold("dot_many", vals[j], "x", f"y{j}", kj[j], (tag, count))


def run_dot_pair_many(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    k0, kj = _ks("dot_pair_many", n, env.ncu, ops.vec, count)
    v0, v1, cross = _out(count), _out(count), C.c_double(CANARY)
    assert L.nka_hip_vec_dot_pair_many(h, n, P(ops.ro("x")), P(ops.ro("z")), ops.ys_ptrs(count), count,
                                       v0.ctypes.data_as(dp), v1.ctypes.data_as(dp), C.byref(cross)) == 0
    _canaries(count, v0, v1)
    ops.hold("dot_pair_many", cross.value, "x", "z", k0, (tag, count))
    for j in range(count):
        ops.hold("dot_pair_many", v0[j], "x", f"y{j}", kj[j], (tag, count))
        ops.hold("dot_pair_many", v1[j], "z", f"y{j}", kj[j], (tag, count))


def run_update_norm2(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    k0, _ = _ks("update_norm2", n, env.ncu, ops.vec, 0)
    for store in (0, 1):
        zd, s = ops.up(ops.o["z"]), C.c_double(CANARY)
        assert L.nka_hip_vec_update_norm2(h, n, P(zd), X.VEC_A, P(ops.ro("x")), store, C.byref(s)) == 0
        ops.hold_norm("update_norm2", s.value, "r", k0, (tag, store))
        assert _bits_equal(zd.cpu().numpy(), ops.o["r"] if store else ops.o["z"]), (n, store)


def run_scale_dot_pair_many(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    k0, kj = _ks("scale_dot_pair_many", n, env.ncu, ops.vec, count)
    for subtract in (0, 1):
        for pre in (0, 1):
            wd, vd = ops.up(ops.o["w"]), ops.up(ops.o["v"])
            vw, vf, cross = _out(count), _out(count), C.c_double(CANARY)
            assert L.nka_hip_vec_scale_dot_pair_many(h, n, P(wd), P(vd), X.VEC_SCALE, subtract, pre, X.VEC_PRE_A, P(ops.ro("f")),
                                                     ops.ys_ptrs(count), count, vw.ctypes.data_as(dp), vf.ctypes.data_as(dp),
                                                     C.byref(cross)) == 0
            _canaries(count, vw, vf)
            wn = f"wn{pre}"
            where = (tag, count, subtract, pre)
            ops.hold("scale_dot_pair_many", cross.value, "f", wn, k0, where)
            for j in range(count):
                ops.hold("scale_dot_pair_many", vw[j], wn, f"y{j}", kj[j], where)
                ops.hold("scale_dot_pair_many", vf[j], "f", f"y{j}", kj[j], where)
            vn = X.VEC_SCALE * ops.o["v"]
            if subtract:
                vn = -1.0 * ops.o[wn] + vn
            assert _bits_equal(wd.cpu().numpy(), ops.o[wn]) and _bits_equal(vd.cpu().numpy(), vn), where


def run_dot_pair_many_scaled(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    k0, kj = _ks("dot_pair_many_scaled", n, env.ncu, ops.vec, count)
    for pre in (0, 1):
        vw, vf, cross = _out(count), _out(count), C.c_double(CANARY)
        assert L.nka_hip_vec_dot_pair_many_scaled(h, n, P(ops.ro("w")), X.VEC_SCALE, pre, X.VEC_PRE_A, P(ops.ro("f")),
                                                  ops.ys_ptrs(count), count, vw.ctypes.data_as(dp), vf.ctypes.data_as(dp),
                                                  C.byref(cross)) == 0
        _canaries(count, vw, vf)
        wn = f"wn{pre}"
        where = (tag, count, pre)
        ops.hold("dot_pair_many_scaled", cross.value, "f", wn, k0, where)
        for j in range(count):
            ops.hold("dot_pair_many_scaled", vw[j], wn, f"y{j}", kj[j], where)
            ops.hold("dot_pair_many_scaled", vf[j], "f", f"y{j}", kj[j], where)
    ops.untouched("w", "f")


def run_diff_norm_dot_pair_many(env, ops, count, tag):
    L, h, n = env.L, env.h, ops.n
    k0, kj = _ks("diff_norm_dot_pair_many", n, env.ncu, ops.vec, count)
    vz, vx, cross, dd = _out(count), _out(count), C.c_double(CANARY), C.c_double(CANARY)
    assert L.nka_hip_vec_diff_norm_dot_pair_many(h, n, P(ops.ro("z")), X.VEC_A, P(ops.ro("x")), ops.ys_ptrs(count), count,
                                                 C.byref(dd), vz.ctypes.data_as(dp), vx.ctypes.data_as(dp), C.byref(cross)) == 0
    _canaries(count, vz, vx)
    where = (tag, count)
    ops.hold("diff_norm_dot_pair_many", dd.value, "r", "r", k0, where)
    ops.hold("diff_norm_dot_pair_many", cross.value, "x", "r", k0, where)
    for j in range(count):
        ops.hold("diff_norm_dot_pair_many", vz[j], "r", f"y{j}", kj[j], where)
        ops.hold("diff_norm_dot_pair_many", vx[j], "x", f"y{j}", kj[j], where)
    ops.untouched("z", "x")


RUN = {"dot": run_dot, "dot_many": run_dot_many, "dot_pair_many": run_dot_pair_many, "update_norm2": run_update_norm2,
       "scale_dot_pair_many": run_scale_dot_pair_many, "dot_pair_many_scaled": run_dot_pair_many_scaled,
       "diff_norm_dot_pair_many": run_diff_norm_dot_pair_many}
MANY = [e for e in RUN if e not in ("dot", "update_norm2")]
MIN_COUNT = {"dot_many": 1}                      # (count == 0 returns before any launch: nothing to hold)
ALIGN = pytest.mark.parametrize("vec", [2, 1], ids=["aligned", "unaligned"])


# ---- the boundary shapes ---------------------------------------------------------------------------------------------------------

@ALIGN
@pytest.mark.parametrize("which", range(len(X.VEC_SHAPE_IDS)), ids=X.VEC_SHAPE_IDS)
@pytest.mark.parametrize("entry", list(RUN))
def test_every_sum_at_the_boundary_shapes(env, entry, which, vec):
    """Every shape of vec_boundary_shapes(G, vec) with the entry's own G -- the most blocks grid_for gives the kernel that
    count selects -- at counts 0 (where the entry launches then), 1, 3, 4, 5; from BIG elements on, counts 0, 1, 2."""
    counts = (0,) if entry in ("dot", "update_norm2") else [c for c in COUNTS if c >= MIN_COUNT.get(entry, 0)]
    by_n = {}
    for count in counts:
        gmax = launches(entry, 1 << 40, env.ncu, vec, count)[0][2]
        n = X.vec_boundary_shapes(gmax, vec)[which]
        if n >= BIG and count > 2:
            continue
        by_n.setdefault(n, []).append(count)
    assert by_n
    for n, cs in sorted(by_n.items()):
        grids = sorted({g for c in cs for _, _, g in launches(entry, n, env.ncu, vec, c)})
        ops = Ops(env, n, grids, vec, max(cs), seed=1000 * which + vec)
        for count in cs:
            RUN[entry](env, ops, count, X.VEC_SHAPE_IDS[which])


# ---- every width -----------------------------------------------------------------------------------------------------------------

def _pool(env, name, n, vec, count):
    """Operands shared by the cases of one test: planted for every grid an entry may launch there, their exact sums
    computed once."""
    key = (name, vec)
    if key not in env.pools:
        env.pools[key] = Ops(env, n, X.vec_all_grids(n, env.ncu, vec), vec, count, seed=len(name) + vec)
    return env.pools[key]


@ALIGN
@pytest.mark.parametrize("count", range(1, X.VEC_MANY_MAX + 1))
@pytest.mark.parametrize("entry", MANY)
def test_every_count_up_to_one_launch(env, entry, count, vec):
    """Counts 1..24 -- every exact width of the window kernels, every padded width 4..24 of the others, 12 included -- at
    three 512-tiles per block of the window kernels' grid and a ragged tail that gives some threads two elements."""
    n = X.vec_widths_shape(env.ncu)
    RUN[entry](env, _pool(env, "widths", n, vec, X.VEC_MANY_MAX), count, "widths")


@ALIGN
@pytest.mark.parametrize("count", [25, 37, 49])
@pytest.mark.parametrize("entry", MANY)
def test_lists_longer_than_one_launch(env, entry, count, vec):
    """25, 37, 49: the balanced groups of the pure-read entries (13 + 12, 19 + 18, 17 + 16 + 16), the 24 + rest split of
    dot_many / dot_pair_many, and the dot_pair_many tail of scale_dot_pair_many against the w it has just stored."""
    n = X.VEC_LONG_SHAPE
    RUN[entry](env, _pool(env, "long", n, vec, 49), count, "long")


# ---- NaN and Inf -----------------------------------------------------------------------------------------------------------------

@ALIGN
@pytest.mark.parametrize("bad", [math.nan, math.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("entry", MANY)
def test_a_non_finite_element_stays_in_the_sums_that_read_it(env, entry, bad, vec):
    """One element of ONE ys[j], the last of a tile: the sums over that vector are NaN / the infinity the exact sum has,
    every other sum still holds its bound (no column leaks into a neighbour)."""
    n, count, j = X.VEC_SMALL_SHAPES[0], 5, 2
    ops = Ops(env, n, X.vec_all_grids(n, env.ncu, vec), vec, count, seed=77 + vec)
    ops.o["ys"][j][3 * 256 * vec - 1] = bad
    RUN[entry](env, ops, count, "non-finite")
    hit = [ex for (a, b), (ex, _) in ops.memo.items() if f"y{j}" in (a, b)]
    assert hit and all(math.isnan(ex) if math.isnan(bad) else math.isinf(ex) for ex in hit)
    assert all(math.isfinite(ex) for (a, b), (ex, _) in ops.memo.items() if f"y{j}" not in (a, b))


# ---- the reference-order dot() ------------------------------------------------------------------------------------------------

def _constants(path, names):
    """constexpr int NAME = <expression of integers and earlier names>; read off a source file."""
    env = {}
    with open(os.path.join(ROOT, path)) as fh:
        for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", fh.read()):
            if re.fullmatch(r"[\w\s*+/()-]+", expr) and all(t in env for t in re.findall(r"[A-Za-z_]\w*", expr)):
                env[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(env)))
    return [env[k] for k in names]


def ordered_lengths():
    (chunk,) = _constants("nka_amd/csrc/vec_ops.hip", ["kDotOrdChunk"])
    block, group = _constants("nka_amd/csrc/nka_chain.hpp", ["kChainBlock", "kChainGroup"])
    hand = 4 * chunk                 # launch_dot_ordered: k_dot_ordered up to here, k_dot_chain beyond
    return [0, 1, 7, 8, 9, chunk - 1, chunk, chunk + 1, hand - 1, hand, hand + 1, group - 1, group, group + 1,
            group + block - 1, group + block, group + block + 1, 2 * group + 1, 3 * group + block + 3]


def _ordered_input(kind, n, rng):
    if kind == "uniform":
        return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    if kind == "normal":
        return rng.standard_normal(n), rng.standard_normal(n)
    if kind == "decades":            # tests/test_chain_sums_gpu.py: magnitudes over the whole range force the element walk
        return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 12, n), rng.uniform(0.5, 2, n)
    if kind == "cancels":            # returns to exactly zero after every pair
        a = np.repeat(rng.uniform(-1, 1, (n + 1) // 2), 2)[:n]
        a[1::2] *= -1.0
        if n % 2:
            a[-1] = 0.0
        return a, np.ones(n)
    if kind == "nan":
        x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        if n:
            y[n // 3] = np.nan
        return x, y
    assert kind == "overflow"
    return np.full(n, 1e300), np.full(n, 1e8)


def _same(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b) or (a != a and b != b)     # (any NaN for a NaN)


def _sequential(x, y):
    with np.errstate(all="ignore"):
        return float(np.add.accumulate(np.concatenate([[0.0], x * y]))[-1])


@pytest.mark.parametrize("offx,offy", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["16-16", "16-8", "8-16", "8-8"])
@pytest.mark.parametrize("kind", ["uniform", "normal", "decades", "cancels", "nan", "overflow"])
def test_reference_order_dot_on_the_bits(env, kind, offx, offy):
    L, h, torch = env.L, env.h, env.torch
    rng = np.random.default_rng(len(kind) + 2 * offx + offy)

    def dev(a, off):
        t = torch.zeros(a.size + 2, dtype=torch.float64, device="cuda")
        v = t[off:off + a.size]
        v.copy_(torch.from_numpy(a))
        assert a.size == 0 or v.data_ptr() % 16 == 8 * off
        return v

    assert L.nka_hip_vec_set_sum_order(h, REFERENCE_ORDER) == 0
    try:
        for n in ordered_lengths():
            x, y = _ordered_input(kind, n, rng)
            xd, yd, r = dev(x, offx), dev(y, offy), C.c_double(CANARY)
            assert L.nka_hip_vec_dot(h, n, P(xd), P(yd), C.byref(r)) == 0
            want = _sequential(x, y)
            assert _same(r.value, want), (kind, n, r.value.hex() if r.value == r.value else r.value, want)
            assert L.nka_hip_vec_norm2(h, n, P(xd), C.byref(r)) == 0
            want = math.sqrt(_sequential(x, x))
            assert _same(r.value, want), (kind, n, "norm2", r.value, want)
    finally:
        assert L.nka_hip_vec_set_sum_order(h, BLOCKED) == 0


@ALIGN
def test_fused_reductions_refuse_reference_order_and_come_back(env, vec):
    """With reference-order sums each of the six fused reductions returns NKA_HIP_ESTATE, writes no operand and no
    result; after set_sum_order(BLOCKED) they work again and dot() is back inside its blocked bound."""
    L, h = env.L, env.h
    n, count = X.VEC_SMALL_SHAPES[1], 3
    ops = Ops(env, n, X.vec_all_grids(n, env.ncu, vec), vec, count, seed=5)
    zd, wd, vd = ops.up(ops.o["z"]), ops.up(ops.o["w"]), ops.up(ops.o["v"])
    xd, fd, ys = ops.ro("x"), ops.ro("f"), ops.ys_ptrs(count)
    a, b, c, d = _out(count), _out(count), C.c_double(CANARY), C.c_double(CANARY)
    A, B = a.ctypes.data_as(dp), b.ctypes.data_as(dp)
    assert L.nka_hip_vec_set_sum_order(h, REFERENCE_ORDER) == 0
    try:
        assert L.nka_hip_vec_dot_many(h, n, P(xd), ys, count, A) == ESTATE
        assert L.nka_hip_vec_dot_pair_many(h, n, P(xd), P(zd), ys, count, A, B, C.byref(c)) == ESTATE
        for store in (0, 1):
            assert L.nka_hip_vec_update_norm2(h, n, P(zd), X.VEC_A, P(xd), store, C.byref(d)) == ESTATE
        assert L.nka_hip_vec_scale_dot_pair_many(h, n, P(wd), P(vd), X.VEC_SCALE, 1, 1, X.VEC_PRE_A, P(fd), ys, count, A, B,
                                                 C.byref(c)) == ESTATE
        assert L.nka_hip_vec_dot_pair_many_scaled(h, n, P(wd), X.VEC_SCALE, 1, X.VEC_PRE_A, P(fd), ys, count, A, B,
                                                  C.byref(c)) == ESTATE
        assert L.nka_hip_vec_diff_norm_dot_pair_many(h, n, P(zd), X.VEC_A, P(xd), ys, count, C.byref(d), A, B,
                                                     C.byref(c)) == ESTATE
        assert b"reference-order" in L.nka_hip_last_error()
        assert (a == CANARY).all() and (b == CANARY).all() and c.value == CANARY and d.value == CANARY
        for dev, host in ((zd, "z"), (wd, "w"), (vd, "v")):
            assert _bits_equal(dev.cpu().numpy(), ops.o[host]), host
        ops.untouched("x", "f", *[f"y{j}" for j in range(count)])
    finally:
        assert L.nka_hip_vec_set_sum_order(h, BLOCKED) == 0
    for entry in RUN:
        RUN[entry](env, ops, count, "after reference order")


def test_set_and_get_sum_order(env):
    L, h = env.L, env.h
    try:
        for order, back in ((REFERENCE_ORDER, REFERENCE_ORDER), (BLOCKED, BLOCKED), (AUTO, BLOCKED),
                            (BLOCKED_ROUNDED, BLOCKED_ROUNDED), (REFERENCE_ORDER, REFERENCE_ORDER)):
            assert L.nka_hip_vec_set_sum_order(h, order) == 0
            assert L.nka_hip_vec_get_sum_order(h) == back, order
            for unknown in (4, -1, 17):
                assert L.nka_hip_vec_set_sum_order(h, unknown) == EINVAL
                assert L.nka_hip_vec_get_sum_order(h) == back, (order, unknown)
    finally:
        assert L.nka_hip_vec_set_sum_order(h, BLOCKED) == 0
    assert L.nka_hip_vec_get_sum_order(h) == BLOCKED
