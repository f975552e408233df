"""The premise of tests/test_dot_weights_sharded_gpu.py, without a GPU.

With w = 1 on the entries a slice owns and 0 on its ghosts (tests/overlap_layout.py), the weighted accelerator on the
overlapped layout IS the plain accelerator on the deduplicated global vector: shown here on the compiled src-C reference
(oracle_py.RefC) whose user dot product is the masked sequential sum over the concatenated overlapped vector, bit for bit.
Then the error bound the GPU test holds every reduced sum to (check d: gamma(K) sum_r sum|ab|, K = the deepest slice's
blocked sum + the world - 1 additions of the exchange) against Fraction arithmetic on a simulation of the blocked partial
sums, and the proof that its planted inputs make a lost boundary entry or a counted ghost impossible to pass."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_sums as X
import overlap_layout as OL

LAYOUTS = {
    # halos of 3 over three ranks
    "halo3 x3": (3001, 3, {"halo": 3}),
    # a rank of 17 ghosts that owns nothing (in the middle) and an empty rank (last), halos of 1
    "ghosts-only + empty x4": (2503, 4, {"owned": [1200, 0, 1303, 0], "ghosts": {1: 17}, "halo": 1}),
    # eight ranks, halos of 130, an owns-nothing rank first and an empty one in the middle
    "halo130 x8": (4099, 8, {"owned": [0, 700, 650, 0, 800, 649, 0, 1300], "ghosts": {0: 17, 6: 5}, "halo": 130}),
}


def _inputs(n, calls, rng):
    """Independent vectors; every seventh call continues the last step, f_t = f_{t-1} + c (f_{t-1} - f_{t-2}) + noise, so
    that the new difference is nearly parallel to the stored one (a dependence drop)."""
    out = []
    for t in range(calls):
        if t % 7 == 5 and t >= 2:
            out.append(out[-1] + 0.75 * (out[-1] - out[-2]) + 1e-9 * rng.standard_normal(n))
        else:
            out.append(rng.standard_normal(n))
    return out


def _masked_dp(w):
    def dp(x, y):
        s = np.cumsum((w * x) * y)          # (cumsum adds element after element: the reference's sequential order)
        return float(s[-1]) if s.size else 0.0
    return dp


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_masked_overlapped_reference_is_the_plain_reference_on_the_global_vector(name):
    from oracle import oracle_py as O
    if not O.have_ref():
        O.build()
    assert O.have_ref(), "the compiled reference is built by build()"
    n, world, spec = LAYOUTS[name]
    ranks = OL.build(n, world, spec)
    assert any(k.src.size == 0 for k in ranks) or name == "halo3 x3"
    assert any(k.src.size > 0 and not k.w.any() for k in ranks) or name == "halo3 x3"
    src = np.concatenate([k.src for k in ranks])
    w = np.concatenate([k.w for k in ranks])
    own = w != 0
    m = 5
    rng = np.random.default_rng(len(name))
    plain = O.RefC(n, m)
    over = O.RefC(src.size, m, dp=_masked_dp(w))
    trash = O.RefC(src.size, m, dp=_masked_dp(w))
    capacity = dependence = 0
    before = 0
    for t, x in enumerate(_inputs(n, 3 * m + 8, rng)):
        fg = x.copy()
        plain.accel_update(fg)
        fo = x[src].copy()
        over.accel_update(fo)
        ft = np.where(own, x[src], 1e3 * rng.standard_normal(src.size))
        trash.accel_update(ft)
        assert np.array_equal(fo[own], fg), (name, t)                      # owned bits: the plain reference's
        assert np.array_equal(fo, fg[src]), (name, t)                      # ghosts: the owner's output bits
        assert np.array_equal(ft[own], fg), (name, t)                      # garbage at the ghosts changes no owned bit
        for ref in (over, trash):
            assert ref.num_vec() == plain.num_vec(), (name, t)
            assert ref.state().list_order() == plain.state().list_order(), (name, t)
        after = plain.num_vec()
        capacity += before == m
        dependence += after < min(before + 1, m)
        before = after
    assert capacity > 0 and dependence > 0, (name, capacity, dependence)   # both kinds of drop were decided
    for slot in plain.state().list_order():
        assert np.array_equal(over.w(slot)[own], plain.w(slot)), (name, slot)
        assert np.array_equal(over.v(slot)[own], plain.v(slot)), (name, slot)
        assert np.array_equal(trash.w(slot)[own], plain.w(slot)), (name, slot)
        assert np.array_equal(trash.v(slot)[own], plain.v(slot)), (name, slot)


def test_named_layouts_express_what_the_gpu_test_needs():
    """Every named layout builds (build() asserts the invariants) and the shapes the issue lists are there."""
    ncu = 256
    L = {nm: OL.build(*OL.named(nm, ncu)) for nm in OL.NAMES}
    for nm, width in (("halo1", 1), ("halo3", 3), ("halo512", 512), ("halo700", 700)):
        mid = L[nm][1]
        assert mid.first == width and mid.src.size - mid.first - (mid.hi - mid.lo) == width
    assert L["halo3"][1].first % 2 == 1
    for nm, r in (("ghost_first", 0), ("ghost_mid", 1), ("ghost_last", len(L["ghost_last"]) - 1)):
        k = L[nm][r]
        assert k.src.size > 0 and not k.w.any() and all(q.w.any() for i, q in enumerate(L[nm]) if i != r)
    assert sum(k.src.size == 0 for k in L["empty"]) == 1
    sh = L["shapes"]
    assert sh[0].src.size == 1 and sh[0].w.all() and sh[1].src.size <= 512 and sh[2].src.size > 8 * ncu * 512
    for k in L["tail_tiles"]:
        owned = k.hi - k.lo
        assert k.first == 0 and owned % 512 == 0 and (k.src.size - owned) % 512 == 0 and k.src.size > owned
        for aligned in (True, False):
            assert X.pass_grids(owned, ncu, aligned) == X.pass_grids(k.src.size, ncu, aligned)
    mv = OL.moved(L["halo3"], 2, OL.named("halo3")[0])
    assert all(np.array_equal(a.src, b.src) for a, b in zip(mv, L["halo3"])) and mv[0].hi == L["halo3"][0].hi + 2


# ---- the bound of check d ------------------------------------------------------------------------------------------------

def fraction_dot(x, y):
    return float(sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y)), Fraction(0)))


def blocked_sum(prod, G):
    """The device's blocked sum of the products `prod` on G blocks of 256 threads, tiles of 512 (as
    tests/test_exact_sums_cpu.py restates it: a rounded product and a rounded sum per step, one rounding more than the fma)."""
    n = prod.size
    ntile = n // 512
    G = max(1, min(G, max(ntile, 1)))
    acc = np.zeros((G, 256))
    for t in range(ntile):
        for q in range(2):
            acc[t % G] = acc[t % G] + prod[t * 512 + q: (t + 1) * 512: 2]
    for i in range(ntile * 512, n):
        acc[G - 1, (i - ntile * 512) % 256] += prod[i]
    partial = []
    for b in range(G):
        r = None
        for wv in range(4):
            v = acc[b, wv * 64:(wv + 1) * 64].copy()
            while v.size > 1:
                v = v[: v.size // 2] + v[v.size // 2:]
            r = v[0] if r is None else r + v[0]
        partial.append(r)
    v = np.array([sum(partial[b] for b in range(lane, G, 64)) for lane in range(64)])
    while v.size > 1:
        v = v[: v.size // 2] + v[v.size // 2:]
    return float(v[0]), G


@pytest.mark.parametrize("spec", [(7 * 512 * 3 + 300, 3, {"halo": 3}),
                                  (9000, 4, {"owned": [4000, 0, 4999, 1], "ghosts": {1: 17}, "halo": [(0, 1), (0, 0), (1, 1), (0, 0)]})])
def test_the_sharded_bound_holds_for_simulated_blocked_partial_sums(spec):
    """world blocked partial sums of fl(w a) b, added in rank order, stay within gamma(K) sum_r sum|fl(w a) b| of the exact
    sum over the owned entries (Fraction arithmetic), K = max_r k_steps(n_r) + (world - 1), on adversarial data with finite
    garbage at the ghosts."""
    n, world, sp = spec
    ranks = OL.build(n, world, sp)
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 30, n))
    b = rng.standard_normal(n)
    G = 7
    total, tot_abs, k = None, 0.0, 0
    for r in ranks:
        al = np.where(r.w != 0, a[r.src], 1e3 * rng.standard_normal(r.src.size))
        aw = r.w * al
        part, g = blocked_sum(aw * b[r.src], G)
        total = part if total is None else total + part               # rank order
        tot_abs += X.abs_dot(aw, b[r.src])
        k = max(k, X.k_steps(r.src.size, g, 2))
    k += world - 1
    ex = fraction_dot(a, b)
    assert abs(total - ex) <= (X.gamma(k) + X.U) * tot_abs, (abs(total - ex) / (X.U * tot_abs), k)


@pytest.mark.parametrize("name", ["halo3", "ghost_mid", "empty", "shapes"])
def test_a_lost_boundary_entry_or_a_counted_ghost_cannot_pass_check_d(name):
    """For the planted inputs of check d (overlap_layout.planted) and every sum an update forms: the product at each rank's
    first and last owned entry, and at the ghost entries next to them, exceeds twice the bound (plus the rounding of the
    exact sum) -- exact_sums.detectable -- so a sum that lost the one or counted the other fails the check."""
    ncu = 256
    n, world, spec = OL.named(name, ncu)
    ranks = OL.build(n, world, spec)
    rng = np.random.default_rng(11)
    fs = [OL.planted(ranks, n, ncu, rng)]
    for _ in range(3):
        fs.append(OL.planted(ranks, n, ncu, rng, prev=fs[-1]))
    d_old = fs[0] - fs[1]
    w_old = d_old / math.sqrt(float(np.dot(d_old, d_old)))
    f, d = fs[3], fs[2] - fs[3]
    w1n = d / math.sqrt(float(np.dot(d, d)))
    pairs = {"<d,d>": (d, d), "<f,d>": (f, d), "<f,w1'>": (f, w1n), "<d,w_p>": (d, w_old), "<w1',w_p>": (w1n, w_old),
             "<f,w_p>": (f, w_old)}
    k = max(max(X.device_k(r.src.size, ncu, al) for al in (True, False)) for r in ranks) + world - 1
    bound = X.gamma(k)
    edges = np.unique(np.concatenate([[r.lo, r.hi - 1, max(r.lo - 1, 0), min(r.hi, n - 1)] for r in ranks if r.hi > r.lo]))
    ghosts = np.unique(np.concatenate([r.src[r.w == 0] for r in ranks] + [np.zeros(0, np.int64)]))
    near = np.intersect1d(edges, ghosts) if ghosts.size else edges
    for what, (x, y) in pairs.items():
        tot = X.abs_dot(x, y)
        for idx in (edges, near):
            worst = float(np.abs(x[idx] * y[idx]).min())
            assert X.detectable(worst, bound, tot), (name, what, worst / tot, bound)
