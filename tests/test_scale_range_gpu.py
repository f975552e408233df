"""Every update path across the binary64 exponent range (tests/scale_range.py; the oracle's side of it is held by
tests/test_scale_range_cpu.py).  Every batch carries all of K_ALL, or of K_FAST, at once: system j runs its round's inputs
scaled by 2^K[j % len(K)], so the regimes sit in neighbouring workgroups or lanes.  Every comparison is _bits_equal.

  1 the reference's order against the oracle over K_ALL -- narrow batch, lane batch, lone handle --, with the witnesses of the
    CPU file seen again on the device's own red[0]: subnormal at -520, zero with a relax at -540, Inf at 511 and 600
  2 the step over K_ALL: fnorm = sqrt(chain), the stop rule at tol = fnorm and one below, x - f_out, dp(f, f) == 0 at -540
  3 the fast sums over K_FAST: a system on 2^k F beside the system on F, every observable by the scaling table; the k = 0
    systems against a batch that holds only them
  4 graphs captured before the first call, replayed over the K_ALL inputs"""
import math

import numpy as np
import pytest

import batch_weights as BW
import scale_range as R
from split_update import _bits_equal, _same_bits

pytestmark = pytest.mark.gpu

PLANTED = -7.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _f64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def _live(st):
    return st.list_order()[1:] if st.pending else st.list_order()


def _decisions(st):
    return st.list_order(), st.free_order(), (st.subspace, st.pending)


def _assert_oracle_state(st, nv, w, v, ora, flavor, where):
    """Decisions, h on the live block and every listed slot against the oracle (compact storage: the v array of a normalised
    pair holds fl(v' - w'))."""
    so = ora.state()
    assert nv == ora.num_vec() and _decisions(st) == _decisions(so), (where, "decisions")
    live = _live(so)
    ix = np.ix_([s - 1 for s in live], [s - 1 for s in live])
    assert _bits_equal(st.h[ix], so.h[ix]), (where, "h")
    for slot in so.list_order():
        wo, vo = ora.w(slot), ora.v(slot)
        if flavor == 2 and slot in live:
            vo = vo - wo
        assert _bits_equal(w(slot), wo), (where, slot, "w")
        assert _bits_equal(v(slot), vo), (where, slot, "v")


class Witnesses:
    """The regimes seen on the device's own red[0], per exponent."""

    def __init__(self):
        self.seen = {k: set() for k in R.K_ALL}

    def note(self, k, rec, red0, nv0, nv):
        if not rec["pending"]:
            return
        if R.is_subnormal(red0):
            self.seen[k].add("subnormal")
        if red0 == 0.0 and rec["d"].any() and nv <= nv0:      # s == 0 from underflow: the pending pair went, the list did not grow
            self.seen[k].add("relax")
        if red0 == math.inf:
            self.seen[k].add("inf")
        if math.isfinite(red0) and red0 >= R.SUBNORMAL:
            self.seen[k].add("normal")

    def assert_all(self, where, overflows_at_505=False):
        print("red[0] seen per exponent", where, {k: sorted(v) for k, v in self.seen.items()})
        assert "subnormal" in self.seen[-520], (where, self.seen, "no subnormal red[0] at -520")
        assert "relax" in self.seen[-540], (where, self.seen, "no zero red[0] with a relax at -540")
        for k in R.K_OVERFLOW:
            assert "inf" in self.seen[k], (where, self.seen, k, "no Inf red[0]")
        for k in R.K_COVARIANT + (-505, 0) + (() if overflows_at_505 else (505,)):
            assert self.seen[k] == {"normal"}, (where, self.seen, k)
        if overflows_at_505:
            assert "inf" in self.seen[505], (where, self.seen, 505, "no Inf red[0]")


# ---- 1. the reference's order against the oracle ----------------------------------------------------------------------------------

def _batch_against_oracle(torch, oracle, b, vlen, mvec, flavor, nsys, replay=None):
    """Every call of the K_ALL inputs on batch b -- through replay(X) -> F where a graph runs it -- against one oracle per system."""
    X = R.batch_inputs(vlen, mvec, nsys)
    ks = R.exponents(nsys)
    runs = [R.OracleRun(oracle, vlen, mvec, flavor) for _ in range(nsys)]
    wit = Witnesses()
    nv0 = b.num_vec()
    for t in range(X.shape[0]):
        recs = [runs[j].update(X[t, j]) for j in range(nsys)]
        if replay is None:
            F = _f64(torch, X[t])
            b.accel_update(F)
        else:
            F = replay(X[t])
        got = F.cpu().numpy()
        nv = b.num_vec()
        for j in range(nsys):
            where = (vlen, mvec, flavor, t, j, ks[j])
            assert _bits_equal(got[j], recs[j]["f"]), (where, "f")
            _assert_oracle_state(b.state(j), nv[j], lambda s: b.w(j, s), lambda s: b.v(j, s), runs[j].ora, flavor, where)
            red0 = float(b.reductions(j)[0])
            if recs[j]["pending"]:
                assert _same_bits(red0, recs[j]["dd"]), (where, "red[0]", red0, recs[j]["dd"])
            wit.note(ks[j], recs[j], red0, nv0[j], nv[j])
        nv0 = nv
    wit.assert_all((vlen, mvec, flavor))


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("vlen, mvec", R.REF_NARROW)
def test_narrow_batch_in_reference_order_carries_the_oracles_bits_at_every_exponent(torch_cuda, oracle, vlen, mvec, flavor):
    import nka_amd
    nsys = R.ROUNDS_REF * len(R.K_ALL)
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    _batch_against_oracle(torch_cuda, oracle, b, vlen, mvec, flavor, nsys)
    b.delete()


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("vlen, mvec", R.REF_LANES)
def test_lane_batch_carries_the_oracles_bits_at_every_exponent(torch_cuda, oracle, vlen, mvec, flavor):
    import nka_amd
    nsys = R.ROUNDS_LANES * len(R.K_ALL)
    assert nsys > nka_amd.batch_lanes_limits(mvec)[0], "more than one group"
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, lanes=True)
    _batch_against_oracle(torch_cuda, oracle, b, vlen, mvec, flavor, nsys)
    b.delete()


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("n, mvec", R.REF_LONE)
def test_lone_handle_in_reference_order_carries_the_oracles_bits_at_every_exponent(torch_cuda, oracle, n, mvec, flavor):
    """One handle per exponent.  n = 5000: the chain sums in their integer form over four whole blocks and a ragged one at
    k = 0 and +-400, their fallbacks at every other k (scale_range.py)."""
    import nka_amd
    torch = torch_cuda
    base = R.base_inputs(n, mvec, 0)
    wit = Witnesses()
    for k in R.K_ALL:
        acc = nka_amd.nka().init(n, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
        run = R.OracleRun(oracle, n, mvec, flavor)
        nv0 = 0
        for t, x in enumerate(R.scaled(base, k)):
            where = (n, mvec, flavor, t, k)
            rec = run.update(x)
            ft = _f64(torch, x)
            acc.accel_update(ft)
            assert _bits_equal(ft.cpu().numpy(), rec["f"]), (where, "f")
            nv = acc.num_vec()
            _assert_oracle_state(acc.state(), nv, acc.w, acc.v, run.ora, flavor, where)
            red0 = float(acc.reductions()[0])
            if rec["pending"]:      # (a lone handle leaves red[0] as it was where it formed no norm)
                assert _same_bits(red0, rec["dd"]), (where, "red[0]", red0, rec["dd"])
            wit.note(k, rec, red0, nv0, nv)
            nv0 = nv
        acc.delete()
    wit.assert_all((n, mvec, flavor), overflows_at_505=n in R.OVERFLOWS_AT_505)


# ---- 2. the step --------------------------------------------------------------------------------------------------------------------

def _step_against_oracle(torch, oracle, b, vlen, mvec, flavor, nsys):
    """accel_step with x, mask, tol and fnorm over K_ALL.  System j retires at every third call (tol = fnorm) and goes on at the
    others (tol = the next double below fnorm); the oracle takes the calls that go on."""
    X = R.batch_inputs(vlen, mvec, nsys)
    ks, rs = R.exponents(nsys), R.rounds(nsys)
    oras = [oracle.OracleNKA(vlen, mvec, flavor) for _ in range(nsys)]
    rng = np.random.default_rng(vlen + mvec)
    x0 = rng.standard_normal((max(rs) + 1, vlen))
    xh = np.stack([R.scaled(x0[r], k) for k, r in zip(ks, rs)])
    Xd = _f64(torch, xh)
    seen = {k: set() for k in R.K_ALL}
    for t in range(X.shape[0]):
        sq = [R.chain(X[t, j], X[t, j]) for j in range(nsys)]
        want = np.array([math.sqrt(s) for s in sq])
        retire = np.array([(t + rs[j]) % 3 == 2 for j in range(nsys)])
        tol = np.where(retire, want, np.nextafter(want, -np.inf))      # (below a zero norm: the largest negative number)
        F, mask, fnorm = _f64(torch, X[t]), _i32(torch, np.ones(nsys)), _f64(torch, np.full(nsys, PLANTED))
        before = [b.state_digest(j) for j in range(nsys)]
        b.accel_step(F, Xd, mask, _f64(torch, tol), fnorm)
        got, xg, m, fn = F.cpu().numpy(), Xd.cpu().numpy(), mask.cpu().numpy(), fnorm.cpu().numpy()
        assert _bits_equal(fn, want), ((vlen, mvec, flavor, t), "fnorm", fn, want)
        assert np.array_equal(m != 0, ~retire), ((vlen, mvec, flavor, t), "the stop rule", m, tol, want)
        nv = b.num_vec()
        for j in range(nsys):
            where = (vlen, mvec, flavor, t, j, ks[j])
            k = ks[j]
            if 0.0 < sq[j] < 2.0 ** -767:      # the branch of the compiler's sqrt that scales its argument
                seen[k].add("scaled sqrt")
            if sq[j] == math.inf:
                seen[k].add("inf")
            if retire[j]:
                assert _bits_equal(got[j], X[t, j]) and _bits_equal(xg[j], xh[j]) and b.state_digest(j) == before[j], (where, "retired")
                if sq[j] == 0.0 and X[t, j].any():
                    assert tol[j] == 0.0 and fn[j] == 0.0
                    seen[k].add("tol 0 retires f != 0")
                continue
            f = X[t, j].copy()
            oras[j].accel_update(f)
            assert _bits_equal(got[j], f), (where, "f")
            xh[j] = xh[j] - f
            assert _bits_equal(xg[j], xh[j]), (where, "x")
            st, so = b.state(j), oras[j].state()
            assert nv[j] == oras[j].num_vec() and _decisions(st) == _decisions(so), (where, "decisions")
    print("the step saw per exponent", (vlen, mvec, flavor), {k: sorted(v) for k, v in seen.items()})
    assert "tol 0 retires f != 0" in seen[-540], seen
    for k in (-520, -505, -400):
        assert "scaled sqrt" in seen[k], (seen, k)
    for k in R.K_OVERFLOW:
        assert "inf" in seen[k], (seen, k)


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("vlen", [7, 64, 700])
def test_the_step_of_a_narrow_batch_in_reference_order_at_every_exponent(torch_cuda, oracle, vlen, flavor):
    import nka_amd
    mvec, nsys = 3, R.ROUNDS_REF * len(R.K_ALL)
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    _step_against_oracle(torch_cuda, oracle, b, vlen, mvec, flavor, nsys)
    b.delete()


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("vlen", [7, 64])
def test_the_step_of_a_lane_batch_at_every_exponent(torch_cuda, oracle, vlen, flavor):
    import nka_amd
    mvec, nsys = 3, R.ROUNDS_LANES * len(R.K_ALL)
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, lanes=True)
    _step_against_oracle(torch_cuda, oracle, b, vlen, mvec, flavor, nsys)
    b.delete()


# ---- 3. the fast sums: covariance ------------------------------------------------------------------------------------------------

def _assert_scaled_twin(get, j, j0, k, mvec, expect_red, where, upto=None):
    """System j (on 2^k F) against system j0 (on F) by the scaling table.  get(j) -> (row of F, red, state, num_vec, w, v)."""
    (f, red, st, nv, w, v), (f0, red0, st0, nv0, w0, v0) = get(j), get(j0)
    cut = slice(None) if upto is None else slice(0, upto)
    assert _bits_equal(f[cut], R.expect_rows(f0[cut], k)), (where, "f")
    assert _bits_equal(red, expect_red(red0, k, mvec)), (where, "red", red, red0)
    assert nv == nv0 and _decisions(st) == _decisions(st0), (where, "decisions")
    assert _bits_equal(st.h, st0.h), (where, "h")
    assert _bits_equal(st.c, R.expect_rows(st0.c, k)), (where, "c")
    order = st0.list_order()
    for s in order:
        kk = k if st0.pending and s == order[0] else 0      # the pending pair is raw: it scales; a normalised pair does not
        assert _bits_equal(w(s)[cut], R.scaled(w0(s)[cut], kk)), (where, s, "w")
        assert _bits_equal(v(s)[cut], R.scaled(v0(s)[cut], kk)), (where, s, "v")


def _covariant_batch(torch, make, vlen, mvec, where0, expect_red=R.expect_red, lens=None):
    """make(nsys, rounds) -> a batch whose system j belongs to round rounds[j].  The batch over K_FAST: its systems on 2^+-400 F
    against its systems on F after every call; and its systems on F against a batch that holds only those."""
    K = R.K_FAST
    nsys = R.ROUNDS_FAST * len(K)
    ks, rs = R.exponents(nsys, K), R.rounds(nsys, K)
    X = R.batch_inputs(vlen, mvec, nsys, K)
    b, unit = make(nsys, rs), make(R.ROUNDS_FAST, list(range(R.ROUNDS_FAST)))
    units = [j for j in range(nsys) if ks[j] == 0]
    grew = dropped = False
    nv0 = b.num_vec()
    for t in range(X.shape[0]):
        F, F1 = _f64(torch, X[t]), _f64(torch, X[t, units])
        b.accel_update(F)
        unit.accel_update(F1)
        got, got1 = F.cpu().numpy(), F1.cpu().numpy()
        nv, nv1 = b.num_vec(), unit.num_vec()

        def get(j):
            return got[j], b.reductions(j), b.state(j), nv[j], lambda s: b.w(j, s), lambda s: b.v(j, s)

        for j in range(nsys):
            upto = None if lens is None else lens[rs[j]]
            if ks[j] != 0:
                _assert_scaled_twin(get, j, len(K) * rs[j], ks[j], mvec, expect_red, where0 + (t, j, ks[j]), upto)
                if upto is not None:
                    assert _bits_equal(got[j][upto:], X[t, j][upto:]), (where0, t, j, "beyond the system's length")
                continue
            r = rs[j]
            where = where0 + (t, j, "against the batch of k = 0 systems")
            assert _bits_equal(got[j], got1[r]) and b.state_digest(j) == unit.state_digest(r), where
            assert _bits_equal(b.reductions(j), unit.reductions(r)) and nv[j] == nv1[r], where
            for s in b.state(j).list_order():
                assert _bits_equal(b.w(j, s), unit.w(r, s)) and _bits_equal(b.v(j, s), unit.v(r, s)), (where, s)
        grew |= bool((nv > nv0).any())
        dropped |= bool(((nv <= nv0) & (nv0 > 0)).any())
        nv0 = nv
    assert grew and dropped, (where0, "the lists never grew, or never dropped")
    b.delete()
    unit.delete()


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("vlen, mvec", R.FAST_NARROW)
def test_fast_sums_of_a_narrow_batch_are_covariant(torch_cuda, vlen, mvec, flavor):
    import nka_amd

    def make(nsys, rs):
        return nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
    _covariant_batch(torch_cuda, make, vlen, mvec, ("narrow", vlen, mvec, flavor))


@pytest.mark.parametrize("vlen, mvec", R.FAST_WIDE)
def test_fast_sums_of_a_wide_batch_are_covariant(torch_cuda, vlen, mvec):
    import nka_amd
    chunk = nka_amd.batch_wide_limits()[0]
    assert -(-vlen // chunk) == (2 if vlen == R.FAST_WIDE[0][0] else 3), "two and three chunks"

    def make(nsys, rs):
        return nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    _covariant_batch(torch_cuda, make, vlen, mvec, ("wide", vlen, mvec))


@pytest.mark.parametrize("vlen, mvec", R.FAST_STORE32)
def test_binary32_slots_are_the_same_bits_at_every_exponent(torch_cuda, vlen, mvec):
    """The normalised slots -- binary32 -- are bit-equal across k, the pending rows -- binary64 -- are scaled."""
    import nka_amd

    def make(nsys, rs):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, storage=nka_amd.STORE_F32)
        assert b.storage() == nka_amd.STORE_F32
        return b
    _covariant_batch(torch_cuda, make, vlen, mvec, ("binary32", vlen, mvec))


@pytest.mark.parametrize("vlen, mvec", R.FAST_WEIGHTED)
def test_fast_sums_of_a_weighted_batch_are_covariant(torch_cuda, vlen, mvec):
    """General weights, NOT scaled, one draw per round: red[0] scales by 4^k, red[1] and red[2+mvec+p] by 2^k, red[2+p] stays."""
    import nka_amd
    W = np.stack([BW.draw_weights(vlen, np.random.default_rng([BW.WEIGHT_SEED, vlen, r])) for r in range(R.ROUNDS_FAST)])

    def make(nsys, rs):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        b.set_dot_weights(np.ascontiguousarray(W[rs]))
        b.restart()
        assert b.dot_weighted()
        return b
    _covariant_batch(torch_cuda, make, vlen, mvec, ("weighted", vlen, mvec))


@pytest.mark.parametrize("wide", [False, True])
def test_fast_sums_with_lengths_are_covariant(torch_cuda, wide):
    """A length per round: the full one, one past a tile (narrow) or a chunk (wide) boundary, and a short one."""
    import nka_amd
    vlen, mvec = R.FAST_LENGTHS_WIDE if wide else R.FAST_LENGTHS_NARROW
    lens = [vlen, 2049 if wide else 513, 65]

    def make(nsys, rs):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide)
        b.set_lengths(np.array([lens[r] for r in rs], np.int32))
        b.restart()
        assert b.has_lengths()
        return b
    _covariant_batch(torch_cuda, make, vlen, mvec, ("lengths", wide, vlen, mvec), lens=lens)


def _expect_red_raw(red, k, mvec):
    """SUMS_BLOCKED of a lone handle sums on the raw difference: <d,d> and <f,d> times 4^k, <d,w_p> and <f,w_p> times 2^k."""
    out = np.array(red, np.float64)
    out[:2] = np.ldexp(out[:2], 2 * int(k))
    out[2:] = np.ldexp(out[2:], int(k))
    return out


@pytest.mark.parametrize("order", ["blocked", "rounded"])
@pytest.mark.parametrize("n, mvec", R.FAST_LONE)
def test_fast_sums_of_a_lone_handle_are_covariant(torch_cuda, n, mvec, order):
    import nka_amd
    torch = torch_cuda
    mode = nka_amd.SUMS_BLOCKED if order == "blocked" else nka_amd.SUMS_BLOCKED_ROUNDED
    expect_red = _expect_red_raw if order == "blocked" else R.expect_red
    for rnd in range(R.ROUNDS_FAST):
        base = R.base_inputs(n, mvec, rnd)
        accs = [nka_amd.nka().init(n, mvec).set_sum_order(mode) for _ in R.K_FAST]
        for t in range(base.shape[0]):
            outs = []
            for a, k in zip(accs, R.K_FAST):
                ft = _f64(torch, R.scaled(base[t], k))
                a.accel_update(ft)
                outs.append(ft.cpu().numpy())

            def get(j):
                a = accs[j]
                return outs[j], a.reductions(), a.state(), a.num_vec(), a.w, a.v

            for j, k in enumerate(R.K_FAST):
                if k != 0:
                    _assert_scaled_twin(get, j, 0, k, mvec, expect_red, ("lone", n, mvec, order, rnd, t, k))
        for a in accs:
            a.delete()


# ---- 4. graphs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [False, True])
def test_a_graph_captured_before_the_first_call_replays_over_every_exponent(torch_cuda, oracle, lanes):
    """The update of test 1, captured before any update has run and replayed over the K_ALL inputs: the oracle's bits, with
    the same witnesses."""
    import nka_amd
    torch = torch_cuda
    vlen, mvec = 64, 3
    nsys = (R.ROUNDS_LANES if lanes else R.ROUNDS_REF) * len(R.K_ALL)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        if lanes:
            b = nka_amd.nka_batch().init(nsys, vlen, mvec, lanes=True)
        else:
            b = nka_amd.nka_batch().init(nsys, vlen, mvec).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
        Fs = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        b.accel_update(Fs)

    def replay(X):
        with torch.cuda.stream(side):
            Fs.copy_(_f64(torch, X))
            g.replay()
        torch.cuda.synchronize()
        return Fs

    _batch_against_oracle(torch, oracle, b, vlen, mvec, b.flavor(), nsys, replay=replay)
    b.delete()
