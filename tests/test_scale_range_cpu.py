"""What tests/test_scale_range_gpu.py rests on, held on the oracle alone (tests/scale_range.py): for every shape, flavour and
seed that file uses,
  1 the oracle is covariant -- outputs, list orders, h, c and stored vectors by the scaling table -- at every k of K_COVARIANT
    and at +-505;
  2 every regime of K_EDGE is met: a subnormal nonzero red[0] at -520, d != 0 with dp(d, d) == 0 and other decisions than at
    k = 0 at -540, dp(d, d) == Inf at 511 and at 600, with red[0] recomputed in numpy as the chain over w1 - f;
  3 every output at every k of K_ALL is finite;
  4 the step's witness: at -540 the chain dp(f, f) is 0 for a nonzero input; and the nonzero elements of the unscaled inputs
    are at least 2^-30 in magnitude (the derivation of K_COVARIANT).
A seed that fails a witness is replaced in scale_range.seed(); no case is skipped."""
import math

import numpy as np
import pytest

import scale_range as R
from split_update import _bits_equal

REF_CASES = ([("narrow", v, m, R.ROUNDS_REF) for v, m in R.REF_NARROW] + [("lanes", v, m, R.ROUNDS_LANES) for v, m in R.REF_LANES]
             + [("lone", v, m, 1) for v, m in R.REF_LONE])
FAST_CASES = sorted(set(R.FAST_NARROW + R.FAST_WIDE + R.FAST_STORE32 + R.FAST_WEIGHTED + R.FAST_LONE
                        + [R.FAST_LENGTHS_NARROW, R.FAST_LENGTHS_WIDE]))


def _run(oracle, vlen, mvec, flavor, base, k, with_dd):
    """One system at exponent k -> per call (record of OracleRun.update, observables after the call)."""
    run = R.OracleRun(oracle, vlen, mvec, flavor)
    out = []
    for x in R.scaled(base, k):
        rec = run.update(x, with_dd)
        out.append((rec, R.observables(run.ora)))
    return out


def _assert_covariant(got, unit, k, where):
    for t, ((rec, obs), (rec0, obs0)) in enumerate(zip(got, unit)):
        assert _bits_equal(rec["f"], R.expect_rows(rec0["f"], k)), (where, k, t, "f")
        (dec, h, c, slots), (dec0, h0, c0, slots0) = obs, obs0
        assert dec == dec0, (where, k, t, "decisions")
        assert _bits_equal(h, h0) and _bits_equal(c, R.expect_rows(c0, k)), (where, k, t, "h, c")
        order, pending = dec[0], dec[3]
        for s in order:
            kk = k if pending and s == order[0] else 0      # the pending pair is raw: it scales; a normalised pair does not
            assert _bits_equal(slots[s][0], R.scaled(slots0[s][0], kk)) and _bits_equal(slots[s][1], R.scaled(slots0[s][1], kk)), (where, k, t, s)


def _assert_finite(got, where, k):
    for t, (rec, (_, h, _, slots)) in enumerate(got):
        assert np.isfinite(rec["f"]).all(), (where, k, t, "f")
        for s, (w, v) in slots.items():
            assert np.isfinite(w).all() and np.isfinite(v).all(), (where, k, t, s)


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("path, vlen, mvec, nrounds", REF_CASES)
def test_reference_order_shapes_meet_every_regime(oracle, path, vlen, mvec, nrounds, flavor):
    for rnd in range(nrounds):
        where = (path, vlen, mvec, flavor, rnd)
        base = R.base_inputs(vlen, mvec, rnd)
        nz = np.abs(base[base != 0.0])
        assert nz.min() >= 2.0 ** -30 and nz.max() <= 2.0 ** 5, (where, "the derivation of K_COVARIANT")
        unit = _run(oracle, vlen, mvec, flavor, base, 0, False)
        _assert_finite(unit, where, 0)
        for k in R.K_SAFE:
            if k == 505 and vlen in R.OVERFLOWS_AT_505:      # (scale_range.py: this long, +505 overflows red[0] already)
                got = _run(oracle, vlen, mvec, flavor, base, k, True)
                assert any(rec["pending"] and rec["dd"] == math.inf for rec, _ in got), (where, k, "no overflow of red[0]")
            else:
                got = _run(oracle, vlen, mvec, flavor, base, k, False)
                _assert_covariant(got, unit, k, where)
            _assert_finite(got, where, k)
        edge = {k: _run(oracle, vlen, mvec, flavor, base, k, True) for k in (-540, -520) + R.K_OVERFLOW}
        for k, got in edge.items():
            _assert_finite(got, where, k)
        assert any(rec["pending"] and R.is_subnormal(rec["dd"]) for rec, _ in edge[-520]), (where, "no subnormal red[0] at -520")
        assert any(rec["pending"] and rec["d"].any() and rec["dd"] == 0.0 for rec, _ in edge[-540]), (where, "no underflow to 0 at -540")
        assert any(obs[0][0] != obs0[0][0] for (_, obs), (_, obs0) in zip(edge[-540], unit)), (where, "-540 took the decisions of k = 0")
        for k in R.K_OVERFLOW:
            assert any(rec["pending"] and rec["dd"] == math.inf for rec, _ in edge[k]), (where, k, "no overflow of red[0]")
        if path != "lone":      # the step runs on these shapes: dp(f, f) == 0 with f != 0 at -540
            assert any(x.any() and R.chain(x, x) == 0.0 for x in R.scaled(base, -540)), (where, "no dp(f, f) == 0 with f != 0")


@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("vlen, mvec", FAST_CASES)
def test_fast_sum_shapes_are_covariant_on_the_oracle(oracle, vlen, mvec, flavor):
    for rnd in range(R.ROUNDS_FAST):
        where = ("fast", vlen, mvec, flavor, rnd)
        base = R.base_inputs(vlen, mvec, rnd)
        nz = np.abs(base[base != 0.0])
        assert nz.min() >= 2.0 ** -30 and nz.max() <= 2.0 ** 5, (where, "the derivation of K_COVARIANT")
        unit = _run(oracle, vlen, mvec, flavor, base, 0, False)
        for k in R.K_COVARIANT:
            got = _run(oracle, vlen, mvec, flavor, base, k, False)
            _assert_covariant(got, unit, k, where)
            _assert_finite(got, where, k)


def test_the_helper_places_every_regime_in_one_batch():
    assert R.K_ALL == R.K_EDGE + R.K_COVARIANT + (0,) and len(set(R.K_ALL)) == 9
    ks, rs = R.exponents(18), R.rounds(18)
    assert ks[:9] == list(R.K_ALL) and ks[9:] == list(R.K_ALL) and rs == [0] * 9 + [1] * 9
    X = R.batch_inputs(7, 3, 18)
    assert X.shape == (13, 18, 7)
    for j in range(18):
        assert _bits_equal(X[:, j], np.ldexp(R.base_inputs(7, 3, rs[j]), ks[j])), j
    red = np.arange(1.0, 9.0)                       # mvec = 3: [dd, fw1, 3 x w1w, 3 x fw]
    got = R.expect_red(red, 5, 3)
    assert got.tolist() == [1024.0, 64.0, 3.0, 4.0, 5.0, 192.0, 224.0, 256.0]
    assert R.chain(np.array([3.0, 4.0]), np.array([3.0, 4.0])) == 25.0 and R.is_subnormal(2.0 ** -1030) and not R.is_subnormal(0.0)
