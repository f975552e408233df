"""CPU only: the premises of the exact weight tests (tests/test_dot_weights_gpu.py, tests 2 and 3) hold for the compiled src-C
reference itself when its user dot product is the weighted sequential sum  dp(x, y) = sum fl(w_i x_i) y_i  (added in index
order, one rounding per operation):
  w_i = 4^k_i  -> a weighted run on f is 2^-k o (a plain run on 2^k o f), bit for bit, with the same decisions;
  w_i in {0,1} -> finite garbage at the masked entries changes no unmasked output and no decision."""
import numpy as np

from oracle import oracle_py


def _seq_dp(w):
    def dp(x, y):
        return float(np.cumsum((w * x) * y)[-1]) if x.size else 0.0      # np.cumsum adds in index order
    return dp


def _plain_dp(x, y):
    return float(np.cumsum(x * y)[-1]) if x.size else 0.0


def test_powers_of_four_on_the_reference():
    n, m = 3001, 5
    rng = np.random.default_rng(11)
    k = rng.integers(-6, 7, size=n)
    sc = np.ldexp(1.0, k)
    a = oracle_py.RefC(n, m, dp=_seq_dp(np.ldexp(1.0, 2 * k)))
    b = oracle_py.RefC(n, m, dp=_plain_dp)
    for t in range(14):
        x = rng.standard_normal(n)
        fa, fb = x.copy(), sc * x
        a.accel_update(fa)
        b.accel_update(fb)
        assert np.array_equal(sc * fa, fb), t
        assert a.num_vec() == b.num_vec() and a.state().list_order() == b.state().list_order(), t


def test_masked_entries_on_the_reference():
    n, m = 3001, 5
    rng = np.random.default_rng(12)
    mask = (rng.random(n) >= 0.3).astype(np.float64)
    keep = mask != 0
    a = oracle_py.RefC(n, m, dp=_seq_dp(mask))
    b = oracle_py.RefC(n, m, dp=_seq_dp(mask))
    for t in range(14):
        x = rng.standard_normal(n)
        y = np.where(keep, x, 1e3 * rng.standard_normal(n))
        a.accel_update(x)
        b.accel_update(y)
        assert np.array_equal(x[keep], y[keep]), t
        assert a.num_vec() == b.num_vec() and a.state().list_order() == b.state().list_order(), t
        for s in a.state().list_order():                       # the stored vectors too, at the unmasked entries
            assert np.array_equal(a.w(s)[keep], b.w(s)[keep]) and np.array_equal(a.v(s)[keep], b.v(s)[keep]), (t, s)
