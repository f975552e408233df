"""The check of tests/test_batch_weights_gpu.py (test 4: every weighted fast sum of a batch inside
gamma(batch_k(n)) * sum|fl(w x) y| of the exact sum of fl(w x) and y) has teeth at its shapes, shown without a GPU: the
kernel's weighted sum restated on the host (batch_weights.thread_sums, workgroup_sum: thread t owns the pairs 2t, 2t + 1 of every
512, per-thread fma order, butterfly, wavefronts 0..3) stays inside the bound on the inputs and weights of that test, and
each of four mutations falls outside it, at every sentinel of the shape."""
import math

import numpy as np
import pytest

import batch_weights as BW
import exact_sums as X


def _operands(n):
    """The operands of the four sums of one update, from the planted inputs and the weights of system 0 of test 4; the
    normalisation uses the weighted norm, as the device does."""
    rng = np.random.default_rng([n, 0])
    w = BW.system_weights(n, 1)[0]
    f_a = X.batch_planted_input(n, rng)
    f_b = X.batch_planted_input(n, rng, prev=f_a)
    f_c = X.batch_planted_input(n, rng, prev=f_b)
    f = X.batch_planted_input(n, rng, prev=f_c)
    d_old = f_a - f_b
    w_old = d_old / math.sqrt(float(np.dot(w * d_old, d_old)))
    d = f_c - f
    w1n = d / math.sqrt(float(np.dot(w * d, d)))
    return w, {"<d,d>": (d, d), "<f,w1'>": (f, w1n), "<w1',w_p>": (w1n, w_old), "<f,w_p>": (f, w_old)}


def _inside(got, w, x, y, n):
    a = w * x
    return abs(got - X.exact_dot(a, y)) <= X.gamma(X.batch_k(n)) * X.abs_dot(a, y)


@pytest.mark.parametrize("n", [65, 513, 4099])
def test_weight_draw_rule(n):
    for k in range(6):
        w = BW.draw_weights(n, np.random.default_rng([BW.WEIGHT_SEED, n, k]))
        BW.assert_weight_rule(n, w)
        if n > 100:
            assert 0.03 * n < (w == 0).sum() < 0.2 * n                 # about 10 % zeros, none of them at a sentinel
        nz = w[w > 0]
        assert nz.min() >= 0.125 and nz.max() <= 8.0
        assert (np.log2(nz) != np.round(np.log2(nz))).mean() > 0.9     # general weights, not powers of two


@pytest.mark.parametrize("n", [65, 513, 4099])
def test_the_weighted_model_is_inside_the_bound_and_every_mutation_outside(n):
    w, sums = _operands(n)
    idx = X.batch_all_sentinels(n)
    picks = [int(i) for i in idx]                                      # every sentinel of the shape
    for what, (x, y) in sums.items():
        acc = BW.thread_sums(w, x, y)
        assert _inside(BW.workgroup_sum(acc), w, x, y, n), (n, what)

        def mutated(xm, wy, i):
            return BW.workgroup_sum(BW.thread_sums(w, xm, y, wy=wy, base=acc, only=BW.owner(i)))
        for i in picks:
            where = (n, what, i)
            one = w.copy()
            one[i] = 1.0                                               # the weight ignored at one sentinel
            assert not _inside(mutated(x, one, i), w, x, y, n), (where, "weight ignored")
            if (i ^ 1) < n:                                            # the weight of the pair's other element
                other = w.copy()
                other[i] = w[i ^ 1]
                assert not _inside(mutated(x, other, i), w, x, y, n), (where, "partner's weight")
            for factor, name in ((0.0, "lost"), (2.0, "doubled")):
                xm = x.copy()
                xm[i] *= factor
                got = mutated(xm, None, i)                   # (the sentinel's product, not the element: <d,d> too)
                assert not _inside(got, w, x, y, n), (where, name)
