"""The solve step of the batched accelerator (nka_hip_batch_accel_step) as far as a machine without a GPU can see it:

  6 the host model of the new sum, dp(f, f) in the batch's fast order, is inside the bound of GPU test 2 and every mutation of
    it -- a weight ignored, the pair partner's weight, a lost element, a doubled element -- is outside, at every sentinel
  7 the solve of GPU test 4 converges on the oracle: every system retires inside the replay budget, at several iterations
  8 the device-resident loop of INTEGRATION.md compiles against include/nka_hip_batch.h"""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_step as S
import batch_weights as BW
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n", [65, 513, 4099])
def test_the_model_of_the_norm_is_inside_the_bound_and_every_mutation_outside(n, weighted):
    rng = np.random.default_rng([n, 0])
    f = X.batch_planted_input(n, rng)
    w = BW.system_weights(n, 1)[0] if weighted else np.ones(n)
    a = w * f

    def norm(acc):
        return float(np.sqrt(BW.workgroup_sum(acc)))
    acc = BW.thread_sums(w, f, f)
    ok, ratio = S.norm_inside(norm(acc), a, f, n)
    assert ok, (n, weighted, ratio)

    def mutated(fm, wy, i):
        return norm(BW.thread_sums(w, fm, f, wy=wy, base=acc, only=BW.owner(i)))
    for i in (int(i) for i in X.batch_all_sentinels(n)):
        where = (n, weighted, i)
        if weighted:
            one = w.copy()
            one[i] = 1.0
            assert not S.norm_inside(mutated(f, one, i), a, f, n)[0], (where, "weight ignored")
            if (i ^ 1) < n:
                other = w.copy()
                other[i] = w[i ^ 1]
                assert not S.norm_inside(mutated(f, other, i), a, f, n)[0], (where, "partner's weight")
        for factor, name in ((0.0, "lost"), (2.0, "doubled")):
            fm = f.copy()
            fm[i] *= factor                                  # (the sentinel's product: first operand only)
            assert not S.norm_inside(mutated(fm, None, i), a, f, n)[0], (where, name)


def test_the_solve_of_the_gpu_test_converges_on_the_oracle(oracle):
    """The inputs of GPU test 4 are chosen here: every system retires SOLVE_SLACK steps inside the budget (the device's fast
    sums may move a close call by a step, never by eight), the systems retire at three or more different iterations, and
    none retires at the first call (tol = 0 there)."""
    retired = S.solve_on_the_oracle(oracle)
    assert (retired >= 1).all(), retired
    assert retired.max() <= S.SOLVE_REPLAYS - S.SOLVE_SLACK, retired
    assert len(set(retired.tolist())) >= 3, retired


def test_integration_md_example_of_the_device_resident_loop_compiles(tmp_path):
    """The second C example of INTEGRATION.md "Many small systems" against include/nka_hip_batch.h (syntax only)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```c\n(.*?)```", text, flags=re.S) if "nka_hip_batch_accel_step" in b]
    assert len(blocks) == 1 and "fnorm" in blocks[0] and "tol" in blocks[0] and "hipMemcpy" in blocks[0]
    src = tmp_path / "device_resident_loop.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
