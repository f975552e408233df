"""The solve step of a wide batch (nka_hip_batch_create_wide_step) as far as a machine without a GPU can see it: the symbols and
the refusals that need no device, the host model of the chunk-order <f,f> against the bound of the GPU test with every
partial lost or doubled outside it, the precondition on that test's inputs, its solve on the oracle, the layout of the new
buffer under sanitizers, and the example of INTEGRATION.md."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_wide as BW
import batch_wide_step as WS
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_entries_exist_and_refuse_on_any_machine():
    import nka_amd
    L = nka_amd.load()
    chunk, cap = nka_amd.batch_wide_limits()
    h = C.c_void_p()
    for nsys, vlen, mvec in [(0, 8, 3), (65536, 8, 3), (4, 0, 3), (4, cap + 1, 3), (4, 8, 0), (4, 8, nka_amd.BATCH_MAX_MVEC + 1)]:
        assert L.nka_hip_batch_create_wide_step(C.byref(h), nsys, vlen, mvec, 0.01, -1, 0, None) == -1 and h.value is None
        assert b"nka_hip_batch_create_wide_step" in L.nka_hip_last_error()
    assert L.nka_hip_batch_create_wide_step(None, 1, 1, 1, 0.01, 0, 0, None) == -1
    assert L.nka_hip_batch_offers_step(None) < 0 and L.nka_hip_last_error()
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert "nka_hip_batch_create_wide_step" in hdr and "nka_hip_batch_offers_step" in hdr
    with pytest.raises(nka_amd.NKAError, match="wide=True"):      # refused before any device is asked for
        nka_amd.nka_batch().init(3, 33, 3, step=True)


def _norm_of(parts, chunks):
    return math.sqrt(BW.model_sum_of(parts, chunks))


@pytest.mark.parametrize("chunks", [2, 9, 10, 17, 257, 512])
def test_the_model_of_the_chunk_order_norm_is_inside_the_bound_and_every_lost_or_doubled_partial_outside(chunks):
    """sqrt of the host model of the chunk-order <f,f> (batch_wide.model_partials / model_sum_of) against the bound of GPU test 4,
    on planted inputs at the library's C: inside it, and outside with ANY ONE partial lost or added twice."""
    c, cap = BW.limits()
    n = (chunks - 1) * c + 1 if chunks != 512 else cap
    assert BW.nchunk(n, c) == chunks and n <= cap
    f = BW.wide_planted_input(n, np.random.default_rng([45, n]), C=c)
    assert BW.undetectable_chunks(f, f, BW.wide_k(n, c), c) == []
    exact = X.exact_dot(f, f)
    parts = BW.model_partials(f, f, c)
    whole = list(range(chunks))
    ok, ratio = WS.norm_inside(_norm_of(parts, whole), f, n, c, exact=exact)
    assert ok, (chunks, ratio, WS.norm_bound(n, c) / X.U)
    for j in whole:
        lost, twice = whole[:j] + whole[j + 1:], whole[:j + 1] + whole[j:]
        assert not WS.norm_inside(_norm_of(parts, lost), f, n, c, exact=exact)[0], (chunks, "lost", j)
        assert not WS.norm_inside(_norm_of(parts, twice), f, n, c, exact=exact)[0], (chunks, "twice", j)


def test_the_inputs_of_the_gpu_test_of_the_norm_meet_their_precondition():
    c, cap = BW.limits()
    for n in WS.exact_shapes(c):
        assert n <= cap
        rows = WS.exact_inputs(n, c)
        assert len(rows) == WS.EXACT_NSYS
        for f in rows:
            assert f.size == n and BW.undetectable_chunks(f, f, BW.wide_k(n, c), c) == [], n
    assert [BW.nchunk(n, c) for n in WS.exact_shapes(c)] == [2, 3, 10, 17, 257]


def test_the_wide_solve_of_the_gpu_test_converges_on_the_oracle(oracle):
    """The inputs of GPU test 7 are chosen here: every system retires SOLVE_SLACK steps inside the budget, at three or more
    different iterations, and none at the first call (tol = 0 there)."""
    retired = WS.solve_on_the_oracle(oracle, BW.limits()[0])
    assert (retired >= 1).all(), retired
    assert retired.max() <= WS.SOLVE_REPLAYS - WS.SOLVE_SLACK, retired
    assert len(set(retired.tolist())) >= 3, retired


def test_layout_of_the_step_buffer_against_a_brute_force_model_under_sanitizers():
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "widestepcheck"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_wide_step_layout_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_integration_md_example_of_a_wide_step_compiles(tmp_path):
    """The C example of INTEGRATION.md for systems too long for one workgroup creates a batch with the step and runs it; against
    include/nka_hip_batch.h (syntax only)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_wide_step" in b]
    assert len(blocks) == 1 and "nka_hip_batch_accel_step" in blocks[0] and "nka_hip_batch_offers_step" in blocks[0]
    src = tmp_path / "wide_step.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
