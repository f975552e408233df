"""The wide batched accelerator (nka_hip_batch_create_wide) as far as a machine without a GPU can see it: the symbols and
the refusals that need no device, the K of its sums against a host model of the chunked sum, the sentinels of the GPU
tests, the layout arithmetic under sanitizers, and the example of INTEGRATION.md."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_wide as BW
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_reports_the_two_constants_of_the_header():
    import nka_amd
    chunk, cap = nka_amd.batch_wide_limits()
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert f"NKA_HIP_BATCH_WIDE_CHUNK = {chunk}" in hdr and f"NKA_HIP_BATCH_WIDE_MAX_VLEN = {cap}" in hdr
    assert chunk in BW.CANDIDATES and chunk % X.BATCH_TILE == 0
    assert cap <= 1024 * chunk and cap & (cap - 1) == 0 and cap > nka_amd.BATCH_MAX_VLEN


def test_wide_create_refuses_what_lies_outside_the_limits_on_any_machine():
    import nka_amd
    L = nka_amd.load()
    chunk, cap = nka_amd.batch_wide_limits()
    h = C.c_void_p()
    for nsys, vlen, mvec in [(0, 8, 3), (65536, 8, 3), (4, 0, 3), (4, cap + 1, 3), (4, 8, 0), (4, 8, nka_amd.BATCH_MAX_MVEC + 1)]:
        assert L.nka_hip_batch_create_wide(C.byref(h), nsys, vlen, mvec, 0.01, -1, 0, None) == -1 and h.value is None
        assert L.nka_hip_last_error()
    assert L.nka_hip_batch_is_wide(None) < 0


def test_wide_k_equals_batch_k_up_to_one_chunk_and_follows_the_kernels_beyond():
    for c in BW.CANDIDATES:
        for n in (1, 2, 65, 513, c - 1, c):
            assert BW.wide_k(n, c) == X.batch_k(n), (c, n)
        assert BW.wide_k(c + 1, c) == 2 * (c // 512) + 9 + 1
        assert BW.wide_k(2 * c + 513, c) == 2 * (c // 512) + 9 + 2
        assert BW.wide_k(1024 * c, c) == 2 * (c // 512) + 9 + 1023
        # the chunk counts at which the chain of k_wide_scalar and the staging loop of wide_norm_sum change behaviour
        for n, chunks in ((8 * c + 1, 9), (9 * c, 9), (9 * c + 1, 10), (15 * c + 513, 16), (16 * c + 1, 17), (17 * c + 33, 18),
                          (256 * c, 256), (256 * c + 1, 257), (256 * c + 513, 257), (512 * c, 512)):
            assert BW.nchunk(n, c) == chunks and BW.wide_k(n, c) == 2 * (c // 512) + 9 + (chunks - 1), (c, n)
    assert [BW.wide_k(n, 4096) for n in (4096, 4097, 8705, 1 << 20)] == [25, 26, 27, 280]
    assert [BW.wide_k(n, 2048) for n in (16 * 2048 + 1, 256 * 2048 + 1, 1 << 20)] == [33, 273, 528]


def test_wide_sentinels_are_those_of_every_chunk_and_its_two_ends():
    for c in BW.CANDIDATES:
        for n in (c + 1, 2 * c + 513):
            idx = BW.wide_sentinel_indices(n, c)
            assert idx.min() == 0 and idx.max() == n - 1 and np.unique(idx).size == idx.size
            for k in range(BW.nchunk(n, c)):
                lo, ln = k * c, min(c, n - k * c)
                assert {lo, lo + ln - 1} <= set(idx)
                assert set(lo + X.batch_all_sentinels(ln)) <= set(idx)
        assert c in BW.wide_sentinel_indices(c + 1, c) and c - 1 in BW.wide_sentinel_indices(c + 1, c)      # the chunk of one element


def _pairs(n, c, rng):
    """The operands of the four sums an update forms, from wide_planted_input (tests/test_exact_sums_cpu.py: _batch_pairs)."""
    f_a = BW.wide_planted_input(n, rng, C=c)
    f_b = BW.wide_planted_input(n, rng, prev=f_a, C=c)
    f_c = BW.wide_planted_input(n, rng, prev=f_b, C=c)
    f = BW.wide_planted_input(n, rng, prev=f_c, C=c)
    d_old = f_a - f_b
    w_old = d_old / math.sqrt(float(np.dot(d_old, d_old)))
    d = f_c - f
    w1n = d / math.sqrt(float(np.dot(d, d)))
    return {"<d,d>": (d, d), "<f,w1'>": (f, w1n), "<w1',w_p>": (w1n, w_old), "<f,w_p>": (f, w_old)}


@pytest.mark.parametrize("c", BW.CANDIDATES)
def test_the_host_model_of_the_chunked_sum_is_inside_the_bound_and_every_sentinel_is_seen(c):
    """Per-thread chains, butterfly, wavefronts, chunk order (batch_wide.model_sum) at 2C + 513 and C + 1: the model is inside
    gamma(wide_k(n)) * sum|xy| on adversarial exponents and on the planted inputs; every sentinel's product exceeds twice the
    bound plus the rounding of the exact sum (exact_sums.detectable), so a sum that lost or doubled it cannot pass; and the
    long way round for a sample -- the two ends of every chunk and every 23rd sentinel --: the model with that sentinel lost
    or doubled lies outside the bound around the exact sum."""
    for n in (2 * c + 513, c + 1):
        k = BW.wide_k(n, c)
        bound = X.gamma(k)
        for seed in range(3):
            rng = np.random.default_rng(1000 * n + seed)
            x = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 30, n))
            y = rng.standard_normal(n)
            err = abs(BW.model_sum(x, y, c) - X.exact_dot(x, y))
            assert err <= bound * X.abs_dot(x, y), (c, n, seed, err / (X.U * X.abs_dot(x, y)), k)
        rng = np.random.default_rng([14, c, n])
        idx = BW.wide_sentinel_indices(n, c)
        ends = {e for q in range(BW.nchunk(n, c)) for e in (q * c, min((q + 1) * c, n) - 1)}
        sample = sorted(ends | set(int(i) for i in idx[::23]))
        for what, (x, y) in _pairs(n, c, rng).items():
            ex, tot = X.exact_dot(x, y), X.abs_dot(x, y)
            assert abs(BW.model_sum(x, y, c) - ex) <= bound * tot, (c, n, what)
            worst = float(np.abs(x[idx] * y[idx]).min())
            assert X.detectable(worst, bound, tot), (c, n, what, worst / tot, bound)
            for i in sample:
                for factor in (0.0, 2.0):
                    xp = x.copy()
                    xp[i] *= factor
                    yp = xp if y is x else y
                    assert abs(BW.model_sum(xp, yp, c) - ex) > bound * tot, (c, n, what, i, factor)


@pytest.mark.parametrize("which", ["8C+1", "9C+1", "16C+1", "256C+1", "cap"])
def test_a_chunk_partial_lost_or_added_twice_breaks_the_bound_at_every_chunk_count_the_gpu_tests_run(which):
    """9, 10, 17, 257 and 512 chunks of the library's C, the four operand pairs of an update from planted inputs: the host
    model of the chunked sum (batch_wide.model_partials, model_sum_of) is inside gamma(wide_k(n)) * sum|xy| of the exact sum,
    and with ANY ONE chunk's partial lost, or added twice, it lies outside -- so the bound of tests/test_batch_wide_gpu.py
    sees either at these shapes.  The condition the GPU tests put on their own operands (batch_wide.undetectable_chunks) holds
    for every (pair, chunk) cell.  Two failures by name: the eight-way chain of k_wide_scalar or its remainder dropping the
    last partial when (nchunk - 1) % 8 == 0, and the staging loop of wide_norm_sum dropping the partials 256 and up."""
    c, cap = BW.limits()
    n = {"8C+1": 8 * c + 1, "9C+1": 9 * c + 1, "16C+1": 16 * c + 1, "256C+1": 256 * c + 1, "cap": cap}[which]
    chunks = BW.nchunk(n, c)
    assert n <= cap and chunks == {"8C+1": 9, "9C+1": 10, "16C+1": 17, "256C+1": 257, "cap": 512}[which], (c, cap, n, chunks)
    k = BW.wide_k(n, c)
    assert k == 2 * (c // 512) + 9 + (chunks - 1)
    bound = X.gamma(k)
    whole = list(range(chunks))
    smallest = math.inf
    for what, (x, y) in _pairs(n, c, np.random.default_rng([14, c, n])).items():
        ex, tot = X.exact_dot(x, y), X.abs_dot(x, y)
        parts = BW.model_partials(x, y, c)
        assert parts.size == chunks
        assert BW.model_sum_of(parts, whole) == BW.model_sum(x, y, c)
        assert abs(BW.model_sum_of(parts, whole) - ex) <= bound * tot, (which, what)
        assert BW.undetectable_chunks(x, y, k, c) == [], (which, what)
        smallest = min(smallest, float(np.abs(BW.chunk_products(x, y, c)).min()) / tot)
        for j in whole:
            lost, twice = whole[:j] + whole[j + 1:], whole[:j + 1] + whole[j:]
            assert len(lost) == chunks - 1 and len(twice) == chunks + 1 and twice.count(j) == 2
            assert abs(BW.model_sum_of(parts, lost) - ex) > bound * tot, (which, what, "lost", j)
            assert abs(BW.model_sum_of(parts, twice) - ex) > bound * tot, (which, what, "twice", j)
        if (chunks - 1) % 8 == 0:      # whole trips of eight behind partial 0 and nothing for the remainder loop
            assert abs(BW.model_sum_of(parts, whole[:-1]) - ex) > bound * tot, (which, what, "the last partial")
        if chunks > X.BATCH_THREADS:   # one trip of the staging loop fills stage[0 .. 255]
            assert abs(BW.model_sum_of(parts, whole[:X.BATCH_THREADS]) - ex) > bound * tot, (which, what, "one staging trip")
    print(f"  {which}: smallest |p_c| / sum|xy| = {smallest:.3g}, threshold {2.0 * bound + X.U:.3g}")


def test_wide_layout_arithmetic_against_a_brute_force_model_under_sanitizers():
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "widecheck"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_wide_layout_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_integration_md_example_of_a_wide_batch_compiles(tmp_path):
    """The C example of INTEGRATION.md for systems too long for one workgroup, against include/nka_hip_batch.h (syntax only).
    Its fence is written ```C: the example of many small systems is looked up as THE block fenced ```c that creates a batch."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_wide" in b]
    assert len(blocks) == 1 and "nka_hip_batch_accel_update" in blocks[0]
    src = tmp_path / "wide_batch.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
