"""The wave batch (nka_hip_batch_create_waves) as far as a machine without a GPU can see it: the host model of its sum against
exact sums and against every lost, doubled or misplaced sentinel; waves_k read off the kernel's text; the layout arithmetic the
kernel and the host share under sanitizers; the shapes of the GPU tests; the example of INTEGRATION.md; the refusals that need no
device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_step as S
import batch_waves as BWV
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nka_amd", "csrc")
NAMES = ("nka_hip_batch_create_waves", "nka_hip_batch_waves_limits")


# ---- the sum --------------------------------------------------------------------------------------------------------------------

def _inside(got, x, y, n):
    tot = X.abs_dot(x, y)
    return abs(got - X.exact_dot(x, y)) <= X.gamma(BWV.waves_k(n)) * tot


@pytest.mark.parametrize("n", BWV.CPU_LENGTHS)
def test_the_model_of_the_wave_sum_is_inside_the_bound_and_every_mutation_outside(n):
    """The lane's strided fma chain, then the butterfly in the kernel's order: inside gamma(waves_k(n)) sum|xy| of the exact sum.
    A sum that loses a sentinel, adds it twice, or takes the pair partner's element in its place is outside."""
    rng = np.random.default_rng([n, 1])
    x = BWV.planted_input(n, rng)
    y = BWV.planted_input(n, rng, prev=x)
    assert _inside(BWV.model_sum(x, y), x, y, n), n
    sent = [int(i) for i in BWV.all_sentinels(n)]
    names = BWV.sentinel_indices(n)
    assert names["wave_edges"].size >= 4 and names["ragged"].size and names["half_pair"].tolist() == [n - 1]
    assert {0, 1, 126, 127, n - 1} <= set(sent) and len(set(np.abs(x[sent]).tolist())) >= 3
    for i in sent:
        partner = (x[i ^ 1], y[i]) if (i ^ 1) < n else (0.0, y[i])      # (beyond n: the zero ld_pair returns)
        for name, terms in (("lost", []), ("doubled", [(x[i], y[i])] * 2), ("partner's element", [partner])):
            got = BWV.model_sum(x, y, take=lambda j, i=i, terms=terms: terms if j == i else [(x[j], y[j])])
            assert not _inside(got, x, y, n), (n, i, name)


def test_waves_k_is_what_the_kernel_does():
    """waves_k(n) = 2 ceil(n / 128) + 6, read off the sources: the tile and the lane's pair, one fma per element and accumulator
    in every sweep, six exchange-and-add levels in wave_sum, no step between wavefronts, and the unit says so itself."""
    unit = open(os.path.join(CSRC, "nka_batch_waves.hip")).read()
    host = open(os.path.join(CSRC, "host_logic.hpp")).read()
    dev = open(os.path.join(CSRC, "nka_device.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in unit.splitlines())
    assert re.search(r"constexpr int kWavesTile = 128;", host) and re.search(r"constexpr int kWavesGroup = 4;", host)
    assert "return 2 * (((n < 1 ? 1 : n) + kWavesTile - 1) / kWavesTile) + 6;" in host
    assert "waves_k(n) = 2 * ceil(n / 128) + 6" in unit
    # the sweep: full tiles then the ragged one, the lane's pair 2 lane of every tile
    sweep = code[code.index("void waves_sweep"):code.index("k_waves_update")]
    assert sweep.count("base + 2 * lane") == 4 and sweep.count("base += kWavesTile") == 2 and "threadIdx" not in sweep
    # every accumulation is one fma per element (q = 0, 1) into one accumulator; nothing else adds into an accumulator
    kern = code[code.index("void k_waves_update"):code.index("void launch_waves_as")]
    fmas = re.findall(r"(acc(?:\[[^\]]+\])?) = fma\(([^;]+), \1\);", kern)
    first = sorted(f[1].split(",")[0].strip() for f in fmas)
    # <d,d>, <f,f> (twice: with and without a pending pair), each weighted and plain, and the three of phase 3, whose first
    # operands fa = fl(w f) and wa = fl(w w1') are formed once per element
    assert first == sorted(["gv[q] * d", "d", "gv[q] * fv[q]", "fv[q]", "gv[q] * fv[q]", "fv[q]", "fa", "wa", "fa"]), first
    # each weighted form stands in an `if constexpr (WGT)` whose `else` is the plain form
    for wgt, plain in (("acc[NNRM - 1] = fma(gv[q] * d, d, acc[NNRM - 1]);", "acc[NNRM - 1] = fma(d, d, acc[NNRM - 1]);"),
                       ("acc[0] = fma(gv[q] * fv[q], fv[q], acc[0]);", "acc[0] = fma(fv[q], fv[q], acc[0]);"),
                       ("acc = fma(gv[q] * fv[q], fv[q], acc);", "acc = fma(fv[q], fv[q], acc);")):
        assert kern.count(f"if constexpr (WGT) {wgt} else {plain}") == 1, wgt
    assert kern.count("double fa = fq;") == 1 and kern.count("if constexpr (WGT) fa = gv[q] * fq;") == 1
    assert kern.count("double wa = wn;") == 1 and kern.count("if constexpr (WGT) wa = gv[q] * wn;") == 1
    assert len(re.findall(r"acc(?:\[[^\]]+\])?\s*(?:\+=|= acc)", kern)) == 0
    assert kern.count("for (int q = 0; q < 2; q++)") >= 4
    # the butterfly: wave_sum, six levels, through registers
    ws = dev[dev.index("__device__ __forceinline__ double wave_sum(double x) {"):]
    ws = ws[:ws.index("}") + 1]
    assert len(re.findall(r"swap_sum32|swap_sum16|row_shl_sum<\d>", ws)) == BWV.LEVELS == 6
    assert "wave_sum(" in kern and "batch_block_sum" not in code
    # design 1: no workgroup barrier, no atomics, no LDS array of sums between wavefronts
    for word in ("__syncthreads", "atomic", "s_barrier", "__shared__ double"):
        assert word not in code.replace('"wavefront"', ""), word
    assert code.count("wave_sync();") >= 3 and "__builtin_amdgcn_wave_barrier()" in code
    for n in (1, 127, 128, 129, 255, 257, 1027, 2048, 4096):
        assert BWV.waves_k(n) == 2 * -(-n // 128) + 6
    assert (BWV.waves_k(128), BWV.waves_k(129), BWV.waves_k(2048)) == (8, 10, 38)


# ---- the layout -----------------------------------------------------------------------------------------------------------------

def _layout_table():
    """`make wavescheck` builds and runs tests/c/batch_waves_layout_check.cpp (-fsanitize=address,undefined; nothing is preloaded);
    run once more for the table it prints: {mvec: (copy_bytes, total bytes)}."""
    subprocess.run(["make", "-s", "-C", CSRC, "wavescheck"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build_host", "batch_waves_layout_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("waves ")]
    return {int(r[1]): (int(r[2]), int(r[3])) for r in rows}


def test_layout_arithmetic_for_every_mvec_under_sanitizers():
    table = _layout_table()
    assert sorted(table) == list(range(1, 33))
    for mvec, (copy, total) in table.items():
        assert copy % 16 == 0 and total == 4 * copy <= BWV.LDS_LIMIT, mvec
        assert copy == BWV.copy_bytes(mvec), (mvec, copy, BWV.copy_bytes(mvec))
    assert table[20][1] < 24 * 1024 and table[32][1] < 48 * 1024
    for nsys in range(1, 4098):
        assert BWV.ngroup(nsys) * BWV.GROUP >= nsys > (BWV.ngroup(nsys) - 1) * BWV.GROUP


def test_the_shapes_of_the_gpu_tests():
    import nka_amd
    group, cap = nka_amd.batch_waves_limits()                # (loads on any machine: the limits need no device)
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert group == BWV.GROUP and f"NKA_HIP_BATCH_WAVES_MAX_VLEN = {cap} " in hdr and cap >= 128 and cap & (cap - 1) == 0
    assert BWV.NSYS % BWV.GROUP == 3, "the last workgroup has one absent wavefront"
    assert BWV.shapes(2048) == [1, 2, 3, 127, 128, 129, 255, 257, 1027, 2047, 2048]
    assert BWV.shapes(1024) == [1, 2, 3, 127, 128, 129, 255, 257, 899, 1023, 1024] and 899 == 7 * 128 + 3
    # the large case: the boundary is crossed, at most nine systems run, the witnesses are masked
    sh = BWV.large_shape(cap)
    each = sh["sys_bytes"] * sh["nsys"]
    kb = sh["boundary"]
    assert each > 2 ** 32 and kb * sh["sys_bytes"] <= 2 ** 32 < (kb + 1) * sh["sys_bytes"]
    assert len(sh["active"]) <= BWV.MAX_ACTIVE and {0, kb - 1, kb, sh["nsys"] - 1} <= set(sh["active"])
    assert sh["witnesses"] and not set(sh["witnesses"]) & set(sh["active"]) and sum(BWV.large_bytes(sh).values()) <= 16 * 2 ** 30
    assert any(8 * BWV.slot_stride(cap) * 4 * k >= 2 ** 32 for k in sh["active"])
    # the step test: thresholds retire systems mid-sequence, at three calls or more, and some systems never retire
    import test_batch_waves_gpu as G
    for n in sorted({min(n, BWV.several_tiles(cap)) for n in BWV.STEP_LENGTHS} | set(BWV.STEP_LENGTHS)):
        for flavor in (0, 1, 2):
            r = G.step_retirements(n, flavor)
            assert len(set(r[r >= 0].tolist())) >= 3 and (r < 0).any() and (r[r >= 0] > 0).all(), (n, flavor, r)


def test_the_replay_budget_of_the_graph_test_holds_on_the_oracle(oracle):
    """The solve the GPU test replays (tests/batch_step.py) with np.dot sums on the oracle: every system retires SOLVE_SLACK steps
    inside SOLVE_REPLAYS, at three or more different iterations, none at the first call.  96 unknowns: inside this kind's cap."""
    retired = S.solve_on_the_oracle(oracle)
    assert (retired >= 1).all() and retired.max() <= S.SOLVE_REPLAYS - S.SOLVE_SLACK and len(set(retired.tolist())) >= 3, retired
    assert 64 < S.SOLVE_VLEN <= 128


# ---- documents and surface ----------------------------------------------------------------------------------------------------------

def test_integration_md_example_of_a_wave_batch_compiles(tmp_path):
    """The C example of INTEGRATION.md for short systems against include/nka_hip_batch.h (syntax only); fenced ```C like the wide
    and the lane batch's."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_waves" in b]
    assert len(blocks) == 1 and "nka_hip_batch_waves_limits" in blocks[0] and "NKA_HIP_BATCH_KIND_WAVES" in blocks[0]
    src = tmp_path / "wave_batch.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_header_and_library_carry_the_entries_and_refuse_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert re.search(r"^ \*   WAVES ", hdr, flags=re.M) and "NKA_HIP_BATCH_KIND_WAVES = 3" in hdr
    L, D = nka_amd.load(), _lib.load_diag()
    for name in NAMES:
        assert hasattr(L, name) and hasattr(D, name) and name in _lib.BATCH_SIGNATURES and name in hdr, name
    g, cap = C.c_int32(), C.c_int64()
    assert L.nka_hip_batch_waves_limits(C.byref(g), C.byref(cap)) == 0 and g.value == 4
    assert L.nka_hip_batch_create_waves(None, 1, 1, 1, 0.01, 0, 0, None) == -1
    h = C.c_void_p()
    for nsys, vlen, mvec, vtol in ((0, 129, 3, 0.01), (4, cap.value + 1, 3, 0.01), (4, 0, 3, 0.01), (4, 129, 33, 0.01), (4, 129, 0, 0.01),
                                   (4, 129, 3, 0.0)):       # (refused before any device is looked for)
        assert L.nka_hip_batch_create_waves(C.byref(h), nsys, vlen, mvec, vtol, 0, 0, None) == -1 and h.value is None
    assert L.nka_hip_last_error()
    assert (nka_amd.KIND_WAVES, nka_amd.KIND_LANES, nka_amd.KIND_WIDE, nka_amd.KIND_NARROW) == (3, 2, 1, 0)
    for kw in ({"wide": True}, {"lanes": True}, {"storage": nka_amd.STORE_F32}):
        with pytest.raises(nka_amd.NKAError):
            nka_amd.nka_batch().init(4, 64, 3, waves=True, **kw)
