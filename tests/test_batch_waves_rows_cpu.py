"""The wave batch's scalar step on the whole wavefront (nka_hip_batch_create_waves_rows; include/nka_hip_batch.h, WAVES ROWS), the
parts that need no GPU.

  1 the census     the sequences of the GPU twin test (batch_wide_rows.script at nine systems, the seeds and the mvec of
                   batch_waves_rows) reach every branch of the drop logic when the oracle alone runs them: a short census on the
                   GPU is then the kernel's doing
  2 the claim      batch_wide_rows.model_step -- the numpy model of batch_scalar_step_rows -- is the oracle's scalar_step at the
                   cap's list length (tests/test_batch_wide_rows_cpu.py holds it at every length 1 ... 33)
  3 the mirror     the header, the exports, BATCH_SIGNATURES, the Python side, the refusals that need no device
  4 the unit       one __global__, no workgroup barrier, the wave_sync ahead of the wavefront step
  5 the LDS        tests/c/batch_waves_rows_layout_check.cpp, a stand-alone program under AddressSanitizer and UBSan; the cap it
                   prints is the library's
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_waves_rows as WR
import batch_wide_rows as R
import test_batch_wide_rows_cpu as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nka_amd", "csrc")
EINVAL = -1


# ---- 1. the census -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mvec,flavor", [(m, 2) for m in WR.MVECS] + [(10, 0), (10, 1), (20, 0), (20, 1)])
def test_the_sequences_meet_the_census_on_the_reference(oracle, mvec, flavor):
    """batch_wide_rows.script for nine systems, at the seeds of the GPU twin test's grid, through nine oracles: per mvec >= 2 at
    least one update with two dependence drops, one with a drop at the first older position, one at the last, a capacity drop, a
    last position evaluated behind a drop, a relax by s == 0 and a solve without a new pair.  mvec = 6 and the cap among them."""
    vlen, mvec = WR.VLENS[0], WR.mvec_of(mvec)
    oras = [oracle.OracleNKA(vlen, mvec, flavor) for _ in range(WR.NSYS)]
    census, older_counts = {}, set()
    for ev in R.script([vlen] * WR.NSYS, mvec, WR.twin_seed(mvec, flavor), ill=WR.ILL):
        if ev["vtol"] is not None:
            for o in oras:
                o.set_vec_tol(ev["vtol"])
        for k in ev["relax"]:
            oras[k].relax()
        for k in ev["restart"]:
            oras[k].restart()
        counts = set()
        for k, x in ev["inputs"].items():
            before = oras[k].state()
            oras[k].accel_update(x.copy())
            for tag in R.census_of(before, oras[k].state(), mvec):
                census[tag] = census.get(tag, 0) + 1
            counts.add(max(len(before.list_order()) - 1, 0))
        if len(ev["inputs"]) == WR.NSYS:
            older_counts.add(len(counts))
    assert max(older_counts) >= 2 or mvec == 1      # one launch holds lists of different length
    if mvec >= 2:
        assert not R.census_short(census), (mvec, census)
    print(f"census on the reference, mvec {mvec}, flavour {flavor}: {sorted(census.items())}")


def test_the_grid_of_the_gpu_tests():
    cap = WR.cap()
    assert WR.NSYS == 9 and WR.NSYS % 4 == 1, "the last workgroup has three absent wavefronts"
    assert WR.ILL < WR.NSYS and WR.ILL not in (1, 5, 2, 6, 3), "the ill system is neither relaxed, restarted nor retired by the script"
    assert WR.VLENS == (65, 129, 385) and [-(-n // 128) for n in WR.VLENS] == [1, 2, 4] and 385 == 3 * 128 + 1
    assert tuple(WR.mvec_of(m) for m in WR.MVECS) == (1, 2, 5, 6, 10, 11, 20, 21, cap) and cap > 21      # both sides of 6 / 11 / 21 rows, and the last class


# ---- 2. the claim --------------------------------------------------------------------------------------------------------------------

def test_the_rows_model_is_the_oracles_scalar_step_at_the_caps_list_length(oracle):
    """The loop of tests/test_batch_wide_rows_cpu.py at mvec = the cap: list lengths 0 ... cap + 1, dependence drops anywhere, the
    first older pivot a few ulp either side of vtol^2, s == 0, a NaN, a relax and a restart."""
    mvec = WR.cap()
    rng = np.random.default_rng(7000 + mvec)
    ora = oracle.OracleNKA(8, mvec, oracle.C_FLAVOR)
    ora.set_vec_tol(TC.VTOL)
    W = np.zeros((mvec + 2, 40))
    lengths, drops, caps, nclose = set(), 0, 0, 0
    for t in range(2 * mvec + 44):
        kind = TC.KINDS[t % len(TC.KINDS)] if t > mvec + 2 else "random"
        if t == mvec + 9:
            ora.relax()
        if t == mvec + 15:
            ora.restart()
        st0, order0, s, hrow, b = TC._gram_case(rng, ora, W, mvec, kind, nclose)
        work = R.Work(st0, mvec, TC.VTOL)
        new = ora.scalar_step(s, hrow, b)
        slot, dep, cap = R.model_step(work, s, hrow, b)
        assert slot == new and TC._agrees(work, ora.state(), order0 if (st0.pending and s != 0.0) else [], b), (t, kind, order0)
        lengths.add(len(order0))
        drops += len(dep)
        caps += cap is not None
        nclose += kind == "close" and st0.pending and len(order0) > 1
    assert lengths >= set(range(0, mvec + 2)) and caps >= 1 and drops >= 2, (sorted(lengths), caps, drops)


# ---- 3. the mirror -------------------------------------------------------------------------------------------------------------------

CREATE = (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_int32])
LIMITS = (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64)])


def test_header_exports_signatures_and_refusals_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    decl = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert re.search(r"int nka_hip_batch_create_waves_rows\(nka_hip_batch_t \*out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,\s*"
                     r"int32_t flavor, int32_t device, void \*stream, int32_t ext\);", decl)
    assert "int nka_hip_batch_waves_rows_limits(int32_t *max_mvec, int32_t mvec, int64_t *lds_bytes);" in decl
    L, D = nka_amd.load(), _lib.load_diag()
    for name, (res, args) in (("nka_hip_batch_create_waves_rows", CREATE), ("nka_hip_batch_waves_rows_limits", LIMITS)):
        assert hasattr(L, name) and hasattr(D, name), name
        assert _lib.BATCH_SIGNATURES[name][0] is res and list(_lib.BATCH_SIGNATURES[name][1]) == args, name
    # the limits: derived, exported, mirrored
    cap, lds = C.c_int32(), C.c_int64()
    assert L.nka_hip_batch_waves_rows_limits(C.byref(cap), 20, C.byref(lds)) == 0 and lds.value == 36672
    assert nka_amd.batch_waves_rows_limits() == (cap.value, nka_amd.batch_waves_rows_limits(cap.value)[1])
    assert nka_amd.batch_waves_rows_limits(20) == (cap.value, 36672) and 21 < cap.value <= nka_amd.BATCH_MAX_MVEC
    assert L.nka_hip_batch_waves_rows_limits(None, cap.value, None) == 0
    assert nka_amd.batch_waves_rows_limits()[1] <= WR.LDS_LIMIT
    for bad in (0, -1, cap.value + 1, 33):
        assert L.nka_hip_batch_waves_rows_limits(C.byref(cap), bad, C.byref(lds)) == EINVAL and str(cap.value).encode() in L.nka_hip_last_error()
    # the working copies alone are those of the wave batch: the matrix is all that is added (waves_lds: 4 x copy_bytes)
    for mvec in range(1, cap.value + 1):
        total = nka_amd.batch_waves_rows_limits(mvec)[1]
        matrix = (8 * (mvec + 2) ** 2 + 15) // 16 * 16
        assert total % 64 == 0 and total - 4 * matrix > 0 and total <= WR.LDS_LIMIT, mvec
    # refusals before any device is looked for
    h = C.c_void_p()
    assert L.nka_hip_batch_create_waves_rows(None, 1, 1, 1, 0.01, 0, 0, None, 0) == EINVAL
    _, vcap = nka_amd.batch_waves_limits()
    for nsys, vlen, mvec, vtol, ext, word in ((4, 129, 3, 0.01, 2, b"ext"), (4, 129, 3, 0.01, -1, b"ext"), (4, 129, cap.value + 1, 0.01, 0, b"1 ... %d" % cap.value),
                                              (4, 129, cap.value + 1, 0.01, 1, b"1 ... %d" % cap.value), (0, 129, 3, 0.01, 0, b"nsys"),
                                              (4, vcap + 1, 3, 0.01, 0, b"vlen"), (4, 0, 3, 0.01, 1, b"vlen"), (4, 129, 33, 0.01, 0, b"mvec"),
                                              (4, 129, 0, 0.01, 1, b"mvec"), (4, 129, 3, 0.0, 0, b"vtol")):
        h.value = 1
        assert L.nka_hip_batch_create_waves_rows(C.byref(h), nsys, vlen, mvec, vtol, 0, 0, None, ext) == EINVAL and h.value is None
        err = L.nka_hip_last_error()
        assert b"nka_hip_batch_create_waves_rows" in err and word in err, (err, word)
    with pytest.raises(nka_amd.NKAError, match="waves=True"):
        nka_amd.nka_batch().init(4, 129, 3, rows=True)
    for kw in ({"wide": True}, {"lanes": True}, {"storage": nka_amd.STORE_F32}):
        with pytest.raises(nka_amd.NKAError):
            nka_amd.nka_batch().init(4, 64, 3, waves=True, rows=True, **kw)
    assert L.nka_hip_batch_offers_scalar_step(None) < 0 and L.nka_hip_last_error()


def test_the_header_carries_the_paragraph():
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    m = re.search(r"^ \*   WAVES ROWS  nka_hip_batch_create_waves_rows: (.*?)^ \*   OUT OF SCOPE", hdr, flags=re.M | re.S)
    assert m, "the paragraph behind SCALAR STEP"
    par = " ".join(m.group(1).replace("\n *", " ").split())
    for phrase in ("nka_hip_batch_set_scalar_step", "NKA_HIP_BATCH_SCALAR_WAVEFRONT", "BOTH STEPS LEAVE THE SAME BITS", "nka_hip_batch_kind is 3",
                   "nka_hip_batch_waves_rows_limits", "64 KiB", "36 672", "64 832", "68 992", "no workgroup barrier",
                   "a captured call keeps the step it was captured with", "nothing further is allocated"):
        assert phrase in par, phrase
    assert hdr.index("*   SCALAR STEP  nka_hip_batch_set_scalar_step:") < m.start()
    step = hdr[hdr.index("*   SCALAR STEP  nka_hip_batch_set_scalar_step:"):m.start()]
    assert "the wave batch and the lane batch keep the one-thread" not in step, "the wave batch is no longer a follow-up"
    assert "WAVES ROWS" in step
    # no ratio is quoted without the record it comes from
    if not os.path.exists(os.path.join(ROOT, "profiles", "r23", "batch_waves_rows_throughput.txt")):
        assert "MEASURED" not in par or not re.search(r"\d\.\d\d", par[par.index("MEASURED"):]), "a ratio without its record"


# ---- 4. the unit ---------------------------------------------------------------------------------------------------------------------

def test_the_one_wave_unit_holds_the_wavefront_step():
    """k_waves_update stays the one kernel of the one wave unit: the wavefront step is one more member of the trailing pack, phase 4
    branches on it at compile time, a wave_sync stands between lane 0's stores of phase 3 and the step, and nothing at workgroup
    scope was added."""
    unit = open(os.path.join(CSRC, "nka_batch_waves.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in unit.splitlines())
    assert code.count("__global__") == 1 and code.count("void waves_sweep(") == 1 and code.count("void wave_sync()") == 1
    for word in ("__syncthreads", "atomic", "s_barrier", "__shared__ double", "hipFuncSetAttribute"):
        assert word not in code.replace('"wavefront"', ""), word
    kern = code[code.index("void k_waves_update"):code.index("void launch_waves_rows_nl")]
    assert "template <int NLMAX> struct WavesRows {};" in code and "constexpr int ROWS = waves_rows_nl<Pack...>;" in kern
    phase4 = kern[kern.index("if constexpr (ROWS > 0) {"):kern.index("for (int i = lane; i < nh; i += 64) ctl.h()[i] = L.h[i];")]
    lines = [ln.strip() for ln in phase4.splitlines() if ln.strip()]
    assert lines[1] == "wave_sync();" and lines[2].startswith("batch_scalar_step_rows<ROWS>(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr, ")
    assert "if (lane == 0) batch_scalar_step(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr);" in phase4 and lines[-1] == "wave_sync();"
    assert "smem + wl.a_base(wv)" in phase4
    # the launch: the instance and its LDS size are chosen together, when the call is enqueued
    launch = code[code.index("void launch_waves_rows_nl"):code.index("void launch_waves_len")]
    assert "nka_host::waves_rows_lds(b->k.mvec).bytes()" in launch and "nka_host::waves_lds(b->k.mvec).bytes()" in launch
    assert "b->waves_rows && b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT" in launch
    for nl in ("6", "11", "21", "nka_host::waves_rows_max_mvec() + 1"):
        assert f"launch_waves_rows_nl<COMB, {nl}, Pack...>" in launch, nl
    host = open(os.path.join(CSRC, "host_logic.hpp")).read()
    assert "constexpr int waves_rows_max_mvec()" in host and not re.search(r"waves_rows_max_mvec\(\)\s*\{\s*return \d+;", host), "derived, not a literal"


# ---- 5. the LDS ----------------------------------------------------------------------------------------------------------------------

def test_the_lds_of_the_wavefront_step_is_laid_out_without_overlap_and_the_cap_is_the_librarys():
    """tests/c/batch_waves_rows_layout_check.cpp paints every piece of waves_rows_lds(mvec) for mvec 1 ... cap and all four
    wavefronts: no overlap, doubles on 8 bytes, copies and matrices on 16, at most 64 KiB at the cap and more at cap + 1.  Built
    with the sanitizers by `make wavesrowscheck`, run as a program."""
    import nka_amd
    subprocess.run(["make", "-s", "-C", CSRC, "wavesrowscheck"], check=True)
    out = subprocess.run([os.path.join(CSRC, "build_host", "batch_waves_rows_layout_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "batch_waves_rows_layout_check: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    cap = int(re.search(r"^cap (\d+)$", out.stdout, flags=re.M).group(1))
    assert cap == nka_amd.batch_waves_rows_limits()[0] == WR.cap()
    table = {int(r[1]): tuple(int(v) for v in r[2:]) for r in (ln.split() for ln in out.stdout.splitlines() if ln.startswith("waves_rows "))}
    assert sorted(table) == list(range(1, cap + 2))
    for mvec in range(1, cap + 1):
        copy, a, total = table[mvec]
        assert total == 4 * (copy + a) == nka_amd.batch_waves_rows_limits(mvec)[1] <= WR.LDS_LIMIT, mvec
    assert table[cap + 1][2] > WR.LDS_LIMIT
    assert (table[20][2], table[28][2], table[29][2]) == (36672, 64832, 68992) if cap == 28 else True
