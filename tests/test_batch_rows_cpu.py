"""The narrow batch's scalar step on one wavefront (nka_hip_batch_create_rows; include/nka_hip_batch.h, NARROW ROWS), the parts that
need no GPU.

  1 the census     the sequences of the GPU twin test (batch_wide_rows.script at eight systems, the seeds, lengths and mvec of
                   batch_rows) reach every branch of the drop logic when the oracle alone runs them: a short census on the GPU is
                   then the kernel's doing
  2 the instance   batch_rows_nlmax holds mvec + 1 at every mvec, with its edges at 10 / 11 and 20 / 21 (the numpy model of the
                   device function against the oracle at every list length 0 ... 33: tests/test_batch_wide_rows_cpu.py)
  3 the mirror     the header, the exports, BATCH_SIGNATURES, the Python side, the refusals that need no device
  4 the units      one __global__ k_batch_update, phase 4 branching at compile time, the one-thread statements still written out,
                   no atomics and no function attribute
  5 the LDS        tests/c/batch_rows_layout_check.cpp, a stand-alone program under AddressSanitizer and UBSan; the sizes it prints
                   are the library's
"""
import ctypes as C
import os
import re
import subprocess

import pytest

import batch_rows as NR
import batch_wide_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nka_amd", "csrc")
EINVAL = -1


# ---- 1. the census -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vlen,mvec,flavor", [(n, m, 2) for n in NR.VLENS for m in NR.MVECS] +
                         [(NR.FLAVOR_VLEN, m, f) for m in (10, 20) for f in (0, 1)])
def test_the_sequences_meet_the_census_on_the_reference(oracle, vlen, mvec, flavor):
    """batch_wide_rows.script for eight systems, at every (vlen, mvec, flavour) of the GPU twin test's grid and its seeds, through
    eight oracles: per mvec >= 2 at least one update with two dependence drops, one with a drop at the first older position, one
    at the last, a capacity drop, a last position evaluated behind a drop, a relax by s == 0 and a solve without a new pair."""
    oras = [oracle.OracleNKA(vlen, mvec, flavor) for _ in range(NR.NSYS)]
    census, older_counts = {}, set()
    for ev in R.script([vlen] * NR.NSYS, mvec, NR.twin_seed(mvec, flavor), ill=NR.ILL):
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
        if len(ev["inputs"]) == NR.NSYS:
            older_counts.add(len(counts))
    assert max(older_counts) >= 2 or mvec == 1      # one launch holds lists of different length
    if mvec >= 2:
        assert not R.census_short(census), (vlen, mvec, census)
    print(f"census on the reference, vlen {vlen}, mvec {mvec}, flavour {flavor}: {sorted(census.items())}")


def test_the_grid_of_the_gpu_tests():
    assert NR.NSYS == 8 and NR.ILL == 7 and NR.ILL not in (1, 5, 2, 6, 3), "the ill system is neither relaxed, restarted nor retired by the script"
    assert NR.VLENS == (65, 513, 1025) and [(n // 512, n % 512) for n in NR.VLENS] == [(0, 65), (1, 1), (2, 1)]
    assert NR.VLENS[0] == NR.AUTO_ORDERED_MAX + 1, "the smallest length NKA_HIP_SUMS_AUTO runs in the fast sums"
    assert NR.MVECS == (1, 2, 5, 10, 11, 20, 21, 32)
    assert {1, 64, 65, NR.PACK_VLEN} <= set(NR.PACK_LENS) and len(NR.PACK_LENS) == NR.NSYS and max(NR.PACK_LENS) == NR.PACK_VLEN


# ---- 2. the instance -----------------------------------------------------------------------------------------------------------------

def test_the_instance_holds_the_longest_list_of_its_mvec():
    """nka_host::batch_rows_nlmax as the layout program prints it: >= mvec + 1 for 1 ... 32, the smallest of 11 / 21 / 33 that is,
    with the edges at mvec 10 / 11 and 20 / 21; the grid of the GPU twin stands on both sides of each."""
    table = _layout_table()
    assert sorted(table) == list(range(1, 33))
    for mvec in range(1, 33):
        nl = table[mvec][4]
        assert nl >= mvec + 1 and nl in NR.NLMAX and nl == NR.nlmax_of(mvec), (mvec, nl)
    assert [table[m][4] for m in (1, 5, 10, 11, 20, 21, 32)] == [11, 11, 11, 21, 21, 33, 33]
    assert {NR.nlmax_of(m) for m in NR.MVECS} == set(NR.NLMAX) and {10, 11, 20, 21, 32} <= set(NR.MVECS)
    host = open(os.path.join(CSRC, "host_logic.hpp")).read()
    assert "constexpr int batch_rows_nlmax(int mvec) { return mvec + 1 <= 11 ? 11 : mvec + 1 <= 21 ? 21 : 33; }" in host


# ---- 3. the mirror -------------------------------------------------------------------------------------------------------------------

CREATE = (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_int32])
LIMITS = (C.c_int, [C.c_int32, C.POINTER(C.c_int64)])


def test_header_exports_signatures_and_refusals_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    decl = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert re.search(r"int nka_hip_batch_create_rows\(nka_hip_batch_t \*out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,\s*"
                     r"int32_t flavor, int32_t device, void \*stream, int32_t storage\);", decl)
    assert "int nka_hip_batch_rows_limits(int32_t mvec, int64_t *lds_bytes);" in decl
    L, D = nka_amd.load(), _lib.load_diag()
    for name, (res, args) in (("nka_hip_batch_create_rows", CREATE), ("nka_hip_batch_rows_limits", LIMITS)):
        assert hasattr(L, name) and hasattr(D, name), name
        assert _lib.BATCH_SIGNATURES[name][0] is res and list(_lib.BATCH_SIGNATURES[name][1]) == args, name
    # the limits: exported, mirrored, and the arithmetic of the layout (batch_rows.lds_bytes restates it)
    lds = C.c_int64()
    assert L.nka_hip_batch_rows_limits(20, C.byref(lds)) == 0 and lds.value == 9168 == nka_amd.batch_rows_limits(20)
    assert nka_amd.batch_rows_limits(32) == 20496 <= 40 * 1024 and L.nka_hip_batch_rows_limits(5, None) == 0
    for mvec in range(1, nka_amd.BATCH_MAX_MVEC + 1):
        assert nka_amd.batch_rows_limits(mvec) == NR.lds_bytes(mvec), mvec
    for bad in (0, -1, nka_amd.BATCH_MAX_MVEC + 1):
        assert L.nka_hip_batch_rows_limits(bad, C.byref(lds)) == EINVAL and b"nka_hip_batch_rows_limits" in L.nka_hip_last_error()
        with pytest.raises(nka_amd.NKAError):
            nka_amd.batch_rows_limits(bad)
    # refusals before any device is looked for: the new entry's name stands in every message, and no handle comes back
    h = C.c_void_p()
    assert L.nka_hip_batch_create_rows(None, 1, 1, 1, 0.01, 0, 0, None, 0) == EINVAL
    F64, F32 = nka_amd.STORE_F64, nka_amd.STORE_F32
    for nsys, vlen, mvec, vtol, flavor, storage, word in ((4, 129, 3, 0.01, 2, 2, b"storage"), (4, 129, 3, 0.01, 2, -1, b"storage"),
                                                          (0, 129, 3, 0.01, 2, F64, b"nsys"), (4, 0, 3, 0.01, 2, F64, b"vlen"),
                                                          (4, nka_amd.BATCH_MAX_VLEN + 1, 3, 0.01, 2, F32, b"vlen"), (4, 129, 0, 0.01, 2, F64, b"mvec"),
                                                          (4, 129, nka_amd.BATCH_MAX_MVEC + 1, 0.01, 2, F32, b"mvec"), (4, 129, 3, 0.0, 2, F64, b"vtol"),
                                                          (4, 129, 3, 0.01, 0, F32, b"binary32"), (4, 129, 3, 0.01, 1, F32, b"binary32")):
        h.value = 1
        assert L.nka_hip_batch_create_rows(C.byref(h), nsys, vlen, mvec, vtol, flavor, 0, None, storage) == EINVAL and h.value is None
        err = L.nka_hip_last_error()
        assert b"nka_hip_batch_create_rows" in err and word in err, (err, word)
    # the Python side: narrow_rows excludes the other kinds; rows=True alone keeps asking for waves=True
    for kw in ({"wide": True}, {"lanes": True}, {"waves": True}, {"waves": True, "rows": True}):
        with pytest.raises(nka_amd.NKAError, match="narrow_rows"):
            nka_amd.nka_batch().init(4, 64, 3, narrow_rows=True, **kw)
    with pytest.raises(nka_amd.NKAError, match="waves=True"):
        nka_amd.nka_batch().init(4, 129, 3, rows=True)
    doc = nka_amd.nka_batch.init.__doc__
    assert "nka_hip_batch_create_rows" in doc and "NARROW ROWS" in doc and "narrow_rows" in doc
    for name in ("set_scalar_step", "scalar_step", "offers_scalar_step"):
        assert "narrow_rows=True" in getattr(nka_amd.nka_batch, name).__doc__, name
    assert "NKA_HIP_ESTATE" in nka_amd.nka_batch.set_scalar_step.__doc__
    assert nka_amd.batch_rows_limits is nka_amd.batch.batch_rows_limits
    assert L.nka_hip_batch_offers_scalar_step(None) < 0 and L.nka_hip_last_error()


def test_the_header_carries_the_paragraph():
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    m = re.search(r"^ \*   NARROW ROWS  nka_hip_batch_create_rows: (.*?)^ \*   OUT OF SCOPE", hdr, flags=re.M | re.S)
    assert m, "the paragraph behind WAVES ROWS"
    par = " ".join(m.group(1).replace("\n *", " ").split())
    for phrase in ("nka_hip_batch_set_scalar_step", "NKA_HIP_BATCH_SCALAR_WAVEFRONT", "BOTH STEPS LEAVE THE SAME BITS", "nka_hip_batch_kind is 0",
                   "nka_hip_batch_rows_limits", "9 168", "20 496", "40 KiB", "NKA_HIP_ESTATE", "nka_hip_batch_set_sum_order",
                   "nka_hip_batch_create_waves_rows", "a captured call keeps the step it was captured with", "nothing further is allocated",
                   "FAST SUMS ONLY", "nothing is silently downgraded", "11 / 21 / 33", "profiles/r24/batch_rows_throughput.txt"):
        assert phrase in par, phrase
    assert hdr.index("*   WAVES ROWS  nka_hip_batch_create_waves_rows:") < m.start()
    step = hdr[hdr.index("*   SCALAR STEP  nka_hip_batch_set_scalar_step:"):hdr.index("*   WAVES ROWS  nka_hip_batch_create_waves_rows:")]
    assert "NARROW ROWS" in step and "Not covered: the narrow batch" not in step, "the narrow batch is no longer a follow-up"
    # no ratio is quoted without the record it comes from
    if not os.path.exists(os.path.join(ROOT, "profiles", "r24", "batch_rows_throughput.txt")):
        assert "MEASURED" not in par or not re.search(r"\d\.\d\d", par[par.index("MEASURED"):]), "a ratio without its record"


# ---- 4. the units --------------------------------------------------------------------------------------------------------------------

def _code(name):
    return "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, name)).read().splitlines())


def test_the_one_kernel_body_holds_the_wavefront_step():
    """k_batch_update stays the one kernel body of the narrow batch (nka_batch_kernel.hpp, compiled by nka_batch.hip and by
    nka_batch_rows.hip): the wavefront step is one more, empty, LAST member of the trailing pack, phase 4 branches on it at
    compile time, the one-thread statements are still written out, and nothing at device scope was added."""
    kern, unit, rows = _code("nka_batch_kernel.hpp"), _code("nka_batch.hip"), _code("nka_batch_rows.hip")
    assert len(re.findall(r"__global__[^;{]*\bk_batch_update\b", kern)) == 1 and kern.count("__global__") == 1
    assert "void k_batch_update" not in unit and "void k_batch_update" not in rows and "__global__" not in rows
    assert "template <int NLMAX> struct BatchRows {};" in kern and "constexpr int ROWS = batch_rows_nl<Step...>;" in kern
    assert "then at most one BatchRows<NLMAX>" in kern and 'static_assert(ROWS == 0 || !ORDERED' in kern
    phase4 = kern[kern.index("if constexpr (ROWS > 0) {"):kern.index("for (int i = t; i < nh; i += kBatchThreads) ctl.h()[i] = L.h[i];")]
    assert "if (t < 64) batch_scalar_step_rows<ROWS>(L, ctl, s, nolder, mvec, ps, red, cs, cc, hdr, " in phase4
    assert "nka_host::batch_rows_lds(mvec).a_off" in phase4 and "} else if (t == 0) {" in phase4
    for stmt in ("const int entry_first = L.first;", "lst_relax(L);", "lst_factor(L);", "lst_solve(L);", "lst_prepend(L, slot);",
                 "lst_store_scalars(L, ctl);", "ctl.ic[IC_NRELAX] = nrelax;"):      # the written-out one-thread step
        assert phase4.count(stmt) == 1, stmt
    assert phase4.rstrip().endswith("__syncthreads();") and phase4.count("__syncthreads();") == 1
    for word in ("atomic", "hipFuncSetAttribute", "s_barrier", "cooperative"):
        assert word not in kern and word not in rows, word
    assert "hipFuncSetAttribute" not in unit
    # the two device functions of nka_batch_dev.hpp are called, not restated
    dev = _code("nka_batch_dev.hpp")
    assert dev.count("void batch_scalar_step_rows(") == 1 and dev.count("void batch_scalar_step(") == 1 and "batch_scalar_step_rows(" not in rows
    # the launch: the instance and its LDS size are chosen together, when the call is enqueued; fast sums only
    assert "nka_host::batch_rows_lds(b->k.mvec).bytes()" in rows and "k_batch_update<COMB, false, WGT, Step..., BatchRows<NLMAX>>" in rows
    for nl in ("11", "21", "nka_host::kWideRowsMaxList"):
        assert f"launch_rows_nl<COMB, WGT, {nl}>" in rows, nl
    for call in ("nka_batch_rows_update(b, f_dev, ld, active_dev);", "nka_batch_rows_step(b, f_dev, ld, x_dev, ldx, active_dev, tol_dev, fnorm_dev);"):
        assert unit.count("else if (b->narrow_rows && b->scalar_step == NKA_HIP_BATCH_SCALAR_WAVEFRONT) " + call) == 1, call
    assert "nka_host::batch_lds(b->k.mvec).bytes()" in unit and "batch_rows_lds(NKA_HIP_BATCH_MAX_MVEC).bytes() <= 40 * 1024" in kern
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("nka_batch_rows.o") >= 2 and "nka_batch_rows.hip" in mk and "nka_batch_kernel.hpp" in mk and "rowscheck" in mk


# ---- 5. the LDS ----------------------------------------------------------------------------------------------------------------------

def _layout_table():
    subprocess.run(["make", "-s", "-C", CSRC, "rowscheck"], check=True)
    out = subprocess.run([os.path.join(CSRC, "build_host", "batch_rows_layout_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "batch_rows_layout_check: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return {int(r[1]): tuple(int(v) for v in r[2:]) for r in (ln.split() for ln in out.stdout.splitlines() if ln.startswith("rows "))}


def test_the_lds_of_the_wavefront_step_is_laid_out_without_overlap_and_is_the_librarys():
    """tests/c/batch_rows_layout_check.cpp paints every piece of batch_rows_lds(mvec) for mvec 1 ... 32: no overlap, doubles on 8
    bytes, the matrix on 16, the pieces of batch_lds where they were, at most 40 KiB.  Built with the sanitizers by
    `make rowscheck`, run as a program; nka_hip_batch_rows_limits returns what it prints."""
    import nka_amd
    table = _layout_table()
    assert sorted(table) == list(range(1, nka_amd.BATCH_MAX_MVEC + 1))
    for mvec, (copy, a_off, a_bytes, total, nl) in table.items():
        assert a_off % 16 == 0 and copy <= a_off < copy + 16 and a_bytes == 8 * (mvec + 2) ** 2 and total == a_off + a_bytes, mvec
        assert total == nka_amd.batch_rows_limits(mvec) == NR.lds_bytes(mvec) <= 40 * 1024, mvec
    assert (table[20][3], table[32][3]) == (9168, 20496)
