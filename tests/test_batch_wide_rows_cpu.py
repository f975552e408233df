"""The wide batch's scalar step on one wavefront (nka_hip_batch_set_scalar_step), the parts that need no GPU.

  1 the claim      a numpy model of batch_scalar_step_rows (batch_wide_rows.model_step: right-looking factorisation with drops, the
                   right-hand side riding along, column-oriented back-substitution, one rounding per operation in the device
                   function's order) against the oracle's scalar_step (left-looking, the reference's loops) at list lengths 1 ... 33:
                   lists, decisions and ALL of h with ==, c with == on the kept entries and == the raw right-hand side on the
                   dropped ones.  Four wrong models must fail.
  2 the census     the sequences of the GPU twin test reach every branch of the drop logic when the oracle alone runs them
  3 the mirror     constants, symbols, signatures
  4 the LDS        tests/c/batch_wide_rows_layout_check.cpp, a stand-alone program under AddressSanitizer and UBSan
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_wide_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTOL = 0.01


def _bits(a, b):
    """== on doubles, bit for bit; a NaN only as NaN (the oracle runs on the host, whose NaN need not be the model's)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def _same_lists(L, st):
    return ((L.first, L.last, L.free, bool(L.subspace), bool(L.pending)) == (st.first, st.last, st.free, st.subspace, st.pending)
            and np.array_equal(L.next[1:], st.next) and np.array_equal(L.prev[1:], st.prev))


def _agrees(L, st, order0, b):
    """The model's working copy against the oracle's state after the same step."""
    if not (_same_lists(L, st) and _bits(L.h[1:, 1:], st.h)):
        return False
    kept = st.list_order()[1:]
    if not _bits(L.c[kept], st.c[[k - 1 for k in kept]]):
        return False
    gone = [k for k in order0[1:] if k not in kept]      # (with a new pair: the raw right-hand side stays in a dropped entry)
    return _bits(L.c[gone], b[gone])


def _gram_case(rng, ora, W, mvec, kind, nclose=2):
    """s, hrow, b of one step on the oracle's present list.  W: slot -> the unit vector the slot holds (a host mirror); nclose: the
    close calls so far -- the first two lie 1e-9 vtol^2 either side of the threshold, where the rounding of 1 - h^2 cannot move
    them across, the later ones within a few ulp of it."""
    st = ora.state()
    order = st.list_order()
    dim = W.shape[1]
    hrow, b = np.zeros(mvec + 2), np.zeros(mvec + 2)
    s = 0.0 if kind == "zero" else 1.0 + rng.random()
    if st.pending:
        older = order[1:]
        if kind == "dependent" and older:      # a combination of older vectors and a little of a new direction
            w = W[older].T @ rng.standard_normal(len(older)) + rng.choice([1e-1, 1e-3, 1e-5, 0.0]) * rng.standard_normal(dim)
        else:
            w = rng.standard_normal(dim)
        w = w / np.linalg.norm(w)
        W[order[0]] = w
        for k in older:
            hrow[k] = W[k] @ w
        if kind == "close" and older:          # the pivot of the first older entry within a few ulp of vtol^2, either side
            delta = rng.choice([0.0, 1e-16, -1e-16, 2e-16, -2e-16, 1e-15, -1e-15, 1e-12, -1e-12]) if nclose >= 2 else (1e-9, -1e-9)[nclose]
            hrow[older[0]] = np.sqrt(1.0 - VTOL * VTOL * (1.0 + delta))
        if kind == "nan" and older:
            hrow[older[rng.integers(len(older))]] = np.nan
    for k in order:
        b[k] = rng.standard_normal()
    return st, order, s, hrow, b


KINDS = ("random", "random", "dependent", "dependent", "close", "random", "dependent", "zero", "random", "nan")


@pytest.mark.parametrize("mvec", range(1, 33))
def test_the_rows_model_is_the_oracles_scalar_step(oracle, mvec):
    """List lengths 1 ... mvec + 1 at every mvec 1 ... 32, so 1 ... 33: the oracle is driven through scalar_step, relax and restart
    alone, on Gram rows of random vectors, of vectors nearly in the span of the list (dependence drops anywhere in it), with the
    first older pivot a few ulp either side of vtol^2, with s == 0 and with a NaN.  At the mvec of the GPU grid every wrong model
    of batch_wide_rows.MUTATIONS must disagree with the oracle at least once."""
    rng = np.random.default_rng(7000 + mvec)
    ora = oracle.OracleNKA(8, mvec, oracle.C_FLAVOR)
    ora.set_vec_tol(VTOL)
    W = np.zeros((mvec + 2, 40))
    mutants = R.MUTATIONS if mvec in R.MVECS and mvec >= 2 else ()
    failed = {m: 0 for m in mutants}
    lengths, drops, caps, flips, nclose = set(), 0, 0, set(), 0
    steps = 2 * mvec + 44
    for t in range(steps):
        kind = KINDS[t % len(KINDS)] if t > mvec + 2 else "random"
        if t == mvec + 9:
            ora.relax()
        if t == mvec + 15:
            ora.restart()
        st0, order0, s, hrow, b = _gram_case(rng, ora, W, mvec, kind, nclose)
        works = {m: R.Work(st0, mvec, VTOL) for m in (None,) + tuple(mutants)}
        new = ora.scalar_step(s, hrow, b)
        st1 = ora.state()
        slot, dep, cap = R.model_step(works[None], s, hrow, b)
        where = (mvec, t, kind, order0)
        assert slot == new and _agrees(works[None], st1, order0 if (st0.pending and s != 0.0) else [], b), where
        for m in mutants:
            R.model_step(works[m], s, hrow, b, mutate=m)
            failed[m] += not _agrees(works[m], st1, order0 if (st0.pending and s != 0.0) else [], b)
        lengths.add(len(order0))
        drops += len(dep)
        caps += cap is not None
        if kind == "close" and st0.pending and len(order0) > 1:
            flips.add(1 in dep)
            nclose += 1
    assert lengths >= set(range(0, mvec + 2)), (mvec, sorted(lengths))
    assert caps >= 1 and (drops >= 2 or mvec == 1), (mvec, caps, drops)
    if mvec >= 2:
        assert flips == {False, True}, (mvec, "the close calls fell on one side only", flips)
    for m in mutants:
        if m == "ascending_back_substitution" and mvec == 2:
            continue      # (at most two entries are kept and the first pivot is 1.0: both orders form the same two values)
        assert failed[m] >= 1, (mvec, m, "a wrong model passed")


@pytest.mark.parametrize("mvec,flavor", [(m, 2) for m in R.MVECS] + [(10, 0), (10, 1), (20, 0), (20, 1)])
def test_the_sequences_meet_the_census_on_the_reference(oracle, mvec, flavor):
    """batch_wide_rows.script, at the seeds of the GPU twin test's grid, through eight oracles: per mvec >= 2 at least one update with two dependence drops, one with a drop
    at the first older position, one at the last, a capacity drop, a last position evaluated behind a drop, a relax by s == 0
    and a solve without a new pair.  A short census on the GPU is then the kernel's or the twin's doing, not the inputs'."""
    vlen = 65
    oras = [oracle.OracleNKA(vlen, mvec, flavor) for _ in range(R.NSYS)]
    census, older_counts = {}, set()
    for t, ev in enumerate(R.script([vlen] * R.NSYS, mvec, R.twin_seed(mvec, flavor))):
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
        if len(ev["inputs"]) == R.NSYS:
            older_counts.add(len(counts))
    assert max(older_counts) >= 2 or mvec == 1      # one launch holds lists of different length
    if mvec >= 2:
        assert not R.census_short(census), (mvec, census)
    print(f"census on the reference, mvec {mvec}, flavour {flavor}: {sorted(census.items())}")


def test_the_python_mirror_of_the_scalar_step():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    m = re.search(r"enum \{ NKA_HIP_BATCH_SCALAR_ONE_THREAD = (\d+), NKA_HIP_BATCH_SCALAR_WAVEFRONT = (\d+) \};", hdr)
    assert m and (int(m.group(1)), int(m.group(2))) == (nka_amd.SCALAR_ONE_THREAD, nka_amd.SCALAR_WAVEFRONT) == (0, 1)
    assert "SCALAR STEP" in hdr
    for decl in ("int nka_hip_batch_set_scalar_step(nka_hip_batch_t b, int32_t how);", "int nka_hip_batch_scalar_step(nka_hip_batch_t b);",
                 "int nka_hip_batch_offers_scalar_step(nka_hip_batch_t b);"):
        assert decl in hdr, decl
    lib = C.CDLL(nka_amd.lib_path())
    want = {"nka_hip_batch_set_scalar_step": (C.c_int, [C.c_void_p, C.c_int32]), "nka_hip_batch_scalar_step": (C.c_int, [C.c_void_p]),
            "nka_hip_batch_offers_scalar_step": (C.c_int, [C.c_void_p])}
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert _lib.BATCH_SIGNATURES[name][0] is res and list(_lib.BATCH_SIGNATURES[name][1]) == args, name
    for name in ("set_scalar_step", "scalar_step", "offers_scalar_step"):
        assert callable(getattr(nka_amd.nka_batch, name)), name
    # a NULL handle is an error of every entry, reported and not a crash
    L = _lib.load()
    assert L.nka_hip_batch_set_scalar_step(None, 0) < 0 and L.nka_hip_batch_scalar_step(None) < 0
    assert L.nka_hip_batch_offers_scalar_step(None) < 0 and L.nka_hip_last_error()


def test_the_lds_of_the_wavefront_step_is_laid_out_without_overlap():
    """tests/c/batch_wide_rows_layout_check.cpp paints every piece of wide_scalar_rows_lds(mvec, nchunk) for mvec 1 ... 32 and
    nchunk 1, 2, 257, 512 (and the cap, 1024): no overlap, the double pieces on 8 bytes, at most 64 KiB.  Built with the
    sanitizers by `make widerowscheck`, run as a program."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "widerowscheck"], check=True)
    out = subprocess.run([os.path.join(csrc, "build_host", "batch_wide_rows_layout_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batch_wide_rows_layout_check: OK" in out.stdout, out.stdout
