"""The wave batch with lengths and weights (nka_hip_batch_create_waves_ext) as far as a machine without a GPU can see it: the host
model of the WEIGHTED wave sum against exact sums and against every ignored, misplaced, lost or doubled sentinel; the lengths and
the large shape of the GPU tests; the budget of the ragged weighted solve on the oracle; prototypes, exports, refusals and text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_step as S
import batch_waves as BWV
import batch_waves_ext as E
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nka_amd", "csrc")
CREATE = (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p])
PROTOTYPES = {"nka_hip_batch_create_waves_ext": CREATE, "nka_hip_batch_offers_lengths": (C.c_int, [C.c_void_p]),
              "nka_hip_batch_offers_weights": (C.c_int, [C.c_void_p])}


# ---- the weighted sum -------------------------------------------------------------------------------------------------------------

def _inside(got, a, y, n):
    return abs(got - X.exact_dot(a, y)) <= X.gamma(BWV.waves_k(n)) * X.abs_dot(a, y)


@pytest.mark.parametrize("n", E.CPU_LENGTHS)
def test_the_model_of_the_weighted_wave_sum_is_inside_the_bound_and_every_mutation_outside(n):
    """batch_waves.model_sum on fl(w o x) and y -- the lane's strided fma chain with the rounded first operand, then the butterfly
    -- is inside gamma(waves_k(n)) sum|fl(w x) y| of the exact sum of fl(w x) and y.  At every sentinel, a sum that ignores the
    weight, takes the pair partner's weight, loses the element or adds it twice is outside: the GPU layer cannot hide such an
    error inside its bound."""
    rng = np.random.default_rng([n, 2])
    x = BWV.planted_input(n, rng)
    y = BWV.planted_input(n, rng, prev=x)
    w = E.draw_weights(n, rng)
    a = w * x                                                # fl(w x): rounded once, before the product
    assert _inside(BWV.model_sum(a, y), a, y, n), n
    sent = [int(i) for i in BWV.all_sentinels(n)]
    assert {0, 1, 126, 127, n - 1} <= set(sent)
    for i in sent:
        pw = w[i ^ 1] if (i ^ 1) < n else 0.0                # (beyond n: the zero ld_pair returns)
        for name, terms in (("weight ignored", [(x[i], y[i])]), ("partner's weight", [(pw * x[i], y[i])]), ("lost", []),
                            ("doubled", [(a[i], y[i])] * 2)):
            got = BWV.model_sum(a, y, take=lambda j, i=i, terms=terms: terms if j == i else [(a[j], y[j])])
            assert not _inside(got, a, y, n), (n, i, name)


def test_the_one_wave_unit_holds_the_weighted_and_the_ragged_kernel():
    """nka_batch_waves.hip is the only wave unit and k_waves_update the only wave kernel: one sweep, one wave_sync, one fma per
    element and accumulator (each weighted product beside its unweighted form), the butterfly of wave_sum, no workgroup barrier,
    no atomics; the weight pair is loaded like a stored vector and phase 6 does not read it; every sys * stride product is in 64
    bits."""
    assert not os.path.exists(os.path.join(CSRC, "nka_batch_waves_ext.hip"))
    assert "nka_batch_waves_ext" not in open(os.path.join(CSRC, "Makefile")).read()
    unit = open(os.path.join(CSRC, "nka_batch_waves.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in unit.splitlines())
    assert code.count("void waves_sweep(") == 1 and code.count("void wave_sync()") == 1 and code.count("__global__") == 1
    kern = code[code.index("void k_waves_update"):code.index("void launch_waves_as")]
    fmas = re.findall(r"(acc(?:\[[^\]]+\])?) = fma\(([^;]+), \1\);", kern)
    first = sorted(f[1].split(",")[0].strip() for f in fmas)
    # phase 2: <d,d> and <f,f> (twice: with and without a pending pair), each weighted and plain; phase 3: the three sums, whose
    # first operands fa = fl(w f) and wa = fl(w w1') are formed once per element
    assert first == sorted(["gv[q] * d", "d", "gv[q] * fv[q]", "fv[q]", "gv[q] * fv[q]", "fv[q]", "fa", "wa", "fa"]), first
    assert kern.count("if constexpr (WGT) fa = gv[q] * fq;") == 1 and kern.count("if constexpr (WGT) wa = gv[q] * wn;") == 1
    assert len(re.findall(r"acc(?:\[[^\]]+\])?\s*(?:\+=|= acc)", kern)) == 0
    for word in ("__syncthreads", "atomic", "s_barrier", "__shared__ double", "batch_block_sum"):
        assert word not in code.replace('"wavefront"', ""), word
    assert code.count("wave_sync();") >= 3 and "wave_sum(" in kern
    phase6 = kern[kern.index("const int ncomb = hdr[HDR_NCOMB];"):]
    assert "gv" not in phase6 and "wg" not in phase6
    assert kern.count("gv = ld_tile<FULL, true>(wg, i, n);") == 3      # phase 2 (twice: with and without a pending pair) and phase 3
    for prod in ("(size_t)sys * (size_t)ld", "(size_t)sys * (size_t)a.sys_stride", "(size_t)sys * (size_t)pack_get<WgtStride>(pack...)",
                 "(size_t)sys * (size_t)st.ldx"):
        assert prod in kern, prod
    assert "pack_get<LenArgs>(pack...).len[sys]" in kern[kern.index("active[sys] == 0"):]      # one load behind the `active` test


# ---- lengths and shapes -------------------------------------------------------------------------------------------------------------

def test_the_lengths_and_the_large_shape_of_the_gpu_tests():
    import nka_amd
    group, cap = nka_amd.batch_waves_limits()
    assert E.VLEN == 385 == 3 * 128 + 1 and E.LENS == (1, 2, 3, 127, 128, 129, 255, 257, 385) and max(E.LENS) == E.VLEN <= cap
    assert E.NSYS == 9 and E.NSYS % group != 0, "the last workgroup has absent wavefronts"
    cases = E.tile_cases()
    assert all(cases.values()), cases                        # an empty, a partial and a full last tile; the half pair of an odd length
    assert 128 in cases["no ragged tile"] and {127, 129, 385} <= set(cases["ragged tile"]) and {1, 3, 385} <= set(cases["half pair"])
    assert max(E.UNIT_LENGTHS + E.EXACT_LENGTHS) <= cap and 899 == 7 * 128 + 3
    # the plan: staggered starts, a repeat, a masked relax and a masked restart, a step without and with thresholds
    kinds = [k for k, _ in E.PLAN]
    assert 8 <= E.CALLS <= 10 and {"update", "repeat", "step", "step-tol"} == set(kinds)
    assert {op[0] for _, op in E.PLAN if op} == {"relax", "restart"} and {E.delay(k) for k in range(E.NSYS)} == {0, 1, 2}
    assert len(E.RETIRE) == 2 and kinds.index("step-tol") > kinds.index("repeat") > max(E.delay(k) for k in range(E.NSYS))
    assert kinds.index("step-tol") < E.CALLS - 1, "calls follow the retirement"
    # the large case
    sh = E.large_shape()
    row, nsys, kb, ks = sh["row_bytes"], sh["nsys"], sh["boundary"], sh["slot_boundary"]
    assert sh["vlen"] == 1024 <= cap and sh["mvec"] == 1 and row == 8 * BWV.slot_stride(1024) == 8192
    assert nsys > 524288 and nsys - 524288 <= 4
    assert row * nsys > 2 ** 32 and kb * row == 2 ** 32                            # F, X, the caller's weights, the weight buffer
    assert ks * row * 2 == 2 ** 32 and 2 * row * nsys > 2 ** 32                    # each slot allocation
    assert 5 <= len(sh["active"]) <= E.MAX_ACTIVE and {0, ks - 1, ks, kb - 1, kb, nsys - 1} <= set(sh["active"])
    assert sorted(sh["lens"]) == sh["active"] and all(1 <= L <= 1024 for L in sh["lens"].values())
    assert {1, 1024} <= set(sh["lens"].values()) and any(L % 2 and L > 128 for L in sh["lens"].values())
    assert sh["witnesses"] and not set(sh["witnesses"]) & set(sh["active"])
    assert {1, ks - 2, ks + 1, kb - 2} <= set(sh["witnesses"])      # beside system 0, where a lost upper half lands, and the neighbours
    total = sum(E.large_bytes(sh).values())
    assert 2 ** 32 * 7 < total <= 36 * 2 ** 30, total


def test_the_replay_budget_of_the_ragged_weighted_solve_holds_on_the_oracle(oracle):
    """The solve the GPU test replays, with np.dot sums on the oracle: every system retires SOLVE_SLACK steps inside SOLVE_REPLAYS,
    at three or more different iterations, none at the first call; the lengths are ragged and inside this kind's range."""
    lens, w = E.solve_lengths(), E.solve_weights()
    assert lens.min() == S.SOLVE_VLEN // 4 and lens.max() == S.SOLVE_VLEN and len(set(lens.tolist())) > 8 and {64, 65} <= set(lens.tolist())
    assert all((w[k, :L] > 0).all() and (w[k, L:] == E.TAIL_WEIGHT).all() for k, L in enumerate(lens))
    left, right = E.solve_couplings()
    for k, L in enumerate(lens):                             # nothing below L reaches across L, or around the row
        assert left[k, 0] == 0 and right[k, L - 1] == 0 and left[k, 1:L].all() and right[k, :L - 1].all() and not left[k, L:].any()
    retired = E.solve_on_the_oracle(oracle)
    assert (retired >= 1).all() and retired.max() <= E.SOLVE_REPLAYS - E.SOLVE_SLACK and len(set(retired.tolist())) >= 3, retired


# ---- prototypes, exports, text ------------------------------------------------------------------------------------------------------

def test_prototypes_exports_and_refusals_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    decl = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    L, D = nka_amd.load(), _lib.load_diag()
    for name, (res, args) in PROTOTYPES.items():
        assert _lib.BATCH_SIGNATURES[name][0] is res and list(_lib.BATCH_SIGNATURES[name][1]) == args, name
        assert hasattr(L, name) and hasattr(D, name) and re.search(r"\bint " + name + r"\(", decl), name
    assert re.search(r"int nka_hip_batch_create_waves_ext\(nka_hip_batch_t \*out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,\s*"
                     r"int32_t flavor, int32_t device, void \*stream\);", decl)
    assert "int nka_hip_batch_offers_lengths(nka_hip_batch_t b);" in decl and "int nka_hip_batch_offers_weights(nka_hip_batch_t b);" in decl
    assert L.nka_hip_batch_offers_lengths(None) < 0 and L.nka_hip_last_error()
    assert L.nka_hip_batch_offers_weights(None) < 0 and L.nka_hip_last_error()
    assert L.nka_hip_batch_create_waves_ext(None, 1, 1, 1, 0.01, 0, 0, None) == -1
    h = C.c_void_p()
    _, cap = nka_amd.batch_waves_limits()
    for nsys, vlen, mvec, vtol in ((0, 129, 3, 0.01), (4, cap + 1, 3, 0.01), (4, 0, 3, 0.01), (4, 129, 33, 0.01), (4, 129, 0, 0.01),
                                   (4, 129, 3, 0.0)):       # the wave batch's limits, refused before any device is looked for
        assert L.nka_hip_batch_create_waves_ext(C.byref(h), nsys, vlen, mvec, vtol, 0, 0, None) == -1 and h.value is None
        assert b"nka_hip_batch_create_waves_ext" in L.nka_hip_last_error()
    with pytest.raises(nka_amd.NKAError, match="waves=True"):
        nka_amd.nka_batch().init(4, 64, 3, ext=True)
    for kw in ({"wide": True}, {"lanes": True}, {"storage": nka_amd.STORE_F32}):
        with pytest.raises(nka_amd.NKAError):
            nka_amd.nka_batch().init(4, 64, 3, waves=True, ext=True, **kw)


def test_the_header_carries_the_paragraph():
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    m = re.search(r"^ \*   WAVES EXT  nka_hip_batch_create_waves_ext: (.*?)^ \*   OUT OF SCOPE", hdr, flags=re.M | re.S)
    assert m, "the paragraph next to WAVES"
    par = " ".join(m.group(1).replace("\n *", " ").split())
    for phrase in ("LENGTHS:", "WEIGHTS:", "NEITHER SET:", "BIT-EQUAL", "nothing at or beyond L is read or written", "FIRST operand",
                   "nka_hip_batch_offers_lengths", "fl(w f) is formed once per element and sweep", "nka_hip_batch_kind stays 3"):
        assert phrase in par, phrase
    assert hdr.index("*   WAVES    nka_hip_batch_create_waves:") < m.start()
    # no ratio is quoted without the record it comes from
    if not os.path.exists(os.path.join(ROOT, "profiles", "r17", "batch_waves_ext_throughput.txt")):
        assert not re.search(r"\d\.\d\d", par[par.index("WHICH KIND"):]), "a ratio without its record"


def test_the_integration_example_still_compiles_and_names_the_new_entry(tmp_path):
    """The wave block of INTEGRATION.md is still the only ```C block that names nka_hip_batch_create_waves; it now names the new
    entry and the two setters too; syntax only, as its sibling test does."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_waves" in b]
    assert len(blocks) == 1
    for name in ("nka_hip_batch_create_waves_ext", "nka_hip_batch_set_lengths", "nka_hip_batch_set_dot_weights", "nka_hip_batch_offers_lengths",
                 "nka_hip_batch_waves_limits", "NKA_HIP_BATCH_KIND_WAVES"):
        assert name in blocks[0], name
    assert re.search(r"nka_hip_batch_create_waves\(", blocks[0]), "the old entry's example stays"
    src = tmp_path / "wave_batch_ext.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
