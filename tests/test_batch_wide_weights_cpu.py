"""The wide batch with diagonal dot weights (nka_hip_batch_create_wide_ext) as far as a machine without a GPU can see it: the host
model of the WEIGHTED chunked sum against exact sums and against every ignored or misplaced weight and every lost or doubled
partial; the shapes of the GPU tests; the budget of the ragged weighted solve on the oracle; the address arithmetic under
sanitizers; prototypes, exports, refusals and text."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_wide as BW
import batch_wide_weights as WW
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nka_amd", "csrc")
CREATE_EXT = (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_int32])


# ---- the weighted chunked sum -------------------------------------------------------------------------------------------------------

def _pairs(n, c, rng):
    """The operands of the four sums an update forms, from wide_planted_input (tests/test_batch_wide_cpu.py: _pairs)."""
    f_a = BW.wide_planted_input(n, rng, C=c)
    f_b = BW.wide_planted_input(n, rng, prev=f_a, C=c)
    f_c = BW.wide_planted_input(n, rng, prev=f_b, C=c)
    f = BW.wide_planted_input(n, rng, prev=f_c, C=c)
    d_old = f_a - f_b
    w_old = d_old / math.sqrt(float(np.dot(d_old, d_old)))
    d = f_c - f
    w1n = d / math.sqrt(float(np.dot(d, d)))
    return {"<d,d>": (d, d), "<f,w1'>": (f, w1n), "<w1',w_p>": (w1n, w_old), "<f,w_p>": (f, w_old), "<f,f>": (f, f)}


@pytest.mark.parametrize("which", sorted(WW.CPU_CHUNKS))
def test_the_model_of_the_weighted_wide_sum_is_inside_the_bound_and_every_mutation_outside(which):
    """9, 10 and 17 chunks of the library's C; the five operand pairs of an update and a step from planted inputs, weights by the
    rule.  batch_wide.model_partials on fl(w o x) and y -- the first operand rounded once, before the product -- and the chunk-order
    chain are inside gamma(wide_k(n)) sum|fl(w x) y| of the exact sum of fl(w x) and y, and the condition the GPU tests put on
    their operands (undetectable_chunks == []) holds.  Outside the bound, so that the GPU layer cannot hide it: at EVERY sentinel a
    sum that ignores the weight or takes the pair partner's; for EVERY chunk a sum that loses its partial or adds it twice."""
    c, _ = BW.limits()
    n = WW.shape(which, c)
    chunks = BW.nchunk(n, c)
    assert chunks == WW.CPU_CHUNKS[which] and chunks in (9, 10, 17)
    k = BW.wide_k(n, c)
    bound = X.gamma(k)
    rng = np.random.default_rng([15, c, n])
    w = WW.draw_weights(n, rng, c)
    WW.assert_weight_rule(n, w, c)
    sent = [int(i) for i in BW.wide_sentinel_indices(n, c)]
    assert {0, c - 1, c, n - 1} <= set(sent)
    whole = list(range(chunks))
    for what, (x, y) in _pairs(n, c, rng).items():
        a = w * x                                            # fl(w x)
        ex, tot = X.exact_dot(a, y), X.abs_dot(a, y)
        parts = BW.model_partials(a, y, c)
        assert parts.size == chunks
        assert abs(BW.model_sum_of(parts, whole) - ex) <= bound * tot, (which, what)
        assert BW.undetectable_chunks(a, y, k, c) == [], (which, what)
        for j in whole:
            lost, twice = whole[:j] + whole[j + 1:], whole[:j + 1] + whole[j:]
            assert abs(BW.model_sum_of(parts, lost) - ex) > bound * tot, (which, what, "lost", j)
            assert abs(BW.model_sum_of(parts, twice) - ex) > bound * tot, (which, what, "twice", j)
        for i in sent:
            q, lo = i // c, (i // c) * c
            pw = w[i ^ 1] if (i ^ 1) < n else 0.0            # (beyond n: the zero ld_pair returns)
            for name, first in (("weight ignored", x[i]), ("partner's weight", pw * x[i])):
                am = a[lo:lo + c].copy()
                am[i - lo] = first
                mutated = parts.copy()
                mutated[q] = BW._workgroup_sum(am * y[lo:lo + c])
                assert abs(BW.model_sum_of(mutated, whole) - ex) > bound * tot, (which, what, name, i)


def test_the_shapes_of_the_gpu_tests_and_the_large_shape():
    c, cap = BW.limits()
    assert [BW.nchunk(WW.shape(s, c), c) for s in WW.EXACT_SHAPES] == [2, 3, 9, 10, 17] and BW.nchunk(WW.shape("256C+1", c), c) == 257
    assert all(BW.nchunk(WW.shape(s, c), c) == 1 for s in ("1", "2", "65", "513", "C-1", "C"))
    sh = WW.large_shape(c, cap)
    nsys, vlen, stride, ld, kb = sh["nsys"], sh["vlen"], sh["stride"], sh["ld"], sh["boundary"]
    assert vlen <= cap and stride == WW.slot_stride(vlen) and stride % 32 == 0 and ld > vlen and sh["mvec"] == 1
    for step in (stride, ld):                                # the weight buffer; the caller's weight rows and F
        assert 8 * kb * step < WW.BYTES_4G < 8 * (kb * step + vlen), "byte 2^32 falls inside row kb"
        assert 8 * ((nsys - 1) * step + vlen) > WW.BYTES_4G
    assert kb in sh["active"] and {0, kb - 1, kb + 1, nsys - 1} <= set(sh["active"]) and len(sh["active"]) <= WW.MAX_ACTIVE
    assert sh["witnesses"] and not set(sh["witnesses"]) & set(sh["active"])
    assert {1, kb - 2, kb + 2} <= set(sh["witnesses"])
    for k in sh["active"]:                                   # where a byte offset that lost its upper half would land
        for step in (stride, ld, 2 * stride):
            assert (8 * k * step) % WW.BYTES_4G // (8 * step) in set(sh["active"]) | set(sh["witnesses"]), (k, step)
    assert any((8 * k * stride) % WW.BYTES_4G // (8 * stride) in sh["witnesses"] for k in sh["active"])
    assert sorted(sh["lens"]) == sh["active"] and all(1 <= L <= vlen for L in sh["lens"].values())
    assert sh["lens"][kb] == vlen, "the row on the boundary runs its whole length in both passes"
    total = sum(WW.large_bytes(sh).values())
    assert 2 ** 32 * 5 < total <= WW.MAX_BYTES, total


def test_the_replay_budget_of_the_ragged_weighted_wide_solve_holds_on_the_oracle(oracle):
    """The solve the GPU test replays, with np.dot sums on the oracle: every system retires SOLVE_SLACK steps inside SOLVE_REPLAYS,
    at three or more different iterations, none at the first call; 16 systems, lengths in [C / 2, 3C], zero weights on every 17th
    entry and powers of four elsewhere."""
    c, _ = BW.limits()
    lens, w = WW.solve_lengths(c), WW.solve_weights(c)
    assert WW.SOLVE_NSYS == 16 == lens.size and lens.min() == c // 2 and lens.max() == 3 * c == WW.solve_vlen(c) and len(set(lens.tolist())) > 8
    for k, L in enumerate(lens):
        head = w[k, :L]
        assert (head[k % 17::17] == 0).all() and (w[k, L:] == WW.TAIL_WEIGHT).all()
        rest = np.delete(head, np.arange(k % 17, L, 17))
        assert (rest > 0).all() and (np.log2(rest) % 2 == 0).all(), "4^k elsewhere"
    left, right = WW.solve_problem(c)[4:]
    for k, L in enumerate(lens):                             # nothing below L reaches across L, or around the row
        assert left[k, 0] == 0 and right[k, L - 1] == 0 and left[k, 1:L].all() and right[k, :L - 1].all() and not left[k, L:].any()
    retired = WW.solve_on_the_oracle(oracle, c)
    assert (retired >= 1).all() and retired.max() <= WW.SOLVE_REPLAYS - WW.SOLVE_SLACK and len(set(retired.tolist())) >= 3, retired


# ---- the address arithmetic ---------------------------------------------------------------------------------------------------------

def test_weight_addresses_of_a_wide_batch_against_a_brute_force_model_under_sanitizers():
    """tests/c/batch_wide_weights_check.cpp (its own main, -fsanitize=address,undefined): for every chunk of the lengths 1 ... 3C + 33
    and both forms, the weight elements a workgroup reads lie inside the system's row and below its length, chunk starts are 16-byte
    aligned, and the offsets equal their __int128 values at the largest legal nsys x stride."""
    subprocess.run(["make", "-s", "-C", CSRC, "wideweightscheck"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build_host", "batch_wide_weights_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    assert "wideweightscheck" in re.search(r"^hostcheck:(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1)


def test_the_weighted_kernels_read_the_weights_like_a_stored_vector_and_launch_the_existing_scalar_and_combine():
    """Both wide units: the weighted norm and sums kernels are templates on LEN written once, the weight pointer is __restrict__ on
    the kernel argument itself and follows the existing arguments with its row stride, the weight pair is loaded with
    ld_tile<FULL, true> from wide_wgt_offset, fl(w f) and fl(w w1') are formed once per element and sweep and stand FIRST in every
    product, and a weighted call launches the existing scalar and combine kernels.  No atomics, no cooperative launch."""
    for unit, norm, sums, tail in (("nka_batch_wide.hip", "k_wide_norm_wgt", "k_wide_sums_wgt", ("k_wide_scalar", "k_wide_combine")),
                                   ("nka_batch_wide_step.hip", "k_wide_step_norm_wgt", "k_wide_step_sums_wgt",
                                    ("k_wide_step_scalar", "k_wide_step_combine"))):
        text = open(os.path.join(CSRC, unit)).read()
        code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
        for word in ("atomic", "hipLaunchCooperativeKernel", "__threadfence"):
            assert word not in code, (unit, word)
        assert code.count(f"void {norm}(") == 1 and code.count(f"void {sums}(") == 1, unit
        kn = code[code.index(f"void {norm}("):code.index(f"void {sums}(")]
        ks = code[code.index(f"void {sums}("):code.index("void launch_wide")]
        for kern in (kn, ks):
            head = kern[:kern.index("{")]
            assert re.search(r"const double \*__restrict__ wgt, int64_t wgt_stride\)\s*$", head), (unit, head)
            assert kern.count("wgt + (size_t)nka_host::wide_wgt_offset(sys, wgt_stride, blockIdx.x)") == 1, unit
            assert "if constexpr (LEN)" in kern and "active[sys] == 0) return;" in kern
            assert kern.index("active[sys] == 0) return;") < kern.index("wide_wgt_offset"), "a masked system returns before it reads anything"
            assert len(re.findall(r"acc(?:\[[^\]]+\])?\s*(?:\+=|= acc)", kern)) == 0
        first = sorted(f.split(",")[0].strip() for f in re.findall(r"acc\[[^\]]+\] = fma\(([^;]+), acc\[[^\]]+\]\);", kn))
        assert first == (["gv[q] * d"] if "step" not in unit else sorted(["gv[q] * d", "gv[q] * fv[q]", "gv[q] * fv[q]"])), (unit, first)
        assert kn.count("gv = ld_tile<FULL, true>(wg, i, n);") == (1 if "step" not in unit else 2)
        first = sorted(f.split(",")[0].strip() for f in re.findall(r"acc\[[^\]]+\] = fma\(([^;]+), acc\[[^\]]+\]\);", ks))
        assert first == ["fa", "fa", "wa_"], (unit, first)
        assert ks.count("const double fa = gv[q] * fq;") == 1 and ks.count("const double wa_ = gv[q] * wn;") == 1
        assert ks.count("gv = ld_tile<FULL, true>(wg, i, n);") == 1
        launch = code[code.index("void launch_wide"):]
        weighted = launch[launch.index("if (b->weighted)"):]
        for name in tail:
            assert name in weighted, (unit, name)
        assert code.count("__global__") == (6 if "step" in unit else 10), unit


# ---- prototypes, exports, refusals, text --------------------------------------------------------------------------------------------

def test_prototype_exports_and_refusals_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    decl = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    L, D = nka_amd.load(), _lib.load_diag()
    name = "nka_hip_batch_create_wide_ext"
    assert _lib.BATCH_SIGNATURES[name][0] is CREATE_EXT[0] and list(_lib.BATCH_SIGNATURES[name][1]) == CREATE_EXT[1]
    assert hasattr(L, name) and hasattr(D, name)
    assert re.search(r"int nka_hip_batch_create_wide_ext\(nka_hip_batch_t \*out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,\s*"
                     r"int32_t flavor, int32_t device, void \*stream, int32_t step\);", decl)
    assert L.nka_hip_batch_create_wide_ext(None, 1, 1, 1, 0.01, 0, 0, None, 0) == -1
    h = C.c_void_p()
    chunk, cap = nka_amd.batch_wide_limits()
    for step in (-1, 2, 2 ** 31 - 1):                        # refused before any device is looked for
        assert L.nka_hip_batch_create_wide_ext(C.byref(h), 4, chunk + 1, 3, 0.01, 0, 0, None, step) == -1 and h.value is None
        assert b"nka_hip_batch_create_wide_ext" in L.nka_hip_last_error() and b"step" in L.nka_hip_last_error()
    for nsys, vlen, mvec, vtol in ((0, 8, 3, 0.01), (65536, 8, 3, 0.01), (4, 0, 3, 0.01), (4, cap + 1, 3, 0.01), (4, 8, 0, 0.01),
                                   (4, 8, nka_amd.BATCH_MAX_MVEC + 1, 0.01), (4, 8, 3, 0.0)):      # the wide batch's limits
        for step in (0, 1):
            assert L.nka_hip_batch_create_wide_ext(C.byref(h), nsys, vlen, mvec, vtol, 0, 0, None, step) == -1 and h.value is None
            assert b"nka_hip_batch_create_wide_ext" in L.nka_hip_last_error()
    with pytest.raises(nka_amd.NKAError, match="waves=True"):
        nka_amd.nka_batch().init(4, 64, 3, ext=True)
    with pytest.raises(nka_amd.NKAError, match="waves=True"):
        nka_amd.nka_batch().init(4, 64, 3, ext=True, step=False, lanes=True)
    for kw in ({"waves": True}, {"lanes": True}, {"storage": nka_amd.STORE_F32}, {"waves": True, "step": True}):
        with pytest.raises(nka_amd.NKAError):
            nka_amd.nka_batch().init(4, chunk + 1, 3, wide=True, ext=True, **kw)
    with pytest.raises(nka_amd.NKAError):
        nka_amd.nka_batch().init(4, 64, 3, ext=True, step=True)
    doc = nka_amd.nka_batch.init.__doc__
    assert "nka_hip_batch_create_wide_ext" in doc and "WIDE EXT" in doc


def test_the_header_carries_the_paragraph_wide_ext():
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    m = re.search(r"^ \*   WIDE EXT  nka_hip_batch_create_wide_ext: (.*?)^ \*   OUT OF SCOPE", hdr, flags=re.M | re.S)
    assert m, "the paragraph"
    par = " ".join(m.group(1).replace("\n *", " ").split())
    for phrase in ("NEITHER SET", "ONE CHUNK:", "SEVERAL CHUNKS:", "EXACT CONSEQUENCES:", "LENGTHS:", "ZERO WEIGHTS:", "FIRST operand",
                   "bit for bit", "gamma(K) sum|fl(w x) y|", "chunk-order chain", "w == 1", "w = 4^k", "does not shield",
                   "nka_hip_batch_offers_weights", "NKA_HIP_ESTATE", "step == 0", "step == 1", "FOUR launches"):
        assert phrase in par, phrase
    assert hdr.index("*   WIDE     nka_hip_batch_create_wide:") < hdr.index("*   WAVES EXT  ") < m.start()
    assert "only the batch above has the weights" not in hdr
    # no ratio is quoted without the record it comes from
    if not os.path.exists(os.path.join(ROOT, "profiles", "r19", "batch_wide_weights_throughput.txt")):
        assert "profiles/r19" not in par and not re.search(r"\d\.\d\d", par), "a figure without its record"


def test_integration_md_example_of_a_weighted_wide_batch_compiles(tmp_path):
    """The wide block of INTEGRATION.md is still the only ```C block that names nka_hip_batch_create_wide; it now names the new
    entry, the setter and the query too; syntax only, as its sibling tests do."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_wide_ext" in b]
    assert len(blocks) == 1
    for name in ("nka_hip_batch_create_wide_ext(&b", "nka_hip_batch_set_dot_weights(b", "nka_hip_batch_offers_weights(b", "nka_hip_batch_accel_step(b",
                 "NKA_HIP_BATCH_KIND_WIDE"):
        assert name in blocks[0], name
    assert re.search(r"nka_hip_batch_create_wide\(", blocks[0]) and "nka_hip_batch_create_wide_step(" in blocks[0], "the old entries' examples stay"
    src = tmp_path / "wide_batch_ext.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
