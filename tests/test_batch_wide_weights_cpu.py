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


def test_the_one_wide_unit_holds_every_form_of_the_five_kernels():
    """nka_batch_wide.hip is the only wide unit: five kernel templates -- the step's norm left the fold of four as a kernel of its
    own, the layout its measurement asked for --, each body written once, what an instance takes in the trailing pack.  The norm and the sums read the weight pair like a stored vector -- ld_tile<FULL, true> from pack_get<WgtRows> +
    wide_wgt_offset, inside if constexpr (WGT), behind the `active` and the length test --, fl(w f) and fl(w w1') are formed once per
    element and sweep and stand FIRST in every product, each weighted product beside its plain form; the scalar kernel and the
    combine never take the weights, and a weighted call launches them.  No atomics, no cooperative launch."""
    assert not os.path.exists(os.path.join(CSRC, "nka_batch_wide_step.hip")), "the step lives in nka_batch_wide.hip"
    assert "nka_batch_wide_step" not in open(os.path.join(CSRC, "Makefile")).read()
    text = open(os.path.join(CSRC, "nka_batch_wide.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert code.count("__global__") == 5      # (the four of the fold, and k_wide_step_norm: the one family its measurement took out)
    for once in ("void wide_list(", "void wide_norm_sum(", "struct WideArgs {", "struct WideStepArgs {", "void k_wide_norm(", "void k_wide_step_norm(",
                 "void k_wide_sums(", "void k_wide_scalar(", "void k_wide_combine("):
        assert code.count(once) == 1, once
    for word in ("atomic", "hipLaunchCooperativeKernel", "__threadfence"):
        assert word not in code, word
    kn = code[code.index("void k_wide_norm("):code.index("void k_wide_step_norm(")]
    kp = code[code.index("void k_wide_step_norm("):code.index("void k_wide_sums(")]
    ks = code[code.index("void k_wide_sums("):code.index("void k_wide_scalar(")]
    tail = code[code.index("void k_wide_scalar("):code.index("void launch_wide(")]
    fma = r"acc\[[^\]]+\] = fma\(([^;]+), acc\[[^\]]+\]\);"
    for kern in (kn, kp, ks):
        head = kern[:kern.index("{")]
        pack = "wgt" if kern is kp else "pack"
        assert re.search(r"const int32_t \*__restrict__ active, (Pack\.\.\. pack|Wgt\.\.\. wgt)\)\s*$", head), head
        assert "static_assert(wide_pack_ok<Pack...>()" in kern or "static_assert(wide_pack_ok<Wgt...>()" in kern
        # a masked system returns before anything of the pack is read; the length test comes before the weight row is addressed
        assert kern.index("active[sys] == 0) return;") < kern.index("pack_get")
        assert kern.index("if (!nka_host::wide_len_owns(sn, ") < kern.index("wide_wgt_offset")
        assert kern.index("if constexpr (LEN)") < kern.index("wide_len_owns") < kern.index("__shared__")
        assert kern.count(f"if constexpr (WGT) wg = pack_get<WgtRows>({pack}...) + (size_t)nka_host::wide_wgt_offset(sys, "
                          f"(int64_t)pack_get<WgtStride>({pack}...), blockIdx.x);") == 1
        assert len(re.findall(r"acc(?:\[[^\]]+\])?\s*(?:\+=|= acc)", kern)) == 0
    # the update's norm: <d,d>; the step's: <d,d> and <f,f>, the latter twice (with and without a pending pair); each weighted form
    # in an if constexpr (WGT) whose else is the plain form; one weight load per sweep body
    first = sorted(f.split(",")[0].strip() for f in re.findall(fma, kn))
    assert first == sorted(["gv[q] * d", "d"]), first
    assert kn.count("if constexpr (WGT) acc[0] = fma(gv[q] * d, d, acc[0]); else acc[0] = fma(d, d, acc[0]);") == 1
    assert kn.count("if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);") == 1 == kn.count("batch_sweep(") == kn.count("gv = ld_tile")
    first = sorted(f.split(",")[0].strip() for f in re.findall(fma, kp))
    assert first == sorted(["gv[q] * d", "gv[q] * fv[q]", "gv[q] * fv[q]", "d", "fv[q]", "fv[q]"]), first
    assert kp.count("if constexpr (WGT) acc[1] = fma(gv[q] * d, d, acc[1]); else acc[1] = fma(d, d, acc[1]);") == 1
    assert kp.count("if constexpr (WGT) acc[0] = fma(gv[q] * fv[q], fv[q], acc[0]); else acc[0] = fma(fv[q], fv[q], acc[0]);") == 2
    assert kp.count("if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);") == 2 == kp.count("batch_sweep(") == kp.count("gv = ld_tile")
    # the step's norm keeps the layout it had: the step's arguments, the lengths in them, in front of f_all; only the weights behind
    assert re.search(r"void k_wide_step_norm\(BatchArgs a, WideArgs wa, WideStepLenArgs st, const double \*__restrict__ f_all,", kp)
    assert "sn = st.len[sys];" in kp and "WideStepArgs" not in kn.split("static_assert")[0]
    # the sums: the three products of today; their first operands are the plain ones unless WGT, formed once per element and sweep
    first = sorted(f.split(",")[0].strip() for f in re.findall(fma, ks))
    assert first == ["fa", "fa", "wa_"], first
    assert ks.count("double fa = fq;") == 1 and ks.count("if constexpr (WGT) fa = gv[q] * fq;") == 1 == ks.count("gv[q] * fq")
    assert ks.count("double wa_ = wn;") == 1 and ks.count("if constexpr (WGT) wa_ = gv[q] * wn;") == 1 == ks.count("gv[q] * wn")
    assert ks.count("if constexpr (WGT) gv = ld_tile<FULL, true>(wg, i, n);") == 1 == ks.count("batch_sweep(") == ks.count("gv = ld_tile")
    # the scalar kernel and the combine never take the weights, and a weighted call launches them
    assert "WgtRows" not in tail and "WgtStride" not in tail and "wide_wgt_offset" not in tail and "gv" not in tail
    assert tail.count("sizeof...(Pack) == (STEP ? 1 : 0) + (LEN ? 1 : 0)") == 2
    launch = code[code.index("void launch_wide("):code.index("void launch_wide_len(")]
    weighted = launch[launch.index("if (b->weighted)"):launch.index("} else {")]
    assert "k_wide_norm<Pack..., WgtRows, WgtStride>" in weighted and "k_wide_sums<COMB, Pack..., WgtRows, WgtStride>" in weighted
    assert "k_wide_step_norm<LEN, WgtRows, WgtStride>" in weighted
    after = launch[launch.index("} else {"):]
    assert "k_wide_scalar<Mask, Pack...>" in after[after.index("}", 1):] and "k_wide_combine<COMB, Pack...>" in after[after.index("}", 1):]
    # four per call: the sums in two forms, the norm in two forms for the update and in two for the step
    assert launch.count("hipLaunchKernelGGL(") == 8 and code.count("hipLaunchKernelGGL(") == 8


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
