"""The WIDE batch with binary32 storage (nka_hip_batch_create_wide_stored; include/nka_hip_batch.h, WIDE STORED) as far as a machine
without a GPU can see it: the prototype, the signature and the exports; what is refused before a device is looked for; the texts; the
address arithmetic under sanitizers; the proof that the bound of the exact-sum layer of tests/test_batch_wide_store32_gpu.py notices
an operand that was not rounded as the contract says; the budget of the solve the GPU test replays; the arithmetic of its large case."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import batch_large as G
import batch_store32 as S32
import batch_wide as BW
import batch_wide_store32 as W32
import batch_wide_weights as WW
import exact_sums as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CREATE_STORED = (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                           C.c_int32, C.c_int32])


# ---- prototype, exports, refusals, text ----------------------------------------------------------------------------------------------

def test_prototype_exports_and_refusals_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    decl = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    L, D = nka_amd.load(), _lib.load_diag()
    name = "nka_hip_batch_create_wide_stored"
    assert _lib.BATCH_SIGNATURES[name][0] is CREATE_STORED[0] and list(_lib.BATCH_SIGNATURES[name][1]) == CREATE_STORED[1]
    assert hasattr(L, name) and hasattr(D, name)
    assert re.search(r"int nka_hip_batch_create_wide_stored\(nka_hip_batch_t \*out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,\s*"
                     r"int32_t flavor, int32_t device, void \*stream, int32_t step, int32_t storage\);", decl)
    F32, F64 = nka_amd.STORE_F32, nka_amd.STORE_F64
    assert L.nka_hip_batch_create_wide_stored(None, 1, 1, 1, 0.01, 0, 0, None, 0, F32) == -1
    h = C.c_void_p()
    chunk, cap = nka_amd.batch_wide_limits()
    for storage in (F32, F64):                               # all of it refused before any device is looked for
        for step in (-1, 2, 2 ** 31 - 1):
            assert L.nka_hip_batch_create_wide_stored(C.byref(h), 4, chunk + 1, 3, 0.01, 0, 0, None, step, storage) == -1 and h.value is None
            assert b"nka_hip_batch_create_wide_stored" in L.nka_hip_last_error() and b"step" in L.nka_hip_last_error()
        for nsys, vlen, mvec, vtol in ((0, 8, 3, 0.01), (65536, 8, 3, 0.01), (4, 0, 3, 0.01), (4, cap + 1, 3, 0.01), (4, 8, 0, 0.01),
                                       (4, 8, nka_amd.BATCH_MAX_MVEC + 1, 0.01), (4, 8, 3, 0.0)):      # the wide batch's limits
            for step in (0, 1):
                assert L.nka_hip_batch_create_wide_stored(C.byref(h), nsys, vlen, mvec, vtol, 0, 0, None, step, storage) == -1 and h.value is None
                assert b"nka_hip_batch_create_wide_stored" in L.nka_hip_last_error()
    for storage in (2, -1, 2 ** 31 - 1):
        assert L.nka_hip_batch_create_wide_stored(C.byref(h), 4, chunk + 1, 3, 0.01, 0, 0, None, 0, storage) == -1 and h.value is None
        assert b"storage" in L.nka_hip_last_error()
    for flavor in (nka_amd.FLAVOR_F08, nka_amd.FLAVOR_F08_VECTOR):
        assert L.nka_hip_batch_create_wide_stored(C.byref(h), 4, chunk + 1, 3, 0.01, flavor, 0, None, 1, F32) == -1 and h.value is None
        assert b"flavour" in L.nka_hip_last_error()
    # the older entries keep their own refusals and texts
    assert L.nka_hip_batch_create_stored(C.byref(h), 4, cap, 3, 0.01, 0, 0, None, F32) == -1 and b"nka_hip_batch_create_wide" in L.nka_hip_last_error()
    assert L.nka_hip_batch_create_wide_ext(C.byref(h), 4, 8, 3, 0.01, 0, 0, None, 2) == -1 and b"nka_hip_batch_create_wide_ext" in L.nka_hip_last_error()
    # Python: the new keyword needs wide=True; the three pinned spellings keep raising
    for kw in ({}, {"storage": F32}, {"lanes": True}, {"waves": True}, {"waves": True, "ext": True}):
        with pytest.raises(nka_amd.NKAError, match="wide_storage"):
            nka_amd.nka_batch().init(4, 64, 3, wide_storage=F32, **kw)
    for kw in ({"wide": True}, {"wide": True, "step": True}, {"wide": True, "ext": True}):
        with pytest.raises(nka_amd.NKAError):                # (on a machine with a device: for `storage`, tests/test_batch_wide_store32_gpu.py)
            nka_amd.nka_batch().init(4, chunk + 1, 3, storage=F32, **kw)
    doc = nka_amd.nka_batch.init.__doc__
    assert "nka_hip_batch_create_wide_stored" in doc and "WIDE STORED" in doc and "wide_storage=STORE_F32" in doc
    assert "not offered by a wide batch yet" not in open(os.path.join(ROOT, "nka_amd", "csrc", "nka_batch.hip")).read()


def test_the_header_carries_the_paragraph_wide_stored():
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    m = re.search(r"^ \*   WIDE STORED  nka_hip_batch_create_wide_stored\((.*?)^ \*   OUT OF SCOPE", hdr, flags=re.M | re.S)
    assert m, "the paragraph"
    par = " ".join(m.group(1).replace("\n *", " ").split())
    for phrase in ("bit for bit and launch for launch", "ONE CHUNK:", "SEVERAL CHUNKS:", "THE CONTRACT", "PER CHUNK", "q(fl(d/s))",
                   "q(fl(fl(v1/s) - w1'))", "the pending pair stays binary64", "subnormals are kept", "+-Inf", "FOUR launches",
                   "no atomics", "capture from the first call", "gamma(K) sum|xy|", "widening is exact", "chunk-order chain",
                   "2 nsys stride (4 (mvec + 1) + 8)", "8-byte aligned", "nothing left allocated", "NKA_HIP_SUMS_REFERENCE_ORDER",
                   "MEMORY:", "COST"):
        assert phrase in par, phrase
    assert hdr.index("*   WIDE EXT  nka_hip_batch_create_wide_ext:") < m.start()
    assert "a batch of nka_hip_batch_create_wide_stored offers it" in " ".join(hdr[hdr.index("*   WIDE     "):hdr.index("*   LENGTHS  ")].replace("\n *", " ").split())
    assert "a batch of nka_hip_batch_create_wide_stored offers it" in " ".join(hdr[hdr.index("*   STORAGE  "):hdr.index("*   LANES    ")].replace("\n *", " ").split())
    # no ratio is quoted without the record it comes from
    if not os.path.exists(os.path.join(ROOT, "profiles", "r21", "batch_wide_store32_throughput.txt")):
        assert "profiles/r21" not in par, "a record that is not there"


def test_integration_md_example_of_a_binary32_wide_batch_compiles(tmp_path):
    """The wide block of INTEGRATION.md names the new entry with both queries; syntax only, as its sibling tests do."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_wide_stored" in b]
    assert len(blocks) == 1
    for name in ("nka_hip_batch_create_wide_stored(&b", "NKA_HIP_BATCH_STORE_F32", "nka_hip_batch_storage(b", "nka_hip_batch_vector_bytes(b",
                 "nka_hip_batch_accel_step(b"):
        assert name in blocks[0], name
    src = tmp_path / "wide_batch_stored.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_the_binary32_members_of_the_wide_unit():
    """Store32Args lives in nka_batch_dev.hpp, once; it is a member of the wide pack ahead of the weights; every binary32 statement
    of the wide unit stands under if constexpr (S32), and the norm kernels take no such statement."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    code = lambda f: "\n".join(ln.split("//")[0] for ln in open(os.path.join(csrc, f)).read().splitlines())
    assert code("nka_batch_dev.hpp").count("struct Store32Args {") == 1 and "struct Store32Args" not in code("nka_batch.hip")
    wide = code("nka_batch_wide.hip")
    assert "struct Store32Args" not in wide
    rank = wide[wide.index("constexpr int wide_pack_rank"):wide.index("constexpr bool wide_pack_ok")]
    assert rank.index("LenRows") < rank.index("Store32Args") < rank.index("WgtRows") < rank.index("WgtStride")
    kn = wide[wide.index("void k_wide_norm("):wide.index("void k_wide_sums(")]
    assert "S32" not in kn and "ld_tile32" not in kn and "batch_q32" not in kn
    for ln in wide.splitlines():
        if ("ld_tile32" in ln or "st_tile32" in ln or "batch_q32(" in ln) and "if constexpr (S32)" not in ln:
            assert ln.startswith("        "), ln             # (inside the S32 block of the combine)
    assert wide.count("static_assert(!S32 || COMB == 2") == 2


# ---- the address arithmetic ------------------------------------------------------------------------------------------------------------

def test_float_slot_and_pending_addresses_of_a_wide_batch_under_sanitizers():
    """tests/c/batch_wide_store32_check.cpp (its own main, -fsanitize=address,undefined): for every chunk of the lengths 1 ... 3C + 33
    the bytes of a float slot row and of the pending row are painted once each below the length and nowhere else, pairs are 8- and
    16-byte aligned, and every offset and size equals its __int128 value at the largest legal arguments."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "widestore32check"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_wide_store32_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^hostcheck:.*\bwidestore32check\b", mk, flags=re.M)


@pytest.mark.parametrize("nsys,vlen,mvec", [(1, 1, 1), (3, 2049, 6), (5, 4609, 10), (2, 6177, 32), (4, 18433, 20)])
def test_vector_bytes_is_the_storage_formula_at_the_wide_stride(nsys, vlen, mvec):
    st = (vlen + 31) // 32 * 32
    assert W32.vector_bytes(nsys, vlen, mvec, W32.STORE_F32) == 2 * nsys * st * (4 * (mvec + 1) + 8)
    assert W32.vector_bytes(nsys, vlen, mvec, W32.STORE_F64) == 2 * nsys * st * 8 * (mvec + 1)


# ---- the sentinels of the exact-sum layer ------------------------------------------------------------------------------------------------

def _operands(n, c, seed):
    """x: a normalised difference before q() (|x| <= 1); y: a widened stored older vector.  At every sentinel of the wide kernels x is
    2^-e (1 + 3 * 2^-25), e in 1..3: q(x) rounds UP by 2^-e 2^-25, truncation rounds DOWN by 3 * 2^-e 2^-25, and keeping x unrounded
    is off by the former; y is +-1/2 there so the product is large (tests/test_batch_store32_cpu.py: _operands)."""
    rng = np.random.default_rng([3233, n, seed])
    x = rng.standard_normal(n) * 0.01
    y = S32.q(rng.standard_normal(n) * 0.01)
    idx = BW.wide_sentinel_indices(n, c)
    x[idx] = np.ldexp(1.0 + 3.0 * 2.0 ** -25, -rng.integers(1, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    y[idx] = 0.5 * rng.choice([-1.0, 1.0], idx.size)
    return x, y, idx


@pytest.mark.parametrize("which", ["C+1", "2C+513"])
def test_an_operand_not_rounded_as_the_contract_says_breaks_the_bound_of_a_chunked_sum(which):
    """The exact-sum layer of the GPU test holds red[2 + p] to gamma(wide_k(n)) sum|xy| of exact_dot(q(w1'), w_p).  On the host model
    of a chunked sum (batch_wide.model_partials, the chunk-order chain): the sum of the contract's operands is inside that bound and
    no chunk's partial could be lost unseen; with ONE planted sentinel taken unrounded, or rounded by truncation, it is outside -- at
    every sentinel of every chunk."""
    c = BW.limits()[0]
    n = WW.shape(which, c)
    x, y, idx = _operands(n, c, 0)
    xq = S32.q(x)
    assert (xq[idx] != x[idx]).all() and (S32.q_trunc(x)[idx] != xq[idx]).all()
    k = BW.wide_k(n, c)
    bound, tot, exact = X.gamma(k), X.abs_dot(xq, y), X.exact_dot(xq, y)
    assert BW.undetectable_chunks(xq, y, k, c) == []
    parts = BW.model_partials(xq, y, c)
    assert abs(BW.model_sum_of(parts, range(parts.size)) - exact) <= bound * tot          # the contract's sum: inside
    for what, wrong in (("unrounded", x), ("truncated", S32.q_trunc(x))):
        for i in idx:
            mut = xq.copy()
            mut[i] = wrong[i]
            term = (mut[i] - xq[i]) * y[i]
            assert X.detectable(term, bound, tot), (what, n, int(i), term, bound * tot)
            ch = int(i) // c
            p2 = parts.copy()
            p2[ch] = BW.model_partials(mut[ch * c:(ch + 1) * c], y[ch * c:(ch + 1) * c], c)[0]
            got = BW.model_sum_of(p2, range(p2.size))
            assert abs(got - exact) > bound * tot, (what, n, int(i), "the bound did not notice")


# ---- the budget of the solve ---------------------------------------------------------------------------------------------------------------

def test_the_replay_budget_of_the_ragged_weighted_solve_holds_on_the_host_model_with_binary32_storage(oracle):
    """The solve the GPU test replays, through the host model of the STORAGE contract with the weighted dot product and np.dot sums:
    every system retires SOLVE_SLACK steps inside SOLVE_REPLAYS with binary32 storage, as it does with binary64 storage; both sets of
    iterations go to the dump directory."""
    import parity_util as P
    c, _ = BW.limits()
    it32 = W32.solve_on_the_model(oracle, c, True)
    it64 = W32.solve_on_the_model(oracle, c, False)
    print("host model, binary32", it32.tolist(), "binary64", it64.tolist())
    out = P.dump_dir(ROOT)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "batch_wide_store32_model_solve.json"), "w") as fh:
            json.dump({"binary32": [int(v) for v in it32], "binary64": [int(v) for v in it64], "tol": WW.SOLVE_TOL, "mvec": WW.SOLVE_MVEC},
                      fh, indent=1, sort_keys=True)
    budget = WW.SOLVE_REPLAYS - WW.SOLVE_SLACK
    assert (it64 >= 1).all() and it64.max() <= budget, it64
    assert (it32 >= 1).all() and it32.max() <= budget and len(set(it32.tolist())) >= 3, it32


# ---- the large case ------------------------------------------------------------------------------------------------------------------------

def test_the_large_case_crosses_what_it_is_there_for():
    sh = W32.LARGE
    assert (sh.kind, sh.vlen, sh.mvec, sh.nsys) == ("wide", 4609, 32, 14030) and G.nchunk(sh) == 3
    elems = G.sys_stride(sh) * sh.nsys
    assert elems > 2 ** 31 and 4 * elems > 2 ** 32                             # one float allocation: elements and bytes
    act, wit, bd = W32.large_active(), W32.large_witnesses(), W32.large_boundaries()
    assert 7 <= len(act) <= W32.MAX_ACTIVE == 9 and act[0] == 0 and act[-1] == sh.nsys - 1 and wit and not set(act) & set(wit)
    assert set(bd) == {2 ** 30, 2 ** 31}
    for B, k in bd.items():
        assert k in act and G.straddles(sh, "w", B, k), (B, k)                  # which system straddles each boundary
        assert k - 1 in act and k + 1 in act
        assert G.extent(sh, "w", k - 1)[1] <= B <= G.extent(sh, "w", k + 1)[0]
    assert bd[2 ** 30] == 2 ** 30 // G.sys_stride(sh) and bd[2 ** 31] == 2 ** 31 // G.sys_stride(sh)
    assert 18 * 10 ** 9 < W32.vector_bytes(sh.nsys, sh.vlen, sh.mvec, W32.STORE_F32) < W32.large_bytes() <= W32.MAX_BYTES == 20 * 2 ** 30
