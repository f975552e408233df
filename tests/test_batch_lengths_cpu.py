"""Per-system lengths of the batched accelerator (nka_hip_batch_set_lengths) as far as a machine without a GPU can see them:
the arithmetic the kernels and the host share under sanitizers, the example of INTEGRATION.md, the four prototypes against the
signatures Python calls them with, the refusals that need no device, and the paint of the GPU tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_lengths as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nka_hip_batch_set_lengths", "nka_hip_batch_set_lengths_host", "nka_hip_batch_get_lengths", "nka_hip_batch_has_lengths")


def test_length_arithmetic_for_every_length_under_sanitizers():
    """tests/c/batch_lengths_check.cpp, a stand-alone program built with -fsanitize=address,undefined: for every length
    1 ... 3 CHUNK + 33 the chunks a system owns, their lengths and the partial cells it reads."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "lengthscheck"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_lengths_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_integration_md_example_of_a_ragged_batch_compiles(tmp_path):
    """The C example of INTEGRATION.md for systems of different length against include/nka_hip_batch.h (syntax only)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```c\n(.*?)```", text, flags=re.S) if "nka_hip_batch_set_lengths" in b]
    assert len(blocks) == 1 and "nka_hip_batch_restart" in blocks[0] and "nka_hip_batch_accel_update" in blocks[0]
    src = tmp_path / "ragged_batch.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def _ctype(decl):
    """One parameter of a prototype -> the ctypes type Python must pass: the handle and DEVICE memory travel as addresses,
    host arrays of int32 as pointers to int32."""
    decl = " ".join(decl.split())
    kind, name = decl.rsplit(" ", 1) if not decl.endswith("*") else (decl, "")
    name = name.lstrip("*")
    if kind.startswith("nka_hip_batch_t"):
        return C.c_void_p
    assert "int32_t" in decl and "*" in decl, decl
    assert name.endswith(("_dev", "_host")), decl
    return C.c_void_p if name.endswith("_dev") else C.POINTER(C.c_int32)


def test_the_four_prototypes_match_the_signatures_python_uses():
    from nka_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read(), flags=re.S)
    for name in NAMES:
        m = re.findall(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert len(m) == 1, (name, m)
        ret, params = m[0]
        restype, argtypes = _lib.BATCH_SIGNATURES[name]
        assert ret == "int" and restype is C.c_int, name
        want = [_ctype(p) for p in params.split(",")]
        assert want == list(argtypes), (name, want, argtypes)
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert "LENGTHS" in hdr and re.search(r"RAGGED BATCHES.*?LENGTHS below", hdr, flags=re.S)


def test_library_exports_the_entries_and_refuses_a_null_handle_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    L, D = nka_amd.load(), _lib.load_diag()
    for name in NAMES:
        assert hasattr(L, name) and hasattr(D, name), name
    v = np.ones(3, np.int32)
    p = v.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.nka_hip_batch_set_lengths(None, None) == -1 and L.nka_hip_last_error()
    assert L.nka_hip_batch_set_lengths_host(None, p) == -1 and L.nka_hip_batch_get_lengths(None, p) == -1
    assert L.nka_hip_batch_has_lengths(None) < 0
    b = nka_amd.nka_batch()
    for call in (lambda: b.set_lengths([1, 2, 3]), b.lengths, b.has_lengths):
        try:
            call()
        except nka_amd.NKAError:
            continue
        raise AssertionError("a batch that was never initialised accepted a call")


def test_the_paint_of_the_gpu_tests_is_what_they_rely_on():
    """Distinct payloads that survive a copy, tails that tell a write, shapes that cover the edges named in the GPU tests."""
    a, b = BL.nan_paint(3, 7, 1), BL.nan_paint(3, 7, 2)
    assert np.isnan(a).all() and not np.intersect1d(a.view(np.uint64), b.view(np.uint64)).size
    c = a.copy()
    assert BL.same_bytes(a, c) and BL.tails_intact(c, a, [7, 1, 3]) == []
    c[1, 1] = a[1, 2]                                   # one NaN replaced by another NaN
    assert BL.tails_intact(c, a, [7, 1, 3]) == [1] and BL.tails_intact(c, a, [7, 2, 3]) == []
    for chunk in (2048, 4096, 8192):
        vlen, lens = BL.wide_shape(chunk)
        assert vlen == 3 * chunk + 33 and max(lens) == vlen and min(lens) == 1 and len(set(-(-n // chunk) for n in lens)) == 4
    assert max(BL.NARROW_LENS) == BL.NARROW_VLEN == 1100 and {1, 2, 63, 64, 65, 511, 512, 513} <= set(BL.NARROW_LENS)
    w = BL.weight_rows((1, 65, 300), 300, 3)
    assert np.isfinite(w).all() and (w[0, 1:] == 2.0 ** 500).all() and (w[1, 65:] == 2.0 ** 500).all() and (w[:, 0] > 0).all()
    m = BL.mask_rows((1, 65, 300), 300)
    assert m.sum(axis=1).tolist() == [1.0, 65.0, 300.0]
