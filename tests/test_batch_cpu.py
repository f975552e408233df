"""The batched accelerator (include/nka_hip_batch.h) as far as a machine without a GPU can see it: the symbols, the loud
failure without a device, the layout arithmetic under sanitizers, and the seed rule of the GPU tests."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                    # declarations only, not the prose
    return set(re.findall(r"\b(nka_hip_batch_[a-z0-9_]+)\s*\(", text))


def test_library_exports_every_symbol_of_the_batch_header():
    import nka_amd
    from nka_amd import _lib
    declared = _declared()
    assert len(declared) >= 15 and "nka_hip_batch_accel_update" in declared
    assert declared == set(_lib.BATCH_SIGNATURES), declared ^ set(_lib.BATCH_SIGNATURES)
    L, D = nka_amd.load(), _lib.load_diag()
    for name in sorted(declared):
        assert hasattr(L, name), f"libnka_hip.so lacks {name}"
        assert hasattr(D, name), f"libnka_hip_diag.so lacks {name}"
    assert nka_amd.nka_batch is not None and nka_amd.BATCH_MAX_MVEC >= 32
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert f"NKA_HIP_BATCH_MAX_VLEN = {nka_amd.BATCH_MAX_VLEN}" in hdr and f"NKA_HIP_BATCH_MAX_MVEC = {nka_amd.BATCH_MAX_MVEC}" in hdr


def test_batch_create_fails_loudly_without_a_device():
    import torch
    import nka_amd
    L = nka_amd.load()
    h = C.c_void_p()
    # arguments outside the limits are refused on any machine, before a device is looked for
    for args in [(0, 8, 3), (4, 0, 3), (4, nka_amd.BATCH_MAX_VLEN + 1, 3), (4, 8, 0), (4, 8, nka_amd.BATCH_MAX_MVEC + 1)]:
        assert L.nka_hip_batch_create(C.byref(h), args[0], args[1], args[2], 0.01, -1, 0, None) == -1 and h.value is None
        assert L.nka_hip_last_error()
    if torch.cuda.is_available():
        return                                   # (with a device the GPU tests take over)
    rc = L.nka_hip_batch_create(C.byref(h), 4, 8, 3, 0.01, -1, 0, None)
    assert rc < 0 and h.value is None
    assert L.nka_hip_last_error()
    with pytest.raises(nka_amd.NKAError):
        nka_amd.nka_batch().init(4, 8, 3)


def test_batch_layout_arithmetic_against_a_brute_force_model_under_sanitizers():
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "batchcheck"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_layout_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_seed_rule_of_the_gpu_tests_finds_agreeing_sequences(oracle):
    """A GUARD FOR THE GPU TESTS, not a test of the product (it runs the oracle and tests/batch_seq.py only, and passes
    without the batched accelerator): a system's seed is the first of a fixed series whose dry run keeps the
    extended-precision restatement on the reference's decisions -- checked here for a few shapes, so that a GPU run
    never meets a system without a seed."""
    import batch_seq as B
    for vlen, mvec in [(1, 1), (7, 5), (65, 20), (257, 32), (700, 5)]:
        calls = B.num_calls(vlen, mvec)
        for k in (0, 17, 36):
            seed = B.pick_seed(oracle, vlen, mvec, k, calls)
            assert B.decisions_agree(oracle, vlen, mvec, seed, calls)
    a, b = B.Sequence(33, 5), B.Sequence(33, 5)
    for _ in range(20):
        assert (a.next() == b.next()).all()


def test_integration_md_example_of_many_small_systems_compiles(tmp_path):
    """The C example of INTEGRATION.md "Many small systems" against include/nka_hip_batch.h (syntax only)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```c\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create" in b]
    assert len(blocks) == 1 and "active" in blocks[0] and len(blocks[0].strip().splitlines()) <= 15
    src = tmp_path / "many_small_systems.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
