"""The lane batch (nka_hip_batch_create_lanes) as far as a machine without a GPU can see it: the layout arithmetic the kernel
and the host share under sanitizers, the Python restatement of it against the C program's table and against the library, the
shape arithmetic of the large-offset case, the example of INTEGRATION.md, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_lanes as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nka_hip_batch_create_lanes", "nka_hip_batch_lanes_limits", "nka_hip_batch_kind")


def _layout_table():
    """`make lanescheck` builds and runs tests/c/batch_lanes_layout_check.cpp (-fsanitize=address,undefined); run once more for
    the table it prints: {mvec: (G, bytes of one lane's working copy)}."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "lanescheck"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_lanes_layout_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("lanes ")]
    return {int(r[1]): (int(r[2]), int(r[3])) for r in rows}


def test_layout_arithmetic_for_every_mvec_under_sanitizers():
    table = _layout_table()
    assert sorted(table) == list(range(1, 33))
    for mvec, (G, lane_bytes) in table.items():
        assert 1 <= G <= 64 and G * lane_bytes <= BL.LDS_BUDGET <= 160 * 1024, mvec
    sizes = [table[m][0] for m in (1, 3, 10, 20, 32)]      # the mvec of the GPU tests
    assert sizes[0] == sizes[1] == 64
    assert len({g for g in sizes if g < 64 and g & (g - 1)}) >= 2, (sizes, "two group sizes below 64 that are no power of two")


def test_the_python_restatement_agrees_with_the_c_program_and_the_library():
    table = _layout_table()
    for mvec in range(1, 33):
        assert (BL.lanes_group(mvec), BL.lane_bytes(mvec)) == table[mvec], mvec
    import nka_amd
    L = nka_amd.load()                                     # (loads on any machine: the limits need no device)
    for mvec in range(1, 33):
        g, cap = C.c_int32(), C.c_int64()
        assert L.nka_hip_batch_lanes_limits(mvec, C.byref(g), C.byref(cap)) == 0
        assert (g.value, cap.value) == (BL.lanes_group(mvec), BL.MAX_VLEN), mvec
        assert nka_amd.batch_lanes_limits(mvec) == (BL.lanes_group(mvec), 64)
    assert L.nka_hip_batch_lanes_limits(0, None, None) == -1 and L.nka_hip_batch_lanes_limits(33, None, None) == -1
    assert L.nka_hip_last_error()
    # vector_bytes: both allocations, the last group whole, no padding of a row
    for vlen, mvec, nsys in ((1, 1, 1), (7, 3, 65), (33, 10, 70), (64, 32, 13), (64, 20, 100000)):
        G = BL.lanes_group(mvec)
        assert BL.vector_bytes(vlen, mvec, nsys) == 2 * 8 * (mvec + 1) * vlen * G * ((nsys + G - 1) // G)
        offs = {BL.slot_offset(vlen, mvec, G, s, k, i) for s in range(min(nsys, 2 * G + 1)) for k in (1, mvec + 1) for i in (0, vlen - 1)}
        assert max(offs) < BL.alloc_elems(vlen, mvec, nsys) and min(offs) == 0


def test_the_shape_arithmetic_of_the_large_case():
    """The boundary is crossed, which group straddles it, at most nine systems run, at most 12 GiB."""
    for G in (None, 5, 6, 7, 14):                          # as built, and what other budgets would give
        sh = BL.large_shape(G)
        G_, gb, nsys, act = sh["G"], sh["group"], sh["nsys"], sh["active"]
        gs = BL.group_stride(sh["vlen"], sh["mvec"], G_)
        each = 8 * BL.alloc_elems(sh["vlen"], sh["mvec"], nsys, G_)
        assert each > 2 ** 32, "the allocation does not pass 2^32 bytes"
        assert 8 * gs * gb < 2 ** 32 < 8 * gs * (gb + 1), "the group does not straddle the boundary"
        lo = 8 * BL.slot_offset(sh["vlen"], sh["mvec"], G_, gb * G_, 1, 0)
        hi = 8 * BL.slot_offset(sh["vlen"], sh["mvec"], G_, gb * G_ + G_ - 1, sh["mvec"] + 1, sh["vlen"] - 1)
        assert lo < 2 ** 32 <= hi
        if G is None:
            assert len(act) <= BL.MAX_ACTIVE and sum(BL.large_bytes(sh).values()) <= BL.MAX_BYTES
            assert {0, nsys - 1} <= set(act) and set(range(gb * G_, (gb + 1) * G_)) <= set(act)
            assert gb * G_ - 1 in act and (nsys - 1) // G_ == gb + 1, "a neighbour on either side of the straddling group"
            for k in act:                                  # every system of the group holds elements on both sides
                if k // G_ == gb:
                    assert 8 * BL.slot_offset(64, 32, G_, k, 1, 0) < 2 ** 32 < 8 * BL.slot_offset(64, 32, G_, k, 33, 63)
            wit = sh["witnesses"]
            assert wit and not set(wit) & set(act) and all(0 <= k < nsys for k in wit)
            # a 32-bit byte offset of the group above the boundary lands in group 0: its masked systems are witnesses
            assert (8 * (gb + 1) * gs) % 2 ** 32 // (8 * gs) == 0 and set(range(1, G_)) <= set(wit)


def test_the_sequences_meet_what_the_gpu_test_asserts(oracle):
    """Dry run of tests/batch_lanes.py: script() on the oracle alone, group 0 of the largest batch of one shape: lists of
    different length, a relax and a dependence drop beside lanes that had none, a list that fills."""
    vlen, mvec = 33, 10
    G = BL.lanes_group(mvec)
    oras = [oracle.OracleNKA(vlen, mvec, 2) for _ in range(G)]
    pend, prev, seen = np.zeros(G, bool), [None] * G, set()
    for op, arg, mask in BL.script(vlen, 2 * G + 3, mvec, 17 * vlen + mvec):
        on = mask[:G] != 0
        nv0 = np.array([o.num_vec() for o in oras])
        if op != "update":
            for k in np.flatnonzero(on):
                (oras[k].relax if op == "relax" else oras[k].restart)()
            pend[on] = False
            continue
        zero = np.zeros(G, bool)
        for k in np.flatnonzero(on):
            zero[k] = pend[k] and np.array_equal(prev[k], arg[k])
            prev[k] = arg[k].copy()
            oras[k].accel_update(arg[k].copy())
        nv = np.array([o.num_vec() for o in oras])
        ran = on & pend
        grew = ran & ~zero & (nv == nv0 + 1)
        seen |= {"lengths"} if len(set(nv.tolist())) > 1 else set()
        seen |= {"relax"} if (ran & zero).any() and grew.any() else set()
        seen |= {"drop"} if (ran & ~zero & (nv0 < mvec) & (nv <= nv0)).any() and grew.any() else set()
        seen |= {"capacity"} if (ran & (nv0 == mvec)).any() else set()
        pend[on] = True
    assert seen == {"lengths", "relax", "drop", "capacity"}, seen
    assert any(op == "relax" for op, _, _ in BL.script(7, 5, 3, 1)) and any(op == "restart" for op, _, _ in BL.script(7, 5, 3, 1))


def test_integration_md_example_of_a_lane_batch_compiles(tmp_path):
    """The C example of INTEGRATION.md for very short systems against include/nka_hip_batch.h (syntax only).  Its fence is
    written ```C, like the wide batch's: the example of many small systems is looked up as THE block fenced ```c that creates a
    batch."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```C\n(.*?)```", text, flags=re.S) if "nka_hip_batch_create_lanes" in b]
    assert len(blocks) == 1 and "nka_hip_batch_lanes_limits" in blocks[0] and "nka_hip_batch_kind" in blocks[0]
    src = tmp_path / "lane_batch.c"
    src.write_text(blocks[0])
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_header_and_library_carry_the_entries_and_refuse_null_handles_on_any_machine():
    import nka_amd
    from nka_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nka_hip_batch.h")).read()
    assert re.search(r"^ \*   LANES ", hdr, flags=re.M) and "NKA_HIP_BATCH_LANES_MAX_VLEN = 64" in hdr
    L, D = nka_amd.load(), _lib.load_diag()
    for name in NAMES:
        assert hasattr(L, name) and hasattr(D, name) and name in _lib.BATCH_SIGNATURES and name in hdr, name
    assert L.nka_hip_batch_kind(None) < 0 and L.nka_hip_last_error()
    assert L.nka_hip_batch_create_lanes(None, 1, 1, 1, 0.01, 0, 0, None) == -1
    h = C.c_void_p()
    for nsys, vlen, mvec in ((0, 8, 3), (4, 65, 3), (4, 0, 3), (4, 8, 33), (4, 8, 0)):      # (refused before any device is looked for)
        assert L.nka_hip_batch_create_lanes(C.byref(h), nsys, vlen, mvec, 0.01, 0, 0, None) == -1 and h.value is None
    assert (nka_amd.KIND_NARROW, nka_amd.KIND_WIDE, nka_amd.KIND_LANES, nka_amd.BATCH_LANES_MAX_VLEN) == (0, 1, 2, 64)
    b = nka_amd.nka_batch()
    try:
        b.kind()
    except nka_amd.NKAError:
        return
    raise AssertionError("a batch that was never initialised accepted a call")
