"""The large-offset tests of the batched accelerator as far as a machine without a GPU can see them: the shapes of
tests/batch_large.py really cross what tests/test_batch_large_gpu.py runs them for, and the arithmetic the kernels and the host
share stays inside its integers at the largest legal arguments (tests/c/batch_large_check.cpp, under sanitizers)."""
import os
import subprocess

import pytest

import batch_large as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = list(G.SHAPES)


def test_arithmetic_at_the_largest_legal_arguments_under_sanitizers():
    """tests/c/batch_large_check.cpp, a stand-alone program built with -fsanitize=address,undefined: wide_part_count and
    wide_part_index at 65 535 systems of 512 chunks, the chunk lengths at the cap, the LDS sizes at mvec = 32 and the overflow
    guard of check_rows at its edge, each against the same formula in __int128."""
    csrc = os.path.join(ROOT, "nka_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "largecheck"], check=True)
    p = subprocess.run([os.path.join(csrc, "build_host", "batch_large_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]


def test_the_figures_worked_out_by_hand_are_what_the_arithmetic_gives():
    """The figures written out by hand where the shapes were chosen."""
    S = G.SHAPES
    assert [(s.kind, s.vlen, s.mvec, s.nsys) for s in S.values()] == [
        ("narrow", 16384, 1, 32800), ("narrow", 16384, 32, 3976), ("narrow", 4099, 3, 2052), ("narrow", 4099, 3, 2052),
        ("wide", 4609, 32, 14030), ("wide", 4609, 3, 2052)]
    b = S["bytes"]
    assert G.on_boundary(b, "w", G.BYTES_4G) == 16384 and G.extent(b, "w", 16384)[0] == G.BYTES_4G
    assert G.on_boundary(b, "F", G.BYTES_4G) == 32766 and G.extent(b, "F", 32766)[0] == G.BYTES_4G - 2
    assert G.on_boundary(b, "X", G.BYTES_4G) == 32762 and G.extent(b, "X", 32762)[0] == G.BYTES_4G - 18
    assert G.on_boundary(b, "wgt", G.BYTES_4G) == 32768 and G.on_boundary(b, "wsrc", G.BYTES_4G) == 32768
    assert all(G.on_boundary(b, s, G.ELEMS_2G) is None for s in G.streams(b))      # (2^31 elements are not reached)
    s = S["slots"]
    assert G.sys_stride(s) == 540672 and G.on_boundary(s, "w", G.ELEMS_2G) == 3971 and G.on_boundary(s, "w", G.BYTES_4G) == 992
    lo = G.extent(s, "w", 3971)[0]
    assert G.ELEMS_2G - lo == 475136 == 29 * 16384            # slots 1 ... 29 below the boundary, 30 ... 33 at or above it
    r = S["rows"]
    assert G.extent(r, "F", 2048) == (2 ** 31 - 2048, 2 ** 31 + 2051) and G.extent(r, "X", 2048) == (2 ** 31 - 4096, 2 ** 31 + 3)
    assert r.ld % 2 == 1 and (2048 * r.ld) % 2 == 0 and (2049 * r.ld) % 2 == 1      # odd ld alternates the 16-byte alignment
    assert G.on_boundary(S["wsrc"], "wsrc", G.ELEMS_2G) == 2048 and G.straddles(S["wsrc"], "wsrc", G.ELEMS_2G, 2048)
    w = S["wide-slots"]
    assert G.nchunk(w) == 3 and G.sys_stride(w) == 153120 and G.on_boundary(w, "w", G.ELEMS_2G) == 14024
    off = G.ELEMS_2G - G.extent(w, "w", 14024)[0]
    assert off == 128768 and off // G.slot_stride(w.vlen) + 1 == 28            # inside slot 28
    wr = S["wide-rows"]
    lo = G.extent(wr, "F", 2048)[0]
    assert G.on_boundary(wr, "F", G.ELEMS_2G) == 2048 and (G.ELEMS_2G - lo) // G.WIDE_CHUNK == 1      # ... in chunk 1


@pytest.mark.parametrize("sid", IDS)
def test_shape_crosses_what_it_claims_and_its_active_set_flanks_it(sid):
    sh = G.SHAPES[sid]
    found = {(stream, name): (B, k) for stream, name, B, k in G.crossings(sh)}
    active = G.active_set(sh)
    assert active == sorted(set(active)) and active[0] == 0 and active[-1] == sh.nsys - 1
    assert len(active) <= G.MAX_ACTIVE, active
    assert set(sh.crosses) <= set(found), (sid, "a boundary of the table is not crossed", set(sh.crosses) - set(found))
    for (stream, name), (B, k) in found.items():      # the claimed ones, and whatever else the shape crosses on its way
        assert G.span(sh, stream) > B and k in active, (sid, stream, name)
        lo, hi = G.extent(sh, stream, k)
        if G.straddles(sh, stream, B, k):
            assert lo < B < hi
        else:                                          # none straddles: k is the first one at or above
            assert lo >= B and G.extent(sh, stream, k - 1)[1] <= B, (sid, stream, name, k)
        below = [j for j in active if G.extent(sh, stream, j)[1] <= B]
        above = [j for j in active if G.extent(sh, stream, j)[0] >= B]
        assert below and above, (sid, stream, name)
        assert k - max(below) <= G.NEAR and min(above) - k <= G.NEAR, (sid, stream, name, k, below, above)
    # the straddling systems the table names
    if sid == "bytes":
        assert G.straddles(sh, "F", G.BYTES_4G, 32766) and G.straddles(sh, "X", G.BYTES_4G, 32762)
    if sid in ("slots", "wide-slots"):
        k = found[("w", "2^31 elements")][1]
        assert G.straddles(sh, "w", G.ELEMS_2G, k) and G.straddles(sh, "w", G.BYTES_4G, found[("w", "2^32 bytes")][1])
    if sid in ("rows", "wide-rows"):
        assert G.straddles(sh, "F", G.ELEMS_2G, 2048) and G.straddles(sh, "F", G.BYTES_4G, 512)
    assert G.total_bytes(sh) <= G.MAX_BYTES, (sid, G.total_bytes(sh) / 2 ** 30)
    assert G.batch_bytes(sh) < G.total_bytes(sh)
    # legal for the library: the caps of the header, and the guard of check_rows
    assert 1 <= sh.mvec <= 32 and sh.ld >= sh.vlen
    assert sh.vlen <= (1048576 if sh.kind == "wide" else 16384) and (sh.kind == "narrow" or sh.nsys <= 65535)
    assert sh.kind == "narrow" or not (sh.weighted or sh.with_x)      # (a wide batch refuses the step and the weights)


@pytest.mark.parametrize("sid", IDS)
def test_witnesses_are_inactive_systems_where_a_wrapped_offset_would_land(sid):
    sh = G.SHAPES[sid]
    active, wit = G.active_set(sh), G.witnesses(sh)
    assert wit and not set(wit) & set(active) and all(0 <= j < sh.nsys for j in wit)
    ss = G.sys_stride(sh)
    for k in active:
        for j in (k - 1, k + 1):
            assert j in wit or j in active or not 0 <= j < sh.nsys
        for wrapped in ((k * ss) % 2 ** 32, (k * ss * 8) % 2 ** 32 // 8):      # in elements of the slot streams
            j = wrapped // ss
            assert j >= sh.nsys or j in active or (j in wit and G.extent(sh, "w", j)[0] <= wrapped < G.extent(sh, "w", j)[1])
    # a shape that passes a boundary of the slot streams has a wrapped landing place far from where it started: a witness, or
    # an active system, which is compared with its twin after every call
    if sid in ("slots", "wide-slots"):
        k = G.on_boundary(sh, "w", G.ELEMS_2G)
        far = (k * ss * 8) % 2 ** 32 // 8 // ss
        assert (far in wit or far in active) and abs(far - k) > 1


@pytest.mark.parametrize("sid", IDS)
def test_lengths_of_the_second_pass(sid):
    sh = G.SHAPES[sid]
    active = G.active_set(sh)
    lens = G.lengths(sh, active)
    assert len(lens) == sh.nsys and all(1 <= n <= sh.vlen for n in lens)
    assert all(n == sh.vlen for k, n in enumerate(lens) if k not in active)
    own = [lens[k] for k in active]
    assert sh.vlen - 1 in own and 513 in own and sh.vlen in own
    if sh.kind == "wide":
        C = G.WIDE_CHUNK
        assert own[:3] == [sh.vlen, 2 * C + 1, C + 513] and {-(-n // C) for n in own} == {1, 2, 3}
