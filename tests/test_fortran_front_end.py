"""The Fortran host layer (nka_amd/fortran): module nka_type over iso_c_binding,
the abstract vector class, the device block vector and the example driver."""
import json
import os
import subprocess

import numpy as np
import pytest

import parity_util as P
import scenarios as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "nka_amd", "fortran", "build")


@pytest.fixture(scope="module")
def fortran_build():
    import nka_amd
    if not os.path.exists(nka_amd.lib_path()):
        nka_amd.build()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "nka_amd", "fortran")], check=True)
    return BUILD


def _tables():
    with open(os.path.join(S.GOLD, "example_tables.json")) as fh:
        return json.load(fh)


def test_example_driver_without_acceleration_matches_reference_table(fortran_build):
    """CPU only (mvec = 0 never touches the GPU): the Fortran restatement of the
    example problem prints the reference's 367-iteration table digit for digit."""
    p = subprocess.run([os.path.join(fortran_build, "nka_example")], capture_output=True, text=True, check=True)
    assert p.stdout.splitlines() == _tables()["f08"]


@pytest.mark.gpu
@pytest.mark.parametrize("args,key", [(["--nka-vec", "5"], "f08 --nka-vec 5"),
                                      (["--sweeps", "4", "--nka-vec", "5"], "f08 --sweeps 4 --nka-vec 5")])
@pytest.mark.parametrize("flavor", ["0", "2"])
def test_config1_through_fortran_front_end_on_gpu(fortran_build, args, key, flavor):
    """BASELINE config 1: Fortran host code -> iso_c_binding -> HIP kernels
    reproduces every printed digit of every iteration of reference_output."""
    p = subprocess.run([os.path.join(fortran_build, "nka_example")] + args + ["--flavor", flavor],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.splitlines() == _tables()[key]


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_norm", [1, 0])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nfield,nper,mvec,ncalls", [(4, 2503, 6, 24), (1, 64, 3, 12), (3, 1, 2, 8), (4, 2503, 20, 45),
                                                     (4, 25003, 30, 50)])   # (lists beyond one launch: the stages store)
def test_abstract_vector_flavour_on_device_block_vector(fortran_build, oracle, tmp_path, nfield, nper, mvec, ncalls,
                                                        compact, fuse_norm):
    """vector_class hooks on a device-resident block vector, driven by the
    vector flavour of nka_type, against the oracle's F08-vector flavour.
    fuse_norm 1 (default): the norm and both inner-product rows in ONE pure-read pass
    (update_norm2_dots; two passes and two reductions per update); 0: the norm stage as a
    pass of its own (NKA_HIP_VEC_FUSE_NORM=0; the reference's rounding of the Gram row)."""
    out = tmp_path / "vec.bin"
    p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), "check", str(nfield), str(nper),
                        str(mvec), str(ncalls), str(out), str(compact)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, NKA_HIP_VEC_FUSE_NORM=str(fuse_norm)))
    assert p.returncode == 0, p.stdout + p.stderr
    n = nfield * nper
    raw = np.fromfile(out, dtype=np.float64).reshape(ncalls, 2 * n + 1)
    ora = oracle.OracleNKA(n, mvec, oracle.F08_VECTOR)
    spread = P.Spread(oracle, n, mvec)
    for t in range(ncalls):
        x, nv, got = raw[t, :n], int(raw[t, n]), raw[t, n + 1:]
        f = x.copy()
        ora.accel_update(f)
        spread.update(x)
        assert nv == ora.num_vec(), (t, nv, ora.num_vec())
        P.check(S.rel_err(got, f, x), ora.state(),
                f"abstract vector {nfield}x{nper} m={mvec} compact={compact} fuse_norm={fuse_norm} vs oracle F08-vector",
                where=t, spread=spread.value,
                truth=spread.truth(got, x))


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("mode,dims,mvec,ncalls", [("check", (4, 2503), 20, 45), ("check", (4, 25003), 30, 50),
                                                   ("checkgrid", (33, 17), 20, 45)])
def test_rounded_sum_mode_of_the_workspace_is_the_separate_norm_stage(fortran_build, tmp_path, mode, dims, mvec, ncalls,
                                                                      compact):
    """hip_block_vector_set_sum_order(ws, NKA_HIP_SUMS_BLOCKED_ROUNDED) (the driver's compact argument + 20) is the
    caller-visible form of what NKA_HIP_VEC_FUSE_NORM=0 does for the tests: the norm as a pass of its own, the Gram
    row summed on the rounded pair.  Same bits call after call, whatever the environment says about fusing."""
    outs = []
    for icompact, fuse in ((compact, "0"), (compact + 20, "1")):
        out = tmp_path / f"r{icompact}.bin"
        p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), mode, str(dims[0]), str(dims[1]),
                            str(mvec), str(ncalls), str(out), str(icompact)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, NKA_HIP_VEC_FUSE_NORM=fuse))
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]
    fused = tmp_path / "fused.bin"                       # (and the mode is not a no-op: the fused default rounds differently)
    p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), mode, str(dims[0]), str(dims[1]),
                        str(mvec), str(ncalls), str(fused), str(compact)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, NKA_HIP_VEC_FUSE_NORM="1"))
    assert p.returncode == 0, p.stdout + p.stderr
    if mode == "check":
        assert fused.read_bytes() != outs[1]


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("mode,dims,mvec,ncalls", [("check", (4, 2503), 20, 45), ("check", (4, 25003), 30, 50),
                                                   ("checkgrid", (33, 17), 20, 45), ("checkgrid", (7, 5), 3, 14)])
def test_deferred_normalisation_through_the_front_end_is_bit_identical(fortran_build, tmp_path, mode, dims, mvec, ncalls,
                                                                       compact):
    """The block vector's scale-and-dot stage as a pure read with the combine stage
    normalising the new pair (the default) against the storing stages
    (NKA_HIP_VEC_DEFER_SCALE=0): the vector flavour of the accelerator must return
    the same bits call after call -- block vector and grid vector (whose ghost ring
    takes the tail path), lists within and beyond one launch."""
    outs = []
    for defer in ("0", "1"):
        out = tmp_path / f"defer{defer}.bin"
        env = dict(os.environ, NKA_HIP_VEC_DEFER_SCALE=defer, NKA_HIP_VEC_FUSE_NORM="0")   # (fusing needs the deferral)
        p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), mode, str(dims[0]), str(dims[1]),
                            str(mvec), str(ncalls), str(out), str(compact)], capture_output=True, text=True, timeout=300,
                           env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nx,ny,mvec,ncalls", [(7, 5, 3, 14), (50, 50, 6, 24), (33, 17, 20, 45), (1, 1, 2, 6)])
def test_abstract_vector_flavour_on_device_grid_vector_with_ghost_ring(fortran_build, oracle, tmp_path, nx, ny, mvec,
                                                                       ncalls, compact):
    """hip_grid_vector: elementwise hooks cover the ghost ring,
    reductions do not (grid_vector_type.F90:104-195).  Every value of the
    (nx+2) x (ny+2) input, ghosts included, is random, so a reduction that saw a
    ghost would change the coefficients.  Checked against the compiled reference
    on its OWN grid_vector (oracle/_ref/libnka_ref_f08vec.so) over the whole array,
    and against the oracle on the interior (which also supplies the pivots of the
    tolerance rule)."""
    out = tmp_path / "grid.bin"
    p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), "checkgrid", str(nx), str(ny),
                        str(mvec), str(ncalls), str(out), str(compact)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    ntot = (nx + 2) * (ny + 2)
    raw = np.fromfile(out, dtype=np.float64).reshape(ncalls, 2 * ntot + 1)
    ora = oracle.OracleNKA(nx * ny, mvec, oracle.F08_VECTOR)
    spread = P.Spread(oracle, nx * ny, mvec)
    have_ref = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libnka_ref_f08vec.so"))
    ref = oracle.RefF08Vector(nx, ny, mvec) if have_ref else None
    key = f"abstract vector on grid vector {nx}x{ny} m={mvec} compact={compact}"
    for t in range(ncalls):
        x = raw[t, :ntot].reshape(ny + 2, nx + 2)          # Fortran array(0:nx+1,0:ny+1), first index fastest
        nv, got = int(raw[t, ntot]), raw[t, ntot + 1:].reshape(ny + 2, nx + 2)
        xin = np.ascontiguousarray(x[1:-1, 1:-1]).ravel()
        f = xin.copy()
        ora.accel_update(f)
        spread.update(xin)
        assert nv == ora.num_vec(), (t, nv, ora.num_vec())
        gin = np.ascontiguousarray(got[1:-1, 1:-1]).ravel()
        P.check(S.rel_err(gin, f, xin), ora.state(), key + " interior vs oracle F08-vector", where=t, spread=spread.value,
                truth=spread.truth(gin, xin))
        if ref is not None:
            full = np.ascontiguousarray(x).ravel().copy()
            ref.accel_update(full)
            assert nv == ref.num_vec(), (t, nv, ref.num_vec())
            # whole array, ghosts included, against the reference's own ghost handling
            # (ghosts included.  No extended-precision run of the reference's grid_vector exists; the interior is held
            #  to the truth rule above -- device within 2 err_ref of the truth, the reference err_ref from it -- so the
            #  two may differ by 3 err_ref; the ghost values see the same coefficients)
            P.record(S.rel_err(got.ravel(), full, x.ravel()), max(1e-12, 3.0 * spread.err_ref),
                     key + " whole array vs compiled reference")


@pytest.mark.gpu
@pytest.mark.parametrize("nfield,nper,mvec,ncalls", [(4, 2503, 6, 24), (1, 64, 3, 12), (3, 1, 2, 8), (4, 2503, 20, 45), (2, 4099, 30, 50),
                                                     (4, 25003, 5, 12)])   # (the last: a dozen groups of the per-sum machinery per dot)
def test_abstract_vector_flavour_with_reference_order_sums_returns_the_reference_bits(fortran_build, oracle, tmp_path, nfield,
                                                                                      nper, mvec, ncalls):
    """hip_block_vector_set_sum_order(ws, NKA_HIP_SUMS_REFERENCE_ORDER) (driver: compact argument + 10): dot() sums element
    after element, the reduction-bearing batched / stage hooks run their default bodies -- the reference's own sequence of
    deferred hook calls -- and the vector flavour of the accelerator returns the oracle's F08-vector outputs BIT FOR BIT."""
    out = tmp_path / "vecref.bin"
    p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), "check", str(nfield), str(nper),
                        str(mvec), str(ncalls), str(out), "10"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    n = nfield * nper
    raw = np.fromfile(out, dtype=np.float64).reshape(ncalls, 2 * n + 1)
    ora = oracle.OracleNKA(n, mvec, oracle.F08_VECTOR)
    for t in range(ncalls):
        x, nv, got = raw[t, :n], int(raw[t, n]), raw[t, n + 1:]
        f = x.copy()
        ora.accel_update(f)
        assert nv == ora.num_vec(), (t, nv, ora.num_vec())
        assert np.array_equal(got, f), (t, float(np.abs(got - f).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,mvec,ncalls", [(7, 5, 3, 14), (50, 50, 6, 24), (33, 17, 20, 45), (1, 1, 2, 6)])
def test_grid_vector_with_reference_order_sums_equals_the_compiled_reference_on_its_own_grid_vector(fortran_build, oracle, tmp_path,
                                                                                                    nx, ny, mvec, ncalls):
    """The same on hip_grid_vector, against the COMPILED reference running its own grid_vector
    (oracle/_ref/libnka_ref_f08vec.so): the whole (nx+2) x (ny+2) array of every output, ghost ring included, equal in
    every bit."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libnka_ref_f08vec.so")):
        pytest.skip("the compiled reference is not built (oracle/_ref)")
    out = tmp_path / "gridref.bin"
    p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), "checkgrid", str(nx), str(ny),
                        str(mvec), str(ncalls), str(out), "10"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    ntot = (nx + 2) * (ny + 2)
    raw = np.fromfile(out, dtype=np.float64).reshape(ncalls, 2 * ntot + 1)
    ref = oracle.RefF08Vector(nx, ny, mvec)
    for t in range(ncalls):
        x, nv, got = raw[t, :ntot], int(raw[t, ntot]), raw[t, ntot + 1:]
        full = x.copy()
        ref.accel_update(full)
        assert nv == ref.num_vec(), (t, nv, ref.num_vec())
        assert np.array_equal(got, full), (t, float(np.abs(got - full).max()))


@pytest.mark.gpu
def test_fortran_array_bench_runs(fortran_build):
    p = subprocess.run([os.path.join(fortran_build, "nka_bench"), "2000000", "6", "5", "0"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "updates/s" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,flavor", [(100003, 6, 2), (4097, 3, 0), (250000, 20, 1)])
def test_out_of_place_update_and_list_bound_through_the_fortran_front_end(fortran_build, n, m, flavor):
    """call accel%accel_update_swap(f_io, f_acc) and accel%list_bound() of the drop-in module nka_type (round 4): against
    accel_update_dev on the same inputs bit for bit, dependence drops and a repeated input included; with a
    synchronisation per call the host's bound equals the true list length (nka_amd/fortran/array/nka_swap_driver.F90)."""
    p = subprocess.run([os.path.join(fortran_build, "nka_swap_driver"), str(n), str(m), str(m + 16), str(flavor)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "OK calls=" in p.stdout
    below = int(p.stdout.split("calls_with_a_bound_below_the_plain_count=")[1].split()[0])
    assert below >= 3, p.stdout            # the dependence drops were seen by the host


@pytest.mark.gpu
def test_abstract_vector_bench_mode_runs(fortran_build):
    p = subprocess.run([os.path.join(fortran_build, "nka_vector_driver"), "bench", "4", "100000", "5", "5"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "updates/s" in p.stdout


def _reverse_dot(x, y):
    d = 0.0
    for a, b in zip(x[::-1].tolist(), y[::-1].tolist()):
        d = d + a * b
    return d


def _lcg_scenario_oracle(oracle, flavor, vtol=0.05, dot=None, with_outputs=False):
    n, m = 501, 4
    X = oracle.lcg_vectors(12, n, seed=1)
    acc = oracle.OracleNKA(n, m, flavor)
    acc.set_vec_tol(vtol)
    if dot is not None:
        acc.set_dot_prod(dot)                      # the oracle's restatement of F08:209-219
    rows, outs = [], []
    for t in range(1, 13):
        f = X[t - 1].copy()
        acc.accel_update(f)
        outs.append(f.copy())
        if t == 6:
            acc.relax()
        if t == 9:
            acc.restart()
        rows.append((t, acc.num_vec(), float(np.sum(f)), float(np.sqrt(np.sum(f * f)))))
    return (rows, np.array(outs)) if with_outputs else rows


def _env_flavor(env_flavor):
    """The front ends pass NKA_HIP_FLAVOR_DEFAULT: compact storage (the C statement) unless
    the environment variable NKA_HIP_FLAVOR names another flavour (include/nka_hip.h)."""
    env = dict(os.environ)
    env.pop("NKA_HIP_FLAVOR", None)
    if env_flavor:
        env["NKA_HIP_FLAVOR"] = env_flavor
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("exe,env_flavor,flavor_name", [("nka_f95_driver", None, "C_FLAVOR"), ("nka_f95_driver", "f08", "F08"),
                                                        ("nka_c_driver", None, "C_FLAVOR")])
def test_f95_wrappers_and_c_compat_header_on_gpu(fortran_build, oracle, exe, env_flavor, flavor_name):
    """Rows f2/f3: the reference's C API names (include/nka_c_compat.h) and its F95
    procedural API (nka_amd/fortran/f95) over the same HIP library."""
    p = subprocess.run([os.path.join(fortran_build, exe)], capture_output=True, text=True, timeout=300,
                       env=_env_flavor(env_flavor))
    assert p.returncode == 0, p.stdout + p.stderr
    want = _lcg_scenario_oracle(oracle, getattr(oracle, flavor_name))
    got = [ln.split() for ln in p.stdout.splitlines() if ln.strip()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (int(g[0]), int(g[1])) == (w[0], w[1])
        assert float(g[2]) == pytest.approx(w[2], abs=1e-11)
        assert float(g[3]) == pytest.approx(w[3], rel=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("exe,args,env_flavor,flavor_name",
                         [("nka_dp_driver", [], "f08", "F08"), ("nka_dp_driver", [], None, "C_FLAVOR"),
                          ("nka_f95_driver", ["dp"], "f08", "F08"), ("nka_f95_driver", ["dp"], None, "C_FLAVOR"),
                          ("nka_c_driver", ["dp"], None, "C_FLAVOR")])
def test_user_dot_product_through_every_front_end(fortran_build, oracle, tmp_path, exe, args, env_flavor, flavor_name):
    """Rows a14 / f2 / f3: a caller's own dot product, installed the reference's way
    -- call a%set_dot_prod(dp) (F08:209-214), the optional dp of the F95
    nka_accel_update (src-F95:278-291), the dp argument of the C nka_init
    (.h:4) -- is really used (it sums in reverse order) and reproduces the oracle's
    set_dot_prod run on the same inputs BIT FOR BIT: the operands handed to dp
    are bit-identical to the reference's, the scalar step and the elementwise
    statements are bit-exact."""
    raw = tmp_path / "out.bin"
    p = subprocess.run([os.path.join(fortran_build, exe)] + args + [str(raw)], capture_output=True, text=True,
                       timeout=300, env=_env_flavor(env_flavor))
    assert p.returncode == 0, p.stdout + p.stderr
    want, outs = _lcg_scenario_oracle(oracle, getattr(oracle, flavor_name), dot=_reverse_dot, with_outputs=True)
    _, plain = _lcg_scenario_oracle(oracle, getattr(oracle, flavor_name), with_outputs=True)
    assert not np.array_equal(outs, plain)                        # the reverse-order dp does change last bits
    got = [ln.split() for ln in p.stdout.splitlines() if ln.strip()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (int(g[0]), int(g[1])) == (w[0], w[1])
    dev = np.fromfile(raw, dtype=np.float64).reshape(outs.shape)
    assert np.array_equal(dev, outs), np.abs(dev - outs).max()


# ---------------------------------------------------------------------------
# Drop-in: the reference's OWN callers compiled unchanged against our modules
# (oracle/Makefile target `dropin`; built only where /root/reference exists, the
# executables travel to the GPU box with oracle/_ref/).
# ---------------------------------------------------------------------------
REFDIR = os.path.join(ROOT, "oracle", "_ref")


def _ours_env():
    """The drop-ins that link libnka_hip.so run against THIS tree's build of it, wherever oracle/_ref was built or put
    (their run path $ORIGIN/../../nka_amd follows a symlinked oracle/_ref to the directory it points to)."""
    lib_dir = os.path.join(ROOT, "nka_amd")
    return dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(d for d in (lib_dir, os.environ.get("LD_LIBRARY_PATH")) if d))


CASES = [([], "f08"), (["--nka-vec", "5"], "f08 --nka-vec 5"), (["--sweeps", "4", "--nka-vec", "5"], "f08 --sweeps 4 --nka-vec 5")]


@pytest.mark.skipif(not os.path.exists(os.path.join(REFDIR, "dropin_example_f08vec")), reason="drop-in build absent")
@pytest.mark.parametrize("args,key", CASES)
def test_reference_vector_caller_and_user_vector_type_against_our_modules(tmp_path, args, key):
    """Reference src-F08-vector/{grid_vector_type,nka_example}.F90 -- a user type
    that extends `vector`, and its caller -- linked with OUR vector_class and
    vector-flavour nka_type: the plugin interface is intact and the three
    reference_output tables come out digit for digit.  (The user's hooks are CPU
    code, so this runs anywhere.)"""
    p = subprocess.run([os.path.join(REFDIR, "dropin_example_f08vec")] + args, cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.splitlines() == _tables()[key]


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(REFDIR, "dropin_example_f08")), reason="drop-in build absent")
@pytest.mark.parametrize("args,key", CASES[1:])
def test_reference_array_caller_against_our_module_on_gpu(tmp_path, args, key):
    """Reference src-F08/nka_example.F90, unchanged, with OUR module nka_type in
    place of the reference's: every accel_update runs on the MI355X and the
    printed tables equal the compiled reference's."""
    p = subprocess.run([os.path.join(REFDIR, "dropin_example_f08")] + args, cwd=tmp_path, capture_output=True,
                       text=True, timeout=300, env=_ours_env())
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.splitlines() == _tables()[key]


@pytest.mark.gpu
@pytest.mark.parametrize("env_flavor,flavor_name", [(None, "C_FLAVOR"), ("f08", "F08")])
def test_assignment_is_a_deep_copy_like_the_reference_type(fortran_build, oracle, tmp_path, env_flavor, flavor_name):
    """`b = a` of the reference's type copies deeply (allocatable components, F08:154-168).  The
    drop-in module clones the device object: copied in mid-stream (after call 5, a pair pending, a
    user dot product installed), `a` and `b` then follow TWO different input streams and each must
    reproduce its own oracle bit for bit (the user dot product makes the sums bit-identical)."""
    raw = tmp_path / "copy.bin"
    p = subprocess.run([os.path.join(fortran_build, "nka_dp_driver"), "copy", str(raw)], capture_output=True, text=True,
                       timeout=300, env=_env_flavor(env_flavor))
    assert p.returncode == 0, p.stdout + p.stderr
    n, m = 501, 4
    fl = getattr(oracle, flavor_name)
    XA = oracle.lcg_vectors(12, n, seed=1)
    XB = oracle.lcg_vectors(7, n, seed=7)
    a = oracle.OracleNKA(n, m, fl)
    a.set_vec_tol(0.05)
    a.set_dot_prod(_reverse_dot)
    b = oracle.OracleNKA(n, m, fl)        # the oracle has no copy: b replays a's first five calls
    b.set_vec_tol(0.05)
    b.set_dot_prod(_reverse_dot)
    want, rows = [], []
    for t in range(1, 13):
        f = XA[t - 1].copy()
        a.accel_update(f)
        want.append(f.copy())
        if t <= 5:
            g = XA[t - 1].copy()
            b.accel_update(g)
        else:
            g = XB[t - 6].copy()
            b.accel_update(g)
            want.append(g.copy())
            if t == 8:
                b.relax()
            rows.append((-t, b.num_vec()))
        if t == 6:
            a.relax()
        if t == 9:
            a.restart()
        rows.append((t, a.num_vec()))
    got_rows = [(int(ln.split()[0]), int(ln.split()[1])) for ln in p.stdout.splitlines() if ln.strip()]
    assert got_rows == rows
    dev = np.fromfile(raw, dtype=np.float64).reshape(len(want), n)
    assert np.array_equal(dev, np.array(want)), np.abs(dev - np.array(want)).max()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(REFDIR, "dropin_example_c")), reason="drop-in build absent")
def test_reference_c_caller_links_unchanged_against_the_c_drop_in_library(tmp_path):
    """Reference src-C/nka_example.c -- its `#include "nonlinear_krylov_accelerator.h"` and the reference's own
    header untouched -- linked with libnka_c_compat.so (the nine reference symbols over libnka_hip.so) in place of
    nonlinear_krylov_accelerator.c: every nka_accel_update runs on the MI355X and the program prints the
    reference's 403-line reference_output (the accelerated AND the unaccelerated solve) line for line."""
    p = subprocess.run([os.path.join(REFDIR, "dropin_example_c")], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       env=_ours_env())
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    want = open(os.path.join(S.GOLD, "reference_output_C.txt")).read().splitlines()
    got = p.stdout.splitlines()
    assert len(got) == len(want) == 403
    assert got == want


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(REFDIR, "dropin_example_f95")), reason="drop-in build absent")
def test_reference_f95_caller_against_our_f95_module_on_gpu(tmp_path):
    """Reference src-F95/nka_example.F90, unchanged, with OUR procedural module nka_type (nka_init,
    nka_accel_update, nka_delete over libnka_hip.so) in place of the reference's: the program prints
    src-F95/reference_output (byte-identical to src-C/reference_output: SURVEY.md 4), 403 lines."""
    p = subprocess.run([os.path.join(REFDIR, "dropin_example_f95")], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       env=_ours_env())
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    want = open(os.path.join(S.GOLD, "reference_output_C.txt")).read().splitlines()
    got = p.stdout.splitlines()
    assert len(got) == len(want) == 403
    assert got == want


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(REFDIR, "dropin_example_f08")) or
                    not os.path.exists(os.path.join(REFDIR, "nka_example_f08")), reason="drop-in / reference build absent")
@pytest.mark.parametrize("args", [["-n", "120", "--nka-vec", "8", "--sweeps", "3"], ["-n", "33", "--nka-vec", "12"],
                                  ["-n", "200", "--nka-vec", "3", "--omega", "1.2"], ["-a", "0.1", "--nka-vec", "20"]])
def test_reference_array_caller_at_other_problem_sizes_against_the_compiled_reference(tmp_path, args):
    """Beyond the three published tables: the reference's unchanged src-F08/nka_example.F90 linked with OUR module
    (every accel_update on the MI355X) against the SAME program linked with the reference's own nka_type (CPU), at
    other grids, subspace sizes and parameters: the same number of iterations, and every printed figure (residual
    norm to 7 digits, reduction, rate) equal to within one unit of its last printed digit (a long run does pass
    through values like 6.9125005 whose seventh digit a difference in the sixteenth decides)."""
    ours = subprocess.run([os.path.join(REFDIR, "dropin_example_f08")] + args, cwd=tmp_path, capture_output=True, text=True,
                          timeout=600, env=_ours_env())
    ref = subprocess.run([os.path.join(REFDIR, "nka_example_f08")] + args, cwd=tmp_path, capture_output=True, text=True,
                         timeout=600)
    assert ours.returncode == 0 and ref.returncode == 0, ours.stdout[-500:] + ours.stderr + ref.stderr
    a, b = ours.stdout.splitlines(), ref.stdout.splitlines()
    assert len(b) > 10 and len(a) == len(b)

    def rows(lines):
        out = []
        for ln in lines:
            t = ln.replace(":", " ").split()
            out.append([float(v) for v in t] if len(t) == 4 and t[0].isdigit() else None)
        return out

    # A slowly converging run amplifies last-bit differences (at -n 200 --nka-vec 3, 934 iterations, the reference's
    # OWN two Fortran flavours print different last digits in 453 lines, up to 1e-5 relative).  So the yardstick is the
    # reference itself: the same program with the reference's src-F08-vector module.  This build must stay at least as
    # close to src-F08 as that -- in how many lines differ and in how far -- with one unit of the last printed digit as
    # the floor.
    ra, rb = rows(a), rows(b)
    vec = os.path.join(REFDIR, "nka_example_f08vec")
    allowed_lines, allowed_rel = 2, 0.0
    if os.path.exists(vec):
        rv = subprocess.run([vec] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        lv = rv.stdout.splitlines()
        if rv.returncode == 0 and len(lv) == len(b):
            allowed_lines = max(allowed_lines, sum(1 for x, y in zip(lv, b) if x != y))
            allowed_rel = max([abs(x[1] - y[1]) / y[1] for x, y in zip(rows(lv), rb) if x and y and y[1] > 0] + [0.0])
    ndiff = 0
    for la, lb, x, y in zip(a, b, ra, rb):
        if la == lb:
            continue
        ndiff += 1
        assert x and y and x[0] == y[0], (la, lb)
        unit = 1.001 * 10.0 ** (np.floor(np.log10(y[1])) - 6)             # one unit of the 7th significant digit
        assert abs(x[1] - y[1]) <= max(unit, allowed_rel * y[1]), (la, lb, allowed_rel)
        assert abs(x[3] - y[3]) <= 1.001e-3, (la, lb)
    assert ndiff <= allowed_lines, (ndiff, allowed_lines, len(b))
