"""The narrow batch's scalar step on one wavefront (nka_hip_batch_create_rows with nka_hip_batch_set_scalar_step;
include/nka_hip_batch.h, NARROW ROWS; phase 4 of k_batch_update, nka_amd/csrc/nka_batch_kernel.hpp, the instances of
nka_amd/csrc/nka_batch_rows.hip).  The contract is bit equality with the one-thread step, debris included.

  1 the twin        two batches of the new entry on the same inputs, one left at the default, one with SCALAR_WAVEFRONT, compared
                    with == after EVERY call (test_batch_wide_rows_gpu._twin): the rows of F (and X), red[], get_state (all of h,
                    c, next, prev, the five scalars), num_vec, the digest (the counters), fnorm, the mask; at the end w and v of
                    every slot.  batch_wide_rows.script drives them through the drop logic, and a CENSUS counted on the one-thread
                    twin's states says that it did: the test fails if the census is short.
  2 the other packs the same with a weight row per system and a shared one, with lengths 1, 64, 65 and vlen, through accel_step
                    with a system retiring, with all three together, and with binary32 storage (plain, and with step + lengths)
  3 the oracle      the three layers of BatchRun (tests/test_batch_sums_exact_gpu.py) with the wavefront step on: independent of
                    the one-thread instances
  4 switching       a batch that alternates the setting on every call; graphs captured with either step
  5 the surface     who offers it, both NKA_HIP_ESTATE refusals in both directions, what creation refuses, the limits
  6 independence    the bits of a system depend on its own values alone

vlen 65 (the smallest length NKA_HIP_SUMS_AUTO runs in the fast sums; one ragged tile), 513 (one full tile and one element), 1025
(two and one); mvec on both sides of every NLMAX edge (11 / 21 / 33 rows) and at the largest."""
import ctypes as C

import numpy as np
import pytest

import batch_rows as NR
import batch_seq as B
import batch_wide_rows as R
import exact_sums as X
import test_batch_sums_exact_gpu as T
import test_batch_wide_rows_gpu as TR

pytestmark = pytest.mark.gpu

_eq, _twin, _mask = TR._eq, TR._twin, TR.TW._mask
EINVAL, ESTATE = -1, -5      # NKA_HIP_EINVAL, NKA_HIP_ESTATE (include/nka_hip.h)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _rows_batch(nsys, vlen, mvec, flavor=2, storage=0):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, narrow_rows=True, storage=storage)
    assert b.kind() == nka_amd.KIND_NARROW and b.offers_scalar_step() and b.scalar_step() == nka_amd.SCALAR_ONE_THREAD
    assert b.offers_lengths() and b.offers_weights() and b.offers_step() and b.storage() == storage
    return b


# ---- 1. the twin ---------------------------------------------------------------------------------------------------------------------

def _twin_case(torch, vlen, mvec, flavor):
    census = _twin(torch, lambda: _rows_batch(NR.NSYS, vlen, mvec, flavor), [vlen] * NR.NSYS, vlen, mvec, seed=NR.twin_seed(mvec, flavor))
    print(f"census of the one-thread twin, vlen {vlen}, mvec {mvec}, flavour {flavor}: {sorted(census.items())}")
    if mvec >= 2:
        assert not R.census_short(census), (vlen, mvec, flavor, "the census is short", census)


@pytest.mark.parametrize("vlen", NR.VLENS)
@pytest.mark.parametrize("mvec", NR.MVECS)
def test_the_wavefront_step_is_the_one_thread_step_bit_for_bit(torch_cuda, mvec, vlen):
    """Eight systems with staggered starts over mvec + 15 calls in the default flavour: lists filled under a tiny vtol and then
    several dependence drops in one update, at the first older position and at the last, capacity drops, the last position of
    a full list evaluated behind a drop, s == 0, masked relax and restart, the path without a new pair, one system fed NaN and
    Inf."""
    _twin_case(torch_cuda, vlen, mvec, 2)


@pytest.mark.parametrize("flavor", [0, 1])
@pytest.mark.parametrize("mvec", [10, 20])
def test_the_wavefront_step_in_the_other_flavours(torch_cuda, mvec, flavor):
    _twin_case(torch_cuda, NR.FLAVOR_VLEN, mvec, flavor)


# ---- 2. the other packs --------------------------------------------------------------------------------------------------------------

PACKS = ["weights", "shared weights", "lengths", "step", "weights lengths step", "f32", "f32 lengths step"]


@pytest.mark.parametrize("pack", PACKS)
def test_the_twin_in_every_other_pack(torch_cuda, pack):
    """The WGT instances with a row per system and with the shared row, the LEN instances with lengths 1, 64, 65 and vlen, the
    STEP instances (x, mask, tol and fnorm; system 3 retires in the middle of the sequence), all three at once, and the binary32
    instances plain and with step + lengths."""
    import nka_amd
    vlen, mvec = NR.PACK_VLEN, NR.PACK_MVEC
    lens = list(NR.PACK_LENS) if "lengths" in pack else [vlen] * NR.NSYS
    assert len(lens) == NR.NSYS and {1, 64, 65, vlen} <= set(NR.PACK_LENS) and max(lens) == vlen
    rng = np.random.default_rng(3)
    wgt = rng.uniform(0.5, 1.5, vlen) if "shared" in pack else rng.uniform(0.5, 1.5, (NR.NSYS, vlen))
    storage = nka_amd.STORE_F32 if "f32" in pack else nka_amd.STORE_F64

    def prepare(b):
        if "lengths" in pack:
            b.set_lengths(lens)
        if "weights" in pack:
            b.set_dot_weights(wgt)
        assert b.has_lengths() == ("lengths" in pack) and b.dot_weighted() == ("weights" in pack)
    census = _twin(torch_cuda, lambda: _rows_batch(NR.NSYS, vlen, mvec, storage=storage), lens, vlen, mvec, seed=NR.twin_seed(mvec, 2),
                   step="step" in pack, prepare=prepare)
    print(f"census of the one-thread twin, pack '{pack}': {sorted(census.items())}")
    assert census.get("capacity", 0) >= 1 and census.get("no_new_pair", 0) >= 1, census


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------------

class RowsRun(T.BatchRun):
    """BatchRun on a batch of the new entry with the wavefront step on: the sums against exact_dot, the device's own red[] through
    the oracle's scalar_step with == on lists, h and c, the elementwise statements bit for bit."""

    def _device(self, odd_ld):
        import nka_amd
        super()._device(odd_ld)
        self.b = _rows_batch(self.nsys, self.n, self.m, self.flavor).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        self.b.set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        assert self.b.scalar_step() == nka_amd.SCALAR_WAVEFRONT and self.b.flavor() == self.flavor


@pytest.mark.parametrize("n", [65, 513])
@pytest.mark.parametrize("mvec", [10, 21, 32])
def test_the_wavefront_step_against_the_oracle(torch_cuda, oracle, mvec, n):
    if mvec == T.SHAPE_MVEC:      # six systems of different list length: a repeated input, a masked relax and a masked restart each
        run = T._planned_run(RowsRun(torch_cuda, oracle, 2, n, mvec, len(T.PLAN), odd_ld=True), seed=n)
        T._assert_planned_coverage(run)
    else:                         # every older count up to mvec, system k starting k % 3 calls late
        run = RowsRun(torch_cuda, oracle, 2, n, mvec, 5, odd_ld=True)
        rngs, prev = [np.random.default_rng([mvec, n, k]) for k in range(run.nsys)], [None] * run.nsys
        for t in range(mvec + 4):
            inputs = {}
            for k in range(run.nsys):
                if t >= k % 3:
                    inputs[k] = prev[k] = X.batch_planted_input(n, rngs[k], prev[k])
            run.update(inputs)
        assert run.widest == mvec and run.lengths_differed


# ---- 4. switching and graphs ---------------------------------------------------------------------------------------------------------

def test_alternating_the_setting_on_every_call_changes_nothing(torch_cuda):
    vlen, mvec = 513, 5
    census = _twin(torch_cuda, lambda: _rows_batch(NR.NSYS, vlen, mvec), [vlen] * NR.NSYS, vlen, mvec, seed=NR.twin_seed(mvec, 2),
                   setting=lambda t: t % 2)
    assert not R.census_short(census), census


@pytest.mark.parametrize("captured", ["wavefront", "one-thread"])
def test_a_captured_call_keeps_the_step_it_was_captured_with(torch_cuda, captured):
    """Captured BEFORE the first update and replayed 40 times through growth, dependence and capacity drops (batch_seq.Sequence),
    masks, two masked relax and a masked restart, against an eager twin of nka_hip_batch_create.  After the capture the setter is
    called with the OTHER value: the replays stay what they were captured as (both leave the same bits, and the replay must not
    fail on a launch whose LDS size belongs to the other step)."""
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = 9, 129, 5
    how = nka_amd.SCALAR_WAVEFRONT if captured == "wavefront" else nka_amd.SCALAR_ONE_THREAD
    seqs = [B.Sequence(vlen, 700 + k) for k in range(nsys)]
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = _rows_batch(nsys, vlen, mvec)
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b.set_scalar_step(how)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.set_scalar_step(how)      # (legal during capture: enqueue-side state only)
        b.accel_update(static, mask)
    b.set_scalar_step(1 - how)
    assert b.scalar_step() == 1 - how
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec)
    full = False
    for t in range(40):
        Xh = np.stack([s.next() for s in seqs])
        m = (rng.random(nsys) < 0.8).astype(np.int32)
        if t in (9, 20):
            rm = _mask(torch, nsys, [1, 4, 6])
            with torch.cuda.stream(side):
                b.relax(rm)
            eager.relax(rm)
        if t == 30:
            rm = _mask(torch, nsys, [0, 5])
            with torch.cuda.stream(side):
                b.restart(rm)
            eager.restart(rm)
        static.copy_(torch.from_numpy(Xh))
        mask.copy_(torch.from_numpy(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = torch.from_numpy(Xh.copy()).cuda()
        eager.accel_update(F, torch.from_numpy(m).cuda())
        assert torch.equal(F, static), t
        assert np.array_equal(b.num_vec(), eager.num_vec()), t
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], t
        full = full or bool((b.num_vec() == mvec).any())
    assert full      # a full list: capacity drops from there on


# ---- 5. the surface ------------------------------------------------------------------------------------------------------------------

def test_who_offers_the_scalar_step_and_what_is_refused(torch_cuda):
    import nka_amd
    from nka_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    nsys, vlen, mvec = 3, 129, 4
    rng = np.random.default_rng(12)
    for storage in (nka_amd.STORE_F64, nka_amd.STORE_F32):
        b = _rows_batch(nsys, vlen, mvec, storage=storage)
        twin = nka_amd.nka_batch().init(nsys, vlen, mvec, storage=storage)
        assert L.nka_hip_batch_offers_scalar_step(b._handle()) == 1 and L.nka_hip_batch_kind(b._handle()) == 0
        assert b.vector_bytes() == twin.vector_bytes() and not b.is_wide()
        assert b.set_scalar_step(nka_amd.SCALAR_WAVEFRONT) is b and b.scalar_step() == nka_amd.SCALAR_WAVEFRONT
        for bad in (2, -1, 17):
            assert L.nka_hip_batch_set_scalar_step(b._handle(), bad) == EINVAL and L.nka_hip_last_error(), (storage, bad)
            with pytest.raises(nka_amd.NKAError):
                b.set_scalar_step(bad)
            assert b.scalar_step() == nka_amd.SCALAR_WAVEFRONT, (storage, bad)
        b.set_scalar_step(nka_amd.SCALAR_ONE_THREAD).set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        F, Ft = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
        for _ in range(mvec + 3):
            x = rng.standard_normal((nsys, vlen))
            F.copy_(torch.from_numpy(x))
            Ft.copy_(torch.from_numpy(x))
            b.accel_update(F)
            twin.accel_update(Ft)
            assert torch.equal(F, Ft), storage
        assert [b.state_digest(k) for k in range(nsys)] == [twin.state_digest(k) for k in range(nsys)], storage
    # batches of the older entries behave as they did: the narrow ones refuse, with "wide" in the sentence, which now names the new entry too
    others = {"create": (vlen, {}), "create_stored": (vlen, dict(storage=nka_amd.STORE_F32)), "lanes": (33, dict(lanes=True)),
              "waves": (65, dict(waves=True))}
    for name, (n, kw) in others.items():
        o = nka_amd.nka_batch().init(nsys, n, mvec, **kw)
        assert not o.offers_scalar_step() and L.nka_hip_batch_offers_scalar_step(o._handle()) == 0, name
        assert L.nka_hip_batch_set_scalar_step(o._handle(), nka_amd.SCALAR_WAVEFRONT) == EINVAL, name
        err = L.nka_hip_last_error()
        assert b"wide" in err and b"nka_hip_batch_create_rows" in err and b"nka_hip_batch_create_waves_rows" in err, (name, err)
        assert o.set_scalar_step(nka_amd.SCALAR_ONE_THREAD) is o and o.scalar_step() == nka_amd.SCALAR_ONE_THREAD, name
    assert nka_amd.nka_batch().init(nsys, 4096, mvec, wide=True).offers_scalar_step()
    assert nka_amd.nka_batch().init(nsys, 65, mvec, waves=True, rows=True).offers_scalar_step()


def test_the_wavefront_step_and_the_reference_order_refuse_each_other(torch_cuda):
    """NKA_HIP_ESTATE in both directions, the batch staying usable and both settings unchanged; each message names the other
    setter and nka_hip_batch_create_waves_rows.  Nothing is downgraded."""
    import nka_amd
    from nka_amd import _lib
    L = _lib.load()
    W, ONE = nka_amd.SCALAR_WAVEFRONT, nka_amd.SCALAR_ONE_THREAD
    # an explicit reference order, then the setter
    b = _rows_batch(2, 129, 3).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    assert L.nka_hip_batch_set_scalar_step(b._handle(), W) == ESTATE
    err = L.nka_hip_last_error()
    assert b"nka_hip_batch_set_sum_order" in err and b"nka_hip_batch_create_waves_rows" in err, err
    with pytest.raises(nka_amd.NKAError):
        b.set_scalar_step(W)
    assert b.scalar_step() == ONE
    b.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED).set_scalar_step(W)
    assert b.scalar_step() == W
    # AUTO at vlen = 64 means the reference order; at 65 the fast sums
    s = _rows_batch(2, NR.AUTO_ORDERED_MAX, 3)
    assert L.nka_hip_batch_set_scalar_step(s._handle(), W) == ESTATE and b"nka_hip_batch_set_sum_order" in L.nka_hip_last_error()
    assert s.scalar_step() == ONE
    s.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED).set_scalar_step(W)
    assert _rows_batch(2, NR.AUTO_ORDERED_MAX + 1, 3).set_scalar_step(W).scalar_step() == W
    # the wavefront step, then the order: explicit reference order, and AUTO where it would mean it
    for batch, order in ((b, nka_amd.SUMS_REFERENCE_ORDER), (s, nka_amd.SUMS_REFERENCE_ORDER), (s, nka_amd.SUMS_AUTO)):
        assert L.nka_hip_batch_set_sum_order(batch._handle(), order) == ESTATE
        err = L.nka_hip_last_error()
        assert b"nka_hip_batch_set_scalar_step" in err and b"nka_hip_batch_create_waves_rows" in err, err
        with pytest.raises(nka_amd.NKAError):
            batch.set_sum_order(order)
        assert batch.scalar_step() == W
    b.set_sum_order(nka_amd.SUMS_AUTO)      # (vlen 129: the fast sums)
    b.set_scalar_step(ONE).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    s.set_scalar_step(ONE).set_sum_order(nka_amd.SUMS_AUTO)
    # still usable, and still what the setters say: the short batch runs the reference order on one thread
    import torch
    F = torch.from_numpy(np.random.default_rng(1).standard_normal((2, NR.AUTO_ORDERED_MAX))).cuda()
    s.accel_update(F)
    s.accel_update(F)
    assert bool(torch.isfinite(F).all())
    # binary32 storage always runs the fast sums: the setter is accepted at vlen <= 64, the reference order stays EINVAL
    q = _rows_batch(2, 33, 3, storage=nka_amd.STORE_F32).set_scalar_step(W)
    assert L.nka_hip_batch_set_sum_order(q._handle(), nka_amd.SUMS_REFERENCE_ORDER) == EINVAL
    q.set_sum_order(nka_amd.SUMS_AUTO)
    assert q.scalar_step() == W
    q.accel_update(torch.from_numpy(np.random.default_rng(2).standard_normal((2, 33))).cuda())


def test_what_creation_refuses_and_the_limits(torch_cuda):
    """Refused before anything is allocated, with the new entry's name in the message, and no handle comes back."""
    import nka_amd
    from nka_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    F64, F32 = nka_amd.STORE_F64, nka_amd.STORE_F32
    cases = ((4, 129, 3, 0.01, 2, 2, b"storage"), (4, 129, 3, 0.01, 2, -1, b"storage"), (4, 129, 3, 0.01, 0, F32, b"binary32"),
             (4, 129, 3, 0.01, 1, F32, b"binary32"), (0, 129, 3, 0.01, 2, F64, b"nsys"), (4, 0, 3, 0.01, 2, F64, b"vlen"),
             (4, nka_amd.BATCH_MAX_VLEN + 1, 3, 0.01, 2, F32, b"vlen"), (4, 129, 0, 0.01, 2, F64, b"mvec"),
             (4, 129, nka_amd.BATCH_MAX_MVEC + 1, 0.01, 2, F64, b"mvec"), (4, 129, 3, 0.0, 2, F64, b"vtol"), (4, 129, 3, -1.0, 2, F32, b"vtol"))
    for nsys, vlen, mvec, vtol, flavor, storage, word in cases:
        h.value = 1
        assert L.nka_hip_batch_create_rows(C.byref(h), nsys, vlen, mvec, vtol, flavor, 0, None, storage) == EINVAL and h.value is None
        err = L.nka_hip_last_error()
        assert b"nka_hip_batch_create_rows" in err and word in err, (err, word)
    assert L.nka_hip_batch_create_rows(None, 4, 129, 3, 0.01, 0, 0, None, F64) == EINVAL
    for kw in ({"wide": True}, {"lanes": True}, {"waves": True}):
        with pytest.raises(nka_amd.NKAError):
            nka_amd.nka_batch().init(4, 64, 3, narrow_rows=True, **kw)
    assert _rows_batch(2, nka_amd.BATCH_MAX_VLEN, nka_amd.BATCH_MAX_MVEC).max_vec() == nka_amd.BATCH_MAX_MVEC      # no new cap
    lds = C.c_int64()
    for mvec in range(1, nka_amd.BATCH_MAX_MVEC + 1):
        assert L.nka_hip_batch_rows_limits(mvec, C.byref(lds)) == 0 and lds.value == NR.lds_bytes(mvec) == nka_amd.batch_rows_limits(mvec)
    assert L.nka_hip_batch_offers_scalar_step(None) < 0 and L.nka_hip_batch_scalar_step(None) < 0 and L.nka_hip_batch_set_scalar_step(None, 1) < 0


# ---- 6. independence -----------------------------------------------------------------------------------------------------------------

def _run_at(torch, vlen, mvec, inputs, nsys, pos, active_others, how):
    """System `pos` of a batch of nsys runs `inputs`; the systems of `active_others` run data of their own, the rest sit out."""
    b = _rows_batch(nsys, vlen, mvec).set_scalar_step(how)
    rng = np.random.default_rng(5 + 11 * nsys + pos)
    F = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    active = sorted(set(active_others) | {pos})
    mask = None if len(active) == nsys else _mask(torch, nsys, active)
    outs = []
    for x in inputs:
        Xh = rng.standard_normal((nsys, vlen))
        Xh[pos] = x
        F.copy_(torch.from_numpy(Xh))
        b.accel_update(F, mask)
        outs.append(F[pos].cpu().numpy())
    st = b.state(pos)
    return outs, b.state_digest(pos), b.reductions(pos), st.h, st.c


def test_results_depend_on_the_systems_own_values_alone(torch_cuda):
    """The wavefront step at nsys 1 and 6, at every position, under four masks of the others: the bits of the one-thread step of a
    batch of one.  The inputs drop by dependence and by capacity (batch_seq.Sequence)."""
    import nka_amd
    vlen, mvec = 129, 5
    seq = B.Sequence(vlen, 79)
    inputs = [seq.next() for _ in range(2 * mvec + 6)]
    base = _run_at(torch_cuda, vlen, mvec, inputs, 1, 0, [], nka_amd.SCALAR_ONE_THREAD)
    runs = [(1, 0, ())]
    for pos in range(6):
        rest = [q for q in range(6) if q != pos]
        runs += [(6, pos, tuple(rest)), (6, pos, ()), (6, pos, tuple(rest[::2])), (6, pos, tuple(rest[1::2]))]
    for nsys, pos, others in runs:
        outs, dig, red, h, c = _run_at(torch_cuda, vlen, mvec, inputs, nsys, pos, others, nka_amd.SCALAR_WAVEFRONT)
        where = (nsys, pos, others)
        assert dig == base[1] and _eq(red, base[2]) and _eq(h, base[3]) and _eq(c, base[4]), where
        assert all(_eq(a, c0) for a, c0 in zip(outs, base[0])), where
