"""The wide batch's scalar step on one wavefront (nka_hip_batch_set_scalar_step; include/nka_hip_batch.h, SCALAR STEP;
batch_scalar_step_rows of nka_amd/csrc/nka_batch_dev.hpp).  The contract is bit equality with the one-thread step, debris included.

  1 the twin        two wide batches on the same inputs, one per step, compared with == after EVERY call: the rows of F (and X),
                    red[], get_state (all of h, c, next, prev, the five scalars), num_vec, the digest, fnorm, the mask; at the end w
                    and v of every slot.  batch_wide_rows.script drives them through the drop logic, and a CENSUS counted on the
                    one-thread twin's states says that it did: the test fails if the census is short.
  2 every pack      the same through create_wide_step (x, mask, tol, fnorm, a system retiring), create_wide_ext (lengths with
                    partial counts 1, 2, 9 and weights) and create_wide_stored (binary32 storage, step, lengths)
  3 the oracle      the three layers of WideRun (tests/test_batch_wide_gpu.py) with the wavefront step on: independent of the
                    one-thread kernel
  4 switching       a batch that alternates the setting on every call; graphs captured with either step
  5 the surface     who offers it, what is refused, and that results depend on the system's own values alone

The scalar step does not depend on vlen beyond the chunk count: 65 (one chunk), C + 1 (two), 8C + 1 (nine: the unrolled chain)."""
import ctypes as C

import numpy as np
import pytest

import batch_seq as B
import batch_wide as BW
import batch_wide_rows as R
import test_batch_sums_exact_gpu as T
import test_batch_wide_gpu as TW

pytestmark = pytest.mark.gpu

PAD = 7.0      # what lies in a row beyond the system's own length


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def CH():
    return BW.limits()


def _vlen(which, c):
    return {"65": 65, "C+1": c + 1, "8C+1": 8 * c + 1}[which]


def _eq(a, b):
    """== on doubles bit for bit, NaN payloads included."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same_state(one, wav, k, where):
    so, sw = one.state(k), wav.state(k)
    assert (so.subspace, so.pending, so.first, so.last, so.free) == (sw.subspace, sw.pending, sw.first, sw.last, sw.free), (where, "scalars")
    assert np.array_equal(so.next, sw.next) and np.array_equal(so.prev, sw.prev), (where, "links")
    assert _eq(so.h, sw.h), (where, "h", np.argwhere(so.h.view(np.int64) != sw.h.view(np.int64)).tolist(), so.list_order())
    assert _eq(so.c, sw.c), (where, "c", so.c, sw.c)
    assert _eq(one.reductions(k), wav.reductions(k)), (where, "red[]")
    assert one.state_digest(k) == wav.state_digest(k), (where, "digest")
    return so


def _twin(torch, make, lens, vlen, mvec, seed, *, step=False, setting=lambda t: 1, prepare=None):
    """`one` never hears of the setter; `wav` runs setting(t) at call t.  -> the census of the one-thread twin."""
    import nka_amd
    nsys = len(lens)
    one, wav = make(), make()
    assert wav.offers_scalar_step() and wav.scalar_step() == nka_amd.SCALAR_ONE_THREAD
    for b in (one, wav):
        if prepare is not None:
            prepare(b)
    Fo, Fw = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
    Xo, Xw = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
    no, nw = (torch.zeros(nsys, dtype=torch.float64, device="cuda") for _ in range(2))
    host = np.full((nsys, vlen), PAD)
    xhost = np.random.default_rng(seed).standard_normal((nsys, vlen))
    census, met_nonfinite = {}, False
    for t, ev in enumerate(R.script(lens, mvec, seed)):
        how = setting(t)
        wav.set_scalar_step(how)
        assert wav.scalar_step() == how and one.scalar_step() == nka_amd.SCALAR_ONE_THREAD
        for b in (one, wav):
            if ev["vtol"] is not None:
                b.set_vec_tol(ev["vtol"])
            if ev["relax"]:
                b.relax(TW._mask(torch, nsys, ev["relax"]))
            if ev["restart"]:
                b.restart(TW._mask(torch, nsys, ev["restart"]))
        for k, x in ev["inputs"].items():
            host[k, :lens[k]] = x
        live = sorted(ev["inputs"])
        before = {k: one.state(k) for k in live}
        mo, mw = TW._mask(torch, nsys, live), TW._mask(torch, nsys, live)
        tol = np.zeros(nsys)
        tol[ev["retire"]] = 1e300
        for b, F, X, m, fn in ((one, Fo, Xo, mo, no), (wav, Fw, Xw, mw, nw)):
            F.copy_(torch.from_numpy(host))
            if step:
                X.copy_(torch.from_numpy(xhost))
                b.accel_step(F, X, m, torch.from_numpy(tol).cuda(), fn)
            else:
                b.accel_update(F, m)
        where = (vlen, mvec, "call", t)
        assert _eq(Fo.cpu().numpy(), Fw.cpu().numpy()), (where, "rows of F")
        retired = []
        if step:
            assert _eq(Xo.cpu().numpy(), Xw.cpu().numpy()), (where, "rows of X")
            assert _eq(no.cpu().numpy()[live], nw.cpu().numpy()[live]), (where, "fnorm")
            assert torch.equal(mo, mw), (where, "the mask")
            retired = [k for k in live if int(mo[k]) == 0]
            assert retired == [k for k in ev["retire"] if k in live], (where, "who retired", retired)
            xhost = Xo.cpu().numpy()
        assert np.array_equal(one.num_vec(), wav.num_vec()), (where, "num_vec")
        for k in range(nsys):
            after = _same_state(one, wav, k, where + ("system", k))
            if k in live and k not in retired:
                for tag in R.census_of(before[k], after, mvec):
                    census[tag] = census.get(tag, 0) + 1
        met_nonfinite = met_nonfinite or not np.isfinite(one.reductions(nsys - 1)).all()
    for k in range(nsys):
        for s in range(1, mvec + 2):
            assert _eq(one.w(k, s), wav.w(k, s)) and _eq(one.v(k, s), wav.v(k, s)), (vlen, mvec, "system", k, "slot", s)
    assert met_nonfinite, "the system fed NaN and Inf never showed them in its sums"
    return census


# ---- 1. the twin ---------------------------------------------------------------------------------------------------------------------

def _twin_case(torch, c, which, mvec, flavor):
    import nka_amd
    vlen = _vlen(which, c)
    census = _twin(torch, lambda: nka_amd.nka_batch().init(R.NSYS, vlen, mvec, flavor=flavor, wide=True), [vlen] * R.NSYS, vlen, mvec,
                   seed=R.twin_seed(mvec, flavor))
    print(f"census of the one-thread twin, vlen {which}, mvec {mvec}, flavour {flavor}: {sorted(census.items())}")
    if mvec >= 2:
        assert not R.census_short(census), (which, mvec, flavor, "the census is short", census)


@pytest.mark.parametrize("which", ["65", "C+1", "8C+1"])
@pytest.mark.parametrize("mvec", R.MVECS)
def test_the_wavefront_step_is_the_one_thread_step_bit_for_bit(torch_cuda, CH, mvec, which):
    """Eight systems with staggered starts over mvec + 15 calls in the default flavour: lists filled under a tiny vtol and then
    several dependence drops in one update, at the first older position and at the last, capacity drops, the last position of
    a full list evaluated behind a drop, s == 0, masked relax and restart, the path without a new pair, one system fed NaN and
    Inf.  Worst census measured on the MI355X over the grid (the smallest count of any tag at mvec >= 2): 1 at mvec 2 ('two_dep' and
    'last_evaluated'), 4 from mvec 5 on ('dep_first', 'relax_s0'); the counts are those of the oracle in tests/test_batch_wide_rows_cpu.py."""
    _twin_case(torch_cuda, CH[0], which, mvec, 2)


@pytest.mark.parametrize("flavor", [0, 1])
@pytest.mark.parametrize("mvec", [10, 20])
def test_the_wavefront_step_in_the_other_flavours(torch_cuda, CH, mvec, flavor):
    _twin_case(torch_cuda, CH[0], "C+1", mvec, flavor)


# ---- 2. every pack -------------------------------------------------------------------------------------------------------------------

def test_the_twin_through_the_solve_step(torch_cuda, CH):
    """create_wide_step: x, mask, tol and fnorm, system 3 retiring in the middle of the sequence (the STEP instance)."""
    import nka_amd
    vlen, mvec = CH[0] + 1, 11
    _twin(torch_cuda, lambda: nka_amd.nka_batch().init(R.NSYS, vlen, mvec, wide=True, step=True), [vlen] * R.NSYS, vlen, mvec, seed=2, step=True)


def test_the_twin_with_lengths_and_weights(torch_cuda, CH):
    """create_wide_ext: systems of 1, 2 and 9 chunks in one batch of 9, and a weight row per system (the LEN instance; the scalar
    launch takes no weights)."""
    import nka_amd
    c = CH[0]
    vlen, mvec = 8 * c + 1, 10
    lens = [8 * c + 1, c, c + 1, 65, 2 * c, 8 * c + 1, c + 1, 513]
    assert sorted({BW.nchunk(n, c) for n in lens}) == [1, 2, 9]
    wgt = np.random.default_rng(3).uniform(0.5, 1.5, (R.NSYS, vlen))

    def prepare(b):
        b.set_lengths(lens).set_dot_weights(wgt)
        assert b.has_lengths() and b.dot_weighted()
    _twin(torch_cuda, lambda: nka_amd.nka_batch().init(R.NSYS, vlen, mvec, wide=True, ext=True), lens, vlen, mvec, seed=3, prepare=prepare)


def test_the_twin_with_binary32_storage_step_and_lengths(torch_cuda, CH):
    """create_wide_stored with NKA_HIP_BATCH_STORE_F32 and the step, lengths set (the STEP + LEN instance; the scalar launch takes
    no storage member)."""
    import nka_amd
    c = CH[0]
    vlen, mvec = c + 1, 21
    lens = [c + 1, c, 65, c + 1, 513, c + 1, 1000, c + 1]

    def prepare(b):
        b.set_lengths(lens)
        assert b.storage() == nka_amd.STORE_F32
    _twin(torch_cuda, lambda: nka_amd.nka_batch().init(R.NSYS, vlen, mvec, wide=True, step=True, wide_storage=nka_amd.STORE_F32), lens, vlen,
          mvec, seed=4, step=True, prepare=prepare)


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------------

class WideRowsRun(TW.WideRun):
    """WideRun with the wavefront step on: the device's own red[] goes to the oracle's scalar_step; lists, h and c with ==; the
    elementwise statements bit for bit."""

    def _device(self, odd_ld):
        import nka_amd
        super()._device(odd_ld)
        self.b.set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        assert self.b.scalar_step() == nka_amd.SCALAR_WAVEFRONT


@pytest.mark.parametrize("which", ["C+1", "8C+1"])
@pytest.mark.parametrize("mvec", [10, 21, 32])
def test_the_wavefront_step_against_the_oracle(torch_cuda, oracle, CH, mvec, which):
    n = _vlen(which, CH[0])
    if mvec == T.SHAPE_MVEC:      # six systems of different list length: a repeated input, a masked relax and a masked restart each
        run = TW._planned_run(WideRowsRun(torch_cuda, oracle, 2, n, mvec, len(T.PLAN), odd_ld=True), seed=n)
        T._assert_planned_coverage(run)
    else:                         # every older count up to mvec, the second system one call late
        run = TW._late_second_system(WideRowsRun(torch_cuda, oracle, 2, n, mvec, 2, odd_ld=True), mvec + 2, seed=mvec)
        assert run.widest == mvec


# ---- 4. switching and graphs ---------------------------------------------------------------------------------------------------------

def test_alternating_the_setting_on_every_call_changes_nothing(torch_cuda, CH):
    import nka_amd
    vlen, mvec = CH[0] + 1, 5
    census = _twin(torch_cuda, lambda: nka_amd.nka_batch().init(R.NSYS, vlen, mvec, wide=True), [vlen] * R.NSYS, vlen, mvec, seed=5,
                   setting=lambda t: t % 2)
    assert not R.census_short(census), census


@pytest.mark.parametrize("captured", ["wavefront", "one-thread"])
def test_a_captured_call_keeps_the_step_it_was_captured_with(torch_cuda, CH, captured):
    """Captured BEFORE the first update and replayed 40 times through growth, dependence and capacity drops (batch_seq.Sequence),
    masks, two masked relax and a masked restart, against an eager one-thread twin.  After the capture the setter is called
    with the OTHER value: the replays stay what they were captured as (both leave the same bits, and the replay must not
    fail or fault on a launch whose LDS size belongs to the other step)."""
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = 8, CH[0] + 1, 5
    how = nka_amd.SCALAR_WAVEFRONT if captured == "wavefront" else nka_amd.SCALAR_ONE_THREAD
    seqs = [B.Sequence(vlen, 700 + k) for k in range(nsys)]
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b.set_scalar_step(how)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.accel_update(static, mask)
    b.set_scalar_step(1 - how)
    assert b.scalar_step() == 1 - how
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    full = False
    for t in range(40):
        Xh = np.stack([s.next() for s in seqs])
        m = (rng.random(nsys) < 0.8).astype(np.int32)
        if t in (9, 20):
            rm = TW._mask(torch, nsys, [1, 4, 6])
            with torch.cuda.stream(side):
                b.relax(rm)
            eager.relax(rm)
        if t == 30:
            rm = TW._mask(torch, nsys, [0, 5])
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

def test_who_offers_the_scalar_step_and_what_is_refused(torch_cuda, CH):
    import nka_amd
    from nka_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    EINVAL = -1
    nsys, vlen, mvec = 3, CH[0] + 33, 4
    wides = {"wide": dict(wide=True), "wide step": dict(wide=True, step=True), "wide ext": dict(wide=True, ext=True),
             "wide ext step": dict(wide=True, ext=True, step=True), "wide stored": dict(wide=True, wide_storage=nka_amd.STORE_F32),
             "wide stored step": dict(wide=True, step=True, wide_storage=nka_amd.STORE_F32)}
    others = {"narrow": (vlen, {}), "lanes": (33, dict(lanes=True)), "waves": (65, dict(waves=True)), "waves ext": (65, dict(waves=True, ext=True))}
    rng = np.random.default_rng(12)
    for name, kw in wides.items():
        b, twin = nka_amd.nka_batch().init(nsys, vlen, mvec, **kw), nka_amd.nka_batch().init(nsys, vlen, mvec, **kw)
        assert b.offers_scalar_step() and L.nka_hip_batch_offers_scalar_step(b._handle()) == 1, name
        assert b.scalar_step() == nka_amd.SCALAR_ONE_THREAD, name
        assert b.set_scalar_step(nka_amd.SCALAR_WAVEFRONT) is b and b.scalar_step() == nka_amd.SCALAR_WAVEFRONT, name
        for bad in (2, -1, 17):
            assert L.nka_hip_batch_set_scalar_step(b._handle(), bad) == EINVAL and L.nka_hip_last_error(), (name, bad)
            with pytest.raises(nka_amd.NKAError):
                b.set_scalar_step(bad)
            assert b.scalar_step() == nka_amd.SCALAR_WAVEFRONT, (name, bad)
        b.set_scalar_step(nka_amd.SCALAR_ONE_THREAD).set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        F, Ft = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
        for _ in range(mvec + 3):
            x = rng.standard_normal((nsys, vlen))
            F.copy_(torch.from_numpy(x))
            Ft.copy_(torch.from_numpy(x))
            b.accel_update(F)
            twin.accel_update(Ft)
            assert torch.equal(F, Ft), name
        assert [b.state_digest(k) for k in range(nsys)] == [twin.state_digest(k) for k in range(nsys)], name
    for name, (n, kw) in others.items():
        b, twin = nka_amd.nka_batch().init(nsys, n, mvec, **kw), nka_amd.nka_batch().init(nsys, n, mvec, **kw)
        assert not b.offers_scalar_step() and L.nka_hip_batch_offers_scalar_step(b._handle()) == 0, name
        assert L.nka_hip_batch_set_scalar_step(b._handle(), nka_amd.SCALAR_WAVEFRONT) == EINVAL and b"wide" in L.nka_hip_last_error(), name
        with pytest.raises(nka_amd.NKAError):
            b.set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        with pytest.raises(nka_amd.NKAError):
            b.set_scalar_step(2)
        assert b.set_scalar_step(nka_amd.SCALAR_ONE_THREAD) is b and b.scalar_step() == nka_amd.SCALAR_ONE_THREAD, name
        F, Ft = (torch.zeros(nsys, n, dtype=torch.float64, device="cuda") for _ in range(2))
        for _ in range(mvec + 2):      # ... and the batch updates as before
            x = rng.standard_normal((nsys, n))
            F.copy_(torch.from_numpy(x))
            Ft.copy_(torch.from_numpy(x))
            b.accel_update(F)
            twin.accel_update(Ft)
            assert torch.equal(F, Ft), name
        assert [b.state_digest(k) for k in range(nsys)] == [twin.state_digest(k) for k in range(nsys)], name
    assert L.nka_hip_batch_offers_scalar_step(None) < 0 and L.nka_hip_batch_scalar_step(None) < 0


def _run_at(torch, nka_amd, vlen, mvec, inputs, nsys, pos, active_others, how):
    """System `pos` of a wide batch of nsys runs `inputs`; the systems of `active_others` run data of their own, the rest sit out."""
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True).set_scalar_step(how)
    rng = np.random.default_rng(5 + 11 * nsys + pos)
    F = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    active = sorted(set(active_others) | {pos})
    mask = None if len(active) == nsys else TW._mask(torch, nsys, active)
    outs = []
    for x in inputs:
        Xh = rng.standard_normal((nsys, vlen))
        Xh[pos] = x
        F.copy_(torch.from_numpy(Xh))
        b.accel_update(F, mask)
        outs.append(F[pos].cpu().numpy())
    st = b.state(pos)
    return outs, b.state_digest(pos), b.reductions(pos), st.h, st.c


def test_results_depend_on_the_systems_own_values_alone(torch_cuda, CH):
    """The wavefront step at nsys 1 and 6, at every position, under four masks of the others: the bits of the one-thread step of
    a batch of one.  The inputs drop by dependence and by capacity (batch_seq.Sequence)."""
    import nka_amd
    vlen, mvec = CH[0] + 1, 5
    seq = B.Sequence(vlen, 79)
    inputs = [seq.next() for _ in range(2 * mvec + 6)]
    base = _run_at(torch_cuda, nka_amd, vlen, mvec, inputs, 1, 0, [], nka_amd.SCALAR_ONE_THREAD)
    runs = [(1, 0, ())]
    for pos in range(6):
        rest = [q for q in range(6) if q != pos]
        runs += [(6, pos, tuple(rest)), (6, pos, ()), (6, pos, tuple(rest[::2])), (6, pos, tuple(rest[1::2]))]
    for nsys, pos, others in runs:
        outs, dig, red, h, c = _run_at(torch_cuda, nka_amd, vlen, mvec, inputs, nsys, pos, others, nka_amd.SCALAR_WAVEFRONT)
        where = (nsys, pos, others)
        assert dig == base[1] and _eq(red, base[2]) and _eq(h, base[3]) and _eq(c, base[4]), where
        assert all(_eq(a, c0) for a, c0 in zip(outs, base[0])), where
