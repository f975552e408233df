"""The wave batch's scalar step on the whole wavefront (nka_hip_batch_create_waves_rows with nka_hip_batch_set_scalar_step;
include/nka_hip_batch.h, WAVES ROWS; phase 4 of k_waves_update, nka_amd/csrc/nka_batch_waves.hip).  The contract is bit equality
with the one-lane step, debris included.

  1 the twin        two batches of the new entry on the same inputs, one left at the default, one with SCALAR_WAVEFRONT, compared
                    with == after EVERY call: the rows of F (and X), red[], get_state (all of h, c, next, prev, the five scalars),
                    num_vec, the digest, fnorm, the mask; at the end w and v of every slot.  batch_wide_rows.script drives them
                    through the drop logic, and a CENSUS counted on the one-lane twin's states says that it did.
  2 every pack      the same through accel_step (x, mask, tol, fnorm, a system retiring) and through ext=True with ragged lengths,
                    a weight row per system, and both together with the step
  3 the oracle      the three layers of WavesRun (tests/test_batch_waves_gpu.py) with the wavefront step on: independent of the
                    one-lane kernel
  4 switching       a batch that alternates the setting on every call; graphs captured with either step
  5 the surface     who offers it, what is refused, and that results depend on the system's own values alone

The scalar step does not depend on vlen beyond the tiles of the sweeps around it: 65 (one ragged tile), 129 (two), 385 (three and a
half pair).  Nine systems: the last workgroup has three absent wavefronts."""
import ctypes as C

import numpy as np
import pytest

import batch_seq as B
import batch_waves_ext as E
import batch_waves_rows as WR
import batch_wide_rows as R
import test_batch_sums_exact_gpu as T
import test_batch_waves_gpu as TWV
import test_batch_wide_rows_gpu as TR

pytestmark = pytest.mark.gpu

PAD = 7.0      # what lies in a row beyond the system's own length
_eq, _same_state, _mask = TR._eq, TR._same_state, TWV._i32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def CAP():
    import nka_amd
    cap, lds = nka_amd.batch_waves_rows_limits()
    assert cap == WR.cap() and 21 < cap and lds <= WR.LDS_LIMIT
    return cap


def _live_mask(torch, nsys, ks):
    m = np.zeros(nsys, np.int32)
    m[list(ks)] = 1
    return _mask(torch, m)


def _rows_batch(nsys, vlen, mvec, flavor=2, ext=False):
    import nka_amd
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, waves=True, rows=True, ext=ext)
    assert b.kind() == nka_amd.KIND_WAVES and b.offers_scalar_step() and b.scalar_step() == nka_amd.SCALAR_ONE_THREAD
    assert b.offers_lengths() == ext and b.offers_weights() == ext
    return b


def _twin(torch, make, lens, vlen, mvec, seed, *, step=False, setting=lambda t: 1, prepare=None):
    """The pattern of tests/test_batch_wide_rows_gpu.py::_twin: `one` never hears of the setter; `wav` runs setting(t) at call t.
    -> the census of the one-lane twin.  System WR.ILL is fed NaN and Inf."""
    import nka_amd
    nsys = len(lens)
    one, wav = make(), make()
    for b in (one, wav):
        if prepare is not None:
            prepare(b)
    Fo, Fw = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
    Xo, Xw = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
    no, nw = (torch.zeros(nsys, dtype=torch.float64, device="cuda") for _ in range(2))
    host = np.full((nsys, vlen), PAD)
    xhost = np.random.default_rng(seed).standard_normal((nsys, vlen))
    census, met_nonfinite = {}, False
    for t, ev in enumerate(R.script(lens, mvec, seed, ill=WR.ILL)):
        how = setting(t)
        wav.set_scalar_step(how)
        assert wav.scalar_step() == how and one.scalar_step() == nka_amd.SCALAR_ONE_THREAD
        for b in (one, wav):
            if ev["vtol"] is not None:
                b.set_vec_tol(ev["vtol"])
            if ev["relax"]:
                b.relax(_live_mask(torch, nsys, ev["relax"]))
            if ev["restart"]:
                b.restart(_live_mask(torch, nsys, ev["restart"]))
        for k, x in ev["inputs"].items():
            host[k, :lens[k]] = x
        live = sorted(ev["inputs"])
        before = {k: one.state(k) for k in live}
        mo, mw = _live_mask(torch, nsys, live), _live_mask(torch, nsys, live)
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
        met_nonfinite = met_nonfinite or not np.isfinite(one.reductions(WR.ILL)).all()
    for k in range(nsys):
        for s in range(1, mvec + 2):
            assert _eq(one.w(k, s), wav.w(k, s)) and _eq(one.v(k, s), wav.v(k, s)), (vlen, mvec, "system", k, "slot", s)
    assert met_nonfinite, "the system fed NaN and Inf never showed them in its sums"
    return census


# ---- 1. the twin ---------------------------------------------------------------------------------------------------------------------

def _twin_case(torch, vlen, mvec, flavor):
    census = _twin(torch, lambda: _rows_batch(WR.NSYS, vlen, mvec, flavor), [vlen] * WR.NSYS, vlen, mvec, seed=WR.twin_seed(mvec, flavor))
    print(f"census of the one-lane twin, vlen {vlen}, mvec {mvec}, flavour {flavor}: {sorted(census.items())}")
    if mvec >= 2:
        assert not R.census_short(census), (vlen, mvec, flavor, "the census is short", census)


@pytest.mark.parametrize("vlen", WR.VLENS)
@pytest.mark.parametrize("mvec", WR.MVECS)
def test_the_wavefront_step_is_the_one_lane_step_bit_for_bit(torch_cuda, CAP, mvec, vlen):
    """Nine systems with staggered starts over mvec + 15 calls in the default flavour: lists filled under a tiny vtol and then
    several dependence drops in one update, at the first older position and at the last, capacity drops, the last position of
    a full list evaluated behind a drop, s == 0, masked relax and restart, the path without a new pair, one system fed NaN and
    Inf.  mvec on both sides of every NLMAX boundary (6 / 11 / 21 / cap + 1 rows) and the cap."""
    assert WR.mvec_of(WR.MVECS[-1]) == CAP
    _twin_case(torch_cuda, vlen, WR.mvec_of(mvec), 2)


@pytest.mark.parametrize("flavor", [0, 1])
@pytest.mark.parametrize("mvec", [10, 20])
def test_the_wavefront_step_in_the_other_flavours(torch_cuda, mvec, flavor):
    _twin_case(torch_cuda, 129, mvec, flavor)


# ---- 2. every pack -------------------------------------------------------------------------------------------------------------------

def test_the_twin_through_the_solve_step(torch_cuda):
    """accel_step: x, mask, tol and fnorm, system 3 retiring in the middle of the sequence (the STEP instance)."""
    vlen, mvec = 129, 11
    _twin(torch_cuda, lambda: _rows_batch(WR.NSYS, vlen, mvec), [vlen] * WR.NSYS, vlen, mvec, seed=2, step=True)


@pytest.mark.parametrize("pack", ["lengths", "weights", "lengths weights step"])
def test_the_twin_with_lengths_and_weights(torch_cuda, pack):
    """ext=True: ragged lengths 1 ... 385 in a batch of 385 (the LEN instances), a weight row per system (the WGT instances), and
    both together with the step."""
    vlen, mvec = E.VLEN, 10
    lens = list(E.LENS) if "lengths" in pack else [vlen] * WR.NSYS
    assert len(lens) == WR.NSYS and max(lens) == vlen == 385
    wgt = np.random.default_rng(3).uniform(0.5, 1.5, (WR.NSYS, vlen))

    def prepare(b):
        if "lengths" in pack:
            b.set_lengths(lens)
        if "weights" in pack:
            b.set_dot_weights(wgt)
        assert b.has_lengths() == ("lengths" in pack) and b.dot_weighted() == ("weights" in pack)
    _twin(torch_cuda, lambda: _rows_batch(WR.NSYS, vlen, mvec, ext=True), lens, vlen, mvec, seed=3, step="step" in pack, prepare=prepare)


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------------

class WavesRowsRun(TWV.WavesRun):
    """WavesRun on a batch of the new entry with the wavefront step on: the device's own red[] goes to the oracle's scalar_step;
    lists, h and c with ==; the elementwise statements bit for bit."""

    def _device(self, odd_ld):
        import nka_amd
        super()._device(odd_ld)
        self.b = _rows_batch(self.nsys, self.n, self.m, self.flavor).set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        assert self.b.scalar_step() == nka_amd.SCALAR_WAVEFRONT


@pytest.mark.parametrize("mvec", [10, 21, "cap"])
def test_the_wavefront_step_against_the_oracle(torch_cuda, oracle, CAP, mvec):
    n, mvec = 129, WR.mvec_of(mvec)
    if mvec == T.SHAPE_MVEC:      # six systems of different list length: a repeated input, a masked relax and a masked restart each
        run = TWV._planned_run(WavesRowsRun(torch_cuda, oracle, 2, n, mvec, len(T.PLAN), odd_ld=True), seed=n)
        T._assert_planned_coverage(run)
    else:                         # every older count up to mvec, system k starting k % 3 calls late
        run = WavesRowsRun(torch_cuda, oracle, 2, n, mvec, 5, odd_ld=True)
        rngs, prev = [np.random.default_rng([mvec, n, k]) for k in range(run.nsys)], [None] * run.nsys
        for t in range(mvec + 4):
            inputs = {}
            for k in range(run.nsys):
                if t >= k % 3:
                    inputs[k] = prev[k] = TWV.BWV.planted_input(n, rngs[k], prev[k])
            run.update(inputs)
        assert run.widest == mvec and run.lengths_differed


# ---- 4. switching and graphs ---------------------------------------------------------------------------------------------------------

def test_alternating_the_setting_on_every_call_changes_nothing(torch_cuda):
    vlen, mvec = 129, 5
    census = _twin(torch_cuda, lambda: _rows_batch(WR.NSYS, vlen, mvec), [vlen] * WR.NSYS, vlen, mvec, seed=WR.twin_seed(mvec, 2),
                   setting=lambda t: t % 2)
    assert not R.census_short(census), census


@pytest.mark.parametrize("captured", ["wavefront", "one-lane"])
def test_a_captured_call_keeps_the_step_it_was_captured_with(torch_cuda, captured):
    """Captured BEFORE the first update and replayed 40 times through growth, dependence and capacity drops (batch_seq.Sequence),
    masks, two masked relax and a masked restart, against an eager one-lane twin (nka_hip_batch_create_waves).  After the capture
    the setter is called with the OTHER value: the replays stay what they were captured as (both leave the same bits, and the
    replay must not fail or fault on a launch whose LDS size belongs to the other step)."""
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
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, waves=True)
    full = False
    for t in range(40):
        Xh = np.stack([s.next() for s in seqs])
        m = (rng.random(nsys) < 0.8).astype(np.int32)
        if t in (9, 20):
            rm = _live_mask(torch, nsys, [1, 4, 6])
            with torch.cuda.stream(side):
                b.relax(rm)
            eager.relax(rm)
        if t == 30:
            rm = _live_mask(torch, nsys, [0, 5])
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

def test_who_offers_the_scalar_step_and_what_is_refused(torch_cuda, CAP):
    import nka_amd
    from nka_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    EINVAL = -1
    nsys, vlen, mvec = 3, 129, 4
    rng = np.random.default_rng(12)
    for ext in (False, True):
        b, twin = _rows_batch(nsys, vlen, mvec, ext=ext), nka_amd.nka_batch().init(nsys, vlen, mvec, waves=True, ext=ext)
        assert L.nka_hip_batch_offers_scalar_step(b._handle()) == 1 and L.nka_hip_batch_kind(b._handle()) == 3
        assert b.vector_bytes() == twin.vector_bytes() and b.storage() == nka_amd.STORE_F64
        assert b.set_scalar_step(nka_amd.SCALAR_WAVEFRONT) is b and b.scalar_step() == nka_amd.SCALAR_WAVEFRONT
        for bad in (2, -1, 17):
            assert L.nka_hip_batch_set_scalar_step(b._handle(), bad) == EINVAL and L.nka_hip_last_error(), (ext, bad)
            with pytest.raises(nka_amd.NKAError):
                b.set_scalar_step(bad)
            assert b.scalar_step() == nka_amd.SCALAR_WAVEFRONT, (ext, bad)
        b.set_scalar_step(nka_amd.SCALAR_ONE_THREAD).set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
        if not ext:      # lengths and weights are refused as on a batch of create_waves, and the batch stays usable
            with pytest.raises(nka_amd.NKAError):
                b.set_lengths([vlen] * nsys)
            with pytest.raises(nka_amd.NKAError):
                b.set_dot_weights(np.ones(vlen))
            assert not b.has_lengths() and not b.dot_weighted()
        with pytest.raises(nka_amd.NKAError):
            b.set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
        F, Ft = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
        for _ in range(mvec + 3):
            x = rng.standard_normal((nsys, vlen))
            F.copy_(torch.from_numpy(x))
            Ft.copy_(torch.from_numpy(x))
            b.accel_update(F)
            twin.accel_update(Ft)
            assert torch.equal(F, Ft), ext
        assert [b.state_digest(k) for k in range(nsys)] == [twin.state_digest(k) for k in range(nsys)], ext
    # every other kind behaves as it did
    others = {"narrow": (vlen, {}), "lanes": (33, dict(lanes=True)), "waves": (65, dict(waves=True)), "waves ext": (65, dict(waves=True, ext=True))}
    for name, (n, kw) in others.items():
        b = nka_amd.nka_batch().init(nsys, n, mvec, **kw)
        assert not b.offers_scalar_step() and L.nka_hip_batch_offers_scalar_step(b._handle()) == 0, name
        assert L.nka_hip_batch_set_scalar_step(b._handle(), nka_amd.SCALAR_WAVEFRONT) == EINVAL and b"wide" in L.nka_hip_last_error(), name
        assert b.set_scalar_step(nka_amd.SCALAR_ONE_THREAD) is b and b.scalar_step() == nka_amd.SCALAR_ONE_THREAD, name
    assert nka_amd.nka_batch().init(nsys, 4096, mvec, wide=True).offers_scalar_step()
    # creation: ext outside {0, 1}, mvec above the cap and the wave limits are refused before anything is allocated (no handle comes back)
    h = C.c_void_p()
    _, vcap = nka_amd.batch_waves_limits()
    for nsys_, vlen_, mvec_, vtol, ext, word in ((4, 129, 3, 0.01, 2, b"ext"), (4, 129, 3, 0.01, -1, b"ext"), (4, 129, CAP + 1, 0.01, 0, str(CAP).encode()),
                                                 (4, 129, CAP + 1, 0.01, 1, str(CAP).encode()), (4, 129, 33, 0.01, 0, b"mvec"), (0, 129, 3, 0.01, 0, b"nsys"),
                                                 (4, vcap + 1, 3, 0.01, 1, b"vlen"), (4, 0, 3, 0.01, 0, b"vlen"), (4, 129, 0, 0.01, 0, b"mvec"),
                                                 (4, 129, 3, 0.0, 0, b"vtol")):
        h.value = 1
        assert L.nka_hip_batch_create_waves_rows(C.byref(h), nsys_, vlen_, mvec_, vtol, 0, 0, None, ext) == EINVAL and h.value is None
        err = L.nka_hip_last_error()
        assert b"nka_hip_batch_create_waves_rows" in err and word in err, (err, word)
    with pytest.raises(nka_amd.NKAError):
        nka_amd.nka_batch().init(4, 129, CAP + 1, waves=True, rows=True)
    assert _rows_batch(4, 129, CAP).max_vec() == CAP
    assert L.nka_hip_batch_create_waves_rows(None, 4, 129, 3, 0.01, 0, 0, None, 0) == EINVAL
    assert L.nka_hip_batch_offers_scalar_step(None) < 0 and L.nka_hip_batch_scalar_step(None) < 0 and L.nka_hip_batch_set_scalar_step(None, 1) < 0


def _run_at(torch, nka_amd, vlen, mvec, inputs, nsys, pos, active_others, how):
    """System `pos` of a batch of nsys runs `inputs`; the systems of `active_others` run data of their own, the rest sit out."""
    b = _rows_batch(nsys, vlen, mvec).set_scalar_step(how)
    rng = np.random.default_rng(5 + 11 * nsys + pos)
    F = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    active = sorted(set(active_others) | {pos})
    mask = None if len(active) == nsys else _live_mask(torch, nsys, active)
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
    """The wavefront step at nsys 1 and 6, at every position (every wavefront of a workgroup, and a second workgroup), under four
    masks of the others: the bits of the one-lane step of a batch of one.  The inputs drop by dependence and by capacity
    (batch_seq.Sequence)."""
    import nka_amd
    vlen, mvec = 129, 5
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
