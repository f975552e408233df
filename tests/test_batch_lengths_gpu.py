"""Per-system lengths of the batched accelerator (nka_hip_batch_set_lengths; include/nka_hip_batch.h, LENGTHS), narrow and wide.

The contract is bit-equality with a TWIN: system k of length L in a batch of length vlen against the same system in a batch of
the same kind created with vlen = L.  Every comparison below is ==; the tails [L, vlen) are painted (tests/batch_lengths.py)
and held byte for byte after every call.

  1 narrow, twins        13 lengths in one batch of 1100; 3 flavours x both explicit sum orders x plain / weighted x ld 1100 / 1101
  2 narrow step          the same through accel_step with X, mask, tol and fnorm; tol is the twin's own fnorm where a system retires
  3 wide, twins          10 lengths around every chunk edge in one batch of 3 C + 33; 8 lengths of 1 ... 18 chunks and 4 of 1 ... 257,
                         where the loops over a system's own partials take whole trips; and no stale partial after a shrink
  4 set to NULL          set_lengths(None) and a restart: the bits of a batch that never had lengths
  5 the older recipe     lengths against weights 1 / 0 on a finite padding
  6 graph                captured before the first update; new lengths and a masked restart between two replays
  7 refusals             0, vlen + 1, a negative length, a short span, a null handle: refused, and nothing changed"""
import ctypes as C
import itertools

import numpy as np
import pytest

import batch_lengths as BL
import batch_seq as B
import batch_wide as BW
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def CH():
    return BW.limits()


def _mask(torch, nsys, ks):
    m = np.zeros(nsys, np.int32)
    m[list(ks)] = 1
    return torch.from_numpy(m).cuda()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_system(a, ka, b, kb, L, where, digest=True, slots="all"):
    """System ka of batch a (length L inside a longer row) against system kb of batch b: red[], the state, num_vec, the digest
    and [0, L) of the slots, bit for bit."""
    assert _bits_equal(a.reductions(ka), b.reductions(kb)), (where, "red[]", a.reductions(ka), b.reductions(kb))
    sa, sb = a.state(ka), b.state(kb)
    assert sa.list_order() == sb.list_order() and sa.free_order() == sb.free_order(), (where, "list")
    assert (sa.subspace, sa.pending, sa.first, sa.last, sa.free) == (sb.subspace, sb.pending, sb.first, sb.last, sb.free), (where, "state")
    assert a.num_vec()[ka] == b.num_vec()[kb], (where, "num_vec")
    if digest:
        assert _bits_equal(sa.h, sb.h) and _bits_equal(sa.c, sb.c), (where, "h, c")
        assert a.state_digest(ka) == b.state_digest(kb), (where, "digest")
    for s in (range(1, a.max_vec() + 2) if slots == "all" else sa.list_order()):
        assert _bits_equal(a.w(ka, s)[:L], b.w(kb, s)[:L]), (where, "w", s)
        assert _bits_equal(a.v(ka, s)[:L], b.v(kb, s)[:L]), (where, "v", s)


class Ragged:
    """One batch with lengths `lens` beside one twin batch of one system per length; update() / step() run both on the same
    inputs and compare everything the contract names."""

    def __init__(self, torch, lens, vlen, mvec, flavor, order=None, wide=False, weights=None, odd_ld=False, with_x=False):
        import nka_amd
        self.torch, self.lens, self.vlen, self.mvec, self.nsys = torch, list(lens), vlen, mvec, len(lens)
        nsys = self.nsys
        self.b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor, wide=wide)
        self.twins = [nka_amd.nka_batch().init(1, L, mvec, flavor=flavor, wide=wide) for L in lens]
        if order is not None:
            for a in [self.b] + self.twins:
                a.set_sum_order(order)
        # every slot as it is right after creation: the tails must still hold this at the end
        self.slots0 = {(k, s): (self.b.w(k, s), self.b.v(k, s)) for k in range(nsys) for s in range(1, mvec + 2)}
        if weights is not None:
            assert weights.shape == (nsys, vlen) and all((weights[k, L:] == BL.TAIL_WEIGHT).all() for k, L in enumerate(lens))
            self.b.set_dot_weights(_dev(torch, weights))
            for k, L in enumerate(lens):
                self.twins[k].set_dot_weights(weights[k:k + 1, :L].copy())
        assert not self.b.has_lengths() and (self.b.lengths() == vlen).all()
        assert self.b.set_lengths(np.array(lens, np.int64)) is self.b
        assert self.b.has_lengths() and self.b.lengths().dtype == np.int32 and self.b.lengths().tolist() == self.lens
        self.ld = vlen + (1 - vlen % 2 if odd_ld else vlen % 2)
        self.paint = {"F": BL.nan_paint(nsys, vlen, 1), "X": BL.nan_paint(nsys, vlen, 2)}
        self.raw = {n: torch.full((nsys * self.ld,), BL.PAD, dtype=torch.float64, device="cuda") for n in (("F", "X") if with_x else ("F",))}
        self.rows = {n: r.view(nsys, self.ld)[:, :vlen] for n, r in self.raw.items()}
        for n, r in self.rows.items():
            r.copy_(torch.from_numpy(self.paint[n]))
        self.tw = {n: [torch.zeros(1, L, dtype=torch.float64, device="cuda") for L in lens] for n in self.raw}

    def put(self, name, xs):
        """xs[k]: the first lens[k] elements of row k (None: leave the row); the tails stay as they are on the device."""
        for k, x in enumerate(xs):
            if x is not None:
                self.rows[name][k, :self.lens[k]].copy_(self.torch.from_numpy(x))
                self.tw[name][k].copy_(self.torch.from_numpy(x.reshape(1, -1)))

    def check_rows(self, where, names=None, only=None):
        for n in (names or self.raw):
            got = self.raw[n].cpu().numpy().reshape(self.nsys, self.ld)
            assert (got[:, self.vlen:] == BL.PAD).all(), (where, n, "the padding between two rows was written")
            assert BL.tails_intact(got[:, :self.vlen], self.paint[n], self.lens) == [], (where, n, "a tail was written")
            for k, L in enumerate(self.lens):
                if only is None or k in only:
                    assert BL.same_bytes(got[k, :L], self.tw[n][k].cpu().numpy()[0]), (where, n, "system", k, "length", L)

    def check_systems(self, where, only=None, digest=True):
        for k, L in enumerate(self.lens):
            if only is None or k in only:
                _same_system(self.b, k, self.twins[k], 0, L, where + ("system", k, "length", L), digest=digest)

    def update(self, xs, where, active=None):
        """active: the systems that run (None: all)."""
        self.put("F", xs)
        self.b.accel_update(self.rows["F"], None if active is None else _mask(self.torch, self.nsys, active))
        for k in (range(self.nsys) if active is None else active):
            self.twins[k].accel_update(self.tw["F"][k])
        self.check_rows(where)
        self.check_systems(where)

    def check_slot_tails(self, where):
        for (k, s), (w0, v0) in self.slots0.items():
            L = self.lens[k]
            assert BL.same_bytes(self.b.w(k, s)[L:], w0[L:]) and BL.same_bytes(self.b.v(k, s)[L:], v0[L:]), (where, "slot tail", k, s)


def _run_updates(r, calls, seed, where):
    seqs = BL.sequences(r.lens, seed)
    full = False
    for t in range(calls):
        r.update([s.next() for s in seqs], where + ("call", t))
        full = full or bool((r.b.num_vec() == r.mvec).any())      # (a full list: capacity drops from there on)
    r.check_slot_tails(where)
    return full


# ---- 1. narrow, bit-equality with twins ----------------------------------------------------------------------------------------

def _orders():
    import nka_amd
    return {"fast": nka_amd.SUMS_BLOCKED_ROUNDED, "reference": nka_amd.SUMS_REFERENCE_ORDER}


@pytest.mark.parametrize("oname", ["fast", "reference"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_narrow_lengths_carry_the_bits_of_a_batch_of_that_length(torch_cuda, flavor, oname):
    """13 systems of 13 lengths in one batch of 1100 against 13 batches of one system; mvec = 3 over 10 calls (the list fills at
    the fourth, capacity drops from there on; batch_seq.Sequence adds dependent, repeated and zero inputs); plain and with one
    weight row per system; ld = 1100 and 1101.  After every call: F[:, :L], red[], the state, num_vec, the digest and [0, L) of
    EVERY slot with ==, and the painted tails byte for byte; at the end the tails of every slot are what they were at creation."""
    vlen, lens = BL.NARROW_VLEN, BL.NARROW_LENS
    for weighted, odd_ld in itertools.product((False, True), (False, True)):
        w = BL.weight_rows(lens, vlen, 3) if weighted else None
        r = Ragged(torch_cuda, lens, vlen, 3, flavor, _orders()[oname], weights=w, odd_ld=odd_ld)
        assert r.ld == (1101 if odd_ld else 1100) and r.b.dot_weighted() == weighted
        assert _run_updates(r, 10, 100 * flavor + 7, (flavor, oname, weighted, r.ld)), "the lists never filled"


def test_narrow_lengths_with_three_groups_of_older_vectors(torch_cuda):
    """mvec = 9 once: the sweep over the older vectors runs three groups of four."""
    r = Ragged(torch_cuda, BL.NARROW_LENS, BL.NARROW_VLEN, 9, 2, _orders()["fast"], odd_ld=True)
    seqs = [np.random.default_rng([9, k]) for k in range(r.nsys)]      # fresh inputs only: the lists grow to nine
    for t in range(12):
        r.update([g.standard_normal(L) for g, L in zip(seqs, r.lens)], ("mvec 9", "call", t))
    assert (r.b.num_vec()[2:] == 9).all(), r.b.num_vec()      # (lengths 1 and 2 cannot hold nine independent vectors)
    r.check_slot_tails(("mvec 9",))


# ---- 2. narrow step --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oname", ["fast", "reference"])
@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_narrow_step_with_lengths_retires_and_corrects_like_the_twins(torch_cuda, flavor, oname):
    """accel_step with X, mask, tol and fnorm over 9 calls, plain and weighted.  System k is to retire at call 2 + k % 6: there
    tol[k] is the fnorm a twin-kind batch of one system forms of that very input (a probe that runs the step without tol), so
    the stop rule r <= tol decides on equal bits; everywhere else tol = fnorm / 2.  fnorm and the mask with ==, X[:, :L] and
    F[:, :L] with ==, the tails of F and X byte for byte; a retired system keeps its rows and its state in both."""
    import nka_amd
    torch = torch_cuda
    vlen, lens, mvec = BL.NARROW_VLEN, BL.NARROW_LENS, 3
    nsys = len(lens)
    for weighted in (False, True):
        w = BL.weight_rows(lens, vlen, 4) if weighted else None
        r = Ragged(torch, lens, vlen, mvec, flavor, _orders()[oname], weights=w, odd_ld=True, with_x=True)
        probes = [nka_amd.nka_batch().init(1, L, mvec, flavor=flavor).set_sum_order(_orders()[oname]) for L in lens]
        if weighted:
            for k, L in enumerate(lens):
                probes[k].set_dot_weights(w[k:k + 1, :L].copy())
        seqs = BL.sequences(lens, 50 + flavor)
        rng = np.random.default_rng(8)
        r.put("X", [rng.standard_normal(L) for L in lens])
        active = torch.ones(nsys, dtype=torch.int32, device="cuda")
        fnorm = torch.full((nsys,), -1.0, dtype=torch.float64, device="cuda")
        t_active = [torch.ones(1, dtype=torch.int32, device="cuda") for _ in lens]
        t_fnorm = [torch.full((1,), -1.0, dtype=torch.float64, device="cuda") for _ in lens]
        retired = set()
        for t in range(9):
            where = (flavor, oname, weighted, "call", t)
            xs = [None if k in retired else s.next() for k, s in enumerate(seqs)]
            tol = np.zeros(nsys)
            for k, L in enumerate(lens):
                if xs[k] is None:
                    continue
                pf = torch.zeros(1, dtype=torch.float64, device="cuda")
                probes[k].accel_step(_dev(torch, xs[k].reshape(1, L)), fnorm=pf)
                tol[k] = float(pf.item()) if t == 2 + k % 6 else 0.5 * float(pf.item())
            r.put("F", xs)
            before = active.cpu().numpy().copy()
            r.b.accel_step(r.rows["F"], r.rows["X"], active, _dev(torch, tol), fnorm)
            for k in range(nsys):
                if before[k]:
                    r.twins[k].accel_step(r.tw["F"][k], r.tw["X"][k], t_active[k], _dev(torch, tol[k:k + 1]), t_fnorm[k])
            got_active, got_fnorm = active.cpu().numpy(), fnorm.cpu().numpy()
            for k in range(nsys):
                assert got_active[k] == int(t_active[k].item()), (where, "mask", k)
                assert BL.same_bytes(got_fnorm[k:k + 1], t_fnorm[k].cpu().numpy()), (where, "fnorm", k, got_fnorm[k])
                if before[k] and not got_active[k]:
                    assert t == 2 + k % 6 or got_fnorm[k] == 0.0, (where, "retired out of turn", k)
                    retired.add(k)
            r.check_rows(where)
            r.check_systems(where)
        assert len(retired) >= 10, retired      # (a zero input retires at once; every scheduled system retired)
        r.check_slot_tails((flavor, oname, weighted))


# ---- 3. wide, bit-equality with wide twins -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mvec", [3, 9])
@pytest.mark.parametrize("flavor", [0, 1, 2])
def test_wide_lengths_carry_the_bits_of_a_wide_batch_of_that_length(torch_cuda, CH, flavor, mvec):
    """Ten systems around every chunk edge in one wide batch of 3 C + 33 (four chunks) against ten wide batches of one system:
    the workgroups of the chunks a system does not own return, and only its own partials are added."""
    vlen, lens = BL.wide_shape(CH[0])
    r = Ragged(torch_cuda, lens, vlen, mvec, flavor, wide=True, odd_ld=(mvec == 3))
    assert r.b.is_wide() and all(t.is_wide() for t in r.twins)
    if mvec == 3:
        assert _run_updates(r, 9, 300 + flavor, ("wide", flavor, mvec))
    else:
        rngs = [np.random.default_rng([19, flavor, k]) for k in range(r.nsys)]
        for t in range(11):
            r.update([g.standard_normal(L) for g, L in zip(rngs, lens)], ("wide", flavor, mvec, "call", t))
        assert (r.b.num_vec()[1:] == 9).all(), r.b.num_vec()
        r.check_slot_tails(("wide", flavor, mvec))


@pytest.mark.parametrize("flavor", [0, 2])
def test_wide_lengths_where_the_chain_over_the_own_partials_takes_whole_trips(torch_cuda, CH, flavor):
    """Eight systems in one wide batch of 17 C + 33 (18 chunks) against eight wide batches of one system: the systems add 1, 2,
    9, 9, 10, 16, 17 and 18 of their partials at a stride of 18, so the eight-way chain of k_wide_scalar runs no trip, one
    and two over nown, with a remainder of none, one and seven.  mvec = 3 over 9 calls: the lists fill, the capacity drop runs.
    The twins at 9, 10, 16 and 17 chunks are shapes tests/test_batch_wide_gpu.py holds to the exact sums."""
    c = CH[0]
    vlen, lens = BL.wide_medium_shape(c)
    assert [BW.nchunk(L, c) for L in lens] == [1, 2, 9, 9, 10, 16, 17, 18] and BW.nchunk(vlen, c) == 18
    r = Ragged(torch_cuda, lens, vlen, 3, flavor, wide=True, odd_ld=True)
    assert r.b.is_wide() and all(t.is_wide() for t in r.twins)
    assert _run_updates(r, 9, 500 + flavor, ("wide, 18 chunks", flavor)), "the lists never filled"


def test_wide_lengths_on_both_sides_of_one_staging_trip(torch_cuda, CH):
    """Four systems in one wide batch of 256 C + 513 (257 chunks) against four wide batches of one system: a system that ends
    with the 256 partials one trip of the staging loop of wide_norm_sum holds, one that is one partial into the second trip, the
    full row, and one of a single chunk that gives 256 chunks up.  Default flavour, mvec = 3, five calls."""
    c, cap = CH
    vlen, lens = BL.wide_long_shape(c)
    assert vlen <= cap and [BW.nchunk(L, c) for L in lens] == [256, 257, 257, 1] and BW.nchunk(vlen, c) == 257
    r = Ragged(torch_cuda, lens, vlen, 3, 2, wide=True, odd_ld=True)
    assert r.b.is_wide() and all(t.is_wide() for t in r.twins)
    _run_updates(r, 5, 600, ("wide, 257 chunks",))
    assert (r.b.num_vec() >= 1).all(), r.b.num_vec()


def test_wide_system_reads_no_partial_of_a_chunk_it_gave_up(torch_cuda, CH):
    """System 1 of three runs at full length and meets a NaN in its third chunk, so the partials of that chunk hold NaN.  Then
    set -> restart -> update: its length shrinks to C + 1 (two chunks), it is restarted under a mask, and from there on it equals
    a wide batch of C + 1 elements that never saw the NaN -- rows, red[], decisions, stored vectors.  (The digest covers h and c,
    which a restart leaves as they were: it is not compared for this system.)  Systems 0 and 2 keep their twins throughout."""
    import nka_amd
    torch = torch_cuda
    c = CH[0]
    vlen, mvec, ill = 3 * c + 33, 3, 1
    lens0, lens1 = [c - 1, vlen, 2 * c + 513], [c - 1, c + 1, 2 * c + 513]
    r = Ragged(torch, lens0, vlen, mvec, 2, wide=True)
    rng = np.random.default_rng(12)
    for t in range(3):
        xs = [rng.standard_normal(L) for L in lens0]
        xs[ill][2 * c + 5] = np.nan
        r.put("F", xs)
        r.b.accel_update(r.rows["F"])
        for k in (0, 2):
            r.twins[k].accel_update(r.tw["F"][k])
        r.check_rows(("ill", t), only=(0, 2))
        r.check_systems(("ill", t), only=(0, 2))
    assert np.isnan(r.b.reductions(ill)[0])
    r.b.set_lengths(lens1)
    r.b.restart(_mask(torch, 3, [ill]))
    r.lens = lens1
    r.twins[ill] = nka_amd.nka_batch().init(1, c + 1, mvec, flavor=2, wide=True)
    r.tw["F"][ill] = torch.zeros(1, c + 1, dtype=torch.float64, device="cuda")
    r.paint["F"] = r.raw["F"].cpu().numpy().reshape(3, r.ld)[:, :vlen].copy()      # the tail of system 1 now starts at C + 1
    for t in range(7):
        where = ("shrunk", t)
        r.put("F", [rng.standard_normal(L) for L in lens1])
        r.b.accel_update(r.rows["F"])
        for k in range(3):
            r.twins[k].accel_update(r.tw["F"][k])
        r.check_rows(where)
        r.check_systems(where, only=(0, 2))
        _same_system(r.b, ill, r.twins[ill], 0, c + 1, where + ("the shrunk system",), digest=False, slots="list")
        assert np.isfinite(r.b.reductions(ill)).all(), where
    assert r.b.num_vec()[ill] == mvec


# ---- 4. set to NULL ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_without_lengths_again_the_batch_is_one_that_never_had_them(torch_cuda, CH, wide):
    """Ragged updates, then set_lengths(None) and a restart: from there on rows, red[], decisions and stored vectors are those of
    a batch that ran full rows all along (its digest differs only through h and c, which a restart leaves: not compared)."""
    import nka_amd
    torch = torch_cuda
    vlen, lens = BL.wide_shape(CH[0]) if wide else (BL.NARROW_VLEN, BL.NARROW_LENS)
    nsys, mvec = len(lens), 3
    a = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide).set_lengths(list(lens))
    plain = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide)
    rng = np.random.default_rng(4)
    Fa, Fp = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
    for t in range(8):
        if t == 3:
            assert a.set_lengths(None) is a and not a.has_lengths() and (a.lengths() == vlen).all()
            a.restart()
            plain.restart()
        x = rng.standard_normal((nsys, vlen))
        for b, F in ((a, Fa), (plain, Fp)):
            F.copy_(torch.from_numpy(x))
            b.accel_update(F)
        if t < 3:
            assert not torch.equal(Fa[:-1], Fp[:-1]) or t == 0
            continue
        assert BL.same_bytes(Fa.cpu().numpy(), Fp.cpu().numpy()), t
        for k in range(nsys):
            _same_system(a, k, plain, k, vlen, ("call", t, "system", k), digest=False, slots="list")
    assert (a.num_vec() == mvec).all()


# ---- 5. the older recipe ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oname", ["fast", "reference"])
def test_lengths_equal_the_zero_weight_recipe_on_a_finite_padding(torch_cuda, oname):
    """A lengths batch against a batch with weight rows 1 below L and 0 from there on (include/nka_hip_batch.h, RAGGED BATCHES)
    on the same rows with a finite padding: F[:, :L], red[] and the digest are equal, in the three flavours."""
    import nka_amd
    torch = torch_cuda
    vlen, lens, mvec = BL.NARROW_VLEN, BL.NARROW_LENS, 3
    nsys = len(lens)
    for flavor in (0, 1, 2):
        a = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(_orders()[oname]).set_lengths(list(lens))
        m = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=flavor).set_sum_order(_orders()[oname])
        m.set_dot_weights(BL.mask_rows(lens, vlen))
        seqs = [B.Sequence(vlen, 900 + k) for k in range(nsys)]
        Fa, Fm = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
        for t in range(9):
            x = np.stack([s.next() for s in seqs])
            for b, F in ((a, Fa), (m, Fm)):
                F.copy_(torch.from_numpy(x))
                b.accel_update(F)
            ga, gm = Fa.cpu().numpy(), Fm.cpu().numpy()
            for k, L in enumerate(lens):
                where = (oname, flavor, "call", t, "system", k)
                assert BL.same_bytes(ga[k, :L], gm[k, :L]), where
                assert BL.same_bytes(ga[k, L:], x[k, L:]), (where, "the tail was written")
                assert _bits_equal(a.reductions(k), m.reductions(k)), where
                assert a.state_digest(k) == m.state_digest(k), where
        assert (a.num_vec() == mvec).any() and np.array_equal(a.num_vec(), m.num_vec())


# ---- 6. graph ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_an_update_with_lengths_is_capturable_and_reads_new_lengths_at_replay(torch_cuda, CH, wide):
    """Captured BEFORE the first update, replayed 24 times through growth, dependence and capacity drops against an eager batch
    that is given the same calls.  Before replay 10 three systems get new lengths -- set_lengths, then a masked restart --, and
    the replays from there on run with them.  set_lengths while the stream captures raises with NKA_HIP_ESTATE (device, host and
    NULL form), changes nothing, and the capture still ends cleanly."""
    import nka_amd
    torch = torch_cuda
    nsys, mvec = 8, 4
    vlen = CH[0] + 513 if wide else 300
    rng = np.random.default_rng(21)
    lens0 = rng.integers(1, vlen + 1, nsys)
    lens0[0], lens0[7] = vlen, 1
    lens1 = lens0.copy()
    changed = [1, 4, 7]
    lens1[changed] = [vlen, 65, vlen // 2 + 1]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide).set_lengths(lens0)
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide).set_lengths(lens0)
    new_dev = _dev(torch, lens1.astype(np.int32))
    new_host = lens1.astype(np.int32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    raised = []
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        b.accel_update(static, mask)
        try:
            b.set_lengths(new_dev)
        except nka_amd.NKAError as e:
            raised.append(str(e))
        rc_host = b._L.nka_hip_batch_set_lengths_host(b._handle(), new_host.ctypes.data_as(C.POINTER(C.c_int32)))
        rc_null = b._L.nka_hip_batch_set_lengths(b._handle(), None)
    assert len(raised) == 1 and f"({ESTATE})" in raised[0] and rc_host == ESTATE and rc_null == ESTATE, (raised, rc_host, rc_null)
    assert b.has_lengths() and b.lengths().tolist() == lens0.tolist()
    seqs = [B.Sequence(vlen, 800 + k) for k in range(nsys)]
    paint = BL.nan_paint(nsys, vlen, 3)
    lens, full = lens0, False
    for t in range(24):
        if t == 10:
            rm = _mask(torch, nsys, changed)
            with torch.cuda.stream(side):
                b.set_lengths(new_dev)
                b.restart(rm)
            eager.set_lengths(new_host)
            eager.restart(rm)
            lens = lens1
        Xh = paint.copy()
        for k, s in enumerate(seqs):
            Xh[k, :lens[k]] = s.next()[:lens[k]]
        m = (rng.random(nsys) < 0.85).astype(np.int32)
        static.copy_(torch.from_numpy(Xh))
        mask.copy_(torch.from_numpy(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = torch.from_numpy(Xh.copy()).cuda()
        eager.accel_update(F, torch.from_numpy(m).cuda())
        got, want = static.cpu().numpy(), F.cpu().numpy()
        assert BL.same_bytes(got, want), t
        assert BL.tails_intact(got, paint, lens) == [], t
        assert np.isfinite(np.concatenate([got[k, :lens[k]] for k in range(nsys)])).all(), t
        assert np.array_equal(b.num_vec(), eager.num_vec()), t
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], t
        assert all(_bits_equal(b.reductions(k), eager.reductions(k)) for k in range(nsys)), t
        full = full or bool((b.num_vec() == mvec).any())
    assert full and b.lengths().tolist() == lens1.tolist()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_refused_lengths_leave_the_previous_ones_in_force(torch_cuda, CH, wide):
    import nka_amd
    from nka_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    i32p = C.POINTER(C.c_int32)
    nsys, mvec = 5, 3
    vlen = CH[0] + 33 if wide else 300
    lens = np.array([vlen, 1, 64, vlen - 1, 129], np.int32)
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide).set_lengths(lens)
    twin = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide).set_lengths(lens)
    rng = np.random.default_rng(6)
    paint = BL.nan_paint(nsys, vlen, 5)

    def rows():
        x = paint.copy()
        for k in range(nsys):
            x[k, :lens[k]] = rng.standard_normal(lens[k])
        return x
    inputs = [rows() for _ in range(5)]
    F, Ft = (torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for _ in range(2))
    for x in inputs[:2]:
        for a, G in ((b, F), (twin, Ft)):
            G.copy_(torch.from_numpy(x))
            a.accel_update(G)
    h = b._handle()
    for bad in (0, vlen + 1, -3):                            # in the LAST entry only
        v = lens.copy()
        v[-1] = bad
        dev = _dev(torch, v)
        assert L.nka_hip_batch_set_lengths(h, C.c_void_p(dev.data_ptr())) == EINVAL and L.nka_hip_last_error(), bad
        assert L.nka_hip_batch_set_lengths_host(h, v.ctypes.data_as(i32p)) == EINVAL, bad
        for form in (dev, v, v.astype(np.int64), v.tolist()):
            with pytest.raises(nka_amd.NKAError):
                b.set_lengths(form)
        assert b.has_lengths() and b.lengths().tolist() == lens.tolist(), bad
    with pytest.raises(nka_amd.NKAError):
        b.set_lengths(np.array([1, 1, 1, 1, 2**32 + 1]))      # (must not wrap into range on its way to int32)
    for form in (lens[:-1], np.ones(nsys), _dev(torch, lens.astype(np.int64)), _dev(torch, lens)[:-1]):
        with pytest.raises(nka_amd.NKAError):
            b.set_lengths(form)
    # a device span one entry short (the library's own allocator: a buffer of exactly known size): two doubles hold four int32
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    assert L.nka_hip_vec_alloc(ws, 2, C.byref(short)) == 0
    torch.cuda.synchronize()
    assert L.nka_hip_batch_set_lengths(h, short) == EINVAL
    assert L.nka_hip_vec_free(ws, short) == 0 and L.nka_hip_vec_workspace_destroy(ws) == 0
    # a null handle
    dev = _dev(torch, lens)
    out = np.zeros(nsys, np.int32)
    assert L.nka_hip_batch_set_lengths(None, C.c_void_p(dev.data_ptr())) == EINVAL
    assert L.nka_hip_batch_set_lengths_host(None, lens.ctypes.data_as(i32p)) == EINVAL
    assert L.nka_hip_batch_get_lengths(None, out.ctypes.data_as(i32p)) == EINVAL and L.nka_hip_batch_get_lengths(h, None) == EINVAL
    assert L.nka_hip_batch_has_lengths(None) < 0
    assert b.has_lengths() and b.lengths().tolist() == lens.tolist()
    # ... and the next updates are those of a batch that was never refused anything
    for t, x in enumerate(inputs[2:]):
        for a, G in ((b, F), (twin, Ft)):
            G.copy_(torch.from_numpy(x))
            a.accel_update(G)
        assert BL.same_bytes(F.cpu().numpy(), Ft.cpu().numpy()), t
        assert BL.tails_intact(F.cpu().numpy(), paint, lens) == [], t
        for k in range(nsys):
            _same_system(b, k, twin, k, vlen, ("after the refusals", t, k))
    assert (b.num_vec()[[0, 2, 3, 4]] == mvec).all()
