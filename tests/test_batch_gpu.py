"""The batched accelerator (include/nka_hip_batch.h, nka_amd.nka_batch): many small systems advanced by one launch, one
workgroup per system.  Every system is held to its own oracle -- bit for bit with reference-order sums, by the numerical
contract (tests/parity_util.py) with the fast sums -- and to the properties batching adds: systems of different list
length in one launch, masks that leave a system's bytes alone, results that do not depend on the batch around a system,
and graph capture from the first call."""
import ctypes as C

import numpy as np
import pytest

import batch_seq as B
import parity_util as P
import scenarios as S

pytestmark = pytest.mark.gpu

VLENS = [1, 7, 64, 65, 257, 700, 4099]
MVECS = [1, 5, 20, 32]
NSYS = 37


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _decisions(st):
    return st.list_order(), st.free_order(), (st.subspace, st.pending)


def _live(st):
    return st.list_order()[1:] if st.pending else st.list_order()


def _assert_decisions(b, k, ora, nv, where):
    sb, so = b.state(k), ora.state()
    assert nv[k] == ora.num_vec(), (where, k)
    assert _decisions(sb) == _decisions(so), (where, k)
    return sb, so


def _assert_bits_of_oracle(b, k, ora, flavor, sb, so, where):
    """h and c on the live entries, every stored w / v of the list: the oracle's bits (compact storage: the v array of a
    normalised pair holds fl(v' - w'), include/nka_hip.h)."""
    live = _live(so)
    ix = np.ix_([s - 1 for s in live], [s - 1 for s in live])
    assert np.array_equal(sb.h[ix], so.h[ix]), (where, k, "h")
    if so.c is not None:
        assert np.array_equal(sb.c[[s - 1 for s in live]], so.c[[s - 1 for s in live]]), (where, k, "c")
    for slot in so.list_order():
        wo, vo = ora.w(slot), ora.v(slot)
        assert np.array_equal(b.w(k, slot), wo), (where, k, slot, "w")
        if flavor == 2 and slot in live:
            vo = vo - wo
        assert np.array_equal(b.v(k, slot), vo), (where, k, slot, "v")


def _assert_bits_of_lone(b, k, lone, entry, sb, where):
    """The same against a lone handle with reference-order sums: state on the live entries, the sums the update formed
    (a lone handle leaves the other entries of red[] as they were, a batch zeroes them), stored vectors as they are."""
    sl = lone.state()
    assert _decisions(sb) == _decisions(sl), (where, k)
    live = _live(sl)
    ix = np.ix_([s - 1 for s in live], [s - 1 for s in live])
    assert np.array_equal(sb.h[ix], sl.h[ix]) and np.array_equal(sb.c[[s - 1 for s in live]], sl.c[[s - 1 for s in live]]), (where, k)
    rb, rl = b.reductions(k), lone.reductions()
    pending, nolder = entry
    m = (len(rb) - 2) // 2
    if pending:
        assert rb[0] == rl[0] or (np.isnan(rb[0]) and np.isnan(rl[0])), (where, k, "red[0]")
        if rb[0] != 0.0:
            assert np.array_equal(rb[1:2 + nolder], rl[1:2 + nolder]), (where, k, "red on w1'")
    assert np.array_equal(rb[2 + m:2 + m + nolder], rl[2 + m:2 + m + nolder]), (where, k, "red on f")
    for slot in sl.list_order():
        assert np.array_equal(b.w(k, slot), lone.w(slot)) and np.array_equal(b.v(k, slot), lone.v(slot)), (where, k, slot)


# ---- 1. reference bits -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavor", [0, 1, 2])
@pytest.mark.parametrize("mvec", MVECS)
@pytest.mark.parametrize("vlen", VLENS)
def test_reference_order_every_system_carries_the_reference_bits(torch_cuda, oracle, vlen, mvec, flavor):
    import nka_amd
    torch = torch_cuda
    b = nka_amd.nka_batch().init(NSYS, vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
    assert b.flavor() == flavor
    oras = [oracle.OracleNKA(vlen, mvec, flavor) for _ in range(NSYS)]
    lones = [nka_amd.nka().init(vlen, mvec, flavor=flavor).set_sum_order(nka_amd.SUMS_REFERENCE_ORDER) for _ in range(NSYS)]
    seqs = [B.Sequence(vlen, 7 * vlen + 31 * mvec + 1000 * k + flavor) for k in range(NSYS)]
    for t in range(B.num_calls(vlen, mvec)):
        X = np.stack([s.next() for s in seqs])
        entry = []
        for o in oras:
            so = o.state()
            entry.append((so.pending, len(_live(so))))
        want = X.copy()
        for k, o in enumerate(oras):
            o.accel_update(want[k])
        F = torch.from_numpy(X.copy()).cuda()
        b.accel_update(F)
        got = F.cpu().numpy()
        nv = b.num_vec()
        for k in range(NSYS):
            where = (vlen, mvec, flavor, t)
            assert np.array_equal(got[k], want[k]), (where, k, float(np.abs(got[k] - want[k]).max()))
            sb, so = _assert_decisions(b, k, oras[k], nv, where)
            _assert_bits_of_oracle(b, k, oras[k], flavor, sb, so, where)
            ft = torch.from_numpy(X[k].copy()).cuda()
            lones[k].accel_update(ft)
            assert torch.equal(ft, F[k]), (where, k, "lone handle")
            _assert_bits_of_lone(b, k, lones[k], entry[k], sb, where)


# ---- 2. fast sums by the contract -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mvec", MVECS)
@pytest.mark.parametrize("vlen", VLENS + ["cap"])
def test_fast_sums_decisions_exact_values_by_the_contract(torch_cuda, oracle, vlen, mvec):
    """SUMS_BLOCKED_ROUNDED, the three flavours side by side on the same sequences (one Spread per system serves them all: it
    runs the reference's three flavours itself), one key per (shape, flavour); conftest's finish() then applies the TYPICAL and
    HARD lines of the contract."""
    import nka_amd
    torch = torch_cuda
    if vlen == "cap":
        vlen = nka_amd.BATCH_MAX_VLEN
    calls = B.num_calls(vlen, mvec)
    seeds = [B.pick_seed(oracle, vlen, mvec, k, calls) for k in range(NSYS)]      # on the CPU, before anything runs on the GPU
    seqs = [B.Sequence(vlen, s) for s in seeds]
    spreads = [P.Spread(oracle, vlen, mvec) for _ in range(NSYS)]
    batches = {fl: nka_amd.nka_batch().init(NSYS, vlen, mvec, flavor=fl).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED) for fl in (0, 1, 2)}
    oras = {fl: [oracle.OracleNKA(vlen, mvec, fl) for _ in range(NSYS)] for fl in (0, 1, 2)}
    for t in range(calls):
        X = np.stack([s.next() for s in seqs])
        for k in range(NSYS):
            spreads[k].update(X[k])
        for fl, b in batches.items():
            want = X.copy()
            for k, o in enumerate(oras[fl]):
                o.accel_update(want[k])
            F = torch.from_numpy(X.copy()).cuda()
            b.accel_update(F)
            got = F.cpu().numpy()
            nv = b.num_vec()
            for k in range(NSYS):
                sb, _ = _assert_decisions(b, k, oras[fl][k], nv, (vlen, mvec, fl, t))
                if np.linalg.norm(X[k]) > 0:
                    P.check(S.rel_err(got[k], want[k], X[k]), sb, f"batch fast sums n={vlen} m={mvec} flavor {fl}", where=(t, k),
                            spread=spreads[k].value, truth=spreads[k].truth(got[k], X[k]))
                else:
                    assert not got[k].any(), (vlen, mvec, fl, t, k)
    assert all(s.decisions_agree for s in spreads)


# ---- 3. independent histories in one launch ---------------------------------------------------------------------------

OP_UPDATE, OP_SIT, OP_RELAX, OP_RESTART = 0, 1, 2, 3


def _script(vlen, seed, steps):
    """One system's draws: (op, input or None) per step."""
    rng = np.random.default_rng(seed)
    seq = B.Sequence(vlen, seed + 1)
    out = []
    for _ in range(steps):
        r = rng.random()
        op = OP_UPDATE if r < 0.72 else OP_SIT if r < 0.84 else OP_RELAX if r < 0.93 else OP_RESTART
        out.append((op, seq.next() if op == OP_UPDATE else None))
    return out


def _script_agrees(oracle, vlen, mvec, script, vtols):
    sp = P.Spread(oracle, vlen, mvec)
    for (op, x), vt in zip(script, vtols):
        if vt is not None:
            sp.set_vec_tol(vt)
        if op == OP_UPDATE:
            sp.update(x)
        elif op == OP_RELAX:
            sp.relax()
        elif op == OP_RESTART:
            sp.restart()
        if not sp.decisions_agree:
            return False
    return True


@pytest.mark.parametrize("mvec", [5, 9])
def test_independent_histories_share_one_launch(torch_cuda, oracle, mvec):
    import nka_amd
    torch = torch_cuda
    nsys, vlen, steps = 64, 257, 300
    grng = np.random.default_rng(4242 + mvec)
    vtols = [float(10.0 ** grng.uniform(-3, -0.3)) if grng.random() < 0.05 else None for _ in range(steps)]   # whole batch
    scripts = []
    for k in range(nsys):                                   # seeds chosen on the CPU: the exact run takes the reference's decisions
        for j in range(50):
            sc = _script(vlen, 90001 * mvec + 101 * k + 7919 * j, steps)
            if _script_agrees(oracle, vlen, mvec, sc, vtols):
                break
        else:
            raise AssertionError(("no seed of the series keeps the exact run on the reference's decisions", mvec, k))
        scripts.append(sc)
    b = nka_amd.nka_batch().init(nsys, vlen, mvec)          # SUMS_AUTO: the fast sums at this length
    fl = b.flavor()
    oras = [oracle.OracleNKA(vlen, mvec, fl) for _ in range(nsys)]
    spreads = [P.Spread(oracle, vlen, mvec) for _ in range(nsys)]
    digest = [b.state_digest(k) for k in range(nsys)]
    lengths_differed = False
    F = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    for t in range(steps):
        if vtols[t] is not None:
            b.set_vec_tol(vtols[t])
            for k in range(nsys):
                oras[k].set_vec_tol(vtols[t])
                spreads[k].set_vec_tol(vtols[t])
            digest = [b.state_digest(k) for k in range(nsys)]
        ops = np.array([scripts[k][t][0] for k in range(nsys)])
        upd = np.flatnonzero(ops == OP_UPDATE)
        if len({len(oras[k].state().list_order()) for k in upd}) > 1:
            lengths_differed = True                          # the hazard batching adds: one launch, several list lengths
        X = F.cpu().numpy()                                  # rows of systems that sit out keep whatever they held
        before = X.copy()
        want = X.copy()
        for k in upd:
            X[k] = scripts[k][t][1]
            want[k] = X[k]
            oras[k].accel_update(want[k])
            spreads[k].update(X[k])
        F.copy_(torch.from_numpy(X))
        masks = {op: torch.from_numpy((ops == op).astype(np.int32)).cuda() for op in (OP_UPDATE, OP_RELAX, OP_RESTART)}
        b.accel_update(F, masks[OP_UPDATE])
        b.relax(masks[OP_RELAX])
        b.restart(masks[OP_RESTART])
        for k in np.flatnonzero(ops == OP_RELAX):
            oras[k].relax(); spreads[k].relax()
        for k in np.flatnonzero(ops == OP_RESTART):
            oras[k].restart(); spreads[k].restart()
        got = F.cpu().numpy()
        nv = b.num_vec()
        for k in range(nsys):
            sb, _ = _assert_decisions(b, k, oras[k], nv, (mvec, t))
            d = b.state_digest(k)
            if ops[k] == OP_UPDATE:
                if np.linalg.norm(X[k]) > 0:
                    P.check(S.rel_err(got[k], want[k], X[k]), sb, f"batch independent histories m={mvec}", where=(t, k),
                            spread=spreads[k].value, truth=spreads[k].truth(got[k], X[k]))
            else:
                assert np.array_equal(got[k], before[k]), (mvec, t, k, "a row outside the update mask changed")
                if ops[k] == OP_SIT:
                    assert d == digest[k], (mvec, t, k, "the state of a system that sat out changed")
            digest[k] = d
    assert lengths_differed


# ---- 4. independence of the batch -------------------------------------------------------------------------------------

def _run_in_batch(torch, nka_amd, order, vlen, mvec, inputs, nsys, pos, others, ld):
    """System `pos` of a batch of nsys runs `inputs`; the others run their own data (`others` = "active") or sit out
    ("idle").  -> (outputs per call, digest, stored vectors of the list)."""
    b = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=0).set_sum_order(order)
    rng = np.random.default_rng(5 + nsys + pos)
    raw = torch.zeros(nsys * ld + 2, dtype=torch.float64, device="cuda")
    F = raw[:nsys * ld].view(nsys, ld)[:, :vlen]
    mask = None
    if others == "idle":
        m = np.zeros(nsys, np.int32)
        m[pos] = 1
        mask = torch.from_numpy(m).cuda()
    outs = []
    for x in inputs:
        X = rng.standard_normal((nsys, vlen))
        X[pos] = x
        F.copy_(torch.from_numpy(X))
        b.accel_update(F, mask)
        outs.append(F[pos].cpu().numpy())
    st = b.state(pos)
    vecs = [(b.w(pos, s), b.v(pos, s)) for s in st.list_order()]
    return outs, b.state_digest(pos), vecs


@pytest.mark.parametrize("order", ["reference", "rounded"])
def test_results_do_not_depend_on_the_batch_around_a_system(torch_cuda, order):
    import nka_amd
    order = nka_amd.SUMS_REFERENCE_ORDER if order == "reference" else nka_amd.SUMS_BLOCKED_ROUNDED
    vlen, mvec = 700, 5
    seq = B.Sequence(vlen, 77)
    inputs = [seq.next() for _ in range(mvec + 9)]
    runs = [(1, 0, "active", vlen), (300, 0, "active", vlen), (300, 299, "active", vlen), (300, 299, "idle", vlen),
            (300, 299, "active", vlen + 1), (300, 298, "idle", vlen + 1), (3, 1, "active", vlen + 32), (1, 0, "active", vlen)]
    assert (299 * (vlen + 1)) % 2 == 1          # that row is NOT 16-byte aligned
    base = _run_in_batch(torch_cuda, nka_amd, order, vlen, mvec, inputs, *runs[0])
    for r in runs[1:]:
        outs, dig, vecs = _run_in_batch(torch_cuda, nka_amd, order, vlen, mvec, inputs, *r)
        assert dig == base[1], r
        for a, c in zip(outs, base[0]):
            assert np.array_equal(a, c), r
        assert len(vecs) == len(base[2])
        for (w, v), (w0, v0) in zip(vecs, base[2]):
            assert np.array_equal(w, w0) and np.array_equal(v, v0), r


# ---- 5. graph capture from the first call -----------------------------------------------------------------------------

def test_update_is_capturable_from_the_first_call(torch_cuda):
    import nka_amd
    torch = torch_cuda
    nsys, vlen, mvec = 48, 300, 6
    seqs = [B.Sequence(vlen, 300 + k) for k in range(nsys)]
    rng = np.random.default_rng(9)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = nka_amd.nka_batch().init(nsys, vlen, mvec)
        static = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                   # before ANY update has run
        b.accel_update(static, mask)
    eager = nka_amd.nka_batch().init(nsys, vlen, mvec)
    for t in range(mvec + 6):
        X = np.stack([s.next() for s in seqs])              # fresh, dependent (drops), repeated and zero inputs
        m = (rng.random(nsys) < 0.8).astype(np.int32)
        static.copy_(torch.from_numpy(X))
        mask.copy_(torch.from_numpy(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        F = torch.from_numpy(X.copy()).cuda()
        eager.accel_update(F, torch.from_numpy(m).cuda())
        assert torch.equal(F, static), t
        assert np.array_equal(b.num_vec(), eager.num_vec()), t
        assert [b.state_digest(k) for k in range(nsys)] == [eager.state_digest(k) for k in range(nsys)], t
    assert len(set(b.num_vec().tolist())) > 1               # drops happened: the systems' lists differ


# ---- 6. surface --------------------------------------------------------------------------------------------------------

def test_limits_and_refused_combinations_leave_the_batch_usable(torch_cuda):
    import nka_amd
    from nka_amd import _lib
    torch = torch_cuda
    L = _lib.load()
    h = C.c_void_p()

    def create(nsys, vlen, mvec, vtol=0.01):
        return L.nka_hip_batch_create(C.byref(h), nsys, vlen, mvec, vtol, -1, 0, None)

    EINVAL = -1
    for args in [(0, 8, 3), (4, 0, 3), (4, nka_amd.BATCH_MAX_VLEN + 1, 3), (4, 8, 0), (4, 8, nka_amd.BATCH_MAX_MVEC + 1)]:
        assert create(*args) == EINVAL and h.value is None, args
        assert L.nka_hip_last_error()
    assert create(4, 8, 3, vtol=0.0) == EINVAL
    nsys, vlen, mvec = 5, 33, 3
    b = nka_amd.nka_batch().init(nsys, vlen, mvec)
    with pytest.raises(nka_amd.NKAError):
        b.set_sum_order(nka_amd.SUMS_BLOCKED)
    with pytest.raises(nka_amd.NKAError):
        b.set_sum_order(17)
    with pytest.raises(nka_amd.NKAError):
        b.set_vec_tol(0.0)
    for bad in (-1, nsys):
        for call in (b.state, b.reductions, b.state_digest, lambda s: b.w(s, 1), lambda s: b.v(s, 1)):
            with pytest.raises(nka_amd.NKAError):
                call(bad)
    with pytest.raises(nka_amd.NKAError):
        b.w(0, mvec + 2)
    F = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    for wrong in (F.float(), torch.zeros(nsys, 2 * vlen, dtype=torch.float64, device="cuda")[:, ::2], F[:-1], F[:, :-1], F[0],
                  F.cpu()):
        with pytest.raises(nka_amd.NKAError):
            b.accel_update(wrong)
    for wrong in (torch.ones(nsys + 1, dtype=torch.int32, device="cuda"), torch.ones(nsys, dtype=torch.int64, device="cuda"),
                  torch.ones(2 * nsys, dtype=torch.int32, device="cuda")[::2], torch.ones(nsys, dtype=torch.int32)):
        with pytest.raises(nka_amd.NKAError):
            b.accel_update(F, wrong)
        with pytest.raises(nka_amd.NKAError):
            b.relax(wrong)
    # an allocation too short for nsys rows of ld doubles is refused BEFORE any launch (a buffer of exactly known size: the
    # library's own allocator; a torch tensor lies inside a larger block of torch's pool)
    ws, short = C.c_void_p(), C.c_void_p()
    assert L.nka_hip_vec_workspace_create(C.byref(ws), 0, None) == 0
    assert L.nka_hip_vec_alloc(ws, (nsys - 1) * vlen + vlen - 1, C.byref(short)) == 0
    torch.cuda.synchronize()
    assert L.nka_hip_batch_accel_update(b._handle(), short, vlen, None) == EINVAL
    assert b"shorter" in L.nka_hip_last_error()
    assert L.nka_hip_vec_free(ws, short) == 0 and L.nka_hip_vec_workspace_destroy(ws) == 0
    assert L.nka_hip_batch_accel_update(b._handle(), C.c_void_p(F.data_ptr()), vlen - 1, None) == EINVAL
    assert L.nka_hip_batch_accel_update(b._handle(), C.c_void_p(F.data_ptr()), 2 ** 62, None) == EINVAL      # (no overflow on the way)
    assert L.nka_hip_batch_accel_update(b._handle(), C.c_void_p(F.data_ptr()), 2 ** 40, None) == EINVAL
    assert L.nka_hip_batch_accel_update(b._handle(), None, vlen, None) == EINVAL
    assert not b.num_vec().any()
    # ... and the batch still works
    rng = np.random.default_rng(1)
    for t in range(3):
        F.copy_(torch.from_numpy(rng.standard_normal((nsys, vlen))))
        b.accel_update(F)
    assert np.array_equal(b.num_vec(), np.full(nsys, 2, np.int32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("order", ["reference", "rounded"])
def test_non_finite_input_stays_inside_its_system(torch_cuda, oracle, bad, order):
    """A NaN / Inf in one system: every other system keeps its bits, and that system takes the oracle's decisions (the
    reference has no guard: s == 0 is false for NaN, hkk > vtol**2 is false for NaN -> the entry is dropped)."""
    import nka_amd
    torch = torch_cuda
    order = nka_amd.SUMS_REFERENCE_ORDER if order == "reference" else nka_amd.SUMS_BLOCKED_ROUNDED
    nsys, vlen, mvec, ill = 6, 257, 3, 2
    rng = np.random.default_rng(17)
    b = nka_amd.nka_batch().init(nsys, vlen, mvec).set_sum_order(order)
    clean = nka_amd.nka_batch().init(nsys, vlen, mvec).set_sum_order(order)
    ora = oracle.OracleNKA(vlen, mvec, b.flavor())
    for t in range(7):
        X = rng.standard_normal((nsys, vlen))
        Xb = X.copy()
        if t == 3:
            Xb[ill, 5] = bad
        f = Xb[ill].copy()
        ora.accel_update(f)
        F, G = torch.from_numpy(Xb.copy()).cuda(), torch.from_numpy(X.copy()).cuda()
        b.accel_update(F)
        clean.accel_update(G)
        others = [k for k in range(nsys) if k != ill]
        assert torch.equal(F[others], G[others]), t
        assert [b.state_digest(k) for k in others] == [clean.state_digest(k) for k in others], t
        assert b.num_vec()[ill] == ora.num_vec(), t
        assert b.state(ill).list_order() == ora.state().list_order(), t
        assert np.array_equal(np.isnan(F[ill].cpu().numpy()), np.isnan(f)), t
    m = np.zeros(nsys, np.int32)
    m[ill] = 1
    b.restart(torch.from_numpy(m).cuda())
    ora.restart()
    for t in range(4):
        X = rng.standard_normal((nsys, vlen))
        f = X[ill].copy()
        ora.accel_update(f)
        F, G = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(X.copy()).cuda()
        b.accel_update(F)
        clean.accel_update(G)
        assert torch.equal(F[others], G[others])
        assert b.num_vec()[ill] == ora.num_vec()
        P.record(S.rel_err(F[ill].cpu().numpy(), f, X[ill]), 1e-12, "batch after a non-finite input and restart n=257 m=3")
