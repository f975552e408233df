"""Worker of tests/test_dot_weights_sharded_gpu.py: diagonal dot-product weights (nka_hip_set_dot_weights) on SHARDED handles
whose slices carry ghost entries -- w = 1 on the entries a slice owns, 0 on its ghosts (tests/overlap_layout.py) -- through
one transport and one sum mode per process (NKA_WS_TRANSPORT = hook | p2p, NKA_WS_SUMS = auto | blocked).

`world` handles of the product library in this one process, each on its own stream and driven by its own host thread, as
tests/_configs3_inproc_worker.py drives them.  With these weights the sharded accelerator is mathematically the PLAIN
accelerator on the deduplicated global vector (tests/test_dot_weights_sharded_cpu.py shows it on the compiled reference), so
the plain checkers apply with n = n_global.  For every named layout, after EVERY call:
  a  num_vec, list order and free order of every rank = oracle_py.OracleNKA(n_global, m, flavor); one state digest; one red[];
  b  the owned parts assembled into the global vector against the extended-precision trajectory: parity_util's truth rule
     at base 1e-12, and parity_util.finish() at the end of the sequence;
  c  every local output entry, ghosts included, torch.equal to the owner's output entry (at the end the stored w and v of
     every live slot likewise); a twin set of handles whose ghosts hold 1e3 * randn, fresh every call, has the same red[],
     h, c, digest, decisions and owned output bits;
  f  (hook) the counts the in-process hook saw: none on the first update, then [1, 1 + 2 mvec] resp. [2 + 2 mvec];
then, on planted inputs (overlap_layout.planted),
  d  every live red[] entry within gamma(K) sum_r sum|fl(w a) b| of exact_sums.exact_dot of its operands rebuilt from the
     ranks' stored vectors, K = max_r device_k(n_r) + (world - 1); entries beyond the list == 0.0;
and once per process the bit anchors e (unit weights = no weights; one more rank that owns nothing, with ghosts or empty,
first / middle / last = the run without it; trailing ghost tiles = the slices without them; w in {0} u {4^k} = the exact
rescaling) and the life cycle g (restart + new weights = a fresh run; a copy of one rank's handle).
Ends at the first failed check.  NKA_WS_ONLY=name,... restricts the layouts (for a look at one of them; the test never sets
it and counts the lines of all)."""
import os
import sys
import threading
import time
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nka_amd  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
import exact_sums as X  # noqa: E402
import overlap_layout as OL  # noqa: E402
import parity_util as P  # noqa: E402
from _configs3_inproc_worker import RankOrderedHook, in_threads  # noqa: E402
from _sharded_ngpu_worker import small_inputs  # noqa: E402

# layout -> (mvec, flavour, weights set from, the rank whose f is one element off 16-byte alignment)
PLAN = {
    "halo1": (5, 0, "device", 0),
    "halo3": (20, 1, "host", 1),
    "halo512": (33, 2, "device", 2),
    "halo700": (5, 1, "host", 5),
    "ghost_first": (20, 2, "device", 0),         # (the rank that owns nothing is the unaligned one)
    "ghost_mid": (5, 0, "host", 2),
    "ghost_last": (20, 0, "device", 3),
    "empty": (20, 2, "host", 0),
    "shapes": (5, 1, "device", 3),
    "tail_tiles": (5, 2, "host", 1),
}
EXACT_MVEC = {"halo1": 12}      # check d runs at mvec = 5 (the host sums every operand pair exactly), one layout at 12
SUM_MODES = {"auto": nka_amd.SUMS_AUTO, "blocked": nka_amd.SUMS_BLOCKED}
Snap = namedtuple("Snap", "f red h c dec dig")
DEV = None
STREAMS = []


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


class Group:
    """One sharded run: a handle per rank of the layout `ranks`, all through `transport` with the sum mode `sums`.
    weights: "device" / "host" (how nka_hip_set_dot_weights gets them), None = no weights; wvals: the weights per rank
    (default: the layout's 0/1)."""

    def __init__(self, ranks, m, flavor, transport, sums, weights="device", unaligned=None, wvals=None):
        self.ranks, self.world, self.m, self.transport = ranks, len(ranks), m, transport
        assert self.world <= len(STREAMS)
        self.src = [torch.from_numpy(k.src).to(DEV) for k in ranks]
        self.own = [torch.from_numpy(k.w != 0).to(DEV) for k in ranks]
        self.bufs = []
        for r, k in enumerate(ranks):
            off = 1 if r == unaligned else 0
            b = torch.empty(k.src.size + 2, dtype=torch.float64, device=DEV)
            assert b.data_ptr() % 16 == 0
            self.bufs.append(b[off:off + k.src.size])
            assert unaligned != r or (k.src.size > 0 and self.bufs[r].data_ptr() % 16 == 8)
        self.accs = [nka_amd.nka().init(k.src.size, m, flavor=flavor, device=0, stream=STREAMS[r].cuda_stream).set_sum_order(SUM_MODES[sums])
                     for r, k in enumerate(ranks)]
        for r, a in enumerate(self.accs):
            a.set_shard(r, self.world)
        if weights is not None:
            self.set_weights(wvals if wvals is not None else [k.w for k in ranks], weights)
        self.counts = [[] for _ in ranks]
        self.ring = None
        self.attach()
        torch.cuda.synchronize()

    def set_weights(self, wvals, how):
        for a, w in zip(self.accs, wvals):
            a.set_dot_weights(f64(w) if how == "device" else np.ascontiguousarray(w, dtype=np.float64))
            assert a.dot_weighted()              # (the empty rank too: weighted without a buffer)

    def hook_of(self, r):
        inner = self.ring.hook_of(r)

        def hook(ptr, count, stream):
            self.counts[r].append(count)
            inner(ptr, count, stream)
        return hook

    def attach(self):
        if self.transport == "hook":
            if self.ring is None:
                self.ring = RankOrderedHook(self.world, 2 + 2 * self.m + 64, DEV)
            for r, a in enumerate(self.accs):
                a.set_dot_prod(self.hook_of(r))
        else:
            for a in self.accs:
                a.p2p_export(self.world)
            boxes = [a.p2p_mailbox() for a in self.accs]
            for r, a in enumerate(self.accs):
                a.p2p_attach_local(boxes, r)

    def update(self, xg, garbage=None):
        """One accel_update of every rank on its slice of the global device vector xg -> the local outputs.  garbage: one
        torch.Generator per rank: the ghosts hold 1e3 * randn instead of copies of their owners' entries."""
        outs = [None] * self.world
        seen = [len(c) for c in self.counts]
        start = threading.Barrier(self.world)
        torch.cuda.synchronize()

        def step(r):
            s = STREAMS[r]
            with torch.cuda.stream(s):
                f = self.bufs[r]
                loc = xg[self.src[r]]
                if garbage is not None:
                    junk = 1e3 * torch.randn(loc.numel(), generator=garbage[r], dtype=torch.float64, device=DEV)
                    loc = torch.where(self.own[r], loc, junk)
                f.copy_(loc)
                s.synchronize()
                start.wait(timeout=120)
                self.accs[r].accel_update(f)
                s.synchronize()
                outs[r] = f.clone()
                s.synchronize()
        in_threads(self.world, step)
        torch.cuda.synchronize()
        self.last_counts = [c[k:] for c, k in zip(self.counts, seen)]
        return outs

    def snapshot(self, outs, n_global, tag):
        """The replicated state (asserted to BE replicated: one digest, one red[], one set of decisions over the ranks)
        and the global vector assembled from the owned entries."""
        g = torch.empty(n_global, dtype=torch.float64, device=DEV)
        for k, o in zip(self.ranks, outs):
            g[k.lo:k.hi] = o[k.first:k.first + k.hi - k.lo]
        reds = [a.reductions() for a in self.accs]
        digs = [a.state_digest() for a in self.accs]
        sts = [a.state() for a in self.accs]
        decs = [(a.num_vec(), st.list_order(), st.free_order()) for a, st in zip(self.accs, sts)]
        for r in range(1, self.world):
            assert np.array_equal(reds[r], reds[0]), (tag, "red[] differs between ranks", r, reds[r], reds[0])
            assert decs[r] == decs[0], (tag, "decisions differ between ranks", r, decs[r], decs[0])
        assert all(d == digs[0] for d in digs), (tag, "digests", [f"{d:016x}" for d in digs])
        return Snap(g, reds[0], sts[0].h, sts[0].c, decs[0], digs[0])

    def close(self):
        torch.cuda.synchronize()
        if self.transport == "p2p":
            for a in self.accs:
                a.p2p_detach()
        for a in self.accs:
            a.delete()
        self.accs = []


def same(a, b, tag, digest=False, scale=None, red=True, live_only=False):
    """Two snapshots hold the same bits: the assembled owned outputs (a's times `scale` where given), red[], h, c, decisions.
    live_only: h and c at the live slots only (a restarted handle keeps the entries of slots it has not reused yet, and
    the digest covers them)."""
    fa = a.f if scale is None else a.f * scale
    assert torch.equal(fa, b.f), (tag, "owned output bits", int((fa != b.f).sum()), float((fa - b.f).abs().max()))
    assert not red or np.array_equal(a.red, b.red), (tag, "red[]", a.red, b.red)
    if live_only:
        live = [k - 1 for k in a.dec[1][1:]]                 # (the pending pair has no row of the factor yet)
        ix = np.ix_(live, live)
        assert np.array_equal(a.h[ix], b.h[ix]) and np.array_equal(a.c[live], b.c[live]), (tag, "h / c of the live slots")
    else:
        assert np.array_equal(a.h, b.h) and np.array_equal(a.c, b.c), (tag, "h / c")
    assert a.dec == b.dec, (tag, "decisions", a.dec, b.dec)
    if digest:
        assert a.dig == b.dig, (tag, "digest", f"{a.dig:016x}", f"{b.dig:016x}")


def run(group, inputs, n, tag, scale=None):
    snaps = []
    for t, x in enumerate(inputs):
        xg = f64(x)
        if scale is not None:
            xg = xg * scale
        snaps.append(group.snapshot(group.update(xg), n, (tag, t)))
    return snaps


def expected_counts(sums, m, first):
    if first:
        return []
    return [1, 1 + 2 * m] if sums == "auto" else [2 + 2 * m]


# ---- checks a, b, c, f on one layout -----------------------------------------------------------------------------------------

def main_sequence(name, transport, sums, ncu):
    n, world, spec = OL.named(name, ncu)
    ranks = OL.build(n, world, spec)
    m, flavor, how, unal = PLAN[name]
    tag = f"weights sharded {name} x{world} ({transport}, {sums}) n={n} m={m} flavor {flavor}"
    A = Group(ranks, m, flavor, transport, sums, weights=how, unaligned=unal)
    B = Group(ranks, m, flavor, transport, sums, weights="host" if how == "device" else "device", unaligned=unal)
    gens = [torch.Generator(device=DEV).manual_seed(1000 + r) for r in range(world)]
    ora = O.OracleNKA(n, m, flavor)
    spread = P.Spread(O, n, m)
    inputs = small_inputs(n, m + 8, seed=321 + len(name))
    snaps, before, capacity, dependence = [], 0, 0, 0
    for t, x in enumerate(inputs):
        f = x.copy()
        ora.accel_update(f)
        spread.update(x)
        xg = f64(x)
        outs = A.update(xg)
        sa = A.snapshot(outs, n, (tag, t))
        # a. decisions: the plain oracle's on the global vector
        so = ora.state()
        assert sa.dec == (ora.num_vec(), so.list_order(), so.free_order()), (tag, t, "decisions", sa.dec, ora.num_vec(), so.list_order())
        # b. the truth rule on the owned entries
        got = sa.f.cpu().numpy()
        err = float(np.linalg.norm(got - f) / np.linalg.norm(x))
        P.check(err, so, tag, base=1e-12, where=t, spread=spread.value, truth=spread.truth(got, x))
        # c. ghosts are their owners' output bits
        for r, o in enumerate(outs):
            assert torch.equal(o, sa.f[A.src[r]]), (tag, t, "rank", r, "ghost outputs differ from their owners'",
                                                     int((o != sa.f[A.src[r]]).sum()))
        #    ... and garbage at the ghosts changes nothing that counts
        sb = B.snapshot(B.update(xg, garbage=gens), n, (tag, t, "garbage twin"))
        same(sa, sb, (tag, t, "garbage at the ghosts"), digest=True)
        # f. the exchanges
        if transport == "hook":
            want = expected_counts(sums, m, t == 0)
            for G in (A, B):
                assert all(c == want for c in G.last_counts), (tag, t, "exchange counts", G.last_counts, want)
        after = ora.num_vec()
        capacity += before == m
        dependence += after < min(before + 1, m)
        before = after
        snaps.append(sa)
    P.finish()
    # c. at the end: the stored vectors of every live slot
    kept = {}
    for G in (A, B):
        for slot in ora.state().list_order():
            for get in ("w", "v"):
                loc = [f64(getattr(a, get)(slot)) for a in G.accs]
                g = torch.empty(n, dtype=torch.float64, device=DEV)
                for k, o in zip(ranks, loc):
                    g[k.lo:k.hi] = o[k.first:k.first + k.hi - k.lo]
                if G is A:
                    for r, o in enumerate(loc):
                        assert torch.equal(o, g[A.src[r]]), (tag, "stored", get, slot, "rank", r, "ghosts differ from their owners'")
                    kept[(slot, get)] = g
                else:
                    assert torch.equal(g, kept[(slot, get)]), (tag, "garbage twin: stored", get, slot)
    rec = P.WORST[tag]
    # the truth ratio: err_dev over what the rule allows beyond the base, truth_factor x err_ref (1 = all of the allowance)
    ratio = rec["err_dev_exact"] / max(P.truth_factor(n) * rec["err_ref_exact"], 1e-300)
    print(f"{tag}: weights from {how}, rank {unal} unaligned, {len(inputs)} calls, capacity drops {capacity}, dependence drops "
          f"{dependence}, err_dev {rec['err_dev_exact']:.2e} err_ref {rec['err_ref_exact']:.2e} truth ratio {ratio:.3f}", flush=True)
    A.close()
    B.close()
    return ranks, inputs, snaps, ratio, len(inputs)


# ---- check d -----------------------------------------------------------------------------------------------------------------

def exact_sums_sequence(name, transport, sums, ncu, worst):
    n, world, spec = OL.named(name, ncu)
    ranks = OL.build(n, world, spec)
    m = EXACT_MVEC.get(name, 5)
    _, flavor, how, unal = PLAN[name]
    tag = f"exact sums {name} x{world} ({transport}, {sums}) n={n} m={m} flavor {flavor}"
    G = Group(ranks, m, flavor, transport, sums, weights=how, unaligned=unal)
    k = max(X.device_k(q.src.size, ncu, r != unal) for r, q in enumerate(ranks)) + (world - 1)
    rounded = sums == "auto"
    rng = np.random.default_rng(n + world)
    W, prev = {}, None
    wl = [q.w for q in ranks]

    def hold(what, red, A, Bv, where):
        ex = X.exact_dot(np.concatenate(A), np.concatenate(Bv))
        tot = sum(X.abs_dot(a, b) for a, b in zip(A, Bv))
        err = abs(red - ex)
        assert err <= X.gamma(k) * tot, (tag, where, what, red, ex, err / (X.U * tot) if tot else err, k)
        if tot > 0:
            worst[what] = max(worst.get(what, 0.0), err / (X.U * tot))

    for t in range(m + 6):
        x = OL.planted(ranks, n, ncu, rng, prev)
        st0 = G.accs[0].state()
        order0, pending = st0.list_order(), st0.pending
        olders = order0[1:] if pending else order0
        snap = G.snapshot(G.update(f64(x)), n, (tag, t))
        red = snap.red
        loc = [x[q.src] for q in ranks]
        fw = [w * a for w, a in zip(wl, loc)]
        if pending:
            d = [W[order0[0]][r] - loc[r] for r in range(world)]
            dw = [w * a for w, a in zip(wl, d)]
            hold("<wd,d>", red[0], dw, d, t)
            s = np.sqrt(np.float64(red[0]))
            assert s > 0.0, (tag, t)
            w1n = [(np.float64(1.0) / s) * a for a in d] if flavor == 1 else [a / s for a in d]
            if rounded:
                hold("<wf,w1'>", red[1], fw, w1n, t)
                for p, q in enumerate(olders):
                    hold("<ww1',w_p>", red[2 + p], [w * a for w, a in zip(wl, w1n)], W[q], (t, p))
            else:
                hold("<wf,d>", red[1], fw, d, t)
                for p, q in enumerate(olders):
                    hold("<wd,w_p>", red[2 + p], dw, W[q], (t, p))
        for p, q in enumerate(olders):
            hold("<wf,w_p>", red[2 + m + p], fw, W[q], (t, p))
        for p in range(len(olders), m):
            assert red[2 + p] == 0.0 and red[2 + m + p] == 0.0, (tag, t, p, red)
        W = {q: [a.w(q) for a in G.accs] for q in G.accs[0].state().list_order()}
        prev = x
    G.close()
    return k


# ---- e. bit anchors -----------------------------------------------------------------------------------------------------------

def anchor_unit_weights(transport, sums):
    """Unit weights on every rank = the same sharded run without weights."""
    n, m = 200_003, 5
    ranks = OL.build(n, 2)
    inputs = small_inputs(n, m + 5, seed=17)
    for flavor in (0, 1, 2):
        a = Group(ranks, m, flavor, transport, sums, weights="device", unaligned=1)
        b = Group(ranks, m, flavor, transport, sums, weights=None, unaligned=1)
        for t, (sa, sb) in enumerate(zip(run(a, inputs, n, "unit weights"), run(b, inputs, n, "no weights"))):
            same(sa, sb, ("e: unit weights = no weights", transport, sums, flavor, t), digest=True)
        a.close()
        b.close()


def anchor_one_more_rank(transport, sums):
    """W ranks plus one that owns nothing -- 17 ghosts with zero weights, or no elements at all -- first, in the middle
    and last = the W-rank run: adding an exact zero changes no sum."""
    n, m, W = 210_011, 5, 3
    base = OL.build(n, W, {"halo": 3})
    inputs = small_inputs(n, m + 5, seed=23)
    g = Group(base, m, 2, transport, sums, weights="device", unaligned=1)
    ref = run(g, inputs, n, "W ranks")
    g.close()
    for pos in (0, 2, W):
        for kind in ("ghosts", "empty"):
            owned = OL.even_split(n, W)
            owned.insert(pos, 0)
            halo = [(3, 3)] * (W + 1)
            ranks = OL.build(n, W + 1, {"owned": owned, "halo": halo, "ghosts": {pos: 17} if kind == "ghosts" else {}})
            rest = OL.without(ranks, pos)
            assert all(np.array_equal(p.src, q.src) and np.array_equal(p.w, q.w) for p, q in zip(rest, base))
            unal = 1 + (pos <= 1)                                        # the same slice as in the W-rank run
            g = Group(ranks, m, 2, transport, sums, weights="host", unaligned=unal)
            got = run(g, inputs, n, f"W + 1 ranks ({kind} at {pos})")
            for t, (sa, sb) in enumerate(zip(got, ref)):
                same(sa, sb, ("e: one more rank that owns nothing", kind, pos, transport, sums, t))
            if transport == "hook":
                assert all(c == g.counts[0] for c in g.counts), ("exchange counts differ on the rank that owns nothing", kind, pos)
            g.close()


def anchor_tail_tiles(transport, sums, ncu, ranks, inputs, snaps):
    """The trailing-ghost-tiles layout = the plain sharded run on the slices without their ghost tiles, at the owned
    entries: the ghost tiles add exact zeros at the END of each block's chain, where both runs take the same grids."""
    n = OL.named("tail_tiles", ncu)[0]
    m, flavor, _, unal = PLAN["tail_tiles"]
    plain = OL.build(n, len(ranks), {"owned": [k.hi - k.lo for k in ranks]})
    for r, (k, p) in enumerate(zip(ranks, plain)):
        assert X.pass_grids(k.src.size, ncu, r != unal) == X.pass_grids(p.src.size, ncu, r != unal), (r, k.src.size, p.src.size)
    g = Group(plain, m, flavor, transport, sums, weights=None, unaligned=unal)
    for t, (sa, sb) in enumerate(zip(snaps, run(g, inputs, n, "slices without ghost tiles"))):
        same(sa, sb, ("e: trailing ghost tiles", transport, sums, t))
    g.close()


def anchor_powers_of_four(transport, sums):
    """w in {0} u {4^k}: 2^-k o (the 0/1-masked sharded run on 2^k o f), bit for bit."""
    n, m = 240_007, 5
    ranks = OL.build(n, 3, {"halo": 3})
    rng = np.random.default_rng(4)
    kexp = rng.integers(-6, 7, size=n)
    sc = f64(np.ldexp(1.0, kexp))
    inputs = small_inputs(n, m + 5, seed=29)
    for flavor in (2, 1):
        a = Group(ranks, m, flavor, transport, sums, weights="host", unaligned=0,
                  wvals=[q.w * np.ldexp(1.0, 2 * kexp[q.src]) for q in ranks])
        b = Group(ranks, m, flavor, transport, sums, weights="device", unaligned=0)
        sa_all = run(a, inputs, n, "w = 4^k")
        sb_all = run(b, inputs, n, "masked run on 2^k o f", scale=sc)
        for t, (sa, sb) in enumerate(zip(sa_all, sb_all)):
            same(sa, sb, ("e: powers of four", transport, sums, flavor, t), scale=sc)
        a.close()
        b.close()


# ---- g. life cycle -------------------------------------------------------------------------------------------------------------

def life_cycle(transport, sums):
    n, m, flavor = 230_003, 5, 2
    ranks = OL.build(n, 3, {"halo": 3})
    ranks2 = OL.moved(ranks, 2, n)
    inputs = small_inputs(n, 6 + 8 + 4, seed=31)
    a = Group(ranks, m, flavor, transport, sums, weights="device", unaligned=2)
    run(a, inputs[:6], n, "before the restart")
    for acc in a.accs:
        acc.restart()
    a.set_weights([q.w for q in ranks2], "host")
    a.ranks = ranks2
    a.own = [torch.from_numpy(q.w != 0).to(DEV) for q in ranks2]
    b = Group(ranks2, m, flavor, transport, sums, weights="device", unaligned=2)
    for t, (sa, sb) in enumerate(zip(run(a, inputs[6:14], n, "restarted"), run(b, inputs[6:14], n, "fresh"))):
        # (the first update after a restart forms no sums: red[] still holds what the last update before it left)
        same(sa, sb, ("g: restart + new weights = a fresh weighted run", transport, sums, t), red=t > 0, live_only=True)
        if transport == "hook":
            assert a.last_counts == b.last_counts
    # a copy of rank 1's handle, swapped in for the original
    old = a.accs[1]
    c = old.copy()
    assert c.dot_weighted()
    if transport == "p2p":
        # (a caller's hook travels with the copy, as the reference's dp does; the mailboxes do not: nka_hip_clone)
        probe = torch.zeros(ranks2[1].src.size, dtype=torch.float64, device=DEV)
        try:
            c.accel_update(probe)
            raise AssertionError("g: the copy of a sharded handle ran without an all-reduce of its own")
        except nka_amd.NKAError as exc:
            assert "no all-reduce yet" in str(exc), str(exc)
        old.p2p_detach()
    a.accs[1] = c
    a.attach()                       # collectively: new mailboxes (p2p) / the rank's hook (hook)
    for t, (sa, sb) in enumerate(zip(run(a, inputs[14:], n, "with the copy"), run(b, inputs[14:], n, "fresh"))):
        same(sa, sb, ("g: the copy continues the run", transport, sums, t), live_only=True)
    old.delete()
    a.close()
    b.close()


def main():
    global DEV
    transport = os.environ.get("NKA_WS_TRANSPORT", "hook")
    sums = os.environ.get("NKA_WS_SUMS", "auto")
    only = [v for v in os.environ.get("NKA_WS_ONLY", "").split(",") if v]
    names = [nm for nm in OL.NAMES if not only or nm in only]
    torch.cuda.set_device(0)
    DEV = torch.device("cuda", 0)
    STREAMS.extend(torch.cuda.Stream(device=DEV) for _ in range(9))
    assert len({s.cuda_stream for s in STREAMS}) == len(STREAMS)
    probe = nka_amd.nka().init(1, 1)
    ncu = probe.device_info()[1]
    probe.delete()
    t0 = time.time()
    calls, ratio, worst, kmax = 0, 0.0, {}, 0
    for nm in names:
        ranks, inputs, snaps, r, c = main_sequence(nm, transport, sums, ncu)
        calls, ratio = calls + c, max(ratio, r)
        if nm == "tail_tiles":
            anchor_tail_tiles(transport, sums, ncu, ranks, inputs, snaps)
        del snaps
        kmax = max(kmax, exact_sums_sequence(nm, transport, sums, ncu, worst))
        calls += EXACT_MVEC.get(nm, 5) + 6
        torch.cuda.empty_cache()
        print(f"  {nm} done at {time.time() - t0:.0f} s", flush=True)
    if not only or "anchors" in only:
        anchor_unit_weights(transport, sums)
        anchor_one_more_rank(transport, sums)
        anchor_powers_of_four(transport, sums)
        life_cycle(transport, sums)
    sums_txt = ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items()))
    print(f"WEIGHTS SHARDED PAIR {transport} {sums}: {calls} calls; layouts {','.join(names)}; worst truth ratio {ratio:.3f}; "
          f"worst err / (u sum|ab|): {sums_txt} (K <= {kmax}); anchors and life cycle {'run' if not only or 'anchors' in only else 'NOT run'}; "
          f"{time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    main()
