"""Both batch kernels beyond 4 GiB and beyond 2^31 elements (include/nka_hip_batch.h, LIMITS: every offset is 64-bit).

Six batches of 17 ... 35 GB in which a handful of systems run and all others are masked out -- a masked system has no byte read
or written, so such a batch costs its allocation, one memset at creation and a few workgroups per update.  The shapes, the
systems that run and the witnesses are arithmetic (tests/batch_large.py, held by tests/test_batch_large_cpu.py).

THE TWIN: one batch of the same kind, flavour, explicit sum order, vlen and mvec with as many systems as run; its system j is
fed what system active[j] of the large batch is fed, call by call.  Results do not depend on nsys, on a system's position, on ld
or on masks (BITS), so EVERY comparison here is ==; there is no tolerance in this file.  What the twins themselves compute is
held to the exact sums, the oracle's scalar step and numpy elsewhere (test_batch_sums_exact_gpu.py, test_batch_wide_gpu.py,
test_batch_step_gpu.py, test_batch_lengths_gpu.py): this file adds the addresses.

After every call, for every system that runs: its row of F (and X), red[], the state, num_vec, the digest, w and v of the slots
in list order -- of every slot at the last call --, fnorm and the mask where there is a step.  Once at the end: num_vec of every
system that never ran is 0; the witnesses (where an offset that lost its upper bits would have landed) still carry the digest of
a fresh batch and slots of zeros; and every element of F and X that no running system owns is still PAD."""
import time

import numpy as np
import pytest

import batch_large as G
import batch_lengths as BL
import batch_seq as B
from split_update import _bits_equal

pytestmark = pytest.mark.gpu

PIECE = 2 ** 26      # elements per piece of the final sweep over F and X: no temporary above 1 GiB


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _same_system(a, ka, b, kb, where, slots):
    """System ka of batch a against system kb of batch b, bit for bit (the model: tests/test_batch_lengths_gpu.py)."""
    assert _bits_equal(a.reductions(ka), b.reductions(kb)), (where, "red[]", a.reductions(ka), b.reductions(kb))
    sa, sb = a.state(ka), b.state(kb)
    assert sa.list_order() == sb.list_order() and sa.free_order() == sb.free_order(), (where, "list", sa.list_order(), sb.list_order())
    assert (sa.subspace, sa.pending, sa.first, sa.last, sa.free) == (sb.subspace, sb.pending, sb.first, sb.last, sb.free), (where, "state")
    assert _bits_equal(sa.h, sb.h) and _bits_equal(sa.c, sb.c), (where, "h, c")
    assert a.state_digest(ka) == b.state_digest(kb), (where, "digest")
    for s in (range(1, a.max_vec() + 2) if slots == "all" else sa.list_order()):
        assert BL.same_bytes(a.w(ka, s), b.w(kb, s)), (where, "w", s)
        assert BL.same_bytes(a.v(ka, s), b.v(kb, s)), (where, "v", s)


class Large:
    """The large batch of a shape beside its twin.  close() frees everything; the tests call it in a `finally`."""

    def __init__(self, torch, sid):
        self.torch, self.sh = torch, G.SHAPES[sid]
        sh = self.sh
        self.active = G.active_set(sh)
        self.na = len(self.active)
        self.b = self.t = self.mask = self.tmask = self.idx = None
        self.raw, self.rows, self.trows, self.host, self.misc = {}, {}, {}, {}, {}
        try:
            self._create(sid)
        except BaseException:
            self.close()
            raise

    def _create(self, sid):
        import nka_amd
        torch, sh = self.torch, self.sh
        need = G.total_bytes(sh)
        free, total = torch.cuda.mem_get_info()
        if free < need + (8 << 30):
            pytest.skip(f"{sid}: {free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB free, the test needs {need / 2**30:.1f} GiB + 8 GiB")
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()
        wide = sh.kind == "wide"
        if wide:
            assert nka_amd.batch_wide_limits()[0] == G.WIDE_CHUNK, "the shapes were worked out for another chunk"
        self.b = nka_amd.nka_batch().init(sh.nsys, sh.vlen, sh.mvec, wide=wide)
        self.t = nka_amd.nka_batch().init(self.na, sh.vlen, sh.mvec, wide=wide)
        assert self.b.is_wide() == wide == self.t.is_wide() and self.b.flavor() == self.t.flavor()
        if not wide:
            self.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        self.fresh_digest = self.b.state_digest(G.witnesses(sh)[0])
        assert self.fresh_digest == nka_amd.nka_batch().init(1, sh.vlen, sh.mvec, wide=wide).state_digest(0)
        for name, ld in (("F", sh.ld), ("X", sh.ldx)):
            if name == "X" and not sh.with_x:
                continue
            self.raw[name] = torch.full((G.span(sh, name),), G.PAD, dtype=torch.float64, device="cuda")
            self.rows[name] = torch.as_strided(self.raw[name], (sh.nsys, sh.vlen), (ld, 1))
            self.trows[name] = torch.zeros(self.na, sh.vlen, dtype=torch.float64, device="cuda")
            self.host[name] = [None] * self.na
        self.mask = torch.zeros(sh.nsys, dtype=torch.int32, device="cuda")
        self.tmask = torch.ones(self.na, dtype=torch.int32, device="cuda")
        self.idx = torch.tensor(self.active, dtype=torch.int64, device="cuda")
        self.mask[self.idx] = 1
        self.lens = [sh.vlen] * self.na
        self.ran = np.zeros(self.na, np.int64)      # updates that ran, per system

    def set_sum_order(self, order):
        self.b.set_sum_order(order)
        self.t.set_sum_order(order)

    def close(self):
        for a in (self.b, self.t):
            if a is not None:
                a.delete()
        self.b = self.t = None
        self.raw.clear(), self.rows.clear(), self.trows.clear(), self.misc.clear()
        self.mask = self.tmask = self.idx = None
        self.torch.cuda.empty_cache()

    # ---- inputs ----
    def write(self, name, rows):
        """rows[j]: the whole row (vlen doubles) of active system j, in the large batch and the twin alike."""
        for j, k in enumerate(self.active):
            x = self.torch.from_numpy(np.ascontiguousarray(rows[j])).cuda()
            self.rows[name][k].copy_(x)
            self.trows[name][j].copy_(x)
            self.host[name][j] = rows[j]

    def padded(self, xs, salt):
        """xs[j] of lens[j] elements -> whole rows whose tails are NaNs of distinct payloads (nothing from lens[j] on is read)."""
        paint = BL.nan_paint(self.na, self.sh.vlen, salt)
        for j, x in enumerate(xs):
            paint[j, :self.lens[j]] = x[:self.lens[j]]
        return paint

    def sub_masks(self, js):
        m, tm = self.torch.zeros_like(self.mask), self.torch.zeros_like(self.tmask)
        sel = self.idx[self.torch.tensor(js, device="cuda")]
        m[sel] = 1
        tm[self.torch.tensor(js, device="cuda")] = 1
        return m, tm

    def relax(self, js):
        m, tm = self.sub_masks(js)
        self.b.relax(m)
        self.t.relax(tm)

    def restart(self, js=None):
        m, tm = self.sub_masks(list(range(self.na)) if js is None else js)
        self.b.restart(m)
        self.t.restart(tm)

    def set_lengths(self):
        """The lengths of the second pass on the systems that run, vlen on all others; the twin gets the same ones."""
        full = G.lengths(self.sh, self.active)
        self.lens = [full[k] for k in self.active]
        self.b.set_lengths(np.array(full, np.int32))
        self.t.set_lengths(np.array(self.lens, np.int32))
        assert self.b.has_lengths() and self.t.has_lengths()

    # ---- calls ----
    def update(self, where, rows, slots="list"):
        self.write("F", rows)
        self.b.accel_update(self.rows["F"], self.mask)
        self.t.accel_update(self.trows["F"], self.tmask)
        self.ran += 1
        self.compare(where, slots)

    def step(self, where, rows, with_tol, slots="list", with_fnorm=True):
        """accel_step with X and the mask; with_fnorm: fnorm too; with_tol: tol too, half the fnorm of the last call without."""
        torch = self.torch
        if with_fnorm and "fnorm" not in self.misc:
            self.misc["fnorm"] = torch.full((self.sh.nsys,), -1.0, dtype=torch.float64, device="cuda")
            self.misc["tfnorm"] = torch.full((self.na,), -1.0, dtype=torch.float64, device="cuda")
        if not with_tol:
            self.misc.pop("tol", None)
        elif "tol" not in self.misc:                 # formed on the device from what the call before left in fnorm
            self.misc["tol"] = 0.5 * self.misc["fnorm"]
            self.misc["ttol"] = 0.5 * self.misc["tfnorm"]
        self.write("F", rows)
        before = self.tmask.cpu().numpy().copy()
        fn, tfn = (self.misc["fnorm"], self.misc["tfnorm"]) if with_fnorm else (None, None)
        tol, ttol = (self.misc["tol"], self.misc["ttol"]) if with_tol else (None, None)
        self.b.accel_step(self.rows["F"], self.rows["X"], self.mask, tol, fn)
        self.t.accel_step(self.trows["F"], self.trows["X"], self.tmask, ttol, tfn)
        got, want = self.mask[self.idx].cpu().numpy(), self.tmask.cpu().numpy()
        assert np.array_equal(got, want), (where, "mask", got, want)
        if with_fnorm:
            assert BL.same_bytes(fn[self.idx].cpu().numpy(), tfn.cpu().numpy()), (where, "fnorm")
        self.ran += before * want
        self.compare(where, slots)

    def compare(self, where, slots):
        nv, tnv = self.b.num_vec(), self.t.num_vec()
        for j, k in enumerate(self.active):
            at = where + ("system", k)
            for name in self.rows:
                got, want = self.rows[name][k].cpu().numpy(), self.trows[name][j].cpu().numpy()
                assert BL.same_bytes(got, want), (at, name, int(np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[0]))
                L = self.lens[j]      # nothing from the system's own length on is written
                assert BL.same_bytes(got[L:], self.host[name][j][L:]), (at, name, "the tail was written")
            assert nv[k] == tnv[j], (at, "num_vec", nv[k], tnv[j])
            _same_system(self.b, k, self.t, j, at, slots)

    # ---- once, at the end ----
    def finish(self, where):
        torch, sh = self.torch, self.sh
        self.compare(where + ("every slot",), "all")
        nv = self.b.num_vec()
        idle = np.ones(sh.nsys, bool)
        idle[self.active] = False
        assert (nv[idle] == 0).all(), (where, "a system that never ran holds vectors", np.flatnonzero(idle & (nv != 0))[:8])
        for k in G.witnesses(sh):
            assert self.b.state_digest(k) == self.fresh_digest, (where, "witness", k, "digest")
            for s in range(1, sh.mvec + 2):
                assert not self.b.w(k, s).any() and not self.b.v(k, s).any(), (where, "witness", k, "slot", s)
        got = self.mask.cpu().numpy()
        assert (got[idle] == 0).all(), (where, "the mask of a system that never ran was written")
        if "fnorm" in self.misc:
            assert (self.misc["fnorm"].cpu().numpy()[idle] == -1.0).all(), (where, "fnorm of a system that never ran was written")
        # F and X: what the running systems own is compared above; paint it over, and everything is PAD again
        for name, raw in self.raw.items():
            for k in self.active:
                self.rows[name][k].fill_(G.PAD)
            ok = torch.ones((), dtype=torch.bool, device="cuda")
            for lo in range(0, raw.numel(), PIECE):
                ok &= (raw[lo:lo + PIECE] == G.PAD).all()
            if not bool(ok.item()):
                for lo in range(0, raw.numel(), PIECE):
                    bad = torch.nonzero(raw[lo:lo + PIECE] != G.PAD)
                    assert bad.numel() == 0, (where, name, "element", lo + int(bad[0]), "of no running system was written")
        wall = time.perf_counter() - self.t0
        peak = torch.cuda.max_memory_allocated() + G.batch_bytes(sh)
        print(f"batch_large {sh.id}: nsys {sh.nsys}, {self.na} systems ran; wall {wall:.2f} s; peak device memory {peak / 1e9:.1f} GB "
              f"(tensors {torch.cuda.max_memory_allocated() / 1e9:.1f} GB + the batch's own {G.batch_bytes(sh) / 1e9:.1f} GB)")


def _sequences(L, seed):
    return [B.Sequence(L.sh.vlen, seed + 31 * j) for j in range(L.na)]


def _weights(L, raw_rows):
    """Ones everywhere; on the rows of the systems that run, powers of two that differ from row to row and along the row.
    -> the rows of the twin (na x vlen)."""
    i = np.arange(L.sh.vlen)
    tw = np.stack([np.ldexp(1.0, 1 + j + (i + j) % 3) for j in range(L.na)])
    for j, k in enumerate(L.active):
        raw_rows[k].copy_(L.torch.from_numpy(tw[j]).cuda())
    return tw


def _fill_the_lists(L, rng, where, calls=36, relax_at=20):
    """`calls` updates on fresh independent inputs with a masked relax partway: the lists fill to mvec = 32, every slot 1 ... 33 is
    written, and from the 34th update on the oldest vector goes."""
    for c in range(calls):
        if c == relax_at:
            L.relax(list(range(0, L.na, 2)))
        L.update(where + ("call", c), L.padded([rng.standard_normal(L.sh.vlen) for _ in range(L.na)], 1))
    nv = L.b.num_vec()
    assert (nv[L.active] == L.sh.mvec).all() and L.sh.mvec == 32, (where, nv[L.active])


# ---- narrow ---------------------------------------------------------------------------------------------------------------------

def test_bytes_every_stream_beyond_4_gib(torch_cuda):
    """32 800 systems of 16 384, mvec = 1: the slots, F (ld 16 385), X (ldx 16 387), the batch's weight buffer and the caller's
    weight rows all pass 2^32 bytes; rows 32 766 of F and 32 762 of X straddle it.  A weighted step with X, mask, tol and fnorm
    in fast sums (7 calls, tol = fnorm of the first call / 2 formed on the device, a masked relax and a masked restart partway); then reference order
    (3 calls: the chains on threads 0, 1 and 64); then, after a restart, per-system lengths -- vlen - 1 and 513 among them -- for
    4 calls in reference order and 2 in fast sums."""
    import nka_amd
    torch = torch_cuda
    L = Large(torch, "bytes")
    try:
        sh = L.sh
        L.raw["wsrc"] = torch.ones(G.span(sh, "wsrc"), dtype=torch.float64, device="cuda")
        wrows = torch.as_strided(L.raw["wsrc"], (sh.nsys, sh.vlen), (sh.ldw, 1))
        tw = _weights(L, wrows)
        L.b.set_dot_weights(wrows)
        L.t.set_dot_weights(tw)
        assert L.b.dot_weighted() and L.t.dot_weighted()
        del L.raw["wsrc"], wrows      # (copied by the set; F and X alone are swept at the end)
        rng = np.random.default_rng(41)
        L.write("X", [rng.standard_normal(sh.vlen) for _ in range(L.na)])
        seqs = _sequences(L, 4150)      # (chosen on the CPU, from the inputs alone: see the asserts on L.ran)
        for c in range(7):
            if c == 3:
                L.relax([1, 4, 6])
            if c == 5:
                L.restart([0, 4, 8])
            L.step(("fast", "call", c), [s.next() for s in seqs], with_tol=c > 0)
        # (an input of less than half the first one's norm retires a system: one goes at call 5, none before)
        assert L.ran.min() >= 4 and L.ran.max() == 7 and (L.ran < 7).any(), L.ran
        ran = L.ran.copy()
        # reference order, every system in again
        L.mask[L.idx] = 1
        L.tmask.fill_(1)
        L.restart()
        L.set_sum_order(nka_amd.SUMS_REFERENCE_ORDER)
        for c in range(3):
            L.step(("reference order", "call", c), [s.next() for s in seqs], with_tol=True)
        assert (L.ran - ran == 3).all(), L.ran - ran
        ran = L.ran.copy()
        # lengths
        L.mask[L.idx] = 1
        L.tmask.fill_(1)
        L.restart()
        L.set_lengths()
        assert sh.vlen - 1 in L.lens and 513 in L.lens
        L.write("X", L.padded([rng.standard_normal(sh.vlen) for _ in range(L.na)], 2))
        for c in range(6):
            if c == 4:
                L.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
            L.step(("lengths", "call", c), L.padded([s.next() for s in seqs], 1), with_tol=c > 0)      # (tol anew: other lengths)
        assert (L.ran - ran >= 4).all(), L.ran - ran
        L.finish(("bytes",))
    finally:
        L.close()


def test_slots_beyond_2_to_the_31_elements(torch_cuda):
    """3976 systems of 16 384, mvec = 32: system 3971 starts 475 136 elements below 2^31 in w and v, so its slots 1 ... 29 lie
    below the boundary and 30 ... 33 at or above it; system 992 straddles 2^32 bytes.  36 updates on fresh inputs fill the lists
    to 32 and write every slot; then dependent, repeated and zero inputs, a masked restart, and three more."""
    L = Large(torch_cuda, "slots")
    try:
        _fill_the_lists(L, np.random.default_rng(42), ("slots",))
        seqs = _sequences(L, 4200)
        for c in range(3):
            L.update(("slots", "mixed", c), [s.next() for s in seqs])
        L.restart([0, 2, 5])
        for c in range(3):
            L.update(("slots", "after the restart", c), [s.next() for s in seqs])
        L.finish(("slots",))
    finally:
        L.close()


def test_rows_beyond_2_to_the_31_elements(torch_cuda):
    """2052 systems of 4099, mvec = 3, ld = 2^20 - 1 and ldx = 2^20 - 2: row 2048 of F covers [2^31 - 2048, 2^31 + 2051), row 2048
    of X [2^31 - 4096, 2^31 + 3), rows 512 straddle 2^32 bytes, and the odd ld alternates the 16-byte alignment of the rows.  A
    plain step with X over 9 calls: the lists fill at the fourth."""
    L = Large(torch_cuda, "rows")
    try:
        rng = np.random.default_rng(43)
        L.write("X", [rng.standard_normal(L.sh.vlen) for _ in range(L.na)])
        seqs = _sequences(L, 4300)
        for c in range(9):
            if c == 4:
                L.relax([1, 3, 5])
            if c == 6:
                L.restart([0, 5])
            L.step(("rows", "call", c), [s.next() for s in seqs], with_tol=False, with_fnorm=False)
        assert (L.b.num_vec()[L.active] >= 1).all()
        L.finish(("rows",))
    finally:
        L.close()


def test_weight_rows_of_the_caller_beyond_2_to_the_31_elements(torch_cuda):
    """2052 weight rows of 4099 at ldw = 2^20 - 1: k_batch_check_weights and k_batch_copy_weights index the caller's memory with
    (e / n) ldw beyond 2^31 elements.  The rows are ones except on the systems that run, so a row read from elsewhere shows."""
    torch = torch_cuda
    L = Large(torch, "wsrc")
    try:
        sh = L.sh
        L.raw["wsrc"] = torch.ones(G.span(sh, "wsrc"), dtype=torch.float64, device="cuda")
        wrows = torch.as_strided(L.raw["wsrc"], (sh.nsys, sh.vlen), (sh.ldw, 1))
        tw = _weights(L, wrows)
        L.b.set_dot_weights(wrows)
        L.t.set_dot_weights(tw)
        assert L.b.dot_weighted() and L.t.dot_weighted()
        del L.raw["wsrc"], wrows
        seqs = _sequences(L, 4400)
        for c in range(8):
            if c == 3:
                L.relax([2, 4])
            if c == 5:
                L.restart([1, 5])
            L.update(("wsrc", "call", c), [s.next() for s in seqs])
        assert (L.b.num_vec()[L.active] >= 1).all()
        L.finish(("wsrc",))
    finally:
        L.close()


# ---- wide -----------------------------------------------------------------------------------------------------------------------

def test_wide_slots_beyond_2_to_the_31_elements(torch_cuda):
    """14 030 wide systems of 4609 (three chunks), mvec = 32: system 14 024 starts 128 768 elements below 2^31 in w and v, inside
    its slot 28; system 3506 straddles 2^32 bytes.  36 updates on fresh inputs fill the lists and write every slot; then a restart
    and the same with per-system lengths (vlen, 2 C + 1, C + 513, ...): the _len kernels hold their own copy of every address."""
    L = Large(torch_cuda, "wide-slots")
    try:
        _fill_the_lists(L, np.random.default_rng(45), ("wide-slots",))
        L.restart()
        L.set_lengths()
        _fill_the_lists(L, np.random.default_rng(46), ("wide-slots", "lengths"))
        L.finish(("wide-slots",))
    finally:
        L.close()


def test_wide_rows_beyond_2_to_the_31_elements(torch_cuda):
    """2052 wide systems of 4609, mvec = 3, ld = 2^20 - 1: row 2048 of F passes 2^31 elements where its chunk 1 begins (sys ld +
    lo), row 512 straddles 2^32 bytes.  8 calls without lengths, then a restart and 8 with."""
    L = Large(torch_cuda, "wide-rows")
    try:
        seqs = _sequences(L, 4600)
        for lengths in (False, True):
            if lengths:
                L.restart()
                L.set_lengths()
            for c in range(8):
                if c == 3:
                    L.relax([1, 3, 5])
                if c == 5:
                    L.restart([0, 4])
                L.update(("wide-rows", "lengths" if lengths else "full", "call", c), L.padded([s.next() for s in seqs], 1))
            assert (L.b.num_vec()[L.active] >= 1).all()
        L.finish(("wide-rows",))
    finally:
        L.close()
