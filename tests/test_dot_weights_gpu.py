"""Diagonal dot-product weights (nka_hip_set_dot_weights, include/nka_hip.h): the exact consequences the header states, on
the MI355X.  w == 1 gives a plain handle's bits; w = 4^k gives 2^-k o (a plain run on 2^k o f) bit for bit; w = 0 removes an
entry from every sum; a captured update reads the handle's weight buffer at replay; the refused combinations leave the
handle as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_BIG = 2 * 256 * 2 * 1024 + 37        # several grid strides of every pass (the norm pass's look-ahead loop too), a ragged tail
WIDTHS = [1, 5, 20, 23, 31, 32, 40]    # prime rings, the widest window, one list of balanced passes


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _inputs(n, count, seed):
    """`count` normal vectors of n elements on the device (drawn there: the host would take longer than the updates)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(n, generator=g, dtype=torch.float64, device="cuda") for _ in range(count)]


def _buf(torch, x, offset):
    """A copy of x, 16-byte aligned (offset 0) or one element off (offset 1)."""
    b = torch.empty(x.numel() + offset, dtype=torch.float64, device="cuda")
    t = b[offset:]
    t.copy_(x)
    return t


def _decisions(a):
    st = a.state()
    return a.num_vec(), st.list_order(), st.free_order()


def _same_state(a, b):
    sa, sb = a.state(), b.state()
    np.testing.assert_array_equal(sa.h, sb.h)
    np.testing.assert_array_equal(sa.c, sb.c)
    assert _decisions(a) == _decisions(b)


@pytest.mark.parametrize("order", [3, 2], ids=["rounded", "blocked"])
@pytest.mark.parametrize("flavor", [0, 1, 2], ids=["f08", "f08vec", "c"])
def test_unit_weights_give_the_plain_bits(torch_cuda, flavor, order):
    """1. w == 1: f after every update, every red[] entry, h and c equal a plain handle's; aligned and one element off,
    list widths across 1..32 and one list of 40, plus the out-of-place entry."""
    import nka_amd
    torch = torch_cuda
    n = N_BIG
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    for m in WIDTHS:
        for offset in (0, 1):
            X = _inputs(n, m + 3, 100 * m + offset + 7 * flavor)
            p = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order)
            w = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(ones)
            assert w.dot_weighted() and not p.dot_weighted()
            for x in X:
                fp, fw = _buf(torch, x, offset), _buf(torch, x, offset)
                p.accel_update(fp)
                w.accel_update(fw)
                assert torch.equal(fp, fw), (m, offset)
                np.testing.assert_array_equal(p.reductions(), w.reductions())
            _same_state(p, w)
    # the out-of-place entry
    m = 20
    X = _inputs(n, m + 3, 99 + flavor)
    p = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order)
    w = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(ones)
    for x in X:
        _, ap = p.accel_update_swap(x.clone())
        _, aw = w.accel_update_swap(x.clone())
        assert torch.equal(ap, aw)
        np.testing.assert_array_equal(p.reductions(), w.reductions())
    _same_state(p, w)


def _pow4_case(torch, n, m, flavor, order, offset, seed, steps):
    import nka_amd
    rng = np.random.default_rng(seed)
    k = rng.integers(-6, 7, size=n)
    wgt = np.ldexp(1.0, 2 * k)                    # 4^k
    sc = torch.from_numpy(np.ldexp(1.0, k)).cuda()    # 2^k
    X = _inputs(n, steps, seed + 1)
    a = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(wgt)      # (the host entry)
    b = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order)
    for x in X:
        fa = _buf(torch, x, offset)
        fb = _buf(torch, x, offset)
        fb.mul_(sc)
        a.accel_update(fa)
        b.accel_update(fb)
        assert torch.equal(fa * sc, fb)
        np.testing.assert_array_equal(a.reductions(), b.reductions())
        assert _decisions(a) == _decisions(b)
    _same_state(a, b)
    scn = sc.cpu().numpy()
    for slot in a.state().list_order():
        np.testing.assert_array_equal(a.w(slot) * scn, b.w(slot))
        np.testing.assert_array_equal(a.v(slot) * scn, b.v(slot))


@pytest.mark.parametrize("order", [3, 2], ids=["rounded", "blocked"])
@pytest.mark.parametrize("flavor", [0, 1, 2], ids=["f08", "f08vec", "c"])
def test_powers_of_four_are_an_exact_rescaling(torch_cuda, flavor, order):
    """2. w_i = 4^k_i, k in [-6, 6]: a weighted run on f equals 2^-k o (a plain run on 2^k o f), bit for bit: f, every red[]
    entry, h, c, the stored w and v of every live slot, and the decisions."""
    n = 300_037
    for m in WIDTHS:
        for offset in (0, 1):
            _pow4_case(torch_cuda, n, m, flavor, order, offset, 1000 + 10 * m + offset + 3 * flavor, m + 3)


def test_powers_of_four_at_full_size(torch_cuda):
    _pow4_case(torch_cuda, 20_000_003, 20, 2, 3, 0, 4242, 24)


@pytest.mark.parametrize("order", [3, 2], ids=["rounded", "blocked"])
def test_masked_entries_do_not_reach_any_sum(torch_cuda, order):
    """3. w in {0, 1} with ~30 % zeros: two runs that differ only by finite garbage at the masked entries give the same bits
    at every unmasked entry, the same red[], h, c and decisions."""
    import nka_amd
    torch = torch_cuda
    n, m = N_BIG, 20
    rng = np.random.default_rng(3)
    mask = (rng.random(n) >= 0.3).astype(np.float64)
    keep = torch.from_numpy(mask != 0).cuda()
    X = _inputs(n, m + 5, 33)
    for flavor in (0, 1, 2):
        a = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(torch.from_numpy(mask).cuda())
        b = nka_amd.nka().init(n, m, flavor=flavor).set_sum_order(order).set_dot_weights(mask)
        for i, x in enumerate(X):
            y = torch.where(keep, x, 1e3 * torch.randn_like(x))
            fa, fb = _buf(torch, x, 0), _buf(torch, y, 0)
            a.accel_update(fa)
            b.accel_update(fb)
            assert torch.equal(fa[keep], fb[keep]), i
            np.testing.assert_array_equal(a.reductions(), b.reductions())
            assert _decisions(a) == _decisions(b)
        _same_state(a, b)


def test_capture_replays_read_the_weight_buffer(torch_cuda):
    """7. A weighted update captured once capture_safe() holds replays like an eager twin; new weight values set between
    replays reach the next replay; setting weights while the stream is capturing is refused."""
    import nka_amd
    torch = torch_cuda
    n, m = 200_003, 5
    rng = np.random.default_rng(7)
    w1 = rng.uniform(0.125, 8.0, n)
    w2 = rng.uniform(0.125, 8.0, n)
    X = _inputs(n, m + 14, 77)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        acc = nka_amd.nka().init(n, m).set_dot_weights(w1)
        twin = nka_amd.nka().init(n, m).set_dot_weights(w1)
    static = torch.empty(n, dtype=torch.float64, device="cuda")
    it = iter(X)

    def eager(x):
        with torch.cuda.stream(side):
            t = x.clone()
            twin.accel_update(t)
        torch.cuda.synchronize()
        return t

    with torch.cuda.stream(side):
        for _ in range(m + 3):
            x = next(it)
            static.copy_(x)
            acc.accel_update(static)
            assert torch.equal(static, eager(x))
    torch.cuda.synchronize()
    assert acc.capture_safe()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        acc.accel_update(static)
        with pytest.raises(nka_amd.NKAError):
            acc.set_dot_weights(w2)              # refused while capturing
    assert acc.dot_weighted()
    for step in range(5 + 5):
        if step == 5:                            # new values: the next replays run with them
            acc.set_dot_weights(w2)
            twin.set_dot_weights(w2)
        x = next(it)
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager(x)), step
    _same_state(acc, twin)


def test_refusals_and_lifecycle(torch_cuda):
    """8. Invalid weights are refused and the old weighting stays; a short buffer is refused; REFERENCE_ORDER and the host
    dot product are refused in both orders; AUTO at n <= 64 takes the rounded passes; a clone carries the weights; clearing
    them and restarting gives a fresh plain handle's bits."""
    import nka_amd
    from nka_amd.nka import NKAError, SUMS_BLOCKED_ROUNDED, SUMS_REFERENCE_ORDER
    torch = torch_cuda
    n, m = 100_003, 6
    rng = np.random.default_rng(8)
    wgt = rng.uniform(0.125, 8.0, n)
    X = _inputs(n, 3 * m, 88)

    def run(h, xs):
        out = []
        for x in xs:
            t = x.clone()
            h.accel_update(t)
            out.append(t)
        return out

    a = nka_amd.nka().init(n, m).set_dot_weights(wgt)
    ref = nka_amd.nka().init(n, m).set_dot_weights(wgt)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        wb = np.ones(n)
        wb[n // 2] = bad
        with pytest.raises(NKAError, match=r"\(-1\).*first at index %d" % (n // 2)):
            a.set_dot_weights(wb)
        with pytest.raises(NKAError, match=r"\(-1\)"):
            a.set_dot_weights(torch.from_numpy(wb).cuda())
        assert a.dot_weighted()
    short = torch.ones(n + 1, dtype=torch.float64, device="cuda")[: n - 1]
    with pytest.raises(NKAError):                       # the Python layer checks the length ...
        a.set_dot_weights(short)
    import ctypes as C
    big = nka_amd.nka().init(1 << 22, 2)                # ... and the library's pointer check below it (32 MB: beyond any
    tiny = torch.ones(4, dtype=torch.float64, device="cuda")      # segment the caching allocator puts a 4-element tensor in)
    assert big._L.nka_hip_set_dot_weights(big._handle(), C.c_void_p(tiny.data_ptr())) == -1
    assert b"shorter" in big._L.nka_hip_last_error()
    assert not big.dot_weighted()
    for fa, fr in zip(run(a, X[:m]), run(ref, X[:m])):  # the old weighting is in force
        assert torch.equal(fa, fr)

    with pytest.raises(NKAError, match=r"\(-1\)"):
        a.set_sum_order(SUMS_REFERENCE_ORDER)
    p = nka_amd.nka().init(n, m).set_sum_order(SUMS_REFERENCE_ORDER)
    with pytest.raises(NKAError, match=r"\(-1\)"):
        p.set_dot_weights(wgt)
    assert not p.dot_weighted()
    with pytest.raises(NKAError, match=r"\(-5\)"):
        a.set_host_dot(lambda x, y: float(x @ y))
    q = nka_amd.nka().init(n, m)
    q.set_host_dot(lambda x, y: float(x @ y))
    with pytest.raises(NKAError, match=r"\(-5\)"):
        q.set_dot_weights(wgt)
    q.set_host_dot(None)
    q.set_dot_weights(wgt)

    # AUTO at n <= 64: the rounded passes, not the reference-order kernels
    ns = 50
    ws = rng.uniform(0.125, 8.0, ns)
    Y = _inputs(ns, 12, 89)
    s_auto = nka_amd.nka().init(ns, 4).set_dot_weights(ws)
    s_rnd = nka_amd.nka().init(ns, 4).set_sum_order(SUMS_BLOCKED_ROUNDED).set_dot_weights(ws)
    for fa, fr in zip(run(s_auto, Y), run(s_rnd, Y)):
        assert torch.equal(fa, fr)

    # a clone carries the weights
    c = a.copy()
    assert c.dot_weighted()
    for fa, fc in zip(run(a, X[m:m + 3]), run(c, X[m:m + 3])):
        assert torch.equal(fa, fc)
    _same_state(a, c)

    # cleared and restarted: a fresh plain handle
    a.set_dot_weights(None)
    assert not a.dot_weighted()
    a.restart()
    fresh = nka_amd.nka().init(n, m)
    for fa, ff in zip(run(a, X[m + 3:]), run(fresh, X[m + 3:])):
        assert torch.equal(fa, ff)
    _same_state(a, fresh)
