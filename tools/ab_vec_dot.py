#!/usr/bin/env python3
"""A/B of builds on the reference-order dot product of LONG vectors (nka_hip_vec_dot with sum order 1 and n > 4096: the one
launch of k_dot_chain).  One workspace per build on the same stream and the same inputs; the builds are alternated in blocks
of K dots for R rounds, order reversed every other round; device time per block from HIP events; the results must agree
bit for bit.

  tools/ab_vec_dot.py nka_amd/libnka_hip_diag.so OTHER/libnka_hip_diag.so ...      the first is the base of the percentages
"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from nka_amd import _lib
    libs = sys.argv[1:]
    torch.cuda.set_device(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Ls, hs = [], []
    for p in libs:
        L = _lib.load_diag_at(p)
        h = C.c_void_p()
        assert L.nka_hip_vec_workspace_create(C.byref(h), 0, stream) == 0
        assert L.nka_hip_vec_set_sum_order(h, 1) == 0
        Ls.append(L)
        hs.append(h)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nbad = 0
    rounds, steps = 20, 20
    for n in (4097, 100003, 1 << 20, 4000001):
        g = torch.Generator(device="cuda").manual_seed(n)
        x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
        y = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
        # bits: dot of aligned and of misaligned operands (the scalar-load path), and the norm
        vals = []
        for L, h in zip(Ls, hs):
            r = C.c_double()
            v = []
            assert L.nka_hip_vec_dot(h, n, P(x), P(y), C.byref(r)) == 0
            v.append(r.value)
            assert L.nka_hip_vec_dot(h, n - 1, P(x[1:]), P(y[1:]), C.byref(r)) == 0
            v.append(r.value)
            assert L.nka_hip_vec_norm2(h, n, P(x), C.byref(r)) == 0
            v.append(r.value)
            vals.append(v)
        bad = sum(v != vals[0] for v in vals[1:])
        nbad += bad
        res = {i: [] for i in range(len(libs))}
        r = C.c_double()
        for rd in range(rounds):
            order = list(range(len(libs)))
            if rd % 2:
                order.reverse()
            for i in order:
                L, h = Ls[i], hs[i]
                assert L.nka_hip_vec_dot(h, n, P(x), P(y), C.byref(r)) == 0       # (one untimed dot after the switch)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    assert L.nka_hip_vec_dot(h, n, P(x), P(y), C.byref(r)) == 0
                e1.record()
                e1.synchronize()
                res[i].append(e0.elapsed_time(e1) / steps)
        base = statistics.median(res[0])
        print(f"n={n}  {rounds} rounds x {steps} dots per build  [bit check: {bad} builds differ from the first]  dot = {vals[0][0]!r}")
        for i, p in enumerate(libs):
            d = res[i]
            print(f"  {p:44s} median {statistics.median(d):.5f} ms  mean {statistics.mean(d):.5f}  min {min(d):.5f}  sd {statistics.pstdev(d):.5f} "
                  f"({100.0 * (statistics.median(d) / base - 1.0):+.3f} % of the first, by medians)", flush=True)
    for L, h in zip(Ls, hs):
        L.nka_hip_vec_workspace_destroy(h)
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main())
