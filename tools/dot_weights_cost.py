#!/usr/bin/env python3
"""What diagonal dot-product weights (nka_hip_set_dot_weights) cost an update: ONE process, one accelerator with weights
and one without, at n = 1e8, m = 20, the default flavour and sum mode; rounds of `--steps` updates alternate between the
two so that clocks and memory state drift alike.  Per-phase device times from nka_hip_set_timing (ms[0] = norm pass + PA +
final sums, ms[1] = scalar step, ms[2] = PB, ms[3] = whole update); medians over every recorded update of a kind.
The byte model: plain 51 words per element at m = 20 in the compact flavour, weighted 53
(the norm pass 2 -> 3, PA 22 -> 23)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nka_amd  # noqa: E402


def measure(n, m, steps, rounds, first, g, f, wgt):
    """One pair of accelerators, `first` created (and run) first; medians of the four phases per kind."""
    accs = {}
    for k in (first, "weighted" if first == "plain" else "plain"):
        accs[k] = nka_amd.nka().init(n, m)
        if k == "weighted":
            accs[k].set_dot_weights(wgt)
    times = {k: [] for k in accs}
    # a fresh random f for every update (as bench.py): no dependence drops, every timed update runs at the full list width
    for a in accs.values():
        a.set_timing(steps)
        for _ in range(m + 2):
            torch.randn(n, generator=g, dtype=torch.float64, device="cuda", out=f)
            a.accel_update(f)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, a in accs.items():
            for _ in range(steps):
                torch.randn(n, generator=g, dtype=torch.float64, device="cuda", out=f)
                a.accel_update(f)
            torch.cuda.synchronize()
            times[k].extend(a.timing_ms(b) for b in range(steps))
    assert all(a.num_vec() == m for a in accs.values())
    for a in accs.values():
        a.delete()
    return {k: [statistics.median(t[i] for t in v) for i in range(4)] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=6, help="pairs of accelerators, created plain-first and weighted-first in turn")
    args = ap.parse_args()
    n, m = int(args.n), args.m
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    f = torch.randn(n, generator=g, dtype=torch.float64, device="cuda")
    wgt = torch.rand(n, generator=g, dtype=torch.float64, device="cuda") + 0.5
    bytes_pa = {"plain": 8.0 * n * (2 + (m + 2)), "weighted": 8.0 * n * (3 + (m + 3))}   # norm pass + PA
    print(f"dot_weights_cost n={n} m={m} {args.repeats} repeats x {args.rounds} rounds x {args.steps} updates per kind, "
          f"device {torch.cuda.get_device_name(0)}")
    print(f"{'repeat':>6} {'first':>8} {'kind':>9} {'sums ms':>9} {'solve ms':>9} {'PB ms':>9} {'update ms':>10} {'sums TB/s':>10} {'of 8 TB/s':>10}")
    ratios, sums_ratios = [], []
    for r in range(args.repeats):
        first = "plain" if r % 2 == 0 else "weighted"
        med = measure(n, m, args.steps, args.rounds, first, g, f, wgt)
        for k in ("plain", "weighted"):
            v = med[k]
            bw = bytes_pa[k] / (v[0] * 1e-3) / 1e12
            print(f"{r:>6} {first:>8} {k:>9} {v[0]:9.4f} {v[1]:9.4f} {v[2]:9.4f} {v[3]:10.4f} {bw:10.3f} {bw / 8.0:10.3f}")
        ratios.append(med["weighted"][3] / med["plain"][3])
        sums_ratios.append(med["weighted"][0] / med["plain"][0])
    q = np.array(ratios)
    print("weighted / plain update per repeat: " + " ".join(f"{x:.4f}" for x in ratios))
    print(f"  median {np.median(q):.4f}  min {q.min():.4f}  max {q.max():.4f}  (byte model 53/51 = {53 / 51:.4f})")
    print("weighted / plain sums phase (norm pass + PA + final sums) per repeat: " + " ".join(f"{x:.4f}" for x in sums_ratios)
          + f"  (byte model 26/24 = {26 / 24:.4f})")


if __name__ == "__main__":
    main()
