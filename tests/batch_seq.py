"""Input sequences of the batched-accelerator tests (tests/test_batch_gpu.py, tests/test_batch_cpu.py): every system of a
batch gets its own seeded sequence mixing fresh inputs, dependent inputs (3-dimensional basis: forces drops), repeated
inputs (s == 0 -> relax inside the update) and zero inputs, as test_randomised_call_sequences_against_oracle does.

pick_seed(): the fast-sum tests judge a system against the extended-precision trajectory, which is only the truth of the
sequence while it takes the reference's decisions (parity_util.Spread.decisions_agree).  That is a property of the oracle
alone, so a seed is chosen for it ON THE CPU, before anything runs on the GPU: the first candidate of a fixed series whose
dry run agrees.  No system is left out; a seed that fails is replaced by the next candidate."""
import numpy as np


def num_calls(vlen, mvec):
    """Enough calls to fill the subspace and drop from it (mvec <= 20); shorter for the longest vectors."""
    return 12 if vlen >= 4099 else min(mvec, 20) + 10


class Sequence:
    """The inputs of one system, drawn call by call: next() -> float64[vlen]."""

    def __init__(self, vlen, seed):
        self.rng = np.random.default_rng(seed)
        self.vlen = int(vlen)
        self.basis = self.rng.standard_normal((3, self.vlen))
        self.prev = None

    def next(self):
        kind = self.rng.random()
        if self.prev is None or kind < 0.55:
            x = self.rng.standard_normal(self.vlen)
        elif kind < 0.85:
            x = self.rng.standard_normal(3) @ self.basis        # dependent: forces drops
        elif kind < 0.95:
            x = self.prev.copy()                                 # repeated: s == 0 -> relax
        else:
            x = np.zeros(self.vlen)
        self.prev = x
        return x


def seed_candidates(vlen, mvec, k):
    base = 100003 * int(vlen) + 1009 * int(mvec) + int(k)
    return [base + 7919 * j for j in range(50)]


def decisions_agree(oracle, vlen, mvec, seed, calls):
    """Dry run of one system's sequence on the CPU: does the extended-precision restatement take the reference's decisions?"""
    ref, exact = oracle.OracleNKA(vlen, mvec, oracle.F08), oracle.OracleExact(vlen, mvec, oracle.F08)
    seq = Sequence(vlen, seed)
    for _ in range(calls):
        x = seq.next()
        for a in (ref, exact):
            f = x.copy()
            a.accel_update(f)
        if exact.state().list_order() != ref.state().list_order():
            return False
    return True


def pick_seed(oracle, vlen, mvec, k, calls):
    for seed in seed_candidates(vlen, mvec, k):
        if decisions_agree(oracle, vlen, mvec, seed, calls):
            return seed
    raise AssertionError(("no seed of the series keeps the exact run on the reference's decisions", vlen, mvec, k))
