"""Input sequences of the batched-accelerator tests (tests/test_batch_gpu.py, tests/test_batch_cpu.py): every system of a
batch gets its own seeded sequence mixing fresh inputs, dependent inputs (3-dimensional basis: forces drops), repeated
inputs (s == 0 -> relax inside the update) and zero inputs, as test_randomised_call_sequences_against_oracle does.

pick_seed(): the fast-sum tests judge a system against the extended-precision trajectory, which is only the truth of the
sequence while it takes the reference's decisions (parity_util.Spread.decisions_agree).  That is a property of the oracle
alone, so a seed is chosen for it ON THE CPU, before anything runs on the GPU: the first candidate of a fixed series whose
dry run agrees.  No system is left out; a seed that fails is replaced by the next candidate.

NearThreshold (at the end): inputs for tests/test_batch_sums_exact_gpu.py, where no seed needs to agree with anything: the
scalar step is held to the oracle's on the device's own sums, and the inputs are built so that the drop rule decides close calls."""
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


# ---- close calls of the drop rule (tests/test_batch_sums_exact_gpu.py: the scalar step given the device's own sums) --------

NEAR_VLENS, NEAR_MVECS, NEAR_NSYS, NEAR_CALLS = (7, 65, 257, 700), (5, 10), 8, 24


class NearThreshold:
    """Inputs that put the drop rule (F08:326, hkk > vtol**2) near its threshold: next() -> (float64[vlen], near).

    With probability one half, once two inputs exist, x_t = x_(t-1) - (d + eps ||d|| g / ||g||) with d = x_(t-2) - x_(t-1),
    g fresh noise and eps log-uniform in [1e-3, 1e-1].  The difference the update of x_t normalises is then
    d + eps ||d|| g/||g||, at an angle of about eps to the stored w = d/||d|| of the pair before it -- the newest of the
    older entries -- whose pivot comes out as hkk ~ eps**2 against vtol**2 = 1e-4: dropped for eps below vtol, kept
    above, a close call in between (`near` = True for such a call).  Otherwise a fresh input."""

    def __init__(self, vlen, seed):
        self.rng = np.random.default_rng(seed)
        self.vlen = int(vlen)
        self.x1 = self.x2 = None            # x_(t-1), x_(t-2)

    def next(self):
        near = self.x2 is not None and self.rng.random() < 0.5
        if near:
            d = self.x2 - self.x1
            g = self.rng.standard_normal(self.vlen)
            eps = 10.0 ** self.rng.uniform(-3.0, -1.0)
            x = self.x1 - (d + eps * np.linalg.norm(d) * g / np.linalg.norm(g))
        else:
            x = self.rng.standard_normal(self.vlen)
        self.x2, self.x1 = self.x1, x
        return x, near


def near_seeds(vlen, mvec):
    """The seeds of the NEAR_NSYS systems of one shape (all flavours run the same inputs).  Fixed here, on the CPU; the guard
    test_near_threshold_generator_meets_both_outcomes (tests/test_exact_sums_cpu.py) holds every series to: at least one
    close call ends with the pair in question dropped and one with it kept.  A series that fails it is replaced HERE."""
    return [500009 * int(vlen) + 3001 * int(mvec) + 17 * k for k in range(NEAR_NSYS)]


def near_outcomes(oracle, vlen, mvec, flavor, seeds=None, calls=NEAR_CALLS):
    """Dry run on the oracle alone -> (close calls that dropped the pair in question, close calls that kept it).  The pair in
    question is the newest older entry at the entry of the call: the one whose w the input was built to be nearly parallel
    to."""
    dropped = kept = 0
    for seed in near_seeds(vlen, mvec) if seeds is None else seeds:
        ora, seq = oracle.OracleNKA(vlen, mvec, flavor), NearThreshold(vlen, seed)
        for _ in range(calls):
            x, near = seq.next()
            order = ora.state().list_order()
            ora.accel_update(x.copy())
            if near and ora.state().pending and len(order) >= 2:
                if order[1] in ora.state().list_order()[1:]:      # ([0] is the new pair: it may have taken the dropped slot)
                    kept += 1
                else:
                    dropped += 1
    return dropped, kept
