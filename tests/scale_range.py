"""Inputs and expectations of tests/test_scale_range_cpu.py and tests/test_scale_range_gpu.py: the update paths across the
binary64 exponent range.  No GPU here.

NKA is exactly covariant under a power-of-two scaling of its inputs as long as nothing underflows or overflows: the run on
2^k o F returns 2^k o (the run on F), with the same decisions.  Outside that range IEEE arithmetic still fixes every bit, so a
path in the reference's order must equal the oracle at every k, and a fast path must be covariant wherever the oracle is.

  K_COVARIANT  -400 puts red[0] = dp(d, d) and the step's dp(f, f) below 2^-767, where the compiler's binary64 sqrt scales its
               argument by 2^256 and its result by 2^-128; +400 is its mirror.  The bound is derived, not fitted: the nonzero
               elements of the unscaled inputs are at least 2^-30 in magnitude (held by the CPU file), so a product is at least
               2^-60, and every partial sum is a multiple of its last bit: a nonzero partial sum stays far above 2^-222, and times
               2^-800 it is still a normal number.  The fast sums are held here.
  K_EDGE       -540  d*d underflows to 0 with d != 0: s == 0, the update relaxes -- other decisions than at k = 0
               -520  red[0] is subnormal: the outputs are no longer covariant, the decisions are those of k = 0
               -505  the last exponent on this side at which every product is normal: covariant
                505  its mirror: covariant
                511  dp(d, d) overflows to Inf in some calls: s == Inf, 1 / s == 0; the outputs stay finite
                600  it overflows in every call with a pending pair
  K_ALL        all of them and 0.

exponents() gives system j of a batch the exponent K[j % len(K)], so that one launch carries every regime in neighbouring
workgroups or lanes; the systems j, j + 1, ..., j + len(K) - 1 of one round share ONE seed, so that their runs can be compared.
Every comparison built on this file is split_update._bits_equal (NaN as NaN): no tolerance anywhere."""
import numpy as np

import batch_seq as B

K_COVARIANT = (-400, 400)
K_EDGE = (-540, -520, -505, 505, 511, 600)
K_ALL = K_EDGE + K_COVARIANT + (0,)
K_SAFE = K_COVARIANT + (-505, 505)      # where the oracle itself is held to covariance (tests/test_scale_range_cpu.py)
K_FAST = (0,) + K_COVARIANT             # the batches of the fast-sum tests: a k = 0 system beside its scaled twins
K_OVERFLOW = (511, 600)
# dp(d, d) is about 2 vlen 4^k: at vlen = 5000 it passes 2^1024 at k = 505 already, so for that shape +505 belongs to the
# overflow regime (the CPU file asserts the Inf instead of covariance there; -505 and +-400 stay covariant).  The lone handle's
# integer-form chain sums run at +-400 and 0 and fall back to the walk beyond 2^+-900, i.e. at every other k.
OVERFLOWS_AT_505 = (5000,)

SUBNORMAL = 2.0 ** -1022                # the smallest normal binary64 number


# ---- shapes (vlen, mvec) of the GPU file, fixed here so that the CPU file holds the oracle on the same ones ------------------

REF_NARROW = [(vlen, mvec) for vlen in (7, 64, 700) for mvec in (3, 10)]      # narrow batch, SUMS_REFERENCE_ORDER
REF_LANES = [(vlen, mvec) for vlen in (7, 64) for mvec in (3, 10)]            # lane batch
REF_LONE = [(n, 5) for n in (7, 64, 700, 5000)]     # lone handle, SUMS_REFERENCE_ORDER; 5000: four whole blocks of 1024 and a ragged one
FAST_NARROW = [(vlen, mvec) for vlen in (65, 700, 1030) for mvec in (3, 10)]  # 1030: two tiles of 512 and a ragged one
FAST_WIDE = [(2048 + 7, 5), (3 * 2048, 5)]                                    # two and three chunks
FAST_STORE32 = [(65, 5), (700, 5)]
FAST_WEIGHTED = [(700, 5)]
FAST_LENGTHS_NARROW, FAST_LENGTHS_WIDE = (700, 5), (2048 + 7, 5)
FAST_LONE = [(700, 5), (1030, 5)]                   # 1030: past one block of the lone handle's chain and two tiles of its passes
ROUNDS_REF = 2                          # rounds (seeds) of a batch over K_ALL: nsys = 18
ROUNDS_LANES = 8                        # ... of a lane batch: nsys = 72, more than one group of 64
ROUNDS_FAST = 3                         # ... of a batch over K_FAST: nsys = 9


def num_calls(mvec):
    """Enough calls to fill the list and drop from it."""
    return mvec + 10


def seed(vlen, mvec, rnd):
    """The seed of round `rnd` of a shape.  A seed that fails a witness of tests/test_scale_range_cpu.py is replaced HERE."""
    return 1234 + int(vlen) + 100003 * int(rnd)


def exponents(nsys, K=K_ALL):
    """The exponent of every system of a batch: K[j % len(K)]."""
    return [K[j % len(K)] for j in range(nsys)]


def rounds(nsys, K=K_ALL):
    """The round (seed index) of every system: j // len(K)."""
    return [j // len(K) for j in range(nsys)]


def scaled(x, k):
    """2^k o x, exactly where nothing leaves the normal range (np.ldexp rounds once into the subnormals, like the arithmetic)."""
    return np.ldexp(np.asarray(x, np.float64), int(k))


def base_inputs(vlen, mvec, rnd, calls=None):
    """The unscaled inputs of one round: float64[calls, vlen] from batch_seq.Sequence (fresh, dependent, repeated and zero)."""
    seq = B.Sequence(vlen, seed(vlen, mvec, rnd))
    return np.stack([seq.next() for _ in range(num_calls(mvec) if calls is None else calls)])


def batch_inputs(vlen, mvec, nsys, K=K_ALL, calls=None):
    """-> float64[calls, nsys, vlen]: system j runs the inputs of round j // len(K) scaled by 2^K[j % len(K)]."""
    base = {}
    out = []
    for k, r in zip(exponents(nsys, K), rounds(nsys, K)):
        if r not in base:
            base[r] = base_inputs(vlen, mvec, r, calls)
        out.append(scaled(base[r], k))
    return np.stack(out, axis=1)


# ---- what a scaling of the inputs by 2^k does to every observable --------------------------------------------------------------

def expect_rows(x, k):
    """Rows of f and x, fnorm, c, and the pending pair (w and v of the newest slot while it is pending): times 2^k."""
    return scaled(x, k)


def expect_red(red, k, mvec):
    """red[0] = dp(d, d) times 4^k; red[1] = dp(f, w1') and red[2 + mvec + p] = dp(f, w_p) times 2^k; red[2 + p] = dp(w1', w_p)
    unchanged."""
    out = np.array(red, np.float64)
    out[0] = np.ldexp(out[0], 2 * int(k))
    out[1] = np.ldexp(out[1], int(k))
    out[2 + mvec:] = np.ldexp(out[2 + mvec:], int(k))
    return out

# h, the list and free order, subspace / pending, num_vec and the normalised slots (w', v' or the compact difference, binary32
# slots included) are unchanged.  c scales, so digests are compared only between runs at the SAME k.


# ---- the oracle-order chain on the host -------------------------------------------------------------------------------------------

def chain(x, y):
    """acc = acc + x_i * y_i, element after element, one rounding per product and per addition (Python floats are binary64 and
    the interpreter contracts nothing): the reference's dot product, oracle/nka_oracle.c seq_dot."""
    acc = 0.0
    for a, b in zip(np.asarray(x, np.float64).tolist(), np.asarray(y, np.float64).tolist()):
        acc = acc + a * b
    return acc


def is_subnormal(x):
    return 0.0 < abs(x) < SUBNORMAL


class OracleRun:
    """One system on the oracle with what the witnesses need from every call: update(x) -> dict with the output `f`, `pending`
    on entry, `d` = w1 - x (None without a pending pair), `dd` = chain(d, d), and `nv0`, `nv` = num_vec before and after."""

    def __init__(self, oracle, vlen, mvec, flavor):
        self.ora = oracle.OracleNKA(vlen, mvec, flavor)

    def update(self, x, with_dd=True):
        st = self.ora.state()
        d = self.ora.w(st.first) - x if st.pending else None
        nv0 = self.ora.num_vec()
        f = np.array(x, np.float64)
        self.ora.accel_update(f)
        return {"f": f, "pending": st.pending, "d": d, "dd": chain(d, d) if with_dd and d is not None else None, "nv0": nv0,
                "nv": self.ora.num_vec()}


def observables(ora):
    """(decisions, h, c, {slot: (w, v)} of the list) of an oracle, as the covariance checks compare them."""
    st = ora.state()
    return ((st.list_order(), st.free_order(), st.subspace, st.pending, ora.num_vec()), st.h.copy(), st.c.copy(),
            {s: (ora.w(s), ora.v(s)) for s in st.list_order()})
