"""What the tests of the WIDE batched accelerator (nka_amd/csrc/nka_batch_wide.hip, nka_hip_batch_create_wide) share: the
chunk as the library was built, the K of its sums, the places where its kernels change hands, and a host model of a sum.

A wide system of n elements is nchunk = ceil(n / C) chunks of C = NKA_HIP_BATCH_WIDE_CHUNK elements, one workgroup each.
Inside a chunk a sum is the narrow kernel's (exact_sums.batch_k: one fma per element into one accumulator per thread, thread
t owning the pair 2t, 2t + 1 of every 512; the butterfly of a wavefront; wavefronts 0..3 in turn); the partials of the
chunks are then added in chunk order, starting from chunk 0, by one thread (k_wide_sums / k_wide_scalar)."""
import numpy as np

import exact_sums as X

CANDIDATES = (2048, 4096, 8192)      # the chunks that were timed against each other (tools/batch_throughput.py --wide)


def limits():
    """(C, max_vlen) read from the library."""
    import nka_amd
    return nka_amd.batch_wide_limits()


def nchunk(n, C):
    return -(-n // C)


def wide_k(n, C=None):
    """Roundings a product can meet in a sum of a wide batch over n elements, read off the kernels as built: up to one chunk the
    narrow kernel's batch_k(n) -- one partial, no chunk-order addition --; beyond it

      per-thread chain   two fma per thread and tile of 512, C / 512 tiles in a full chunk:   2 * (C / 512)
      batch_block_sum    the butterfly of six additions and wavefronts 1..3 added to 0:       9
      chunk order        part[0] + part[1] + ... + part[nchunk - 1], one chain:               nchunk - 1"""
    C = C or limits()[0]
    if n <= C:
        return X.batch_k(n)
    return 2 * (C // X.BATCH_TILE) + X.WAVE_LEVELS + (X.WAVES - 1) + (nchunk(n, C) - 1)


def wide_sentinel_indices(n, C=None):
    """Indices where the wide kernels change hands: exact_sums.batch_sentinel_indices of every chunk, shifted to the chunk, and
    the first and the last element of every chunk (where one workgroup's partial ends and the next one's begins)."""
    C = C or limits()[0]
    out = []
    for c in range(nchunk(n, C)):
        lo, ln = c * C, min(C, n - c * C)
        out.append(lo + X.batch_all_sentinels(ln))
        out.append(np.array([lo, lo + ln - 1], dtype=np.int64))
    return np.unique(np.concatenate(out))


def wide_planted_input(n, rng, prev=None, background=0.125, C=None):
    """exact_sums.batch_planted_input with the sentinels of a wide system."""
    x = rng.standard_normal(n) * background
    idx = wide_sentinel_indices(n, C)
    val = np.ldexp(1.0, rng.integers(0, 4, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    if prev is not None:
        same = val == prev[idx]
        val[same] = -val[same]
    x[idx] = val
    return x


def _workgroup_sum(prod):
    """One workgroup's sum of the rounded products `prod` (tests/test_exact_sums_cpu.py: _batch_sum): a rounded product and a
    rounded addition where the device takes one fma -- one rounding MORE per element."""
    n = prod.size
    acc = np.zeros(X.BATCH_THREADS)
    for base in range(0, n, X.BATCH_TILE):
        for q in range(2):
            part = prod[base + q: min(base + X.BATCH_TILE, n): 2]
            acc[:part.size] = acc[:part.size] + part
    waves = []
    for w in range(X.WAVES):
        v = acc[w * X.WAVE:(w + 1) * X.WAVE].copy()
        while v.size > 1:
            v = v[: v.size // 2] + v[v.size // 2:]
        waves.append(v[0])
    r = waves[0]
    for w in waves[1:]:
        r = r + w
    return r


def model_partials(x, y, C):
    """The partial of every chunk as a workgroup forms it -> float64[nchunk]."""
    prod = x * y
    return np.array([_workgroup_sum(prod[lo:lo + C]) for lo in range(0, x.size, C)])


def model_sum_of(parts, chunks):
    """The chunk-order chain over the partials `parts`, adding the chunks of the list `chunks` in the order given: range(nchunk)
    is what the kernels do; a list without c is a sum that lost chunk c's partial, one with c twice a sum that added it twice."""
    chunks = list(chunks)
    r = parts[chunks[0]]
    for c in chunks[1:]:
        r = r + parts[c]
    return float(r)


def model_sum(x, y, C):
    """The summation order of a wide batch restated on the host: per chunk the workgroup's sum, then the chunks in order."""
    parts = model_partials(x, y, C)
    return model_sum_of(parts, range(parts.size))


def chunk_products(x, y, C):
    """sum of x_i y_i over every chunk, plain numpy -> float64[nchunk]: what a sum loses when it loses that chunk's partial."""
    return np.add.reduceat(x * y, np.arange(0, x.size, C))


def undetectable_chunks(x, y, k, C):
    """The chunks whose partial a sum held to gamma(k) * sum|xy| could lose or add twice unseen (exact_sums.detectable): a
    condition on the operands alone.  Operands whose products are all zero have none: every subset of their partials sums to 0.
    Nor have operands with a NaN or an Inf, whose sum is held to be NaN / Inf exactly and not to a bound."""
    with np.errstate(all="ignore"):
        tot = X.abs_dot(x, y)
    if tot == 0.0 or not np.isfinite(tot):
        return []
    bound = X.gamma(k)
    return [c for c, p in enumerate(chunk_products(x, y, C)) if not X.detectable(p, bound, tot)]
