"""What the tests of per-system lengths (nka_hip_batch_set_lengths; tests/test_batch_lengths_gpu.py, test_batch_lengths_cpu.py)
share: the shapes, the paint of the tails, the inputs and the weights.  No GPU here.

A system of length L in a batch of length vlen is held, with ==, to a TWIN: the same system in a batch of the same kind created
with vlen = L.  Everything from L on is painted before the first call -- rows of F and X with NaNs of distinct payloads, weight
rows with 2^500 (weights must be finite) -- so that a tail element read into a sum shows up as NaN or overflow against the
twin, and a tail element written shows up as a changed payload."""
import numpy as np

import batch_seq as B
import batch_weights as BWt

# narrow: two full tiles and a ragged one; the half pair of an odd length, a wavefront edge, a tile edge, the full row
NARROW_VLEN = 1100
NARROW_LENS = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1099, 1100)
TAIL_WEIGHT = 2.0 ** 500
PAD = 7.25                    # what lies between two rows when ld > vlen


def wide_shape(c):
    """(vlen, lengths) of the wide tests for the chunk c: one element, a ragged tile, both sides of every chunk edge, a chunk
    of one tile and one element, the last chunk of 32 and of 33 elements."""
    return 3 * c + 33, (1, 511, c - 1, c, c + 1, 2 * c, 2 * c + 513, 3 * c, 3 * c + 32, 3 * c + 33)


def wide_medium_shape(c):
    """(vlen, lengths): 18 chunks, of which the systems add 1, 2, 9, 9, 10, 16, 17 and 18 partials at a stride of 18 -- the
    eight-way chain over a system's own partials (k_wide_scalar with lengths) with no trip, one and two, and a remainder of none, one and
    seven.  Every twin's vlen but 9 C, 1 and the full row is a shape that tests/test_batch_wide_gpu.py holds to the exact sums."""
    return 17 * c + 33, (1, c + 1, 8 * c + 1, 9 * c, 9 * c + 1, 15 * c + 513, 16 * c + 1, 17 * c + 33)


def wide_long_shape(c):
    """(vlen, lengths): 257 chunks; a system that ends with the first trip of the staging loop of <d,d> (256 partials), one
    partial into the second trip, the full row, and one that gives 256 chunks up."""
    return 256 * c + 513, (256 * c, 256 * c + 1, 256 * c + 513, c)


def nan_paint(nsys, vlen, salt):
    """nsys x vlen quiet NaNs, every one with a payload of its own (salt tells F from X)."""
    bits = np.uint64(0x7FF8000000000000) | (np.uint64(salt) << np.uint64(32)) | (np.arange(nsys * vlen, dtype=np.uint64) + np.uint64(1))
    out = bits.view(np.float64).reshape(nsys, vlen).copy()
    assert np.isnan(out).all() and np.unique(out.view(np.uint64)).size == out.size
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def tails_intact(got, paint, lens):
    """Rows of `got` from lens[k] on against the paint, byte for byte -> the systems whose tail was written."""
    return [k for k, L in enumerate(lens) if not same_bytes(got[k, L:], paint[k, L:])]


def sequences(lens, seed):
    """One batch_seq.Sequence per system, of the system's own length."""
    return [B.Sequence(L, seed + 31 * k) for k, L in enumerate(lens)]


def weight_rows(lens, vlen, seed):
    """nsys x vlen: batch_weights.draw_weights of the system's own length below L (zeros, values that are no power of two),
    2^500 from there on."""
    w = np.full((len(lens), vlen), TAIL_WEIGHT)
    for k, L in enumerate(lens):
        w[k, :L] = BWt.draw_weights(L, np.random.default_rng([seed, L, k]))
    return w


def mask_rows(lens, vlen):
    """The zero-weight recipe of the header (WEIGHTS, RAGGED BATCHES): 1 below L, 0 from there on."""
    w = np.zeros((len(lens), vlen))
    for k, L in enumerate(lens):
        w[k, :L] = 1.0
    return w
