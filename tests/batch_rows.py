"""Helpers of the tests of the narrow batch's scalar step on one wavefront (nka_hip_batch_create_rows; include/nka_hip_batch.h,
NARROW ROWS): tests/test_batch_rows_cpu.py and tests/test_batch_rows_gpu.py.  The sequences, the census and the numpy model are
those of tests/batch_wide_rows.py; this file holds the grid and the shapes of the packs."""
import batch_wide_rows as R

NSYS = R.NSYS                    # eight systems, one workgroup each
ILL = NSYS - 1                   # the system batch_wide_rows.script feeds NaN and Inf
# 65: the smallest length NKA_HIP_SUMS_AUTO runs in the fast sums, one ragged tile of 512; 513: one full tile and one element;
# 1025: two full tiles and one element
VLENS = (65, 513, 1025)
MVECS = (1, 2, 5, 10, 11, 20, 21, 32)      # both sides of every NLMAX edge (11 / 21 / 33 rows) and the largest mvec
NLMAX = (11, 21, 33)
FLAVOR_VLEN = 513                # the other two flavours run at mvec 10 and 20 at this length
AUTO_ORDERED_MAX = 64            # up to this vlen NKA_HIP_SUMS_AUTO means the reference order (kOrdAutoMax, nka_device.hpp)

# the packs of test 2: lengths 1, 64, 65 and vlen among the eight systems of a batch of PACK_VLEN
PACK_VLEN, PACK_MVEC = 513, 10
PACK_LENS = (513, 1, 64, 65, 513, 300, 512, 513)


def nlmax_of(mvec):
    """The instance the library runs at mvec: the smallest of NLMAX that holds mvec + 1 (nka_host::batch_rows_nlmax)."""
    return next(nl for nl in NLMAX if nl >= mvec + 1)


def twin_seed(mvec, flavor):
    """The seed of the twin test's sequences at this point of its grid: that of the wide batch's twin, whose census the oracle
    meets at eight systems (tests/test_batch_rows_cpu.py runs the same ones at the lengths of this grid)."""
    return R.twin_seed(mvec, flavor)


def lds_bytes(mvec):
    """batch_rows_lds(mvec).bytes(), restated: the working copy of batch_lds -- doubles h, c, red, cc, sm, res, then int32 next,
    prev, ps, cs, hdr --, rounded up to 16 bytes, then the matrix of (mvec + 2)^2 doubles."""
    m1 = mvec + 1
    ndouble = (m1 + 1) ** 2 + (m1 + 1) + (2 + 2 * mvec) + m1 + 4 * 9 + 10
    nint = 2 * (m1 + 1) + 2 * m1 + 8
    return (8 * ndouble + 4 * nint + 15) // 16 * 16 + 8 * (mvec + 2) ** 2
