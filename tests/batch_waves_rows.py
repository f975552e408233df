"""Helpers of the tests of the wave batch's scalar step on the whole wavefront (nka_hip_batch_create_waves_rows;
include/nka_hip_batch.h, WAVES ROWS): tests/test_batch_waves_rows_cpu.py and tests/test_batch_waves_rows_gpu.py.  The sequences,
the census and the numpy model are those of tests/batch_wide_rows.py; this file holds the grid."""

NSYS = 9                         # three workgroups, the last with three absent wavefronts
ILL = 7                          # the system batch_wide_rows.script feeds NaN and Inf
VLENS = (65, 129, 385)           # one ragged tile, two tiles, three tiles and a half pair
LDS_LIMIT = 64 * 1024            # the dynamic LDS a launch may ask for without a function attribute


def cap():
    """The cap on mvec, derived in nka_amd/csrc/host_logic.hpp (waves_rows_max_mvec) and read from the library when a test runs (no
    device needed; not at import: the GPU tests load the library behind torch)."""
    import nka_amd
    return nka_amd.batch_waves_rows_limits()[0]


MVECS = (1, 2, 5, 6, 10, 11, 20, 21, "cap")      # both sides of every NLMAX boundary (6 / 11 / 21 / cap + 1 rows) and the cap


def mvec_of(which):
    return cap() if which == "cap" else int(which)


def twin_seed(mvec, flavor):
    """The seed of the twin test's sequences at this point of its grid: that of the wide batch's twin (the CPU census runs the same
    ones at nine systems; a seed that fell short there would be replaced HERE)."""
    import batch_wide_rows as R
    return R.twin_seed(mvec, flavor)
