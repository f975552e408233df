"""nka_amd -- MI355X-native drop-in for the accel_update path of nncarlson/nka.

The product is libnka_hip.so (hand-written HIP for gfx950 behind the C ABI of
include/nka_hip.h).  This package holds only what that path needs:
  csrc/      HIP kernels + the C ABI
  fortran/   the Fortran host side (module nka_type, vector_class, ...) over iso_c_binding
  nka.py     a Python mirror of the reference's `type nka` used by tests and bench.py
  batch.py   the same for a batch of systems advanced together (include/nka_hip_batch.h): one workgroup per system (with
             narrow_rows=True: the opt-in scalar step on one wavefront), or
             wide: a system split across workgroups (with step=True: its solve step too), or lanes: one lane per system (very short systems), or waves: one
             wavefront per system (short systems; with ext=True: per-system lengths and dot weights too; with rows=True: the opt-in scalar step on
             the whole wavefront)
  dist.py    slicing + RCCL bootstrap for the sharded (one rank per GPU) run
There is NO CPU fallback: without the HIP library every entry point raises.
"""
from ._lib import build, lib_path, load  # noqa: F401
from .nka import (FLAVOR_C, FLAVOR_DEFAULT, FLAVOR_F08, FLAVOR_F08_VECTOR, SUMS_AUTO, SUMS_BLOCKED, SUMS_BLOCKED_ROUNDED,  # noqa: F401
                  SUMS_REFERENCE_ORDER, NKAError, nka)
from .batch import (BATCH_LANES_MAX_VLEN, BATCH_MAX_MVEC, BATCH_MAX_VLEN, KIND_LANES, KIND_NARROW, KIND_WAVES, KIND_WIDE,  # noqa: F401
                    SCALAR_ONE_THREAD, SCALAR_WAVEFRONT, STORE_F32, STORE_F64, batch_lanes_limits, batch_rows_limits, batch_waves_limits,
                    batch_waves_rows_limits, batch_wide_limits, nka_batch)
