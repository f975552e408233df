"""Python mirror of the batched accelerator (include/nka_hip_batch.h): `nsys` independent NKA states of equal shape,
advanced by ONE kernel launch per call, one workgroup per system -- or, with init(..., wide=True), by four launches with every
system split across workgroups (systems too long for one workgroup).  Method names are those of `nka_amd.nka`; the
per-system queries take the system's index first.  All arithmetic happens in libnka_hip.so on the GPU; this file is
plumbing (ctypes + torch for device memory and streams)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .nka import FLAVOR_DEFAULT, NKAError, State, _check

BATCH_MAX_VLEN, BATCH_MAX_MVEC = 16384, 32      # NKA_HIP_BATCH_MAX_VLEN / _MVEC (include/nka_hip_batch.h)
STORE_F64, STORE_F32 = 0, 1                     # NKA_HIP_BATCH_STORE_F64 / _F32 (include/nka_hip_batch.h, STORAGE)
SCALAR_ONE_THREAD, SCALAR_WAVEFRONT = 0, 1      # NKA_HIP_BATCH_SCALAR_ONE_THREAD / _WAVEFRONT (include/nka_hip_batch.h, SCALAR STEP)


def batch_wide_limits():
    """(chunk, max_vlen) of a wide batch -- NKA_HIP_BATCH_WIDE_CHUNK and NKA_HIP_BATCH_WIDE_MAX_VLEN as the loaded library
    was built (nka_hip_batch_wide_limits)."""
    chunk, cap = C.c_int64(), C.c_int64()
    L = _lib.load()
    _check(L.nka_hip_batch_wide_limits(C.byref(chunk), C.byref(cap)), "nka_hip_batch_wide_limits", L)
    return int(chunk.value), int(cap.value)


BATCH_LANES_MAX_VLEN = 64                       # NKA_HIP_BATCH_LANES_MAX_VLEN (include/nka_hip_batch.h, LANES)
KIND_NARROW, KIND_WIDE, KIND_LANES, KIND_WAVES = 0, 1, 2, 3    # NKA_HIP_BATCH_KIND_*


def batch_lanes_limits(mvec: int):
    """(systems_per_group, max_vlen) of a lane batch at this mvec -- how many systems one workgroup advances, as the loaded
    library was built, and NKA_HIP_BATCH_LANES_MAX_VLEN (nka_hip_batch_lanes_limits)."""
    group, cap = C.c_int32(), C.c_int64()
    L = _lib.load()
    _check(L.nka_hip_batch_lanes_limits(int(mvec), C.byref(group), C.byref(cap)), "nka_hip_batch_lanes_limits", L)
    return int(group.value), int(cap.value)


def batch_waves_limits():
    """(systems_per_group, max_vlen) of a wave batch -- the wavefronts of a workgroup, one system each (4), and
    NKA_HIP_BATCH_WAVES_MAX_VLEN as the loaded library was built (nka_hip_batch_waves_limits)."""
    group, cap = C.c_int32(), C.c_int64()
    L = _lib.load()
    _check(L.nka_hip_batch_waves_limits(C.byref(group), C.byref(cap)), "nka_hip_batch_waves_limits", L)
    return int(group.value), int(cap.value)


def batch_waves_rows_limits(mvec: int | None = None):
    """(max_mvec, lds_bytes) of a wave batch that offers the scalar step on the wavefront (init(..., waves=True, rows=True);
    nka_hip_batch_waves_rows_limits): the largest mvec whose four working copies and four matrices fit the 64 KiB of dynamic LDS
    a launch may ask for, as the loaded library was built, and the LDS of one workgroup at `mvec` (default: at that cap)."""
    cap, lds = C.c_int32(), C.c_int64()
    L = _lib.load()
    _check(L.nka_hip_batch_waves_rows_limits(C.byref(cap), 1, None), "nka_hip_batch_waves_rows_limits", L)
    _check(L.nka_hip_batch_waves_rows_limits(None, int(cap.value if mvec is None else mvec), C.byref(lds)),
           "nka_hip_batch_waves_rows_limits", L)
    return int(cap.value), int(lds.value)


def batch_rows_limits(mvec: int):
    """lds_bytes of one workgroup of a narrow batch that runs the scalar step on wavefront 0 (init(..., narrow_rows=True) with
    set_scalar_step(SCALAR_WAVEFRONT); nka_hip_batch_rows_limits): the working copy and, behind it, the matrix of (mvec + 2)^2
    doubles, as the loaded library was built.  mvec outside 1 ... BATCH_MAX_MVEC raises NKAError."""
    lds = C.c_int64()
    L = _lib.load()
    _check(L.nka_hip_batch_rows_limits(int(mvec), C.byref(lds)), "nka_hip_batch_rows_limits", L)
    return int(lds.value)


class nka_batch:  # noqa: N801  (beside the reference's type name `nka`)
    """A batch of MI355X accelerator objects; see the module docstring."""

    def __init__(self):
        self._h = None
        self._L = _lib.load()          # raises if the HIP library is missing: no CPU path

    def init(self, nsys: int, vlen: int, mvec: int, *, flavor: int = FLAVOR_DEFAULT, device: int | None = None,
             stream: int | None = None, wide: bool = False, storage: int = STORE_F64, lanes: bool = False,
             waves: bool = False, step: bool = False, ext: bool = False, wide_storage: int = STORE_F64, rows: bool = False,
             narrow_rows: bool = False):
        """nsys systems of vlen elements, at most mvec vectors each, vtol = 0.01, all restarted.  `stream` is a raw
        hipStream_t (default: torch's current stream on `device`, followed from call to call like `nka`).  wide: every
        system split across workgroups (nka_hip_batch_create_wide: vlen up to batch_wide_limits()[1]; accel_update, masks,
        restart / relax, graphs and per-system lengths -- set_lengths -- are offered; accel_step -- without step=True, below --, weights -- without ext=True, below -- and the
        reference sum order are refused).  storage=STORE_F32 (nka_hip_batch_create_stored; include/nka_hip_batch.h, STORAGE): the
        normalised subspace vectors are kept in binary32 -- 0.55 of the slot memory at mvec = 20 --, every product and sum
        still binary64, the pending pair still binary64.  Such a batch runs the default flavour (FLAVOR_C) and the rounded fast
        sums only: the F08 flavours, set_sum_order(SUMS_REFERENCE_ORDER) and wide=True are refused (NKAError).
        lanes: ONE LANE PER SYSTEM (nka_hip_batch_create_lanes; include/nka_hip_batch.h, LANES) for very short systems, vlen up
        to batch_lanes_limits(mvec)[1] = 64: every sum in the reference's order, bit-equal to a narrow batch with
        SUMS_REFERENCE_ORDER; accel_update, accel_step, masks, restart / relax and graphs are offered, weights, lengths and the
        fast sums refused.  Together with wide=True or storage != STORE_F64 it raises NKAError.
        waves: ONE WAVEFRONT PER SYSTEM, four systems per workgroup (nka_hip_batch_create_waves; include/nka_hip_batch.h, WAVES),
        vlen up to batch_waves_limits()[1] = 1024, on the storage of the default batch: the rounded fast sums at every vlen (their own
        bits, the numerical contract of SUMS_BLOCKED_ROUNDED); accel_update, accel_step, masks, restart / relax and graphs are
        offered, weights, lengths and the reference sum order refused.  Together with wide=True, lanes=True or
        storage != STORE_F64 it raises NKAError.
        ext (with waves=True only): the wave batch WITH per-system lengths and diagonal dot weights (nka_hip_batch_create_waves_ext;
        include/nka_hip_batch.h, WAVES EXT) -- set_lengths and set_dot_weights are offered with the contracts of the default batch,
        a system of length L carries the bits of a wave batch of vlen = L, and with neither set the batch is the plain wave batch
        bit for bit.  ext=True with neither waves=True nor wide=True raises NKAError.
        rows (with waves=True only, with or without ext=True): the wave batch that OFFERS THE SCALAR STEP ON THE WHOLE WAVEFRONT
        (nka_hip_batch_create_waves_rows; include/nka_hip_batch.h, WAVES ROWS) -- set_scalar_step(SCALAR_WAVEFRONT) is accepted, and
        both steps leave the same bits; until it is called the batch is the wave batch (ext=True: with lengths and weights) bit for
        bit and launch for launch.  mvec is at most batch_waves_rows_limits()[0] = 28.  rows=True without waves=True raises NKAError.
        ext (with wide=True, with or without step=True): the wide batch WITH diagonal dot weights (nka_hip_batch_create_wide_ext;
        include/nka_hip_batch.h, WIDE EXT) -- set_dot_weights is offered in both forms, one shared row or one row per system, with
        the contract of the default batch per chunk; at one chunk it is the weighted default batch bit for bit, with unit weights or
        none set it is the plain wide batch bit for bit.  The reference sum order and binary32 storage stay refused.
        step (with wide=True only): the wide batch WITH the solve step (nka_hip_batch_create_wide_step; include/nka_hip_batch.h,
        WIDE: STEP of a wide batch) -- one more buffer of nsys x nchunk doubles, accel_step as four launches, everything else the
        wide batch bit for bit.  Every other kind offers the step already: step=True without wide=True raises NKAError.
        wide_storage (with wide=True only; with or without step=True, ext=True or not): wide_storage=STORE_F32 is the wide batch WITH
        binary32 storage of the normalised subspace vectors (nka_hip_batch_create_wide_stored; include/nka_hip_batch.h, WIDE STORED)
        -- the STORAGE contract per chunk, the pending pair and every product and sum still binary64; the default flavour and the
        rounded fast sums only; weights and lengths are offered, accel_step with step=True; at one chunk it is the default batch with
        storage=STORE_F32 bit for bit.  storage=STORE_F32 together with wide=True keeps raising: the keyword of the wide batch is
        this one.  wide_storage != STORE_F64 without wide=True raises NKAError.
        narrow_rows: the default batch -- one workgroup per system, vlen up to 16 384, every flavour, weights, lengths, accel_step,
        storage=STORE_F32 or not -- that OFFERS THE SCALAR STEP ON ONE WAVEFRONT (nka_hip_batch_create_rows; include/nka_hip_batch.h,
        NARROW ROWS): set_scalar_step(SCALAR_WAVEFRONT) is accepted while the batch runs the fast sums, and both steps leave the
        same bits; until it is called the batch is the default batch bit for bit and launch for launch.  Together with wide=True,
        lanes=True or waves=True it raises NKAError."""
        import torch

        if step and not wide:
            raise NKAError("nka_batch init: step=True selects the wide batch with the solve step and needs wide=True (every other "
                           "kind offers accel_step already)")
        if ext and not (waves or wide):
            raise NKAError("nka_batch init: ext=True selects the wave batch with lengths and weights and needs waves=True, or the wide "
                           "batch with weights and needs wide=True (the default batch offers both already)")
        if rows and not waves:
            raise NKAError("nka_batch init: rows=True selects the wave batch that offers the scalar step on the wavefront and needs "
                           "waves=True (a wide batch offers set_scalar_step already)")
        if narrow_rows and (wide or lanes or waves):
            raise NKAError("nka_batch init: narrow_rows=True selects the default batch (one workgroup per system) that offers the scalar "
                           "step on one wavefront and excludes wide=True, lanes=True and waves=True (a wide batch offers "
                           "set_scalar_step already; a wave batch: waves=True, rows=True)")
        if int(wide_storage) != STORE_F64 and not wide:
            raise NKAError("nka_batch init: wide_storage selects the storage of a wide batch and needs wide=True (the default batch: "
                           "storage=STORE_F32)")
        if waves and (wide or lanes):
            raise NKAError("nka_batch init: waves=True excludes wide=True and lanes=True (one wavefront per system, a system split "
                           "across workgroups, or one lane per system)")
        if waves and int(storage) != STORE_F64:
            raise NKAError("nka_batch init: binary32 storage is not offered by a wave batch (storage=STORE_F64)")

        if lanes and wide:
            raise NKAError("nka_batch init: lanes=True and wide=True exclude each other (one lane per system, or a system split "
                           "across workgroups)")
        if lanes and int(storage) != STORE_F64:
            raise NKAError("nka_batch init: binary32 storage is not offered by a lane batch (storage=STORE_F64)")
        self.delete()
        if not torch.cuda.is_available():
            raise NKAError("no HIP device visible: nka_amd has no CPU path")
        if device is None:
            device = torch.cuda.current_device()
        explicit_stream = stream
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        h = C.c_void_p()
        if narrow_rows:
            _check(self._L.nka_hip_batch_create_rows(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                     C.c_void_p(stream), int(storage)), "nka_hip_batch_create_rows", self._L)
        elif int(storage) != STORE_F64:
            if wide:
                raise NKAError("nka_batch init: binary32 storage is not offered by a wide batch (storage=STORE_F64) through `storage`: "
                               "wide_storage=STORE_F32 selects it")
            _check(self._L.nka_hip_batch_create_stored(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                       C.c_void_p(stream), int(storage)), "nka_hip_batch_create_stored", self._L)
        elif wide and int(wide_storage) != STORE_F64:
            _check(self._L.nka_hip_batch_create_wide_stored(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                            C.c_void_p(stream), 1 if step else 0, int(wide_storage)),
                   "nka_hip_batch_create_wide_stored", self._L)
        elif lanes:
            _check(self._L.nka_hip_batch_create_lanes(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                      C.c_void_p(stream)), "nka_hip_batch_create_lanes", self._L)
        elif waves and rows:
            _check(self._L.nka_hip_batch_create_waves_rows(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                           C.c_void_p(stream), 1 if ext else 0), "nka_hip_batch_create_waves_rows", self._L)
        elif waves and ext:
            _check(self._L.nka_hip_batch_create_waves_ext(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                          C.c_void_p(stream)), "nka_hip_batch_create_waves_ext", self._L)
        elif waves:
            _check(self._L.nka_hip_batch_create_waves(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                      C.c_void_p(stream)), "nka_hip_batch_create_waves", self._L)
        elif wide and ext:
            _check(self._L.nka_hip_batch_create_wide_ext(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                         C.c_void_p(stream), 1 if step else 0), "nka_hip_batch_create_wide_ext", self._L)
        elif wide and step:
            _check(self._L.nka_hip_batch_create_wide_step(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device),
                                                          C.c_void_p(stream)), "nka_hip_batch_create_wide_step", self._L)
        else:
            create = self._L.nka_hip_batch_create_wide if wide else self._L.nka_hip_batch_create
            _check(create(C.byref(h), int(nsys), int(vlen), int(mvec), 0.01, int(flavor), int(device), C.c_void_p(stream)),
                   "nka_hip_batch_create_wide" if wide else "nka_hip_batch_create", self._L)
        self._h, self._device, self._nsys, self._vlen, self._mvec = h, device, int(nsys), int(vlen), int(mvec)
        self._stream, self._follow_torch_stream = int(stream), explicit_stream is None
        return self

    def delete(self):
        if self._h is not None:
            self._L.nka_hip_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise NKAError("nka_batch object used before init")
        return self._h

    def _follow(self):
        if self._follow_torch_stream:      # stay on torch's CURRENT stream (e.g. inside `with torch.cuda.stream(s)`)
            import torch
            cur = int(torch.cuda.current_stream(self._device).cuda_stream)
            if cur != self._stream:
                self.set_stream(cur)

    def _mask(self, active, what):
        """-> device address of the int32 mask, or None for all systems."""
        if active is None:
            return None
        import torch
        if not (isinstance(active, torch.Tensor) and active.is_cuda and active.dtype == torch.int32 and active.is_contiguous()
                and active.dim() == 1 and active.device.index == self._device):
            raise NKAError(f"{what}: the mask must be a contiguous 1-d int32 CUDA tensor on the batch's device, or None")
        if active.numel() != self._nsys:
            raise NKAError(f"{what}: the mask must have one entry per system ({self._nsys}), got {active.numel()}")
        return C.c_void_p(active.data_ptr())

    def set_stream(self, stream: int):
        _check(self._L.nka_hip_batch_set_stream(self._handle(), C.c_void_p(int(stream))), "batch_set_stream", self._L)
        self._stream = int(stream)

    def _rows(self, F, what):
        """-> (device address, row stride) of nsys rows of vlen float64 elements."""
        import torch
        if not (isinstance(F, torch.Tensor) and F.is_cuda and F.dtype == torch.float64 and F.dim() == 2):
            raise NKAError(f"{what}: need a 2-d float64 CUDA tensor, one row per system")
        if F.shape[0] != self._nsys or F.shape[1] != self._vlen:
            raise NKAError(f"{what}: need {self._nsys} rows of {self._vlen} elements, got {tuple(F.shape)}")
        if (self._vlen > 1 and F.stride(1) != 1) or (self._nsys > 1 and F.stride(0) < self._vlen):
            raise NKAError(f"{what}: the rows must be contiguous (element stride 1) and must not overlap")
        if F.device.index != self._device:
            raise NKAError(f"{what}: tensor lives on another device than the batch")
        ld = int(F.stride(0)) if self._nsys > 1 else max(int(F.stride(0)), self._vlen)
        return C.c_void_p(F.data_ptr()), ld

    def _per_system(self, v, what, name):
        """-> device address of nsys float64 entries, or None."""
        if v is None:
            return None
        import torch
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 and v.is_contiguous() and v.dim() == 1
                and v.device.index == self._device):
            raise NKAError(f"{what}: {name} must be a contiguous 1-d float64 CUDA tensor on the batch's device, or None")
        if v.numel() != self._nsys:
            raise NKAError(f"{what}: {name} must have one entry per system ({self._nsys}), got {v.numel()}")
        return C.c_void_p(v.data_ptr())

    def accel_update(self, F, active=None):
        """F: 2-d float64 CUDA tensor, one row per system (nsys x vlen; rows contiguous, the row stride is `ld`), updated in
        place, asynchronously on the batch's stream.  active: optional int32 CUDA tensor of nsys entries, 0 = the system sits
        this call out (its row and its state are not touched)."""
        h = self._handle()
        ptr, ld = self._rows(F, "batch accel_update")
        mask = self._mask(active, "batch accel_update")
        self._follow()
        _check(self._L.nka_hip_batch_accel_update(h, ptr, ld, mask), "batch_accel_update", self._L)
        return F

    def accel_step(self, F, X=None, active=None, tol=None, fnorm=None):
        """One solve step per system active on entry, in the one launch of accel_update (nka_hip_batch_accel_step; include/
        nka_hip_batch.h, STEP): fnorm[sys] = sqrt(dp(f, f)) with the batch's own dot product; if that is <= tol[sys] the system
        retires itself -- active[sys] = 0, nothing else of it written --, otherwise F's row is updated as by accel_update and
        X's row becomes X - F.  X: like F, with its own row stride, not overlapping F.  active: as in accel_update, but WRITTEN.
        tol, fnorm: contiguous 1-d float64 CUDA tensors of nsys entries; tol needs active.  Each may be None.  A wide batch
        offers it only when created with step=True, and then as four launches in a line (offers_step())."""
        h = self._handle()
        what = "batch accel_step"
        ptr, ld = self._rows(F, what)
        xptr, ldx = self._rows(X, what + ": X") if X is not None else (None, 0)
        mask = self._mask(active, what)
        tolp, fnp = self._per_system(tol, what, "tol"), self._per_system(fnorm, what, "fnorm")
        if tolp is not None and mask is None:
            raise NKAError(f"{what}: tol needs a mask (a system retires by clearing its entry of `active`)")
        self._follow()
        _check(self._L.nka_hip_batch_accel_step(h, ptr, ld, xptr, ldx, mask, tolp, fnp), "batch_accel_step", self._L)
        return F

    def restart(self, active=None):
        mask = self._mask(active, "batch restart")
        self._follow()
        _check(self._L.nka_hip_batch_restart(self._handle(), mask), "batch_restart", self._L)

    def relax(self, active=None):
        mask = self._mask(active, "batch relax")
        self._follow()
        _check(self._L.nka_hip_batch_relax(self._handle(), mask), "batch_relax", self._L)

    def set_vec_tol(self, vtol: float):
        """For ALL systems; ordered on the stream like the updates around it."""
        self._follow()
        _check(self._L.nka_hip_batch_set_vec_tol(self._handle(), float(vtol)), "batch_set_vec_tol", self._L)

    def set_sum_order(self, order: int):
        """SUMS_AUTO (reference order up to 64 elements, else SUMS_BLOCKED_ROUNDED), SUMS_REFERENCE_ORDER or
        SUMS_BLOCKED_ROUNDED; SUMS_BLOCKED is refused.  A batch with binary32 storage refuses SUMS_REFERENCE_ORDER, and its
        SUMS_AUTO is SUMS_BLOCKED_ROUNDED at every length.  Returns self."""
        _check(self._L.nka_hip_batch_set_sum_order(self._handle(), int(order)), "batch_set_sum_order", self._L)
        return self

    def set_scalar_step(self, how: int):
        """SCALAR_ONE_THREAD (the default) or SCALAR_WAVEFRONT: how a wide batch runs the third launch of an update or step
        (include/nka_hip_batch.h, SCALAR STEP), and a wave batch of rows=True and a default batch of narrow_rows=True phase 4 of
        their one launch (WAVES ROWS, NARROW ROWS) -- the Gram row, the Cholesky with its drop decisions, both substitutions and the
        combine plan on one thread, or the same arithmetic spread over one wavefront.  Both leave the same bits, so switching
        between calls changes no result.  Enqueue-side state only: no synchronisation, no allocation; applies from the next
        accel_update / accel_step on, and a captured call keeps the step it was captured with.  SCALAR_WAVEFRONT on a batch that
        does not offer it (offers_scalar_step()) and any other value raise NKAError and the batch stays usable.  A batch of
        narrow_rows=True has the wavefront step for the fast sums only: SCALAR_WAVEFRONT while it forms its sums in the reference
        order (explicitly, or SUMS_AUTO at vlen <= 64), and set_sum_order to such an order while SCALAR_WAVEFRONT is set, raise
        NKAError (NKA_HIP_ESTATE) -- nothing is silently downgraded.  Returns self."""
        _check(self._L.nka_hip_batch_set_scalar_step(self._handle(), int(how)), "batch_set_scalar_step", self._L)
        return self

    def scalar_step(self) -> int:
        """SCALAR_ONE_THREAD or SCALAR_WAVEFRONT: what the next call of a wide batch, a wave batch of rows=True or a default batch of
        narrow_rows=True runs with (nka_hip_batch_scalar_step); every other batch: SCALAR_ONE_THREAD."""
        r = self._L.nka_hip_batch_scalar_step(self._handle())
        _check(min(r, 0), "batch_scalar_step", self._L)
        return r

    def offers_scalar_step(self) -> bool:
        """True where set_scalar_step(SCALAR_WAVEFRONT) is offered: every wide batch, with or without step=True, ext=True or
        wide_storage=STORE_F32, a wave batch of init(..., waves=True, rows=True) and a default batch of init(..., narrow_rows=True),
        either storage (nka_hip_batch_offers_scalar_step)."""
        r = self._L.nka_hip_batch_offers_scalar_step(self._handle())
        _check(min(r, 0), "batch_offers_scalar_step", self._L)
        return bool(r)

    def set_dot_weights(self, w):
        """Diagonal weights of the dot product, <x,y>_w = sum_i w_i x_i y_i per system (include/nka_hip_batch.h, WEIGHTS): a
        float64 CUDA tensor on the batch's device or a numpy array, 1-d of vlen entries (one row shared by all systems) or 2-d
        nsys x vlen (row `sys` weights system `sys`; element stride 1, the row stride is `ldw`); None: plain sums again.
        Finite and >= 0; copied, so `w` is free again on return.  Synchronises; applies from the next update on -- follow it
        with restart().  Offered by the default batch, by a wave batch created with ext=True and by a wide batch created with
        ext=True (offers_weights()); every other kind raises NKAError and stays usable.  Returns self."""
        import torch
        h = self._handle()
        what = "batch set_dot_weights"
        if w is None:
            self._follow()
            _check(self._L.nka_hip_batch_set_dot_weights(h, None, 0), "batch_set_dot_weights", self._L)
            return self
        if isinstance(w, torch.Tensor):
            if not (w.is_cuda and w.dtype == torch.float64 and w.device.index == self._device):
                raise NKAError(f"{what}: a tensor must be float64 and live on the batch's device")
            shape, strides = tuple(w.shape), tuple(w.stride())
            entry, ptr = self._L.nka_hip_batch_set_dot_weights, w.data_ptr()
        elif isinstance(w, np.ndarray):
            if w.dtype != np.float64 or w.strides is None or any(st % 8 for st in w.strides):
                raise NKAError(f"{what}: an array must be float64")
            shape, strides = tuple(w.shape), tuple(st // 8 for st in w.strides)
            entry, ptr = self._L.nka_hip_batch_set_dot_weights_host, w.ctypes.data
        else:
            raise NKAError(f"{what}: need a float64 CUDA tensor, a numpy array or None")
        if shape == (self._vlen,):
            if self._vlen > 1 and strides[0] != 1:
                raise NKAError(f"{what}: the element stride must be 1")
            ldw = 0
        elif shape == (self._nsys, self._vlen):
            if (self._vlen > 1 and strides[1] != 1) or (self._nsys > 1 and strides[0] < self._vlen):
                raise NKAError(f"{what}: the rows must be contiguous (element stride 1) and must not overlap")
            ldw = int(strides[0]) if self._nsys > 1 else max(int(strides[0]), self._vlen)
        else:
            raise NKAError(f"{what}: need {self._vlen} entries (shared) or {self._nsys} rows of {self._vlen}, got {shape}")
        self._follow()
        _check(entry(h, C.c_void_p(ptr), ldw), "batch_set_dot_weights", self._L)
        return self

    def dot_weighted(self) -> bool:
        """True while diagonal dot-product weights are set (nka_hip_batch_dot_weighted)."""
        r = self._L.nka_hip_batch_dot_weighted(self._handle())
        _check(min(r, 0), "batch_dot_weighted", self._L)
        return r == 1

    def set_lengths(self, lens):
        """Per-system lengths, 1 <= lens[sys] <= vlen (include/nka_hip_batch.h, LENGTHS): system `sys` is lens[sys] elements
        long in every phase of an update or step, and nothing from there on is read or written in its rows of F and X, its
        weight row or its slots -- a ragged batch without padding weights, on both kinds of batch.  lens: a contiguous 1-d
        int32 CUDA tensor on the batch's device, a numpy integer array or a sequence, nsys entries; None: vlen everywhere
        again.  Copied and validated (an invalid length raises and leaves the previous lengths in force).  Synchronises;
        applies from the next update on -- follow it with restart() for the systems whose length changed.  The tensors F and
        X keep their shape, nsys x vlen.  Returns self."""
        import torch
        h = self._handle()
        what = "batch set_lengths"
        if lens is None:
            self._follow()
            _check(self._L.nka_hip_batch_set_lengths(h, None), "batch_set_lengths", self._L)
            return self
        if isinstance(lens, torch.Tensor):
            if not (lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and lens.dim() == 1
                    and lens.device.index == self._device):
                raise NKAError(f"{what}: a tensor must be a contiguous 1-d int32 CUDA tensor on the batch's device")
            if lens.numel() != self._nsys:
                raise NKAError(f"{what}: need one length per system ({self._nsys}), got {lens.numel()}")
            self._follow()
            _check(self._L.nka_hip_batch_set_lengths(h, C.c_void_p(lens.data_ptr())), "batch_set_lengths", self._L)
            return self
        arr = np.asarray(lens)
        if arr.ndim != 1 or arr.size != self._nsys or not np.issubdtype(arr.dtype, np.integer):
            raise NKAError(f"{what}: need {self._nsys} integers (an int32 CUDA tensor, a numpy integer array, a sequence or None)")
        if (arr < -2**31).any() or (arr >= 2**31).any():      # (the cast to int32 below must not wrap a wide integer into range)
            raise NKAError(f"{what}: every length must be 1 ... vlen = {self._vlen} (the previous lengths stay in force)")
        arr = np.ascontiguousarray(arr, dtype=np.int32)
        self._follow()
        _check(self._L.nka_hip_batch_set_lengths_host(h, arr.ctypes.data_as(_lib._i32p)), "batch_set_lengths_host", self._L)
        return self

    def lengths(self) -> np.ndarray:
        """The length every system runs with at the next update: vlen everywhere while none are set."""
        h = self._handle()
        out = np.zeros(self._nsys, np.int32)
        _check(self._L.nka_hip_batch_get_lengths(h, out.ctypes.data_as(_lib._i32p)), "batch_get_lengths", self._L)
        return out

    def has_lengths(self) -> bool:
        """True while per-system lengths are set (nka_hip_batch_has_lengths)."""
        r = self._L.nka_hip_batch_has_lengths(self._handle())
        _check(min(r, 0), "batch_has_lengths", self._L)
        return r == 1

    # -- queries (synchronise) ---------------------------------------------
    def num_sys(self) -> int:
        return self._nsys

    def vec_len(self) -> int:
        return self._vlen

    def max_vec(self) -> int:
        return self._mvec

    def flavor(self) -> int:
        return self._L.nka_hip_batch_flavor(self._handle())

    def storage(self) -> int:
        """STORE_F64 or STORE_F32: how the batch keeps its normalised subspace vectors (nka_hip_batch_storage)."""
        r = self._L.nka_hip_batch_storage(self._handle())
        _check(min(r, 0), "batch_storage", self._L)
        return r

    def vector_bytes(self) -> int:
        """Bytes of device memory the batch allocated for its stored vectors: slots and, with binary32 storage, the two
        pending buffers (nka_hip_batch_vector_bytes)."""
        r = int(self._L.nka_hip_batch_vector_bytes(self._handle()))
        _check(min(r, 0), "batch_vector_bytes", self._L)
        return r

    def is_wide(self) -> bool:
        """True for a batch created with wide=True (nka_hip_batch_is_wide)."""
        r = self._L.nka_hip_batch_is_wide(self._handle())
        _check(min(r, 0), "batch_is_wide", self._L)
        return r == 1

    def offers_step(self) -> bool:
        """True where accel_step is offered: every kind but a wide batch created without step=True, with or without ext=True
        (nka_hip_batch_offers_step)."""
        r = self._L.nka_hip_batch_offers_step(self._handle())
        _check(min(r, 0), "batch_offers_step", self._L)
        return bool(r)

    def offers_lengths(self) -> bool:
        """True where set_lengths is offered: every kind but a lane batch and a wave batch created without ext=True
        (nka_hip_batch_offers_lengths)."""
        r = self._L.nka_hip_batch_offers_lengths(self._handle())
        _check(min(r, 0), "batch_offers_lengths", self._L)
        return bool(r)

    def offers_weights(self) -> bool:
        """True where set_dot_weights is offered: the default batch (either storage), a wave batch created with ext=True and a
        wide batch created with ext=True (nka_hip_batch_offers_weights)."""
        r = self._L.nka_hip_batch_offers_weights(self._handle())
        _check(min(r, 0), "batch_offers_weights", self._L)
        return bool(r)

    def kind(self) -> int:
        """KIND_NARROW (one workgroup per system), KIND_WIDE, KIND_LANES or KIND_WAVES (nka_hip_batch_kind)."""
        r = self._L.nka_hip_batch_kind(self._handle())
        _check(min(r, 0), "batch_kind", self._L)
        return r

    def num_vec(self) -> np.ndarray:
        out = np.zeros(self._nsys, np.int32)
        _check(self._L.nka_hip_batch_num_vec(self._handle(), out.ctypes.data_as(_lib._i32p)), "batch_num_vec", self._L)
        return out

    def state(self, sys: int) -> State:
        n = self._mvec + 1
        ints = [C.c_int32() for _ in range(5)]
        nxt = np.zeros(n, np.int32)
        prv = np.zeros(n, np.int32)
        h = np.zeros((n, n), np.float64)
        c = np.zeros(n, np.float64)
        _check(self._L.nka_hip_batch_get_state(self._handle(), int(sys), *[C.byref(i) for i in ints],
                                               nxt.ctypes.data_as(_lib._i32p), prv.ctypes.data_as(_lib._i32p),
                                               h.ctypes.data_as(_lib._dp), c.ctypes.data_as(_lib._dp)), "batch_get_state", self._L)
        return State(ints[0].value, ints[1].value, ints[2].value, ints[3].value, ints[4].value, nxt, prv, h.T.copy(), c)

    def reductions(self, sys: int) -> np.ndarray:
        """[<d,d>, <f,w1'>, <w1',w_p>..., <f,w_p>...] of the system's most recent update (zeros where it formed no sum)."""
        out = np.zeros(2 + 2 * self._mvec)
        _check(self._L.nka_hip_batch_get_reductions(self._handle(), int(sys), out.ctypes.data_as(_lib._dp)),
               "batch_get_reductions", self._L)
        return out

    def w(self, sys: int, slot: int) -> np.ndarray:
        out = np.zeros(self._vlen)
        _check(self._L.nka_hip_batch_get_w(self._handle(), int(sys), int(slot), out.ctypes.data_as(_lib._dp)), "batch_get_w", self._L)
        return out

    def v(self, sys: int, slot: int) -> np.ndarray:
        out = np.zeros(self._vlen)
        _check(self._L.nka_hip_batch_get_v(self._handle(), int(sys), int(slot), out.ctypes.data_as(_lib._dp)), "batch_get_v", self._L)
        return out

    def state_digest(self, sys: int) -> int:
        d = C.c_uint64()
        _check(self._L.nka_hip_batch_state_digest(self._handle(), int(sys), C.byref(d)), "batch_state_digest", self._L)
        return int(d.value)
