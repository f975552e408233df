#!/usr/bin/env python3
"""Throughput of the batched accelerator (include/nka_hip_batch.h) against the same systems as lone handles.

Two contenders on the same inputs, alternated in ONE process, profiler off, device events around windows of at least
--window seconds, every shape warmed, median of --repeats windows:
  (a) nka_hip_batch_accel_update: the whole batch in one launch;
  (b) nsys lone nka_hip_accel_update handles, one after another on one stream, called straight through the C ABI (no
      Python wrapper between two updates).
Steady state, full list, default flavour and default sums.  Before every update both contenders copy the next of
mvec + 3 random input sets into their f (device to device; the same cost on both sides, so the ratio (b)/(a) is, if
anything, understated): inputs must not repeat while their difference is still in the subspace, or it collapses.

Per grid point: updates/s of the whole batch (a), bytes moved 8*nsys*vlen*(11+L+k) (compact storage, L = mvec - 1 older
vectors in the sums, k = mvec combined) over time as a share of 8 TB/s, and the ratio time(b)/time(a); the bar for
nsys >= 16 is 1.06.  --probe-vlens / --probe-nsys add points beyond the grid (to find the length at which the loop over
lone handles catches up: the cap NKA_HIP_BATCH_MAX_VLEN).  Every line is flushed as it is measured.

--weights measures something else, with the same windows and the same alternation: three batches on the same inputs -- plain
sums, diagonal weights in the form all systems share (nka_hip_batch_set_dot_weights, ldw = 0) and one row of weights per
system -- and no lone handles.  Weights 2^U(-3, 3).  Per point: the time of an update of each and the two ratios
weighted / plain, beside the ratio of the streams an update reads or writes per element: 2 + 6 G + (7 + k) without weights
(norm pass 2; G = ceil(L / 4) sweeps of 6; combine 7 + k in compact storage), 3 + 7 G + (7 + k) with them.  No bar.

--step measures the solve step (nka_hip_batch_accel_step), again with the same windows and alternation, three variants of one
iteration on the same inputs (the copy of the next input into F stands for the caller's residual in all three):
  (a) nka_hip_batch_accel_update alone;
  (b) what a caller composes from accel_update: torch.linalg.vector_norm(F, dim=1), the mask update (r > tol, written straight
      into the int32 mask: the cheapest form, one launch), accel_update under the mask, and the masked X -= F (one addcmul);
  (c) accel_step with X, the mask, tol and fnorm.
tol = 0 with residuals that are never zero, so no system retires in (b) or (c).  Per point: the three times, (c)/(b) with the
spread of the windows -- the condition is that (c) is not slower than (b) by more than that spread -- and (c)/(a) beside the
ratio of streams per element, 2 + 6 G + (9 + k) over 2 + 6 G + (7 + k): the step reads and writes x in the combine.

--wide measures the wide batch (nka_hip_batch_create_wide: a system split across workgroups, four launches per update), same
windows, same alternation, on the same inputs:
  (a) the wide batch;
  (b) the same systems as lone handles in a loop on one stream;
  (c) the narrow batch, where vlen <= NKA_HIP_BATCH_MAX_VLEN.
Grid nsys 4,16,64,256 x vlen 4096,16384,32768,65536,262144,1048576 x mvec 10,20; a point whose stored vectors (one contender's
slots) exceed --slots-gb is skipped and listed.  The bar of 1.06 on time(b)/time(a) applies at nsys >= 16 and vlen 32768 or
65536; every other point is recorded without one.  The line at the top names the chunk and the cap of the library loaded
(NKA_HIP_LIB: a candidate build of another chunk).

--lengths measures per-system lengths (nka_hip_batch_set_lengths) with the method of --weights -- same inputs, variants
alternated in one process, the same windows:
  (a) a plain batch at vlen;
  (b) the zero-weight recipe: one weight row per system, 1 below the system's length and 0 from there on (narrow only);
  (c) per-system lengths;
(b) and (c) twice: every length = vlen, and lengths from a fixed seed, uniform in [vlen / 4, vlen].  Narrow points nsys 256,4096 x
vlen 1024,16384 x mvec 10,20; wide points, (a) and (c) only, (16, 65 536) and (64, 262 144) x mvec 10,20.  Two conditions, both
against code that exists without (c): with every length = vlen (c) is not slower than (a) beyond the spread of the five windows;
with ragged lengths (c) is not slower than (b) on the same lengths beyond that spread.  A point that misses is marked, not tuned.

--lanes measures the lane batch (nka_hip_batch_create_lanes: one lane per system) with the method of --store32:
  (a) a narrow batch at SUMS_AUTO; (a') a second one, the control; (b) the lane batch;
nsys 256,4096,65536 x vlen 8,32,64 x mvec 5,10,20 with accel_update, then accel_step with X, mask, tol and fnorm at vlen 32.  The
condition at nsys >= 4096: (b) takes less time than (a) by more than the control's difference and the spread of the windows.

--waves measures the wave batch (nka_hip_batch_create_waves: one wavefront per system, four systems per workgroup) with the same
method:
  (a) a narrow batch at SUMS_BLOCKED_ROUNDED; (a') a second one, the control; (b) the wave batch;
nsys 256,4096,65536 x vlen 65,128,256,512,1024,2048,4096 x mvec 5,10,20 with accel_update, then accel_step with X, mask, tol and
fnorm at vlen 256 x mvec 10,20; a point that needs more than --mem-gb (here 40) is skipped and listed, and so is a vlen beyond
the cap of the library loaded (a candidate build with a larger NKA_HIP_BATCH_WAVES_MAX_VLEN measures the lengths that decide
the cap).  THE CAP RULE, evaluated at the end: the largest power of two v such that at nsys = 4096, at every vlen <= v of the grid
and every mvec, (b) takes less time than (a) by more than |a - a'|; 128 if that holds nowhere.

--waves-ext measures the wave batch with lengths and weights (nka_hip_batch_create_waves_ext) with the method of --waves -- same
inputs, the variants alternated in one process, flavour C, SUMS_BLOCKED_ROUNDED, full lists:
  (a) a narrow batch with ragged lengths, uniform in [vlen / 4, vlen] from a fixed seed; (a') the same again, the control;
  (b) an ext wave batch with the same lengths;
  (c) a plain wave batch, without lengths; (d) an ext batch with every length = vlen: (d) against (c) is what the length argument costs;
  (e) a narrow batch with one weight row per system; (f) an ext batch with the same weights.
nsys 4096 x vlen 128,256,1024 x mvec 10,20, then 65 536 x 256 x 10; a point that needs more than --mem-gb (here 40) is skipped and
listed.  (b) won against (a) when a - b > |a - a'|, and (f) against (e) by the same rule; every point is recorded, lost ones too.

--wide-step measures the solve step of a wide batch (nka_hip_batch_create_wide_step) with the method of --step on wide batches:
  (a) accel_update of a plain wide batch;
  (b) the loop a caller composes from it: vector_norm, the mask update, accel_update under the mask, the masked X -= F;
  (b') the same loop a second time, on a batch of its own: the control;
  (c) accel_step with X, the mask, tol and fnorm on a batch of the new entry, no system retiring.
nsys 16,64,256 x vlen 32768,65536,262144 x mvec 10,20; a point that needs more than --mem-gb (here 40) is skipped and listed.  No
ratio is fixed: a point counts as won when b - c > |b - b'|, as lost when c - b > |b - b'|, and is level otherwise.

--wide-weights measures diagonal dot weights on wide batches (nka_hip_batch_create_wide_ext) with the method of --weights:
  (a) a plain wide batch; (a') the same again, the control;
  (b) an ext batch with one shared weight row; (c) an ext batch with one weight row per system;
  (d) an ext batch with nothing set: it launches the kernels of (a), so (d)/(a) should lie within |a - a'| / a;
  (e) a loop over lone handles with nka_hip_set_dot_weights, the only thing such a caller had before.
nsys 16,64,256 x vlen 32768,262144 x mvec 10,20 with accel_update, then accel_step with X, mask, tol and fnorm at 64 x 65536 (no
(e) there); a point that needs more than --mem-gb (here 40) is skipped and listed.  Beside b/a and c/a stands the stream model's
prediction (norm 2 -> 3 streams, each sweep of four 6 -> 7, combine unchanged).  No ratio is fixed: (c) won against (e) when
e - c > |a - a'|.

--wide-store32 measures binary32 storage of a wide batch (nka_hip_batch_create_wide_stored) with the method of --store32:
  (a) a binary64 wide batch of nka_hip_batch_create_wide; (a') the same again, the control; (b) the binary32 wide batch.
nsys 16,64,256 x vlen 32768,65536,262144 x mvec 10,20 with accel_update, then accel_step with X, mask, tol and fnorm at 64 x 65536
x 20; a point that needs more than --mem-gb (here 40) is skipped and listed; vector_bytes is held to the formula at every point.
The condition, fixed before measuring: at 256 x 65536, both mvec, a - b > |a - a'| + the largest window spread of the point.  The
byte model of --store32 stands beside b/a as a prediction.

--wide-rows measures the scalar step of a wide batch on one wavefront (nka_hip_batch_set_scalar_step) with the method of
--wide-store32:
  (a) a wide batch with the one-thread step; (a') the same again, the control; (b) a wide batch with NKA_HIP_BATCH_SCALAR_WAVEFRONT;
  (e) at nsys = 4 only: a loop over four lone handles on one stream.
nsys 4,16,64,256 x vlen 32768,65536,262144 x mvec 5,10,20,32 with accel_update, then accel_step with X, mask, tol and fnorm at 16 x
65536 x 20; a point that needs more than --mem-gb (here 40) is skipped and listed.  The condition, fixed before measuring: at 16 x
65536 x 20, a - b > |a - a'| + the largest window spread of the point.  Whether four systems at mvec = 20 stop losing to four
lone handles (e/b against e/a) is recorded without a bar.

--waves-rows measures the scalar step of a wave batch on the whole wavefront (nka_hip_batch_create_waves_rows with
nka_hip_batch_set_scalar_step) with the method of --wide-rows:
  (a) a wave batch of nka_hip_batch_create_waves, one lane runs the step; (a') the same again, the control; (b) a wave batch of
  the new entry with NKA_HIP_BATCH_SCALAR_WAVEFRONT; (n) at nsys = 256 only: a narrow batch at NKA_HIP_SUMS_BLOCKED_ROUNDED.
nsys 256,4096,65536 x vlen 65,256,1024 x mvec 5,10,20 and the cap of nka_hip_batch_waves_rows_limits with accel_update, then
accel_step with X, mask, tol and fnorm at 4096 x 256 x 10 and x 20; a point that needs more than --mem-gb (here 40) is skipped and
listed.  The condition, fixed before measuring: at 4096 x 256 x 20 and at 256 x 256 x 20, a - b > |a - a'| + the largest window
spread of the three.  Every point is judged won / lost / inside the noise by that rule; whether the wave batch still loses to the
narrow batch at 256 systems is recorded without a bar.

--rows measures the scalar step of a narrow batch on one wavefront (nka_hip_batch_create_rows with nka_hip_batch_set_scalar_step)
with the method of --wide-rows:
  (a) a narrow batch of nka_hip_batch_create_rows left at the one-thread step; (a') the same again, the control; (b) a narrow batch of
  the same entry with NKA_HIP_BATCH_SCALAR_WAVEFRONT; (w) at vlen <= 1024 only: a wave batch of nka_hip_batch_create_waves_rows with
  NKA_HIP_BATCH_SCALAR_WAVEFRONT.
nsys 16,256,4096 x vlen 256,1024,4096,16384 x mvec 5,10,20,32 with accel_update (the wave batch stops at its cap on mvec); a point
that needs more than --mem-gb (here 40) is skipped and listed.  The condition, fixed before measuring: at 256 x 4096 x 20, a - b >
|a - a'| + the largest window spread of the three.  Every point is judged won / lost / inside the noise by that rule; b/w is
recorded without a bar."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
BAR = 1.06


def measure(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    npool = mvec + 3
    need = 8.0 * nsys * vlen * (2 * 2 * (mvec + 1) + npool + 2)          # both contenders' slots, the pool, two f
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    Fa = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
    Fb = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
    batch = nka_amd.nka_batch().init(nsys, vlen, mvec)
    lones = [nka_amd.nka().init(vlen, mvec) for _ in range(nsys)]
    hb = batch._handle()
    hl = [a._handle() for a in lones]
    pl = [C.c_void_p(Fb[k].data_ptr()) for k in range(nsys)]
    pa, ld = C.c_void_p(Fa.data_ptr()), int(Fa.stride(0)) if nsys > 1 else vlen
    upd_a, upd_b = L.nka_hip_batch_accel_update, L.nka_hip_accel_update
    step = [0]

    def run_a(reps):
        for _ in range(reps):
            Fa.copy_(pool[step[0] % npool])
            step[0] += 1
            assert upd_a(hb, pa, ld, None) == 0

    def run_b(reps):
        for _ in range(reps):
            Fb.copy_(pool[step[0] % npool])
            step[0] += 1
            for k in range(nsys):
                if upd_b(hl[k], pl[k]) != 0:
                    raise RuntimeError(L.nka_hip_last_error())

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    for fn in (run_a, run_b):                      # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        fn(mvec + 4)
    torch.cuda.synchronize()
    assert (batch.num_vec() == mvec).all() and lones[0].num_vec() == mvec and lones[-1].num_vec() == mvec
    reps = {}
    for name, fn in (("a", run_a), ("b", run_b)):
        t = timed(fn, 3)
        reps[name] = max(3, int(window / t) + 1)
    ta, tb = [], []
    for _ in range(repeats):                       # alternate the contenders
        ta.append(timed(run_a, reps["a"]))
        tb.append(timed(run_b, reps["b"]))
    assert (batch.num_vec() == mvec).all() and lones[0].num_vec() == mvec
    a, b = statistics.median(ta), statistics.median(tb)
    nbytes = 8.0 * nsys * vlen * (11 + (mvec - 1) + mvec)
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec, t_batch_us=a * 1e6, t_lone_us=b * 1e6, updates_per_s=1.0 / a,
               system_updates_per_s=nsys / a, share_of_peak=nbytes / a / PEAK, ratio=b / a, reps_a=reps["a"], reps_b=reps["b"],
               spread_a=(max(ta) - min(ta)) / a, spread_b=(max(tb) - min(tb)) / b)
    for x in lones:
        x.delete()
    batch.delete()
    del pool, Fa, Fb
    torch.cuda.empty_cache()
    return out


def measure_weights(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    npool = mvec + 3
    need = 8.0 * nsys * vlen * (3 * 2 * (mvec + 1) + npool + 3 + 2)       # three batches' slots, the pool, three f, weights
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    w = torch.exp2(6.0 * torch.rand(nsys, vlen, dtype=torch.float64, device="cuda") - 3.0)
    forms = {"plain": None, "shared": w[0], "rows": w}
    Fs, hs, batches = {}, {}, {}
    for name, wf in forms.items():
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec).set_dot_weights(wf)
        hs[name] = batches[name]._handle()
    assert [b.dot_weighted() for b in batches.values()] == [False, True, True]
    ld = int(Fs["plain"].stride(0)) if nsys > 1 else vlen
    upd = L.nka_hip_batch_accel_update
    step = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[step[0] % npool])
            step[0] += 1
            assert upd(h, p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in forms}
    for name in forms:                             # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    for name in forms:
        assert (batches[name].num_vec() == mvec).all(), name
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in forms:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    for name in forms:
        assert (batches[name].num_vec() == mvec).all(), name
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
        batches[name].delete()
    del pool, w, forms, Fs
    torch.cuda.empty_cache()
    return out


def store32_bytes_model(mvec):
    """Bytes an update moves per element at a full list, default flavour, re-reads of f and w1 counted as memory: norm pass 16;
    each sweep of four older vectors 48 with binary64 storage, 32 with binary32; combine of k = mvec pairs 8 (7 + k) and
    56 + 4 (k - 1).  -> (binary64, binary32)"""
    g = (mvec - 1 + 3) // 4
    return 16 + 48 * g + 8 * (7 + mvec), 16 + 32 * g + 56 + 4 * (mvec - 1)


def measure_store32(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    """(a) a binary64 batch, flavour C; (a') a second one of the same shape, the control for what two allocations alone do to
    two batches of equal work; (b) the binary32 batch.  Same inputs, alternated, as measure_weights."""
    npool = mvec + 3
    stride = (vlen + 31) // 32 * 32
    vec = {s: 2 * nsys * stride * (8 * (mvec + 1) if s == nka_amd.STORE_F64 else 4 * (mvec + 1) + 8) for s in (nka_amd.STORE_F64, nka_amd.STORE_F32)}
    need = 2 * vec[nka_amd.STORE_F64] + vec[nka_amd.STORE_F32] + 8.0 * nsys * vlen * (npool + 3)
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    forms = {"a": nka_amd.STORE_F64, "a2": nka_amd.STORE_F64, "b": nka_amd.STORE_F32}
    Fs, hs, batches = {}, {}, {}
    for name, storage in forms.items():
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, storage=storage)
        assert batches[name].storage() == storage and batches[name].vector_bytes() == vec[storage], name
        hs[name] = batches[name]._handle()
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd = L.nka_hip_batch_accel_update
    step = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[step[0] % npool])
            step[0] += 1
            assert upd(h, p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in forms}
    for name in forms:                             # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    for name in forms:
        assert (batches[name].num_vec() == mvec).all(), name
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in forms:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec, bytes_a=vec[nka_amd.STORE_F64], bytes_b=vec[nka_amd.STORE_F32])
    for name in forms:
        assert (batches[name].num_vec() == mvec).all(), name
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
        batches[name].delete()
    del pool, Fs
    torch.cuda.empty_cache()
    return out


def store32_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    if args.store32_extra:
        points.append((4096, 64, 10))
    emit(f"# one update of (a) a binary64 batch, (a') a second binary64 batch of the same shape -- the control -- and (b) a batch "
         f"with binary32 storage (nka_hip_batch_create_stored); {torch.cuda.get_device_name(0)}; windows >= {args.window} s, median "
         f"of {args.repeats}, the three alternated on the same inputs; flavour C, default sums, full list")
    emit("# byte model per element: 16 + 48 G + 8 (7 + k) binary64, 16 + 32 G + 56 + 4 (k - 1) binary32, G = ceil((mvec - 1) / 4), "
         "k = mvec: 308 / 472 = 0.65 at mvec 20, 204 / 296 = 0.69 at 10 (a prediction, not a bar)")
    emit("# CONDITION at 4096 x 16384, both mvec: b/a below 1 by more than the larger of the window spread and |a - a'| / a")
    emit(f"{'nsys':>5} {'vlen':>6} {'mvec':>4} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8} {'model':>6} "
         f"{'vectors a MB':>12} {'vectors b MB':>12} {'b/a mem':>7}  condition")
    t0 = time.time()
    verdicts = []
    for n, v, m in points:
        r = measure_store32(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            emit(f"{n:5d} {v:6d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        b64, b32 = store32_bytes_model(m)
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        noise = max(ctl, r["spread_a"], r["spread_a2"], r["spread_b"])
        cond = "-"
        if (n, v) == (4096, 16384):
            cond = "HELD" if 1.0 - ratio > noise else "MISSED"
            verdicts.append(cond)
        emit(f"{n:5d} {v:6d} {m:4d} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} {ctl:8.3f} "
             f"{b32 / b64:6.3f} {r['bytes_a'] / 1e6:12.1f} {r['bytes_b'] / 1e6:12.1f} {r['bytes_b'] / r['bytes_a']:7.3f}  {cond}   "
             f"(spread a {100 * r['spread_a']:.1f} % a' {100 * r['spread_a2']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# condition: {', '.join(verdicts) if verdicts else 'not measured (no point at 4096 x 16384)'}; {len(points)} points in "
         f"{time.time() - t0:.0f} s")
    return 0


def measure_wide_store32(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, step):
    """(a) a binary64 wide batch of nka_hip_batch_create_wide (step: _create_wide_step), whose kernels are untouched by the binary32
    instances; (a') a second one, the control; (b) the wide batch with binary32 storage (nka_hip_batch_create_wide_stored).  Same
    inputs, alternated, as measure_store32.  step: accel_step with X, mask, tol (nobody retires) and fnorm."""
    npool = mvec + 3
    stride = (vlen + 31) // 32 * 32
    vec = {s: 2 * nsys * stride * (8 * (mvec + 1) if s == nka_amd.STORE_F64 else 4 * (mvec + 1) + 8) for s in (nka_amd.STORE_F64, nka_amd.STORE_F32)}
    need = 2 * vec[nka_amd.STORE_F64] + vec[nka_amd.STORE_F32] + 8.0 * nsys * vlen * (npool + 3 + (3 if step else 0))
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    forms = {"a": nka_amd.STORE_F64, "a2": nka_amd.STORE_F64, "b": nka_amd.STORE_F32}
    Fs, Xs, hs, batches = {}, {}, {}, {}
    for name, storage in forms.items():
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        if storage == nka_amd.STORE_F32:
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, wide=True, wide_storage=storage, step=step)
        else:
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, wide=True, step=step)
        assert batches[name].is_wide() and batches[name].storage() == storage and batches[name].vector_bytes() == vec[storage], name
        hs[name] = batches[name]._handle()
        if step:
            Xs[name] = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    tol = torch.full((nsys,), -1.0, dtype=torch.float64, device="cuda")
    fnorm = torch.zeros(nsys, dtype=torch.float64, device="cuda")
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd, stp = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step
    it = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[it[0] % npool])
            it[0] += 1
            if step:
                assert stp(h, p, ld, C.c_void_p(Xs[name].data_ptr()), ld, C.c_void_p(mask.data_ptr()), C.c_void_p(tol.data_ptr()),
                           C.c_void_p(fnorm.data_ptr())) == 0
            else:
                assert upd(h, p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in forms}
    for name in forms:                             # warm: fill the lists (steady state), settle clocks and caches
        it[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    for name in forms:
        assert (batches[name].num_vec() == mvec).all(), name
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in forms:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec, bytes_a=vec[nka_amd.STORE_F64], bytes_b=vec[nka_amd.STORE_F32])
    for name in forms:
        assert (batches[name].num_vec() == mvec).all() and bool(mask.all()), name
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
        batches[name].delete()
    del pool, Fs, Xs
    torch.cuda.empty_cache()
    return out


def wide_store32_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m, False) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    points.append((64, 65536, 20, True))
    emit(f"# one update of (a) a binary64 wide batch (nka_hip_batch_create_wide), (a') a second one of the same shape -- the control -- "
         f"and (b) a wide batch with binary32 storage (nka_hip_batch_create_wide_stored); {torch.cuda.get_device_name(0)}; windows >= "
         f"{args.window} s, median of {args.repeats}, the three alternated on the same inputs; flavour C, full list; the last row: "
         f"accel_step with X, mask, tol and fnorm (a, a': nka_hip_batch_create_wide_step)")
    emit("# byte model per element: 16 + 48 G + 8 (7 + k) binary64, 16 + 32 G + 56 + 4 (k - 1) binary32, G = ceil((mvec - 1) / 4), "
         "k = mvec: 308 / 472 = 0.65 at mvec 20, 204 / 296 = 0.69 at 10 (a prediction, not a bar)")
    emit("# CONDITION at 256 x 65536, both mvec: a - b > |a - a'| + the largest window spread of the point (x a)")
    emit(f"{'nsys':>5} {'vlen':>7} {'mvec':>4} {'call':>6} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8} {'model':>6} "
         f"{'vectors a MB':>12} {'vectors b MB':>12} {'b/a mem':>7}  condition")
    t0 = time.time()
    verdicts = []
    for n, v, m, step in points:
        r = measure_wide_store32(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, step)
        if r is None:
            emit(f"{n:5d} {v:7d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        b64, b32 = store32_bytes_model(m)
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        spread = max(r["spread_a"], r["spread_a2"], r["spread_b"])
        won = r["a"] - r["b"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        cond = "-"
        if (n, v) == (256, 65536) and not step:
            cond = "HELD" if won else "MISSED"
            verdicts.append(cond)
        emit(f"{n:5d} {v:7d} {m:4d} {'step' if step else 'update':>6} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} "
             f"{ctl:8.3f} {b32 / b64:6.3f} {r['bytes_a'] / 1e6:12.1f} {r['bytes_b'] / 1e6:12.1f} {r['bytes_b'] / r['bytes_a']:7.3f}  {cond}   "
             f"({'won' if won else 'not won'}; spread a {100 * r['spread_a']:.1f} % a' {100 * r['spread_a2']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# condition: {', '.join(verdicts) if verdicts else 'not measured (no point at 256 x 65536)'}; {len(points)} points in "
         f"{time.time() - t0:.0f} s")
    return 0


def measure_wide_rows(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, step, lone):
    """(a) a wide batch with the one-thread scalar step, whose kernels the wavefront instances leave untouched; (a') a second one,
    the control; (b) a wide batch with nka_hip_batch_set_scalar_step(NKA_HIP_BATCH_SCALAR_WAVEFRONT); lone: (e) a loop over nsys
    lone handles on one stream.  Same inputs, alternated, as measure_wide_store32.  step: accel_step with X, mask, tol (nobody
    retires) and fnorm."""
    npool = mvec + 3
    stride = (vlen + 31) // 32 * 32
    nforms = 3 + (1 if lone else 0)
    need = nforms * 16.0 * nsys * stride * (mvec + 1) + 8.0 * nsys * vlen * (npool + nforms + (3 if step else 0))
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    forms = {"a": nka_amd.SCALAR_ONE_THREAD, "a2": nka_amd.SCALAR_ONE_THREAD, "b": nka_amd.SCALAR_WAVEFRONT}
    names = list(forms) + (["e"] if lone else [])
    Fs, Xs, hs, batches = {}, {}, {}, {}
    for name in names:
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
    for name, how in forms.items():
        batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, wide=True, step=step).set_scalar_step(how)
        assert batches[name].is_wide() and batches[name].scalar_step() == how, name
        hs[name] = batches[name]._handle()
        if step:
            Xs[name] = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    lones = [nka_amd.nka().init(vlen, mvec) for _ in range(nsys)] if lone else []
    hl = [x._handle() for x in lones]
    pl = [C.c_void_p(Fs["e"][k].data_ptr()) for k in range(nsys)] if lone else []
    mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    tol = torch.full((nsys,), -1.0, dtype=torch.float64, device="cuda")
    fnorm = torch.zeros(nsys, dtype=torch.float64, device="cuda")
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd, stp, upd_lone = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step, L.nka_hip_accel_update
    it = [0]

    def run(name, reps):
        F = Fs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[it[0] % npool])
            it[0] += 1
            if name == "e":
                for k in range(nsys):
                    if upd_lone(hl[k], pl[k]) != 0:
                        raise RuntimeError(L.nka_hip_last_error())
            elif step:
                assert stp(hs[name], p, ld, C.c_void_p(Xs[name].data_ptr()), ld, C.c_void_p(mask.data_ptr()), C.c_void_p(tol.data_ptr()),
                           C.c_void_p(fnorm.data_ptr())) == 0
            else:
                assert upd(hs[name], p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in names}
    for name in names:                             # warm: fill the lists (steady state), settle clocks and caches
        it[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    assert torch.equal(Fs["a"], Fs["b"]) and torch.equal(Fs["a"], Fs["a2"])      # the same bits, whichever step ran
    for name in names:
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in names:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    for name in forms:
        assert (batches[name].num_vec() == mvec).all() and bool(mask.all()), name
    for name in names:
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
    for b in batches.values():
        b.delete()
    for x in lones:
        x.delete()
    del pool, Fs, Xs
    torch.cuda.empty_cache()
    return out


WIDE_ROWS_CONDITION_AT = (16, 65536, 20)


def wide_rows_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m, False) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    points.append(WIDE_ROWS_CONDITION_AT + (True,))
    emit(f"# one update of (a) a wide batch with the one-thread scalar step, (a') a second one of the same shape -- the control -- and "
         f"(b) a wide batch with nka_hip_batch_set_scalar_step(NKA_HIP_BATCH_SCALAR_WAVEFRONT); (e) at nsys = 4: a loop over four lone "
         f"handles on one stream; {torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of {args.repeats}, the contenders "
         f"alternated on the same inputs; flavour C, full list; the last row: accel_step with X, mask, tol and fnorm "
         f"(nka_hip_batch_create_wide_step)")
    emit(f"# CONDITION at {WIDE_ROWS_CONDITION_AT}: a - b > |a - a'| + the largest window spread of the point (x a); every other point "
         f"and e/a, e/b are recorded without a bar")
    emit(f"{'nsys':>5} {'vlen':>7} {'mvec':>4} {'call':>6} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8} {'e us':>10} "
         f"{'e/a':>6} {'e/b':>6}  condition")
    t0 = time.time()
    verdicts, wins, losses, skipped = [], [], [], []
    for n, v, m, step in points:
        r = measure_wide_rows(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, step, lone=(n == 4 and not step))
        if r is None:
            skipped.append((n, v, m))
            emit(f"{n:5d} {v:7d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        spread = max(r["spread_a"], r["spread_a2"], r["spread_b"])
        won = r["a"] - r["b"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        lost = r["b"] - r["a"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        (wins if won else losses if lost else []).append((n, v, m) + (("step",) if step else ()))
        cond = "-"
        if (n, v, m) == WIDE_ROWS_CONDITION_AT and not step:
            cond = "HELD" if won else "MISSED"
            verdicts.append(cond)
        e_us = f"{r['e'] * 1e6:10.1f} {r['e'] / r['a']:6.2f} {r['e'] / r['b']:6.2f}" if "e" in r else f"{'-':>10} {'-':>6} {'-':>6}"
        emit(f"{n:5d} {v:7d} {m:4d} {'step' if step else 'update':>6} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} "
             f"{ctl:8.3f} {e_us}  {cond}   ({'won' if won else 'lost' if lost else 'inside the noise'}; spread a {100 * r['spread_a']:.1f} % "
             f"a' {100 * r['spread_a2']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# condition: {', '.join(verdicts) if verdicts else 'not measured (no point at ' + str(WIDE_ROWS_CONDITION_AT) + ')'}; won "
         f"{len(wins)}: {wins}; lost {len(losses)}: {losses}; skipped: {skipped if skipped else 'none'}; {len(points)} points in "
         f"{time.time() - t0:.0f} s")
    return 0


def measure_waves_rows(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, step, narrow):
    """(a) a wave batch of nka_hip_batch_create_waves with the one-lane scalar step, whose kernels the wavefront instances leave
    untouched; (a') a second one, the control; (b) a wave batch of nka_hip_batch_create_waves_rows with
    nka_hip_batch_set_scalar_step(NKA_HIP_BATCH_SCALAR_WAVEFRONT); narrow: (n) a narrow batch at the rounded fast sums.  Same
    inputs, alternated, as measure_wide_rows.  step: accel_step with X, mask, tol (nobody retires) and fnorm."""
    npool = mvec + 3
    stride = (vlen + 31) // 32 * 32
    nforms = 3 + (1 if narrow else 0)
    need = nforms * 16.0 * nsys * stride * (mvec + 1) + 8.0 * nsys * vlen * (npool + nforms + (3 if step else 0))
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    names = ["a", "a2", "b"] + (["n"] if narrow else [])
    Fs, Xs, hs, batches = {}, {}, {}, {}
    for name in names:
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        if name == "b":
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, waves=True, rows=True)
            batches[name].set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
            assert batches[name].scalar_step() == nka_amd.SCALAR_WAVEFRONT
        elif name == "n":
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C).set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        else:
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, waves=True)
            assert not batches[name].offers_scalar_step()
        assert batches[name].kind() == (nka_amd.KIND_NARROW if name == "n" else nka_amd.KIND_WAVES), name
        hs[name] = batches[name]._handle()
        if step:
            Xs[name] = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
    mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    tol = torch.full((nsys,), -1.0, dtype=torch.float64, device="cuda")
    fnorm = torch.zeros(nsys, dtype=torch.float64, device="cuda")
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd, stp = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step
    it = [0]

    def run(name, reps):
        F = Fs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[it[0] % npool])
            it[0] += 1
            if step:
                assert stp(hs[name], p, ld, C.c_void_p(Xs[name].data_ptr()), ld, C.c_void_p(mask.data_ptr()), C.c_void_p(tol.data_ptr()),
                           C.c_void_p(fnorm.data_ptr())) == 0
            else:
                assert upd(hs[name], p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in names}
    for name in names:                             # warm: fill the lists (steady state), settle clocks and caches
        it[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    assert torch.equal(Fs["a"], Fs["b"]) and torch.equal(Fs["a"], Fs["a2"])      # the same bits, whichever step ran
    for name in names:
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in names:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    for name in names:
        assert (batches[name].num_vec() == mvec).all() and bool(mask.all()), name
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
    for b in batches.values():
        b.delete()
    del pool, Fs, Xs
    torch.cuda.empty_cache()
    return out


WAVES_ROWS_CONDITION_AT = ((4096, 256, 20), (256, 256, 20))
WAVES_ROWS_STEP_AT = ((4096, 256, 10), (4096, 256, 20))
WAVES_ROWS_NARROW_NSYS = 256


def waves_rows_points(nsys, vlens, mvecs, step=True):
    """The grid of --waves-rows: every update point, then the steps (x, mask, tol, fnorm) where the grid is the default one."""
    points = [(n, v, m, False) for v in vlens for m in mvecs for n in nsys]
    return points + ([p + (True,) for p in WAVES_ROWS_STEP_AT] if step else [])


def waves_rows_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    cap, _ = nka_amd.batch_waves_rows_limits()
    points = waves_rows_points(ints(args.nsys), ints(args.vlens), ints(args.mvecs), step=args.waves_rows_steps)
    # (the condition stands at the head of the record)
    emit(f"# CONDITION, fixed before the run, at {WAVES_ROWS_CONDITION_AT[0]} and at {WAVES_ROWS_CONDITION_AT[1]}: a - b > |a - a'| + the "
         f"largest window spread of the three (x a); every other point is recorded and judged won / lost / inside the noise by the same "
         f"rule, n/a and n/b without a bar")
    emit(f"# one update of (a) a wave batch with the one-lane scalar step (nka_hip_batch_create_waves), (a') a second one of the same "
         f"shape -- the control -- and (b) a wave batch of nka_hip_batch_create_waves_rows with nka_hip_batch_set_scalar_step("
         f"NKA_HIP_BATCH_SCALAR_WAVEFRONT); (n) at nsys = {WAVES_ROWS_NARROW_NSYS}: a narrow batch at NKA_HIP_SUMS_BLOCKED_ROUNDED; "
         f"{torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of {args.repeats}, the contenders alternated on the same "
         f"inputs; flavour C, full lists; the cap on mvec is {cap} ({nka_amd.batch_waves_rows_limits()[1]} bytes of LDS per workgroup; "
         f"{nka_amd.batch_waves_rows_limits(20)[1]} at mvec 20); rows marked step: accel_step with X, mask, tol and fnorm")
    emit(f"{'nsys':>6} {'vlen':>5} {'mvec':>4} {'call':>6} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8} {'n us':>10} "
         f"{'a/n':>6} {'b/n':>6}  condition")
    t0 = time.time()
    verdicts, wins, losses, noise, skipped, narrow = [], [], [], [], [], []
    for n, v, m, step in points:
        r = measure_waves_rows(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, step,
                               narrow=(n == WAVES_ROWS_NARROW_NSYS and not step))
        if r is None:
            skipped.append((n, v, m))
            emit(f"{n:6d} {v:5d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        spread = max(r["spread_a"], r["spread_a2"], r["spread_b"])
        won = r["a"] - r["b"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        lost = r["b"] - r["a"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        (wins if won else losses if lost else noise).append((n, v, m) + (("step",) if step else ()))
        cond = "-"
        if (n, v, m) in WAVES_ROWS_CONDITION_AT and not step:
            cond = "HELD" if won else "MISSED"
            verdicts.append(f"{cond} at {(n, v, m)}")
        if "n" in r:
            narrow.append(((n, v, m), r["a"] / r["n"], r["b"] / r["n"]))
            n_us = f"{r['n'] * 1e6:10.1f} {r['a'] / r['n']:6.2f} {r['b'] / r['n']:6.2f}"
        else:
            n_us = f"{'-':>10} {'-':>6} {'-':>6}"
        emit(f"{n:6d} {v:5d} {m:4d} {'step' if step else 'update':>6} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} "
             f"{ctl:8.3f} {n_us}  {cond}   ({'won' if won else 'lost' if lost else 'inside the noise'}; spread a {100 * r['spread_a']:.1f} % "
             f"a' {100 * r['spread_a2']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# condition: {'; '.join(verdicts) if verdicts else 'not measured (no point at ' + str(WAVES_ROWS_CONDITION_AT) + ')'}; won "
         f"{len(wins)}: {wins}; lost {len(losses)}: {losses}; inside the noise {len(noise)}: {noise}; skipped: {skipped if skipped else 'none'}; "
         f"{len(points)} points in {time.time() - t0:.0f} s")
    if narrow:
        emit(f"# against the narrow batch at {WAVES_ROWS_NARROW_NSYS} systems (time / narrow's time): the one-lane wave batch "
             f"{min(x[1] for x in narrow):.2f} ... {max(x[1] for x in narrow):.2f}, with the wavefront step {min(x[2] for x in narrow):.2f} ... "
             f"{max(x[2] for x in narrow):.2f}; still slower than the narrow batch at {[x[0] for x in narrow if x[2] > 1.0]}")
    return 0


def measure_rows(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, waves):
    """(a) a narrow batch of nka_hip_batch_create_rows left at the one-thread scalar step, which launches the instances every
    narrow batch launches; (a') a second one, the control; (b) a third with nka_hip_batch_set_scalar_step(
    NKA_HIP_BATCH_SCALAR_WAVEFRONT); waves: (w) a wave batch of nka_hip_batch_create_waves_rows with the wavefront step.  Same inputs,
    alternated, as measure_wide_rows; the fast sums (NKA_HIP_SUMS_AUTO beyond 64 elements)."""
    npool = mvec + 3
    stride = (vlen + 31) // 32 * 32
    names = ["a", "a2", "b"] + (["w"] if waves else [])
    need = len(names) * 16.0 * nsys * stride * (mvec + 1) + 8.0 * nsys * vlen * (npool + len(names))
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    Fs, hs, batches = {}, {}, {}
    for name in names:
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        if name == "w":
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, waves=True, rows=True)
        else:
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, narrow_rows=True)
        assert batches[name].offers_scalar_step() and batches[name].scalar_step() == nka_amd.SCALAR_ONE_THREAD, name
        if name in ("b", "w"):
            batches[name].set_scalar_step(nka_amd.SCALAR_WAVEFRONT)
            assert batches[name].scalar_step() == nka_amd.SCALAR_WAVEFRONT
        assert batches[name].kind() == (nka_amd.KIND_WAVES if name == "w" else nka_amd.KIND_NARROW), name
        hs[name] = batches[name]._handle()
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd = L.nka_hip_batch_accel_update
    it = [0]

    def run(name, reps):
        F = Fs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[it[0] % npool])
            it[0] += 1
            assert upd(hs[name], p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in names}
    for name in names:                             # warm: fill the lists (steady state), settle clocks and caches
        it[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    assert torch.equal(Fs["a"], Fs["b"]) and torch.equal(Fs["a"], Fs["a2"])      # the same bits, whichever step ran
    for name in names:
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in names:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    for name in names:
        assert (batches[name].num_vec() == mvec).all(), name
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
    for b in batches.values():
        b.delete()
    del pool, Fs
    torch.cuda.empty_cache()
    return out


ROWS_CONDITION_AT = (256, 4096, 20)


def rows_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    wcap, _ = nka_amd.batch_waves_rows_limits()
    _, wvlen = nka_amd.batch_waves_limits()
    points = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    # (the condition stands at the head of the record)
    emit(f"# CONDITION, fixed before the run, at {ROWS_CONDITION_AT}: a - b > |a - a'| + the largest window spread of the three (x a); "
         f"every other point is recorded and judged won / lost / inside the noise by the same rule, b/w without a bar")
    emit(f"# one update of (a) a narrow batch of nka_hip_batch_create_rows left at the one-thread scalar step, (a') a second one of the "
         f"same shape -- the control -- and (b) a third with nka_hip_batch_set_scalar_step(NKA_HIP_BATCH_SCALAR_WAVEFRONT); (w) at vlen <= "
         f"{wvlen} and mvec <= {wcap}: a wave batch of nka_hip_batch_create_waves_rows with the wavefront step; "
         f"{torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of {args.repeats}, the contenders alternated on the same "
         f"inputs; flavour C, full lists, the fast sums; dynamic LDS of a wavefront-step launch: {nka_amd.batch_rows_limits(5)} / "
         f"{nka_amd.batch_rows_limits(10)} / {nka_amd.batch_rows_limits(20)} / {nka_amd.batch_rows_limits(32)} bytes at mvec 5 / 10 / 20 / 32")
    emit(f"{'nsys':>6} {'vlen':>5} {'mvec':>4} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8} {'w us':>10} {'b/w':>6}  condition")
    t0 = time.time()
    verdicts, wins, losses, noise, skipped = [], [], [], [], []
    for n, v, m in points:
        r = measure_rows(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, waves=(v <= wvlen and m <= wcap))
        if r is None:
            skipped.append((n, v, m))
            emit(f"{n:6d} {v:5d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        spread = max(r["spread_a"], r["spread_a2"], r["spread_b"])
        won = r["a"] - r["b"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        lost = r["b"] - r["a"] > abs(r["a"] - r["a2"]) + spread * r["a"]
        (wins if won else losses if lost else noise).append((n, v, m))
        cond = "-"
        if (n, v, m) == ROWS_CONDITION_AT:
            cond = "HELD" if won else "MISSED"
            verdicts.append(f"{cond} at {(n, v, m)}")
        w_us = f"{r['w'] * 1e6:10.1f} {r['b'] / r['w']:6.2f}" if "w" in r else f"{'-':>10} {'-':>6}"
        emit(f"{n:6d} {v:5d} {m:4d} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} {ctl:8.3f} {w_us}  {cond}   "
             f"({'won' if won else 'lost' if lost else 'inside the noise'}; spread a {100 * r['spread_a']:.1f} % a' {100 * r['spread_a2']:.1f} % "
             f"b {100 * r['spread_b']:.1f} %)")
    emit(f"# condition: {'; '.join(verdicts) if verdicts else 'not measured (no point at ' + str(ROWS_CONDITION_AT) + ')'}; won "
         f"{len(wins)}: {wins}; lost {len(losses)}: {losses}; inside the noise {len(noise)}: {noise}; skipped: {skipped if skipped else 'none'}; "
         f"{len(points)} points in {time.time() - t0:.0f} s")
    return 0


def measure_lanes(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, step, waves=False):
    """(a) a narrow batch at SUMS_AUTO (vlen <= 64: the reference order); (a') a second one, the control for what two batches
    of equal work differ by; (b) the lane batch.  Same inputs, alternated, as measure_store32.  step: accel_step with X, mask,
    tol (zero: nothing retires) and fnorm instead of accel_update.  waves: (b) is the wave batch, (a) and (a') run the rounded
    fast sums."""
    npool = mvec + 3
    if 8.0 * nsys * ((vlen + 31) // 32 * 32) * (mvec + 1) * 2 * 3 + 8.0 * nsys * vlen * (npool + 8) > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    forms = {"a": False, "a2": False, "b": True}
    Fs, Xs, hs, batches = {}, {}, {}, {}
    mask = torch.ones(nsys, dtype=torch.int32, device="cuda")
    tol, fnorm = torch.zeros(nsys, dtype=torch.float64, device="cuda"), torch.zeros(nsys, dtype=torch.float64, device="cuda")
    for name, lanes in forms.items():
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        Xs[name] = torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda")
        if waves:
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, waves=lanes)
            batches[name].set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
            assert batches[name].kind() == (nka_amd.KIND_WAVES if lanes else nka_amd.KIND_NARROW), name
        else:
            batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, lanes=lanes)
            assert batches[name].kind() == (nka_amd.KIND_LANES if lanes else nka_amd.KIND_NARROW), name
        hs[name] = batches[name]._handle()
    ld = vlen
    upd, stp = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step
    count = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        p, px = C.c_void_p(F.data_ptr()), C.c_void_p(Xs[name].data_ptr())
        for _ in range(reps):
            F.copy_(pool[count[0] % npool])
            count[0] += 1
            if step:
                assert stp(h, p, ld, px, ld, C.c_void_p(mask.data_ptr()), C.c_void_p(tol.data_ptr()), C.c_void_p(fnorm.data_ptr())) == 0
            else:
                assert upd(h, p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in forms}
    for name in forms:                             # warm: fill the lists (steady state), settle clocks and caches
        count[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    nv = batches["a"].num_vec()                    # (vlen < mvec: a list holds at most vlen independent vectors, the same in all three)
    for name in forms:
        assert (batches[name].num_vec() == nv).all(), name
    for name in forms:
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in forms:
            ts[name].append(timed(name, reps[name]))
    assert bool(mask.all()), "a system retired: the windows did not time equal work"
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    for name in forms:
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
    for name in forms:
        batches[name].delete()
    del pool, Fs, Xs
    torch.cuda.empty_cache()
    return out


def lanes_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m, False) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    points += [(n, 32, m, True) for m in ints(args.mvecs) for n in ints(args.nsys)]
    emit(f"# one call of (a) a narrow batch at SUMS_AUTO (one workgroup of 256 threads per system; its kernels are the parent "
         f"commit's), (a') a second narrow batch of the same shape -- the control -- and (b) the lane batch "
         f"(nka_hip_batch_create_lanes: one lane per system); {torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of "
         f"{args.repeats}, the three alternated on the same inputs; flavour C, full list; the time includes the copy of the input "
         f"into F (equal for the three)")
    emit("# systems per workgroup of (b): " + ", ".join(f"mvec {m}: {nka_amd.batch_lanes_limits(m)[0]}" for m in ints(args.mvecs)))
    emit("# CONDITION at nsys >= 4096: b/a below 1 by more than the larger of the window spreads and |a - a'| / a; nothing is expected at 256")
    emit(f"{'call':>6} {'nsys':>6} {'vlen':>4} {'mvec':>4} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8}  condition")
    t0 = time.time()
    verdicts = []
    for n, v, m, step in points:
        r = measure_lanes(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, step)
        what = "step" if step else "update"
        if r is None:
            emit(f"{what:>6} {n:6d} {v:4d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        noise = max(ctl, r["spread_a"], r["spread_a2"], r["spread_b"])
        cond = "-"
        if n >= 4096:
            cond = "HELD" if 1.0 - ratio > noise else "MISSED"
            verdicts.append(cond)
        emit(f"{what:>6} {n:6d} {v:4d} {m:4d} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} {ctl:8.3f}  {cond}   "
             f"(spread a {100 * r['spread_a']:.1f} % a' {100 * r['spread_a2']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# condition: {verdicts.count('HELD')} HELD, {verdicts.count('MISSED')} MISSED of {len(verdicts)} points at nsys >= 4096; "
         f"{len(points)} points in {time.time() - t0:.0f} s")
    return 0


def waves_cap(rows, vlens, mvecs):
    """THE CAP RULE on the measured rows {(nsys, vlen, mvec): (a, a2, b)} of accel_update: the largest power of two v such that at
    nsys = 4096 every vlen <= v of the grid, at every mvec, was measured and has a - b > |a - a2|; 128 if there is none."""
    def won(v, m):
        r = rows.get((4096, v, m))
        return r is not None and r[0] - r[2] > abs(r[0] - r[1])
    cap, v = 128, 128
    while v <= max(vlens):
        if all(won(u, m) for u in vlens if u <= v for m in mvecs):
            cap = v
        v *= 2
    return cap


def waves_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    per_group, cap = nka_amd.batch_waves_limits()
    # the points that decide the cap first, the largest batches last
    order = sorted(ints(args.nsys), key=lambda n: (n != 4096, n))
    points = [(n, v, m, False) for n in order for v in ints(args.vlens) for m in ints(args.mvecs)]
    points += [(n, 256, m, True) for n in order for m in ints(args.mvecs) if m != 5]
    emit(f"# one call of (a) a narrow batch at SUMS_BLOCKED_ROUNDED (one workgroup of 256 threads per system; its kernels are the "
         f"parent commit's), (a') a second narrow batch of the same shape -- the control -- and (b) the wave batch "
         f"(nka_hip_batch_create_waves: one wavefront per system, {per_group} systems per workgroup); {torch.cuda.get_device_name(0)}; "
         f"windows >= {args.window} s, median of {args.repeats}, the three alternated on the same inputs; flavour C, full list; the "
         f"time includes the copy of the input into F (equal for the three)")
    emit(f"# NKA_HIP_BATCH_WAVES_MAX_VLEN of the library loaded: {cap}")
    emit("# won: a - b > |a - a'| (THE CAP RULE reads the rows of accel_update at nsys = 4096)")
    emit(f"{'call':>6} {'nsys':>6} {'vlen':>4} {'mvec':>4} {'a us':>10} {'a2 us':>10} {'b us':>10} {'b/a':>6} {'|a-a2|/a':>8}  won")
    t0 = time.time()
    rows, nwon, nlost = {}, 0, 0
    for n, v, m, step in points:
        what = "step" if step else "update"
        if v > cap:
            emit(f"{what:>6} {n:6d} {v:4d} {m:4d}   EXCLUDED: beyond the cap of the library loaded")
            continue
        r = measure_lanes(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, step, waves=True)
        if r is None:
            emit(f"{what:>6} {n:6d} {v:4d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        ratio, ctl = r["b"] / r["a"], abs(r["a"] - r["a2"]) / r["a"]
        won = r["a"] - r["b"] > abs(r["a"] - r["a2"])
        nwon, nlost = nwon + won, nlost + (not won)
        if not step:
            rows[(n, v, m)] = (r["a"], r["a2"], r["b"])
        emit(f"{what:>6} {n:6d} {v:4d} {m:4d} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {ratio:6.3f} {ctl:8.3f}  "
             f"{'yes' if won else 'NO'}   (spread a {100 * r['spread_a']:.1f} % a' {100 * r['spread_a2']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# won at {nwon} of {nwon + nlost} measured points; {len(points)} points in {time.time() - t0:.0f} s")
    emit(f"# THE CAP RULE on the rows at nsys = 4096: NKA_HIP_BATCH_WAVES_MAX_VLEN = {waves_cap(rows, ints(args.vlens), ints(args.mvecs))}")
    return 0


def measure_waves_ext(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    """--waves-ext: the seven variants of the module docstring on the same inputs, alternated.  The ragged lengths are
    ragged_lengths (below); the weights 2^U(-1, 1) per system and element from a fixed seed."""
    import numpy as np
    names = ["a", "a2", "b", "c", "d", "e", "f"]
    npool = mvec + 3
    if 8.0 * nsys * ((vlen + 31) // 32 * 32) * ((mvec + 1) * 2 * len(names) + 3) + 8.0 * nsys * vlen * (npool + len(names)) > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    ragged, full = ragged_lengths(nsys, vlen), np.full(nsys, vlen, np.int32)
    gen = torch.Generator(device="cuda").manual_seed(LENGTHS_SEED)
    w = torch.exp2(2.0 * torch.rand(nsys, vlen, dtype=torch.float64, device="cuda", generator=gen) - 1.0)
    Fs, hs, batches = {}, {}, {}
    for name in names:
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        waves = name in ("b", "c", "d", "f")
        b = batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, flavor=nka_amd.FLAVOR_C, waves=waves, ext=waves and name != "c")
        b.set_sum_order(nka_amd.SUMS_BLOCKED_ROUNDED)
        assert b.kind() == (nka_amd.KIND_WAVES if waves else nka_amd.KIND_NARROW), name
        if name in ("a", "a2", "b"):
            b.set_lengths(ragged)
        if name == "d":
            b.set_lengths(full)
        if name in ("e", "f"):
            b.set_dot_weights(w)
        hs[name] = b._handle()
    del w
    upd = L.nka_hip_batch_accel_update
    count = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[count[0] % npool])
            count[0] += 1
            assert upd(h, p, vlen, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in names}
    for name in names:                             # warm: fill the lists (steady state), settle clocks and caches
        count[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    for name in names:                             # (a system shorter than mvec holds at most that many independent vectors)
        assert (batches[name].num_vec() == np.minimum(mvec, batches[name].lengths())).all(), name
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in names:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec, mean_len=float(ragged.mean()))
    for name in names:
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
        batches[name].delete()
    del pool, Fs
    torch.cuda.empty_cache()
    return out


def waves_ext_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    per_group, cap = nka_amd.batch_waves_limits()
    points = [(n, v, m) for n in ints(args.nsys) for v in ints(args.vlens) for m in ints(args.mvecs)] + [(65536, 256, 10)]
    emit(f"# one update of (a) a narrow batch with ragged lengths (uniform in [vlen/4, vlen], seed {LENGTHS_SEED}; its kernels are the "
         f"parent commit's), (a') the same again -- the control --, (b) an ext wave batch (nka_hip_batch_create_waves_ext) with the same "
         f"lengths, (c) a plain wave batch without lengths (the parent commit's kernels), (d) an ext batch with every length = vlen, "
         f"(e) a narrow batch with one weight row per system, (f) an ext batch with the same weights; {torch.cuda.get_device_name(0)}; "
         f"windows >= {args.window} s, median of {args.repeats}, the seven alternated on the same inputs; flavour C, "
         f"SUMS_BLOCKED_ROUNDED, full lists; the time includes the copy of the input into F (equal for all)")
    emit(f"# NKA_HIP_BATCH_WAVES_MAX_VLEN of the library loaded: {cap}; {per_group} systems per workgroup")
    emit("# b won: a - b > |a - a'|;  f won: e - f > |a - a'|;  d/c: what the length argument costs")
    emit(f"{'nsys':>6} {'vlen':>4} {'mvec':>4} {'mean len':>8} {'a us':>9} {'a2 us':>9} {'b us':>9} {'c us':>9} {'d us':>9} {'e us':>9} {'f us':>9} "
         f"{'b/a':>6} {'|a-a2|/a':>8} {'d/c':>6} {'f/e':>6}  b won  f won")
    t0 = time.time()
    tally = {"b": [0, 0], "f": [0, 0]}
    for n, v, m in points:
        if v > cap:
            emit(f"{n:6d} {v:4d} {m:4d}   EXCLUDED: beyond the cap of the library loaded")
            continue
        r = measure_waves_ext(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            emit(f"{n:6d} {v:4d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        ctl = abs(r["a"] - r["a2"])
        bwon, fwon = r["a"] - r["b"] > ctl, r["e"] - r["f"] > ctl
        tally["b"][not bwon] += 1
        tally["f"][not fwon] += 1
        spreads = " ".join(f"{k} {100 * r['spread_' + k]:.1f} %" for k in ("a", "a2", "b", "c", "d", "e", "f"))
        emit(f"{n:6d} {v:4d} {m:4d} {r['mean_len']:8.0f} " + " ".join(f"{r[k] * 1e6:9.1f}" for k in ("a", "a2", "b", "c", "d", "e", "f")) +
             f" {r['b'] / r['a']:6.3f} {ctl / r['a']:8.3f} {r['d'] / r['c']:6.3f} {r['f'] / r['e']:6.3f}  {'yes' if bwon else 'NO':>5}  "
             f"{'yes' if fwon else 'NO':>5}   (spread {spreads})")
    emit(f"# (b) won at {tally['b'][0]} of {sum(tally['b'])} measured points, (f) at {tally['f'][0]} of {sum(tally['f'])}; "
         f"{len(points)} points in {time.time() - t0:.0f} s")
    return 0


LENGTHS_SEED = 2024


def ragged_lengths(nsys, vlen):
    """The ragged lengths of --lengths: fixed seed, uniform in [vlen / 4, vlen]."""
    import numpy as np
    return np.random.default_rng([LENGTHS_SEED, nsys, vlen]).integers(vlen // 4, vlen + 1, nsys).astype(np.int32)


def measure_lengths(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, wide):
    """--lengths: (a) a plain batch at vlen; (b) the zero-weight recipe, one weight row per system (narrow only); (c) per-system
    lengths -- (b) and (c) once with every length = vlen and once with ragged_lengths.  The same inputs for all, alternated."""
    import numpy as np
    names = ["a", "c_full", "c_ragged"] if wide else ["a", "b_full", "c_full", "b_ragged", "c_ragged"]
    npool = mvec + 3
    need = 8.0 * nsys * vlen * (len(names) * (2 * (mvec + 1) + 1) + npool + 2 * 2)
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    lens = {"full": np.full(nsys, vlen, np.int32), "ragged": ragged_lengths(nsys, vlen)}
    Fs, hs, batches = {}, {}, {}
    for name in names:
        Fs[name] = torch.empty(nsys, vlen, dtype=torch.float64, device="cuda")
        b = batches[name] = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=wide)
        kind, _, which = name.partition("_")
        if kind == "b":
            w = (torch.arange(vlen, device="cuda")[None, :] < torch.from_numpy(lens[which]).cuda()[:, None]).to(torch.float64)
            b.set_dot_weights(w)
            del w
        if kind == "c":
            b.set_lengths(lens[which])
        hs[name] = b._handle()
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd = L.nka_hip_batch_accel_update
    step = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        p = C.c_void_p(F.data_ptr())
        for _ in range(reps):
            F.copy_(pool[step[0] % npool])
            step[0] += 1
            assert upd(h, p, ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {name: [] for name in names}
    for name in names:                             # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        run(name, mvec + 4)
    torch.cuda.synchronize()
    for name in names:
        assert (batches[name].num_vec() == mvec).all(), name
        reps[name] = max(3, int(window / timed(name, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for name in names:
            ts[name].append(timed(name, reps[name]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec, mean_len=float(lens["ragged"].mean()))
    for name in names:
        assert (batches[name].num_vec() == mvec).all(), name
        med = statistics.median(ts[name])
        out[name], out["spread_" + name] = med, (max(ts[name]) - min(ts[name])) / med
        batches[name].delete()
    del pool, Fs
    torch.cuda.empty_cache()
    return out


def lengths_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    narrow = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    wide = [(n, v, m) for n, v in ((16, 65536), (64, 262144)) for m in ints(args.mvecs)] if args.lengths_wide else []
    emit(f"# one update of (a) a plain batch at vlen, (b) the zero-weight recipe (one weight row per system: 1 below the length, 0 "
         f"from there on), (c) per-system lengths (nka_hip_batch_set_lengths); (b) and (c) with every length = vlen (full) and with "
         f"lengths uniform in [vlen/4, vlen], seed {LENGTHS_SEED} (ragged); {torch.cuda.get_device_name(0)}; windows >= {args.window} s, "
         f"median of {args.repeats}, the variants alternated; default flavour and sums, full list")
    emit("# conditions: c_full / a <= 1 + spread (the same work plus one scalar load); c_ragged / b_ragged <= 1 + spread (fewer "
         "streams over fewer elements); spread = the larger of the two variants' (max - min) / median over the windows")
    t0, missed = time.time(), []
    for kind, points in (("narrow", narrow), ("wide", wide)):
        if not points:
            continue
        emit(f"# {kind}")
        emit(f"{'nsys':>5} {'vlen':>7} {'mvec':>4} {'mean len':>9} {'a us':>9} {'b full':>9} {'c full':>9} {'b ragged':>9} {'c ragged':>9} "
             f"{'c_full/a':>8} {'c_rag/b_rag':>11} {'c_rag/a':>8}")
        for n, v, m in points:
            r = measure_lengths(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, kind == "wide")
            if r is None:
                emit(f"{n:5d} {v:7d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
                continue
            us = lambda k: f"{r[k] * 1e6:9.1f}" if k in r else f"{'-':>9}"              # noqa: E731
            full = r["c_full"] / r["a"]
            rag = r["c_ragged"] / r["b_ragged"] if "b_ragged" in r else float("nan")
            verdict = []
            if full > 1.0 + max(r["spread_c_full"], r["spread_a"]):
                verdict.append("c_full/a MISSED")
            if "b_ragged" in r and rag > 1.0 + max(r["spread_c_ragged"], r["spread_b_ragged"]):
                verdict.append("c_rag/b_rag MISSED")
            if verdict:
                missed.append((kind, n, v, m) + tuple(verdict))
            spreads = " ".join(f"{k} {100 * r['spread_' + k]:.1f} %" for k in ("a", "b_full", "c_full", "b_ragged", "c_ragged") if k in r)
            emit(f"{n:5d} {v:7d} {m:4d} {r['mean_len']:9.0f} {us('a')} {us('b_full')} {us('c_full')} {us('b_ragged')} {us('c_ragged')} "
                 f"{full:8.3f} {rag:11.3f} {r['c_ragged'] / r['a']:8.3f}   {'; '.join(verdict) if verdict else 'ok'}   (spread {spreads})")
    emit(f"# {len(narrow) + len(wide)} points in {time.time() - t0:.0f} s; missed a condition: {missed if missed else 'nowhere'}")
    return 0


def measure_step(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    npool = mvec + 3
    need = 8.0 * nsys * vlen * (3 * 2 * (mvec + 1) + npool + 3 + 2)       # three batches' slots, the pool, three f, two x
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    names = ("a", "b", "c")
    Fs = {v: torch.empty(nsys, vlen, dtype=torch.float64, device="cuda") for v in names}
    Xs = {v: torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for v in ("b", "c")}
    masks = {v: torch.ones(nsys, dtype=torch.int32, device="cuda") for v in ("b", "c")}
    tol = torch.zeros(nsys, dtype=torch.float64, device="cuda")
    rb, rc = (torch.zeros(nsys, dtype=torch.float64, device="cuda") for _ in range(2))
    batches = {v: nka_amd.nka_batch().init(nsys, vlen, mvec) for v in names}
    hs = {v: batches[v]._handle() for v in names}
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    P = lambda t: C.c_void_p(t.data_ptr())                                           # noqa: E731
    upd, stp = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step
    step = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        for _ in range(reps):
            F.copy_(pool[step[0] % npool])
            step[0] += 1
            if name == "a":
                assert upd(h, P(F), ld, None) == 0
            elif name == "b":
                torch.linalg.vector_norm(F, dim=1, out=rb)
                torch.gt(rb, tol, out=masks["b"])
                assert upd(h, P(F), ld, P(masks["b"])) == 0
                torch.addcmul(Xs["b"], F, masks["b"][:, None], value=-1.0, out=Xs["b"])
            else:
                assert stp(h, P(F), ld, P(Xs["c"]), ld, P(masks["c"]), P(tol), P(rc)) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {v: [] for v in names}
    for v in names:                                # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        run(v, mvec + 4)
    torch.cuda.synchronize()
    assert torch.equal(Fs["b"], Fs["c"]) and torch.equal(Xs["b"], Xs["c"]) and torch.equal(Fs["a"], Fs["c"])      # the same work
    for v in names:
        assert (batches[v].num_vec() == mvec).all(), v
        reps[v] = max(3, int(window / timed(v, 3)) + 1)
    for _ in range(repeats):                       # alternate the variants
        for v in names:
            ts[v].append(timed(v, reps[v]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    assert masks["b"].all() and masks["c"].all()   # nothing retired
    for v in names:
        assert (batches[v].num_vec() == mvec).all(), v
        med = statistics.median(ts[v])
        out[v], out["spread_" + v] = med, (max(ts[v]) - min(ts[v])) / med
        batches[v].delete()
    del pool, Fs, Xs
    torch.cuda.empty_cache()
    return out


def measure_wide_step(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    """measure_step on wide batches, with the composed loop twice: (b') is the control that says what two runs of the SAME loop
    differ by.  (a), (b) and (b') run plain wide batches -- the update instances of nka_batch_wide.hip --, (c) the batch with the step."""
    npool = mvec + 3
    need = 8.0 * nsys * vlen * (4 * 2 * (mvec + 1) + npool + 4 + 3)       # four batches' slots, the pool, four f, three x
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    names = ("a", "b", "b2", "c")
    Fs = {v: torch.empty(nsys, vlen, dtype=torch.float64, device="cuda") for v in names}
    Xs = {v: torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for v in ("b", "b2", "c")}
    masks = {v: torch.ones(nsys, dtype=torch.int32, device="cuda") for v in ("b", "b2", "c")}
    tol = torch.zeros(nsys, dtype=torch.float64, device="cuda")
    rs = {v: torch.zeros(nsys, dtype=torch.float64, device="cuda") for v in ("b", "b2", "c")}
    batches = {v: nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True, step=(v == "c")) for v in names}
    assert batches["c"].offers_step() and not batches["a"].offers_step()
    hs = {v: batches[v]._handle() for v in names}
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    P = lambda t: C.c_void_p(t.data_ptr())                                           # noqa: E731
    upd, stp = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step
    step = [0]

    def run(name, reps):
        F, h = Fs[name], hs[name]
        for _ in range(reps):
            F.copy_(pool[step[0] % npool])
            step[0] += 1
            if name == "a":
                assert upd(h, P(F), ld, None) == 0
            elif name == "c":
                assert stp(h, P(F), ld, P(Xs["c"]), ld, P(masks["c"]), P(tol), P(rs["c"])) == 0
            else:
                torch.linalg.vector_norm(F, dim=1, out=rs[name])
                torch.gt(rs[name], tol, out=masks[name])
                assert upd(h, P(F), ld, P(masks[name])) == 0
                torch.addcmul(Xs[name], F, masks[name][:, None], value=-1.0, out=Xs[name])

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {v: [] for v in names}
    for v in names:                                # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        run(v, mvec + 4)
    torch.cuda.synchronize()
    for v in ("a", "b", "b2"):                     # the same work
        assert torch.equal(Fs[v], Fs["c"]), v
    assert torch.equal(Xs["b"], Xs["c"]) and torch.equal(Xs["b2"], Xs["c"])
    for v in names:
        assert (batches[v].num_vec() == mvec).all(), v
        reps[v] = max(3, int(window / timed(v, 3)) + 1)
    for _ in range(repeats):                       # alternate the variants
        for v in names:
            ts[v].append(timed(v, reps[v]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    assert all(m.all() for m in masks.values())    # nothing retired
    for v in names:
        assert (batches[v].num_vec() == mvec).all(), v
        med = statistics.median(ts[v])
        out[v], out["spread_" + v] = med, (max(ts[v]) - min(ts[v])) / med
        batches[v].delete()
    del pool, Fs, Xs
    torch.cuda.empty_cache()
    return out


def wide_step_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    emit(f"# one iteration on WIDE batches: (a) accel_update; (b) vector_norm + mask update + accel_update(mask) + masked X -= F; (b') "
         f"the same loop a second time, the control; (c) accel_step of a batch of nka_hip_batch_create_wide_step with X, mask, tol, "
         f"fnorm; {torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of {args.repeats}, the four alternated on the "
         f"same inputs; default flavour and sums, full list; tol = 0: no system retires; the time includes the copy of the input "
         f"into F (equal for the four)")
    emit("# (a), (b) and (b') run the update instances of nka_batch_wide.hip; a point is WON when b - c > |b - b'|, LOST when c - b > |b - b'|")
    emit(f"{'nsys':>5} {'vlen':>7} {'mvec':>4} {'(a) us':>10} {'(b) us':>10} {'(b2) us':>10} {'(c) us':>10} {'c/b':>7} {'c/a':>7} "
         f"{'|b-b2|/b':>8}  c vs b")
    t0 = time.time()
    tally = {"won": [], "lost": [], "level": []}
    for n, v, m in points:
        r = measure_wide_step(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            emit(f"{n:5d} {v:7d} {m:4d}   SKIPPED: the four batches and the inputs need more than {args.mem_gb:g} GB of device memory")
            continue
        noise = abs(r["b"] - r["b2"])
        verdict = "won" if r["b"] - r["c"] > noise else "lost" if r["c"] - r["b"] > noise else "level"
        tally[verdict].append((n, v, m, round(r["c"] / r["b"], 3)))
        emit(f"{n:5d} {v:7d} {m:4d} {r['a'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {r['b2'] * 1e6:10.1f} {r['c'] * 1e6:10.1f} "
             f"{r['c'] / r['b']:7.3f} {r['c'] / r['a']:7.3f} {noise / r['b']:8.4f}  {verdict.upper():5}   "
             f"(spread a {100 * r['spread_a']:.1f} % b {100 * r['spread_b']:.1f} % b2 {100 * r['spread_b2']:.1f} % c {100 * r['spread_c']:.1f} %)")
    emit(f"# {len(points)} points in {time.time() - t0:.0f} s; won {len(tally['won'])}, level {len(tally['level'])}, lost {len(tally['lost'])}"
         f"{': ' + str(tally['lost']) if tally['lost'] else ''}")
    return 0


def wide_weights_streams(mvec, weighted):
    """Streams of vlen doubles an update of a wide batch reads or writes per element, full list, compact storage: the norm launch 2
    (3 with weights), G = ceil(L / 4) sweeps of 6 (7 with weights) over L = mvec - 1 older vectors, the combine 7 + k, k = mvec."""
    g = -(-(mvec - 1) // 4)
    return (3 + 7 * g if weighted else 2 + 6 * g) + 7 + mvec


def measure_wide_weights(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget, step):
    """Six variants on the same inputs, alternated: (a) a plain wide batch, (a2) the same again, the control, (b) an ext batch with
    the shared row, (c) an ext batch with one row per system, (d) an ext batch with nothing set, (e) a loop over lone handles with
    nka_hip_set_dot_weights (update only).  step: accel_step with X, the mask, tol = 0 and fnorm on batches that offer it."""
    npool = mvec + 3
    names = ("a", "a2", "b", "c", "d") + (() if step else ("e",))
    need = 8.0 * nsys * vlen * (len(names) * 2 * (mvec + 1) + npool + len(names) * (2 if step else 1) + 3)
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    w = torch.exp2(6.0 * torch.rand(nsys, vlen, dtype=torch.float64, device="cuda") - 3.0)
    Fs = {v: torch.empty(nsys, vlen, dtype=torch.float64, device="cuda") for v in names}
    Xs = {v: torch.zeros(nsys, vlen, dtype=torch.float64, device="cuda") for v in names} if step else {}
    masks = {v: torch.ones(nsys, dtype=torch.int32, device="cuda") for v in names}
    tol = torch.zeros(nsys, dtype=torch.float64, device="cuda")
    rs = {v: torch.zeros(nsys, dtype=torch.float64, device="cuda") for v in names}
    batches = {v: nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True, step=step, ext=v in ("b", "c", "d")) for v in names if v != "e"}
    batches["b"].set_dot_weights(w[0])
    batches["c"].set_dot_weights(w)
    assert [batches[v].dot_weighted() for v in ("a", "a2", "b", "c", "d")] == [False, False, True, True, False]
    assert batches["d"].offers_weights() and not batches["a"].offers_weights()
    lones = []
    if not step:
        lones = [nka_amd.nka().init(vlen, mvec).set_dot_weights(w[k]) for k in range(nsys)]
        hl = [x._handle() for x in lones]
        pl = [C.c_void_p(Fs["e"][k].data_ptr()) for k in range(nsys)]
    hs = {v: b._handle() for v, b in batches.items()}
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    P = lambda t: C.c_void_p(t.data_ptr())                                           # noqa: E731
    upd, stp, upd_lone = L.nka_hip_batch_accel_update, L.nka_hip_batch_accel_step, L.nka_hip_accel_update
    count = [0]

    def run(name, reps):
        F = Fs[name]
        for _ in range(reps):
            F.copy_(pool[count[0] % npool])
            count[0] += 1
            if name == "e":
                for k in range(nsys):
                    if upd_lone(hl[k], pl[k]) != 0:
                        raise RuntimeError(L.nka_hip_last_error())
            elif step:
                assert stp(hs[name], P(F), ld, P(Xs[name]), ld, P(masks[name]), P(tol), P(rs[name])) == 0
            else:
                assert upd(hs[name], P(F), ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    reps, ts = {}, {v: [] for v in names}
    for v in names:                                # warm: fill the lists (steady state), settle clocks and caches
        count[0] = 0
        run(v, mvec + 4)
    torch.cuda.synchronize()
    for v in ("a2", "d"):                          # the same kernels on the same inputs: the same bits
        assert torch.equal(Fs[v], Fs["a"]), v
    for v in names:
        if v != "e":
            assert (batches[v].num_vec() == mvec).all(), v
        reps[v] = max(3, int(window / timed(v, 3)) + 1)
    for _ in range(repeats):                       # alternate the variants
        for v in names:
            ts[v].append(timed(v, reps[v]))
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    assert all(m.all() for m in masks.values())    # nothing retired
    for v in names:
        med = statistics.median(ts[v])
        out[v], out["spread_" + v] = med, (max(ts[v]) - min(ts[v])) / med
    for b in list(batches.values()) + lones:
        b.delete()
    del pool, w, Fs, Xs
    torch.cuda.empty_cache()
    return out


def wide_weights_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m, False) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    points += [(64, 65536, m, True) for m in ints(args.mvecs)]                       # the step variants at one point
    chunk, cap = nka_amd.batch_wide_limits()
    emit(f"# diagonal dot weights on WIDE batches (nka_hip_batch_create_wide_ext; chunk {chunk}, cap {cap}): (a) a plain wide batch; (a2) "
         f"the same again, the control; (b) an ext batch, one shared weight row; (c) an ext batch, one weight row per system; (d) an ext "
         f"batch with nothing set; (e) a loop over lone handles with nka_hip_set_dot_weights on one stream; {torch.cuda.get_device_name(0)}; "
         f"windows >= {args.window} s, median of {args.repeats}, the variants alternated on the same inputs; default flavour, full "
         f"list; weights 2^U(-3, 3); the time includes the copy of the input into F (equal for all)")
    emit("# streams per element: norm 2 -> 3, each sweep of four 6 -> 7, combine 7 + k unchanged; (d) launches the kernels of (a); "
         "(c) against (e): WON when e - c > |a - a2|, LOST when c - e > |a - a2|; `step`: accel_step with X, mask, tol = 0 and fnorm, no (e)")
    emit(f"{'nsys':>5} {'vlen':>7} {'mvec':>4} {'call':>6} {'(a) us':>10} {'(a2) us':>10} {'(b) us':>10} {'(c) us':>10} {'(d) us':>10} {'(e) us':>11} "
         f"{'b/a':>6} {'c/a':>6} {'model':>6} {'d/a':>6} {'|a-a2|/a':>8} {'e/c':>7}  c vs e")
    t0 = time.time()
    tally = {"won": [], "lost": [], "level": []}
    for n, v, m, step in points:
        r = measure_wide_weights(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9, step)
        call = "step" if step else "update"
        if r is None:
            emit(f"{n:5d} {v:7d} {m:4d} {call:>6}   SKIPPED: the batches, the lone handles and the inputs need more than {args.mem_gb:g} GB of "
                 f"device memory")
            continue
        noise = abs(r["a"] - r["a2"])
        model = wide_weights_streams(m, True) / wide_weights_streams(m, False)
        if step:
            e_us, e_c, verdict = f"{'-':>11}", f"{'-':>7}", "-"
        else:
            verdict = "won" if r["e"] - r["c"] > noise else "lost" if r["c"] - r["e"] > noise else "level"
            tally[verdict].append((n, v, m, round(r["e"] / r["c"], 2)))
            e_us, e_c = f"{r['e'] * 1e6:11.1f}", f"{r['e'] / r['c']:7.2f}"
        emit(f"{n:5d} {v:7d} {m:4d} {call:>6} {r['a'] * 1e6:10.1f} {r['a2'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {r['c'] * 1e6:10.1f} "
             f"{r['d'] * 1e6:10.1f} {e_us} {r['b'] / r['a']:6.3f} {r['c'] / r['a']:6.3f} {model:6.3f} {r['d'] / r['a']:6.3f} "
             f"{noise / r['a']:8.4f} {e_c}  {verdict.upper():5}   (spread " +
             " ".join(f"{k} {100 * r['spread_' + k]:.1f} %" for k in ("a", "a2", "b", "c", "d") + (() if step else ("e",))) + ")")
    emit(f"# {len(points)} points in {time.time() - t0:.0f} s; (c) against (e): won {len(tally['won'])}, level {len(tally['level'])}, "
         f"lost {len(tally['lost'])}{': ' + str(tally['lost']) if tally['lost'] else ''}")
    return 0


def measure_wide(torch, nka_amd, L, nsys, vlen, mvec, window, repeats, mem_budget):
    npool = mvec + 3
    narrow = vlen <= nka_amd.BATCH_MAX_VLEN
    names = ("a", "b", "c") if narrow else ("a", "b")
    need = 8.0 * nsys * vlen * (len(names) * 2 * (mvec + 1) + npool + len(names))      # the contenders' slots, the pool, their f
    if need > mem_budget:
        return None
    pool = torch.randn(npool, nsys, vlen, dtype=torch.float64, device="cuda")
    Fs = {v: torch.empty(nsys, vlen, dtype=torch.float64, device="cuda") for v in names}
    wide = nka_amd.nka_batch().init(nsys, vlen, mvec, wide=True)
    batches = {"a": wide}
    if narrow:
        batches["c"] = nka_amd.nka_batch().init(nsys, vlen, mvec)
    lones = [nka_amd.nka().init(vlen, mvec) for _ in range(nsys)]
    hl = [a._handle() for a in lones]
    pl = [C.c_void_p(Fs["b"][k].data_ptr()) for k in range(nsys)]
    ld = int(Fs["a"].stride(0)) if nsys > 1 else vlen
    upd_batch, upd_lone = L.nka_hip_batch_accel_update, L.nka_hip_accel_update
    step = [0]

    def run(name, reps):
        F = Fs[name]
        for _ in range(reps):
            F.copy_(pool[step[0] % npool])
            step[0] += 1
            if name == "b":
                for k in range(nsys):
                    if upd_lone(hl[k], pl[k]) != 0:
                        raise RuntimeError(L.nka_hip_last_error())
            else:
                assert upd_batch(batches[name]._handle(), C.c_void_p(F.data_ptr()), ld, None) == 0

    def timed(name, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(name, reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    def full():
        return all((b.num_vec() == mvec).all() for b in batches.values()) and lones[0].num_vec() == mvec and lones[-1].num_vec() == mvec

    reps, ts = {}, {v: [] for v in names}
    for v in names:                                # warm: fill the lists (steady state), settle clocks and caches
        step[0] = 0
        run(v, mvec + 4)
    torch.cuda.synchronize()
    assert full()
    assert torch.allclose(Fs["a"], Fs["b"], rtol=0, atol=1e-9 * float(Fs["b"].abs().max()))      # the same work
    for v in names:
        reps[v] = max(3, int(window / timed(v, 3)) + 1)
    for _ in range(repeats):                       # alternate the contenders
        for v in names:
            ts[v].append(timed(v, reps[v]))
    assert full()
    out = dict(nsys=nsys, vlen=vlen, mvec=mvec)
    for v in names:
        med = statistics.median(ts[v])
        out[v], out["spread_" + v] = med, (max(ts[v]) - min(ts[v])) / med
    out["share"] = 8.0 * nsys * vlen * (11 + (mvec - 1) + mvec) / out["a"] / PEAK
    for x in lones:
        x.delete()
    for b in batches.values():
        b.delete()
    del pool, Fs
    torch.cuda.empty_cache()
    return out


WIDE_BARRED_VLENS = (32768, 65536)


def wide_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    chunk, cap = nka_amd.batch_wide_limits()
    emit(f"# wide batch (a) against nsys lone handles in a loop on one stream (b) and the narrow batch (c, vlen <= "
         f"{nka_amd.BATCH_MAX_VLEN}); {torch.cuda.get_device_name(0)}; chunk = {chunk}, cap = {cap} ({nka_amd.lib_path()}); windows >= "
         f"{args.window} s, median of {args.repeats}, contenders alternated; default flavour and sums, full list")
    emit(f"# share = 8*nsys*vlen*(11 + L + k) / time(a) / 8 TB/s; bar at nsys >= 16 and vlen in {WIDE_BARRED_VLENS}: b/a >= {BAR}; "
         f"every other point is recorded without a bar")
    emit(f"{'nsys':>5} {'vlen':>8} {'mvec':>4} {'(a) wide us':>12} {'(b) loop us':>12} {'(c) narrow us':>13} {'share':>6} {'b/a':>7} "
         f"{'c/a':>7}  bar")
    t0 = time.time()
    missed, skipped = [], []
    for n, v, m in points:
        if v > cap:
            emit(f"{n:5d} {v:8d} {m:4d}   beyond the cap of this library")
            continue
        slots = 8.0 * n * v * 2 * (m + 1)
        r = None if slots > args.slots_gb * 1e9 else measure_wide(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            skipped.append((n, v, m))
            emit(f"{n:5d} {v:8d} {m:4d}   SKIPPED: one contender's stored vectors take {slots / 1e9:.0f} GB (limit {args.slots_gb:g} GB), or "
                 f"all contenders together more than {args.mem_gb:g} GB")
            continue
        barred = n >= 16 and v in WIDE_BARRED_VLENS
        ratio = r["b"] / r["a"]
        bar = "-" if not barred else ("ok" if ratio >= BAR else "MISSED")
        if bar == "MISSED":
            missed.append((n, v, m, round(ratio, 3)))
        c_us = f"{r['c'] * 1e6:13.1f}" if "c" in r else f"{'-':>13}"
        c_ratio = f"{r['c'] / r['a']:7.2f}" if "c" in r else f"{'-':>7}"
        spreads = " ".join(f"{k} {100 * r['spread_' + k]:.1f} %" for k in ("a", "b", "c") if k in r)
        emit(f"{n:5d} {v:8d} {m:4d} {r['a'] * 1e6:12.1f} {r['b'] * 1e6:12.1f} {c_us} {r['share']:6.3f} {ratio:7.2f} {c_ratio}  {bar}   "
             f"(spread {spreads})")
    emit(f"# {len(points)} points in {time.time() - t0:.0f} s; skipped: {skipped if skipped else 'none'}; missed the bar: "
         f"{missed if missed else 'none'}")
    return 0


def step_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    emit(f"# one iteration: (a) accel_update; (b) vector_norm + mask update + accel_update(mask) + masked X -= F; (c) accel_step "
         f"with X, mask, tol, fnorm; {torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of {args.repeats}, the "
         f"three alternated; default flavour and sums, full list; tol = 0: no system retires")
    emit("# streams per element and update: 2 + 6 G + (7 + k) for (a), 2 + 6 G + (9 + k) for (c), G = ceil((mvec - 1) / 4), k = mvec")
    emit("# condition: (c) not slower than (b) by more than the spread of the windows (the larger of the two spreads)")
    emit(f"{'nsys':>5} {'vlen':>6} {'mvec':>4} {'(a) us':>10} {'(b) us':>10} {'(c) us':>10} {'c/b':>7} {'c/a':>7} {'streams c/a':>11}  c vs b")
    t0 = time.time()
    missed = []
    for n, v, m in points:
        r = measure_step(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            emit(f"{n:5d} {v:6d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        g = (m - 1 + 3) // 4
        pred = (2 + 6 * g + 9 + m) / (2 + 6 * g + 7 + m)
        ok = r["c"] <= r["b"] * (1.0 + max(r["spread_b"], r["spread_c"]))
        if not ok:
            missed.append((n, v, m, round(r["c"] / r["b"], 3)))
        emit(f"{n:5d} {v:6d} {m:4d} {r['a'] * 1e6:10.1f} {r['b'] * 1e6:10.1f} {r['c'] * 1e6:10.1f} {r['c'] / r['b']:7.3f} "
             f"{r['c'] / r['a']:7.3f} {pred:11.3f}  {'ok' if ok else 'MISSED'}   "
             f"(spread a {100 * r['spread_a']:.1f} % b {100 * r['spread_b']:.1f} % c {100 * r['spread_c']:.1f} %)")
    emit(f"# {len(points)} points in {time.time() - t0:.0f} s; (c) slower than (b) beyond the spread: {missed if missed else 'nowhere'}")
    return 0


def weights_main(args, torch, nka_amd, L, emit):
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    points = [(n, v, m) for v in ints(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    emit(f"# one update of a batch with plain sums, with diagonal weights all systems share (ldw = 0) and with one row of "
         f"weights per system; {torch.cuda.get_device_name(0)}; windows >= {args.window} s, median of {args.repeats}, the three "
         f"alternated; default flavour and sums, full list; weights 2^U(-3,3)")
    emit("# streams per element and update: 2 + 6 G + (7 + k) plain, 3 + 7 G + (7 + k) weighted, G = ceil((mvec - 1) / 4), k = mvec")
    emit(f"{'nsys':>5} {'vlen':>6} {'mvec':>4} {'plain us':>10} {'shared us':>10} {'rows us':>10} {'shared/plain':>12} "
         f"{'rows/plain':>10} {'streams w/p':>11}")
    t0 = time.time()
    for n, v, m in points:
        r = measure_weights(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            emit(f"{n:5d} {v:6d} {m:4d}   EXCLUDED: needs more than {args.mem_gb:g} GB of device memory")
            continue
        g = (m - 1 + 3) // 4
        pred = (3 + 7 * g + 7 + m) / (2 + 6 * g + 7 + m)
        emit(f"{n:5d} {v:6d} {m:4d} {r['plain'] * 1e6:10.1f} {r['shared'] * 1e6:10.1f} {r['rows'] * 1e6:10.1f} "
             f"{r['shared'] / r['plain']:12.3f} {r['rows'] / r['plain']:10.3f} {pred:11.3f}   "
             f"(spread plain {100 * r['spread_plain']:.1f} % shared {100 * r['spread_shared']:.1f} % rows {100 * r['spread_rows']:.1f} %)")
    emit(f"# {len(points)} points in {time.time() - t0:.0f} s")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nsys", default="1,16,256,1024,4096")
    ap.add_argument("--vlens", default="64,1024,16384,cap")
    ap.add_argument("--mvecs", default="5,10,20")
    ap.add_argument("--probe-vlens", default="", help="extra lengths, measured at --probe-nsys only")
    ap.add_argument("--probe-nsys", default="16")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mem-gb", type=float, default=200.0, help="skip (and say so) a point that needs more device memory")
    ap.add_argument("--out", default=None)
    ap.add_argument("--weights", action="store_true",
                    help="time a weighted batch (shared and per-system weights) beside the plain one; without --nsys / --vlens / "
                         "--mvecs: nsys 256,4096 x vlen 1024,16384 x mvec 10,20")
    ap.add_argument("--step", action="store_true",
                    help="time accel_step against accel_update and against the loop a caller composes from it; without --nsys / "
                         "--vlens / --mvecs: nsys 256,4096 x vlen 64,1024,16384 x mvec 10,20")
    ap.add_argument("--wide", action="store_true",
                    help="time the wide batch against the loop over lone handles and the narrow batch; without --nsys / --vlens / "
                         "--mvecs: nsys 4,16,64,256 x vlen 4096,16384,32768,65536,262144,1048576 x mvec 10,20")
    ap.add_argument("--slots-gb", type=float, default=64.0, help="--wide: skip a point whose stored vectors exceed this")
    ap.add_argument("--lengths", action="store_true",
                    help="time per-system lengths beside a plain batch and the zero-weight recipe; without --nsys / --vlens / --mvecs: "
                         "nsys 256,4096 x vlen 1024,16384 x mvec 10,20, then the wide batch at (16, 65536) and (64, 262144)")
    ap.add_argument("--store32", action="store_true",
                    help="time a batch with binary32 storage beside two binary64 batches (the second: a control); without --nsys / "
                         "--vlens / --mvecs: nsys 256,4096 x vlen 1024,16384 x mvec 10,20, plus 4096 x 64 x 10")
    ap.add_argument("--lanes", action="store_true",
                    help="time the lane batch (one lane per system) beside two narrow batches (the second: a control); without "
                         "--nsys / --vlens / --mvecs: nsys 256,4096,65536 x vlen 8,32,64 x mvec 5,10,20, then accel_step at vlen 32")
    ap.add_argument("--waves", action="store_true",
                    help="time the wave batch (one wavefront per system) beside two narrow batches at the rounded fast sums (the second: "
                         "a control); without --nsys / --vlens / --mvecs / --mem-gb: nsys 256,4096,65536 x vlen 65,128,256,512,1024,2048,"
                         "4096 x mvec 5,10,20, 40 GB, then accel_step at vlen 256 x mvec 10,20; prints the cap its rule yields")
    ap.add_argument("--waves-ext", action="store_true",
                    help="time the wave batch with lengths and weights (nka_hip_batch_create_waves_ext) beside narrow batches with the "
                         "same lengths and weights and beside the plain wave batch; without --nsys / --vlens / --mvecs / --mem-gb: nsys "
                         "4096 x vlen 128,256,1024 x mvec 10,20, then 65536 x 256 x 10, 40 GB")
    ap.add_argument("--wide-step", action="store_true",
                    help="time accel_step of a wide batch (nka_hip_batch_create_wide_step) against the wide accel_update and against "
                         "the loop a caller composes from it, run twice (the second: a control); without --nsys / --vlens / --mvecs / "
                         "--mem-gb: nsys 16,64,256 x vlen 32768,65536,262144 x mvec 10,20, 40 GB")
    ap.add_argument("--wide-weights", action="store_true",
                    help="time diagonal dot weights on wide batches (nka_hip_batch_create_wide_ext): a plain wide batch twice, ext "
                         "batches with a shared row, with one row per system and with nothing set, and a loop over lone handles with "
                         "weights; without --nsys / --vlens / --mvecs / --mem-gb: nsys 16,64,256 x vlen 32768,262144 x mvec 10,20, "
                         "then accel_step at 64 x 65536, 40 GB")
    ap.add_argument("--wide-store32", action="store_true",
                    help="time binary32 storage of a wide batch (nka_hip_batch_create_wide_stored) against a binary64 wide batch and a "
                         "second one as a control; without --nsys / --vlens / --mvecs / --mem-gb: nsys 16,64,256 x vlen "
                         "32768,65536,262144 x mvec 10,20, then accel_step at 64 x 65536 x 20, 40 GB")
    ap.add_argument("--wide-rows", action="store_true",
                    help="time the scalar step of a wide batch on one wavefront (nka_hip_batch_set_scalar_step) against the one-thread "
                         "step and a second one-thread batch as a control, at nsys = 4 also against four lone handles; without --nsys / "
                         "--vlens / --mvecs / --mem-gb: nsys 4,16,64,256 x vlen 32768,65536,262144 x mvec 5,10,20,32, then accel_step at "
                         "16 x 65536 x 20, 40 GB")
    ap.add_argument("--waves-rows", action="store_true",
                    help="time the scalar step of a wave batch on the whole wavefront (nka_hip_batch_create_waves_rows, "
                         "nka_hip_batch_set_scalar_step) against the one-lane wave batch and a second one as a control, at nsys = 256 also "
                         "against the narrow batch; without --nsys / --vlens / --mvecs / --mem-gb: nsys 256,4096,65536 x vlen 65,256,1024 x "
                         "mvec 5,10,20,cap, then accel_step at 4096 x 256 x 10,20, 40 GB")
    ap.add_argument("--rows", action="store_true",
                    help="time the scalar step of a narrow batch on one wavefront (nka_hip_batch_create_rows, nka_hip_batch_set_scalar_step) "
                         "against the one-thread step and a second one-thread batch as a control, at vlen <= 1024 also against the wave "
                         "batch of nka_hip_batch_create_waves_rows; without --nsys / --vlens / --mvecs / --mem-gb: nsys 16,256,4096 x vlen "
                         "256,1024,4096,16384 x mvec 5,10,20,32, 40 GB")
    ap.add_argument("--no-waves-rows-steps", dest="waves_rows_steps", action="store_false", help="--waves-rows: leave the two steps out")
    ap.add_argument("--no-store32-extra", dest="store32_extra", action="store_false", help="--store32: leave 4096 x 64 x 10 out")
    ap.add_argument("--no-lengths-wide", dest="lengths_wide", action="store_false", help="--lengths: leave the wide points out")
    args = ap.parse_args()
    import torch
    import nka_amd
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    L = nka_amd.load()
    if args.waves_rows:      # (ahead of the grid below: the last mvec of this mode is the library's cap)
        for name, grid_w in (("nsys", "256,4096,65536"), ("vlens", "65,256,1024"), ("mvecs", f"5,10,20,{nka_amd.batch_waves_rows_limits()[0]}"),
                             ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
    if args.rows:
        for name, grid_w in (("nsys", "16,256,4096"), ("vlens", "256,1024,4096,16384"), ("mvecs", "5,10,20,32"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
    cap = nka_amd.BATCH_MAX_VLEN
    vl = lambda s: list(dict.fromkeys(cap if v == "cap" else int(v) for v in s.split(",") if v))      # noqa: E731  (cap may be in the list already)
    ints = lambda s: [int(v) for v in s.split(",") if v]                             # noqa: E731
    grid = [(n, v, m) for v in vl(args.vlens) for m in ints(args.mvecs) for n in ints(args.nsys)]
    # the probes first: they decide the cap
    points = [(n, v, m) for v in vl(args.probe_vlens) for m in ints(args.mvecs) for n in ints(args.probe_nsys) if (n, v, m) not in grid]
    points += grid
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if args.waves_rows:
        return waves_rows_main(args, torch, nka_amd, L, emit)
    if args.rows:
        return rows_main(args, torch, nka_amd, L, emit)
    if args.wide_rows:
        for name, grid_w in (("nsys", "4,16,64,256"), ("vlens", "32768,65536,262144"), ("mvecs", "5,10,20,32"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return wide_rows_main(args, torch, nka_amd, L, emit)
    if args.wide_store32:
        for name, grid_w in (("nsys", "16,64,256"), ("vlens", "32768,65536,262144"), ("mvecs", "10,20"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return wide_store32_main(args, torch, nka_amd, L, emit)
    if args.wide_weights:
        for name, grid_w in (("nsys", "16,64,256"), ("vlens", "32768,262144"), ("mvecs", "10,20"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return wide_weights_main(args, torch, nka_amd, L, emit)
    if args.wide_step:
        for name, grid_w in (("nsys", "16,64,256"), ("vlens", "32768,65536,262144"), ("mvecs", "10,20"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return wide_step_main(args, torch, nka_amd, L, emit)
    if args.waves_ext:
        for name, grid_w in (("nsys", "4096"), ("vlens", "128,256,1024"), ("mvecs", "10,20"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return waves_ext_main(args, torch, nka_amd, L, emit)
    if args.waves:
        for name, grid_w in (("nsys", "256,4096,65536"), ("vlens", "65,128,256,512,1024,2048,4096"), ("mvecs", "5,10,20"), ("mem_gb", 40.0)):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return waves_main(args, torch, nka_amd, L, emit)
    if args.lanes:
        for name, grid_l in (("nsys", "256,4096,65536"), ("vlens", "8,32,64"), ("mvecs", "5,10,20")):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_l)
        return lanes_main(args, torch, nka_amd, L, emit)
    if args.store32:
        for name, grid_s in (("nsys", "256,4096"), ("vlens", "1024,16384"), ("mvecs", "10,20")):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_s)
        return store32_main(args, torch, nka_amd, L, emit)
    if args.lengths:
        for name, grid_l in (("nsys", "256,4096"), ("vlens", "1024,16384"), ("mvecs", "10,20")):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_l)
        return lengths_main(args, torch, nka_amd, L, emit)
    if args.wide:
        for name, grid_w in (("nsys", "4,16,64,256"), ("vlens", "4096,16384,32768,65536,262144,1048576"), ("mvecs", "10,20")):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return wide_main(args, torch, nka_amd, L, emit)
    if args.step:
        for name, grid_s in (("nsys", "256,4096"), ("vlens", "64,1024,16384"), ("mvecs", "10,20")):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_s)
        return step_main(args, torch, nka_amd, L, emit)
    if args.weights:
        for name, grid_w in (("nsys", "256,4096"), ("vlens", "1024,16384"), ("mvecs", "10,20")):
            if getattr(args, name) == ap.get_default(name):
                setattr(args, name, grid_w)
        return weights_main(args, torch, nka_amd, L, emit)
    emit(f"# batched update (a) against nsys lone handles in a loop on one stream (b); {torch.cuda.get_device_name(0)}; "
         f"windows >= {args.window} s, median of {args.repeats}, contenders alternated; cap = {cap}; default flavour and sums, "
         f"full list")
    emit("# bytes = 8*nsys*vlen*(11 + L + k), L = mvec - 1, k = mvec; share = bytes / time(a) / 8 TB/s; bar for nsys >= 16: "
         f"ratio >= {BAR}")
    emit(f"{'nsys':>5} {'vlen':>6} {'mvec':>4} {'batch us':>10} {'lone-loop us':>12} {'batch upd/s':>12} {'system upd/s':>13} "
         f"{'share of 8 TB/s':>15} {'ratio b/a':>9}  bar")
    t0 = time.time()
    missed = []
    for n, v, m in points:
        r = measure(torch, nka_amd, L, n, v, m, args.window, args.repeats, args.mem_gb * 1e9)
        if r is None:
            emit(f"{n:5d} {v:6d} {m:4d}   EXCLUDED: both contenders' stored vectors and the input pool, resident together so that "
                 f"the two can alternate, need more than {args.mem_gb:g} GB of device memory")
            continue
        bar = "-" if n < 16 else ("ok" if r["ratio"] >= BAR else "MISSED")
        if bar == "MISSED":
            missed.append((n, v, m, r["ratio"]))
        emit(f"{n:5d} {v:6d} {m:4d} {r['t_batch_us']:10.1f} {r['t_lone_us']:12.1f} {r['updates_per_s']:12.1f} "
             f"{r['system_updates_per_s']:13.0f} {r['share_of_peak']:15.3f} {r['ratio']:9.2f}  {bar}   "
             f"(spread a {100 * r['spread_a']:.1f} % b {100 * r['spread_b']:.1f} %)")
    emit(f"# {len(points)} points in {time.time() - t0:.0f} s; missed the bar: {missed if missed else 'none'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
