/*
 * nka_hip_batch.h -- OPTIONAL: a BATCHED accelerator, many small independent systems advanced by one kernel launch
 * (libnka_hip.so; the core of include/nka_hip.h and its entries do not change, and nothing here changes what they return).
 *
 * A lone handle (nka_hip_create) spends a small update on kernel boundaries and on a scalar step that runs on one wavefront
 * while the rest of the device idles.  A caller with MANY independent small systems of equal shape -- an ensemble or
 * parameter sweep, one nonlinear solve per mesh column or subdomain, the stages of an implicit integrator per cell -- creates
 * one batch instead: `nsys` independent NKA states (own subspace, own drop decisions, own history), and
 * nka_hip_batch_accel_update advances all of them in ONE launch with ONE workgroup per system (nka_amd/csrc/nka_batch.hip:
 * skip / norm / other sums / scalar step / combine, separated by workgroup barriers instead of kernel boundaries).  A lone
 * system is what lone handles are for: a batch of one is supported and correct, but it runs on one compute unit.
 *
 *   LAYOUT   f_dev is nsys rows of ld doubles (ld >= vlen), row `sys` holds system `sys`.  Its span -- (nsys-1)*ld + vlen
 *            doubles -- and the mask's are checked against their allocations before any launch, like every pointer that
 *            crosses this ABI.  Rows that are 16-byte aligned are read with 16-byte loads, others element by element: the
 *            same bits.
 *   MASKS    active_dev: nsys int32 in DEVICE memory (0 = the system sits this call out), or NULL for all systems.  The mask
 *            stays on the device, so a caller's per-system convergence test never reaches the host.  For a system that sits
 *            out, its row of f and every byte of its state are left exactly as they were.
 *   ASYNC    accel_update, accel_step, restart, relax and set_vec_tol only enqueue on the batch's stream: no allocation, no
 *            synchronisation.  The queries synchronise it.  Not thread-safe per batch; distinct batches are independent.
 *   GRAPHS   The list length is read on the device, per system: no kernel width depends on what the host knows.  An update
 *            can therefore be captured into a hipGraph FROM THE FIRST UPDATE ON and replayed through drops, relax and
 *            restart (a lone handle: only once its list is full, nka_hip_capture_safe).
 *   BITS     Results are bitwise reproducible and do not depend on nsys, on a system's position in the batch, on ld or the
 *            alignment of its row, or on which other systems are active: no workgroup reads what another writes, there are
 *            no atomics, flags or cooperative launches.  The bits are held over the whole binary64 exponent range, inputs of
 *            magnitude 2^-540 ... 2^600 -- subnormal and underflowed norms, s == 0 from underflow and s == Inf included -- against the
 *            oracle for the reference order and the lane batch, and as exact covariance under 2^+-400 for the fast sums
 *            (tests/test_scale_range_gpu.py).
 *   ERRORS   Status codes, nka_hip_last_error() and the resolution of NKA_HIP_FLAVOR_DEFAULT / NKA_HIP_FLAVOR are the core's.
 *            Storage is the lone handle's for the flavour: nka_hip_batch_get_w / _get_v return what nka_hip_get_w / _get_v
 *            return (compact storage in the C flavour: v holds fl(v' - w') of a normalised pair).
 *   SUMS     NKA_HIP_SUMS_AUTO = reference order for vlen <= 64, else _BLOCKED_ROUNDED; NKA_HIP_SUMS_REFERENCE_ORDER (every
 *            sum element after element, one rounding per product and per addition, the norm first, then the rows on the
 *            rounded w1': a system then carries the BITS of the reference flavour it runs; validation speed, at every vlen)
 *            and NKA_HIP_SUMS_BLOCKED_ROUNDED (products by fma, per-thread strided accumulation, fixed-order reduction over
 *            the workgroup; held to the numerical contract of nka_hip.h, items 1 and 3) are accepted.  NKA_HIP_SUMS_BLOCKED is
 *            refused with NKA_HIP_EINVAL: a batch has no exchange to save.
 *   LIMITS   1 <= vlen <= NKA_HIP_BATCH_MAX_VLEN, 1 <= mvec <= NKA_HIP_BATCH_MAX_MVEC, nsys >= 1, vtol > 0: NKA_HIP_EINVAL
 *            outside; device memory that does not suffice: NKA_HIP_ENOMEM.  NKA_HIP_BATCH_MAX_VLEN = 16 384 is MEASURED
 *            (profiles/r08/batch_throughput.txt, 1 x MI355X): the largest power of two at which the batch beats a loop over
 *            lone handles at every grid point from 16 systems on.  At the cap, mvec = 20: 1.52 x with 16 systems, 17 x with
 *            256, 23 x with 4096 (0.55 of 8 TB/s); at vlen = 1024, mvec = 10: 9.2 x / 151 x / 444 x.  Beyond it a 16-system
 *            batch -- 16 of 256 compute units -- loses (0.99 x at 32 768, mvec = 20): longer systems are for WIDE below, or lone handles.  A
 *            batch of ONE is slower than a lone handle at most shapes (0.10 ... 1.76 x, recorded without a bar).  Every offset
 *            into w, v, f, x and the weight rows is formed in 64 bits, in both kinds of batch and with lengths: systems beyond
 *            4 GiB and beyond 2^31 elements are held to a small twin batch with == (tests/test_batch_large_gpu.py).
 *   WEIGHTS  nka_hip_batch_set_dot_weights: the dp  <x,y>_w = sum_i w_i x_i y_i  per system, on the device, inside the same
 *            one launch (unknowns of different scale, masks on ghost or fixed entries, ragged batches).  a_w = fl(w_i * a_i)
 *            is the FIRST operand of every product; with d = fl(w1 - f) and w1' the flavour's rounding as above:
 *                          NKA_HIP_SUMS_BLOCKED_ROUNDED                 NKA_HIP_SUMS_REFERENCE_ORDER
 *              red[0]      sum fma(fl(w d),   d,   .)                   acc = acc + fl(w d)   * d       dp(d, d)
 *              red[1]      sum fma(fl(w f),   w1', .)                   acc = acc + fl(w f)   * w1'     dp(f, w1')
 *              red[2+p]    sum fma(fl(w w1'), w_p, .)                   acc = acc + fl(w w1') * w_p     dp(w1', w_p)
 *              red[2+m+p]  sum fma(fl(w f),   w_p, .)                   acc = acc + fl(w f)   * w_p     dp(f, w_p)
 *            The fast column is the NKA_HIP_SUMS_BLOCKED_ROUNDED column of the table under nka_hip_set_dot_weights (nka_hip.h)
 *            with the batch's element -> thread map, per-thread order and workgroup reduction unchanged; fl(w f) is formed once
 *            per element and sweep.  In reference order a system carries the bits of the reference run with
 *            dp(x, y) = sum in order of fl(fl(w_i x_i) * y_i), the operands in the order the reference passes them.  UNLIKE A
 *            LONE HANDLE, a batch therefore does NOT refuse weights in reference order, and NKA_HIP_SUMS_AUTO resolves as
 *            without weights: reference order up to 64 elements.  The combine does not read the weights.  Exact consequences
 *            (tests/test_batch_weights_gpu.py): w == 1 returns the plain batch's bits; w_i = 4^k per system returns
 *            2^-k o (a plain batch on 2^k o F), bit for bit, with the same decisions; w_i = 0 keeps entry i out of every sum
 *            and every decision while the values there stay finite (0 * Inf is NaN, as in the reference's dp).
 *            RAGGED BATCHES: systems of different length L_sys <= vlen are padded to vlen, with w = 1 below L_sys and 0 from
 *            there on.  Sums, decisions and f[0 .. L_sys) of such a system are then BIT-EQUAL to those of a batch of
 *            vlen = L_sys -- fma(+-0, b, acc) = acc for finite b, and a thread meets its elements in the same order at either
 *            length -- whatever finite values the padding of f holds (the combine still runs over it: keep it finite).
 *            The recipe costs a stream, runs every pass over the padding, uses up the weights and does not exist for a wide
 *            batch: LENGTHS below gives a system its own length natively, on both kinds of batch.
 *            COST, MEASURED (profiles/r09/batch_weights_throughput.txt, 1 x MI355X; nsys 256 / 4096 x vlen 1024 / 16 384 x
 *            mvec 10 / 20): a weighted update takes 0.93 ... 1.03 x the time of a plain one with the shared row, 0.93 ... 1.14 x
 *            with one row per system -- the 1.14 (mvec 10; 1.10 at mvec 20) at 4096 x 16 384, where 512 MB of weights stream
 *            from memory and the count of streams per element (norm pass 2 -> 3, each sweep of four 6 -> 7, combine unchanged:
 *            +10.8 % / +10.2 %) is what it costs.
 *   STEP     nka_hip_batch_accel_step: the loop around an update -- f = residual(x); test ||f||; accel_update(f); x -= f, the
 *            reference's own example (nka_example.F90:243-254) -- with everything but the residual inside the SAME one launch.
 *            Per system with active[sys] != 0 on entry (active_dev == NULL: all):
 *              1  r = sqrt(dp(f, f)) with the dot product the batch runs at that moment, weights and sum order: fast sums
 *                 sum fma(a, f_i, .) with a = f_i, or fl(w_i f_i) when weighted, in the element -> thread map, per-thread order
 *                 and workgroup reduction of every other sum; reference order acc = acc + a * f_i, element after element.
 *                 fnorm_dev[sys] = r if fnorm_dev is given.  The stop rule therefore measures what the accelerator minimises.
 *              2  if tol_dev is given and r <= tol_dev[sys], the system RETIRES ITSELF: active_dev[sys] = 0, and nothing else of
 *                 it is written -- its rows of f and x, its control block, red[], slots and digest stay as they were.  A NaN on
 *                 either side compares false and the system goes on, like the reference with a NaN norm.  The reference's
 *                 example stops at `<`; this entry stops at `<=`, so that tol = 0 retires an exactly zero residual.
 *              3  otherwise the update of nka_hip_batch_accel_update -- the row of f, the state and red[] BIT-EQUAL to that
 *                 entry's -- and then, if x_dev is given, x_i = fl(x_i - f_out_i) over the row (f_out: what the update leaves
 *                 in f).  Rows of x that are 16-byte aligned use 16-byte accesses, others go element by element: the same bits.
 *            A system inactive on entry has nothing read or written, fnorm_dev[sys] included.  One launch on the batch's
 *            stream, nothing allocated or synchronised, capturable from the first call on; each workgroup writes only its own
 *            entries of active and fnorm, so BITS above holds unchanged.  NKA_HIP_EINVAL, the batch staying usable: tol_dev
 *            without active_dev (a system cannot retire without a mask); ldx < vlen; the span of x overlapping the span of f;
 *            fnorm overlapping tol (a threshold would be overwritten while it is read); the span of x ((nsys-1)*ldx + vlen
 *            doubles), fnorm, tol or active (nsys entries each) not inside its allocation.
 *            RELATIVE TOLERANCES: call once with tol_dev = NULL and fnorm_dev given, then form tol = TOL * fnorm with a device
 *            operation of the caller's: no host round trip.
 *            COST, MEASURED (profiles/r10/batch_step_throughput.txt, 1 x MI355X; nsys 256 / 4096 x vlen 64 / 1024 / 16 384 x
 *            mvec 10 / 20): a step with x, mask, tol and fnorm takes 0.92 ... 1.10 x the time of a plain update (the combine
 *            moves 9 + k streams per element instead of 7 + k) and 0.75 ... 0.99 x the time of the same loop composed from
 *            accel_update and three kernels of the caller -- EXCEPT at 4096 x 64, which runs in reference order: 1.21 / 1.07 x
 *            a plain update and 1.06 / 1.03 x the composed loop (mvec 10 / 20; dp(f, f) is one more dependent chain there).
 *   WIDE     nka_hip_batch_create_wide: the same handle type, every entry below and every guarantee above (MASKS, ASYNC, GRAPHS,
 *            BITS), for systems too long for one workgroup: a system is ceil(vlen / NKA_HIP_BATCH_WIDE_CHUNK) chunks with ONE
 *            WORKGROUP PER CHUNK, and an update is FOUR launches in a line on the batch's stream (nka_amd/csrc/
 *            nka_batch_wide.hip: norm / other sums / scalar step / combine), the phases that need a sum over the whole system
 *            separated by kernel boundaries.  Within a launch no workgroup reads what another writes: still no flags, no
 *            spinning, no atomics, no cooperative launch.  A sum is formed per chunk exactly as the batch above forms it over a
 *            system -- a chunk is whole tiles of 512 elements -- and the partials of the chunks are then added IN CHUNK ORDER,
 *            starting from chunk 0, by one thread: the bits of a sum depend on NKA_HIP_BATCH_WIDE_CHUNK and on nothing else, and
 *            a wide batch of at most one chunk returns the bits of the batch above in NKA_HIP_SUMS_BLOCKED_ROUNDED.  red[] keeps
 *            its meaning, the zeros included; which partials are read is decided from the list, never from what the buffer
 *            holds.  Captured into a graph it is four kernel nodes in a line, from the first update on.
 *            1 <= vlen <= NKA_HIP_BATCH_WIDE_MAX_VLEN (short systems are legal), mvec as above, nsys <= 65 535 (the system is
 *            the second grid index).  Beside the slots it allocates nsys * (2 + 2 mvec) * nchunk doubles of partial sums and
 *            the combine plan (the control block's comb_slots / comb_c stay zero, so that its digest is the narrow batch's).
 *            NKA_HIP_SUMS_AUTO and _BLOCKED_ROUNDED both mean the rounded fast sums, at every vlen.  REFUSED with NKA_HIP_EINVAL,
 *            the batch staying usable: nka_hip_batch_accel_step on a batch of nka_hip_batch_create_wide (a batch of
 *            nka_hip_batch_create_wide_step offers it: STEP below); on a batch of these two entries nka_hip_batch_set_dot_weights and
 *            _set_dot_weights_host (nka_hip_batch_dot_weighted returns 0; a batch of nka_hip_batch_create_wide_ext offers them: WIDE
 *            EXT below); on every wide batch NKA_HIP_SUMS_REFERENCE_ORDER and _BLOCKED through
 *            _set_sum_order, and binary32 storage (a batch of nka_hip_batch_create_wide_stored offers it: WIDE STORED below).  A
 *            caller who needs the reference order has the batch above up to 16 384 elements and lone handles beyond.
 *            STEP of a wide batch: nka_hip_batch_create_wide_step is nka_hip_batch_create_wide -- the same limits, refusals, kind
 *            (nka_hip_batch_kind 1, _is_wide 1) and accel_update, bit for bit and launch for launch -- with ONE MORE BUFFER: nsys *
 *            nchunk doubles, one partial of <f,f> per chunk and system, zero-initialised, freed at destroy, never moved.  That
 *            buffer is why the step has a creation entry of its own: what nka_hip_batch_create_wide allocates stays what it
 *            documents, and such a batch keeps refusing the step.  nka_hip_batch_offers_step tells the two apart.  On a batch of
 *            the new entry nka_hip_batch_accel_step is FOUR launches in a line (nka_amd/csrc/nka_batch_wide.hip), per
 *            system active on entry:
 *              1  r = sqrt(sum_c q_c), q_c the fast-sum <f,f> of chunk c;
 *              2  q_c = sum fma(f_i, f_i, .) in the chunk's element -> thread map and per-thread order, reduced over the
 *                 workgroup like every other sum of the chunk (lanes by butterfly, then wavefronts 0, 1, 2, 3);
 *              3  the partials are added in chunk order from chunk 0, by one thread: r depends on NKA_HIP_BATCH_WIDE_CHUNK and on
 *                 nothing else, and at one chunk it is the r of the batch above in NKA_HIP_SUMS_BLOCKED_ROUNDED;
 *              4  fnorm_dev[sys] = r if fnorm_dev is given;
 *              5  if tol_dev is given and r <= tol_dev[sys] the system retires: active_dev[sys] = 0, and nothing else of it is
 *                 written -- rows of f and x, control block, red[], slots and digest stay (its partial sums are scratch: no later
 *                 call reads one it did not write itself).  A NaN on either side compares false;
 *              6  otherwise the update is BIT-EQUAL to accel_update of a wide batch -- row of f, state, red[], slots --, and
 *                 x_i = fl(x_i - f_out_i) if x_dev is given, with 16-byte accesses on a 16-byte-aligned row and element by element
 *                 otherwise: the same bits;
 *              7  a system inactive on entry has nothing read or written, fnorm_dev[sys] included;
 *              8  every pointer but f may be NULL;
 *              9  captured into a graph it is four kernel nodes in a line, from the first call on; nothing is allocated or
 *                 synchronised.
 *            tol is read by launches 2 and 3 and fnorm written by launch 3 (their overlap is refused, as above); active[sys] is
 *            cleared by launch 3, in the one workgroup of that launch that reads the entry, and read again by launch 4: within a
 *            launch no workgroup reads what another writes.  The host checks are those of STEP above.  LENGTHS below applies: a
 *            system's r, update and x -= f_out cover len[sys] elements and its own chunks.
 *            COST, MEASURED (profiles/r16/batch_wide_step_throughput.txt, 1 x MI355X; nsys 16 / 64 / 256 x vlen 32 768 / 65 536 /
 *            262 144 x mvec 10 / 20; default flavour, full lists; the two points at 256 x 262 144 need more than 40 GB and were
 *            not measured): a step with x, mask, tol and fnorm, no system retiring, takes 0.80 ... 0.99 x the time of the same
 *            loop composed from accel_update of a wide batch and three kernels of the caller -- 0.81 / 0.80 / 0.80 at 16 systems
 *            and mvec 10, 0.90 ... 0.96 at mvec 20 up to 64 systems -- and 0.98 ... 1.11 x the time of a plain wide update.  With
 *            the composed loop run twice as its own control (it differs from itself by at most 3.0 %), the step is faster by
 *            more than that difference at 15 of the 16 points and level at one (256 x 65 536 x 20: 0.987, control 3.0 %);
 *            slower nowhere.  One measurement; no ratio was fixed beforehand.
 *            BOTH CONSTANTS ARE MEASURED (profiles/r11/batch_wide_throughput.txt, 1 x MI355X) and frozen.  CHUNK = 2048: of
 *            2048 / 4096 / 8192 the fastest at (nsys, vlen, mvec) = (16, 65 536, 20) and (64, 262 144, 10): 243.7 / 260.4 /
 *            320.6 us and 828.0 / 831.7 / 853.5 us per update, windows spread 0.1 %.  MAX_VLEN = 1 048 576: by the rule of
 *            NKA_HIP_BATCH_MAX_VLEN, 16 systems still beat the loop over lone handles there at both mvec (1.31 x at mvec 10, 1.18 x
 *            at 20), and the grid holds no longer system; 1024 chunks would be the limit.
 *            WHICH OF THE THREE ENTRIES (time of the loop over lone handles / time of the wide batch; default flavour, full
 *            list): from 16 systems on the wide batch wins at every length measured -- at 32 768 and 65 536 elements, where the
 *            batch above is not offered, 2.35 ... 15.2 x (16 systems: 6.05 / 4.69 x at mvec 10, 2.67 / 2.35 x at mvec 20; 256
 *            systems: 15.2 / 8.15 x and 11.0 / 6.20 x, 0.50 ... 0.58 of 8 TB/s), at 262 144: 1.65 ... 3.03 x, at 1 048 576:
 *            1.18 ... 1.42 x.  Up to 16 384 elements take the batch above for few or very many short systems and the wide one in
 *            between: at 4096 elements the two are level (wide / narrow 0.90 ... 1.06), at 16 384 the wide batch is 1.04 ... 2.45 x
 *            faster (2.45 x at 16 systems, 1.14 / 1.04 x at 256); both have the step (the wide one through
 *            nka_hip_batch_create_wide_step) and the weights (the wide one through nka_hip_batch_create_wide_ext: WIDE EXT below), and only the batch above has the reference order.  FOUR systems: the wide batch wins at mvec = 10 (1.05 ... 1.95 x) and LOSES to four lone handles at
 *            mvec = 20 at every length (0.67 ... 0.86 x): the scalar step of a system runs on one thread, 127 us at mvec = 20 (59 %
 *            of an update at 16 x 65 536), and a lone handle's does not (SCALAR STEP below: the opt-in that runs it on one wavefront,
 *            and what the loss becomes with it).  A lone system stays with a lone handle.
 *   LENGTHS  nka_hip_batch_set_lengths: RAGGED BATCHES without padding weights, on both kinds of batch.  System `sys` is
 *            len[sys] elements long, 1 <= len[sys] <= vlen, in EVERY phase of accel_update and accel_step: the norm and the
 *            other sums in either order, the step's dp(f, f) and x -= f_out, the weight loads, the combine and the ring stores.
 *            The kernel reads len[sys] once at entry (one uniform scalar load per workgroup); NOTHING at an index >= len[sys]
 *            of the system's rows of f and x, of its weight row or of any of its slots is read or written, so the tails may
 *            hold anything, NaN included.  In a wide batch the system owns its first ceil(len[sys] / CHUNK) chunks; the
 *            workgroups of its other chunks return before they read anything, and only its own partials are added, in chunk
 *            order from chunk 0 (the partials keep the batch's stride; the grid stays nchunk x nsys).  Still no workgroup reads
 *            what another writes: no flags, no atomics, no spinning, no cooperative launch.
 *            THE CONTRACT: for a system of length L in a batch of length vlen >= L that has had that length since creation or
 *            since its last restart, after every accel_update / accel_step the following are BIT-EQUAL to those of the same
 *            system in a batch of the same kind created with vlen = L: f[0 .. L), x[0 .. L), red[], the state, num_vec, the
 *            digest, fnorm and the retirement decision, and [0 .. L) of every slot.  Same kind: narrow against narrow, wide
 *            against wide, the same flavour, the same EXPLICIT sum order, the same weights on [0 .. L).  The elements from L on
 *            are untouched.  This is derived, not fitted: the element -> thread map and the order in which a thread meets its
 *            elements do not depend on the length, and a chunk is whole tiles (tests/test_batch_lengths_gpu.py holds it with ==).
 *            UNCHANGED BY LENGTHS: f_dev, x_dev and the weight rows keep their shape -- nsys rows of ld / ldx / ldw >= vlen --
 *            and their span checks; nka_hip_batch_get_w / _get_v return vlen doubles; NKA_HIP_SUMS_AUTO keeps resolving from the
 *            batch's vlen, never from a system's length (the host needs no length to pick a kernel, which is what keeps a
 *            replay valid); everything a wide batch refuses stays refused; a batch without lengths computes and launches
 *            exactly what it did.  A length of 0 is refused: a system that should sit out is what `active` is for.
 *   STORAGE  nka_hip_batch_create_stored(..., NKA_HIP_BATCH_STORE_F32): OPT-IN binary32 storage of the NORMALISED subspace vectors.
 *            Everything a batch stores except the pending pair is a normalised vector -- w' has norm 1, v' is scaled by the
 *            same 1/s -- used only as an operand of sums and of the combine; the stored vectors are nearly all of an update's
 *            memory traffic and the memory limit on nsys.  With q(x) = conversion to binary32, round to nearest even, widened
 *            back exactly, EVERY PRODUCT AND ACCUMULATION STAYS binary64, and:
 *              1  it runs the default flavour (NKA_HIP_FLAVOR_C: compact storage) and NKA_HIP_SUMS_BLOCKED_ROUNDED only;
 *                 NKA_HIP_SUMS_AUTO resolves to _BLOCKED_ROUNDED at EVERY vlen, vlen <= 64 included.  REFUSED with NKA_HIP_EINVAL:
 *                 the two F08 flavours and NKA_HIP_SUMS_REFERENCE_ORDER (their point is the reference's bits, which this storage
 *                 gives up), and a WIDE batch with this storage through this entry and the three older wide entries, which stay
 *                 binary64 (a batch of nka_hip_batch_create_wide_stored offers it: WIDE STORED below).
 *              2  THE PENDING PAIR STAYS binary64: the raw pair (w_new = f_in, v_new = f_out) lives in two buffers of the batch,
 *                 one row per system at the slot stride, not in the ring slot.  d = fl(w1 - f), red[0] and s = sqrt(red[0]) are
 *                 therefore exactly those of binary64 storage.
 *              3  w1' = q(fl(d/s)).  This rounded value is the operand of every sum of phase 3 (fl(w w1') the first operand under
 *                 weights, as in WEIGHTS), the value stored in the ring slot, and the value the compact difference is formed from.
 *              4  the ring slot's v holds q(fl(fl(v1/s) - w1')), w1' the rounded value of 3, and the combine applies exactly that
 *                 stored value for pair 0 and every older pair: x = fl(x + fl(c v_p)) in list order, in binary64.  WHAT IS STORED
 *                 IS WHAT WAS USED: Gram rows, right-hand sides and the combine see one and the same set of vectors.
 *              5  binary32 SUBNORMAL results are kept (the kernels run with f32 denormals enabled; the stored bits are numpy's
 *                 astype(float32), tests/test_batch_store32_gpu.py).  |w1'| <= 1 cannot overflow.  A component of
 *                 fl(v1/s) - w1' beyond the binary32 range is stored as +-Inf, and the system then carries non-finite values
 *                 inside its own rows, like a system that was fed them; no other system is affected.  Systems whose unknowns
 *                 differ by more than about 1e38 in scale between a moving and a frozen entry are for binary64 storage.
 *              6  every other guarantee above holds unchanged: MASKS, ASYNC, GRAPHS from the first update, BITS, WEIGHTS, STEP and
 *                 LENGTHS (nothing at or beyond len[sys] of the binary32 slots or the pending buffers is read or written),
 *                 restart / relax / set_vec_tol and the span checks.
 *              7  nka_hip_batch_get_w / _get_v return binary64 arrays: for the slot of the pending pair the pending buffers'
 *                 rows, for any other slot the widened stored values; a never-written slot reads zeros.  state_digest,
 *                 get_state, num_vec and get_reductions keep their meaning.
 *            MEMORY: the stored vectors take 2 nsys stride (4 (mvec + 1) + 8) bytes instead of 2 nsys stride 8 (mvec + 1)
 *            (stride: vlen rounded up to 32; nka_hip_batch_vector_bytes), 0.55 of binary64 storage at mvec = 20 and 0.59 at 10.
 *            A batch created with nka_hip_batch_create, or with NKA_HIP_BATCH_STORE_F64, computes and launches exactly what it did.
 *            COST, MEASURED (profiles/r13/batch_store32_throughput.txt, 1 x MI355X; a binary64 batch, a second one as a control and
 *            the binary32 batch alternated on the same inputs; nsys 256 / 4096 x vlen 1024 / 16 384 x mvec 10 / 20): at
 *            4096 x 16 384, where an update is bound by the bytes it moves, 0.760 (mvec 10) and 0.714 (mvec 20) of the time of
 *            the binary64 update -- the byte model (per element: norm pass 16 B; each sweep of four 48 -> 32 B; combine
 *            8 (7 + k) -> 56 + 4 (k - 1) B) predicts 0.69 and 0.65 --, the two binary64 batches differing by 2.1 % and 0.8 %;
 *            0.82 / 0.87 at 4096 x 1024, 0.89 / 0.90 at 256 x 16 384, 0.98 / 1.02 at 256 x 1024.  At 4096 x 64 x 10 it takes
 *            1.22 x: binary64 storage runs such systems in reference order under NKA_HIP_SUMS_AUTO, this storage the fast sums.
 *   LANES    nka_hip_batch_create_lanes: the same handle type for VERY SHORT systems, 1 <= vlen <= NKA_HIP_BATCH_LANES_MAX_VLEN = 64,
 *            with ONE LANE PER SYSTEM (nka_amd/csrc/nka_batch_lanes.hip).  The batch above gives such a system a workgroup of
 *            256 threads of which one forms each sum and one runs the scalar step; here a workgroup is one wavefront that
 *            advances G systems -- nka_hip_batch_lanes_limits(mvec): the most working copies that fit 64 KiB of LDS, at most 64;
 *            64 up to mvec = 6, 37 at 10, 13 at 20, 6 at 32 --, lane l of workgroup g owns system g * G + l through every phase,
 *            and the grid is ceil(nsys / G).  One launch per call.  The cap is DERIVED, not measured: it is the range in which
 *            NKA_HIP_SUMS_AUTO of the batch above already means the reference order, so a lane batch and a default batch from
 *            nka_hip_batch_create are interchangeable bit for bit.  mvec, vtol, nsys >= 1 and all three flavours as above.
 *            OFFERED with their signatures and guarantees (MASKS, ASYNC, GRAPHS from the first update, BITS, the span checks):
 *            accel_update; accel_step with x, tol, fnorm and active each optional, and its refusals; restart, relax,
 *            set_vec_tol, set_stream; num_vec, get_state, get_reductions, get_w, get_v (gathered from the interleaved slots),
 *            state_digest, storage (NKA_HIP_BATCH_STORE_F64), vector_bytes (2 * 8 * ceil(nsys / G) * G * (mvec + 1) * vlen: the
 *            slots are interleaved across the systems of a group, the last group whole, rows not padded); set_sum_order with
 *            NKA_HIP_SUMS_AUTO and _REFERENCE_ORDER, which both mean the reference order.  nka_hip_batch_is_wide returns 0,
 *            nka_hip_batch_kind 2.  REFUSED with NKA_HIP_EINVAL, the batch staying usable: nka_hip_batch_set_dot_weights and
 *            _host (dot_weighted returns 0), nka_hip_batch_set_lengths and _host (has_lengths returns 0), NKA_HIP_SUMS_BLOCKED
 *            and _BLOCKED_ROUNDED, and creation with vlen > 64; a caller who needs one of these has the batch above.  There is
 *            no binary32 storage for this kind (nka_hip_batch_create_stored stays the batch above): a possible follow-up.
 *            THE CONTRACT: for every system, after every call, the row of f, the row of x, red[] with its zeros, the state,
 *            num_vec and the digest, fnorm and the retirement decision, and w and v of every slot are BIT-EQUAL to those of the
 *            same system in a batch from nka_hip_batch_create of the same flavour in NKA_HIP_SUMS_REFERENCE_ORDER -- and
 *            therefore to the reference flavour it runs.  This is derived, not fitted: each sum is one chain a = a + x * y in
 *            element order on one lane, one rounding per product and per addition (contraction off), the operands in the order
 *            of the reference-order kernel above; the scalar step is the same statements on the lane's own working copy; the
 *            elementwise statements are the flavour's (fl(d/s) or fl(fl(1/s) d), the flavour's association of the combine,
 *            compact storage in the C flavour).  The bits do not depend on nsys, on the position of the system, on the lane
 *            or group it lands in, on the other systems' masks or values, or on ld / ldx.  A masked, retired or absent system
 *            is a predicated lane: no byte of it is read or written, and no workgroup or lane reads what another's system owns
 *            (tests/test_batch_lanes_gpu.py holds all of it with ==).
 *            WHICH OF THE THREE KINDS, MEASURED (profiles/r14/batch_lanes_throughput.txt, 1 x MI355X): time of a call / time of
 *            the batch above at NKA_HIP_SUMS_AUTO, default flavour, full lists, the two alternated with a second batch above as
 *            the control (it differs by at most 2.2 %).  At 65 536 systems the lane batch WINS where a working copy is small:
 *            mvec = 5: 0.32 / 0.46 / 0.58 at vlen 8 / 32 / 64; mvec = 10: 0.46 / 0.85 at vlen 8 / 32 (1.10 at 64); a step with x,
 *            mask, tol and fnorm at vlen 32: 0.49 / 0.81.  It LOSES at mvec = 20 (1.41 / 1.09 / 1.74; 13 systems per wavefront,
 *            two wavefronts per CU: LDS bounds residency), at 4096 systems nearly everywhere (1.00 ... 2.63; 0.97 at 32 x 20) and
 *            at 256 systems everywhere (1.9 ... 5.5): a call then costs the latency of one wavefront that does serially what 256
 *            threads share, 48 ... 470 us whatever nsys is.  So: tens of thousands of systems of at most 64 unknowns with mvec up
 *            to about 10 -- this kind; fewer systems or mvec = 20 -- the batch above, which returns the same bits; systems
 *            beyond 16 384 unknowns -- WIDE.
 *   WAVES    nka_hip_batch_create_waves: the same handle type for SHORT systems, 1 <= vlen <= NKA_HIP_BATCH_WAVES_MAX_VLEN, with ONE
 *            WAVEFRONT PER SYSTEM (nka_amd/csrc/nka_batch_waves.hip).  The batch above gives a system a workgroup of 256 threads,
 *            of which one runs the scalar step while 255 wait at a barrier, and a 512-element tile that a system of a few hundred
 *            unknowns fills by a quarter; here a workgroup is four wavefronts that advance four systems -- wavefront w of
 *            workgroup g owns system 4 g + w through every phase, the grid is ceil(nsys / 4) --, no wavefront ever waits for
 *            another (no workgroup barrier in the kernel: a masked, retired or absent system's wavefront returns on its own), and a
 *            tile is 128 elements.  One launch per call.  Storage, control blocks and every query are those of the batch above:
 *            nothing further is allocated.  mvec, vtol, nsys >= 1 and all three flavours as above.
 *            OFFERED with their signatures and guarantees (MASKS, ASYNC, GRAPHS from the first update, BITS, the span checks):
 *            accel_update; accel_step with x, active, tol and fnorm each optional, and its refusals; restart, relax, set_vec_tol,
 *            set_stream; num_vec, get_state, get_reductions, get_w, get_v, state_digest, storage (NKA_HIP_BATCH_STORE_F64),
 *            vector_bytes (the formula of the batch above); set_sum_order with NKA_HIP_SUMS_AUTO and _BLOCKED_ROUNDED, which
 *            both mean the rounded fast sums at EVERY vlen (also at vlen <= 64, where _AUTO of the batch above means the reference
 *            order).  nka_hip_batch_is_wide returns 0, nka_hip_batch_kind 3.  REFUSED with NKA_HIP_EINVAL, the batch staying
 *            usable: nka_hip_batch_set_dot_weights and _host (dot_weighted returns 0), nka_hip_batch_set_lengths and _host
 *            (has_lengths returns 0), NKA_HIP_SUMS_REFERENCE_ORDER and _BLOCKED, binary32 storage (nka_hip_batch_create_stored
 *            stays the batch above), and creation with vlen above the cap, mvec outside 1 ... 32, nsys < 1 or vtol <= 0; a caller
 *            who needs one of these has the batch above.
 *            THE CONTRACT is the NUMERICAL one of the batch above in NKA_HIP_SUMS_BLOCKED_ROUNDED, and the sums are NOT ITS BITS:
 *            a sum here is two fma per lane and 128-element tile (lane l owns the pair 2l, 2l + 1 of every tile, in increasing
 *            order) and then the six-level butterfly of one wavefront, where the batch above sums 512-element tiles over 256
 *            threads and adds four wavefronts.  Every entry of red[] is within gamma(K) sum|x_i y_i| of the exact sum of its
 *            operands, K = 2 ceil(vlen / 128) + 6 (derived from the kernel, held by tests/test_batch_waves_gpu.py), with the
 *            zeros of the batch above; the sums on w1' are taken on the ROUNDED w1' the slot will hold; given its sums, the scalar
 *            step is the reference's by construction (the same statements, run by lane 0 on the wavefront's working copy), and
 *            the elementwise statements are the flavour's, bit for bit.  The bits of a system depend on its own values alone: not
 *            on nsys, on the system's position or the wavefront it lands on, on the other systems' masks or values (NaN and Inf
 *            included), on ld / ldx or on the alignment of a row.
 *            WHICH KIND, MEASURED: (profiles/r15/batch_waves_throughput.txt, 1 x MI355X): time of a call / time of the batch above at
 *            NKA_HIP_SUMS_BLOCKED_ROUNDED, default flavour, full lists, the two alternated with a second batch above as the
 *            control (it differs by at most 3.8 %), mvec = 5 / 10 / 20.  NKA_HIP_BATCH_WAVES_MAX_VLEN = 1024 is MEASURED: the
 *            largest power of two v such that at 4096 systems, at every vlen <= v of the grid (65, 128, 256, 512, 1024, 2048,
 *            4096; a build with the cap at 4096 measured them) and at all three mvec, this kind is faster than the batch above by
 *            more than the control's difference.  At 4096 systems it WINS up to the cap: 0.36 / 0.33 / 0.29 at vlen 65,
 *            0.37 / 0.33 / 0.30 at 128, 0.44 / 0.39 / 0.31 at 256, 0.81 / 0.59 / 0.39 at 512, 0.93 / 0.73 / 0.52 at 1024; beyond it
 *            the short lists lose -- 1.09 / 0.94 / 0.69 at 2048, 1.20 / 1.11 / 0.90 at 4096 --, which is why the cap is where it is.
 *            At 65 536 systems: 0.28 / 0.26 / 0.25 at 65, 0.25 / 0.25 / 0.25 at 128, 0.36 / 0.29 / 0.26 at 256, 0.76 / 0.56 at 512
 *            (mvec 5 / 10), and 1.01 at 1024 x 5 -- a LOSS inside the cap; a step with x, mask, tol and fnorm at vlen 256, mvec
 *            10 / 20: 0.42 / 0.35 at 4096 systems, 0.36 / 0.31 at 65 536.  At 256 systems it LOSES EVERYWHERE, 1.04 ... 1.23 up to
 *            vlen 256, 1.3 ... 1.4 at 512, 1.4 ... 1.8 at 1024 (1.6 ... 2.4 beyond the cap): 64 workgroups cannot fill 256 compute
 *            units, and a call then costs the latency of one wavefront that sweeps alone what 256 threads share.  So: thousands of
 *            systems of 65 ... 1024 unknowns -- this kind (the longer the list the larger the gain; at mvec = 5 and vlen 1024 it is
 *            a draw); a few hundred systems or fewer, longer systems, or a caller who needs the reference order or binary32 storage
 *            -- the batch above (weights and lengths: WAVES EXT below); at most 64 unknowns and tens of thousands of systems with mvec up to about
 *            10 -- LANES; beyond 16 384 unknowns -- WIDE.
 *   WAVES EXT  nka_hip_batch_create_waves_ext: THE WAVE BATCH WITH LENGTHS AND WEIGHTS (nka_amd/csrc/nka_batch_waves.hip).  Limits,
 *            cap, flavours, storage and every guarantee of WAVES; nothing more is allocated at creation (the weight and the length
 *            buffer come at the first set, as in the batch above), and nka_hip_batch_kind stays 3.  What it adds is exactly the two
 *            entries WAVES refuses: nka_hip_batch_set_lengths / _host and nka_hip_batch_set_dot_weights / _host, with the host side,
 *            the checks and the refusals of the batch above (values checked before they are copied, refused values leave the
 *            previous ones in force, NKA_HIP_ESTATE while the stream is capturing, a row stride of 0 = one shared row).
 *            set_sum_order and binary32 storage stay refused as in WAVES.  A batch of nka_hip_batch_create_waves keeps every
 *            refusal it has; nka_hip_batch_offers_lengths / _offers_weights tell the two apart.
 *            LENGTHS: system sys with len[sys] = L is BIT-EQUAL to the same system of a batch of nka_hip_batch_create_waves with
 *            vlen = L -- f[0..L) and x[0..L), red[], state, num_vec and digest, fnorm and the retirement decision, [0..L) of every
 *            slot --, and nothing at or beyond L is read or written in a row of f or x, in the weight row or in a slot.  Derived,
 *            not fitted: lane l owns the pair 2l, 2l + 1 of every 128-element tile and meets its pairs in increasing order
 *            whatever the length is, and the butterfly does not depend on it.
 *            WEIGHTS: fl(w_i a_i) is the FIRST operand of every product, the table of the batch above: red[0] = sum fma(fl(w d), d, .),
 *            red[1] = sum fma(fl(w f), w1', .), red[2+p] = sum fma(fl(w w1'), w_p, .), red[2+m+p] = sum fma(fl(w f), w_p, .), the
 *            step's <f,f> = sum fma(fl(w f), f, .); fl(w f) is formed once per element and sweep, the combine does not read the
 *            weights.  Every entry is within gamma(K) sum|fl(w x) y| of the exact sum of fl(w x) and y with the K of WAVES at the
 *            system's length (the first operand is already rounded, so K does not change).
 *            NEITHER SET: the batch runs the kernels of WAVES and is that batch bit for bit.  A captured call keeps whether it
 *            was weighted, in which form, and whether it had lengths; it reads the VALUES at replay (GRAPHS from the first update).
 *            WHICH KIND, MEASURED (profiles/r17/batch_waves_ext_throughput.txt, tools/batch_throughput.py --waves-ext, 1 x MI355X):
 *            seven variants alternated in one process on the same inputs, default flavour, NKA_HIP_SUMS_BLOCKED_ROUNDED, full lists,
 *            median of five windows; lengths uniform in [vlen / 4, vlen]; the control (a second batch above with the same lengths)
 *            differs by at most 0.2 %.  RAGGED LENGTHS, time of an update / time of the batch above with the same lengths, mvec =
 *            10 / 20: 0.33 / 0.29 at 4096 x 128, 0.36 / 0.30 at 4096 x 256, 0.63 / 0.43 at 4096 x 1024, 0.30 at 65 536 x 256 x 10.
 *            ONE WEIGHT ROW PER SYSTEM, against the batch above with the same weights: 0.36 / 0.33 at 4096 x 128, 0.44 / 0.36 at
 *            4096 x 256, 0.87 / 0.61 at 4096 x 1024, 0.37 at 65 536 x 256 x 10.  WHAT THE LENGTH ARGUMENT COSTS (every length = vlen
 *            against a batch of nka_hip_batch_create_waves): 1.000 ... 1.014.  Won at 7 of 7 points in both comparisons.  So:
 *            thousands of systems of up to 1024 unknowns that differ in length or in the scale of their unknowns -- this entry;
 *            for every other case the sentences of WAVES stand (256 systems were not measured here: there WAVES loses).
 *   WIDE EXT  nka_hip_batch_create_wide_ext: THE WIDE BATCH WITH WEIGHTS (nka_amd/csrc/nka_batch_wide.hip).
 *            Limits, allocations and every guarantee of nka_hip_batch_create_wide for step == 0 and of nka_hip_batch_create_wide_step
 *            for step == 1 (any other step: NKA_HIP_EINVAL); nka_hip_batch_kind stays 1, _is_wide 1, _offers_lengths 1, _offers_step
 *            returns step, and the weight buffer comes at the first set, as in the batch above.  What it adds is exactly the entry
 *            WIDE refuses: nka_hip_batch_set_dot_weights / _host, with the host side, the checks and the refusals of the batch
 *            above (values checked before they are copied, refused values leave the previous weighting in force, NKA_HIP_ESTATE
 *            while the stream is capturing, a row stride of 0 = one shared row).  set_sum_order and binary32 storage stay refused as
 *            in WIDE; a batch of the two other wide entries keeps refusing the weights; nka_hip_batch_offers_weights tells them apart.
 *            A weighted update, and a weighted step, is still FOUR launches in a line: the first two are the weighted kernels of a
 *            chunk, the scalar step and the combine do not read the weights and are the launches of WIDE.  Within a launch no
 *            workgroup reads what another writes: no flags, no spinning, no atomics, no cooperative launch.
 *            WEIGHTS: fl(w_i a_i) is the FIRST operand of every product, the table of the batch above, per chunk:
 *            part[0] = sum fma(fl(w d), d, .), red[1] = sum fma(fl(w f), w1', .), red[2+p] = sum fma(fl(w w1'), w_p, .), red[2+m+p] =
 *            sum fma(fl(w f), w_p, .), the step's <f,f> = sum fma(fl(w f), f, .); fl(w f) is formed once per element and sweep.
 *            NEITHER SET (weights nor lengths): the batch launches the kernels of WIDE and is a batch of nka_hip_batch_create_wide /
 *            _create_wide_step bit for bit.  ONE CHUNK: a weighted wide batch of at most one chunk is the weighted batch above in
 *            NKA_HIP_SUMS_BLOCKED_ROUNDED, bit for bit.  SEVERAL CHUNKS: every entry of red[] and the step's <f,f> lies within
 *            gamma(K) sum|fl(w x) y| of the exact sum of fl(w x) and y, with the K of WIDE at the system's length (the first operand
 *            is already rounded, so K does not change); red[0] is the chunk-order chain of the chunks' partials.  EXACT
 *            CONSEQUENCES: w == 1 gives the plain wide batch's bits; w = 4^k is an exact rescaling, as under WEIGHTS.  LENGTHS: the
 *            contract of LENGTHS holds with "the same weights on [0 .. L)", and nothing at or beyond len[sys] of the weight row is
 *            read.  ZERO WEIGHTS: a zero weight does not shield a non-finite value, as in the batch above.  A captured call keeps
 *            whether it was weighted and in which form, and reads the VALUES at replay (GRAPHS from the first update).
 *            COST: the norm launch streams three vectors instead of two and each sweep of four of the sums launch seven instead of
 *            six; the combine is unchanged.  What that costs is recorded in profiles/r19/batch_wide_weights_throughput.txt (tools/
 *            batch_throughput.py --wide-weights) and read in docs/design/12_batched_systems.md, "Wide batch: weights".
 *   WIDE STORED  nka_hip_batch_create_wide_stored(..., step, storage): THE WIDE BATCH WITH BINARY32 STORAGE of the normalised subspace
 *            vectors (nka_amd/csrc/nka_batch_wide.hip).  storage == NKA_HIP_BATCH_STORE_F64: the batch of
 *            nka_hip_batch_create_wide_ext(..., step), bit for bit and launch for launch.  storage == NKA_HIP_BATCH_STORE_F32: the
 *            limits of nka_hip_batch_create_wide, step 0 or 1 as in WIDE EXT (the buffer of the step only for 1), weights and
 *            lengths offered; nka_hip_batch_kind 1, _is_wide 1, _offers_step = step, _offers_weights 1, _offers_lengths 1,
 *            nka_hip_batch_storage NKA_HIP_BATCH_STORE_F32, nka_hip_batch_vector_bytes = 2 nsys stride (4 (mvec + 1) + 8), the
 *            formula of STORAGE at the wide batch's slot stride: float slots and the two binary64 pending buffers of one row per
 *            system, zero-initialised, freed at destroy, never moved.  REFUSED with NKA_HIP_EINVAL, nothing left allocated: the two
 *            F08 flavours with binary32, an unknown storage, a step outside {0, 1}, the wide limits.  set_sum_order refuses
 *            NKA_HIP_SUMS_REFERENCE_ORDER and _BLOCKED as on every wide batch; _AUTO and _BLOCKED_ROUNDED are the rounded fast
 *            sums.  The four older entries (_create_wide, _create_wide_step, _create_wide_ext, _create_stored) allocate, refuse and
 *            compute what they did.
 *            THE CONTRACT is that of STORAGE, points 2 to 7, PER CHUNK: the pending pair stays binary64 in the pending rows, so d,
 *            red[0] and s are exactly those of a binary64 wide batch; w1' = q(fl(d/s)) is the operand of every sum (fl(w w1') the
 *            first operand under weights), the value stored and the value the compact difference is formed from; the slot's v
 *            holds q(fl(fl(v1/s) - w1')) and the combine applies exactly that value; binary32 subnormals are kept, a value beyond
 *            the binary32 range becomes +-Inf and stays in its own system; every product and accumulation is binary64;
 *            nka_hip_batch_get_w / _get_v return binary64 (the pending rows for the slot of the pending pair, the widened floats
 *            otherwise).  The two norm launches read binary64 data only, f and the raw w1 of the pending row.  WHAT THE WIDE BATCH
 *            GUARANTEES HOLDS UNCHANGED: FOUR launches in a line; within a launch no workgroup reads what another writes, no flags,
 *            no atomics, no spinning, no cooperative launch; capture from the first call; MASKS, LENGTHS (nothing at or beyond
 *            len[sys] of a float slot or a pending row is read or written), WEIGHTS and STEP.  A chunk starts on a multiple of 2048
 *            elements, so a float pair stays 8-byte aligned.
 *            ONE CHUNK: a binary32 wide batch of at most one chunk is the binary32 batch of nka_hip_batch_create_stored, bit for
 *            bit.  SEVERAL CHUNKS: every entry of red[] and the step's <f,f> lies within gamma(K) sum|xy| of the exact sum of the
 *            operands actually used -- the widened stored values and q(w1') --, with the K of WIDE at the system's length: K is
 *            unchanged, because widening is exact and the narrowing precedes the product; red[0] is the chunk-order chain of the
 *            chunks' partials (tests/test_batch_wide_store32_gpu.py holds all of it).
 *            MEMORY: 0.55 of the stored vectors of a binary64 wide batch at mvec = 20 and 0.59 at 10, as in STORAGE.
 *            COST, MEASURED (profiles/r21/batch_wide_store32_throughput.txt, 1 x MI355X; a binary64 batch of
 *            nka_hip_batch_create_wide, a second one as a control and the binary32 batch alternated on the same inputs; nsys 16 /
 *            64 / 256 x vlen 32 768 / 65 536 / 262 144 x mvec 10 / 20, default flavour, full lists; 256 x 262 144 x 20 needs more
 *            than 40 GB and was not measured).  THE CONDITION, fixed beforehand -- at 256 x 65 536, both mvec, a - b > |a - a'| plus
 *            the largest window spread -- HELD: 0.674 (mvec 10) and 0.648 (mvec 20) of the time of the binary64 update, the two
 *            binary64 batches differing by 2.3 % and 2.6 %; the byte model of STORAGE predicts 0.69 and 0.65.  From 64 systems on
 *            0.65 ... 0.81 at every point (0.78 / 0.81 at 64 x 32 768, 0.69 / 0.65 at 64 x 262 144, 0.69 at 256 x 262 144 x 10); at
 *            16 systems 0.99 / 0.98 at 32 768, 0.86 / 0.85 at 65 536 and 0.75 / 0.77 at 262 144 (there the scalar step on one thread
 *            is a large share of a call: SCALAR STEP below); a step with x, mask, tol and fnorm at 64 x 65 536 x 20: 0.75.  Faster by more than the
 *            control's difference and the window spread at all 18 points.  One measurement.
 *   SCALAR STEP  nka_hip_batch_set_scalar_step: an OPT-IN choice of how a wide batch runs the third of its four launches -- the
 *            Gram row, the Cholesky factor with its drop decisions, both substitutions and the combine plan of a system.
 *            NKA_HIP_BATCH_SCALAR_ONE_THREAD, the default: one thread runs the reference's loops, an O(mvec^3) chain of dependent LDS
 *            round trips; a batch that never calls the setter launches exactly the kernels it always did.
 *            NKA_HIP_BATCH_SCALAR_WAVEFRONT: the same arithmetic on ONE WAVEFRONT, the way k_solve_rows does it for a lone handle
 *            -- lane p holds row p of the position-indexed Gram matrix in registers, the factorisation is right-looking, pivots and
 *            column entries travel by v_readlane, the right-hand side rides along as one more row, the back-substitution runs by
 *            columns -- in about mvec sequential steps.  Every entry receives the subtractions of the reference's inner loop in the
 *            same order and then the same division (no contraction: every a - l l_q is two roundings), and the debris is the
 *            one-thread step's too: the row of a dependence-dropped entry is stored at the kept columns ahead of it and its
 *            diagonal never, the row of the capacity-dropped entry is not touched, c of a dropped entry keeps the raw right-hand
 *            side, the drops reach the free list in list order, a NaN pivot drops, the last position of a full list is evaluated
 *            by its pivot once an entry ahead of it was dropped; without a new pair (the first update, after relax or restart, s ==
 *            0) one lane runs the one-thread statements.  So BOTH STEPS LEAVE THE SAME BITS -- f, x, fnorm, the mask, red[], all of
 *            h and c, the lists, the counters, nka_hip_batch_state_digest, every stored vector -- and SWITCHING BETWEEN CALLS CHANGES
 *            NO RESULT.  The setter is enqueue-side state: no synchronisation, no allocation (the matrix lives in dynamic LDS,
 *            13.0 KiB at mvec = 20 and 24.0 KiB at 32 with 512 chunks), no new creation entry; it applies from the next accel_update /
 *            accel_step on, and a captured call keeps the step it was captured with.  The instance is chosen from mvec (6 / 11 / 21 /
 *            33 rows), fixed at creation.  Within the launch no workgroup reads what another writes: no flags, no spinning, no
 *            atomics, no cooperative launch.  Offered by every wide batch (all five wide creation entries, both storages, with
 *            lengths, weights and the step: the third launch reads neither weights nor stored vectors); NKA_HIP_EINVAL, the batch
 *            staying usable, for any other value and for _WAVEFRONT on a narrow batch of nka_hip_batch_create / _create_stored, on a
 *            lane batch and on a wave batch of nka_hip_batch_create_waves / _create_waves_ext (_ONE_THREAD is accepted everywhere; a
 *            wave batch of nka_hip_batch_create_waves_rows accepts both, WAVES ROWS below, and so does a narrow batch of
 *            nka_hip_batch_create_rows, NARROW ROWS below; nka_hip_batch_offers_scalar_step tells them apart).
 *            MEASURED (profiles/r22/batch_wide_rows_throughput.txt, tools/batch_throughput.py --wide-rows: a one-thread batch a, a
 *            second one a' as the control, the wavefront batch b, alternated on the same inputs, windows >= 0.5 s, median of 5; nsys
 *            4 / 16 / 64 / 256 x vlen 32 768 / 65 536 / 262 144 x mvec 5 / 10 / 20 / 32, default flavour, full lists; 256 x 262 144
 *            at mvec >= 10 needs more than 40 GB and was not measured).  THE CONDITION, fixed beforehand -- at 16 x 65 536 x 20, a - b
 *            > |a - a'| plus the largest window spread -- HELD: 249.7 -> 111.4 us, b/a = 0.446 (|a - a'|/a = 0.002); the third launch
 *            itself 154.6 -> 16.8 us in a kernel trace of its own.  b/a at 16 systems: 0.89 / 0.67 / 0.33 / 0.18 at 32 768 (mvec 5 /
 *            10 / 20 / 32), 0.92 / 0.74 / 0.45 / 0.25 at 65 536, 0.96 / 0.91 / 0.72 / 0.53 at 262 144; a step with x, mask, tol and
 *            fnorm at 16 x 65 536 x 20: 0.453.  The gain shrinks as the other three launches grow: at 256 systems 0.97 / 0.92 / 0.82 /
 *            0.69 at 32 768 and 0.99 / 1.00 / 0.96 / 0.77 at 65 536.  Won (by more than the control's difference and the window
 *            spread) at 40 of the 46 measured points (the step among them), lost at none; inside the noise at 256 x 65 536 x 10 and x 20 and at 64 / 256 x 262 144 x 5,
 *            64 x 262 144 x 10 and x 20.  FOUR systems at mvec = 20, where WIDE records a loss to four lone handles: the loop over
 *            four lone handles takes 0.69 / 0.74 / 0.83 of the one-thread batch's time at 32 768 / 65 536 / 262 144 and 2.25 / 2.29 /
 *            1.76 x the wavefront batch's -- with the opt-in the batch no longer loses.  One measurement; the default stays
 *            _ONE_THREAD.  The wave batch offers the same choice through an entry of its own, WAVES ROWS below, and so
 *            does the narrow batch, whose scalar step sits inside its one kernel (its older instances held to their machine code):
 *            NARROW ROWS below.  Not covered: the lane batch keeps the one-lane step -- a follow-up.
 *   WAVES ROWS  nka_hip_batch_create_waves_rows: THE WAVE BATCH THAT OFFERS THE SCALAR STEP ON THE WHOLE WAVEFRONT
 *            (nka_amd/csrc/nka_batch_waves.hip).  In WAVES lane 0 of a system's wavefront runs the scalar step while 63 lanes wait, and
 *            from mvec = 10 on that step, not the memory traffic, is what an update costs (profiles/r15/batch_waves_throughput.txt:
 *            about 20 / 50 / 210 us at mvec 5 / 10 / 20 whatever nsys and vlen are).  A batch of this entry accepts
 *            nka_hip_batch_set_scalar_step(b, NKA_HIP_BATCH_SCALAR_WAVEFRONT): phase 4 of the one kernel then runs the device function
 *            of SCALAR STEP on all 64 lanes of the system's own wavefront, in about mvec sequential steps.  ext == 0: limits,
 *            allocations, refusals and guarantees of nka_hip_batch_create_waves; ext == 1: those of nka_hip_batch_create_waves_ext
 *            (nka_hip_batch_offers_lengths / _offers_weights return ext); any other ext: NKA_HIP_EINVAL.  nka_hip_batch_kind is 3,
 *            nka_hip_batch_offers_scalar_step 1, and nothing further is allocated: the matrix of the step lives in dynamic LDS.  The
 *            default is NKA_HIP_BATCH_SCALAR_ONE_THREAD, which here means one lane; until the setter is called with _WAVEFRONT the batch
 *            launches the kernels of the corresponding entry and is that batch bit for bit and launch for launch.  The setter is
 *            enqueue-side state only (no synchronisation, no allocation, legal while the stream is capturing), applies from the next
 *            accel_update / accel_step on, and a captured call keeps the step it was captured with -- the instance and the LDS size
 *            it asks for are chosen together when the call is enqueued.  A new entry, because the old ones must not change: a batch
 *            of nka_hip_batch_create_waves or _create_waves_ext, every lane batch and every narrow batch but one of
 *            nka_hip_batch_create_rows (NARROW ROWS below) keeps refusing _WAVEFRONT.
 *            THE CONTRACT: BOTH STEPS LEAVE THE SAME BITS, so switching between calls changes no result.  For every system, after
 *            every call: the rows of f and x, fnorm, the mask and the retirement decision, red[], all of h and c (the debris of
 *            dropped rows included), the links, the five list scalars and the counters, nka_hip_batch_state_digest, w and v of every
 *            slot are those of a one-lane wave batch of the same entry kind on the same inputs -- in all three flavours, with and
 *            without lengths and weights, on the paths without a new pair (first update, after relax or restart, s == 0), and when
 *            the system is fed NaN and Inf (tests/test_batch_waves_rows_gpu.py).  Everything WAVES guarantees stays: no workgroup barrier,
 *            no atomics, flags or spinning (the step is built from wavefront-level means only; one more wavefront-scope fence stands
 *            between lane 0's stores of the sums and the step); a masked, retired or absent system's wavefront returns on its own,
 *            before it touches LDS; graphs from the first call; a system's bits depend on its own values alone.
 *            THE CAP ON mvec IS DERIVED, NOT MEASURED: beside the working copy a system needs a matrix of (mvec + 2)^2 doubles, rounded
 *            up to 16 bytes, and four copies plus four matrices must fit the 64 KiB of dynamic LDS a launch may ask for without a
 *            function attribute: 36 672 bytes per workgroup at mvec = 20, 64 832 at 28 (fits), 68 992 at 29 (does not).  Creation with
 *            mvec above the cap is NKA_HIP_EINVAL with the cap named and nothing left allocated; nka_hip_batch_waves_rows_limits
 *            returns the cap and the bytes at an mvec, as the library was built (nka_host::waves_rows_max_mvec, a constexpr search;
 *            tests/c/batch_waves_rows_layout_check.cpp paints the layout).  mvec 29 ... 32: nka_hip_batch_create_waves.  The instance
 *            is chosen from mvec (6 / 11 / 21 / cap + 1 rows): 96 more instances of the one kernel, none with scratch or a spill, none
 *            with more registers than its one-lane twin; 1.7 x the LDS per workgroup lowers the resident wavefronts of the sweeps,
 *            which is the price the measurement weighs.
 *            MEASURED (profiles/r23/batch_waves_rows_throughput.txt, tools/batch_throughput.py --waves-rows, 1 x MI355X: a one-lane
 *            wave batch a of nka_hip_batch_create_waves, a second one a' as the control, the wavefront batch b, alternated on the
 *            same inputs, windows >= 0.5 s, median of 5; nsys 256 / 4096 / 65 536 x vlen 65 / 256 / 1024 x mvec 5 / 10 / 20 / 28,
 *            default flavour, full lists; 65 536 x 1024 at mvec >= 10 needs more than 40 GB and was not measured).  THE CONDITION,
 *            fixed beforehand -- at 4096 x 256 x 20 and at 256 x 256 x 20, a - b > |a - a'| plus the largest window spread of the
 *            three -- HELD at both: 244.1 -> 93.8 us (b/a = 0.384) and 211.1 -> 30.6 us (0.145), the two one-lane batches differing
 *            by 0.0 % and 0.3 %.  b/a at mvec 5 / 10 / 20 / 28 -- 256 systems: 0.67 / 0.39 / 0.15 / 0.09 at vlen 65, 0.64 / 0.38 /
 *            0.15 / 0.10 at 256, 0.81 / 0.61 / 0.30 / 0.19 at 1024; 4096 systems: 0.82 / 0.55 / 0.26 / 0.25 at 65, 0.90 / 0.69 / 0.38 /
 *            0.31 at 256, 0.99 / 0.98 / 0.84 / 0.67 at 1024; 65 536 systems: 0.85 / 0.62 / 0.34 / 0.31 at 65, 1.11 / 0.92 / 0.48 / 0.32
 *            at 256, 0.92 at 1024 x 5; a step with x, mask, tol and fnorm at 4096 x 256 x 10 / 20: 0.72 / 0.40.  By the same rule WON
 *            at 34 of the 35 measured points (the two steps among them), LOST at none, INSIDE THE NOISE at 65 536 x 256 x 5 (b/a =
 *            1.11 where the two one-lane batches themselves differ by 10.5 %).  The gain shrinks where the sweeps, not the step, fill
 *            the time: 4096 x 1024 at mvec 5 / 10 (0.99 / 0.98) -- there the larger LDS footprint costs what the step saves.  AGAINST
 *            THE NARROW BATCH AT 256 SYSTEMS, where WAVES records a loss everywhere (here 1.10 ... 1.81 x the narrow batch's time):
 *            with the wavefront step the wave batch takes 0.74 / 0.47 / 0.18 / 0.11 of it at vlen 65, 0.73 / 0.46 / 0.18 / 0.11 at
 *            256, and 1.47 / 1.05 / 0.42 / 0.25 at 1024 -- it no longer loses except at 256 x 1024 with mvec 5 and 10.  So: a wave
 *            batch with mvec from about 10 on, at any nsys, or with any mvec at a few hundred systems up to vlen 256 -- this entry
 *            with _WAVEFRONT; mvec 29 ... 32 -- nka_hip_batch_create_waves.  One measurement; the default stays _ONE_THREAD.
 *   NARROW ROWS  nka_hip_batch_create_rows: THE NARROW BATCH THAT OFFERS THE SCALAR STEP ON ONE WAVEFRONT (nka_amd/csrc/
 *            nka_batch_kernel.hpp, the instances of nka_amd/csrc/nka_batch_rows.hip).  The batch at the head of this file -- one
 *            workgroup per system, vlen up to 16 384, all three flavours, weights, lengths, accel_step, either storage -- runs
 *            phase 4 of its one kernel on thread 0 while 255 threads wait at a barrier: 22 / 42 / 151 us per update at mvec 5 / 10 / 20,
 *            whatever nsys is (profiles/r08/batch_throughput.txt).  A batch of this entry accepts nka_hip_batch_set_scalar_step(b,
 *            NKA_HIP_BATCH_SCALAR_WAVEFRONT): phase 4 then runs the device function of SCALAR STEP on the 64 lanes of wavefront 0 of
 *            the system's workgroup, between the same two barriers, in about mvec sequential steps; wavefronts 1 to 3 go on to the
 *            second barrier.  storage == NKA_HIP_BATCH_STORE_F64: arguments, limits, allocations, refusals and guarantees of
 *            nka_hip_batch_create; NKA_HIP_BATCH_STORE_F32: those of nka_hip_batch_create_stored (the default flavour only); any
 *            other storage: NKA_HIP_EINVAL, with this entry's name in every message.  nka_hip_batch_kind is 0,
 *            nka_hip_batch_offers_scalar_step 1, _offers_lengths, _offers_weights and _offers_step 1, and nothing further is
 *            allocated: one host flag, and the matrix of the step lives in dynamic LDS.  mvec up to NKA_HIP_BATCH_MAX_MVEC: there is
 *            no new cap.  The default is NKA_HIP_BATCH_SCALAR_ONE_THREAD; until the setter is called with _WAVEFRONT the batch
 *            launches the kernels of the corresponding entry and is that batch bit for bit and launch for launch.  The setter is
 *            enqueue-side state only (no synchronisation, no allocation, legal while the stream is capturing), applies from the next
 *            accel_update / accel_step on, and a captured call keeps the step it was captured with -- the instance and the LDS size
 *            it asks for are chosen together when the call is enqueued.  A new entry, because the old ones must not change: a batch
 *            of nka_hip_batch_create or _create_stored keeps refusing _WAVEFRONT and keeps returning 0 from _offers_scalar_step.
 *            FAST SUMS ONLY: the wavefront instances exist for the rounded fast sums.  The reference order is validation speed --
 *            n dependent additions per sum --, and systems of at most 1024 elements have nka_hip_batch_create_waves_rows.
 *            nka_hip_batch_set_scalar_step(b, _WAVEFRONT) is therefore refused with NKA_HIP_ESTATE while the batch forms its sums in
 *            the reference order (NKA_HIP_SUMS_REFERENCE_ORDER, or NKA_HIP_SUMS_AUTO at vlen <= 64), and nka_hip_batch_set_sum_order
 *            with an order that would mean the reference order is refused with NKA_HIP_ESTATE while _WAVEFRONT is set; each message
 *            names the other setter and nka_hip_batch_create_waves_rows, the batch stays usable and both settings stay as they were.
 *            A binary32 batch always runs the fast sums, at every vlen.  So nothing is silently downgraded: a call runs the step
 *            and the sum order the two getters report.
 *            THE CONTRACT: BOTH STEPS LEAVE THE SAME BITS, so switching between calls changes no result.  For every system, after
 *            every call: the rows of f and x, fnorm, the mask and the retirement decision, red[], all of h and c (the debris of
 *            dropped rows included), the links, the five list scalars and the counters, nka_hip_batch_state_digest, w and v of every
 *            slot are those of the one-thread step on the same inputs -- in all three flavours, with weights (a row per system or
 *            the shared row), lengths, accel_step and binary32 storage in any combination, on the paths without a new pair (first
 *            update, after relax or restart, s == 0), and when the system is fed NaN and Inf (tests/test_batch_rows_gpu.py).
 *            Everything the batch guarantees stays: within the launch no workgroup reads what another writes, no flags, no
 *            spinning, no atomics, no cooperative launch (the step is built from wavefront-level means only, and the two workgroup
 *            barriers around phase 4 are the ones that were there); MASKS, ASYNC, GRAPHS from the first call, BITS.
 *            LDS: the working copy at the offsets it has in every other instance, and behind it, on the next multiple of 16 bytes,
 *            the matrix of (mvec + 2)^2 doubles -- 9 168 bytes per workgroup at mvec = 20 (5 296 without the matrix), 20 496 at 32
 *            (11 248): at most 40 KiB, so four workgroups still share a CU by LDS, and no function attribute is needed.
 *            nka_hip_batch_rows_limits returns the bytes at an mvec, as the library was built (nka_host::batch_rows_lds;
 *            tests/c/batch_rows_layout_check.cpp paints the layout).  The instance is chosen from mvec (11 / 21 / 33 rows; the
 *            11-row instance serves the short lists, where a 6-row instance gave the wide and the wave batch 0.86 ... 0.99): 96 more
 *            instances of the one kernel body -- 32 fast packs x 3, a unit of their own --, none with scratch or a vector-register
 *            spill, 90 to 99 VGPR each, the 33-row instances included (at least four wavefronts per SIMD, as their one-thread
 *            twins have), every older instance unchanged instruction for instruction.
 *            MEASURED (profiles/r24/batch_rows_throughput.txt, tools/batch_throughput.py --rows, 1 x MI355X: a one-thread batch a of
 *            this entry, a second one a' as the control, the wavefront batch b, alternated on the same inputs, windows >= 0.5 s,
 *            median of 5; nsys 16 / 256 / 4096 x vlen 256 / 1024 / 4096 / 16 384 x mvec 5 / 10 / 20 / 32, default flavour, full lists;
 *            4096 x 16 384 at mvec >= 10 needs more than 40 GB and was not measured).  THE CONDITION, fixed beforehand -- at 256 x
 *            4096 x 20, a - b > |a - a'| plus the largest window spread of the three -- HELD: 238.8 -> 106.2 us, b/a = 0.445 (|a -
 *            a'|/a = 0.001); the kernel itself 234.0 -> 100.9 us in a kernel trace of its own.  b/a at mvec 5 / 10 / 20 / 32 -- 16
 *            systems: 0.80 / 0.45 / 0.18 / 0.08 at vlen 256, 0.80 / 0.47 / 0.18 / 0.09 at 1024, 0.89 / 0.62 / 0.29 / 0.17 at 4096,
 *            0.96 / 0.87 / 0.62 / 0.39 at 16 384; 256 systems: 0.80 / 0.46 / 0.18 / 0.09, 0.87 / 0.52 / 0.21 / 0.10, 0.92 / 0.74 /
 *            0.45 / 0.24, 0.95 / 0.91 / 0.72 / 0.54; 4096 systems, sixteen workgroups to a CU: 0.84 / 0.51 / 0.24 / 0.12, 0.90 /
 *            0.70 / 0.40 / 0.20, 0.98 / 0.94 / 0.82 / 0.59, and 0.92 at 16 384 x 5.  By the same rule WON at all 45 measured
 *            points, LOST at none, none inside the noise (the two one-thread batches differ by at most 4.0 %).  At 16 systems of 256
 *            unknowns 17.8 / 40.9 / 163.1 / 525.4 us per update become 14.2 / 18.6 / 28.9 / 44.3.  The gain shrinks where the sweeps, not the step, fill the time -- 4096 x 4096 x 5: 0.98 -- and was not known
 *            beforehand for launches in which several workgroups share a CU: at 4096 systems it is 0.12 ... 0.98.  AGAINST THE
 *            WAVE BATCH of nka_hip_batch_create_waves_rows with _WAVEFRONT (b/w, vlen <= 1024, mvec <= 28, recorded without a bar):
 *            at vlen 256 level at 16 and 256 systems from mvec 10 on (0.98 ... 1.01; 1.12 / 1.13 at mvec 5) and 1.9 ... 2.1 at 4096
 *            systems, where four systems share a workgroup there; at vlen 1024 0.50 ... 0.62 at 16 and 256 systems and level (0.99 ...
 *            1.01) at 4096.  So: mvec from about 10 on, or a few hundred systems and fewer at any mvec -- this entry with
 *            _WAVEFRONT, at every vlen up to 16 384; thousands of systems of at most 256 unknowns -- WAVES ROWS.  One measurement;
 *            the default stays _ONE_THREAD.
 *   OUT OF SCOPE  per-system mvec or vtol, an automatic restart on a length change, sharding and all-reduce hooks, the user dot product, a per-call weight argument, the out-of-place entry,
 *            the abstract-vector path and Fortran bindings: the reference has no batched type to mirror.  A caller who needs
 *            any of these uses lone handles.
 */
#ifndef NKA_HIP_BATCH_H
#define NKA_HIP_BATCH_H

#include <stdint.h>

#include "nka_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nka_hip_batch_state *nka_hip_batch_t;

enum { NKA_HIP_BATCH_MAX_VLEN = 16384, NKA_HIP_BATCH_MAX_MVEC = 32 };
/* WIDE above: elements per workgroup of a wide batch, and its longest system */
enum { NKA_HIP_BATCH_WIDE_CHUNK = 2048, NKA_HIP_BATCH_WIDE_MAX_VLEN = 1048576 };

/* nsys accelerators of vlen elements and at most mvec vectors each, all restarted (F08:185-200 per system); `device` and
 * `stream` as in nka_hip_create.  Allocates 2*nsys*(mvec+1) slot vectors (slot stride: vlen rounded up to 32 doubles). */
int nka_hip_batch_create(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                         int32_t flavor, int32_t device, void *stream);
/* WIDE above: the same handle type with every system split across ceil(vlen / NKA_HIP_BATCH_WIDE_CHUNK) workgroups;
 * 1 <= vlen <= NKA_HIP_BATCH_WIDE_MAX_VLEN, nsys <= 65535, mvec and vtol as above.  Allocates the partial sums beside the slots. */
int nka_hip_batch_create_wide(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                              int32_t flavor, int32_t device, void *stream);
/* WIDE above, STEP of a wide batch: nka_hip_batch_create_wide with one more buffer (nsys * nchunk doubles), the only wide batch
 * that offers nka_hip_batch_accel_step.  _offers_step: 1 = accel_step is offered (narrow, lanes, waves, and a wide batch of
 * this entry), 0 = refused (a wide batch of nka_hip_batch_create_wide); < 0 on error. */
int nka_hip_batch_create_wide_step(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                                   int32_t flavor, int32_t device, void *stream);
int nka_hip_batch_offers_step(nka_hip_batch_t b);
/* STORAGE above: how the normalised subspace vectors are kept.  _create_stored with NKA_HIP_BATCH_STORE_F64 is
 * nka_hip_batch_create; with NKA_HIP_BATCH_STORE_F32 it allocates 2*nsys*(mvec+1) slot vectors of binary32 elements at the same
 * stride in elements and two pending buffers of nsys*stride doubles (zero-initialised, freed by destroy only, never moved), and
 * refuses every flavour but NKA_HIP_FLAVOR_C (NKA_HIP_EINVAL, nothing left allocated).  Any other storage: NKA_HIP_EINVAL.
 * _storage: the value the batch was created with; < 0 on error.  _vector_bytes: the bytes of device memory the batch allocated
 * for its stored vectors (slots and pending buffers); < 0 on error. */
enum { NKA_HIP_BATCH_STORE_F64 = 0, NKA_HIP_BATCH_STORE_F32 = 1 };
int nka_hip_batch_create_stored(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                                int32_t flavor, int32_t device, void *stream, int32_t storage);
int nka_hip_batch_storage(nka_hip_batch_t b);
int64_t nka_hip_batch_vector_bytes(nka_hip_batch_t b);
/* LANES above: the same handle type with ONE LANE PER SYSTEM; 1 <= vlen <= NKA_HIP_BATCH_LANES_MAX_VLEN, mvec, vtol and the three
 * flavours as above, nsys >= 1.  Allocates the slots interleaved across the systems of a group (binary64 only).
 * _lanes_limits: how many systems one workgroup advances at this mvec, as the library was built, and the cap on vlen (either
 * output may be NULL); NKA_HIP_EINVAL for an mvec outside 1 ... NKA_HIP_BATCH_MAX_MVEC.
 * _kind: 0 = one workgroup per system (narrow), 1 = wide, 2 = lanes; < 0 on error. */
enum { NKA_HIP_BATCH_LANES_MAX_VLEN = 64 };
enum { NKA_HIP_BATCH_KIND_NARROW = 0, NKA_HIP_BATCH_KIND_WIDE = 1, NKA_HIP_BATCH_KIND_LANES = 2 };
int nka_hip_batch_create_lanes(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                               int32_t flavor, int32_t device, void *stream);
int nka_hip_batch_lanes_limits(int32_t mvec, int32_t *systems_per_group, int64_t *max_vlen);
int nka_hip_batch_kind(nka_hip_batch_t b);
/* WAVES above: the same handle type with ONE WAVEFRONT PER SYSTEM, four systems per workgroup; 1 <= vlen <=
 * NKA_HIP_BATCH_WAVES_MAX_VLEN, mvec, vtol and the three flavours as above, nsys >= 1.  Allocates what nka_hip_batch_create
 * allocates and nothing more (binary64 only).  _waves_limits: the systems one workgroup advances (4) and the cap on vlen, as the
 * library was built (either output may be NULL).  _kind returns 3 for such a batch. */
enum { NKA_HIP_BATCH_WAVES_MAX_VLEN = 1024 };
enum { NKA_HIP_BATCH_KIND_WAVES = 3 };
int nka_hip_batch_create_waves(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                               int32_t flavor, int32_t device, void *stream);
int nka_hip_batch_waves_limits(int32_t *systems_per_group, int64_t *max_vlen);
/* WAVES EXT above: nka_hip_batch_create_waves with nka_hip_batch_set_lengths / _host and nka_hip_batch_set_dot_weights / _host
 * offered; arguments, limits, allocations and _kind (3) as for nka_hip_batch_create_waves.
 * _offers_lengths / _offers_weights: 1 = the setters are offered, 0 = refused; < 0 on error (a NULL handle).  Lengths: every kind
 * but lanes and a batch of nka_hip_batch_create_waves; weights: narrow (either storage), a batch of this entry and a wide batch of
 * nka_hip_batch_create_wide_ext. */
int nka_hip_batch_create_waves_ext(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                                   int32_t flavor, int32_t device, void *stream);
int nka_hip_batch_offers_lengths(nka_hip_batch_t b);
int nka_hip_batch_offers_weights(nka_hip_batch_t b);
/* WAVES ROWS above: a wave batch that offers nka_hip_batch_set_scalar_step(b, NKA_HIP_BATCH_SCALAR_WAVEFRONT).  ext == 0: arguments,
 * limits, allocations, refusals and guarantees of nka_hip_batch_create_waves; ext == 1: those of nka_hip_batch_create_waves_ext
 * (_offers_lengths and _offers_weights return ext); any other ext: NKA_HIP_EINVAL.  mvec above the cap of _waves_rows_limits:
 * NKA_HIP_EINVAL, nothing left allocated.  _kind 3; nothing further is allocated.  Until the setter is called with _WAVEFRONT the
 * batch launches the kernels of the corresponding entry and is that batch bit for bit and launch for launch.
 * _waves_rows_limits: the cap on mvec -- the largest whose four working copies and four matrices fit 64 KiB of LDS, as the library
 * was built -- and the LDS bytes of one workgroup at `mvec` (either output may be NULL); NKA_HIP_EINVAL for an mvec outside 1 ... cap. */
int nka_hip_batch_create_waves_rows(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                                    int32_t flavor, int32_t device, void *stream, int32_t ext);
int nka_hip_batch_waves_rows_limits(int32_t *max_mvec, int32_t mvec, int64_t *lds_bytes);
/* NARROW ROWS above: a narrow batch (one workgroup per system) that offers nka_hip_batch_set_scalar_step(b,
 * NKA_HIP_BATCH_SCALAR_WAVEFRONT).  storage == NKA_HIP_BATCH_STORE_F64: arguments, limits, allocations, refusals and guarantees of
 * nka_hip_batch_create; NKA_HIP_BATCH_STORE_F32: those of nka_hip_batch_create_stored; any other storage: NKA_HIP_EINVAL.  _kind 0;
 * nothing further is allocated; mvec up to NKA_HIP_BATCH_MAX_MVEC.  Until the setter is called with _WAVEFRONT the batch launches the
 * kernels of the corresponding entry and is that batch bit for bit and launch for launch.  The wavefront step runs with the fast sums
 * only: NKA_HIP_ESTATE from the setter while the batch forms its sums in the reference order, and from nka_hip_batch_set_sum_order
 * for such an order while _WAVEFRONT is set.
 * _rows_limits: the dynamic LDS of a wavefront-step launch at `mvec`, as the library was built (lds_bytes may be NULL);
 * NKA_HIP_EINVAL for an mvec outside 1 ... NKA_HIP_BATCH_MAX_MVEC. */
int nka_hip_batch_create_rows(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                              int32_t flavor, int32_t device, void *stream, int32_t storage);
int nka_hip_batch_rows_limits(int32_t mvec, int64_t *lds_bytes);
/* WIDE EXT above: the wide batch with nka_hip_batch_set_dot_weights / _host offered.  step == 0: arguments, limits, allocations and
 * guarantees of nka_hip_batch_create_wide; step == 1: those of nka_hip_batch_create_wide_step; any other step: NKA_HIP_EINVAL.
 * _kind 1, _is_wide 1, _offers_lengths 1, _offers_weights 1, _offers_step = step. */
int nka_hip_batch_create_wide_ext(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                                  int32_t flavor, int32_t device, void *stream, int32_t step);
/* WIDE STORED above: the wide batch with a choice of storage.  storage == NKA_HIP_BATCH_STORE_F64: nka_hip_batch_create_wide_ext(...,
 * step), bit for bit and launch for launch.  storage == NKA_HIP_BATCH_STORE_F32: the limits of nka_hip_batch_create_wide, step 0 or 1
 * as in nka_hip_batch_create_wide_ext, 2*nsys*(mvec+1) slot vectors of binary32 elements at the wide batch's slot stride and two
 * pending buffers of nsys*stride doubles (zero-initialised, freed by destroy only, never moved); _kind 1, _is_wide 1, _offers_lengths
 * 1, _offers_weights 1, _offers_step = step, _storage NKA_HIP_BATCH_STORE_F32.  NKA_HIP_EINVAL, nothing left allocated: every flavour
 * but NKA_HIP_FLAVOR_C with binary32, any other storage, any other step, the wide limits. */
int nka_hip_batch_create_wide_stored(nka_hip_batch_t *out, int32_t nsys, int64_t vlen, int32_t mvec, double vtol,
                                     int32_t flavor, int32_t device, void *stream, int32_t step, int32_t storage);
int nka_hip_batch_is_wide(nka_hip_batch_t b);                    /* 1 = wide, 0 = narrow, lanes or waves; < 0 on error */
int nka_hip_batch_wide_limits(int64_t *chunk, int64_t *max_vlen);  /* the two constants, as the library was built */
int nka_hip_batch_destroy(nka_hip_batch_t b);

/* call a%accel_update(f) for every active system, one launch.  Rows of inactive systems are not touched. */
int nka_hip_batch_accel_update(nka_hip_batch_t b, double *f_dev, int64_t ld, const int32_t *active_dev);
/* STEP above: norm, stop rule, update and correction of every active system, one launch (a wide batch of
 * nka_hip_batch_create_wide_step: four).  x_dev (iterate rows, ldx apart),
 * active_dev (READ AND WRITTEN), tol_dev (nsys thresholds) and fnorm_dev (nsys doubles out) may each be NULL. */
int nka_hip_batch_accel_step(nka_hip_batch_t b, double *f_dev, int64_t ld, double *x_dev, int64_t ldx, int32_t *active_dev,
                             const double *tol_dev, double *fnorm_dev);
/* call a%restart() / a%relax() for every active system (F08:422-457). */
int nka_hip_batch_restart(nka_hip_batch_t b, const int32_t *active_dev);
int nka_hip_batch_relax(nka_hip_batch_t b, const int32_t *active_dev);
/* call a%set_vec_tol(vtol) for ALL systems (F08:202-207); stream-ordered like the updates around it. */
int nka_hip_batch_set_vec_tol(nka_hip_batch_t b, double vtol);
int nka_hip_batch_set_sum_order(nka_hip_batch_t b, int32_t order);
/* SCALAR STEP, WAVES ROWS and NARROW ROWS above: how a wide batch runs the third launch of an update or step, and a wave batch of
 * nka_hip_batch_create_waves_rows and a narrow batch of nka_hip_batch_create_rows phase 4 of their one launch.  _set_scalar_step changes enqueue-side state only
 * (no synchronisation, no allocation, legal while the stream is capturing) and applies from the next accel_update / accel_step on; a
 * captured call keeps the step it was captured with.  Both steps leave the same bits, so switching between calls changes no
 * result.  NKA_HIP_EINVAL, the batch staying usable and its setting unchanged: any value but the two below; _WAVEFRONT on a batch
 * that does not offer it (_ONE_THREAD is accepted by every batch).  NKA_HIP_ESTATE, likewise: _WAVEFRONT on a narrow batch of
 * nka_hip_batch_create_rows while it forms its sums in the reference order (NARROW ROWS above).  _scalar_step: the value the next
 * call runs with (default _ONE_THREAD); < 0 on error.  _offers_scalar_step: 1 = every wide batch (all five wide creation entries,
 * both storages), a wave batch of nka_hip_batch_create_waves_rows (ext 0 or 1) and a narrow batch of nka_hip_batch_create_rows
 * (either storage); 0 = a narrow batch of nka_hip_batch_create or _create_stored, lanes, and a wave batch of
 * nka_hip_batch_create_waves or _create_waves_ext; < 0 on error. */
enum { NKA_HIP_BATCH_SCALAR_ONE_THREAD = 0, NKA_HIP_BATCH_SCALAR_WAVEFRONT = 1 };
int nka_hip_batch_set_scalar_step(nka_hip_batch_t b, int32_t how);
int nka_hip_batch_scalar_step(nka_hip_batch_t b);
int nka_hip_batch_offers_scalar_step(nka_hip_batch_t b);
/* DIAGONAL WEIGHTS (WEIGHTS above), as nka_hip_set_dot_weights of a lone handle, per system:
 *   ldw >= vlen  nsys rows of ldw doubles, row `sys` weights system `sys`; what lies between two rows is never read
 *   ldw == 0     ONE row of vlen doubles that all systems share
 *   other ldw    NKA_HIP_EINVAL
 *   w == NULL    plain sums again (ldw is ignored)
 * _set_dot_weights takes device memory -- its span, (nsys-1)*ldw + vlen doubles for rows and vlen for the shared row, is
 * checked against its allocation before any read --, _set_dot_weights_host host memory.  The values are COPIED into a buffer
 * of the batch and checked on the device row by row: every weight must be finite and >= 0, otherwise NKA_HIP_EINVAL and the
 * previous weighting stays in force.  The call synchronises, and the caller's memory is free again when it returns; it is
 * refused with NKA_HIP_ESTATE while the batch's stream is capturing.  A change applies from the next update on and to ALL
 * systems (there is no mask); the subspaces then mix two metrics, so follow it with nka_hip_batch_restart.
 * The buffer -- nsys rows at the slot stride, so every row is 16-byte aligned -- is allocated at the FIRST set, freed by
 * nka_hip_batch_destroy only, and never moves; it serves both forms (the shared form writes row 0 and runs with row stride
 * 0).  Whether an update is weighted, the buffer's address and the row stride are arguments of its launch: a captured update
 * keeps whether it was weighted and which form it ran, and reads the buffer's VALUES at replay, so new values of the same
 * form set between replays apply to the next replay.
 * nka_hip_batch_dot_weighted: 1 = the next update is weighted, 0 = plain; < 0 on error. */
int nka_hip_batch_set_dot_weights(nka_hip_batch_t b, const double *w_dev, int64_t ldw);
int nka_hip_batch_set_dot_weights_host(nka_hip_batch_t b, const double *w_host, int64_t ldw);
int nka_hip_batch_dot_weighted(nka_hip_batch_t b);
/* PER-SYSTEM LENGTHS (LENGTHS above), on the model of nka_hip_batch_set_dot_weights: nsys int32, 1 <= len[sys] <= vlen.
 * _set_lengths takes device memory -- its span, nsys entries, is checked against its allocation before any read --,
 * _set_lengths_host host memory; NULL makes all systems vlen long again.  The values are COPIED into a buffer of the batch and
 * VALIDATED BEFORE THEY GET THERE (the device entry stages its span on the host): any length outside 1 ... vlen -- 0 included --
 * returns NKA_HIP_EINVAL and the previous lengths stay in force, so no update kernel ever reads a length that did not pass.
 * The call synchronises, and the caller's memory is free again when it returns; it is refused with NKA_HIP_ESTATE while the
 * batch's stream is capturing.  A change applies from the next update on; the stored vectors of a system whose length changed
 * hold a tail of the other length, so follow it with nka_hip_batch_restart for those systems (there is no automatic restart).
 * The buffer is allocated at the FIRST set, freed by nka_hip_batch_destroy only, and never moves.  Whether an update runs with
 * lengths, and the buffer's address, are arguments of its launch -- the kernel instance and a pointer appended after the
 * existing arguments --: a captured update keeps whether it had lengths and reads the buffer's VALUES at replay, so new lengths
 * set between replays apply to the next replay (NULL writes vlen into every entry for such a replay).
 * _get_lengths: nsys int32 to host memory, vlen everywhere while none are set.  _has_lengths: 1 / 0; < 0 on error. */
int nka_hip_batch_set_lengths(nka_hip_batch_t b, const int32_t *len_dev);
int nka_hip_batch_set_lengths_host(nka_hip_batch_t b, const int32_t *len_host);
int nka_hip_batch_get_lengths(nka_hip_batch_t b, int32_t *len_host);
int nka_hip_batch_has_lengths(nka_hip_batch_t b);
/* Rebind to another hipStream_t; work already enqueued stays ordered before. */
int nka_hip_batch_set_stream(nka_hip_batch_t b, void *stream);

/* ---- queries (synchronise the stream) ---- */
int nka_hip_batch_num_vec(nka_hip_batch_t b, int32_t *num_vec_host /* nsys */);
int nka_hip_batch_flavor(nka_hip_batch_t b);   /* NKA_HIP_FLAVOR_* the batch runs (DEFAULT resolved); < 0 on error */
/* System `sys` (0-based) as nka_hip_get_state / _get_reductions / _get_w / _get_v / nka_hip_state_digest report a lone
 * handle (nka_hip_ext.h), with ONE DIFFERENCE in the reductions: a batched update REWRITES ALL 2 + 2*mvec entries of red[],
 * with zero wherever it formed no sum (no pending pair: red[0]; s == 0 or no pending pair: red[1], red[2+p]; beyond the
 * list: red[2+p], red[2+mvec+p]), whereas a lone handle leaves such entries as an earlier update wrote them.  The entries an
 * update does form carry the lone handle's bits with reference-order sums.  red[1] and red[2+p] are the sums on the
 * NORMALISED difference, <f,w1'> and <w1',w_p>, in both sum orders. */
int nka_hip_batch_get_state(nka_hip_batch_t b, int32_t sys, int32_t *subspace, int32_t *pending, int32_t *first,
                            int32_t *last, int32_t *free_, int32_t *next, int32_t *prev, double *h, double *c);
int nka_hip_batch_get_reductions(nka_hip_batch_t b, int32_t sys, double *red_out);
int nka_hip_batch_get_w(nka_hip_batch_t b, int32_t sys, int32_t slot, double *host_out);
int nka_hip_batch_get_v(nka_hip_batch_t b, int32_t sys, int32_t slot, double *host_out);
int nka_hip_batch_state_digest(nka_hip_batch_t b, int32_t sys, uint64_t *digest);

#ifdef __cplusplus
}
#endif
#endif /* NKA_HIP_BATCH_H */
