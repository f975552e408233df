"""The shapes of the large-offset tests of the batched accelerator (tests/test_batch_large_gpu.py, test_batch_large_cpu.py), as
arithmetic.  No GPU here.

A batch lays system `sys` at  sys * stride_of_the_stream  elements from the start of each of its streams (include/
nka_hip_batch.h, LAYOUT; nka_amd/csrc/host_logic.hpp, batch_layout):

  w, v    the slots: (mvec + 1) slots per system, a slot every `stride` = vlen rounded up to 32 doubles; sys_stride = (mvec + 1) stride
  F, X    the caller's rows, ld and ldx apart
  wgt     the batch's own weight buffer: one row per system at the slot stride
  wsrc    the caller's weight rows, ldw apart

Two boundaries matter to an offset that lost its upper half: 2^32 BYTES (2^29 doubles; a 32-bit byte offset) and 2^31 ELEMENTS
(a signed 32-bit index; 16 GiB).  A shape names the (stream, boundary) pairs it crosses; everything else -- the system that
straddles a boundary, the few systems that run (the rest are masked out, which costs nothing: no byte of a masked system is
read or written), the witnesses where a wrapped write would have landed, the bytes of every allocation -- is derived here and
held by tests/test_batch_large_cpu.py."""
from collections import namedtuple

BYTES_4G = 2 ** 29      # 2^32 bytes, in doubles
ELEMS_2G = 2 ** 31      # 2^31 elements
BOUNDARIES = {"2^32 bytes": BYTES_4G, "2^31 elements": ELEMS_2G}
MAX_ACTIVE = 9
MAX_BYTES = 36 * 2 ** 30
NEAR = 3                # a boundary is flanked by active systems at most this many systems away from the one on it
WIDE_CHUNK = 2048       # NKA_HIP_BATCH_WIDE_CHUNK as the header freezes it (the GPU test asserts the library agrees)
PAD = 7.25              # what every element of F and X holds that no active system owns

Shape = namedtuple("Shape", "id kind vlen mvec nsys ld ldx ldw weighted with_x crosses")

# crosses: the (stream, boundary) pairs the shape is there for
SHAPES = {s.id: s for s in (
    Shape("bytes", "narrow", 16384, 1, 32800, 16385, 16387, 16384, True, True,
          (("w", "2^32 bytes"), ("F", "2^32 bytes"), ("X", "2^32 bytes"), ("wgt", "2^32 bytes"), ("wsrc", "2^32 bytes"))),
    Shape("slots", "narrow", 16384, 32, 3976, 16384, None, None, False, False,
          (("w", "2^32 bytes"), ("w", "2^31 elements"))),
    Shape("rows", "narrow", 4099, 3, 2052, 2 ** 20 - 1, 2 ** 20 - 2, None, False, True,
          (("F", "2^32 bytes"), ("X", "2^32 bytes"), ("F", "2^31 elements"), ("X", "2^31 elements"))),
    Shape("wsrc", "narrow", 4099, 3, 2052, 4099, None, 2 ** 20 - 1, True, False,
          (("wsrc", "2^32 bytes"), ("wsrc", "2^31 elements"))),
    Shape("wide-slots", "wide", 4609, 32, 14030, 4609, None, None, False, False,
          (("w", "2^32 bytes"), ("w", "2^31 elements"))),
    Shape("wide-rows", "wide", 4609, 3, 2052, 2 ** 20 - 1, None, None, False, False,
          (("F", "2^32 bytes"), ("F", "2^31 elements"))),
)}


def slot_stride(vlen):
    return (vlen + 31) // 32 * 32


def sys_stride(sh):
    return (sh.mvec + 1) * slot_stride(sh.vlen)


def nchunk(sh):
    return -(-sh.vlen // WIDE_CHUNK) if sh.kind == "wide" else 1


def streams(sh):
    """{stream: (elements between two systems, elements of one system)} of the streams the shape has.  v lies like w."""
    out = {"w": (sys_stride(sh), sys_stride(sh)), "F": (sh.ld, sh.vlen)}
    if sh.with_x:
        out["X"] = (sh.ldx, sh.vlen)
    if sh.weighted:
        out["wgt"] = (slot_stride(sh.vlen), sh.vlen)
        out["wsrc"] = (sh.ldw, sh.vlen)
    return out


def span(sh, stream):
    """Elements from the start of the stream to the end of its last system."""
    step, own = streams(sh)[stream]
    return (sh.nsys - 1) * step + own


def extent(sh, stream, k):
    """[start, end) of system k in the stream, in elements."""
    step, own = streams(sh)[stream]
    return k * step, k * step + own


def on_boundary(sh, stream, B):
    """The system whose span straddles element B of the stream (start < B < end), or the first one that starts at or above
    B if none straddles; None if the stream ends at or below B."""
    if span(sh, stream) <= B:
        return None
    step, own = streams(sh)[stream]
    k = B // step
    if k * step < B < k * step + own:
        return k
    k = -(-B // step)
    return k if k < sh.nsys else None


def straddles(sh, stream, B, k):
    lo, hi = extent(sh, stream, k)
    return lo < B < hi


def crossings(sh):
    """[(stream, boundary name, B, k)] for every pair the shape claims AND every other boundary one of its streams crosses."""
    out = []
    for name, B in BOUNDARIES.items():
        for stream in streams(sh):
            k = on_boundary(sh, stream, B)
            if k is not None:
                out.append((stream, name, B, k))
    return out


def _flanked(sh, stream, B, k, have, below):
    """Does `have` hold a system within NEAR of k that lies wholly below B (ends at or below it), or wholly at or above it?"""
    for j in have:
        lo, hi = extent(sh, stream, j)
        if abs(j - k) <= NEAR and (hi <= B if below else lo >= B):
            return True
    return False


def active_set(sh):
    """The systems that run: system 0, the last one, the system on every boundary a stream crosses, and -- unless an active
    system within NEAR of it already lies wholly on that side -- its neighbour below and above.  (A system that STARTS on the
    boundary is itself the first one above.)  Sorted."""
    cr = crossings(sh)
    have = {0, sh.nsys - 1} | {k for _, _, _, k in cr}
    for stream, _, B, k in cr:
        for below in (True, False):
            if not _flanked(sh, stream, B, k, have, below):
                j = k - 1 if below else k + 1
                assert 0 <= j < sh.nsys, (sh.id, stream, B, k)
                have.add(j)
    return sorted(have)


def witnesses(sh):
    """Systems that never run and where an offset that lost its upper bits would have landed: the inactive neighbours k +- 1
    of every active k, and the systems that hold element (k sys_stride) mod 2^32 and byte (8 k sys_stride) mod 2^32 of the slot
    streams.  Sorted; none is active."""
    act = set(active_set(sh))
    ss = sys_stride(sh)
    out = set()
    for k in act:
        cand = [k - 1, k + 1, (k * ss) % 2 ** 32 // ss, (k * ss * 8) % 2 ** 32 // 8 // ss]
        out |= {j for j in cand if 0 <= j < sh.nsys and j not in act}
    return sorted(out)


def allocations(sh):
    """{name: bytes} of every device allocation the GPU test of the shape holds at once: the batch's own (w, v, the control
    blocks, the partial sums and the combine plan of a wide batch, the weight buffer) and the caller's (F, X, the weight rows,
    the per-system mask, tol and fnorm).  The twin of a handful of systems is left out."""
    m1 = sh.mvec + 1
    m1p = m1 + 32                                        # nka_ctl.hpp: m1p(), ic_count() and dc_count()
    ic = 16 + 2 * (m1 + 1) + 2 * m1p
    dc = 2 + (m1 + 1) ** 2 + (m1 + 1) + m1p + (2 + 2 * sh.mvec) + 16
    out = {"w": 8 * sys_stride(sh) * sh.nsys, "v": 8 * sys_stride(sh) * sh.nsys,
           "ic": 4 * ((ic + 31) // 32 * 32) * sh.nsys, "dc": 8 * ((dc + 31) // 32 * 32) * sh.nsys,
           "F": 8 * span(sh, "F"), "per system": (4 + 8 + 8 + 4) * sh.nsys}
    if sh.kind == "wide":
        out["part"] = 8 * sh.nsys * (2 + 2 * sh.mvec) * nchunk(sh)
        out["plan"] = (8 + 4) * sh.nsys * m1
    if sh.with_x:
        out["X"] = 8 * span(sh, "X")
    if sh.weighted:
        out["wgt"] = 8 * span(sh, "wgt")
        out["wsrc"] = 8 * span(sh, "wsrc")
    return out


def batch_bytes(sh):
    """What the batch itself allocates (hipMalloc of the library, which torch's counters do not see)."""
    return sum(v for k, v in allocations(sh).items() if k in ("w", "v", "ic", "dc", "part", "plan", "wgt"))


def total_bytes(sh):
    return sum(allocations(sh).values())


def lengths(sh, active):
    """Per-system lengths of the second pass: vlen on every inactive system; on the active ones vlen, vlen - 1, 513 and, for a
    wide batch, 2 C + 1 and C + 513 first, then lengths that end in every chunk in turn (none too short to hold mvec = 32
    independent vectors; the sixth, which is the system on 2^31 elements in every wide shape, runs vlen - 1).  -> nsys ints."""
    C = WIDE_CHUNK
    pool = [sh.vlen, 2 * C + 1, C + 513, C, 513, sh.vlen - 1, 2 * C, C + 1, 2 * C - 1] if sh.kind == "wide" else \
           [sh.vlen, sh.vlen - 1, 513, 1, 4097, 512, sh.vlen - 31, 65, 1025]
    pool = [min(p, sh.vlen) for p in pool]
    out = [sh.vlen] * sh.nsys
    for j, k in enumerate(active):
        out[k] = pool[j % len(pool)]
    return out
