"""Plan hazard audit: what every ``idh_op`` reads and writes, derived from the descriptor alone, and the hazards of a scheduled op list.

``idh_schedule_ops`` reorders a plan by dependency level and marks launch groups from the (buffer id, c0, c1) regions each plan builder
(``nhwc.Plan`` and csrc/networks.hip) records by hand next to the pointers it puts into the op.  This module knows nothing of those regions:
``footprints`` computes the floats an op touches from the op's own fields (geometry of include/idh_ops.h, as tests/conv_op_ref.py and
tests/op_kind_ref.py encode it), ``conflict`` decides exactly whether two footprints share a float, and ``audit`` walks a scheduled list for

  order        a conflicting pair (read after write, write after write, write after read) whose later-built op is scheduled first
  concurrency  a conflicting pair inside one launch group (a run of consecutive ops with one non-zero ``group`` in one segment: the runs
               csrc/conv.hip gather_run / run_nchw_to_nhwc merge into one grid; kMaxGroup and the workgroup caps that split a run are
               ignored, which over-reports)
  internal     an op whose own writes conflict with its own reads (no kind works in place)
  containment  a footprint outside the workspace / the weight blob / the tensors the caller declared

A missing region is found as such, whether or not the race it allows would have been lost on a given run.  tests/test_plan_audit_gpu.py
holds ``footprints`` against the kernels (NaN outside the predicted reads changes no bit, the floats written are exactly the predicted ones).

Units: a footprint counts in floats; ``base`` is the op's pointer / 4.  Pure Python + numpy; the weight extents come from the library's own
size functions (``idh_packed_weight_floats`` ...), which are host code.
"""
import numpy as np

OP_CONV, OP_UPSAMPLE2, OP_IMPORT, OP_EXPORT, OP_HEAD, OP_INSTNORM, OP_NEAREST, OP_COPY, OP_PW_NCHW, OP_PW_UP, OP_STEM = 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12
KIND_NAMES = {1: "CONV", 2: "UPSAMPLE2", 3: "NCHW_TO_NHWC", 4: "NHWC_TO_NCHW", 6: "POINTWISE_HEAD", 7: "INSTNORM", 8: "UPSAMPLE2_NEAREST", 9: "COPY",
              10: "POINTWISE_NCHW", 11: "POINTWISE_UP", 12: "STEM"}
TILE_SPLIT, TILE_WINO, TILE_WINO4 = 11, 12, 13  # IDH_SPLIT_F16X3, IDH_TILE_WINO, IDH_TILE_WINO4
INSTNORM_CHUNK = 1024  # pixels per chunk of the statistics pass (include/idh_ops.h: ceil(HW / 1024))

ACTIVATION, WEIGHT = "activation", "weight"


def ceil16(v):
    return (v + 15) & ~15


class Footprint:
    """The floats {base + p * cs + c : 0 <= p < pixels, c_lo <= c < c_hi} (strided), or the range [base, base + pixels) (dense: cs == 1).
    ``what`` names the descriptor field; ``role`` tells weights and biases (blob) from activations; ``scratch``: a workspace the op writes
    and reads back itself (split-K partials, InstanceNorm partials and statistics) - listed with the writes, exempt from the internal check."""

    __slots__ = ("base", "pixels", "cs", "c_lo", "c_hi", "what", "role", "scratch")

    def __init__(self, base, pixels, cs, c_lo, c_hi, what, role=ACTIVATION, scratch=False):
        base, pixels, cs, c_lo, c_hi = int(base), int(pixels), int(cs), int(c_lo), int(c_hi)
        assert pixels > 0 and cs > 0 and 0 <= c_lo < c_hi, (what, pixels, cs, c_lo, c_hi)
        if c_hi - c_lo >= cs and cs > 1:  # consecutive pixels touch: one range
            base, pixels, cs, c_lo, c_hi = base + c_lo, (pixels - 1) * cs + c_hi - c_lo, 1, 0, 1
        self.base, self.pixels, self.cs, self.c_lo, self.c_hi, self.what, self.role, self.scratch = base, pixels, cs, c_lo, c_hi, what, role, scratch

    @property
    def dense(self):
        return self.cs == 1

    @property
    def lo(self):  # first float
        return self.base + self.c_lo

    @property
    def hi(self):  # one past the last float
        return self.base + (self.pixels - 1) * self.cs + self.c_hi

    @property
    def count(self):
        return self.pixels * (self.c_hi - self.c_lo)

    def indices(self, origin):
        """Every float of the footprint as an index relative to ``origin`` (floats), for the tests that poison / compare buffers."""
        p = np.arange(self.pixels, dtype=np.int64)[:, None] * self.cs
        return (self.base - origin + p + np.arange(self.c_lo, self.c_hi, dtype=np.int64)[None, :]).reshape(-1)

    def __repr__(self):
        if self.dense:
            return f"{self.what}[0x{4 * self.lo:x}, +{self.pixels} floats)"
        return f"{self.what}[0x{4 * self.base:x}: {self.pixels} px x cs {self.cs}, ch {self.c_lo}..{self.c_hi})"


def dense(ptr, floats, what, role=ACTIVATION, scratch=False):
    assert ptr % 4 == 0, (what, ptr)
    return Footprint(ptr // 4, floats, 1, 0, 1, what, role, scratch)


def strided(ptr, pixels, cs, c_lo, c_hi, what):
    assert ptr % 4 == 0, (what, ptr)
    return Footprint(ptr // 4, pixels, cs, c_lo, c_hi, what)


# ----------------------------------------------------------------------------------------------------------------------------------------
# weights: the library's own size functions (host code, no device)
# ----------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from implicit_depth_amd import _lib

    return _lib.lib()


def conv_weight_floats(op, i):
    """Floats of src[i].w as the kernel selected by tile_m reads them; 0: the kernel does not read that pointer."""
    s, L = op.src[i], _L()
    if op.tile_m == TILE_SPLIT:  # one blob for both sources behind src[0].w; src[1].w is ignored
        if i:
            return 0
        nbytes = L.idh_packed_split_weight_bytes(op.Cout, s.Cin, op.src[1].Cin if op.src[1].in_ else 0, TILE_SPLIT)
        assert nbytes % 4 == 0
        return nbytes // 4
    if i == 0 and op.tile_m == TILE_WINO4:
        return L.idh_packed_wino4_weight_floats(op.Cout, s.Cin)
    if i == 0 and op.tile_m == TILE_WINO:
        return L.idh_packed_wino_weight_floats(op.Cout, s.Cin)
    return L.idh_packed_weight_floats(op.Cout, s.Cin, s.ks)


# ----------------------------------------------------------------------------------------------------------------------------------------
# footprints
# ----------------------------------------------------------------------------------------------------------------------------------------
def _conv(op, split):
    reads, writes = [], []
    M = op.N * op.Ho * op.Wo
    for i in range(2):
        s = op.src[i]
        if not s.in_:
            continue
        px = op.N * s.H * s.W
        if s.up_in[0]:  # virtual concat: channels [0, up_c0) of `in`, then the x2 upsampling of the half-size maps
            if s.up_c0:
                reads.append(strided(s.in_, px, s.cs, 0, s.up_c0, f"src[{i}].in"))
            for j in range(2):
                if s.up_in[j]:
                    reads.append(strided(s.up_in[j], op.N * (s.H // 2) * (s.W // 2), s.up_cs[j], 0, s.up_C, f"src[{i}].up_in[{j}]"))
        else:  # whole 16-channel blocks
            reads.append(strided(s.in_, px, s.cs, 0, ceil16(s.Cin), f"src[{i}].in"))
        if s.w:
            n = conv_weight_floats(op, i)
            if n:
                reads.append(dense(s.w, n, f"src[{i}].w", WEIGHT))
        if s.norm:
            reads.append(dense(s.norm, op.N * 2 * s.Cin, f"src[{i}].norm"))
    if op.bias:
        reads.append(dense(op.bias, op.Cout, "bias", WEIGHT))
    if op.res:
        reads.append(strided(op.res, M, op.res_cs, 0, op.Cout, "res"))
    writes.append(strided(op.out, M, op.out_cs, 0, op.Cout, "out"))
    S = op.split_k if split is None else split
    if S > 1 and op.ws:
        writes.append(dense(op.ws, S * M * ceil16(op.Cout), "ws", scratch=True))
    return reads, writes


def _stem_images(op):
    """The strided batch view of IDH_OP_STEM: N dense (3, H, W) images in groups of up_C."""
    s = op.src[0]
    img = 3 * s.H * s.W
    per = s.up_C or op.N
    img_stride = s.up_cs[0] or img
    grp_stride = s.up_cs[1] or per * img_stride
    if img_stride == img and grp_stride == per * img:
        return [dense(s.in_, op.N * img, "src[0].in")]
    return [dense(s.in_ + 4 * ((k // per) * grp_stride + (k % per) * img_stride), img, f"src[0].in image {k}") for k in range(op.N)]


def footprints(op, split=None):
    """(reads, writes) of one ``idh_op`` (an ``nhwc.Op``), each a list of Footprint.  ``split``: the split count the conv runs with when it is
    known to be clamped below ``op.split_k`` (``idh_conv_variant``'s S); default: ``op.split_k``, the workspace the header asks for."""
    k, s = op.kind, op.src[0]
    px = op.N * s.H * s.W
    if k == OP_CONV:
        return _conv(op, split)
    if k in (OP_UPSAMPLE2, OP_NEAREST, OP_COPY):
        scale = 1 if k == OP_COPY else 4
        return [strided(s.in_, px, s.cs, 0, s.Cin, "src[0].in")], [strided(op.out, scale * px, op.out_cs, 0, s.Cin, "out")]
    if k == OP_IMPORT:
        return [dense(s.in_, px * s.Cin, "src[0].in")], [strided(op.out, px, op.out_cs, 0, s.Cin, "out")]
    if k == OP_EXPORT:
        return [strided(s.in_, px, s.cs, 0, s.Cin, "src[0].in")], [dense(op.out, px * s.Cin, "out")]
    if k == OP_HEAD:
        reads = [strided(s.in_, px, s.cs, 0, s.Cin, "src[0].in"), dense(s.w, s.Cin, "src[0].w", WEIGHT)]
        if op.bias:
            reads.append(dense(op.bias, 1, "bias", WEIGHT))
        writes = [dense(op.out, px, "out")]
        if op.ws:  # exp(out), a second output
            writes.append(dense(op.ws, px, "ws"))
        return reads, writes
    if k == OP_INSTNORM:
        nchunks = -(-(s.H * s.W) // INSTNORM_CHUNK)
        writes = [dense(op.ws, op.N * (nchunks + 1) * 2 * s.Cin, "ws", scratch=True)]
        if op.out:
            writes.append(strided(op.out, px, op.out_cs, 0, s.Cin, "out"))
        return [strided(s.in_, px, s.cs, 0, s.Cin, "src[0].in")], writes
    if k == OP_PW_NCHW:
        reads = [dense(s.in_, px * s.Cin, "src[0].in"), dense(s.w, _L().idh_packed_weight_floats(op.Cout, s.Cin, 1), "src[0].w", WEIGHT)]
        if op.bias:
            reads.append(dense(op.bias, op.Cout, "bias", WEIGHT))
        return reads, [strided(op.out, px, op.out_cs, 0, op.Cout, "out")]
    if k == OP_PW_UP:
        lo = op.src[1]
        reads = [strided(s.in_, px, s.cs, 0, s.Cin, "src[0].in"), strided(lo.in_, op.N * lo.H * lo.W, lo.cs, 0, op.Cout, "src[1].in"),
                 dense(s.w, _L().idh_packed_weight_floats(op.Cout, s.Cin, 1), "src[0].w", WEIGHT)]
        if op.bias:
            reads.append(dense(op.bias, op.Cout, "bias", WEIGHT))
        return reads, [strided(op.out, px, op.out_cs, 0, op.Cout, "out")]
    if k == OP_STEM:
        reads = _stem_images(op) + [dense(s.w, _L().idh_stem_weight_floats(), "src[0].w", WEIGHT)]
        return reads, [strided(op.out, op.N * op.Ho * op.Wo, op.out_cs, 0, 64, "out")]
    raise ValueError(f"no footprint for op kind {k}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# conflict
# ----------------------------------------------------------------------------------------------------------------------------------------
def conflict(a, b, counter=None):
    """True when the two footprints share a float.  Exact for two strided sets of one channel stride and for anything against a dense
    range given as [lo, hi); two strided sets of different channel strides whose ranges intersect count as a conflict (``counter``, a
    one-element list, counts those decisions: a well-formed plan has none)."""
    if a.hi <= b.lo or b.hi <= a.lo:
        return False
    if a.dense or b.dense:
        return True
    if a.cs != b.cs:
        if counter is not None:
            counter[0] += 1
        return True
    # pixel p of a holds [a.lo + p cs, + wa), pixel q of b [b.lo + q cs, + wb): they meet iff -wb < d + k cs < wa with k = q - p, d = b.lo - a.lo
    cs, wa, wb, d = a.cs, a.c_hi - a.c_lo, b.c_hi - b.c_lo, b.lo - a.lo
    k_min = (-wb - d) // cs + 1  # smallest k with d + k cs > -wb
    k_max = -((d - wa) // cs) - 1  # largest k with d + k cs < wa
    for k in range(k_min, k_max + 1):
        if max(0, -k) < min(a.pixels, b.pixels - k):  # some p in [0, a.pixels) with p + k in [0, b.pixels)
            return True
    return False


# ----------------------------------------------------------------------------------------------------------------------------------------
# audit
# ----------------------------------------------------------------------------------------------------------------------------------------
class Finding:
    """kind: "order" / "concurrency" / "internal" / "containment"; hazard: "RAW" / "WAW" / "WAR" between op a (the earlier-built one)
    and op b, or what a footprint should have been contained in."""

    def __init__(self, kind, hazard, a, b, fa, fb):
        self.kind, self.hazard, self.a, self.b, self.fa, self.fb = kind, hazard, a, b, fa, fb

    def key(self):
        """(kind, hazard, build index of a, field of a, build index of b, field of b)"""
        return (self.kind, self.hazard, self.a["build"], self.fa.what, self.b["build"] if self.b else None, self.fb.what if self.fb is not None else None)

    def __repr__(self):
        d = lambda o: f"op at {o['pos']} (built {o['build']}, {KIND_NAMES.get(o['kind'], o['kind'])}, tile {o['tile_m']}x{o['tile_n']}, group {o['group']})"
        tail = f" <-> {d(self.b)} {self.fb!r}" if self.b else (f" not inside {self.fb}" if self.fb is not None else "")
        return f"{self.kind} {self.hazard}: {d(self.a)} {self.fa!r}{tail}"


class Findings(list):
    """The findings of one audit + its counters: ops, launch groups (runs of >= 2 ops), the largest group, op pairs examined, pairs of
    footprints decided exactly, decisions by the conservative different-stride rule."""

    ops = groups = largest_group = pairs = decided = conservative = 0

    def summary(self):
        return (f"{self.ops} ops, {self.groups} launch groups (largest {self.largest_group}), {self.pairs} pairs examined, "
                f"{self.decided} footprint pairs decided, {self.conservative} by the different-stride rule, {len(self)} conflicts")


def launch_groups(ops, n_first):
    """group index per position: consecutive ops of one segment with the same non-zero ``group`` share one, every other op has its own."""
    ids, cur = [], -1
    for i, op in enumerate(ops):
        same = i > 0 and i != n_first and op.group != 0 and ops[i - 1].group == op.group
        cur += 0 if same else 1
        ids.append(cur)
    return ids


def _describe(ops, order, i):
    op = ops[i]
    return {"pos": i, "build": int(order[i]), "kind": op.kind, "tile_m": op.tile_m, "tile_n": op.tile_n, "group": op.group}


def _inside(f, lo, hi):
    return lo <= f.lo and f.hi <= hi


def audit(ops, order, n_first, ws=None, blob=None, externals=None, splits=None):
    """Hazards of a scheduled op list.  ``ops``: the descriptors in scheduled order; ``order[i]``: the build index of the op at position i;
    ops [0, n_first) and the rest are the two segments (they run one after the other).

    Containment (each optional): ``ws`` = (address, floats) of the plan's workspace, ``blob`` = (address, floats) of its weight blob,
    ``externals`` = [(address, floats)] of the tensors the caller declared.  With ``blob``, every weight / bias read lies inside it and
    nothing else touches it.  With ``ws``, a footprint that touches the workspace lies inside it.  With ``ws`` and ``externals``, every
    other activation footprint lies inside one declared tensor.  ``splits``: per position, the clamped split count (see ``footprints``)."""
    n = len(ops)
    order = [int(v) for v in order]
    assert len(order) >= n and sorted(order[:n]) == list(range(n)), "order is a permutation of the build indices"
    out = Findings()
    out.ops = n
    gid = launch_groups(ops, n_first)
    sizes = np.bincount(np.asarray(gid, dtype=np.int64), minlength=1) if n else np.zeros(1, dtype=np.int64)
    out.groups, out.largest_group = int((sizes >= 2).sum()), int(sizes.max()) if n else 0
    fps = [footprints(op, None if splits is None else splits[i]) for i, op in enumerate(ops)]
    desc = lambda i: _describe(ops, order, i)
    counter = [0]

    # ---- internal
    for i, (reads, writes) in enumerate(fps):
        for w in writes:
            for r in reads:
                if conflict(w, r, counter):
                    out.append(Finding("internal", "RAW", desc(i), desc(i), w, r))
            for w2 in writes:
                if w2 is not w and id(w) < id(w2) and conflict(w, w2, counter):
                    out.append(Finding("internal", "WAW", desc(i), desc(i), w, w2))

    # ---- order and concurrency: every pair of ops; the hulls are compared at once, the survivors decided exactly
    flat = [(i, f, is_w) for i, (reads, writes) in enumerate(fps) for is_w, fs in ((False, reads), (True, writes)) for f in fs]
    out.pairs = n * (n - 1) // 2
    if flat:
        pos = np.array([t[0] for t in flat])
        lo = np.array([t[1].lo for t in flat], dtype=np.int64)
        hi = np.array([t[1].hi for t in flat], dtype=np.int64)
        wr = np.array([t[2] for t in flat])
        cand = (lo[:, None] < hi[None, :]) & (lo[None, :] < hi[:, None]) & (wr[:, None] | wr[None, :]) & (pos[:, None] < pos[None, :])
        for x, y in zip(*np.nonzero(cand)):
            (i, fi, wi), (j, fj, wj) = flat[x], flat[y]
            out.decided += 1
            if not conflict(fi, fj, counter):
                continue
            # a = the op built first
            first_is_i = order[i] < order[j]
            a, fa, wa, b, fb, wb = (i, fi, wi, j, fj, wj) if first_is_i else (j, fj, wj, i, fi, wi)
            hazard = "WAW" if wa and wb else ("RAW" if wa else "WAR")
            if gid[i] == gid[j]:
                out.append(Finding("concurrency", hazard, desc(a), desc(b), fa, fb))
            elif not first_is_i:  # position i runs first, yet it was built later
                out.append(Finding("order", hazard, desc(a), desc(b), fa, fb))

    # ---- containment
    rng = lambda r: (r[0] // 4, r[0] // 4 + r[1])
    if blob is not None or ws is not None:
        for i, (reads, writes) in enumerate(fps):
            for f in reads + writes:
                if f.role == WEIGHT:
                    if blob is not None and not _inside(f, *rng(blob)):
                        out.append(Finding("containment", "weight outside the blob", desc(i), None, f, f"blob [0x{blob[0]:x}, +{blob[1]} floats)"))
                    continue
                if blob is not None and f.lo < rng(blob)[1] and rng(blob)[0] < f.hi:
                    out.append(Finding("containment", "activation inside the blob", desc(i), None, f, f"blob [0x{blob[0]:x}, +{blob[1]} floats)"))
                    continue
                if ws is None:
                    continue
                w0, w1 = rng(ws)
                if f.lo < w1 and w0 < f.hi:
                    if not _inside(f, w0, w1):
                        out.append(Finding("containment", "straddles the workspace", desc(i), None, f, f"workspace [0x{ws[0]:x}, +{ws[1]} floats)"))
                elif externals is not None and not any(_inside(f, *rng(e)) for e in externals):
                    out.append(Finding("containment", "outside every declared tensor", desc(i), None, f, f"{len(externals)} declared tensors"))
    out.conservative = counter[0]
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# the C++ builder's plans, through idh_debug_set_plan_observer
# ----------------------------------------------------------------------------------------------------------------------------------------
class ObservedPlan:
    def __init__(self, ops, n_first, order, ws, blob):
        self.ops, self.n_first, self.order, self.ws, self.blob = ops, n_first, order, ws, blob

    def audit(self, externals=None):
        return audit(self.ops, self.order, self.n_first, ws=self.ws, blob=self.blob, externals=externals)


class observe:
    """``with observe() as plans:`` - every plan csrc/networks.hip schedules inside the block is appended to ``plans`` (copies: the
    library's arrays die when the callback returns)."""

    def __enter__(self):
        import ctypes as C

        from implicit_depth_amd import _lib, nhwc

        self.plans = plans = []

        def cb(ops, n, n_first, order, ws, ws_floats, blob, blob_floats, user):
            arr = (nhwc.Op * n).from_buffer_copy(C.string_at(ops, n * C.sizeof(nhwc.Op))) if n else []
            plans.append(ObservedPlan(list(arr), n_first, [order[i] for i in range(n)], (ws or 0, ws_floats), (blob or 0, blob_floats)))

        self._cb = _lib.PlanObserver(cb)  # (kept alive for as long as the library holds it)
        self._L = _lib.lib()
        self._L.idh_debug_set_plan_observer(self._cb, None)
        return plans

    def __exit__(self, *exc):
        self._L.idh_debug_set_plan_observer(type(self._cb)(), None)  # a NULL function pointer clears the hook
        return False
