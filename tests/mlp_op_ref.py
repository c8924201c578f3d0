"""Hand-built calls of the nine C entry points of csrc/mlp.hip (include/idh.h) and their fp64 references.

``mlp.py`` only emits the shapes of the shipped network (64 features in a wide NHWC buffer or 65 / 66-float rows, B = 1 for the
prior); test_mlp_op_cpu.py / test_mlp_op_gpu.py call the entry points themselves, so that channel tails (Cf % 16 != 0), both homes
of W1 (LDS up to 64 features, global memory above), the persistent tile loop, every feature layout, the search with priors and
Thresholder tables, multi-frame ``idh_sample_prior_fwd`` and both weight packers are reached at a small size.  One set of tables
(``LOGIT_CASES``, ``SEARCH_CASES``, ``PRIOR_CASES``, ``PACK_CASES``, ``PACK_F16_CASES``) serves both files.

Buffers are hostile on purpose: the features are a slice of a larger buffer in which every float outside the Cf channels of the M
rows is NaN (channels [Cf, feat_cs), the floats before the base, whole rows after row M - 1); outputs are slices of buffers
prefilled with a NaN bit pattern whose surroundings must come back bit-identical; ``vecs[2]`` (the prior column of W1) is NaN
when ``has_prior`` is 0, and so is the unused tail of ``vecs[5]``.
"""
import math
import zlib

import numpy as np
import torch

import implicit_depth_amd.synthetic as syn
from oracle import networks as onet

U = 2.0 ** -24  # fp32 unit roundoff
PREFILL = 0x7FC5A5A5  # quiet NaN with a payload: an unwritten element fails the comparison, a stray store changes the bits
GUARD = 8  # prefilled words either side of every output
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
HID = 128
ACC_C = 4  # the "+ c" of the accumulation term: bias, the two rank-1 terms (or partial sums of the lane reduction) and one spare
ELU_ERR = 3 * U  # see logit_bound
NAN = float("nan")


def _seed(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------
class LogitCase:
    """entry: "fp32" | "f16x3" | "strided".  prior: None | "tensor" | -1.0 | 0.37 (null pointer + prior_const).
    layout (row entries): "dense" (feat_cs = Cf), "wide" (Cf + 12, base 16 floats in), "row65" / "row66" (base 1 float in),
    "base1" (Cf + 4, base 1 float in: 4- but not 16-byte aligned rows of a stride that is a multiple of 4);
    (strided): "nchw" (channel planes), "frames2" (every second frame of an NCHW tensor), "nhwc" (rows as strides)."""

    def __init__(self, entry, cf, B, HW, P, prior, layout):
        self.entry, self.cf, self.B, self.HW, self.P, self.prior, self.layout = entry, cf, B, HW, P, prior, layout
        pn = "noprior" if prior is None else (prior if isinstance(prior, str) else f"const{prior:g}")
        self.name = f"{entry}-c{cf}-b{B}x{HW}-p{P}-{pn}-{layout}"

    @property
    def M(self):
        return self.B * self.HW

    @property
    def has_prior(self):
        return self.prior is not None

    @property
    def large(self):
        return self.M > 4096


PERSISTENT_HW = {"fp32": 24593, "strided": 24593, "f16x3": 16403}  # B = 2: 3075 tiles > 256 x 12, 2051 tiles > 256 x 8

LOGIT_CASES = [LogitCase(*a) for a in (
    # every Cf, M in {1, 15, 16, 17}, 3 x 21, P in {1, 3}, the four priors and every layout, per entry point
    ("fp32", 4, 1, 1, 1, None, "dense"),
    ("fp32", 20, 1, 15, 3, "tensor", "wide"),
    ("fp32", 20, 3, 21, 3, None, "base1"),
    ("fp32", 48, 1, 16, 1, -1.0, "dense"),
    ("fp32", 64, 1, 17, 3, 0.37, "row65"),
    ("fp32", 64, 3, 21, 3, "tensor", "row66"),
    ("fp32", 68, 3, 21, 3, None, "base1"),
    ("fp32", 128, 3, 21, 1, "tensor", "wide"),
    ("fp32", 256, 1, 17, 3, -1.0, "base1"),
    ("fp32", 64, 2, PERSISTENT_HW["fp32"], 1, None, "dense"),
    ("f16x3", 4, 1, 15, 3, "tensor", "wide"),
    ("f16x3", 20, 1, 1, 1, None, "dense"),
    ("f16x3", 48, 1, 17, 3, 0.37, "wide"),
    ("f16x3", 64, 3, 21, 3, -1.0, "dense"),
    ("f16x3", 68, 1, 16, 1, "tensor", "dense"),
    ("f16x3", 128, 3, 21, 3, None, "wide"),
    ("f16x3", 256, 1, 16, 3, "tensor", "dense"),
    ("f16x3", 64, 2, PERSISTENT_HW["f16x3"], 1, "tensor", "dense"),
    ("strided", 4, 1, 17, 3, None, "nchw"),
    ("strided", 20, 3, 21, 3, "tensor", "frames2"),
    ("strided", 48, 1, 15, 1, -1.0, "nhwc"),
    ("strided", 64, 1, 1, 1, 0.37, "nchw"),
    ("strided", 68, 3, 21, 3, "tensor", "nhwc"),
    ("strided", 128, 1, 16, 3, None, "nchw"),
    ("strided", 256, 3, 21, 1, -1.0, "frames2"),
    ("strided", 64, 2, PERSISTENT_HW["strided"], 1, None, "nchw"),
)]
assert len({c.name for c in LOGIT_CASES}) == len(LOGIT_CASES)

# Thresholder tables (bins ascending, thresholds in (0, 1)).  "edge": 3.75, the first query of a (0.5, 8) search, IS an edge (bucketize
# counts the edges strictly below the query).  "clamp": every edge lies below the later queries of a (1, 3) search that moved lo, so
# the count reaches n_bins and is clamped to the last bin.  "one": n_bins = 1.
TABLES = {
    "edge": ([1.5, 2.5, 3.75, 5.0, 6.5], [0.3, 0.4, 0.5, 0.6, 0.45]),
    "clamp": ([1.2, 1.6, 2.0], [0.35, 0.5, 0.65]),
    "one": ([2.0], [0.4]),
}
SEARCH_ITERS = 12


class SearchCase:
    """entry: "fp32" | "f16x3"; thr: a constant threshold (float) or a key of TABLES."""

    def __init__(self, entry, cf, prior, lo, hi, thr, layout, B=2, HW=21 * 13):
        self.entry, self.cf, self.prior, self.lo, self.hi, self.thr, self.layout, self.B, self.HW = entry, cf, prior, lo, hi, thr, layout, B, HW
        self.P = 1
        pn = "noprior" if prior is None else (prior if isinstance(prior, str) else f"const{prior:g}")
        self.name = f"search-{entry}-c{cf}-{pn}-{lo:g}to{hi:g}-thr{thr}-{layout}"

    M = LogitCase.M
    has_prior = LogitCase.has_prior

    @property
    def table(self):
        return TABLES[self.thr] if isinstance(self.thr, str) else None


SEARCH_CASES = [SearchCase(*a) for a in (
    ("fp32", 64, None, 0.5, 8.0, 0.5, "dense"),
    ("fp32", 64, "tensor", 1.0, 3.0, 0.3, "wide"),
    ("fp32", 64, -1.0, 0.5, 8.0, 0.3, "wide"),
    ("fp32", 64, None, 0.5, 8.0, "edge", "wide"),
    ("fp32", 64, "tensor", 1.0, 3.0, "clamp", "dense"),
    ("fp32", 64, 0.37, 0.5, 8.0, "one", "dense"),
    ("fp32", 20, "tensor", 0.5, 8.0, "edge", "wide"),
    ("f16x3", 64, None, 1.0, 3.0, 0.5, "wide"),
    ("f16x3", 64, "tensor", 0.5, 8.0, 0.3, "dense"),
    ("f16x3", 64, -1.0, 0.5, 8.0, 0.5, "wide"),
    ("f16x3", 64, None, 0.5, 8.0, "one", "dense"),
    ("f16x3", 64, "tensor", 0.5, 8.0, "edge", "wide"),
    ("f16x3", 64, 0.37, 1.0, 3.0, "clamp", "dense"),
    ("f16x3", 20, None, 0.5, 8.0, 0.3, "dense"),
)]
assert len({c.name for c in SEARCH_CASES}) == len(SEARCH_CASES)


class PriorCase:
    """kind: "general" (three poses and intrinsics, the last frame's previous camera looks the other way), "tie" (every sample
    coordinate on x + 0.5, all arithmetic exact), "identity" (out == prior where the depth is positive)."""

    def __init__(self, kind, Q, P, H, W, B=3):
        self.kind, self.Q, self.P, self.H, self.W, self.B = kind, Q, P, H, W, B
        self.name = f"prior-{kind}-q{Q}p{P}-{H}x{W}"


PRIOR_CASES = [PriorCase("general", 1, 3, 13, 19), PriorCase("general", 2, 2, 13, 19), PriorCase("general", 2, 4, 13, 19),
               PriorCase("general", 2, 3, 300, 301),  # P H W = 270900 > 1024 blocks x 256 threads: the grid-stride loop
               PriorCase("tie", 1, 1, 8, 16, B=1), PriorCase("identity", 2, 3, 8, 16, B=2)]

PACK_CASES = [(n_in, col0, col0 + n_in + extra) for n_in in (4, 20, 64, 65, 128) for col0, extra in ((0, 3), (1, 1))]  # (n_in, col0, ld)
PACK_F16_CASES = [(20, 1, 23), (128, 0, 131)]


# ------------------------------------------------------------------------------------------------------------------
# weights and inputs (CPU, seeded by the case name)
# ------------------------------------------------------------------------------------------------------------------
def make_net(cf, has_prior, seed, depth_gain=1.0):
    """BinaryMLPNetwork scale 0 with W1 of width 1 + Cf (+ 1), filled by synthetic.fill_state_dict as the existing MLP tests do."""
    from implicit_depth_amd import networks as net

    m = net.BinaryMLPNetwork([cf], mlp_size=HID, use_prior=has_prior)
    syn.fill_state_dict(m, seed=seed & 0x7FFFFFFF, gain=1.2)
    if depth_gain != 1.0:
        with torch.no_grad():
            m.mlps["s0"][0].weight[:, 0] *= depth_gain  # make the logit depend visibly on the query depth
    return m


def weights64(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def logit_inputs(case):
    """feat (B, Cf, HW), depth (B, P, HW), prior (B, P, HW) | None - CPU fp32.  The depth planes contain 0 and 80."""
    s = _seed(case.name)
    feat = syn.randn((case.B, case.cf, case.HW), s, "feat")
    depth = 0.5 + 7.5 * torch.rand((case.B, case.P, case.HW), generator=torch.Generator().manual_seed(s))
    flat = depth.view(-1)
    flat[-1] = 80.0
    if flat.numel() > 1:
        flat[0] = 0.0
    if flat.numel() > 8:
        flat[flat.numel() // 2] = 0.0
        flat[flat.numel() // 3] = 80.0
    prior = None
    if case.prior == "tensor":
        prior = torch.tanh(syn.randn((case.B, case.P, case.HW), s, "prior"))  # distinct per plane
    return feat, depth, prior


def prior64(case, prior, shape):
    if not case.has_prior:
        return None
    if prior is not None:
        return prior.double()
    return torch.full(shape, float(np.float32(case.prior)), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------
# fp64 reference and the derived elementwise bound of the logits
# ------------------------------------------------------------------------------------------------------------------
def reference_logits(w, feat, depth, prior):
    """oracle.networks.occlusion_logits on (B, Cf, HW) features: (B, P, HW) fp64."""
    f = feat.double().unsqueeze(-1)
    d = depth.double().unsqueeze(-1)
    return onet.occlusion_logits(f, d, w, None if prior is None else prior.double().unsqueeze(-1)).squeeze(-1)


def logit_bound(w, feat, depth, prior, f16=False, elu=onet.elu):
    """(fp64 logits, elementwise bound), both (B, P, HW).  The bound is derived, not measured (u = 2^-24):

    A sum of K products accumulated in fp32 in any order, plus c further terms, errs by at most (K + c) u S with S the sum of the
    magnitudes |w||x| (+ |bias| ...); twice that is allowed because the rounding inside the matrix unit is unspecified:
    ``acc(K, S) = 2 (K + c) u S`` with c = 4.  Errors already present in the inputs pass through as |W| e.

    layer 1   a1 = b1 + W1f f + wd d (+ wp p): K = Cf + 3 terms, S1 = |b1| + |W1f||f| + |wd||d| + |wp||p|;  e_a1 = acc(Cf + 3, S1).
    ELU       elu is 1-Lipschitz, so e_h = e_a + e_elu.  The kernel forms exp(x) - 1 with __expf = v_exp_f32(x * log2 e) for x <= 0:
              the argument t = fl(x * fl(log2 e)) carries two roundings, |dt| <= 2 u |t|, so 2^t is off by the factor 2^dt: relative
              error ln 2 * 2 u |x| log2 e = 2 u |x|; v_exp_f32 itself is accurate to 1 ulp (<= 2 u relative); the subtraction rounds
              once (<= u, the result lies in (-1, 0]).  e^x (2 |x| + 2) u + u <= 3 u for every x <= 0 (the first term grows towards
              x = 0, where it is 2 u); for x > 0 the kernel returns x itself.  e_elu = 3 u everywhere (a pre-activation within its
              error of 0 may take either branch).
    layer 2   a2 = b2 + W2 h1: e_a2 = |W2| e_h1 + acc(128, S2), S2 = |b2| + |W2| (|h1| + e_h1).
              f16x3 (csrc/split_f16.h): h1 is scaled per pixel by 2^(14 - ex), 2^ex <= max |h1|, W2 per row likewise, and each scaled
              value v becomes hi = f16(v), lo = f16(v - hi): |v - hi| <= 2^-11 |v| and lo's own rounding <= 2^-11 |v - hi|, i.e. the
              pair misses v by at most 2^-22 |v| (2^-24 absolute where a piece is subnormal: 2^-38 of the row's / pixel's maximum after
              unscaling).  The kernel adds hi.hi + hi.lo + lo.hi and drops lo.lo, <= 2^-22 |w||x|.  Products of two f16 are exact
              in fp32, the 3 x 128 of them are accumulated in fp32 and the power-of-two unscaling is exact:
              e_a2 = |W2| e_h1 + 3 * 2^-22 S2' + 2^-38 (|W2|_1 max|h1| + max|W2| |h1|_1) + acc(3 * 128, S2),  S2' = |W2| (|h1| + e_h1).
    layer 3   logit = b3 + w3 h2 (32 fmas per lane, two shuffle adds, + b3): e = |w3| e_h2 + acc(128, S3) + u |logit| for the result's
              own rounding."""
    c = ACC_C
    acc = lambda K, S: 2 * (K + c) * U * S
    W1, b1 = w["mlps.s0.0.weight"], w["mlps.s0.0.bias"]
    W2, b2 = w["mlps.s0.2.weight"], w["mlps.s0.2.bias"]
    W3, b3 = w["mlps.s0.4.weight"], w["mlps.s0.4.bias"]
    cf = feat.shape[1]
    f = feat.double().permute(0, 2, 1)  # B, HW, Cf
    W1f, wd = W1[:, 1:1 + cf], W1[:, 0]
    pre = f @ W1f.t() + b1  # B, HW, 128
    Spre = f.abs() @ W1f.abs().t() + b1.abs()
    d = depth.double().unsqueeze(-1)  # B, P, HW, 1
    a1 = pre.unsqueeze(1) + d * wd
    S1 = Spre.unsqueeze(1) + d.abs() * wd.abs()
    if prior is not None:
        p = prior.double().unsqueeze(-1)
        wp = W1[:, 1 + cf]
        a1, S1 = a1 + p * wp, S1 + p.abs() * wp.abs()
    e_h1 = acc(cf + 3, S1) + ELU_ERR
    h1 = elu(a1)
    h1m = h1.abs() + e_h1
    a2 = h1 @ W2.t() + b2
    S2p = h1m @ W2.abs().t()
    S2 = S2p + b2.abs()
    e_a2 = e_h1 @ W2.abs().t()
    if f16:
        floor = 2.0 ** -38 * (W2.abs().sum(1) * h1m.max(-1, keepdim=True).values + W2.abs().max(1).values * h1m.sum(-1, keepdim=True))
        e_a2 = e_a2 + 3 * 2.0 ** -22 * S2p + floor + acc(3 * HID, S2)
    else:
        e_a2 = e_a2 + acc(HID, S2)
    e_h2 = e_a2 + ELU_ERR
    h2 = elu(a2)
    w3 = W3[0]
    logit = h2 @ w3 + b3[0]
    S3 = (h2.abs() + e_h2) @ w3.abs() + b3[0].abs()
    tol = e_h2 @ w3.abs() + acc(HID, S3) + U * logit.abs()
    return logit, tol



# ------------------------------------------------------------------------------------------------------------------
# device side: packed weights, hostile feature buffers, output slices
# ------------------------------------------------------------------------------------------------------------------
def pack_net(m, cf, has_prior, f16, device="cuda"):
    """(w1f_packed, w2 packed | f16-packed, vecs6x128) exactly as mlp._prepared builds them: W1 through idh_pack_mlp_weight with
    ld = 1 + Cf (+ 1) > n_in and col0 = 1.  vecs[2] is NaN without a prior column, and so are vecs[5][1:]."""
    from implicit_depth_amd import _lib

    L = _lib.lib()
    seq = m.mlps["s0"]
    w1 = seq[0].weight.detach().to(device).contiguous()
    w2 = seq[2].weight.detach().to(device).contiguous()
    st = _lib.stream_ptr()
    w1p = torch.empty(L.idh_packed_mlp_weight_floats(cf), device=device)
    assert L.idh_pack_mlp_weight(w1.data_ptr(), w1p.data_ptr(), w1.shape[1], 1, cf, st) == OK
    if f16:
        w2p = torch.empty(L.idh_packed_mlp_weight_f16_bytes(HID) // 4, device=device, dtype=torch.int32)
        assert L.idh_pack_mlp_weight_f16(w2.data_ptr(), w2p.data_ptr(), HID, 0, HID, st) == OK
    else:
        w2p = torch.empty(L.idh_packed_mlp_weight_floats(HID), device=device)
        assert L.idh_pack_mlp_weight(w2.data_ptr(), w2p.data_ptr(), HID, 0, HID, st) == OK
    vecs = torch.full((6, HID), NAN)
    vecs[0] = seq[0].bias.detach()
    vecs[1] = seq[0].weight.detach()[:, 0]
    if has_prior:
        vecs[2] = seq[0].weight.detach()[:, cf + 1]
    vecs[3] = seq[2].bias.detach()
    vecs[4] = seq[4].weight.detach()[0]
    vecs[5, 0] = seq[4].bias.detach()[0]
    torch.cuda.synchronize()
    return w1p, w2p, vecs.to(device)


ROW_LAYOUTS = {"dense": (0, 0), "wide": (12, 16), "row65": (None, 1), "row66": (None, 1), "base1": (4, 1)}  # (feat_cs - Cf, base offset in floats)


def row_layout(case):
    """(feat_cs, base offset in floats) of a row-based case."""
    extra, off = ROW_LAYOUTS[case.layout]
    cs = {"row65": 65, "row66": 66}.get(case.layout) or case.cf + extra
    return cs, off


def feature_buffer(case, feat):
    """A NaN-filled CPU buffer with the case's features laid out in it.  Returns (flat buffer, base offset in floats, args) where
    args is (feat_cs,) for the row entry points and (batch stride, pixel stride, channel stride) for the strided one."""
    B, cf, HW = feat.shape
    rows = feat.permute(0, 2, 1).reshape(B * HW, cf)
    if case.layout in ROW_LAYOUTS or case.layout == "nhwc":
        cs, off = row_layout(case) if case.layout != "nhwc" else (cf + 5, 3)
        buf = torch.full((off + (B * HW + 2) * cs,), NAN)  # two whole NaN rows behind row M - 1
        buf[off: off + B * HW * cs].view(B * HW, cs)[:, :cf] = rows
        return buf, off, ((cs,) if case.layout != "nhwc" else (HW * cs, cs, 1))
    step = 2 if case.layout == "frames2" else 1
    t = torch.full((B * step, cf + 2, HW), NAN)  # [depth | features | prior] channel planes: only the features are real
    t[::step, 1:1 + cf] = feat
    return t.view(-1), HW, (step * (cf + 2) * HW, 1, HW)


class Out:
    """n floats in the middle of a prefilled int32 buffer."""

    def __init__(self, n, device="cuda"):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), PREFILL, dtype=torch.int32, device=device)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def read(self):
        """(values as CPU fp32, True when the guard words are untouched)."""
        raw = self.buf.cpu()
        clean = bool((raw[:GUARD] == PREFILL).all() and (raw[GUARD + self.n:] == PREFILL).all())
        return raw[GUARD: GUARD + self.n].clone().view(torch.float32), clean


def run_logits(L, case, dev, entry=None):
    """One launch of the case's entry point into a fresh output; returns (rc, Out).  dev: dict of device tensors from device_case."""
    from implicit_depth_amd import _lib

    entry = entry or case.entry
    out = Out(case.B * case.P * case.HW)
    fptr = dev["fbuf"].data_ptr() + 4 * dev["off"]
    pconst = float(case.prior) if isinstance(case.prior, float) else 0.0
    tail = (dev["depth"].data_ptr(), _lib.ptr(dev["prior"]), int(case.has_prior), pconst, dev["w1p"].data_ptr(), dev["w2p"].data_ptr(),
            dev["vecs"].data_ptr(), case.B, case.P, case.HW, out.ptr, _lib.stream_ptr())
    if entry == "strided":
        bs, ps, chs = dev["fargs"] if len(dev["fargs"]) == 3 else (case.HW * dev["fargs"][0], dev["fargs"][0], 1)
        rc = L.idh_binary_mlp_strided_fwd(fptr, bs, ps, chs, case.cf, *tail)
    else:
        fn = L.idh_binary_mlp_f16x3_fwd if entry == "f16x3" else L.idh_binary_mlp_fwd
        cs = dev["fargs"][0] if len(dev["fargs"]) == 1 else dev["fargs"][1]
        rc = fn(fptr, cs, case.cf, *tail)
    torch.cuda.synchronize()
    return rc, out


def device_case(case, m, feat, depth=None, prior=None, device="cuda"):
    buf, off, fargs = feature_buffer(case, feat)
    w1p, w2p, vecs = pack_net(m, case.cf, case.has_prior, case.entry == "f16x3", device)
    return {"fbuf": buf.to(device), "off": off, "fargs": fargs, "w1p": w1p, "w2p": w2p, "vecs": vecs,
            "depth": None if depth is None else depth.contiguous().to(device), "prior": None if prior is None else prior.contiguous().to(device)}


# ------------------------------------------------------------------------------------------------------------------
# search
# ------------------------------------------------------------------------------------------------------------------
def search_inputs(case):
    """feat (B, Cf, HW), prior (B, 1, HW) | None."""
    s = _seed(case.name)
    feat = syn.randn((case.B, case.cf, case.HW), s, "feat")
    prior = torch.tanh(syn.randn((case.B, 1, case.HW), s, "prior")) if case.prior == "tensor" else None
    return feat, prior


def search_net(case):
    """The case's network: the depth column of W1 is tripled so that the logit depends visibly on the query, and b3 is shifted so that
    the fp64 logit of the first query minus its threshold has median 0 over the image - half the pixels move hi at the first step, half
    lo (decided on the reference alone, test_mlp_op_cpu.py::test_search_case_inputs checks the outcome)."""
    m = make_net(case.cf, case.has_prior, _seed(case.name), depth_gain=3.0)
    feat, prior = search_inputs(case)
    shape = (case.B, 1, case.HW)
    q0 = np.full(shape, first_query(case), dtype=np.float32)
    ref = reference_logits(weights64(m), feat, torch.from_numpy(q0), prior64(case, prior, shape))
    shift = (ref - torch.from_numpy(thresholds_at(case, q0)[0].astype(np.float64))).median().item()
    with torch.no_grad():
        m.mlps["s0"][4].bias -= shift
    return m


def table_tensors(case):
    """(bins, thr_logits) fp32 of a Thresholder case: thr_logits = log(t / (1 - t)) is the caller's transform (mlp.infer_depth)."""
    bins, thr = (torch.tensor(v, dtype=torch.float32) for v in case.table)
    return bins, torch.log(thr / (1 - thr))


def const_thr_logit(t):
    """logf(t / (1.f - t)) as the host code forms it, in numpy fp32."""
    t = np.float32(t)
    return np.log(t / (np.float32(1.0) - t), dtype=np.float32)


def thresholds_at(case, q):
    """fp32 threshold logit per pixel for the queries q (numpy fp32), and the bucket index (None for a constant)."""
    if case.table is None:
        return np.full(q.shape, const_thr_logit(case.thr), dtype=np.float32), None
    bins, tl = (t.numpy() for t in table_tensors(case))
    idx = (bins[None, :] < q.reshape(-1, 1)).sum(1).reshape(q.shape)  # torch.bucketize(right=False): edges strictly below the query
    return tl[np.minimum(idx, len(bins) - 1)], idx


def first_query(case):
    return (np.float32(case.hi) - np.float32(case.lo)) * np.float32(0.5)


def search_step(case, lo, hi, q, logit, thr):
    """One fp32 step of the rule: logit < thr moves hi, otherwise lo; next query (hi + lo) * 0.5f."""
    vis = logit < thr
    hi = np.where(vis, q, hi).astype(np.float32)
    lo = np.where(vis, lo, q).astype(np.float32)
    return lo, hi, ((hi + lo) * np.float32(0.5)).astype(np.float32)


def simulate_search(case, w, feat, prior):
    """The search with the fp64 MLP deciding (queries kept in fp32): list of per-step dicts {q, idx, vis}."""
    shape = (case.B, 1, case.HW)
    lo = np.full(shape, case.lo, dtype=np.float32)
    hi = np.full(shape, case.hi, dtype=np.float32)
    q = np.full(shape, first_query(case), dtype=np.float32)
    p64 = prior64(case, prior, shape)
    steps = []
    for _ in range(SEARCH_ITERS):
        logit = reference_logits(w, feat, torch.from_numpy(q), p64).numpy()
        thr, idx = thresholds_at(case, q)
        steps.append({"q": q.copy(), "idx": idx, "vis": logit < thr})
        lo, hi, q = search_step(case, lo, hi, q, logit, thr.astype(np.float64))
    return steps


def run_search(L, case, dev, iters):
    """One launch with the given iteration count into fresh outputs: (rc, search depths Out, last logits Out)."""
    from implicit_depth_amd import _lib

    sd, lg = Out(case.M), Out(case.M)
    fptr = dev["fbuf"].data_ptr() + 4 * dev["off"]
    cs = dev["fargs"][0]
    pconst = float(case.prior) if isinstance(case.prior, float) else 0.0
    head = (fptr, cs, case.cf, _lib.ptr(dev["prior"]), int(case.has_prior), pconst, dev["w1p"].data_ptr(), dev["w2p"].data_ptr(), dev["vecs"].data_ptr(),
            case.B, case.HW, iters, case.lo, case.hi)
    tail = (sd.ptr, lg.ptr, _lib.stream_ptr())
    bins, tl = dev.get("bins"), dev.get("thr_logits")
    if case.entry == "f16x3":
        t = 0.5 if case.table else case.thr
        rc = L.idh_binary_mlp_search_f16x3_fwd(*head, t, _lib.ptr(bins), _lib.ptr(tl), 0 if bins is None else bins.numel(), *tail)
    elif case.table:
        rc = L.idh_binary_mlp_search_thr_fwd(*head, bins.data_ptr(), tl.data_ptr(), bins.numel(), *tail)
    else:
        rc = L.idh_binary_mlp_search_fwd(*head, case.thr, *tail)
    torch.cuda.synchronize()
    return rc, sd, lg


# ------------------------------------------------------------------------------------------------------------------
# sample_prior
# ------------------------------------------------------------------------------------------------------------------
TIE_K = (16.0, 16.0, 8.0, 4.0)  # fx, fy, cx, cy: powers of two
TIE_T = (2.5 / 16.0, 1.0 / 16.0)  # camera-space translation: sx = x + 2.5 (a tie in every column), sy = y + 1


def _pinhole(fx, fy, cx, cy):
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def prior_inputs(case):
    """fp32 CPU tensors: depth (B,P,H,W), prior (B,Q,H,W), cur_world_T_cam, prior_cam_T_world, K, invK (B,4,4)."""
    s = _seed(case.name)
    B, Q, P, H, W = case.B, case.Q, case.P, case.H, case.W
    g = torch.Generator().manual_seed(s)
    prior = torch.rand((B, Q, H, W), generator=g) + torch.arange(Q).view(1, Q, 1, 1)  # in [q, q + 1): the planes hold distinct values
    eye = torch.eye(4, dtype=torch.float64)
    if case.kind in ("tie", "identity"):
        K = _pinhole(*TIE_K)
        cur = eye.clone()
        rel = eye.clone()
        if case.kind == "tie":
            rel[0, 3], rel[1, 3] = TIE_T
            depth = torch.ones(B, P, H, W)
        else:
            depth = 0.5 + 5 * torch.rand((B, P, H, W), generator=g)
            depth[:, :, ::3, 1::4] = 0.0
            depth[:, :, 1::3, ::5] = -1.5
        mats = [torch.stack([m] * B) for m in (cur, rel, K, torch.linalg.inv(K))]
        return (depth, prior) + tuple(m.float() for m in mats)
    depth = 0.5 + 5.5 * torch.rand((B, P, H, W), generator=g)
    depth[:, :, ::4, ::3] = 0.0  # zeros and negatives: -1 whatever the geometry
    depth[:, :, 1::5, 2::4] = -2.0
    cur, pcw, Ks = [], [], []
    for b in range(B):
        c = syn.source_pose(b + 2)
        rel = syn.source_pose(b)  # previous camera in the current camera's frame
        if b == B - 1:  # the last frame's previous camera looks the other way: every point with positive depth lies behind it
            rel = syn._rot_y(math.pi) @ rel
        cur.append(c)
        pcw.append(torch.linalg.inv(c @ rel))
        Ks.append(syn.intrinsics(W + 2 * b, H + b))
    K = torch.stack(Ks)
    mats = (torch.stack(cur).float(), torch.stack(pcw).float(), K.float())
    return (depth, prior) + mats + (torch.linalg.inv(K).float(),)


def prior_reference(case, depth, prior, cur, pcw, K, invK):
    """fp64 oracle.networks.sample_prior plane by plane (plane p samples channel min(p, Q - 1)): (B, P, H, W) fp64."""
    d64, args = depth.double(), [t.double() for t in (cur, pcw, K, invK)]
    outs = [onet.sample_prior(d64[:, p:p + 1], prior.double()[:, min(p, case.Q - 1)][:, None], *args) for p in range(case.P)]
    return torch.cat(outs, 1)


def prior_skip_mask(case, depth, cur, pcw, K, invK):
    """Pixels whose fp64 sample coordinate lies within delta of a rounding boundary k + 0.5 in x or y (the image border, sx = -0.5
    and sx = W - 0.5, is such a boundary too): there the kernel's fp32 coordinate may round to the other texel.  (B, P, H, W) bool.

    delta is the fp32 error of the coordinate chain of sample_prior_k, propagated in fp64 through magnitudes (u = 2^-24; an fma
    chain of n terms errs by at most n u times the sum of the magnitudes of its terms):
      T = A B, Pm = K T (4-term fma dots):    eT = 4u |A||B|,  eP = |K| eT + 4u |K||T|
      ray = invK[:3,:3] (x + .5, y + .5, 1):   e_ray = 3u |invK||pix|;   X = d ray:  eX = |d| e_ray + u |X|
      c = Pm[:, :3] X + Pm[:, 3]:              ec = eP[:, :3] |X| + |Pm[:, :3]| eX + eP[:, 3] + 4u (|Pm[:, :3]||X| + |Pm[:, 3]|)
      z = max(c_z, 1e-5) (1-Lipschitz: ez = ec_z, or the rounding of 1e-5f alone where c_z + ec_z < 1e-5), u = c_x / z:
                                               eu = (ec_x + |u| ez) / (z - ez) + u |u|
      sx = ((2 (u / W - .5) + 1) W - 1) / 2 = u - .5 with five roundings: u/W, - .5, + 1, * W, - 1, together <= 6u (|u| + W)
      delta_x = 2 (eu + 6u (|u| + W)), the factor 2 for the reference's own fp64 evaluation being compared at fp32 inputs and for
      second-order terms.  Where z - ec_z <= 0 the pixel is skipped if its depth is positive (never the case in these tables
      unless the point sits on the clamp itself).  Pixels with depth <= 0 give -1 whatever the coordinate and are never skipped."""
    B, P, H, W = depth.shape
    if case.kind == "tie":  # every operation of the chain is exact in fp32 and in fp64 (powers of two, unit depth): nothing to skip, ties included
        return torch.zeros(B, P, H, W, dtype=torch.bool)
    A, Bm, Kd, iK = (t.double() for t in (pcw, cur, K, invK))
    T = A @ Bm
    eT = 4 * U * (A.abs() @ Bm.abs())
    Pm = (Kd @ T)[:, :3]
    eP = (Kd.abs() @ eT + 4 * U * (Kd.abs() @ T.abs()))[:, :3]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)
    ray = iK[:, :3, :3] @ pix  # B, 3, N
    e_ray = 3 * U * (iK[:, :3, :3].abs() @ pix)
    skip = torch.zeros(B, P, H * W, dtype=torch.bool)
    for p in range(P):
        d = depth[:, p].double().reshape(B, 1, -1)
        X = ray * d
        eX = d.abs() * e_ray + U * X.abs()
        c = Pm[:, :, :3] @ X + Pm[:, :, 3:4]
        ec = eP[:, :, :3] @ X.abs() + Pm[:, :, :3].abs() @ eX + eP[:, :, 3:4] + 4 * U * (Pm[:, :, :3].abs() @ X.abs() + Pm[:, :, 3:4].abs())
        z = c[:, 2].clamp_min(1e-5)
        ez = torch.where(c[:, 2] + ec[:, 2] < 1e-5, U * 1e-5 * torch.ones_like(z), ec[:, 2])  # well behind the camera both sides clamp to the same 1e-5f
        den = z - ez
        bad = den <= 0
        den = den.clamp_min(1e-30)
        near = torch.zeros(B, H * W, dtype=torch.bool)
        for ax, size in ((0, W), (1, H)):
            uu = c[:, ax] / z
            eu = (ec[:, ax] + uu.abs() * ez) / den + U * uu.abs()
            delta = 2 * (eu + 6 * U * (uu.abs() + size))
            s = uu - 0.5
            dist = ((s - 0.5) - torch.round(s - 0.5)).abs()  # distance of s to the nearest k + 0.5
            near |= (dist <= delta) & (s > -1.5 - delta) & (s < size + 0.5 + delta)  # far outside the image every candidate texel is out of range
        skip[:, p] = (near | bad) & (d[:, 0] > 0)
    return skip.view(B, P, H, W)


def run_sample_prior(L, case, dev):
    from implicit_depth_amd import _lib

    out = Out(case.B * case.P * case.H * case.W)
    depth, prior, cur, pcw, K, invK = dev
    rc = L.idh_sample_prior_fwd(depth.data_ptr(), prior.data_ptr(), case.Q, cur.data_ptr(), pcw.data_ptr(), K.data_ptr(), invK.data_ptr(),
                                case.B, case.P, case.H, case.W, out.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------------------------
# packers
# ------------------------------------------------------------------------------------------------------------------
def pack_source(n_in, col0, ld, seed):
    """(128, ld) fp32 with NaN outside columns [col0, col0 + n_in); row magnitudes spread over several binades."""
    w = torch.full((HID, ld), NAN)
    vals = syn.randn((HID, n_in), seed, "packw") * torch.exp2(torch.arange(HID, dtype=torch.float32) % 7 - 3).view(HID, 1)
    w[:, col0: col0 + n_in] = vals
    return w


def packed_fragment_order(w, col0, n_in):
    """numpy statement of idh_pack_mlp_weight: dst[c][i][lane][e] = W[16 i + (lane & 15)][col0 + 16 c + 4 (lane >> 4) + e], zero for k >= n_in."""
    w = w.numpy()
    cb = (n_in + 15) // 16
    dst = np.zeros((cb, 8, 64, 4), dtype=np.float32)
    for c in range(cb):
        for i in range(8):
            for lane in range(64):
                for e in range(4):
                    k = 16 * c + 4 * (lane >> 4) + e
                    if k < n_in:
                        dst[c, i, lane, e] = w[16 * i + (lane & 15), col0 + k]
    return dst


def decode_f16_pack(raw_bytes, n_in):
    """idh_pack_mlp_weight_f16's blob -> (hi, lo) as (128, 32 nb32) fp64 in logical [row][k] order, and the 128 row scales (fp32).
    Layout [nb32][8 i][2 piece][64 lane][8 halves]: half e of lane (ln, q) is k = 32 c + 16 (e >> 2) + 4 q + (e & 3), row 16 i + ln."""
    nb = (n_in + 31) // 32
    body = nb * 8 * 2 * 64 * 8
    halves = np.frombuffer(raw_bytes[: body * 2], dtype=np.float16).reshape(nb, 8, 2, 64, 8).astype(np.float64)
    scales = np.frombuffer(raw_bytes[body * 2: body * 2 + HID * 4], dtype=np.float32)
    pieces = np.zeros((2, HID, 32 * nb))
    for c in range(nb):
        for i in range(8):
            for lane in range(64):
                for e in range(8):
                    k = 32 * c + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3)
                    pieces[:, 16 * i + (lane & 15), k] = halves[c, i, :, lane, e]
    return pieces[0], pieces[1], scales
