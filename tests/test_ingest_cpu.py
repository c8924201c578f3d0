"""CPU-side checks of the frame ingest (include/idh_ingest.h, implicit_depth_amd/ingest.py): the numpy restatement (tests/ingest_ref.py)
against the goldens Pillow and torch wrote (tests/golden/g_ingest.npz) and, where Pillow is importable, against Pillow itself; the
host-only coefficient entry points against the restatement; the intrinsics pyramid; refusals before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ingest_ref as ref
from conftest import ROOT

FILTERS = sorted(ref.FILTER_NAMES)
# every (source, target) length pair of the colour cases, per dimension, plus ARKit's and the largest supported camera frame
DIMS = sorted({(s[i], d[i]) for _, s, d in ref.COLOR_CASES for i in (0, 1)} | {(1920, 512), (1440, 384), (4032, 512), (3024, 384), (1, 1), (1, 5), (8, 1)})


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_ingest.npz")))


@pytest.mark.parametrize("fname", FILTERS)
@pytest.mark.parametrize("case", ref.COLOR_CASES, ids=[c[0] for c in ref.COLOR_CASES])
def test_ref_equals_golden_colour(golden, case, fname):
    name, src, dst = case
    x = golden[f"{name}_in"]
    assert x.shape == (3,) + src + (3,) and np.array_equal(x, ref.color_input(name, src, 100 + ref.COLOR_CASES.index(case)))
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])  # different content per frame
    img, u8 = ref.load_color(x, dst, ref.FILTER_NAMES[fname])
    assert np.array_equal(u8, golden[f"{name}_{fname}_u8"])
    c = np.arange(3)[None, :, None, None]
    assert np.array_equal(img, golden["normalize_table"][c, np.moveaxis(u8, 3, 1)])
    assert np.array_equal(ref.load_color(x, dst, ref.FILTER_NAMES[fname], normalise=False)[0], golden["to_tensor_table"][c, np.moveaxis(u8, 3, 1)])


@pytest.mark.parametrize("fname", FILTERS)
def test_ref_equals_live_pillow(golden, fname):
    Image = pytest.importorskip("PIL.Image")
    pf = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[fname]
    for name, src, dst in ref.COLOR_CASES:
        if src == dst:
            continue
        x = golden[f"{name}_in"][0]
        assert np.array_equal(np.asarray(Image.fromarray(x).resize((dst[1], dst[0]), resample=pf)), ref.resize_u8(x, dst, ref.FILTER_NAMES[fname])), name
    for name, src, dst in ref.DEPTH_CASES:
        if dst is not None:
            d = golden[f"{name}_in"][0]
            got = d[ref.nearest_index(src[0], dst[0])][:, ref.nearest_index(src[1], dst[1])]
            assert np.array_equal(np.asarray(Image.fromarray(d).resize((dst[1], dst[0]), resample=Image.NEAREST)), got), name


def test_clipping_cases_hit_both_ends_after_each_pass(golden):
    """The checkerboard and the stripes over- and undershoot: the unclipped sums of the first pass leave 0..255 on both sides, and so do
    those of the second pass run on the clipped bytes."""
    for name in ("checker", "stripes"):
        _, src, dst = next(c for c in ref.COLOR_CASES if c[0] == name)
        x = golden[f"{name}_in"]
        lo1 = hi1 = lo2 = hi2 = False
        for f in x:
            wide1 = ref._pass(f, *ref.coeffs(src[1], dst[1], ref.BICUBIC), axis=1, wide=True)
            mid = np.clip(wide1, 0, 255).astype(np.uint8)
            wide2 = ref._pass(mid, *ref.coeffs(src[0], dst[0], ref.BICUBIC), axis=0, wide=True)
            lo1, hi1, lo2, hi2 = lo1 or wide1.min() < 0, hi1 or wide1.max() > 255, lo2 or wide2.min() < 0, hi2 or wide2.max() > 255
        assert lo1 and hi1 and lo2 and hi2, (name, lo1, hi1, lo2, hi2)


def test_wide_intermediate_case_differs(golden):
    """ref.WIDE_INTERMEDIATE_CASE is the case the GPU test names: keeping the first pass wider than uint8 changes its result."""
    name, fname = ref.WIDE_INTERMEDIATE_CASE
    _, src, dst = next(c for c in ref.COLOR_CASES if c[0] == name)
    wide = np.stack([ref.resize_u8_wide_intermediate(f, dst, ref.FILTER_NAMES[fname]) for f in golden[f"{name}_in"]])
    assert not np.array_equal(wide, golden[f"{name}_{fname}_u8"])


@pytest.mark.parametrize("case", ref.DEPTH_CASES, ids=[c[0] for c in ref.DEPTH_CASES])
def test_ref_equals_golden_depth(golden, case):
    name, src, dst = case
    d = golden[f"{name}_in"]
    assert all((d == v).any() for v in ref.DEPTH_SPECIALS)
    depth, mask, mask_b = ref.load_depth(d, dst)
    assert np.array_equal(depth, golden[f"{name}_depth"], equal_nan=True) and np.array_equal(np.isnan(depth), ~golden[f"{name}_mask_b"])
    assert np.array_equal(mask, golden[f"{name}_mask"]) and np.array_equal(mask_b, golden[f"{name}_mask_b"])
    assert mask_b.any() and not mask_b.all()


@pytest.mark.parametrize("fname", FILTERS)
def test_coeffs_pack_equals_ref(fname):
    from implicit_depth_amd import ingest

    for n_in, n_out in DIMS:
        if n_in == n_out:
            continue
        bounds, taps = ingest.resize_coeffs(n_in, n_out, fname)
        rb, rt = ref.coeffs(n_in, n_out, ref.FILTER_NAMES[fname])
        assert bounds.dtype == np.int32 and taps.dtype == np.int32 and taps.shape == (n_out, ref.ksize(n_in, n_out, ref.FILTER_NAMES[fname]))
        assert np.array_equal(bounds, rb) and np.array_equal(taps, rt), (n_in, n_out)
        assert taps.shape[1] <= 33 and int(np.abs(taps.astype(np.int64)).sum(1).max()) < 1 << 23  # int32 sums cannot overflow


def test_coeffs_entry_points_refuse():
    from implicit_depth_amd import _lib, ingest

    L = _lib.lib()
    nb, nt = C.c_int64(), C.c_int64()
    assert L.idh_resize_coeffs_sizes(64, 8, 1, C.byref(nb), C.byref(nt)) == 0 and (nb.value, nt.value) == (16, 8 * 33)
    assert L.idh_resize_coeffs_sizes(65, 8, 1, C.byref(nb), C.byref(nt)) == -2  # ratio above 8
    assert L.idh_resize_coeffs_sizes(0, 8, 1, C.byref(nb), C.byref(nt)) == -1 and L.idh_resize_coeffs_sizes(8, 0, 1, C.byref(nb), C.byref(nt)) == -1
    assert L.idh_resize_coeffs_sizes(16, 8, 2, C.byref(nb), C.byref(nt)) == -1 and L.idh_resize_coeffs_sizes(16, 8, 1, None, C.byref(nt)) == -1
    buf = np.zeros(64, np.int32)
    assert L.idh_resize_coeffs_pack(16, 8, 0, None, buf.ctypes.data) == -1 and L.idh_resize_coeffs_pack(65, 8, 0, buf.ctypes.data, buf.ctypes.data) == -2
    with pytest.raises(_lib.IdhError):
        ingest.resize_coeffs(65, 8, "bicubic")
    with pytest.raises(_lib.IdhError):
        ingest.resize_coeffs(16, 8, "lanczos")


def _color_args(**over):
    from implicit_depth_amd import _lib

    a = _lib.IngestColorArgs()
    a.frames_bHW3, a.x_bounds, a.x_taps, a.y_bounds, a.y_taps, a.image_b3hw = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    a.filter, a.normalize, a.B, a.Hs, a.Ws, a.h, a.w = 1, 1, 0, 37, 53, 24, 32
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_color_entry_validates_before_launching():
    """B = 0 everywhere a request is well formed: nothing is launched on the fake addresses."""
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_ingest_color_args() == C.sizeof(_lib.IngestColorArgs) == _lib.IngestColorArgs().struct_size
    call = lambda a: L.idh_ingest_color_fwd(C.byref(a), None)
    assert L.idh_ingest_color_fwd(None, None) == -1
    assert call(_color_args()) == 0
    assert call(_color_args(struct_size=C.sizeof(_lib.IngestColorArgs) - 8)) == -1 and call(_color_args(struct_size=C.sizeof(_lib.IngestColorArgs) + 8)) == 0
    assert call(_color_args(frames_bHW3=None)) == -1 and call(_color_args(image_b3hw=None)) == -1  # no output at all
    assert call(_color_args(image_b3hw=None, resized_bhw3=0x7000)) == 0
    for k in ("Hs", "Ws", "h", "w"):
        assert call(_color_args(**{k: 0})) == -1, k
    assert call(_color_args(B=-1)) == -1 and call(_color_args(filter=2)) == -1
    for k in ("x_bounds", "x_taps", "y_bounds", "y_taps"):  # a table is missing for a dimension that changes
        assert call(_color_args(**{k: None})) == -1, k
    assert call(_color_args(Hs=24)) == -1  # ... or given for one that does not
    assert call(_color_args(Hs=24, y_bounds=None, y_taps=None)) == 0
    assert call(_color_args(Hs=24, Ws=32, x_bounds=None, x_taps=None, y_bounds=None, y_taps=None)) == 0  # no resize at all
    assert call(_color_args(Hs=24 * 8 + 1)) == -2 and call(_color_args(Ws=32 * 8 + 1)) == -2 and call(_color_args(Hs=24 * 8, Ws=32 * 8)) == 0
    assert call(_color_args(B=70000)) == -2


def test_depth_entry_validates_before_launching():
    from implicit_depth_amd import _lib

    L = _lib.lib()
    assert L.idh_sizeof_ingest_depth_args() == C.sizeof(_lib.IngestDepthArgs) == _lib.IngestDepthArgs().struct_size

    def call(**over):
        a = _lib.IngestDepthArgs()
        a.depth_bHW, a.depth_b1hw, a.mask_b1hw, a.mask_b_b1hw = 0x1000, 0x2000, 0x3000, 0x4000
        a.value_scale, a.min_valid, a.max_valid, a.B, a.Hs, a.Ws, a.h, a.w = 1e-3, 1e-3, 10.0, 0, 48, 64, 24, 32
        for k, v in over.items():
            setattr(a, k, v)
        return L.idh_ingest_depth_fwd(C.byref(a), None)

    assert L.idh_ingest_depth_fwd(None, None) == -1
    assert call() == 0 and call(struct_size=8) == -1
    assert call(depth_bHW=None) == -1 and call(mask_b1hw=None) == -1 and call(h=0) == -1 and call(Ws=0) == -1 and call(B=-1) == -1
    assert call(depth_b1hw=None, mask_b1hw=None, mask_b_b1hw=None) == -1  # no triple requested
    full = dict(full_depth_b1HW=0x5000, full_mask_b1HW=0x6000, full_mask_b_b1HW=0x7000)
    assert call(**full) == 0 and call(depth_b1hw=None, mask_b1hw=None, mask_b_b1hw=None, h=0, w=0, **full) == 0
    assert call(full_depth_b1HW=0x5000) == -1
    assert call(B=2, Hs=32768, Ws=32768) == -2


def test_intrinsics_pyramid_equals_restated_maths():
    from implicit_depth_amd import ingest

    rng = np.random.default_rng(5)
    K = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    K[:, 0, 0], K[:, 1, 1] = 570 + 20 * rng.random(3), 575 + 20 * rng.random(3)
    K[:, 0, 2], K[:, 1, 2] = 318 + 5 * rng.random(3), 241 + 5 * rng.random(3)
    for Kin in (K, K[0], torch.from_numpy(K)):
        got = ingest.intrinsics_pyramid(Kin, (480, 640), (192, 256), include_full_depth_K=True)
        want = ref.intrinsics_pyramid(K if np.ndim(Kin) == 3 else K[:1], (480, 640), (192, 256), include_full_depth_K=True)
        assert sorted(got) == sorted(want) and len(got) == 12
        for k, v in got.items():
            assert v.dtype == np.float32 and np.array_equal(v.reshape(-1, 4, 4), want[k]), k
    assert "K_full_depth_b44" not in ingest.intrinsics_pyramid(K, (480, 640), (192, 256))
    s0 = ingest.intrinsics_pyramid(K, (480, 640), (192, 256))["K_s0_b44"]
    assert np.array_equal(s0[:, 0], K[:, 0] * np.float32(256 / 640)) and np.array_equal(s0[:, 1], K[:, 1] * np.float32(192 / 480))


def test_python_functions_refuse_what_the_kernels_cannot_take():
    from implicit_depth_amd import _lib, ingest
    import implicit_depth_amd

    assert implicit_depth_amd.FrameIngest is ingest.FrameIngest and implicit_depth_amd.load_color is ingest.load_color
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_lib.IdhError):  # CPU tensors
        ingest.load_color(img, (4, 4))
    with pytest.raises(_lib.IdhError):
        ingest.load_depth(torch.zeros(1, 8, 8, dtype=torch.uint16))
    with pytest.raises(_lib.IdhError):
        ingest.FrameIngest((4, 4), (2, 2))(img, np.eye(4)[None], np.eye(4))
    with pytest.raises(_lib.IdhError):
        ingest.FrameIngest((4, 4), (2, 2), resample="nearest")
    with pytest.raises(_lib.IdhError):
        ingest.FrameIngest((4, 0), (2, 2))
    with pytest.raises(_lib.IdhError):
        ingest.intrinsics_pyramid(np.eye(3), (8, 8), (4, 4))
