"""ctypes binding of lib/libidh.so (the C ABI in include/idh.h).

There is deliberately NO fallback: if the library is missing or a call fails the product
path raises.  ``import torch`` happens before the CDLL load so that libidh.so's
``libamdhip64.so.7`` dependency resolves to the HIP runtime PyTorch-ROCm already mapped
(one runtime per process: device pointers and streams are then interchangeable).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# IDH_LIB: developer override used by the ablation builds of tools/abl_split.sh
LIB_PATH = os.environ.get("IDH_LIB") or os.path.join(_HERE, "lib", "libidh.so")

_lib = None
MIN_ABI_VERSION = 112

f32p = C.c_void_p  # device pointers travel as integers


class IdhError(RuntimeError):
    pass


class VolumeOpts(C.Structure):
    """ctypes mirror of ``idh_volume_opts`` (include/idh.h)."""

    _fields_ = [("cur_batch_stride", C.c_int64), ("src_batch_stride", C.c_int64), ("planes", C.c_void_p),
                ("planes_batch_stride", C.c_int64), ("planes_plane_stride", C.c_int64), ("planes_pixel_stride", C.c_int32),
                ("kernel", C.c_int32), ("scratch", C.c_void_p), ("scratch_floats", C.c_int64), ("struct_size", C.c_int64),
                ("fv_keep_empty_views", C.c_int32), ("win_units_per_split", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(VolumeOpts)


CV_KERNEL_LANE, CV_KERNEL_QUAD, CV_KERNEL_WINDOW = 1, 2, 3  # IDH_CV_KERNEL_* of include/idh.h


class EvalArgs(C.Structure):
    """ctypes mirror of ``idh_eval_args`` (include/idh.h, fused per-frame test evaluation)."""

    _fields_ = [("struct_size", C.c_int64), ("prediction", C.c_void_p), ("pred_kind", C.c_int32), ("sampling", C.c_int32),
                ("sigmoid_multiplier", C.c_float), ("surface_threshold", C.c_float), ("rendered_bphw", C.c_void_p), ("depth_b1hw", C.c_void_p),
                ("gt_b1HW", C.c_void_p), ("thresholds", C.c_void_p), ("bins", C.c_void_p), ("T", C.c_int32), ("n_bins", C.c_int32),
                ("tag_mask", C.c_int32), ("B", C.c_int32), ("P", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(EvalArgs)


EVAL_PRED_LOGITS, EVAL_PRED_DEPTH = 0, 1  # IDH_EVAL_PRED_*
EVAL_BILINEAR, EVAL_NEAREST = 0, 1  # IDH_EVAL_BILINEAR / IDH_EVAL_NEAREST
EVAL_TAG_ALL, EVAL_TAG_SURFACE, EVAL_TAG_BOUNDARY = 1, 2, 4  # IDH_EVAL_TAG_*


class CompositeArgs(C.Structure):
    """ctypes mirror of ``idh_composite_args`` (include/idh_composite.h, AR compositing)."""

    _fields_ = [("struct_size", C.c_int64), ("image_bHW3", C.c_void_p), ("virtual_rgba_bHW4", C.c_void_p), ("map_b1hw", C.c_void_p),
                ("virtual_depth_bHW", C.c_void_p), ("fade_b", C.c_void_p), ("out_bHW3", C.c_void_p), ("matte_out_bHW", C.c_void_p),
                ("plane_distance", C.c_double), ("colour", C.c_double * 3), ("sigmoid_multiplier", C.c_float), ("mode", C.c_int32),
                ("has_colour", C.c_int32), ("has_plane", C.c_int32), ("bgr", C.c_int32), ("B", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(CompositeArgs)


COMPOSITE_MASK_LOGITS, COMPOSITE_MASK_PROB, COMPOSITE_DEPTH_SOFT, COMPOSITE_DEPTH_HARD = 0, 1, 2, 3  # IDH_COMPOSITE_*


class IngestColorArgs(C.Structure):
    """ctypes mirror of ``idh_ingest_color_args`` (include/idh_ingest.h, frame ingest)."""

    _fields_ = [("struct_size", C.c_int64), ("frames_bHW3", C.c_void_p), ("x_bounds", C.c_void_p), ("x_taps", C.c_void_p), ("y_bounds", C.c_void_p),
                ("y_taps", C.c_void_p), ("image_b3hw", C.c_void_p), ("resized_bhw3", C.c_void_p), ("filter", C.c_int32), ("normalize", C.c_int32),
                ("B", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(IngestColorArgs)


class IngestDepthArgs(C.Structure):
    """ctypes mirror of ``idh_ingest_depth_args`` (include/idh_ingest.h)."""

    _fields_ = [("struct_size", C.c_int64), ("depth_bHW", C.c_void_p), ("depth_b1hw", C.c_void_p), ("mask_b1hw", C.c_void_p),
                ("mask_b_b1hw", C.c_void_p), ("full_depth_b1HW", C.c_void_p), ("full_mask_b1HW", C.c_void_p), ("full_mask_b_b1HW", C.c_void_p),
                ("value_scale", C.c_float), ("min_valid", C.c_float), ("max_valid", C.c_float), ("B", C.c_int32), ("Hs", C.c_int32),
                ("Ws", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(IngestDepthArgs)


class Bank(C.Structure):
    """ctypes mirror of ``idh_bank`` (include/idh_bank.h, keyframe feature bank)."""

    _fields_ = [("struct_size", C.c_int64), ("feats", C.c_void_p), ("mats", C.c_void_p), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("C", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(Bank)


BANK_MAX_SLOTS, BANK_MAX_VIEWS = 64, 1024  # IDH_BANK_MAX_*


class NormalsArgs(C.Structure):
    """ctypes mirror of ``idh_normals_args`` (include/idh_geometry.h, surface normals from depth)."""

    _fields_ = [("struct_size", C.c_int64), ("depth_b1hw", C.c_void_p), ("invK_b44", C.c_void_p), ("world_R_cam_b33", C.c_void_p),
                ("flags_b1hw", C.c_void_p), ("normals_b3hw", C.c_void_p), ("valid_b1hw", C.c_void_p), ("smoothing_std", C.c_float),
                ("kernel_size", C.c_int32), ("orient", C.c_int32), ("need", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(NormalsArgs)


class PatchNormalsArgs(C.Structure):
    """ctypes mirror of ``idh_patch_normals_args`` (include/idh_geometry.h)."""

    _fields_ = [("struct_size", C.c_int64), ("points_bn93", C.c_void_p), ("cam_centre_b3", C.c_void_p), ("flags_bn9", C.c_void_p),
                ("normals_bn3", C.c_void_p), ("valid_bn", C.c_void_p), ("orient", C.c_int32), ("need", C.c_int32), ("B", C.c_int32),
                ("N", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(PatchNormalsArgs)


class RasterShadedArgs(C.Structure):
    """ctypes mirror of ``idh_raster_shaded_args`` (include/idh_raster.h, shaded mesh render)."""

    _fields_ = [("struct_size", C.c_int64), ("verts_v3", C.c_void_p), ("faces_f3", C.c_void_p), ("cam_T_world_b44", C.c_void_p), ("K_b44", C.c_void_p),
                ("colors_v4", C.c_void_p), ("attrs_vc", C.c_void_p), ("depth_b1hw", C.c_void_p), ("pix_to_face_bhw", C.c_void_p),
                ("bary_bhw3", C.c_void_p), ("attr_out_bhwc", C.c_void_p), ("rgba_bhw4", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("ambient", C.c_float), ("empty_depth", C.c_float), ("V", C.c_int32), ("F", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(RasterShadedArgs)


RASTER_MAX_ATTRS = 16  # channels of idh_raster_shaded_args.attrs_vc


class DepthWarpArgs(C.Structure):
    """ctypes mirror of ``idh_depth_warp_args`` (include/idh_raster.h, depth reprojection)."""

    _fields_ = [("struct_size", C.c_int64), ("depth_m1hw", C.c_void_p), ("src_invK_m44", C.c_void_p), ("cam_T_src_bm44", C.c_void_p),
                ("K_b44", C.c_void_p), ("depth_b1hw", C.c_void_p), ("source_bhw", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("tear_ratio", C.c_float), ("empty_depth", C.c_float), ("B", C.c_int32), ("M", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(DepthWarpArgs)


class TsdfVolume(C.Structure):
    """ctypes mirror of ``idh_tsdf_volume`` (include/idh_fusion.h, TSDF fusion)."""

    _fields_ = [("struct_size", C.c_int64), ("values", C.c_void_p), ("block_flags", C.c_void_p), ("block_flag_bytes", C.c_int64),
                ("origin", C.c_float * 3), ("voxel_size", C.c_float), ("trunc_voxels", C.c_float), ("Nz", C.c_int32), ("Ny", C.c_int32),
                ("Nx", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfVolume)


class TsdfIntegrateArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_integrate_args`` (include/idh_fusion.h)."""

    _fields_ = [("struct_size", C.c_int64), ("volume", TsdfVolume), ("depth_m1hw", C.c_void_p), ("K_m44", C.c_void_p),
                ("cam_T_world_m44", C.c_void_p), ("max_weight", C.c_float), ("M", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfIntegrateArgs)


class TsdfRaycastArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_raycast_args`` (include/idh_fusion.h)."""

    _fields_ = [("struct_size", C.c_int64), ("volume", TsdfVolume), ("world_T_cam_b44", C.c_void_p), ("invK_b44", C.c_void_p),
                ("depth_b1hw", C.c_void_p), ("flags_bhw", C.c_void_p), ("normals_b3hw", C.c_void_p), ("near", C.c_float),
                ("step_voxels", C.c_float), ("empty_depth", C.c_float), ("max_steps", C.c_int32), ("world_normals", C.c_int32),
                ("skip", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfRaycastArgs)


class TsdfMeshArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_mesh_args`` (include/idh_fusion.h, mesh extraction)."""

    _fields_ = [("struct_size", C.c_int64), ("volume", TsdfVolume), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("totals", C.c_void_p), ("verts_v3", C.c_void_p), ("faces_f3", C.c_void_p), ("weights_v", C.c_void_p),
                ("vert_capacity", C.c_int64), ("face_capacity", C.c_int64), ("min_weight", C.c_float), ("use_block_flags", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfMeshArgs)


class TsdfIntegrateColorArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_integrate_color_args`` (include/idh_fusion.h, TSDF colour)."""

    _fields_ = TsdfIntegrateArgs._fields_ + [("colors_zyx4", C.c_void_p), ("color_mhw3", C.c_void_p), ("color_K_m44", C.c_void_p),
                                             ("hc", C.c_int32), ("wc", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfIntegrateColorArgs)


class TsdfRaycastColorArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_raycast_color_args`` (include/idh_fusion.h)."""

    _fields_ = TsdfRaycastArgs._fields_ + [("colors_zyx4", C.c_void_p), ("rgba_bhw4", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfRaycastColorArgs)


class TsdfMeshColorsArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_mesh_colors_args`` (include/idh_fusion.h)."""

    _fields_ = [("struct_size", C.c_int64), ("mesh", TsdfMeshArgs), ("colors_zyx4", C.c_void_p), ("rgba_v4", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfMeshColorsArgs)
        self.mesh.struct_size = C.sizeof(TsdfMeshArgs)


class TsdfIntegrateWeightedArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_integrate_weighted_args`` (include/idh_fusion.h, per-observation weights)."""

    _fields_ = TsdfIntegrateColorArgs._fields_ + [("weight_m1hw", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfIntegrateWeightedArgs)


class TsdfShiftArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_shift_args`` (include/idh_fusion.h, a volume that follows the camera)."""

    _fields_ = [("struct_size", C.c_int64), ("src", TsdfVolume), ("dst", TsdfVolume), ("src_colors_zyx4", C.c_void_p),
                ("dst_colors_zyx4", C.c_void_p), ("shift", C.c_int32 * 3)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfShiftArgs)


class TsdfAlignArgs(C.Structure):
    """ctypes mirror of ``idh_tsdf_align_args`` (include/idh_fusion.h, pose alignment against the volume)."""

    _fields_ = [("struct_size", C.c_int64), ("volume", TsdfVolume), ("depth_11hw", C.c_void_p), ("invK_44", C.c_void_p),
                ("weight_11hw", C.c_void_p), ("world_T_cam_in_44", C.c_void_p), ("world_T_cam_out_44", C.c_void_p), ("records_i40", C.c_void_p),
                ("rows_hw8", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("damping", C.c_double),
                ("min_step", C.c_double), ("min_pivot_ratio", C.c_double), ("huber", C.c_float), ("h", C.c_int32), ("w", C.c_int32),
                ("iters", C.c_int32), ("stride", C.c_int32), ("min_count", C.c_int32), ("max_workgroups", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TsdfAlignArgs)
        self.volume.struct_size = C.sizeof(TsdfVolume)


class MvConsistencyArgs(C.Structure):
    """ctypes mirror of ``idh_mv_consistency_args`` (include/idh_geometry.h, multi-view depth consistency)."""

    _fields_ = [("struct_size", C.c_int64), ("depth_b1hw", C.c_void_p), ("gate_depth_b1hw", C.c_void_p), ("invK_b44", C.c_void_p),
                ("world_T_cam_b44", C.c_void_p), ("src_depth_bk1hw", C.c_void_p), ("src_K_bk44", C.c_void_p), ("src_cam_T_world_bk44", C.c_void_p),
                ("counts_b3hw", C.c_void_p), ("weight_b1hw", C.c_void_p), ("filtered_depth_b1hw", C.c_void_p), ("visible_bkhw", C.c_void_p),
                ("err_bkhw", C.c_void_p), ("loss", C.c_void_p), ("loss_sum_k", C.c_void_p), ("loss_count_k", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("ratio", C.c_float), ("log_tol", C.c_float), ("min_consistent", C.c_int32),
                ("max_conflict", C.c_int32), ("B", C.c_int32), ("K", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("src_h", C.c_int32),
                ("src_w", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(MvConsistencyArgs)


class EdgeMaskArgs(C.Structure):
    """ctypes mirror of ``idh_edge_mask_args`` (include/idh_geometry.h, edge mask of a depth map)."""

    _fields_ = [("struct_size", C.c_int64), ("depth_b1hw", C.c_void_p), ("mask_b1hw", C.c_void_p), ("sobel_b1hw", C.c_void_p),
                ("threshold_b", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("q", C.c_float), ("dilate", C.c_int32),
                ("mask_u8", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(EdgeMaskArgs)


class BdValLossesArgs(C.Structure):
    """ctypes mirror of ``idh_bd_val_losses_args`` (include/idh_geometry.h, BDModel's validation losses)."""

    _fields_ = [("struct_size", C.c_int64), ("pred_bdhw", C.c_void_p), ("rendered_bdhw", C.c_void_p), ("depth_b1hw", C.c_void_p),
                ("edge_mask_b1hw", C.c_void_p), ("out5", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("bd_regularisation_weight", C.c_float), ("positive_weight", C.c_float), ("max_workgroups", C.c_int32), ("B", C.c_int32),
                ("D", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(BdValLossesArgs)


class RegValLossesArgs(C.Structure):
    """ctypes mirror of ``idh_reg_val_losses_args`` (include/idh_geometry.h, DepthModel's validation losses)."""

    _fields_ = [("struct_size", C.c_int64), ("depth_gt_b1hw", C.c_void_p), ("depth_pred_b1hw", C.c_void_p), ("mask_b_b1hw", C.c_void_p),
                ("log_depth_pred_s", C.c_void_p * 4), ("normals_gt_b3hw", C.c_void_p), ("normals_pred_b3hw", C.c_void_p), ("mv_loss", C.c_void_p),
                ("out16", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("si_lambda", C.c_float),
                ("hypersim", C.c_int32), ("num_scales", C.c_int32), ("terms", C.c_int32), ("max_workgroups", C.c_int32), ("B", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("scale_h", C.c_int32 * 4), ("scale_w", C.c_int32 * 4)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(RegValLossesArgs)


REG_TERM_GRAD, REG_TERM_POINT, REG_TERM_NORMALS = 1, 2, 4  # IDH_REG_TERM_*
MV_MAX_SOURCES, MV_MAX_MAPS = 16, 128  # IDH_MV_MAX_*
TSDF_MAX_MAPS, TSDF_MAX_CAMERAS, TSDF_MAX_STEPS = 16, 128, 65536  # IDH_TSDF_MAX_*
TSDF_HIT, TSDF_NONE_KNOWN, TSDF_SOME_KNOWN, TSDF_NO_NORMAL = 1, 2, 4, 8  # IDH_TSDF_* flag bits

RESIZE_BILINEAR, RESIZE_BICUBIC = 0, 1  # IDH_RESIZE_*
INGEST_MAX_RATIO = 8  # IDH_INGEST_MAX_RATIO


class ConvDescSrc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "cs", "Cin", "ks", "stride", "is_cat", "_r")]


class ConvDesc(C.Structure):
    """ctypes mirror of ``idh_conv_desc`` (include/idh_ops.h, kernel selection of one conv)."""

    _fields_ = ([(n, C.c_int32) for n in ("N", "Ho", "Wo", "Cout", "pad_mode", "act")] + [("slope", C.c_float)] +
                [(n, C.c_int32) for n in ("out_cs", "res_cs", "has_res", "has_norm", "any_size", "math", "n_src")] + [("src", ConvDescSrc * 2)])


class ConvTuning(C.Structure):
    """ctypes mirror of ``idh_conv_tuning``: the field names are the lower-case names of nhwc.py's module globals."""

    _fields_ = ([(n, C.c_int32) for n in ("winograd", "winograd4", "winograd4_proj", "s2_first", "wino_min_tiles", "wino4_min_tiles", "split_min_blocks",
                                          "narrow_tile_below", "narrowest_tile_below", "split_min_chunks", "split_max", "s2_first_min_blocks",
                                          "fused_up_rows", "target_waves", "min_waves", "_r")] +
                [(n, C.c_double) for n in ("wino_min_fill", "wino4_min_fill", "proj_chunk_weight")])


class ConvChoice(C.Structure):
    """ctypes mirror of ``idh_conv_choice``."""

    _fields_ = [(n, C.c_int32) for n in ("tile_m", "tile_n", "split_k", "w_layout", "families", "lds_tile_m", "lds_split_k", "lds_subtiles", "split_rows",
                                         "direct_tile_m", "direct_tile_n", "direct_split_k")]


# idh_plan_observer of include/idh_net.h: (ops, n, n_first, order, ws, ws_floats, blob, blob_floats, user); ops = n nhwc.Op descriptors
PlanObserver = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p)

_SIGS = {
    "idh_version": (C.c_int, []),
    "idh_debug_set_plan_observer": (None, [PlanObserver, C.c_void_p]),
    "idh_sizeof_volume_opts": (C.c_size_t, []),
    "idh_cost_volume_dot_scratch_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "idh_cost_volume_dot_plan": (C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "idh_error_string": (C.c_char_p, [C.c_int]),
    "idh_nchw_to_nhwc_f32": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "idh_nhwc_to_nchw_f32": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "idh_packed_weight_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "idh_pack_conv_weight": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "idh_packed_split_weight_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "idh_pack_conv_weight_split": (C.c_int, [f32p, f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "idh_packed_wino_weight_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "idh_pack_conv_weight_wino": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_void_p]),
    "idh_packed_wino4_weight_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "idh_pack_conv_weight_wino4": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_void_p]),
    "idh_stem_weight_floats": (C.c_size_t, []),
    "idh_pack_stem_weight": (C.c_int, [f32p] * 5 + [C.c_float, f32p, C.c_void_p]),
    "idh_fold_conv_bn": (C.c_int, [f32p, C.c_int, C.c_int] + [f32p] * 4 + [C.c_float, f32p, f32p, C.c_void_p]),
    "idh_sizeof_op": (C.c_size_t, []),
    "idh_run_ops": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "idh_count_launches": (C.c_int, [C.c_void_p, C.c_int]),
    "idh_conv_variant": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "idh_conv_tuning_defaults": (None, [C.POINTER(ConvTuning)]),
    "idh_conv_select": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvTuning), C.POINTER(ConvChoice)]),
    "idh_sizeof_conv_select": (None, [C.POINTER(C.c_size_t)]),
    "idh_schedule_ops": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "idh_packed_mlp_weight_floats": (C.c_size_t, [C.c_int]),
    "idh_pack_mlp_weight": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "idh_binary_mlp_fwd": (C.c_int, [f32p, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "idh_binary_mlp_strided_fwd": (C.c_int, [f32p, C.c_longlong, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "idh_binary_mlp_f16x3_fwd": (C.c_int, [f32p, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "idh_feature_volume_workspace_bytes": (C.c_size_t, [C.c_int]),
    "idh_feature_volume_plane_groups": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2),
    "idh_feature_volume_grid": (C.c_int, [C.c_longlong]),
    "idh_feature_volume_skip_task": (C.c_longlong, [C.c_longlong] + [C.c_int] * 4),
    "idh_feature_volume_fwd": (
        C.c_int,
        [f32p] * 6 + [C.c_float, C.c_float] + [C.c_int] * 6 + [f32p] * 6 + [f32p, C.c_int, f32p, C.c_void_p, f32p, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "idh_feature_volume_f16x3_fwd": (
        C.c_int,
        [f32p] * 6 + [C.c_float, C.c_float] + [C.c_int] * 6 + [f32p] * 6 + [f32p, C.c_int, f32p, C.c_void_p, f32p, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "idh_feature_volume_ex_fwd": (
        C.c_int,
        [f32p] * 6 + [C.c_float, C.c_float] + [C.c_int] * 6 + [f32p] * 6 + [f32p, C.c_int, f32p, C.c_void_p, f32p, C.c_void_p, C.c_size_t,
                                                                  C.c_int, C.POINTER(VolumeOpts), C.c_void_p],
    ),
    "idh_cost_volume_dot_ex_fwd": (
        C.c_int,
        [f32p, f32p, f32p, f32p, f32p, C.c_float, C.c_float] + [C.c_int] * 6 + [f32p, C.c_int, f32p, f32p, C.POINTER(VolumeOpts), C.c_void_p],
    ),
    "idh_cost_volume_dot_kernel_name": (C.c_char_p, [C.c_int] * 5),
    "idh_packed_mlp_weight_f16_bytes": (C.c_size_t, [C.c_int]),
    "idh_pack_mlp_weight_f16": (C.c_int, [f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "idh_binary_mlp_search_fwd": (C.c_int, [f32p, C.c_int, C.c_int, f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int,
                                            C.c_float, C.c_float, C.c_float, f32p, f32p, C.c_void_p]),
    "idh_binary_mlp_search_thr_fwd": (C.c_int, [f32p, C.c_int, C.c_int, f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int,
                                                C.c_float, C.c_float, f32p, f32p, C.c_int, f32p, f32p, C.c_void_p]),
    "idh_binary_mlp_search_f16x3_fwd": (C.c_int, [f32p, C.c_int, C.c_int, f32p, C.c_int, C.c_float, f32p, C.c_void_p, f32p, C.c_int, C.c_int, C.c_int,
                                                  C.c_float, C.c_float, C.c_float, f32p, f32p, C.c_int, f32p, f32p, C.c_void_p]),
    "idh_metrics_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "idh_plane_iou_fwd": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "idh_depth_metrics_fwd": (C.c_int, [f32p, f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "idh_sizeof_eval_args": (C.c_size_t, []),
    "idh_eval_frame_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "idh_eval_masks_fwd": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, f32p, f32p, C.c_void_p, C.c_void_p]),
    "idh_eval_plane_scores_fwd": (C.c_int, [C.POINTER(EvalArgs), f32p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "idh_eval_depth_metrics_fwd": (C.c_int, [f32p, f32p] + [C.c_int] * 6 + [C.c_float, C.c_int, f32p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "idh_raster_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "idh_raster_depth_fwd": (C.c_int, [f32p, C.c_int, C.c_void_p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "idh_vertex_predictions_fwd": (C.c_int, [f32p, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_float, f32p, C.c_void_p]),
    "idh_vertex_occlusion_changes_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "idh_sizeof_raster_shaded_args": (C.c_size_t, []),
    "idh_raster_shaded_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "idh_raster_shaded_fwd": (C.c_int, [C.POINTER(RasterShadedArgs), C.c_void_p]),
    "idh_sizeof_depth_warp_args": (C.c_size_t, []),
    "idh_depth_warp_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "idh_depth_warp_fwd": (C.c_int, [C.POINTER(DepthWarpArgs), C.c_void_p]),
    "idh_sizeof_tsdf_volume": (C.c_size_t, []),
    "idh_sizeof_tsdf_integrate_args": (C.c_size_t, []),
    "idh_sizeof_tsdf_raycast_args": (C.c_size_t, []),
    "idh_tsdf_block_flag_bytes": (C.c_size_t, [C.c_int] * 3),
    "idh_tsdf_reset_fwd": (C.c_int, [C.POINTER(TsdfVolume), C.c_void_p]),
    "idh_tsdf_flags_fwd": (C.c_int, [C.POINTER(TsdfVolume), C.c_void_p]),
    "idh_tsdf_integrate_fwd": (C.c_int, [C.POINTER(TsdfIntegrateArgs), C.c_void_p]),
    "idh_tsdf_raycast_fwd": (C.c_int, [C.POINTER(TsdfRaycastArgs), C.c_void_p]),
    "idh_sizeof_tsdf_mesh_args": (C.c_size_t, []),
    "idh_tsdf_mesh_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "idh_tsdf_mesh_count_fwd": (C.c_int, [C.POINTER(TsdfMeshArgs), C.c_void_p]),
    "idh_tsdf_mesh_emit_fwd": (C.c_int, [C.POINTER(TsdfMeshArgs), C.c_void_p]),
    "idh_sizeof_tsdf_integrate_color_args": (C.c_size_t, []),
    "idh_sizeof_tsdf_raycast_color_args": (C.c_size_t, []),
    "idh_sizeof_tsdf_mesh_colors_args": (C.c_size_t, []),
    "idh_tsdf_integrate_color_fwd": (C.c_int, [C.POINTER(TsdfIntegrateColorArgs), C.c_void_p]),
    "idh_tsdf_raycast_color_fwd": (C.c_int, [C.POINTER(TsdfRaycastColorArgs), C.c_void_p]),
    "idh_tsdf_mesh_colors_fwd": (C.c_int, [C.POINTER(TsdfMeshColorsArgs), C.c_void_p]),
    "idh_sizeof_tsdf_integrate_weighted_args": (C.c_size_t, []),
    "idh_tsdf_integrate_weighted_fwd": (C.c_int, [C.POINTER(TsdfIntegrateWeightedArgs), C.c_void_p]),
    "idh_sizeof_tsdf_shift_args": (C.c_size_t, []),
    "idh_tsdf_shift_fwd": (C.c_int, [C.POINTER(TsdfShiftArgs), C.c_void_p]),
    "idh_sizeof_tsdf_align_args": (C.c_size_t, []),
    "idh_tsdf_align_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "idh_tsdf_align_fwd": (C.c_int, [C.POINTER(TsdfAlignArgs), C.c_void_p]),
    "idh_sizeof_mv_consistency_args": (C.c_size_t, []),
    "idh_mv_consistency_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "idh_mv_consistency_fwd": (C.c_int, [C.POINTER(MvConsistencyArgs), C.c_void_p]),
    "idh_sizeof_edge_mask_args": (C.c_size_t, []),
    "idh_edge_mask_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "idh_edge_mask_fwd": (C.c_int, [C.POINTER(EdgeMaskArgs), C.c_void_p]),
    "idh_sizeof_bd_val_losses_args": (C.c_size_t, []),
    "idh_bd_val_losses_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "idh_bd_val_losses_fwd": (C.c_int, [C.POINTER(BdValLossesArgs), C.c_void_p]),
    "idh_sizeof_reg_val_losses_args": (C.c_size_t, []),
    "idh_reg_val_losses_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "idh_reg_val_losses_fwd": (C.c_int, [C.POINTER(RegValLossesArgs), C.c_void_p]),
    "idh_sizeof_composite_args": (C.c_size_t, []),
    "idh_prep_rendered_depth_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "idh_composite_fwd": (C.c_int, [C.POINTER(CompositeArgs), C.c_void_p]),
    "idh_resize_coeffs_sizes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "idh_resize_coeffs_pack": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "idh_sizeof_ingest_color_args": (C.c_size_t, []),
    "idh_sizeof_ingest_depth_args": (C.c_size_t, []),
    "idh_ingest_color_fwd": (C.c_int, [C.POINTER(IngestColorArgs), C.c_void_p]),
    "idh_ingest_depth_fwd": (C.c_int, [C.POINTER(IngestDepthArgs), C.c_void_p]),
    "idh_sizeof_bank": (C.c_size_t, []),
    "idh_bank_commit_fwd": (C.c_int, [C.POINTER(Bank), C.c_int, f32p, f32p, f32p, f32p, C.c_void_p]),
    "idh_bank_gather_fwd": (C.c_int, [C.POINTER(Bank), C.POINTER(C.c_int32), f32p, f32p, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_void_p]),
    "idh_sample_prior_fwd": (C.c_int, [f32p, f32p, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "idh_binary_mlp_rays_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_int, C.c_float, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, C.c_void_p]),
    "idh_binary_mlp_rays_search_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                                 f32p, f32p, f32p, C.c_int, C.c_float, C.c_float, C.c_float, f32p, f32p, C.c_int, f32p, f32p, f32p, f32p,
                                                 C.c_void_p, f32p, C.c_void_p]),
    "idh_binary_mlp_view_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p, f32p,
                                          f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_float, f32p, C.c_void_p, f32p, f32p, C.c_void_p]),
    "idh_binary_mlp_view_search_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, f32p, f32p, f32p, f32p,
                                                 f32p, f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, C.c_float, C.c_float, C.c_float, f32p, f32p,
                                                 C.c_int, C.c_float, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "idh_binary_mlp_view_keys_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_int), C.c_int,
                                               f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, f32p, C.c_int, C.c_float, f32p, f32p,
                                               f32p, C.c_float, f32p, C.c_void_p, f32p, f32p, C.c_void_p]),
    "idh_binary_mlp_view_keys_search_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_int),
                                                      C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, f32p, C.c_int,
                                                      C.c_float, f32p, f32p, f32p, C.c_int, C.c_float, C.c_float, C.c_float, f32p, f32p, C.c_int,
                                                      C.c_float, f32p, f32p, C.c_void_p, f32p, C.c_void_p, C.c_void_p]),
    "idh_binary_mlp_view_march_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, f32p, f32p, f32p, f32p,
                                                f32p, f32p, C.c_int, C.c_float, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_float, f32p, f32p,
                                                C.c_int, C.c_float, f32p, f32p, C.c_void_p, C.c_void_p, f32p, C.c_void_p]),
    "idh_binary_mlp_view_keys_march_fwd": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_int),
                                                     C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, f32p, f32p, f32p, f32p, f32p, f32p, C.c_int,
                                                     C.c_float, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_float, f32p, f32p, C.c_int,
                                                     C.c_float, f32p, f32p, C.c_void_p, C.c_void_p, f32p, C.c_void_p, C.c_void_p]),
    "idh_sizeof_normals_args": (C.c_size_t, []),
    "idh_sizeof_patch_normals_args": (C.c_size_t, []),
    "idh_depth_normals_fwd": (C.c_int, [C.POINTER(NormalsArgs), C.c_void_p]),
    "idh_patch_normals_fwd": (C.c_int, [C.POINTER(PatchNormalsArgs), C.c_void_p]),
    "idh_project_points_fwd": (C.c_int, [f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_void_p, f32p, f32p, f32p, f32p, C.c_void_p]),
    "idh_cost_volume_dot_fwd": (
        C.c_int,
        [f32p, f32p, f32p, f32p, f32p, C.c_float, C.c_float] + [C.c_int] * 6 + [f32p, C.c_int, f32p, f32p, C.c_void_p],
    ),
}


def _all_sigs():
    from . import model_abi, net_abi  # (structs of include/idh_net.h / idh_model.h live there; imported lazily: they import this module)

    return {**_SIGS, **net_abi.SIGS, **model_abi.SIGS}


def declared_symbols():
    return sorted(_all_sigs())


def lib():
    """Load (once) and return the ctypes handle; raises IdhError if the .so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IdhError(
                f"{LIB_PATH} not found — the gfx950 HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)."
            )
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _all_sigs().items():
            try:
                fn = getattr(h, name)
            except AttributeError:  # entry points added without an ABI bump (additive: idh_binary_mlp_rays_fwd, idh_project_points_fwd, idh_binary_mlp_rays_search_fwd, idh_binary_mlp_view_fwd, idh_binary_mlp_view_search_fwd, idh_binary_mlp_view_keys_fwd, idh_binary_mlp_view_keys_search_fwd, idh_binary_mlp_view_march_fwd, idh_binary_mlp_view_keys_march_fwd, idh_depth_normals_fwd, idh_patch_normals_fwd, idh_raster_shaded_fwd, idh_depth_warp_fwd, idh_tsdf_integrate_fwd, idh_tsdf_raycast_fwd, idh_tsdf_mesh_count_fwd) are found missing here
                raise IdhError(f"{LIB_PATH} does not export {name}: it was built from an older tree; rebuild with `python implicit-depth_amd/build.py --force`") from None
            fn.restype = res
            fn.argtypes = args
        # the ABI this mirror was written against (include/idh.h): struct layouts, tile codes and packed-weight layouts changed at these versions
        # (102: IDH_TILE_WINO4 names the shared-transform F(4x4) kernel and ITS packed layout - blobs packed by an older library are not portable)
        ver = h.idh_version()
        if ver < MIN_ABI_VERSION and not os.environ.get("IDH_LIB_ANY_ABI"):  # (IDH_LIB_ANY_ABI: A/B timing against a library built from an older tree)
            raise IdhError(f"{LIB_PATH} reports ABI version {ver}, this binding needs >= {MIN_ABI_VERSION}: rebuild with `python implicit-depth_amd/build.py --force`")
        if h.idh_sizeof_eval_args() != C.sizeof(EvalArgs):
            raise IdhError(f"{LIB_PATH}: sizeof(idh_eval_args) = {h.idh_sizeof_eval_args()} in the library, {C.sizeof(EvalArgs)} in this binding")
        if h.idh_sizeof_composite_args() != C.sizeof(CompositeArgs):
            raise IdhError(f"{LIB_PATH}: sizeof(idh_composite_args) = {h.idh_sizeof_composite_args()} in the library, {C.sizeof(CompositeArgs)} in this binding")
        for what, got, mirror in (("idh_ingest_color_args", h.idh_sizeof_ingest_color_args(), IngestColorArgs),
                                  ("idh_ingest_depth_args", h.idh_sizeof_ingest_depth_args(), IngestDepthArgs),
                                  ("idh_bank", h.idh_sizeof_bank(), Bank),
                                  ("idh_normals_args", h.idh_sizeof_normals_args(), NormalsArgs),
                                  ("idh_patch_normals_args", h.idh_sizeof_patch_normals_args(), PatchNormalsArgs),
                                  ("idh_raster_shaded_args", h.idh_sizeof_raster_shaded_args(), RasterShadedArgs),
                                  ("idh_depth_warp_args", h.idh_sizeof_depth_warp_args(), DepthWarpArgs),
                                  ("idh_tsdf_volume", h.idh_sizeof_tsdf_volume(), TsdfVolume),
                                  ("idh_tsdf_integrate_args", h.idh_sizeof_tsdf_integrate_args(), TsdfIntegrateArgs),
                                  ("idh_tsdf_raycast_args", h.idh_sizeof_tsdf_raycast_args(), TsdfRaycastArgs),
                                  ("idh_tsdf_mesh_args", h.idh_sizeof_tsdf_mesh_args(), TsdfMeshArgs),
                                  ("idh_tsdf_integrate_color_args", h.idh_sizeof_tsdf_integrate_color_args(), TsdfIntegrateColorArgs),
                                  ("idh_tsdf_raycast_color_args", h.idh_sizeof_tsdf_raycast_color_args(), TsdfRaycastColorArgs),
                                  ("idh_tsdf_mesh_colors_args", h.idh_sizeof_tsdf_mesh_colors_args(), TsdfMeshColorsArgs),
                                  ("idh_tsdf_integrate_weighted_args", h.idh_sizeof_tsdf_integrate_weighted_args(), TsdfIntegrateWeightedArgs),
                                  ("idh_tsdf_shift_args", h.idh_sizeof_tsdf_shift_args(), TsdfShiftArgs),
                                  ("idh_tsdf_align_args", h.idh_sizeof_tsdf_align_args(), TsdfAlignArgs),
                                  ("idh_mv_consistency_args", h.idh_sizeof_mv_consistency_args(), MvConsistencyArgs),
                                  ("idh_edge_mask_args", h.idh_sizeof_edge_mask_args(), EdgeMaskArgs),
                                  ("idh_bd_val_losses_args", h.idh_sizeof_bd_val_losses_args(), BdValLossesArgs),
                                  ("idh_reg_val_losses_args", h.idh_sizeof_reg_val_losses_args(), RegValLossesArgs)):
            if got != C.sizeof(mirror):
                raise IdhError(f"{LIB_PATH}: sizeof({what}) = {got} in the library, {C.sizeof(mirror)} in this binding")
        sizes = (C.c_size_t * 3)()
        h.idh_sizeof_conv_select(sizes)
        if list(sizes) != [C.sizeof(ConvDesc), C.sizeof(ConvTuning), C.sizeof(ConvChoice)]:
            raise IdhError(f"{LIB_PATH}: sizeof(idh_conv_desc / _tuning / _choice) = {list(sizes)} in the library, another in this binding")
        if h.idh_sizeof_volume_opts() != C.sizeof(VolumeOpts):
            raise IdhError(f"{LIB_PATH}: sizeof(idh_volume_opts) = {h.idh_sizeof_volume_opts()} in the library, {C.sizeof(VolumeOpts)} in this binding")
        _lib = h
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().idh_error_string(code).decode()
        raise IdhError(f"{what} failed: {msg} ({code})")


def ptr(t: "torch.Tensor | None"):
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


_weights_epoch = 0


def invalidate_weight_caches() -> None:
    """Forget every packed-weight / plan cache entry keyed on parameters whose modifications torch does not count
    (tensors created under ``torch.inference_mode()``).  Called automatically after ``load_state_dict`` on the drop-in
    modules and ``HotPath``; call it by hand after any other in-place edit of inference-mode parameters
    (``param.copy_()``, ``param.mul_()`` ... inside ``with torch.inference_mode():``)."""
    global _weights_epoch
    _weights_epoch += 1


def _sd_post_hook(module, incompatible_keys) -> None:
    """load_state_dict post-hook (a module-level function, not a closure: a module carrying it still pickles)."""
    invalidate_weight_caches()


def watch_state_dict_loads(module) -> None:
    """``load_state_dict()`` on the module, on any parent, or on ANY of its submodules (e.g. straight into ``cost_volume.mlp`` or a
    ``Conv2d`` inside a decoder's ``ModuleDict``) invalidates the caches above: load_state_dict runs the post-hooks of every module
    it descends into, so the hook is registered on each of them."""
    for m in module.modules():
        if not m.__dict__.get("_idh_sd_hook"):
            m.register_load_state_dict_post_hook(_sd_post_hook)
            m.__dict__["_idh_sd_hook"] = True


def param_version(t):
    """Cache key component that changes when parameter ``t`` is modified in place: torch's version counter — or, for
    tensors created under ``torch.inference_mode()`` (no counter, yet ``load_state_dict`` / ``copy_`` inside inference mode DO
    modify them), the epoch bumped by ``invalidate_weight_caches()``."""
    try:
        return t._version
    except RuntimeError:
        return ("inference", _weights_epoch)


def require_cuda_f32(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise IdhError("implicit_depth_amd kernels need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.float32:
            raise IdhError(f"implicit_depth_amd kernels are fp32 (got {t.dtype})")
