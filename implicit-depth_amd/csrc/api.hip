#include "idh_common.h"

extern "C" int idh_version(void) { return 112; }  // 101: idh_volume_opts.scratch / scratch_floats / struct_size; 102: Winograd F(4x4) conv (IDH_TILE_WINO4);
                                                   // 103: struct_size accepted when >= the fields it guards, hidden visibility (the C ABI is the only export);
                                                   // 104: IDH_OP_POINTWISE_UP, tile_m 8 / 9 for a lone 3x3 stride-2 source, split-K boundaries of the LDS conv in cost units
                                                   // 105: idh_binary_mlp_fwd takes any feature row stride / 4-byte-aligned base; network-level entry points idh_basic_block_fwd,
                                                   //      idh_cvencoder_fwd, idh_unetpp_fwd (csrc/networks.hip); idh_pack_conv_weight_wino4 row order (w4_v2p); run lists in idh_volume_opts.scratch
                                                   // 106: whole-model entry points idh_model_sizes / _pack / _fwd (include/idh_model.h, csrc/model.hip)
                                                   // 107: idh_feature_volume_plane_groups (host-only query of the feature volume's plane partition)
                                                   // 108: idh_conv_variant (host-only query of the kernel an IDH_OP_CONV descriptor runs on); IDH_OP_SPLITK_REDUCE documented as reserved
                                                   // 109: idh_binary_mlp_f16x3_fwd and the three search entry points refuse a feature base that is not 16-byte aligned (they read rows with dwordx4 loads)
                                                   // 110: tile_m = IDH_SPLIT_F16X3 refuses a second source that is not a plain 1x1 stride-1 projection (a 3x3 stride-2 one was accepted and computed wrongly)
                                                   // 111: idh_conv_select / idh_conv_tuning_defaults / idh_schedule_ops (csrc/plan_select.hip): the one kernel-selection rule and level scheduler of both plan builders
                                                   // (still 111) idh_binary_mlp_rays_fwd / idh_project_points_fwd (csrc/mlp_rays.hip) are additive: no struct, code or packed layout changed, so the
                                                   //      version stays; a binding that needs them finds them missing by name when it loads an older library
                                                   // (still 111) idh_volume_opts.reserved0 is now win_units_per_split (same offset and size; 0 = what every caller wrote there = automatic) and
                                                   //      idh_cost_volume_dot_plan (host-only query of the window kernel's plane split and scratch layout) is additive
                                                   // 112: idh_debug_set_plan_observer (include/idh_net.h): a host-only hook that shows every scheduled plan of csrc/networks.hip; the made-up addresses
                                                   //      of the *_sizes plans no longer collide (one range per caller-owned tensor, workspace and blob apart)
extern "C" size_t idh_sizeof_volume_opts(void) { return sizeof(idh_volume_opts); }

extern "C" const char *idh_error_string(int code) {
    switch (code) {
        case IDH_OK: return "ok";
        case IDH_EINVAL: return "invalid argument (shape, null pointer or parameter)";
        case IDH_EUNSUPPORTED: return "configuration not covered by the gfx950 kernels";
        case IDH_ELAUNCH: return "HIP kernel launch failed";
        case IDH_EWORKSPACE: return "workspace missing or too small";
        default: return "unknown idh error";
    }
}
