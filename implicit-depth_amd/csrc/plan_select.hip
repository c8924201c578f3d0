// Host-side planning shared by the two plan builders (implicit-depth_amd/nhwc.py's Plan and csrc/networks.hip's): which kernel, tile and split-K
// factor a conv runs with (idh_conv_select), and the dependency-level schedule of an op list (idh_schedule_ops).  No device code and no HIP
// header: this file also compiles with the plain host compiler.  What the thresholds mean and how they were measured: nhwc.py, next to the
// module globals that carry the shipped values (idh_conv_tuning_defaults must equal them; tests/test_abi.py compares).
#include <algorithm>
#include <array>
#include <vector>

#include "../../include/idh.h"
#include "../../include/idh_ops.h"

namespace {

typedef long long i64;
inline int ceil16(int v) { return (v + 15) & ~15; }
inline i64 cdiv(i64 a, i64 b) { return (a + b - 1) / b; }
inline int lds_subtiles(int cout) { return cout % 64 == 0 ? 4 : (cout % 32 == 0 ? 2 : 1); }  // 16-channel sub-tiles per workgroup of conv3x3_lds_k

struct Shape {  // a descriptor with its tuning: the predicates and choosers below read both
    const idh_conv_desc &d;
    const idh_conv_tuning &t;
    const idh_conv_desc_src &s0, &s1;
    bool two;

    // a plain 3x3 stride-1 zero-padded first source and, if any, a 1x1 stride-1 projection behind it: what both Winograd kernels and the
    // split-precision kernel take
    bool plain3(int cout_mult, bool cat_ok) const {
        if (s0.ks != 3 || s0.stride != 1 || d.pad_mode != IDH_PAD_ZEROS || d.Cout % cout_mult || (!cat_ok && s0.is_cat)) return false;
        return !two || (s1.ks == 1 && s1.stride == 1 && (cat_ok || !s1.is_cat));
    }
    // the 32 x 8 pixel tile grid covers the map well enough, and there are enough tiles of `ch` channels
    bool wino_grid(int ch, double min_fill, int min_tiles) const {
        const i64 ty = cdiv(d.Ho, 8), tx = cdiv(d.Wo, 32);
        if ((double)((i64)d.Ho * d.Wo) < min_fill * (ty * 8) * (tx * 32)) return false;
        return d.N * ty * tx * (d.Cout / ch) >= min_tiles;
    }
    bool wino() const { return plain3(32, false) && wino_grid(32, t.wino_min_fill, t.wino_min_tiles); }
    // idh_conv::wino4_supported (csrc/conv_wino4.hip) plus the fill / tile-count rule: the per-image byte sizes are 32-bit buffer ranges in the
    // kernel, so a layer beyond them is planned onto F(2x2) / the direct kernels instead of failing at run time
    bool wino4() const {
        if (!plain3(64, false) || (two && !t.winograd4_proj)) return false;
        if ((d.act != IDH_ACT_NONE && d.act != IDH_ACT_LRELU && d.act != IDH_ACT_ELU) || (d.act == IDH_ACT_LRELU && !(d.slope >= 0.f && d.slope <= 1.f))) return false;
        if (s0.Cin <= 16) return false;  // (the copy pipeline runs a pair of 8-channel stages ahead)
        if ((i64)s0.H * s0.W * s0.cs * 4 >= (1ll << 30)) return false;  // (the halo's 32-bit offsets run a few rows past an image)
        if ((i64)d.Ho * d.Wo * d.out_cs * 4 >= (1ll << 31) || (d.has_res && (i64)d.Ho * d.Wo * d.res_cs * 4 >= (1ll << 31))) return false;
        if (two && ((i64)s1.H * s1.W * s1.cs * 4 >= (1ll << 31) || (i64)((s1.Cin + 15) / 16) * 4 * ceil16(d.Cout) * 64 >= (1ll << 31))) return false;
        if ((i64)((s0.Cin + 15) / 16) * 4 * ceil16(d.Cout) * 36 * 16 * 4 >= (1ll << 31)) return false;  // packed weights
        return d.any_size || wino_grid(64, t.wino4_min_fill, t.wino4_min_tiles);
    }
    bool split() const {
        if (!plain3(64, true) || d.Wo < 16 || d.Ho < 8) return false;
        return d.N * cdiv(d.Ho, 8) * cdiv(d.Wo, 16) * (d.Cout / 64) >= t.split_min_blocks;
    }
    bool lds() const {  // csrc/conv.hip conv3x3_lds_k
        if (s0.ks != 3 || s0.stride != 1 || d.Cout % 16 || d.Wo < 16) return false;
        if (d.pad_mode != IDH_PAD_ZEROS && (d.pad_mode != IDH_PAD_REPLICATE || two)) return false;
        if (!two || (s1.ks == 1 && s1.stride == 1)) return true;  // BasicBlock's downsample(x): 1x1, or 3x3 stride 2
        return s1.ks == 3 && s1.stride == 2 && d.pad_mode == IDH_PAD_ZEROS && d.Cout % 32 == 0 && !s1.is_cat;
    }
    bool s2_first() const {  // a lone 3x3 stride-2 conv on the LDS kernel's stride-2 loader
        if (!t.s2_first || two || s0.ks != 3 || s0.stride != 2 || d.pad_mode != IDH_PAD_ZEROS || d.Cout % 32 || d.Wo < 16 || s0.is_cat) return false;
        return d.N * cdiv(d.Wo, 16) * cdiv(d.Ho, 4) * (d.Cout / (16 * lds_subtiles(d.Cout))) >= t.s2_first_min_blocks;
    }

    // 16-row tiles of the split-precision kernel when they fill 256 CUs x 3 resident workgroups without wasting rows, else 8-row tiles
    int split_rows() const {
        auto eff = [&](int rows, double bonus) {
            const i64 ty = cdiv(d.Ho, rows), blocks = d.N * ty * cdiv(d.Wo, 16) * (d.Cout / 64);
            return bonus * ((double)d.Ho / (double)(ty * rows)) * std::min(1.0, blocks / 768.0);
        };
        return d.Ho >= 16 && eff(16, 1.0) >= eff(8, 0.93) ? 16 : 8;
    }
    // LDS kernel: 8-row tiles (code 8) when they give one full round of 256 CUs x 3 resident workgroups, else 4-row tiles (code 9); split K only
    // when the grid still cannot fill the chip and every split keeps >= split_min_chunks chunks (a 1x1 chunk counts proj_chunk_weight of a 3x3 one)
    void lds_tile(int &code, int &split) const {
        double chunks = 0;
        for (int i = 0; i <= (int)two; ++i) chunks += (ceil16(d.src[i].Cin) / 16) * (d.src[i].ks == 3 ? 1.0 : t.proj_chunk_weight);
        const i64 per_row = d.N * cdiv(d.Wo, 16) * (d.Cout / (16 * lds_subtiles(d.Cout)));
        const bool rows4 = per_row * cdiv(d.Ho, 8) < 768;
        code = rows4 ? 9 : 8;
        const i64 blocks = per_row * cdiv(d.Ho, rows4 ? 4 : 8);
        split = (int)std::max<i64>(1, std::min<i64>({cdiv(768, blocks), (int)chunks / t.split_min_chunks, t.split_max}));
    }
    // direct kernel: the largest wave tile that still gives target_waves waves; split K below min_waves
    void direct_tile(int &tm, int &tn, int &split) const {
        int steps = 0;
        for (int i = 0; i <= (int)two; ++i) steps += d.src[i].ks * d.src[i].ks * (ceil16(d.src[i].Cin) / 16);
        const i64 M = (i64)d.N * d.Ho * d.Wo;
        const int nsub = ceil16(d.Cout) / 16;
        tn = nsub % 4 == 0 ? 4 : (nsub % 2 == 0 ? 2 : 1);
        i64 waves = 0;
        for (int cand : {4, 2, 1}) {
            waves = cdiv(M, 16 * cand) * (nsub / tn);
            tm = cand;
            if (waves >= t.target_waves) break;
        }
        split = waves < t.min_waves ? (int)std::max<i64>(1, std::min<i64>({cdiv(t.min_waves, waves), steps / 4, 32})) : 1;
    }
};

// Order of the ops of one dependency level, and which of them carry the level's group id (r[0] < 3): the F(2x2) convs first (one persistent
// conv3x3_wino_group_k grid: plain ones, then those with a fused 1x1 source, the largest first so that the small ones fill its tail); the 4-row
// LDS convs by channel tile (one conv3x3_lds_group_k grid per run of equal tiles); the other members a mixed level_k launch can host (the direct conv
// with 16x64 wave tiles, bilinear x2 upsampling, the layout imports: adjacent, one import_nchw_group_k grid when small); the rest run alone
void launch_rank(const idh_op &op, int flags, i64 r[3]) {
    const bool conv = op.kind == IDH_OP_CONV, merge = flags & IDH_SCHED_MERGE_LEVELS;
    r[0] = 3; r[1] = 0; r[2] = 0;
    if ((flags & IDH_SCHED_WINO_GROUP) && conv && op.tile_m == IDH_TILE_WINO) { r[0] = -1; r[1] = op.src[1].in ? 1 : 0; r[2] = -(i64)op.N * op.Ho * op.Wo * op.Cout; }
    else if (conv && op.tile_m == 9) { r[0] = 0; r[1] = op.tile_n; }
    else if (merge && conv && op.tile_m == 1 && op.tile_n == 4) { r[0] = 1; }
    else if (merge && op.kind == IDH_OP_UPSAMPLE2) { r[0] = 2; }
    else if (merge && op.kind == IDH_OP_NCHW_TO_NHWC) { r[0] = 2; r[1] = 1; }
}

}  // namespace

extern "C" void idh_conv_tuning_defaults(idh_conv_tuning *t) {
    if (t) *t = idh_conv_tuning{1, 1, 1, 1, 128, 768, 256, 400, 0, 6, 16, 512, 4, 2048, 1024, 0, 0.74, 0.85, 0.5};
}

extern "C" void idh_sizeof_conv_select(size_t out[3]) {
    if (out) { out[0] = sizeof(idh_conv_desc); out[1] = sizeof(idh_conv_tuning); out[2] = sizeof(idh_conv_choice); }
}

extern "C" int idh_conv_select(const idh_conv_desc *desc, const idh_conv_tuning *tuning, idh_conv_choice *out) {
    idh_conv_tuning def;
    idh_conv_tuning_defaults(&def);
    const idh_conv_tuning &t = tuning ? *tuning : def;
    if (!desc || !out || desc->n_src < 1 || desc->n_src > 2 || desc->N <= 0 || desc->Ho <= 0 || desc->Wo <= 0 || desc->Cout <= 0) return IDH_EINVAL;
    if ((desc->math != 0 && desc->math != IDH_SPLIT_F16X3) || desc->out_cs < 0 || desc->res_cs < 0 || t.split_min_chunks < 1) return IDH_EINVAL;
    for (int i = 0; i < desc->n_src; ++i) {
        const idh_conv_desc_src &s = desc->src[i];
        if ((s.ks != 1 && s.ks != 3) || s.stride < 1 || s.Cin < 0 || s.H < 0 || s.W < 0 || s.cs < 0) return IDH_EINVAL;
    }
    const idh_conv_desc &d = *desc;
    const Shape s{d, t, d.src[0], d.src[1], d.n_src == 2};
    const bool fp32 = d.math == 0, cat = d.src[0].is_cat || (s.two && d.src[1].is_cat);
    idh_conv_choice c{};
    c.families = (s.wino() ? IDH_FAMILY_WINO : 0) | (s.wino4() ? IDH_FAMILY_WINO4 : 0) | (s.split() ? IDH_FAMILY_SPLIT : 0) | (s.lds() ? IDH_FAMILY_LDS : 0) |
                 (s.s2_first() ? IDH_FAMILY_S2_FIRST : 0);
    c.lds_subtiles = lds_subtiles(d.Cout);
    if (d.Cout % 16 == 0) s.lds_tile(c.lds_tile_m, c.lds_split_k);
    c.split_rows = s.split_rows();
    s.direct_tile(c.direct_tile_m, c.direct_tile_n, c.direct_split_k);
    // the cascade: split precision (opt-in math), F(4x4), F(2x2), the LDS-staged kernel, its stride-2 loader for a lone source, the direct kernel
    const bool plain = fp32 && !d.has_norm;
    c.split_k = 1;
    if (!fp32 && (c.families & IDH_FAMILY_SPLIT)) {
        c.w_layout = IDH_W_SPLIT; c.tile_m = d.math; c.tile_n = c.split_rows;
    } else if (plain && t.winograd4 && (!s.two || !d.has_res) && (c.families & IDH_FAMILY_WINO4)) {
        c.w_layout = IDH_W_WINO4; c.tile_m = IDH_TILE_WINO4;
    } else if (plain && t.winograd && (c.families & IDH_FAMILY_WINO)) {
        c.w_layout = IDH_W_WINO; c.tile_m = IDH_TILE_WINO;
    } else if (c.families & IDH_FAMILY_LDS) {
        c.tile_m = c.lds_tile_m == 8 && t.fused_up_rows == 4 && cat ? 9 : c.lds_tile_m;
        c.tile_n = c.lds_subtiles;
        c.split_k = c.lds_split_k;
        // small grids: narrower channel tiles (64 -> 32 -> 16) shorten each workgroup's MFMA phase and spread it over more CUs
        if (c.tile_n == 4 && c.tile_m == 9 && t.narrow_tile_below && !cat) {
            const i64 blocks64 = d.N * cdiv(d.Ho, 4) * cdiv(d.Wo, 16) * (d.Cout / 64) * c.split_k;
            if (blocks64 < t.narrow_tile_below) c.tile_n = blocks64 < t.narrowest_tile_below ? 1 : 2;
        }
        c.tile_n = c.tile_n == 4 ? 0 : c.tile_n;
    } else if (plain && (c.families & IDH_FAMILY_S2_FIRST)) {
        c.tile_m = c.lds_tile_m; c.split_k = c.lds_split_k;
        c.tile_n = c.lds_subtiles == 4 ? 0 : c.lds_subtiles;
    } else {
        c.tile_m = c.direct_tile_m; c.tile_n = c.direct_tile_n; c.split_k = c.direct_split_k;
    }
    *out = c;
    return IDH_OK;
}

extern "C" int idh_schedule_ops(idh_op *ops, int n, int n_first, const uint64_t *regions, const int32_t *offsets, int flags, int32_t *order, int32_t *levels) {
    if (n < 0 || (n > 0 && (!ops || !regions || !offsets))) return IDH_EINVAL;
    for (int k = 0; k < 2 * n; ++k)
        if (offsets[k] < 0 || offsets[k + 1] < offsets[k]) return IDH_EINVAL;
    n_first = std::max(0, std::min(n_first, n));
    auto overlap = [&](int a0, int a1, int b0, int b1) {
        for (int a = a0; a < a1; ++a)
            for (int b = b0; b < b1; ++b) {
                const uint64_t *x = regions + 3 * (size_t)a, *y = regions + 3 * (size_t)b;
                if (x[0] == y[0] && x[1] < y[2] && y[1] < x[2]) return true;
            }
        return false;
    };
    std::vector<int> level(n, 0), perm(n);
    std::vector<std::array<i64, 6>> key(n);
    for (int j = 0; j < n; ++j) {
        const int32_t *oj = offsets + 2 * j;  // reads [oj[0], oj[1]), writes [oj[1], oj[2])
        for (int i = j < n_first ? 0 : n_first; i < j; ++i) {
            const int32_t *oi = offsets + 2 * i;
            if (overlap(oi[1], oi[2], oj[0], oj[1]) || overlap(oi[1], oi[2], oj[1], oj[2]) || overlap(oi[0], oi[1], oj[1], oj[2])) level[j] = std::max(level[j], level[i] + 1);
        }
        i64 r[3];
        launch_rank(ops[j], flags, r);
        key[j] = {j < n_first ? 0 : 1, level[j], r[0], r[1], r[2], j};
        ops[j].group = r[0] < 3 ? level[j] + 1 : 0;
        perm[j] = j;
    }
    std::sort(perm.begin(), perm.end(), [&](int a, int b) { return key[a] < key[b]; });
    const std::vector<idh_op> built(ops, ops + n);
    for (int k = 0; k < n; ++k) {
        ops[k] = built[perm[k]];
        if (order) order[k] = perm[k];
        if (levels) levels[k] = level[perm[k]];
    }
    return IDH_OK;
}
