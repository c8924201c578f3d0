/*
 * idh_ops.h — op descriptors for the conv / upsample / layout stage of the hot path.
 *
 * The reference runs CVEncoder / BDDecoderPP / DepthDecoderPP (modules/networks.py:20-215)
 * as ~150 nn.Conv2d + F.interpolate + torch.cat calls.  Here a network pass is a flat array
 * of idh_op descriptors, built once per (module, shape) by the host and submitted with ONE
 * call, idh_run_ops(); an op is one gfx950 kernel launch on the given stream, or shares a launch with the other
 * independent ops of its dependency level (idh_op.group).
 * All activations are NHWC fp32.  "cs" = channel stride = floats between consecutive pixels
 * (>= channel count), which is how torch.cat along channels is eliminated: producers write
 * straight into a channel slice of the consumer's input buffer.
 */
#ifndef IDH_OPS_H_
#define IDH_OPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations of this header are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

enum {
    IDH_OP_CONV = 1,        /* implicit-GEMM conv on fp32 MFMA (layers.py:59-75 convs)       */
    IDH_OP_UPSAMPLE2 = 2,   /* bilinear x2, align_corners=False (generic_utils.py:94-103).  32-bit element indices since ABI 104:
                               N*H*W*C/4 (input channel quads) and the same count of the output must stay below 2^31 - i.e. inputs
                               under 32 GiB - else IDH_EUNSUPPORTED (no 64-bit-index variant is kept; split the batch) */
    IDH_OP_NCHW_TO_NHWC = 3,/* strided layout import: (N,C,H,W) dense -> NHWC slice of channel stride out_cs, any channel count;
                               0 < N <= 65535, H, W, Cin > 0, else IDH_EINVAL.  Up to 8 consecutive imports with one non-zero group id share a
                               grid; a member of more than 4096 blocks (64 pixels x 32 channels each) keeps its own */
    IDH_OP_NHWC_TO_NCHW = 4,/* strided layout export: NHWC slice -> (N,C,H,W) dense.  src[0].in / .cs / .H / .W / .Cin = the slice, any channel count;
                               0 < N <= 65535, H, W, Cin > 0, cs >= Cin, else IDH_EINVAL */
    IDH_OP_SPLITK_REDUCE = 5,/* RESERVED, never accepted: idh_run_ops / idh_count_launches answer IDH_EINVAL for it.  The sum of the
                                split-K partials (+ bias + residual + activation) is implicit in an IDH_OP_CONV with split_k > 1, which
                                launches its own reduce (one grid for all split members of a group); the number stays taken */
    IDH_OP_POINTWISE_HEAD = 6,/* 1x1 conv to 1 channel (DepthDecoderPP heads, networks.py:158-161); ws != NULL: a second
                                 (N,1,H,W) output = exp(out), the depth map of depth_model.py:425-433.  src[0].w = Cin floats, bias = 1 float or
                                 NULL; N, H, W, Cin > 0, Cin and cs multiples of 4, cs >= Cin, else IDH_EINVAL */
    IDH_OP_COPY = 9,        /* channel-strided NHWC -> NHWC slice copy.  N, H, W, Cin > 0, Cin / cs / out_cs multiples of 4, cs >= Cin and
                               out_cs >= Cin (a narrower stride would make pixels overlap), else IDH_EINVAL */
    IDH_OP_UPSAMPLE2_NEAREST = 8, /* nearest x2 (SkipDecoder, networks_fast.py:43); the rules of IDH_OP_COPY */
    IDH_OP_POINTWISE_NCHW = 10, /* 1x1 conv 64 -> 128 read straight from a dense (N,64,H,W) tensor into an NHWC slice: the first
                                   layer of the matching-encoder head (networks.py:279) without a layout-import pass;
                                   src[0].w = idh_pack_conv_weight(128, 64, 1); other widths: IDH_EUNSUPPORTED */
    IDH_OP_POINTWISE_UP = 11, /* out = W . x (+ bias) + up2(low): a 1x1 conv of an NHWC tensor plus the x2 bilinear upsampling (IDH_OP_UPSAMPLE2's
                                 expression) of a half-resolution NHWC tensor of Cout channels - the projection branch of the decoder blocks on
                                 cat(right, up(lo), up(lo2)) (networks.py:52-77, layers.py:86-92), whose upsampled two thirds are projected at low
                                 resolution because a 1x1 conv commutes with bilinear upsampling.  src[0] = x (N,H,W,Cin), w =
                                 idh_pack_conv_weight(Cout, Cin, 1); src[1].in / .cs / .H / .W = the (N,H/2,W/2,Cout) map; Cin == Cout in {64, 128},
                                 H and W even; other shapes: IDH_EUNSUPPORTED */
    IDH_OP_STEM = 12,       /* ResNet18 stem of the matching encoder up to its anti-aliased max-pool (implicit-depth_amd/backbone.py: conv1 7x7/2 3->64
                               with eval-mode BatchNorm folded in, ReLU, MaxPool2d(2, 1), BlurPool = ReflectionPad2d((1, 2, 1, 2)) + depthwise 4x4
                               filter outer([1,3,3,1], [1,3,3,1]) / 64 at stride 2 - a fixed filter, not read from memory), one fused pass
                               (csrc/stem.hip stem_conv7_pool_k).  src[0].in = image 0 of N dense fp32 (3, H, W) images, H, W >= 8;
                               src[0].H / .W = H, W; src[0].Cin = 3; src[0].w = idh_pack_stem_weight output; images in groups (a (B, K+1, 3, H, W)
                               view): src[0].up_C = images per group (0: one group of N), src[0].up_cs[0] = floats between consecutive images of a
                               group (0: 3 H W), src[0].up_cs[1] = floats between groups (0: up_C times the image stride).  out = NHWC (N, Ho, Wo,
                               out_cs), channels [0, 64) written, 16-byte aligned, out_cs >= 64 and a multiple of 4; Cout = 64; Ho = floor(ceil(H/2) / 2),
                               Wo likewise.  bias / res / ws / act unused */
    IDH_OP_INSTNORM = 7     /* nn.InstanceNorm2d (no affine, eps 1e-5) [+ LeakyReLU] on NHWC; matching-encoder
                               head networks.py:279-283.  0 < N <= 65535, H, W > 0, Cin a multiple of 4 with (Cin / 4) | 256, else IDH_EINVAL.  ws: N*(ceil(HW/1024)+1)*2*C floats (chunk partials + mean/rstd);
                               out == NULL: statistics only — float[N][2][C] at ws + N*ceil(HW/1024)*2*C, for a
                               consumer convolution that normalises on load (idh_conv_src.norm) */
};

#define IDH_PAD_ZEROS 0
#define IDH_PAD_REPLICATE 1

/* One conv source: input tensor + its packed weights.  A conv op may sum TWO sources into
 * the same accumulator: BasicBlock's conv2(h) + downsample(x) (layers.py:86-92) becomes one
 * launch whose second source is the 1x1 (or strided 3x3) projection of the block input. */
typedef struct idh_conv_src {
    const float *in; /* NHWC, N x H x W x (cs) */
    const float *w;  /* packed by idh_pack_conv_weight: [ks*ks][Cin_pad/4][Cout_pad][4] */
    int32_t cs, H, W, Cin;
    int32_t ks, stride, pad_mode, _r;
    /* Virtual concat with fused bilinear x2 (the UNet++ decoder's torch.cat([x, upsample(a), upsample(b)], 1),
     * networks.py:64-76): channels [0, up_c0) come from `in`; channels [up_c0 + i*up_C, up_c0 + (i+1)*up_C) are the
     * x2 bilinear upsampling (align_corners=False, generic_utils.py:94-103) of up_in[i], an NHWC map of (H/2, W/2)
     * with channel stride up_cs[i], interpolated while the consumer conv stages its halo — the upsampled tensor and
     * the concat buffer are never written.  up_in[0] == NULL: plain source.  LDS-staged 3x3 / fused 1x1 sources
     * only; up_c0 and up_C multiples of 16, H and W even, Cin == up_c0 + n_segments * up_C. */
    const float *up_in[2];
    int32_t up_cs[2];
    int32_t up_c0, up_C;
    /* Normalise-on-load: norm != NULL -> the kernel reads x' = act((x - mean[n][c]) * rstd[n][c]) instead of x, with
     * norm = the statistics an IDH_OP_INSTNORM left in its workspace (float[N][2][Cin]: means then 1/sqrt(var + eps)).
     * nn.InstanceNorm2d + LeakyReLU between two convolutions of the matching-encoder head (networks.py:280-281) then
     * cost one statistics pass and no normalised copy of the tensor.  Same expression as the materialising kernel
     * (bit-identical); padding is applied after the normalisation (a zero-padded tap stays 0).  src[0] of the
     * LDS-staged 3x3 kernel with 16-channel output tiles only (IDH_EUNSUPPORTED otherwise). */
    const float *norm;
    float norm_slope;
    int32_t norm_act;  /* IDH_ACT_* */
} idh_conv_src;

typedef struct idh_op {
    int32_t kind;
    int32_t N;            /* batch */
    idh_conv_src src[2];  /* src[1].in == NULL when unused */
    const float *bias;    /* Cout floats (already summed over sources) or NULL */
    const float *res;     /* residual NHWC (same Ho x Wo) or NULL */
    float *out;           /* NHWC Ho x Wo x out_cs (or NCHW for the export op) */
    float *ws;            /* split-K partials: split_k x M x Cout_pad floats */
    int32_t res_cs, out_cs;
    int32_t Ho, Wo, Cout;
    int32_t act;          /* IDH_ACT_* */
    float slope;
    int32_t split_k;      /* 1 = no split */
    int32_t tile_m, tile_n; /* direct kernel: wave tile in 16-wide MFMA sub-tiles (1,2,4), 0 = auto;
                               tile_m = 8 / 9 selects the LDS-staged kernel with 8- / 4-row tiles (3x3 stride 1 [+ a 1x1 or a
                               3x3 stride-2 second source], or a LONE 3x3 stride-2 zero-padded source with Cout % 32 == 0 and
                               Wo >= 16 - conv1 of a stride-2 BasicBlock - which runs on the kernel's stride-2 loader);
                               tile_m = IDH_SPLIT_F16X3 selects the split-precision
                               kernel (3x3 stride 1, zero padding, Cout % 64 == 0, Wo >= 16, split_k == 1; src[0].w =
                               idh_pack_conv_weight_split output of the same mode; src[1], if any: a 1x1
                               stride-1 projection of an output-sized tensor, no up / norm); there tile_n = 8
                               selects 8-row instead of 16-row tiles (0 / 16: 16 rows; other values: IDH_EUNSUPPORTED) */
    int32_t group;        /* != 0: consecutive CONV / UPSAMPLE2 ops with the same id are mutually independent (one
                               dependency level of the plan, see idh_schedule_ops below) and may be launched as
                               ONE grid: runs of 4-row LDS convs with equal channel tiles always are; a mixed run
                               (4-row LDS convs with 64- / 32-channel tiles, the 16x64-tile direct conv, bilinear
                               upsampling) is when each member has <= 512 workgroups, i.e. at small batch */
} idh_op;

/* Repack OIHW conv weights (reference nn.Conv2d layout) for the MFMA B-fragment loads:
 * dst[tap][ci/4][co][ci%4], zero padded to Cin_pad = ceil16(Cin), Cout_pad = ceil16(Cout).
 * dst must hold idh_packed_weight_floats(Cout,Cin,ks) floats. */
size_t idh_packed_weight_floats(int Cout, int Cin, int ks);
int idh_pack_conv_weight(const float *w_oihw, float *dst, int Cout, int Cin, int ks, void *stream);

/* Split-precision convolution (csrc/conv_split.hip), opt-in: fp32 operands expanded into 16-bit pieces,
 * cross products accumulated in fp32 on the f16 matrix cores — fp32-equivalent results
 * (error ~4e-7 of the output scale, like an fp32 FMA chain) at 3/16 of the fp32-MFMA cost.
 *   IDH_SPLIT_F16X3:  x/s = x0+x1 (2 f16 pieces, power-of-two scaling per output channel for the
 *                     weights and per halo chunk for the activations), 3 products.
 * Packed weights: [Cin_pad/16][tap row 3][Cout/64][tap in row 3][piece][ci half 2][co 64][8] 16-bit,
 * followed by Cout per-channel scale floats and Cout exponents.  3x3 kernels, Cout % 64 == 0
 * (IDH_EUNSUPPORTED otherwise).
 * A fused 1x1 second source (src[1]: BasicBlock's downsample(x)) is packed into the same blob
 * (w_1x1 = (Cout, Cin_1x1) row-major or NULL / 0): [3x3 panels][1x1 panels: Cin_1x1_pad/16 x Cout/64 x
 * piece x half x 64 x 8][scales]; src[1].w is then ignored by the kernel (but must be non-NULL).  src[1] must be exactly that: ks = 1,
 * stride = 1, H x W = Ho x Wo, no up_in, no norm.  Any other second source - the 3x3 stride-2 projection the LDS-staged kernel takes
 * included - is refused with IDH_EUNSUPPORTED (until ABI 109 that one was accepted and computed as if it were 1x1). */
#define IDH_SPLIT_F16X3 11
size_t idh_packed_split_weight_bytes(int Cout, int Cin, int Cin_1x1, int mode);
int idh_pack_conv_weight_split(const float *w_oihw, const float *w_1x1, void *dst, int Cout, int Cin, int Cin_1x1, int mode,
                               void *stream);

/* Winograd F(2x2,3x3) convolution (csrc/conv_wino.hip): the same fp32 operands and fp32 accumulation on
 * v_mfma_f32_16x16x4_f32, with 16 instead of 36 multiplications per 2x2 output tile and input channel (the 3x3
 * stride-1 convs of BasicBlock, layers.py:59-95).  IDH_OP_CONV with tile_m = IDH_TILE_WINO; src[0].w = the output of
 * idh_pack_conv_weight_wino (U = G g G^T per (co, ci), in MFMA A-fragment order:
 * [Cin_pad/8][Cout_pad/16][position 16][ci pair 4][co 16][2]); tile_n is ignored (32 x 8 pixel x 32 channel tiles).
 * Shape family: 3x3, stride 1, zero padding, Cout % 32 == 0, split_k == 1; src[1] may be a 1x1 stride-1 projection of a
 * tensor of the same size (weights packed by idh_pack_conv_weight as usual); anything else: IDH_EUNSUPPORTED.  Results differ from the direct kernel by fp32 rounding only (~1e-6 of the output scale). */
#define IDH_TILE_WINO 12
size_t idh_packed_wino_weight_floats(int Cout, int Cin);
int idh_pack_conv_weight_wino(const float *w_oihw, float *dst, int Cout, int Cin, void *stream);

/* Winograd F(4x4,3x3) convolution (csrc/conv_wino4.hip, conv3x3_wino4_k): 36 instead of 64 multiplications per 4x4 output pixels
 * and input channel (1.78x fewer MFMAs than IDH_TILE_WINO), fp32 operands and accumulation, interpolation points {0, +-1/2, +-2, inf};
 * for the plain 3x3 stride-1 convs of BasicBlock / the decoders (layers.py:59-95, networks.py:20-215).  IDH_OP_CONV with
 * tile_m = IDH_TILE_WINO4; src[0].w = the output of idh_pack_conv_weight_wino4 (U = G g G^T per (co, ci) in MFMA A-fragment order:
 * [Cin_pad/8][Cout_pad/16][k-step 2][position group 9][lane 64][4], ci = 8 stage + 2 (lane >> 4) + k-step; row g, element e = slot 4 g + e of the kernel's
 * V layout - since ABI 105 a quadrant's nine positions are slots 8 q .. 8 q + 7 and 32 + q (csrc/conv_wino4.hip w4_v2p), quadrant-major before: repack after upgrading);
 * 32 x 8 pixel x 64 channel tiles, the input transform shared through LDS by the four 16-channel waves of a tile, two persistent
 * workgroups per CU.  Shape family: 3x3, stride 1, zero padding, Cin > 16, Cout % 64 == 0, split_k == 1, act NONE / LRELU / ELU; src[1] may be
 * a 1x1 stride-1 projection of a tensor of the output's size (weights packed by idh_pack_conv_weight as usual; then res must be NULL);
 * anything else: IDH_EUNSUPPORTED.  Error against fp64 ~2-7e-6 of
 * the output scale (direct kernel ~1e-6, F(2x2) ~4e-7).  (ABI 101 had a register-transform kernel under this code with another
 * weight layout and code 14 for this one; 102 keeps one kernel, one code.) */
#define IDH_TILE_WINO4 13
size_t idh_packed_wino4_weight_floats(int Cout, int Cin);
int idh_pack_conv_weight_wino4(const float *w_oihw, float *dst, int Cout, int Cin, void *stream);

/* IDH_OP_STEM weights: conv1 (64, 3, 7, 7) OIHW times bn_weight / sqrt(bn_var + eps) in the kernel's MFMA B-fragment order
 * ([channel quarter 4][K-step 42][lane 64], taps kx padded 7 -> 8 with zeros), then the 64 folded biases bn_bias - bn_mean * bn_weight /
 * sqrt(bn_var + eps).  All pointers device memory; dst holds idh_stem_weight_floats() floats. */
size_t idh_stem_weight_floats(void);
int idh_pack_stem_weight(const float *w_oihw, const float *bn_weight, const float *bn_bias, const float *bn_mean, const float *bn_var, float eps,
                         float *dst, void *stream);
/* Eval-mode BatchNorm folded into the conv before it: w_out[o][i] = w[o][i] * s[o], b_out[o] = bn_bias[o] - bn_mean[o] * s[o],
 * s = bn_weight / sqrt(bn_var + eps) in fp32, i < per_out (= Cin * ks * ks).  The layer1 convs of the stem (BasicBlock conv + bn). */
int idh_fold_conv_bn(const float *w, int cout, int per_out, const float *bn_weight, const float *bn_bias, const float *bn_mean,
                     const float *bn_var, float eps, float *w_out, float *b_out, void *stream);

/* sizeof(idh_op) as compiled into the library (bindings assert their mirror matches). */
size_t idh_sizeof_op(void);

/* Launch n ops in order on `stream`. `ops_host` is HOST memory (pointers inside are device). */
int idh_run_ops(const idh_op *ops_host, int n, void *stream);

/* Number of kernel launches idh_run_ops() would issue for these ops (same validation and grouping decisions, nothing
 * is launched; usable without a GPU), or a negative IDH_E* code. */
int idh_count_launches(const idh_op *ops_host, int n);

/* Host-only query (ABI >= 108): the kernel variant idh_run_ops() would launch for ONE IDH_OP_CONV descriptor run alone - the same validation and
 * dispatch decision (nothing is launched, no device access; usable without a GPU).  Returns what idh_run_ops would return for the op
 * (IDH_EINVAL also for a NULL argument or another kind); on IDH_OK fills
 *   out = { lds_rows, nj, tm, tn, S, up, norm, s2 }
 *   lds_rows  8 / 4: LDS-staged 3x3 kernel with 8- / 4-row tiles; 0: direct kernel; 16: split-precision; 32 / 36: Winograd F(2x2) / F(4x4)
 *   nj        LDS kernel: 16-channel output sub-tiles per workgroup (4, 2, 1); 0 otherwise
 *   tm, tn    direct kernel: wave tile in 16-wide sub-tiles; split-precision / Winograd: the tile code and its tile rows; 0 on the LDS kernel
 *   S         split count after clamping to the step / chunk count (1 = the kernel writes final values, ws unused)
 *   up, norm  0 / 1: a source has fused x2-upsampled segments / source 0 is normalised on load
 *   s2        0 / 1: the LDS kernel's stride-2 loader runs (a 3x3 stride-2 second source, or a lone one behind an empty first source)
 * A request the LDS kernel does not cover (tile_m = 8 / 9 with Wo < 16, a Cout its channel tile does not divide, ...) is not an error: it
 * runs on the direct kernel, and only this query tells. */
int idh_conv_variant(const idh_op *op, int32_t out[8]);

/* Kernel selection of one IDH_OP_CONV (ABI >= 111; csrc/plan_select.hip: host only, no device access, usable without a GPU).  THE rule
 * of the library: nhwc.Plan.conv and the C++ plan builder behind include/idh_net.h / idh_model.h both fill a descriptor and take the
 * answer, so the two produce the same op for the same layer by construction. */
typedef struct idh_conv_desc_src {
    int32_t H, W, cs;        /* the source view; 0 where unknown (a size that is 0 passes the 32-bit range checks) */
    int32_t Cin, ks, stride; /* ks 1 / 3; Cin 0: unknown (then never F(4x4)) */
    int32_t is_cat, _r;      /* a fused-upsample concat source (idh_conv_src.up_in) */
} idh_conv_desc_src;

typedef struct idh_conv_desc {
    int32_t N, Ho, Wo, Cout, pad_mode, act;
    float slope;
    int32_t out_cs, res_cs, has_res; /* channel strides of the output / residual tensors (0: unknown) */
    int32_t has_norm;                /* source 0 is normalised on load (idh_conv_src.norm) */
    int32_t any_size;                /* F(4x4) for its whole shape family, whatever the tile count (batch-size-independent rounding) */
    int32_t math;                    /* 0 = fp32, IDH_SPLIT_F16X3 */
    int32_t n_src;                   /* 1 / 2 */
    idh_conv_desc_src src[2];
} idh_conv_desc;

/* Every knob that shapes the choice; the shipped values and their measurements are the module globals of nhwc.py of the same names. */
typedef struct idh_conv_tuning {
    int32_t winograd, winograd4, winograd4_proj, s2_first; /* switches */
    int32_t wino_min_tiles, wino4_min_tiles, split_min_blocks, narrow_tile_below, narrowest_tile_below, split_min_chunks, split_max,
        s2_first_min_blocks, fused_up_rows, target_waves, min_waves, _r;
    double wino_min_fill, wino4_min_fill, proj_chunk_weight;
} idh_conv_tuning;
void idh_conv_tuning_defaults(idh_conv_tuning *t);

#define IDH_W_DIRECT 0 /* idh_pack_conv_weight */
#define IDH_W_WINO 1   /* idh_pack_conv_weight_wino */
#define IDH_W_WINO4 2  /* idh_pack_conv_weight_wino4 */
#define IDH_W_SPLIT 3  /* idh_pack_conv_weight_split (one blob for both sources) */
#define IDH_FAMILY_WINO 1 /* shape families the layer belongs to, whichever of them the cascade picks */
#define IDH_FAMILY_WINO4 2
#define IDH_FAMILY_SPLIT 4
#define IDH_FAMILY_LDS 8
#define IDH_FAMILY_S2_FIRST 16

typedef struct idh_conv_choice {
    int32_t tile_m, tile_n, split_k; /* what the idh_op carries */
    int32_t w_layout;                /* IDH_W_*: packed layout of src[0].w (the other source: IDH_W_DIRECT, or the same blob for IDH_W_SPLIT) */
    int32_t families;                /* IDH_FAMILY_* bits */
    /* the choosers on their own, whatever family wins: LDS-staged kernel (0 unless Cout % 16 == 0), split-precision tile rows, direct kernel */
    int32_t lds_tile_m, lds_split_k, lds_subtiles, split_rows, direct_tile_m, direct_tile_n, direct_split_k;
} idh_conv_choice;

/* IDH_EINVAL: NULL desc / out, n_src not 1 / 2, ks not 1 / 3, non-positive N / Ho / Wo / Cout, a negative size of a source, an unknown math, tuning->split_min_chunks < 1.  tuning == NULL: the defaults. */
int idh_conv_select(const idh_conv_desc *desc, const idh_conv_tuning *tuning, idh_conv_choice *out);
/* sizeof of the three structs as compiled into the library: out = { desc, tuning, choice } */
void idh_sizeof_conv_select(size_t out[3]);

/* The level scheduler of a plan (ABI >= 111; host only): ops [0, n_first) and [n_first, n) are two segments, each levelled on its own (a kernel
 * outside the plan may run between them).  An op's level = 1 + the highest level of an earlier op of its segment it depends on (read after write,
 * write after write, write after read of overlapping regions); each segment is sorted IN PLACE by (level, launch rank, build index), and `group`
 * is set to level + 1 for the ops a grouped launch can host (idh_op.group) and to 0 for the others.  Regions are (buffer id, first channel,
 * one-past-last channel) triples in `regions`; op k reads regions [offsets[2k], offsets[2k+1]) and writes [offsets[2k+1], offsets[2k+2]).
 * order[i] (optional) = the build index of the op now at position i, levels[i] (optional) = its level. */
#define IDH_SCHED_MERGE_LEVELS 1 /* the direct 16x64-tile conv, bilinear upsampling and layout imports of a level join its group (level_k) */
#define IDH_SCHED_WINO_GROUP 2   /* the F(2x2) convs of a level lead it, under its group id (conv3x3_wino_group_k) */
int idh_schedule_ops(idh_op *ops, int n, int n_first, const uint64_t *regions, const int32_t *offsets, int flags, int32_t *order, int32_t *levels);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
