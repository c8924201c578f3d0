// Whole-model entry points (include/idh_model.h): pipeline.HotPath.forward as one C call, for hosts that are not Python.
//
// Composes what exists - the matching-encoder head or the layout import, the volume launchers (idh_cost_volume_dot_ex_fwd / idh_feature_volume_ex_fwd), the conv stage of
// csrc/networks.hip (CVEncoder + UNet++ decoder in ONE op list, nhwc.Plan's kernel choices), the occlusion-MLP / search launchers and
// sample_prior - in the order HotPath.forward enqueues them, with the same arguments, so the results are bit-identical to it
// (tests/test_model_abi_gpu.py).  Device code of its own: the weight-packing gathers (the column maps of cost_volume.py FeatureVolumeManager._packed
// and mlp.py _prepared, which the Python side does with torch indexing) and the sigmoid that hands a frame chain's last prediction to the next call.
#include <cstring>
#include <vector>

#include "idh_common.h"
#include "net_plan.h"
#include "../../include/idh_model.h"

namespace {

using idh_internal::ConvStage;

constexpr int kAbi = 106;
constexpr int kHidden = 128;       // MLP width of both MLPs (reference networks.py:88, cost_volume.py:405-423)
constexpr int kMaxCols = 256;      // gathered columns per launch of pack_cols_k

inline size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

// ---- packing kernels ------------------------------------------------------------------------------------------------------------------------
struct ColMap {
    int n;
    int col[kMaxCols];  // -1: structurally zero column
};

// idh_pack_mlp_weight's fragment order (csrc/mlp.hip pack_mlp_weight_k) over a column-gathered matrix: dst[c][i][lane][4] = W[16i + (lane&15)][cols[k]],
// k = 16c + 4(lane>>4) + e, zero for k >= n or cols[k] < 0 - the bytes FeatureVolumeManager._packed gets from frag(pick(cols))
__global__ __launch_bounds__(256) void pack_cols_k(const float *__restrict__ w, int ld, ColMap cols, float *__restrict__ dst, int cblocks) {
    const int total = cblocks * (kHidden / 16) * 64 * 4;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const int e = t & 3, lane = (t >> 2) & 63, i = (t >> 8) % (kHidden / 16), c = (t >> 8) / (kHidden / 16);
        const int n = 16 * i + (lane & 15), k = 16 * c + 4 * (lane >> 4) + e;
        const int col = k < cols.n ? cols.col[k] : -1;
        dst[t] = col >= 0 ? w[(size_t)n * ld + col] : 0.f;
    }
}

// (128, n) row-major gather of columns [col0, col0 + n): the pose columns (w1_pose_rowmajor)
__global__ __launch_bounds__(256) void gather_cols_k(const float *__restrict__ w, int ld, int col0, int n, float *__restrict__ dst) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < kHidden * n) dst[t] = w[(size_t)(t / n) * ld + col0 + t % n];
}

// b1 + the K "valid" columns, summed in fp64 and rounded once (cost_volume.py _packed, fold_mask)
__global__ __launch_bounds__(128) void fold_bias_k(const float *__restrict__ b1, const float *__restrict__ w, int ld, int col0, int n, float *__restrict__ dst) {
    const int r = threadIdx.x;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += (double)w[(size_t)r * ld + col0 + k];
    dst[r] = (float)((double)(b1 ? b1[r] : 0.f) + s);
}

struct Rows {
    const float *src[6];
    int stride[6], count[6];
};
// rows of 128 floats: row r, element i = src[r][i * stride[r]] for i < count[r], else 0 (the vecs blocks of both MLP kernels)
__global__ __launch_bounds__(128) void rows_k(Rows rows, float *__restrict__ dst) {
    const int r = blockIdx.x, i = threadIdx.x;
    dst[r * kHidden + i] = (rows.src[r] && i < rows.count[r]) ? rows.src[r][(size_t)i * rows.stride[r]] : 0.f;
}

// Thresholder thresholds -> logits, as mlp.infer_depth: log(t / (1 - t))
__global__ __launch_bounds__(256) void thr_logits_k(const float *__restrict__ t, float *__restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float v = t[i];
        out[i] = logf(v / (1.f - v));
    }
}

// prior_out of a frame chain: torch.sigmoid of the last frame's logits (1 / (1 + exp(-x)))
__global__ __launch_bounds__(256) void sigmoid_k(const float *__restrict__ x, float *__restrict__ out, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = 1.f / (1.f + expf(-x[i]));
}

// ---- the feature-volume MLP's column maps (cost_volume.py feature_mlp_column_maps, fold_mask=True: fv_mlp_k, K <= 8, C = 16) -----------------
void fv_column_maps(int K, int C, std::vector<int> &vox, std::vector<int> &pix, int &pose0, int &mask0) {
    const int base = C * (K + 1);
    const int col_plane = base + 2 * K, base_r = base + 4 * K + 1;
    vox.clear(); pix.clear();
    for (int i = 0; i < C * K; ++i) vox.push_back(i);
    for (int cblk = 0; cblk < 4; ++cblk)
        for (int q = 0; q < 4; ++q)
            for (int kk = 0; kk < 4; ++kk) {
                const int idx = 4 * cblk + kk, v = q + 4 * (idx / 6);
                int col = -1;
                if (idx < 12 && v < K) {
                    const int slot = idx % 6;
                    col = slot == 0 ? base + K + v : slot == 1 ? base + 2 * K + 1 + v : slot == 2 ? base + 3 * K + 1 + v : base_r + 3 + 3 * v + (slot - 3);
                } else if ((K < 8 && idx == 6 && q == 3) || (K == 8 && idx == 12 && q == 0)) {
                    col = col_plane;
                }
                vox.push_back(col);
            }
    for (int i = 0; i < C; ++i) pix.push_back(C * K + i);
    for (int q = 0; q < 4; ++q)
        for (int kk = 0; kk < 4; ++kk) pix.push_back((q == 0 && kk < 3) ? base_r + kk : -1);
    pose0 = base_r + 3 * (K + 1);
    mask0 = base;
}

// ---- the layout of one (desc, B): conv stage + the blob / workspace regions around it ---------------------------------------------------------
struct Layout {
    ConvStage cs{};
    int H0 = 0, W0 = 0, F = 0;
    // blob offsets (floats)
    size_t b_fv_w1v = 0, b_fv_w1p = 0, b_fv_pose = 0, b_fv_b1 = 0, b_fv_w2 = 0, b_fv_vecs = 0, b_mlp_w1 = 0, b_mlp_w2 = 0, b_mlp_vecs = 0, b_bins = 0,
           b_thr = 0, blob_floats = 0;
    // workspace offsets (floats)
    size_t w_cur = 0, w_src = 0, w_planes = 0, w_vol = 0, w_prior = 0, w_prior1 = 0, ws_floats = 0;
    size_t vol_ws_bytes = 0;
    long long dot_scratch = 0;
    int n_vox = 0;
    uint64_t key = 0;
};

bool is_bd(const idh_model_desc *d) { return d->kind == IDH_MODEL_BD; }
bool search(const idh_model_desc *d) { return d->query == IDH_QUERY_SEARCH || d->query == IDH_QUERY_SEARCH_THR; }
bool has_prior_buf(const idh_model_desc *d) { return is_bd(d) && (d->prior_mode == IDH_PRIOR_INPUTS || d->prior_mode == IDH_PRIOR_CHAIN); }

int check_desc(const idh_model_desc *d, int B) {
    if (!d || !d->net || B <= 0 || B > 65535) return IDH_EINVAL;
    if (d->kind != IDH_MODEL_BD && d->kind != IDH_MODEL_DEPTH) return IDH_EINVAL;
    if (d->K <= 0 || d->C <= 0 || d->D <= 0 || d->H <= 0 || d->W <= 0) return IDH_EINVAL;
    if (d->volume == IDH_VOLUME_ZERO || d->skip_decoder || d->math != 0 || d->matching_scale != 1) return IDH_EUNSUPPORTED;
    if (d->matching_input != IDH_MATCH_FEATS_NCHW && d->matching_input != IDH_MATCH_LAYER1_NCHW && d->matching_input != IDH_MATCH_LAYER1_NHWC)
        return IDH_EINVAL;
    if (d->matching_input != IDH_MATCH_FEATS_NCHW && d->net->match_head[1].cout != d->C) return IDH_EINVAL;  // the head's 3x3 conv makes the features
    if (d->volume == IDH_VOLUME_FEATURE_MLP) {
        if (d->C != 16 || d->K > 8) return IDH_EUNSUPPORTED;  // fv_mlp_k's folded layout (the shipped configs: K = 7, C = 16)
    } else if (d->volume == IDH_VOLUME_DOT) {
        if ((d->C != 16 && d->C != 32) || d->K > IDH_MAX_SOURCE_VIEWS) return IDH_EUNSUPPORTED;
    } else {
        return IDH_EINVAL;
    }
    if (d->D % 16) return IDH_EUNSUPPORTED;  // the depth counts checked against HotPath (64, 96: no padding channels in the CVEncoder's input)
    if (!(d->min_depth > 0.f) || !(d->max_depth > d->min_depth)) return IDH_EINVAL;
    if (is_bd(d)) {
        if (d->query != IDH_QUERY_PLANES && !search(d)) return IDH_EINVAL;
        if (d->prior_mode < IDH_PRIOR_NONE || d->prior_mode > IDH_PRIOR_CHAIN) return IDH_EINVAL;
        if (d->P <= 0 && (d->query == IDH_QUERY_PLANES || has_prior_buf(d) || d->prior_mode == IDH_PRIOR_WARPED)) return IDH_EINVAL;
        if (d->prior_mode != IDH_PRIOR_NONE && !d->use_prior) return IDH_EINVAL;
        if (d->prior_mode == IDH_PRIOR_CHAIN && search(d)) return IDH_EINVAL;  // (HotPath: frame_chain excludes infer_depth)
        if (search(d) && (d->search_iters <= 0 || d->search_iters > 64)) return IDH_EINVAL;
        if (d->query == IDH_QUERY_SEARCH_THR && d->n_thr_bins <= 0) return IDH_EINVAL;
    }
    return IDH_OK;
}

uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 1099511628211ull; }
    return h;
}

// conv-stage description of (desc, B); the pyramid shapes follow the CVEncoder's strides (checked by the builder)
void stage_of(const idh_model_desc *d, int B, const idh_model_inputs *in, float *const *log_depth, float *const *depth, ConvStage &cs) {
    const idh_model_params *n = d->net;
    cs = ConvStage{};
    cs.enc = n->cv_blocks; cs.n_enc = 4; cs.dec = n->dec_blocks;
    cs.heads = d->kind == IDH_MODEL_DEPTH ? n->depth_heads : nullptr;
    cs.scales = d->kind == IDH_MODEL_DEPTH ? IDH_SCALES_ALL : 0x1;  // the occlusion MLP reads scale 0 only; the 1x1 depth heads are outputs at all four
    cs.N = B; cs.H = d->H; cs.W = d->W; cs.D = d->D;
    int h = d->H, w = d->W;
    for (int i = 0; i < 4; ++i) {  // level i + 1 = CVEncoder level i's output size
        const int st = n->cv_blocks[3 * i].conv1.stride;
        if (st == 1 || st == 2) { h = (h + 2 - 3) / st + 1; w = (w + 2 - 3) / st + 1; }
        const int cimg = n->cv_blocks[3 * i + 1].conv1.cin - n->cv_blocks[3 * i].conv1.cout;
        cs.img[i + 1] = idh_tensor{in ? const_cast<float *>(in->pyramid[i + 1]) : nullptr, IDH_LAYOUT_NCHW, cimg, h, w, 0};
    }
    // level 0 feeds the decoder's right_conv_00 (block 14 of the idh_unetpp_fwd order) at twice level 1's size
    cs.img[0] = idh_tensor{in ? const_cast<float *>(in->pyramid[0]) : nullptr, IDH_LAYOUT_NCHW, n->dec_blocks[14].conv1.cin, 2 * cs.img[1].H, 2 * cs.img[1].W, 0};
    cs.log_depth = log_depth; cs.depth = depth;
    cs.head_mode = d->matching_input == IDH_MATCH_LAYER1_NCHW ? 1 : d->matching_input == IDH_MATCH_LAYER1_NHWC ? 2 : 0;
    cs.K = d->K;
    cs.head = n->match_head;
    cs.layer1 = in ? in->matching_layer1 : nullptr;
}

int layout_of(const idh_model_desc *d, int B, Layout &L) {
    int rc = check_desc(d, B);
    if (rc != IDH_OK) return rc;
    stage_of(d, B, nullptr, nullptr, nullptr, L.cs);
    rc = idh_internal::conv_stage(idh_internal::STAGE_SIZES, &L.cs, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    if (rc != IDH_OK) return rc;
    L.H0 = L.cs.feat0_H; L.W0 = L.cs.feat0_W; L.F = L.cs.feat0_C;
    size_t b = align64(L.cs.weight_floats), w = align64(L.cs.ws_floats);
    auto take = [](size_t &off, size_t n) { const size_t o = off; off = align64(off + n); return o; };
    if (d->volume == IDH_VOLUME_FEATURE_MLP) {
        L.n_vox = d->C * d->K + 64;
        L.b_fv_w1v = take(b, idh_packed_mlp_weight_floats(L.n_vox));
        L.b_fv_w1p = take(b, idh_packed_mlp_weight_floats(d->C + 16));
        L.b_fv_pose = take(b, (size_t)kHidden * 3 * d->K);
        L.b_fv_b1 = take(b, kHidden);
        L.b_fv_w2 = take(b, idh_packed_mlp_weight_floats(kHidden));
        L.b_fv_vecs = take(b, 3 * kHidden);
        L.vol_ws_bytes = idh_feature_volume_workspace_bytes(B);
        L.w_vol = take(w, (L.vol_ws_bytes + 3) / 4);
    } else {
        L.dot_scratch = idh_cost_volume_dot_scratch_floats(B, d->K, d->C, d->H, d->W, d->D);
        if (L.dot_scratch < 0) return (int)L.dot_scratch;
        L.w_vol = take(w, (size_t)L.dot_scratch);
    }
    if (is_bd(d)) {
        L.b_mlp_w1 = take(b, idh_packed_mlp_weight_floats(L.F));
        L.b_mlp_w2 = take(b, idh_packed_mlp_weight_floats(kHidden));
        L.b_mlp_vecs = take(b, 6 * kHidden);
        if (d->query == IDH_QUERY_SEARCH_THR) {
            L.b_bins = take(b, d->n_thr_bins);
            L.b_thr = take(b, d->n_thr_bins);
        }
        const size_t plane = (size_t)L.H0 * L.W0;
        if (has_prior_buf(d)) L.w_prior = take(w, (size_t)B * d->P * plane);
        if (search(d) && d->prior_mode != IDH_PRIOR_NONE && d->P > 1) L.w_prior1 = take(w, (size_t)B * plane);
    }
    if (d->matching_input == IDH_MATCH_FEATS_NCHW) {  // NHWC copies of the caller's features (with the head, its output buffer is read in place)
        L.w_cur = take(w, (size_t)B * d->H * d->W * d->C);
        L.w_src = take(w, (size_t)B * d->K * d->H * d->W * d->C);
    }
    L.w_planes = take(w, d->D);
    L.blob_floats = b;
    L.ws_floats = w;
    // the plan key: ABI, every field of the description but the architecture pointer, B, the conv stage's op list and the sizes
    uint64_t k = 1469598103934665603ull;
    const int abi = kAbi;
    k = fnv(k, &abi, sizeof abi);
    k = fnv(k, d, offsetof(idh_model_desc, net));
    k = fnv(k, &B, sizeof B);
    k = fnv(k, &L.cs.layout_hash, sizeof L.cs.layout_hash);
    k = fnv(k, &L.blob_floats, sizeof L.blob_floats);
    k = fnv(k, &L.ws_floats, sizeof L.ws_floats);
    L.key = k;
    return IDH_OK;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------
struct Range {
    uintptr_t a, b;
};

struct Fwd {
    const idh_model_desc *d;
    const Layout *L;
    const ConvStage *cs;  // the stage as laid out in the caller's workspace (cv_in, feat0)
    const float *blob;
    float *ws;
    const idh_model_inputs *in;
    const idh_model_outputs *out;
    int B;
    hipStream_t st;
};

// before the conv stage's ops: the NCHW import of the matching features and the volume, written NHWC into the CVEncoder's input buffer
// (HotPath.forward steps 0 and 1)
int volume_stage(void *ctx) {
    const Fwd &f = *static_cast<const Fwd *>(ctx);
    const idh_model_desc *d = f.d;
    const Layout &L = *f.L;
    const int B = f.B, K = d->K, C = d->C, H = d->H, W = d->W, D = d->D;
    float *planes = f.ws + L.w_planes;
    const float *cur, *src;
    long long stride = 0;  // batch stride of both feature pointers (floats); 0 = dense (B, ...) / (B, K, ...)
    if (f.cs->match) {  // the head's (B, K+1, H, W, C) output: frame b's current view, then its K sources
        cur = f.cs->match;
        src = f.cs->match + (size_t)H * W * C;
        stride = (long long)(K + 1) * H * W * C;
    } else {
        float *c = f.ws + L.w_cur, *s = f.ws + L.w_src;
        int rc = idh_nchw_to_nhwc_f32(f.in->matching_cur, c, B, C, H * W, f.st);
        if (rc == IDH_OK) rc = idh_nchw_to_nhwc_f32(f.in->matching_src, s, B * K, C, H * W, f.st);
        if (rc != IDH_OK) return rc;
        cur = c; src = s;
    }
    idh_volume_opts o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.cur_batch_stride = o.src_batch_stride = stride;
    if (d->volume == IDH_VOLUME_DOT) {
        if (L.dot_scratch) { o.scratch = f.ws + L.w_vol; o.scratch_floats = L.dot_scratch; }
        return idh_cost_volume_dot_ex_fwd(cur, src, f.in->src_K, f.in->src_cam_T_cur_cam, f.in->cur_invK, d->min_depth, d->max_depth, B, K, C, H, W, D,
                                          f.cs->cv_in, f.cs->cv_cs, f.out->lowest_cost, planes, (L.dot_scratch || stride) ? &o : nullptr, f.st);
    }
    const float *bl = f.blob;
    return idh_feature_volume_ex_fwd(cur, src, f.in->src_K, f.in->src_cam_T_cur_cam, f.in->cur_cam_T_src_cam, f.in->cur_invK, d->min_depth, d->max_depth,
                                     B, K, C, H, W, D, bl + L.b_fv_w1v, bl + L.b_fv_w1p, bl + L.b_fv_pose, bl + L.b_fv_b1, bl + L.b_fv_w2, bl + L.b_fv_vecs,
                                     f.cs->cv_in, f.cs->cv_cs, f.out->lowest_cost, d->return_mask ? f.out->overall_mask : nullptr, planes, f.ws + L.w_vol,
                                     L.vol_ws_bytes, 0, stride ? &o : nullptr, f.st);
}

// step 3 of HotPath.forward: prior warp + occlusion MLP / depth search (BDModel)
int query_stage(const Fwd &f) {
    const idh_model_desc *d = f.d;
    const Layout &L = *f.L;
    const idh_model_inputs *in = f.in;
    const idh_model_outputs *out = f.out;
    const int B = f.B, P = d->P, H0 = L.H0, W0 = L.W0, HW = H0 * W0;
    const float *feat = f.cs->feat0, *w1 = f.blob + L.b_mlp_w1, *w2 = f.blob + L.b_mlp_w2, *vecs = f.blob + L.b_mlp_vecs;
    const int fcs = f.cs->feat0_cs, F = L.F, up = d->use_prior ? 1 : 0;
    float *prior = out->prior_mask ? out->prior_mask : f.ws + L.w_prior;
    int rc = IDH_OK;
    if (d->prior_mode == IDH_PRIOR_CHAIN) {
        // frame b's prior = sample_prior of sigmoid(frame b-1's logits) with frame b-1's cam_T_world (HotPath frame_chain, inference.py:139-157)
        for (int b = 0; b < B && rc == IDH_OK; ++b) {
            const float *pb = nullptr;
            const size_t fo = (size_t)b * P * HW;
            if (b == 0 && in->prior_prediction) {
                rc = idh_sample_prior_fwd(in->rendered_depth, in->prior_prediction, in->prior_channels, in->world_T_cam, in->prior_cam_T_world, in->K_s0,
                                          in->invK_s0, 1, P, H0, W0, prior, f.st);
                pb = prior;
            } else if (b > 0) {
                rc = idh_internal::sample_prior_from_logits(in->rendered_depth + fo, out->pred_0 + fo - (size_t)P * HW, P, in->world_T_cam + 16 * b,
                                                            in->cam_T_world + 16 * (b - 1), in->K_s0 + 16 * b, in->invK_s0 + 16 * b, 1, P, H0, W0,
                                                            prior + fo, f.st);
                pb = prior + fo;
            }
            if (rc == IDH_OK)
                rc = idh_binary_mlp_fwd(feat + (size_t)b * HW * fcs, fcs, F, in->rendered_depth + fo, pb, up, -1.f, w1, w2, vecs, 1, P, HW, out->pred_0 + fo, f.st);
        }
        if (rc == IDH_OK && out->prior_out) {
            const int n = P * HW;
            hipLaunchKernelGGL(sigmoid_k, dim3(std::min(idh_cdiv(n, 256), 2048)), dim3(256), 0, f.st, out->pred_0 + (size_t)(B - 1) * n, out->prior_out, n);
            IDH_CHECK_LAUNCH();
        }
        return rc;
    }
    const float *pr = nullptr;
    if (d->prior_mode == IDH_PRIOR_WARPED) {
        pr = in->prior;
    } else if (d->prior_mode == IDH_PRIOR_INPUTS) {
        rc = idh_sample_prior_fwd(in->rendered_depth, in->prior_prediction, in->prior_channels, in->world_T_cam, in->prior_cam_T_world, in->K_s0, in->invK_s0,
                                  B, P, H0, W0, prior, f.st);
        if (rc != IDH_OK) return rc;
        pr = prior;
    }
    if (!search(d)) return idh_binary_mlp_fwd(feat, fcs, F, in->rendered_depth, pr, up, -1.f, w1, w2, vecs, B, P, HW, out->pred_0, f.st);
    if (pr && P > 1) {  // prior[:, :1].contiguous()
        float *p1 = f.ws + L.w_prior1;
        if (hipMemcpy2DAsync(p1, (size_t)HW * 4, pr, (size_t)P * HW * 4, (size_t)HW * 4, B, hipMemcpyDeviceToDevice, f.st) != hipSuccess) return IDH_ELAUNCH;
        pr = p1;
    }
    if (d->query == IDH_QUERY_SEARCH_THR)
        return idh_binary_mlp_search_thr_fwd(feat, fcs, F, pr, up, -1.f, w1, w2, vecs, B, HW, d->search_iters, d->search_lo, d->search_hi, f.blob + L.b_bins,
                                             f.blob + L.b_thr, d->n_thr_bins, out->search_depths, out->pred_0, f.st);
    return idh_binary_mlp_search_fwd(feat, fcs, F, pr, up, -1.f, w1, w2, vecs, B, HW, d->search_iters, d->search_lo, d->search_hi, d->search_threshold,
                                     out->search_depths, out->pred_0, f.st);
}

bool aligned16(const void *p) { return p && ((uintptr_t)p & 15) == 0; }

// host-side validation of (inputs, outputs): every pointer the call will touch, and no output range overlapping anything else
int check_io(const idh_model_desc *d, const Layout &L, int B, const float *blob, const idh_model_inputs *in, const idh_model_outputs *out, const float *ws) {
    if (!in || !out) return IDH_EINVAL;
    const size_t K = d->K, C = d->C, HWm = (size_t)d->H * d->W, P = d->P > 0 ? d->P : 0, HW0 = (size_t)L.H0 * L.W0;
    std::vector<Range> ins, outs;
    auto add = [](std::vector<Range> &v, const void *p, size_t bytes) {
        if (p && bytes) v.push_back(Range{(uintptr_t)p, (uintptr_t)p + bytes});
        return p != nullptr;
    };
    bool ok = true;
    const bool head = d->matching_input != IDH_MATCH_FEATS_NCHW;
    if (head) ok &= add(ins, in->matching_layer1, 4ull * B * (K + 1) * d->net->match_head[0].cin * HWm);
    else ok &= add(ins, in->matching_cur, 4 * B * C * HWm) && add(ins, in->matching_src, 4 * B * K * C * HWm);
    for (int i = 0; i < 5; ++i) ok &= add(ins, in->pyramid[i], 4ull * B * L.cs.img[i].C * L.cs.img[i].H * L.cs.img[i].W);
    ok &= add(ins, in->src_cam_T_cur_cam, 64 * B * K) && add(ins, in->src_K, 64 * B * K) && add(ins, in->cur_invK, 64ull * B);
    if (d->volume == IDH_VOLUME_FEATURE_MLP) ok &= add(ins, in->cur_cam_T_src_cam, 64 * B * K);
    ok &= add(outs, out->lowest_cost, 4 * B * HWm);
    if (d->volume == IDH_VOLUME_FEATURE_MLP && d->return_mask) ok &= add(outs, out->overall_mask, B * HWm);
    if (d->kind == IDH_MODEL_DEPTH) {
        for (int i = 0; i < 4; ++i) {
            const size_t n = 4ull * B * (L.H0 >> i) * (L.W0 >> i);
            ok &= add(outs, out->log_depth[i], n);
            add(outs, out->depth[i], n);
        }
    } else {
        const bool srch = search(d);
        ok &= add(outs, out->pred_0, 4 * B * (srch ? 1 : P) * HW0);
        if (srch) ok &= add(outs, out->search_depths, 4 * B * HW0);
        if (d->query == IDH_QUERY_PLANES || has_prior_buf(d)) ok &= add(ins, in->rendered_depth, 4 * B * P * HW0);
        if (d->prior_mode == IDH_PRIOR_WARPED) ok &= add(ins, in->prior, 4 * B * P * HW0);
        if (d->prior_mode == IDH_PRIOR_INPUTS || d->prior_mode == IDH_PRIOR_CHAIN) {
            const size_t nb = d->prior_mode == IDH_PRIOR_INPUTS ? B : 1;
            const bool start = in->prior_prediction != nullptr;
            if (d->prior_mode == IDH_PRIOR_INPUTS && !start) return IDH_EINVAL;
            if (start != (in->prior_cam_T_world != nullptr) || (start && in->prior_channels <= 0)) return IDH_EINVAL;
            if (start) ok &= add(ins, in->prior_prediction, 4 * nb * in->prior_channels * HW0) && add(ins, in->prior_cam_T_world, 64 * nb);
            ok &= add(ins, in->world_T_cam, 64ull * B) && add(ins, in->K_s0, 64ull * B) && add(ins, in->invK_s0, 64ull * B);
            if (d->prior_mode == IDH_PRIOR_CHAIN) ok &= add(ins, in->cam_T_world, 64ull * B);
            add(outs, out->prior_mask, 4 * B * P * HW0);
        }
        if (d->prior_mode == IDH_PRIOR_CHAIN) add(outs, out->prior_out, 4 * P * HW0);
    }
    if (!ok) return IDH_EINVAL;
    // 16-byte alignment of the maps the kernels read with vector loads
    if ((head ? !aligned16(in->matching_layer1) : (!aligned16(in->matching_cur) || !aligned16(in->matching_src))) || !aligned16(out->lowest_cost))
        return IDH_EINVAL;
    for (int i = 0; i < 5; ++i)
        if (!aligned16(in->pyramid[i])) return IDH_EINVAL;
    ins.push_back(Range{(uintptr_t)blob, (uintptr_t)(blob + L.blob_floats)});
    ins.push_back(Range{(uintptr_t)ws, (uintptr_t)(ws + L.ws_floats)});
    for (size_t i = 0; i < outs.size(); ++i) {
        for (const Range &r : ins)
            if (outs[i].a < r.b && r.a < outs[i].b) return IDH_EINVAL;
        for (size_t j = 0; j < i; ++j)
            if (outs[i].a < outs[j].b && outs[j].a < outs[i].b) return IDH_EINVAL;
    }
    return IDH_OK;
}

int pack_cols(const float *w, int ld, const std::vector<int> &cols, float *dst, hipStream_t st) {
    if ((int)cols.size() > kMaxCols) return IDH_EUNSUPPORTED;
    ColMap m;
    std::memset(&m, 0, sizeof m);
    m.n = (int)cols.size();
    for (int i = 0; i < m.n; ++i) m.col[i] = cols[i];
    const int cblocks = (m.n + 15) / 16;
    hipLaunchKernelGGL(pack_cols_k, dim3(idh_cdiv(cblocks * (kHidden / 16) * 256, 256)), dim3(256), 0, st, w, ld, m, dst, cblocks);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

int launch_rows(const Rows &r, int n, float *dst, hipStream_t st) {
    hipLaunchKernelGGL(rows_k, dim3(n), dim3(kHidden), 0, st, r, dst);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

}  // namespace

extern "C" int idh_model_sizes(const idh_model_desc *desc, int B, idh_model_size_info *sizes) {
    if (!sizes) return IDH_EINVAL;
    Layout L;
    const int rc = layout_of(desc, B, L);
    if (rc != IDH_OK) return rc;
    sizes->weight_floats = L.blob_floats;
    sizes->workspace_floats = L.ws_floats;
    sizes->plan_key = L.key;
    sizes->conv_ops = L.cs.ops;
    sizes->conv_launches = L.cs.launches;
    return IDH_OK;
}

extern "C" int idh_model_pack(const idh_model_desc *d, const idh_model_params *p, int B, float *blob, void *stream) {
    if (!p || !blob || ((uintptr_t)blob & 255)) return IDH_EINVAL;
    Layout L;
    int rc = layout_of(d, B, L);
    if (rc != IDH_OK) return rc;
    if (d->net != p) {  // the architecture the sizes came from must be the one packed
        Layout L2;
        idh_model_desc d2 = *d;
        d2.net = p;
        rc = layout_of(&d2, B, L2);
        if (rc != IDH_OK) return rc;
        if (L2.key != L.key) return IDH_EINVAL;
    }
    hipStream_t st = idh_stream(stream);
    ConvStage cs;
    stage_of(d, B, nullptr, nullptr, nullptr, cs);
    rc = idh_internal::conv_stage(idh_internal::STAGE_PACK, &cs, nullptr, 0, blob, st, nullptr, nullptr);
    if (rc != IDH_OK) return rc;
    if (d->volume == IDH_VOLUME_FEATURE_MLP) {
        for (int i = 0; i < 3; ++i)
            if (!p->fv_w[i] || !p->fv_b[i]) return IDH_EINVAL;
        const int K = d->K, C = d->C, ld = C * (K + 1) + 10 * K + 4;
        std::vector<int> vox, pix;
        int pose0, mask0;
        fv_column_maps(K, C, vox, pix, pose0, mask0);
        if ((int)vox.size() != L.n_vox) return IDH_EINVAL;
        if ((rc = pack_cols(p->fv_w[0], ld, vox, blob + L.b_fv_w1v, st)) != IDH_OK) return rc;
        if ((rc = pack_cols(p->fv_w[0], ld, pix, blob + L.b_fv_w1p, st)) != IDH_OK) return rc;
        hipLaunchKernelGGL(gather_cols_k, dim3(idh_cdiv(kHidden * 3 * K, 256)), dim3(256), 0, st, p->fv_w[0], ld, pose0, 3 * K, blob + L.b_fv_pose);
        IDH_CHECK_LAUNCH();
        hipLaunchKernelGGL(fold_bias_k, dim3(1), dim3(kHidden), 0, st, p->fv_b[0], p->fv_w[0], ld, mask0, K, blob + L.b_fv_b1);
        IDH_CHECK_LAUNCH();
        if ((rc = idh_pack_mlp_weight(p->fv_w[1], blob + L.b_fv_w2, kHidden, 0, kHidden, st)) != IDH_OK) return rc;
        const Rows r{{p->fv_b[1], p->fv_w[2], p->fv_b[2], nullptr, nullptr, nullptr}, {1, 1, 1, 0, 0, 0}, {kHidden, kHidden, 1, 0, 0, 0}};
        if ((rc = launch_rows(r, 3, blob + L.b_fv_vecs, st)) != IDH_OK) return rc;
    }
    if (is_bd(d)) {
        for (int i = 0; i < 3; ++i)
            if (!p->mlp_w[i] || !p->mlp_b[i]) return IDH_EINVAL;
        const int F = L.F, ld = 1 + F + (d->use_prior ? 1 : 0);
        if ((rc = idh_pack_mlp_weight(p->mlp_w[0], blob + L.b_mlp_w1, ld, 1, F, st)) != IDH_OK) return rc;
        if ((rc = idh_pack_mlp_weight(p->mlp_w[1], blob + L.b_mlp_w2, kHidden, 0, kHidden, st)) != IDH_OK) return rc;
        // vecs6x128 = {b1, W1[:, depth], W1[:, prior], b2, W3[0, :], [b3, 0 ...]} (mlp.py _prepared)
        const Rows r{{p->mlp_b[0], p->mlp_w[0], d->use_prior ? p->mlp_w[0] + F + 1 : nullptr, p->mlp_b[1], p->mlp_w[2], p->mlp_b[2]},
                     {1, ld, ld, 1, 1, 1},
                     {kHidden, kHidden, kHidden, kHidden, kHidden, 1}};
        if ((rc = launch_rows(r, 6, blob + L.b_mlp_vecs, st)) != IDH_OK) return rc;
        if (d->query == IDH_QUERY_SEARCH_THR) {
            if (!p->thr_bins || !p->thr_values) return IDH_EINVAL;
            if (hipMemcpyAsync(blob + L.b_bins, p->thr_bins, sizeof(float) * d->n_thr_bins, hipMemcpyDeviceToDevice, st) != hipSuccess) return IDH_ELAUNCH;
            hipLaunchKernelGGL(thr_logits_k, dim3(idh_cdiv(d->n_thr_bins, 256)), dim3(256), 0, st, p->thr_values, blob + L.b_thr, d->n_thr_bins);
            IDH_CHECK_LAUNCH();
        }
    }
    return IDH_OK;
}

extern "C" int idh_model_fwd(const idh_model_desc *d, const float *blob, size_t weight_floats, uint64_t plan_key, int B, const idh_model_inputs *in,
                             const idh_model_outputs *out, float *ws, size_t ws_floats, void *stream) {
    Layout L;
    int rc = layout_of(d, B, L);
    if (rc != IDH_OK) return rc;
    if (plan_key != L.key || weight_floats != L.blob_floats) return IDH_EINVAL;  // a blob packed for another (desc, B): never read
    if (!blob || ((uintptr_t)blob & 255)) return IDH_EINVAL;
    if (!ws || ((uintptr_t)ws & 255) || ws_floats < L.ws_floats) return IDH_EWORKSPACE;
    if ((rc = check_io(d, L, B, blob, in, out, ws)) != IDH_OK) return rc;
    ConvStage cs;
    stage_of(d, B, in, d->kind == IDH_MODEL_DEPTH ? out->log_depth : nullptr, d->kind == IDH_MODEL_DEPTH ? out->depth : nullptr, cs);
    Fwd f{d, &L, &cs, blob, ws, in, out, B, idh_stream(stream)};
    // the stage occupies the head of the workspace and of the blob (the same layout the size query computed); the volume runs inside it,
    // after the op list is built and before its first op
    rc = idh_internal::conv_stage(idh_internal::STAGE_RUN, &cs, ws, L.cs.ws_floats, const_cast<float *>(blob), f.st, volume_stage, &f);
    if (rc != IDH_OK || !is_bd(d)) return rc;
    return query_stage(f);
}
