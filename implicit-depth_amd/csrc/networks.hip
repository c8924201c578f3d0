// Network-level entry points of the conv stage (include/idh_net.h): BasicBlock, CVEncoder, the UNet++ decoders as host-side builders over
// idh_run_ops.  Replaces BasicBlock.forward (reference modules/layers.py:78-95), CVEncoder.forward (modules/networks.py:186-215) and
// BDDecoderPP / DepthDecoderPP.forward (modules/networks.py:64-84, 163-183) for hosts that are not Python.
//
// This file contains NO kernels of its own except a bias adder: it is the plan builder of implicit-depth_amd/nhwc.py's Plan for hosts without Python (fp32
// arithmetic, default tuning) - buffers carved out of the caller's workspace, packed weights out of the caller's blob, the same concat elimination
// (producers write channel slices), the same liveness reuse of the big activation temporaries.  Kernel, tile and split-K of every conv come from
// idh_conv_select and the dependency-level schedule with its launch groups from idh_schedule_ops (csrc/plan_select.hip), the functions nhwc.py calls
// too - so a pass is the same op list the Python drop-ins replay and the results are bit-identical to theirs (tests/test_net_abi_gpu.py compares
// the two, and both with the reference's goldens).
#include <algorithm>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "idh_common.h"
#include "net_plan.h"
#include "../../include/idh_net.h"
#include "../../include/idh_ops.h"

namespace {

// ---- the switches of nhwc.py this builder mirrors (the defaults; the Python side can be re-tuned at run time, this side is the shipped setting)
constexpr long long kReuseMinBytes = 64ll << 20;  // REUSE_MIN_BYTES
constexpr bool kFuseHeadNorm = true;      // FUSE_HEAD_NORM (matching-encoder head: InstanceNorm + LeakyReLU applied by the 3x3 conv on load)
constexpr bool kFuseHeadImport = true;    // FUSE_HEAD_IMPORT (... and its 1x1 conv reading the backbone's NCHW map in place)

inline int ceil16(int v) { return (v + 15) & ~15; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

__global__ __launch_bounds__(256) void bias_sum_k(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (a ? a[i] : 0.f) + (b ? b[i] : 0.f);
}

enum Mode { MODE_SIZES, MODE_PACK, MODE_RUN };

// idh_debug_set_plan_observer (include/idh_net.h): called by Plan::finish with the scheduled op list; host only, off by default
idh_plan_observer g_observer = nullptr;
void *g_observer_user = nullptr;

// Addresses of a plan that is never run (MODE_SIZES / MODE_PACK): nothing dereferences them, but a plan audit reads them, so two distinct tensors
// never share a float - 16 TiB per class, 256 GiB per caller-owned tensor (the largest, B = 32 at 384 x 512, stays under 2 GiB)
constexpr int kFakeClassShift = 44, kFakeTensorShift = 38;
enum FakeClass : uintptr_t { FAKE_WS = 1, FAKE_EXTERNAL = 2, FAKE_BLOB = 3, FAKE_PHANTOM = 7 };
inline float *fake_address(FakeClass c, size_t index = 0) {
    return reinterpret_cast<float *>(((uintptr_t)c << kFakeClassShift) + ((uintptr_t)index << kFakeTensorShift));
}

struct Buf {
    float *base;  // device address of channel 0 of pixel 0 (a fake, aligned address in MODE_SIZES / MODE_PACK)
    int N, H, W, cs;
    bool internal;
    bool zero_fill;  // internal buffer with padding channels: cleared on the stream before the pass
    size_t floats;
};

struct View {
    int buf = -1, c0 = 0, C = 0;
};

struct Region {
    uint64_t buf, c0, c1;  // (idh_schedule_ops' triple)
};

struct Meta {
    std::vector<Region> reads, writes;
};

struct Src {
    View v;
    const idh_conv_params *cv;
};

// normalise-on-load of a conv's first source (idh_conv_src.norm): the statistics an IDH_OP_INSTNORM leaves in its workspace
struct Norm {
    const float *stats = nullptr;
    int buf = -1;  // pseudo-buffer of the statistics (dependency tracking only)
    int act = IDH_ACT_NONE;
    float slope = 0.2f;
};

class Plan {
  public:
    Plan(Mode mode, float *ws, size_t ws_cap, float *blob, hipStream_t st) : mode_(mode), ws_(ws), ws_cap_(ws_cap), blob_(blob), st_(st) {
        if (mode_ != MODE_RUN) ws_ = fake_address(FAKE_WS);   // fake, aligned: only offsets matter
        if (mode_ == MODE_SIZES) blob_ = fake_address(FAKE_BLOB);
    }

    int err = IDH_OK;
    std::vector<idh_op> ops;
    std::vector<Meta> meta;
    std::vector<Buf> bufs;
    size_t ws_off = 0, blob_off = 0;
    int n_wino4 = 0, n_wino2 = 0, recycled = 0;

    int N(const View &v) const { return bufs[v.buf].N; }
    int H(const View &v) const { return bufs[v.buf].H; }
    int W(const View &v) const { return bufs[v.buf].W; }
    int cs(const View &v) const { return bufs[v.buf].cs; }
    float *ptr(const View &v) const { return bufs[v.buf].base + v.c0; }
    static View slice(const View &v, int c0, int C) { return View{v.buf, v.c0 + c0, C}; }

    float *ws_alloc(size_t floats) {
        float *p = ws_ + ws_off;
        ws_off = align64(ws_off + floats);
        if (mode_ == MODE_RUN && ws_off > ws_cap_) err = IDH_EWORKSPACE;
        return p;
    }
    float *blob_alloc(size_t floats) {
        float *p = blob_ + blob_off;
        blob_off = align64(blob_off + floats);
        return p;
    }

    // Dense NHWC buffer of the plan (Plan.buffer): channel counts that are not a multiple of 16 get zero padding channels
    View buffer(int n, int h, int w, int c) {
        const int cs_ = ceil16(c);
        if (dry_) return phantom(n, h, w, c, cs_);
        if (cs_ == c) {
            auto it = free_.find(std::make_tuple(n, h, w, cs_));
            if (it != free_.end() && !it->second.empty()) {
                const int b = it->second.back();
                it->second.pop_back();
                ++recycled;
                return View{b, 0, c};
            }
        }
        Buf b{};
        b.N = n; b.H = h; b.W = w; b.cs = cs_; b.internal = true; b.zero_fill = cs_ != c;
        b.floats = (size_t)n * h * w * cs_;
        b.base = ws_alloc(b.floats);
        bufs.push_back(b);
        return View{(int)bufs.size() - 1, 0, c};
    }
    // A view with a shape and no memory, for reserve_block: the kernel-family predicates see the dimensions, nothing is allocated or pooled
    View phantom(int n, int h, int w, int c, int cs_) {
        Buf b{};
        b.N = n; b.H = h; b.W = w; b.cs = cs_; b.internal = false; b.zero_fill = false;
        b.base = fake_address(FAKE_PHANTOM, bufs.size());
        bufs.push_back(b);
        return View{(int)bufs.size() - 1, 0, c};
    }
    // A caller-owned tensor of a plan that is never run: each gets an address range of its own
    float *fake_tensor() { return fake_address(FAKE_EXTERNAL, n_fake_++); }
    // A pointer the caller hands in: itself in a plan that runs, else the next made-up tensor (one fake_tensor() per call, in recording order)
    template <class T> T *caller_ptr(T *p) { return mode_ == MODE_RUN ? p : fake_tensor(); }
    // A caller-owned NHWC tensor as a view (read or written in place)
    View external(const idh_tensor &t, int n) {
        Buf b{};
        b.N = n; b.H = t.H; b.W = t.W; b.cs = t.cs; b.internal = false; b.zero_fill = false;
        b.base = caller_ptr(t.ptr);
        bufs.push_back(b);
        return View{(int)bufs.size() - 1, 0, t.C};
    }
    // Plan.release: the caller records no further op on `v` (a whole internal buffer): a later buffer() of the same shape may alias it
    void release(const View &v) {
        const Buf &b = bufs[v.buf];
        if (!b.internal || v.c0 != 0 || v.C != b.cs || (long long)b.floats * 4 < kReuseMinBytes) return;
        auto &pool = free_[std::make_tuple(b.N, b.H, b.W, b.cs)];
        if (std::find(pool.begin(), pool.end(), v.buf) != pool.end()) { err = IDH_EINVAL; return; }
        pool.push_back(v.buf);
    }

    static Region region(const View &v, bool pad16 = false) { return Region{(uint64_t)v.buf, (uint64_t)v.c0, (uint64_t)(v.c0 + (pad16 ? ceil16(v.C) : v.C))}; }

    // ---- kernel selection: idh_conv_select on the shapes of the views (nhwc.Plan.conv asks the same function) ----------------------------------
    int select(const std::vector<Src> &srcs, const View &out, int act, float slope, const View *res, int pad_mode, bool norm, bool any_size,
               idh_conv_choice *c) const {
        idh_conv_desc d{};
        d.N = N(out); d.Ho = H(out); d.Wo = W(out); d.Cout = srcs[0].cv->cout; d.pad_mode = pad_mode; d.act = act; d.slope = slope;
        d.out_cs = cs(out); d.has_res = res != nullptr; d.res_cs = res ? cs(*res) : 0; d.has_norm = norm; d.any_size = any_size;
        d.n_src = (int)srcs.size();
        for (size_t i = 0; i < srcs.size(); ++i) {
            const View &v = srcs[i].v;
            d.src[i] = idh_conv_desc_src{H(v), W(v), cs(v), srcs[i].cv->cin, srcs[i].cv->ks, srcs[i].cv->stride, 0, 0};
        }
        return idh_conv_select(&d, nullptr, c);
    }

    // ---- weights -----------------------------------------------------------------------------------------------------------------------
    const float *packed(const idh_conv_params &cv, int lay) {  // lay: IDH_W_DIRECT / _WINO / _WINO4
        size_t n = 0;
        if (lay == IDH_W_WINO4) n = idh_packed_wino4_weight_floats(cv.cout, cv.cin);
        else if (lay == IDH_W_WINO) n = idh_packed_wino_weight_floats(cv.cout, cv.cin);
        else n = idh_packed_weight_floats(cv.cout, cv.cin, cv.ks);
        float *dst = blob_alloc(n);
        if (mode_ == MODE_PACK) {
            if (!cv.weight) { err = IDH_EINVAL; return dst; }
            int rc;
            if (lay == IDH_W_WINO4) rc = idh_pack_conv_weight_wino4(cv.weight, dst, cv.cout, cv.cin, st_);
            else if (lay == IDH_W_WINO) rc = idh_pack_conv_weight_wino(cv.weight, dst, cv.cout, cv.cin, st_);
            else rc = idh_pack_conv_weight(cv.weight, dst, cv.cout, cv.cin, cv.ks, st_);
            if (rc != IDH_OK) err = rc;
        }
        return dst;
    }
    const float *bias_of(const idh_conv_params &a, const idh_conv_params *b) {
        // (the blob always holds cout floats per conv launch: a layer's kernel then never reads the caller's parameter memory)
        float *dst = blob_alloc(a.cout);
        if (mode_ == MODE_PACK) {
            hipLaunchKernelGGL(bias_sum_k, dim3(cdiv(a.cout, 256)), dim3(256), 0, st_, a.bias, b ? b->bias : nullptr, dst, a.cout);
            if (hipGetLastError() != hipSuccess) err = IDH_ELAUNCH;
        }
        return dst;
    }

    // ---- recording (Plan._record / _fill_src): every op below is zeroed by new_op and enters the plan through push, with the regions
    // idh_schedule_ops orders it by
    static idh_op new_op(int kind, int n) {
        idh_op op;
        std::memset(&op, 0, sizeof op);
        op.kind = kind; op.N = n;
        return op;
    }
    void src_of(idh_conv_src &s, const View &v) const { s.in = ptr(v); s.cs = cs(v); s.H = H(v); s.W = W(v); s.Cin = v.C; }
    void push(const idh_op &op, Meta m) {
        ops.push_back(op);
        meta.push_back(std::move(m));
    }

    // ---- ops (Plan.conv / upsample2 / import_nchw / export_nchw / head) ---------------------------------------------------------------------
    View conv(const View &x, const idh_conv_params &cv, const View &out, int act, float slope, const View *res, const View *x2, const idh_conv_params *cv2,
              int pad_mode = IDH_PAD_ZEROS, const Norm *norm = nullptr, bool wino4_any_size = false) {
        if (err) return out;
        idh_op op = new_op(IDH_OP_CONV, N(x));
        std::vector<Src> srcs{{x, &cv}};
        if (x2) srcs.push_back({*x2, cv2});
        const int n = N(out), Ho = H(out), Wo = W(out), cout = cv.cout;
        if (out.C != cout) { err = IDH_EINVAL; return out; }
        idh_conv_choice ch;
        if ((err = select(srcs, out, act, slope, res, pad_mode, norm != nullptr, wino4_any_size, &ch)) != IDH_OK) return out;
        for (size_t i = 0; i < srcs.size(); ++i) {
            const View &v = srcs[i].v;
            const idh_conv_params &c = *srcs[i].cv;
            if (v.C != c.cin || (c.ks != 1 && c.ks != 3) || c.cout != cout) { err = IDH_EINVAL; return out; }
            if (v.C % 16 && (v.c0 != 0 || cs(v) != ceil16(v.C))) { err = IDH_EINVAL; return out; }  // odd channel counts: whole zero-padded buffers only
            idh_conv_src &s = op.src[i];
            src_of(s, v);
            s.w = packed(c, i == 0 ? ch.w_layout : IDH_W_DIRECT); s.ks = c.ks; s.stride = c.stride; s.pad_mode = pad_mode;
        }
        op.bias = bias_of(cv, cv2);  // (always present in the blob - BasicBlock's convs all have one, layers.py:52-55; a NULL bias packs as zeros)
        if (res) { op.res = ptr(*res); op.res_cs = cs(*res); }
        op.out = ptr(out); op.out_cs = cs(out);
        op.Ho = Ho; op.Wo = Wo; op.Cout = cout;
        op.act = act; op.slope = slope;
        const long long M = (long long)n * Ho * Wo;
        const int tm = ch.tile_m, tn = ch.tile_n, split = ch.split_k;
        n_wino4 += tm == IDH_TILE_WINO4 && !dry_;
        n_wino2 += tm == IDH_TILE_WINO && !dry_;
        op.tile_m = tm; op.tile_n = tn; op.split_k = split;
        if (norm) {  // (Plan.conv: the LDS-staged kernel with 16-channel tiles and one source only)
            if ((tm != 8 && tm != 9) || tn != 1 || x2) { err = IDH_EINVAL; return out; }
            op.src[0].norm = norm->stats; op.src[0].norm_act = norm->act; op.src[0].norm_slope = norm->slope;
        }
        if (dry_) return out;  // (reserve_block: the blob slots are taken, in the layout this conv's kernel reads; no op, no workspace)
        if (split > 1) op.ws = ws_alloc((size_t)split * M * ceil16(cout));
        Meta m{{}, {region(out)}};
        if (res) m.reads.push_back(region(*res));
        if (norm) m.reads.push_back(Region{(uint64_t)norm->buf, 0, 1});
        for (const Src &s : srcs) m.reads.push_back(region(s.v, true));
        push(op, m);
        return out;
    }
    void upsample2(const View &x, const View &out) {
        if (err) return;
        idh_op op = new_op(IDH_OP_UPSAMPLE2, N(x));
        src_of(op.src[0], x);
        op.out = ptr(out); op.out_cs = cs(out);
        push(op, Meta{{region(x)}, {region(out)}});
    }
    void import_nchw(const float *src, int n, int C, int H_, int W_, const View &out) {
        if (err) return;
        if (n != N(out) || H_ != H(out) || W_ != W(out) || C != out.C) { err = IDH_EINVAL; return; }
        idh_op op = new_op(IDH_OP_NCHW_TO_NHWC, n);
        op.src[0].in = caller_ptr(src);
        op.src[0].H = H_; op.src[0].W = W_; op.src[0].Cin = C;
        op.out = ptr(out); op.out_cs = cs(out);
        push(op, Meta{{}, {region(out)}});
    }
    void export_nchw(const View &x, float *dst) {
        if (err) return;
        idh_op op = new_op(IDH_OP_NHWC_TO_NCHW, N(x));
        src_of(op.src[0], x);
        op.out = caller_ptr(dst);
        push(op, Meta{{region(x)}, {}});
    }
    void head(const View &x, const idh_conv_params &cv, float *out, float *out_exp) {
        if (err) return;
        if (cv.cout != 1 || cv.ks != 1 || cv.cin != x.C) { err = IDH_EINVAL; return; }
        float *w = blob_alloc(cv.cin), *b = blob_alloc(1);
        if (mode_ == MODE_PACK) {
            if (!cv.weight || !cv.bias) { err = IDH_EINVAL; return; }
            if (hipMemcpyAsync(w, cv.weight, sizeof(float) * cv.cin, hipMemcpyDeviceToDevice, st_) != hipSuccess ||
                hipMemcpyAsync(b, cv.bias, sizeof(float), hipMemcpyDeviceToDevice, st_) != hipSuccess) err = IDH_ELAUNCH;
        }
        idh_op op = new_op(IDH_OP_POINTWISE_HEAD, N(x));
        src_of(op.src[0], x);
        op.src[0].w = w;
        op.bias = b;
        op.out = caller_ptr(out);
        op.ws = mode_ == MODE_RUN ? out_exp : nullptr;
        push(op, Meta{{region(x)}, {}});
    }

    // Plan.instance_norm: nn.InstanceNorm2d (no affine, eps 1e-5) [+ LeakyReLU]; out == nullptr: statistics only, for a normalise-on-load conv
    Norm instance_norm(const View &x, const View *out, int act, float slope) {
        Norm nm;
        if (err) return nm;
        if (x.C % 4 || 256 % (x.C / 4)) { err = IDH_EINVAL; return nm; }
        const int nchunks = cdiv(H(x) * W(x), 1024);
        float *w = ws_alloc((size_t)N(x) * (nchunks + 1) * 2 * x.C);
        idh_op op = new_op(IDH_OP_INSTNORM, N(x));
        src_of(op.src[0], x);
        op.act = act; op.slope = slope;
        if (out) { op.out = ptr(*out); op.out_cs = cs(*out); }
        op.ws = w;
        Meta m{{region(x)}, {}};
        if (out) {
            m.writes.push_back(region(*out));
        } else {
            Buf b{};  // the statistics as a pseudo-buffer: a dependency between this op and the conv that reads them
            b.base = w + (size_t)N(x) * nchunks * 2 * x.C; b.N = N(x); b.H = 1; b.W = 1; b.cs = 1; b.internal = false;
            bufs.push_back(b);
            nm.stats = b.base; nm.buf = (int)bufs.size() - 1;
            m.writes.push_back(Region{(uint64_t)nm.buf, 0, 1});
        }
        push(op, m);
        return nm;
    }
    static bool pointwise_nchw_eligible(const idh_conv_params &c) { return c.ks == 1 && c.stride == 1 && c.cin == 64 && c.cout == 128; }
    // Plan.pointwise_nchw: 1x1 conv read straight from a dense (n, C, H, W) tensor into an NHWC view
    void pointwise_nchw(const float *src, int n, int C, int H_, int W_, const idh_conv_params &cv, const View &out) {
        if (err) return;
        if (n != N(out) || H_ != H(out) || W_ != W(out) || C != cv.cin || out.C != cv.cout || !pointwise_nchw_eligible(cv)) { err = IDH_EINVAL; return; }
        idh_op op = new_op(IDH_OP_POINTWISE_NCHW, n);
        idh_conv_src &s = op.src[0];
        s.in = caller_ptr(src);
        s.w = packed(cv, IDH_W_DIRECT); s.H = H_; s.W = W_; s.Cin = C; s.ks = 1; s.stride = 1;
        op.bias = bias_of(cv, nullptr);
        op.out = ptr(out); op.out_cs = cs(out); op.Ho = H_; op.Wo = W_; op.Cout = cv.cout;
        push(op, Meta{{}, {region(out)}});
    }

    // ---- the fused ResNet18 stem pass (Plan.stem): N dense NCHW images -> NHWC 64-channel view
    void stem(const float *images, int n, int h, int w, const float *blob, const View &out) {
        if (err) return;
        idh_op op = new_op(IDH_OP_STEM, n);
        idh_conv_src &s = op.src[0];
        s.in = caller_ptr(images);
        s.w = blob; s.H = h; s.W = w; s.Cin = 3;
        s.up_C = n; s.up_cs[0] = 3 * h * w; s.up_cs[1] = n * 3 * h * w;  // (Plan.stem: one group of N dense images)
        op.out = ptr(out); op.out_cs = cs(out); op.Ho = H(out); op.Wo = W(out); op.Cout = 64;
        push(op, Meta{{}, {region(out)}});
    }

    // ---- BasicBlock (Plan.basic_block; reference layers.py:78-95) ------------------------------------------------------------------------------
    View basic_block(const View &x, const idh_block_params &blk, const View *out_opt = nullptr) {
        const int st = blk.conv1.stride;
        if (st != 1 && st != 2) { err = IDH_EINVAL; return x; }
        const int Ho = (H(x) + 2 - 3) / st + 1, Wo = (W(x) + 2 - 3) / st + 1;
        const int planes = blk.conv1.cout;
        const View h = buffer(N(x), Ho, Wo, planes);
        conv(x, blk.conv1, h, IDH_ACT_LRELU, 0.2f, nullptr, nullptr, nullptr);
        const View out = out_opt ? *out_opt : buffer(N(x), Ho, Wo, planes);
        if (H(out) != Ho || W(out) != Wo) { err = IDH_EINVAL; return out; }
        if (blk.downsample.ks == 0) {
            if (x.C != planes || st != 1) { err = IDH_EINVAL; return out; }
            conv(h, blk.conv2, out, IDH_ACT_LRELU, 0.2f, &x, nullptr, nullptr);
        } else {
            conv(h, blk.conv2, out, IDH_ACT_LRELU, 0.2f, nullptr, &x, &blk.downsample);
        }
        release(h);  // the block's intermediate dies with conv2
        return out;
    }

    // The blob slots of a BasicBlock that this pass does not run (a decoder scale the caller does not read): the same packed() / bias_of()
    // calls, with the same kernel selection, as basic_block(x, blk) would make - MODE_PACK fills them, so a blob serves every scale mask -
    // and nothing else: no op, no buffer, no workspace.  out_cs: the pixel stride of the caller's NHWC output tensor (0: a plan buffer).
    void reserve_block(const View &x, const idh_block_params &blk, int out_cs) {
        dry_ = true;
        if (out_cs) {
            const int st = blk.conv1.stride == 2 ? 2 : 1;
            const View o = phantom(N(x), (H(x) + 2 - 3) / st + 1, (W(x) + 2 - 3) / st + 1, blk.conv1.cout, out_cs);
            basic_block(x, blk, &o);
        } else {
            basic_block(x, blk);
        }
        dry_ = false;
    }

    // ---- Plan.schedule_segments: idh_schedule_ops over the regions recorded per op (ops [0, n_first) and the rest are levelled and ordered each
    // on their own - the volume kernel runs between them)
    int schedule(int n_first, std::vector<int32_t> &order) {
        std::vector<Region> flat;
        std::vector<int32_t> offs{0};
        for (const Meta &m : meta)
            for (const std::vector<Region> *rs : {&m.reads, &m.writes}) {
                flat.insert(flat.end(), rs->begin(), rs->end());
                offs.push_back((int32_t)flat.size());
            }
        flat.push_back(Region{});  // (a non-NULL array for a plan whose ops touch nothing)
        order.assign(ops.size() + 1, 0);  // (+ 1: non-NULL for an empty plan)
        return idh_schedule_ops(ops.data(), (int)ops.size(), n_first, &flat[0].buf, offs.data(), IDH_SCHED_MERGE_LEVELS | IDH_SCHED_WINO_GROUP, order.data(), nullptr);
    }

    int finish(idh_net_sizes *sizes, int n_first = 0) {
        std::vector<int32_t> order;
        if (err || (err = schedule(n_first, order)) != IDH_OK) return err;
        if (g_observer) g_observer(ops.data(), (int)ops.size(), n_first, order.data(), ws_, ws_off, blob_, blob_off, g_observer_user);
        if (sizes) {
            sizes->workspace_floats = ws_off;
            sizes->weight_floats = blob_off;
            sizes->ops = (int)ops.size();
            sizes->launches = idh_count_launches(ops.data(), (int)ops.size());
            sizes->wino4 = n_wino4; sizes->wino2 = n_wino2; sizes->recycled = recycled;
            if (sizes->launches < 0) return sizes->launches;
        }
        if (mode_ == MODE_RUN) {
            if (ws_off > ws_cap_) return IDH_EWORKSPACE;
            // padding channels first: nothing an op or before_run writes may be cleared afterwards
            for (const Buf &b : bufs)
                if (b.internal && b.zero_fill && hipMemsetAsync(b.base, 0, b.floats * sizeof(float), st_) != hipSuccess) return IDH_ELAUNCH;
            int rc = n_first ? idh_run_ops(ops.data(), n_first, st_) : IDH_OK;
            if (rc == IDH_OK && before_run) rc = before_run(before_ctx);
            return rc != IDH_OK ? rc : idh_run_ops(ops.data() + n_first, (int)ops.size() - n_first, st_);
        }
        return IDH_OK;
    }

    Mode mode() const { return mode_; }
    hipStream_t stream() const { return st_; }
    int (*before_run)(void *) = nullptr;  // MODE_RUN: called after scheduling, before the pass is enqueued (the whole-model entry's volume)
    void *before_ctx = nullptr;

  private:
    Mode mode_;
    float *ws_;
    size_t ws_cap_;
    float *blob_;
    hipStream_t st_;
    bool dry_ = false;  // reserve_block
    size_t n_fake_ = 0;  // fake_tensor
    std::map<std::tuple<int, int, int, int>, std::vector<int>> free_;
};

// `read`: the tensor is read by a conv (whole 16-channel blocks: an odd channel count must be a zero-padded buffer of its own); a tensor that is
// only written may be any 16-byte-aligned channel slice
bool tensor_ok(const idh_tensor *t, bool need_ptr, bool read = true) {
    if (!t || t->C <= 0 || t->H <= 0 || t->W <= 0) return false;
    if (t->layout != IDH_LAYOUT_NHWC && t->layout != IDH_LAYOUT_NCHW) return false;
    if (t->layout == IDH_LAYOUT_NHWC && (t->cs < t->C || (t->cs & 3) || (read && (t->C & 15) && t->cs != ceil16(t->C)))) return false;
    if (need_ptr && (!t->ptr || ((uintptr_t)t->ptr & 15))) return false;
    return true;
}

// an input tensor as a view of the plan: NHWC in place, NCHW through a layout import into a plan buffer
View input_view(Plan &p, const idh_tensor &t, int N) {
    if (t.layout == IDH_LAYOUT_NHWC) return p.external(t, N);
    const View v = p.buffer(N, t.H, t.W, t.C);
    p.import_nchw(t.ptr, N, t.C, t.H, t.W, v);
    return v;
}
// where a block that produces output tensor `t` should write: the caller's NHWC memory, or a plan buffer that is exported afterwards
View output_view(Plan &p, const idh_tensor &t, int N) {
    if (t.layout == IDH_LAYOUT_NHWC) return p.external(t, N);
    return p.buffer(N, t.H, t.W, t.C);
}
void output_done(Plan &p, const idh_tensor &t, const View &v) {
    if (t.layout == IDH_LAYOUT_NCHW) p.export_nchw(v, t.ptr);
}

// ---- the three networks ---------------------------------------------------------------------------------------------------------------------
int build_basic_block(Plan &p, const idh_block_params *blk, int N, const idh_tensor *x, const idh_tensor *out) {
    const bool run = p.mode() == MODE_RUN;
    if (!blk || N <= 0 || !tensor_ok(x, run) || !tensor_ok(out, run, false) || x->C != blk->conv1.cin || out->C != blk->conv1.cout) return IDH_EINVAL;
    const View xin = input_view(p, *x, N);
    const View o = output_view(p, *out, N);
    p.basic_block(xin, *blk, &o);
    output_done(p, *out, o);
    return p.err;
}

// nhwc.build_matching_stem: stem pass, then layer1 = 2 x (conv1 + ReLU, conv2 + identity + ReLU), BatchNorms folded into the blob by *_pack
int build_matching_stem(Plan &p, const idh_stem_params *sp, int N, const idh_tensor *img, const idh_tensor *out) {
    const bool run = p.mode() == MODE_RUN;
    if (!sp || N <= 0 || !img || img->layout != IDH_LAYOUT_NCHW || img->C != 3 || img->H < 8 || img->W < 8 || (run && !img->ptr)) return IDH_EINVAL;
    const int Ho = ((img->H + 1) / 2) / 2, Wo = ((img->W + 1) / 2) / 2;
    if ((long long)N * 3 * img->H * img->W >= (1ll << 31) || !tensor_ok(out, run, false) || out->C != 64 || out->H != Ho || out->W != Wo)
        return (long long)N * 3 * img->H * img->W >= (1ll << 31) ? IDH_EUNSUPPORTED : IDH_EINVAL;
    // blob: [stem weights][4 x (folded OIHW 64x64x3x3, folded bias 64)][what the four convs pack from them]
    float *stem_w = p.blob_alloc(idh_stem_weight_floats());
    idh_conv_params convs[4];
    for (int i = 0; i < 4; ++i) {
        float *fw = p.blob_alloc(64 * 64 * 9), *fb = p.blob_alloc(64);
        convs[i] = idh_conv_params{fw, fb, 64, 64, 3, 1};
    }
    if (p.mode() == MODE_PACK) {
        auto bn_ok = [](const idh_bn_params &b) { return b.weight && b.bias && b.running_mean && b.running_var && b.eps >= 0.f; };
        if (!sp->conv1_weight || !bn_ok(sp->bn1)) return IDH_EINVAL;
        for (int i = 0; i < 4; ++i)
            if (!sp->layer1_conv[i] || !bn_ok(sp->layer1_bn[i])) return IDH_EINVAL;
        int rc = idh_pack_stem_weight(sp->conv1_weight, sp->bn1.weight, sp->bn1.bias, sp->bn1.running_mean, sp->bn1.running_var, sp->bn1.eps, stem_w,
                                      p.stream());
        for (int i = 0; i < 4 && rc == IDH_OK; ++i) {
            const idh_bn_params &b = sp->layer1_bn[i];
            rc = idh_fold_conv_bn(sp->layer1_conv[i], 64, 64 * 9, b.weight, b.bias, b.running_mean, b.running_var, b.eps, const_cast<float *>(convs[i].weight),
                                  const_cast<float *>(convs[i].bias), p.stream());
        }
        if (rc != IDH_OK) return rc;
    }
    View x = p.buffer(N, Ho, Wo, 64);
    p.stem(img->ptr, N, img->H, img->W, stem_w, x);
    for (int b = 0; b < 2; ++b) {
        const View h = p.buffer(N, Ho, Wo, 64);
        p.conv(x, convs[2 * b], h, IDH_ACT_LRELU, 0.f, nullptr, nullptr, nullptr, IDH_PAD_ZEROS, nullptr, true);
        const View y = b == 1 ? output_view(p, *out, N) : p.buffer(N, Ho, Wo, 64);
        p.conv(h, convs[2 * b + 1], y, IDH_ACT_LRELU, 0.f, &x, nullptr, nullptr, IDH_PAD_ZEROS, nullptr, true);
        p.release(h);
        if (b == 0) p.release(x);
        x = y;
    }
    output_done(p, *out, x);
    return p.err;
}

// CVEncoder.forward (networks.py:208-215): x = ds_conv_i(x); x = cat([x, img_feats[i]]); x = conv_i(x)
// outs == NULL: level i's output stays a plan buffer (levels[i]), as in one HotPath plan
int cvencoder_body(Plan &p, const idh_block_params *blocks, int num_blocks, int N, View x, const idh_tensor *img, const idh_tensor *outs,
                   std::vector<View> *levels) {
    const bool run = p.mode() == MODE_RUN;
    for (int i = 0; i < num_blocks; ++i) {
        const idh_block_params &ds = blocks[3 * i], &c0 = blocks[3 * i + 1], &c1 = blocks[3 * i + 2];
        if (!tensor_ok(&img[i], run) || (outs && !tensor_ok(&outs[i], run))) return IDH_EINVAL;
        const int st = ds.conv1.stride;
        if (st != 1 && st != 2) return IDH_EINVAL;
        const int Ho = (p.H(x) + 2 - 3) / st + 1, Wo = (p.W(x) + 2 - 3) / st + 1;
        const int cout = ds.conv1.cout, cimg = img[i].C;
        if (img[i].H != Ho || img[i].W != Wo || c0.conv1.cin != cout + cimg) return IDH_EINVAL;
        if (outs && (outs[i].C != c1.conv1.cout || outs[i].H != Ho || outs[i].W != Wo)) return IDH_EINVAL;
        const View cat = p.buffer(N, Ho, Wo, cout + cimg);
        const View left = Plan::slice(cat, 0, cout);
        p.basic_block(x, ds, &left);
        const View right = Plan::slice(cat, cout, cimg);
        if (img[i].layout == IDH_LAYOUT_NCHW) p.import_nchw(img[i].ptr, N, cimg, Ho, Wo, right);
        else return IDH_EUNSUPPORTED;  // (an NHWC image-feature map would need a copy op into the concat slice: the reference hands NCHW)
        View y = p.basic_block(cat, c0);
        if (outs) {
            const View o = output_view(p, outs[i], N);
            y = p.basic_block(y, c1, &o);
            output_done(p, outs[i], y);
        } else {
            y = p.basic_block(y, c1);
        }
        if (levels) levels->push_back(y);
        x = y;
        if (p.err) return p.err;
    }
    return p.err;
}

int build_cvencoder(Plan &p, const idh_block_params *blocks, int num_blocks, int N, const idh_tensor *cost, const idh_tensor *img, const idh_tensor *outs) {
    const bool run = p.mode() == MODE_RUN;
    if (!blocks || num_blocks <= 0 || num_blocks > 8 || N <= 0 || !tensor_ok(cost, run) || !img || !outs) return IDH_EINVAL;
    return cvencoder_body(p, blocks, num_blocks, N, input_view(p, *cost, N), img, outs, nullptr);
}

// BDDecoderPP / DepthDecoderPP.forward (networks.py:64-84, 163-183) over the five input views; *feat0 (optional): the top-left result
// scales (nhwc.build_decoder): bit i = the caller reads the output_i result.  A scale without its bit gets no output_i block - the grid node
// X(i, 4-i) under it is built either way, the next column reads it.  keep_slots: such a block still takes its blob slots (reserve_block), so
// that the blob layout, weight_floats and a packed blob do not depend on the mask.
int unetpp_body(Plan &p, const idh_block_params *blocks, const idh_conv_params *heads, int N, std::vector<View> prev, const idh_tensor *fouts,
                float *const *log_depth, float *const *depth, View *feat0, unsigned scales = IDH_SCALES_ALL, bool keep_slots = false) {
    const bool run = p.mode() == MODE_RUN;
    if ((scales & ~(unsigned)IDH_SCALES_ALL) || (heads && scales != IDH_SCALES_ALL)) return IDH_EINVAL;  // (the 1x1 heads are outputs at every scale)
    const idh_block_params *out_blk[4] = {nullptr, &blocks[46], &blocks[47], &blocks[48]};
    auto sel = [&](int i) { return ((scales >> i) & 1u) != 0; };
    auto given = [&](int i) { return fouts && fouts[i].C > 0; };  // (C == 0 skips a level; decided by the shape alone so that sizes / pack / fwd agree)
    auto want = [&](int i) { return given(i) && sel(i); };
    std::vector<View> outputs;
    View final_v[4];
    int bi = 0;
    for (int j = 1; j <= 4; ++j) {
        for (int i = 4 - j; i >= 0; --i) {
            const idh_block_params &right = blocks[bi++], &diag = blocks[bi++];
            const bool has_up = (i + j) != 4;
            const idh_block_params *up = has_up ? &blocks[bi++] : nullptr;
            const idh_block_params &in0 = blocks[bi++], &in1 = blocks[bi++];
            const int cout = right.conv1.cout;
            const View xi = prev[i];
            const View cat = p.buffer(N, p.H(xi), p.W(xi), cout * (has_up ? 3 : 2));
            const View s0 = Plan::slice(cat, 0, cout);
            p.basic_block(xi, right, &s0);
            const View lo = p.basic_block(prev[i + 1], diag);
            if (p.H(lo) * 2 != p.H(xi) || p.W(lo) * 2 != p.W(xi)) return IDH_EINVAL;
            // (liveness reuse) prev[i + 1] is X(i+1, 4-(i+1)), the last node of its row: up_conv and the output head read it in the column
            // before, this diag_conv was its last reader
            if (j > 1 && !has_up) p.release(prev[i + 1]);
            p.upsample2(lo, Plan::slice(cat, cout, cout));
            p.release(lo);  // (liveness reuse: the half-resolution map has no reader after its upsampling)
            if (has_up) {
                const View lo2 = p.basic_block(outputs.back(), *up);
                p.upsample2(lo2, Plan::slice(cat, 2 * cout, cout));
                p.release(lo2);
            }
            const View y0 = p.basic_block(cat, in0);
            p.release(cat);
            // the decoder's top-left result IS feature_s0 (output_0[0] = nn.Identity, networks.py:61): written straight into the caller's tensor
            const bool last = j == 4 - i;
            View y;
            if (last && i == 0 && want(0) && fouts[0].layout == IDH_LAYOUT_NHWC) {
                if (!tensor_ok(&fouts[0], run) || fouts[0].C != in1.conv1.cout) return IDH_EINVAL;
                const View o = p.external(fouts[0], N);
                y = p.basic_block(y0, in1, &o);
            } else {
                y = p.basic_block(y0, in1);
                if (last && i == 0 && want(0)) {
                    if (!tensor_ok(&fouts[0], run) || fouts[0].C != in1.conv1.cout) return IDH_EINVAL;
                    p.export_nchw(y, fouts[0].ptr);
                }
            }
            p.release(y0);
            outputs.push_back(y);
            if (last) {  // the only (i, j) whose output_i result survives in the reference's dict
                if (i == 0) final_v[0] = y;
                else if (!sel(i)) {
                    if (keep_slots && given(i)) p.reserve_block(y, *out_blk[i], fouts[i].layout == IDH_LAYOUT_NHWC ? fouts[i].cs : 0);
                } else if (want(i)) {
                    if (!tensor_ok(&fouts[i], run) || fouts[i].C != out_blk[i]->conv1.cout) return IDH_EINVAL;
                    const View o = output_view(p, fouts[i], N);
                    final_v[i] = p.basic_block(y, *out_blk[i], &o);
                    output_done(p, fouts[i], final_v[i]);
                } else if (heads) {
                    final_v[i] = p.basic_block(y, *out_blk[i]);
                }
            }
            if (p.err) return p.err;
        }
        prev.assign(outputs.rbegin(), outputs.rend());
    }
    if (heads) {
        for (int i = 0; i < 4; ++i) {
            if (run && (!log_depth || !log_depth[i])) return IDH_EINVAL;
            p.head(final_v[i], heads[i], run ? log_depth[i] : nullptr, (run && depth) ? depth[i] : nullptr);
        }
    }
    if (feat0) *feat0 = final_v[0];
    return p.err;
}

int build_unetpp(Plan &p, const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, int N, const idh_tensor *feats,
                 const idh_tensor *fouts, float *const *log_depth, float *const *depth, unsigned scales = IDH_SCALES_ALL) {
    const bool run = p.mode() == MODE_RUN;
    if (!blocks || n_blocks != IDH_UNETPP_BLOCKS || N <= 0 || !feats) return IDH_EINVAL;
    std::vector<View> prev;
    for (int i = 0; i < 5; ++i) {
        if (!tensor_ok(&feats[i], run)) return IDH_EINVAL;
        if (i && (feats[i].H * 2 != feats[i - 1].H || feats[i].W * 2 != feats[i - 1].W)) return IDH_EINVAL;  // pyramid levels differ by exactly x2
        prev.push_back(input_view(p, feats[i], N));
    }
    return unetpp_body(p, blocks, heads, N, prev, fouts, log_depth, depth, nullptr, scales, true);
}

// FNV-1a over what decides a pass's arithmetic and memory layout: each op's kind, shapes and kernel choice
uint64_t layout_hash(const std::vector<idh_op> &ops) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](long long v) {
        for (int i = 0; i < 8; ++i) { h ^= (uint64_t)((v >> (8 * i)) & 0xff); h *= 1099511628211ull; }
    };
    for (const idh_op &op : ops) {
        mix(op.kind); mix(op.N); mix(op.Ho); mix(op.Wo); mix(op.Cout); mix(op.tile_m); mix(op.tile_n); mix(op.split_k); mix(op.act); mix(op.group);
        for (const idh_conv_src &s : op.src) { mix(s.Cin); mix(s.H); mix(s.W); mix(s.cs); mix(s.ks); mix(s.stride); mix(s.pad_mode); mix(s.norm != nullptr); }
    }
    return h;
}

// Every extern "C" network entry below: the pointer checks of its mode, the Plan, the network's builder, then the schedule and (MODE_RUN) the
// pass.  sizes: MODE_SIZES only.  null_ws_ok: MODE_RUN accepts ws == NULL when ws_floats == 0 (a BasicBlock may need no workspace).
// build(p): the builder's return code; whatever it checks comes after every pointer check and before finish.
template <class Build>
int net_entry(Mode mode, const float *blob, float *ws, size_t ws_floats, void *stream, idh_net_sizes *sizes, bool null_ws_ok, Build build) {
    if (mode == MODE_SIZES && !sizes) return IDH_EINVAL;
    if (mode != MODE_SIZES && (!blob || ((uintptr_t)blob & 255))) return IDH_EINVAL;
    if (mode == MODE_RUN && !(null_ws_ok && !ws_floats) && (!ws || ((uintptr_t)ws & 255))) return IDH_EINVAL;
    Plan p(mode, ws, ws_floats, const_cast<float *>(blob), idh_stream(stream));
    const int rc = build(p);
    if (rc != IDH_OK) return rc;
    return mode == MODE_PACK ? p.err : p.finish(sizes);
}

}  // namespace

// The conv stage of one HotPath plan (pipeline.py HotPath._plan): the volume buffer, the layout import of pyramid level 0, the CVEncoder
// (importing levels 1..4 into its concat slices) and the UNet++ decoder over [level 0 | CVEncoder outputs], all in one op list.
int idh_internal::conv_stage(int mode, ConvStage *s, float *ws, size_t ws_cap, float *blob, hipStream_t st, int (*before_ops)(void *), void *ctx) {
    const Mode m = mode == STAGE_SIZES ? MODE_SIZES : mode == STAGE_PACK ? MODE_PACK : MODE_RUN;
    if (!s || !s->enc || s->n_enc != 4 || !s->dec || s->N <= 0 || s->H <= 0 || s->W <= 0 || s->D <= 0) return IDH_EINVAL;
    Plan p(m, ws, ws_cap, blob, st);
    s->match = nullptr;
    s->n_head_ops = 0;
    if (s->head_mode) {
        // nhwc.build_matching_head over all N (K+1) images at once (HotPath._plan): 1x1 conv, InstanceNorm + LeakyReLU, 3x3 conv (replicate
        // padding), InstanceNorm; output = ONE (N, K+1, H, W, C) buffer the volume kernel addresses with batch strides
        if (!s->head || s->K <= 0 || (s->head_mode != 1 && s->head_mode != 2)) return IDH_EINVAL;
        const idh_conv_params &c1 = s->head[0], &c2 = s->head[1];
        const int M = s->N * (s->K + 1), H = s->H, W = s->W;
        if (c1.ks != 1 || c1.stride != 1 || c2.ks != 3 || c2.stride != 1 || c2.cin != c1.cout) return IDH_EINVAL;
        if (m == MODE_RUN && (!s->layer1 || ((uintptr_t)s->layer1 & 15))) return IDH_EINVAL;
        const View h = p.buffer(M, H, W, c1.cout);
        if (s->head_mode == 1 && kFuseHeadImport && Plan::pointwise_nchw_eligible(c1)) {
            p.pointwise_nchw(s->layer1, M, c1.cin, H, W, c1, h);  // the 1x1 conv reads the NCHW map in place
        } else {
            View x;
            if (s->head_mode == 1) {
                x = p.buffer(M, H, W, c1.cin);
                p.import_nchw(s->layer1, M, c1.cin, H, W, x);
            } else {  // channels-last producer: the conv reads the caller's tensor in place
                const idh_tensor t{const_cast<float *>(s->layer1), IDH_LAYOUT_NHWC, c1.cin, H, W, c1.cin};
                if (!tensor_ok(&t, m == MODE_RUN)) return IDH_EINVAL;
                x = p.external(t, M);
            }
            p.conv(x, c1, h, IDH_ACT_NONE, 0.2f, nullptr, nullptr, nullptr);
        }
        const View y = p.buffer(M, H, W, c2.cout);
        idh_conv_choice hc;  // (nhwc.norm_on_load_eligible: the LDS-staged 3x3 kernel with 16-channel tiles, whole 16-channel input blocks)
        if (p.select({{h, &c2}}, y, IDH_ACT_NONE, 0.2f, nullptr, IDH_PAD_REPLICATE, false, false, &hc) != IDH_OK) return IDH_EINVAL;
        if (kFuseHeadNorm && h.C % 16 == 0 && hc.lds_subtiles == 1 && (hc.families & IDH_FAMILY_LDS)) {
            const Norm nm = p.instance_norm(h, nullptr, IDH_ACT_NONE, 0.2f);
            Norm on = nm;
            on.act = IDH_ACT_LRELU; on.slope = 0.2f;
            p.conv(h, c2, y, IDH_ACT_NONE, 0.2f, nullptr, nullptr, nullptr, IDH_PAD_REPLICATE, &on);
        } else {
            const View hn = p.buffer(M, H, W, c1.cout);
            p.instance_norm(h, &hn, IDH_ACT_LRELU, 0.2f);
            p.conv(hn, c2, y, IDH_ACT_NONE, 0.2f, nullptr, nullptr, nullptr, IDH_PAD_REPLICATE);
        }
        const View mo = p.buffer(M, H, W, c2.cout);
        p.instance_norm(y, &mo, IDH_ACT_NONE, 0.2f);
        if (p.err) return p.err;
        if (p.cs(mo) != mo.C) return IDH_EUNSUPPORTED;  // (the volume kernels read dense (N, K+1, H, W, C) features)
        s->match = p.ptr(mo);
        s->n_head_ops = (int)p.ops.size();
    }
    const View cv_in = p.buffer(s->N, s->H, s->W, s->D);
    for (int i = 0; i < 5; ++i)
        if (s->img[i].layout != IDH_LAYOUT_NCHW || !tensor_ok(&s->img[i], m == MODE_RUN)) return IDH_EINVAL;
    const View v0 = input_view(p, s->img[0], s->N);
    std::vector<View> levels{v0};
    int rc = cvencoder_body(p, s->enc, s->n_enc, s->N, cv_in, &s->img[1], nullptr, &levels);
    if (rc != IDH_OK) return rc;
    for (int i = 1; i < 5; ++i)
        if (p.H(levels[i]) * 2 != p.H(levels[i - 1]) || p.W(levels[i]) * 2 != p.W(levels[i - 1])) return IDH_EINVAL;
    View f0;
    rc = unetpp_body(p, s->dec, s->heads, s->N, levels, nullptr, s->log_depth, s->depth, &f0, s->scales);
    if (rc != IDH_OK) return rc;
    s->cv_in = p.ptr(cv_in);
    s->cv_cs = p.cs(cv_in);
    s->feat0 = p.ptr(f0);
    s->feat0_cs = p.cs(f0); s->feat0_C = f0.C; s->feat0_H = p.H(f0); s->feat0_W = p.W(f0);
    for (int i = 0; i < 5; ++i) { s->level_H[i] = p.H(levels[i]); s->level_W[i] = p.W(levels[i]); }
    p.before_run = before_ops;
    p.before_ctx = ctx;
    idh_net_sizes sz{};
    if (m == MODE_PACK) return p.err;
    rc = p.finish(m == MODE_SIZES ? &sz : nullptr, s->n_head_ops);
    if (rc != IDH_OK) return rc;
    if (m == MODE_SIZES) {
        s->ws_floats = sz.workspace_floats; s->weight_floats = sz.weight_floats; s->ops = sz.ops; s->launches = sz.launches;
        s->layout_hash = layout_hash(p.ops);
    }
    return IDH_OK;
}

extern "C" void idh_debug_set_plan_observer(idh_plan_observer fn, void *user) {
    g_observer = fn;
    g_observer_user = user;
}

extern "C" int idh_basic_block_sizes(const idh_block_params *blk, int N, const idh_tensor *x, const idh_tensor *out, idh_net_sizes *sizes) {
    return net_entry(MODE_SIZES, nullptr, nullptr, 0, nullptr, sizes, false, [&](Plan &p) { return build_basic_block(p, blk, N, x, out); });
}
extern "C" int idh_basic_block_pack(const idh_block_params *blk, int N, const idh_tensor *x, const idh_tensor *out, float *blob, void *stream) {
    return net_entry(MODE_PACK, blob, nullptr, 0, stream, nullptr, false, [&](Plan &p) { return build_basic_block(p, blk, N, x, out); });
}
extern "C" int idh_basic_block_fwd(const idh_block_params *blk, const float *blob, int N, const idh_tensor *x, const idh_tensor *out, float *ws,
                                   size_t ws_floats, void *stream) {
    return net_entry(MODE_RUN, blob, ws, ws_floats, stream, nullptr, true, [&](Plan &p) { return build_basic_block(p, blk, N, x, out); });
}

extern "C" int idh_cvencoder_sizes(const idh_block_params *blocks, int num_blocks, int N, const idh_tensor *cost, const idh_tensor *img_feats,
                                   const idh_tensor *outs, idh_net_sizes *sizes) {
    return net_entry(MODE_SIZES, nullptr, nullptr, 0, nullptr, sizes, false,
                     [&](Plan &p) { return build_cvencoder(p, blocks, num_blocks, N, cost, img_feats, outs); });
}
extern "C" int idh_cvencoder_pack(const idh_block_params *blocks, int num_blocks, int N, const idh_tensor *cost, const idh_tensor *img_feats,
                                  const idh_tensor *outs, float *blob, void *stream) {
    return net_entry(MODE_PACK, blob, nullptr, 0, stream, nullptr, false,
                     [&](Plan &p) { return build_cvencoder(p, blocks, num_blocks, N, cost, img_feats, outs); });
}
extern "C" int idh_cvencoder_fwd(const idh_block_params *blocks, int num_blocks, const float *blob, int N, const idh_tensor *cost,
                                 const idh_tensor *img_feats, const idh_tensor *outs, float *ws, size_t ws_floats, void *stream) {
    return net_entry(MODE_RUN, blob, ws, ws_floats, stream, nullptr, false,
                     [&](Plan &p) { return build_cvencoder(p, blocks, num_blocks, N, cost, img_feats, outs); });
}

extern "C" int idh_unetpp_sizes(const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, int N, const idh_tensor *feats,
                                const idh_tensor *feature_outs, idh_net_sizes *sizes) {
    return net_entry(MODE_SIZES, nullptr, nullptr, 0, nullptr, sizes, false,
                     [&](Plan &p) { return build_unetpp(p, blocks, n_blocks, heads, N, feats, feature_outs, nullptr, nullptr); });
}
extern "C" int idh_unetpp_pack(const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, int N, const idh_tensor *feats,
                               const idh_tensor *feature_outs, float *blob, void *stream) {
    return net_entry(MODE_PACK, blob, nullptr, 0, stream, nullptr, false,
                     [&](Plan &p) { return build_unetpp(p, blocks, n_blocks, heads, N, feats, feature_outs, nullptr, nullptr); });
}
extern "C" int idh_unetpp_fwd(const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, const float *blob, int N,
                              const idh_tensor *feats, const idh_tensor *feature_outs, float *const *log_depth_outs, float *const *depth_outs,
                              float *ws, size_t ws_floats, void *stream) {
    return net_entry(MODE_RUN, blob, ws, ws_floats, stream, nullptr, false,
                     [&](Plan &p) { return build_unetpp(p, blocks, n_blocks, heads, N, feats, feature_outs, log_depth_outs, depth_outs); });
}

extern "C" int idh_unetpp_sizes_ex(const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, int N, const idh_tensor *feats,
                                   const idh_tensor *feature_outs, uint32_t scales, idh_net_sizes *sizes) {
    return net_entry(MODE_SIZES, nullptr, nullptr, 0, nullptr, sizes, false,
                     [&](Plan &p) { return build_unetpp(p, blocks, n_blocks, heads, N, feats, feature_outs, nullptr, nullptr, scales); });
}
extern "C" int idh_unetpp_pack_ex(const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, int N, const idh_tensor *feats,
                                  const idh_tensor *feature_outs, uint32_t scales, float *blob, void *stream) {
    return net_entry(MODE_PACK, blob, nullptr, 0, stream, nullptr, false,
                     [&](Plan &p) { return build_unetpp(p, blocks, n_blocks, heads, N, feats, feature_outs, nullptr, nullptr, scales); });
}
extern "C" int idh_unetpp_fwd_ex(const idh_block_params *blocks, int n_blocks, const idh_conv_params *heads, const float *blob, size_t weight_floats,
                                 int N, const idh_tensor *feats, const idh_tensor *feature_outs, uint32_t scales, float *const *log_depth_outs,
                                 float *const *depth_outs, float *ws, size_t ws_floats, void *stream) {
    return net_entry(MODE_RUN, blob, ws, ws_floats, stream, nullptr, false, [&](Plan &p) {
        const int rc = build_unetpp(p, blocks, n_blocks, heads, N, feats, feature_outs, log_depth_outs, depth_outs, scales);
        if (rc != IDH_OK) return rc;
        return weight_floats != p.blob_off ? IDH_EINVAL : IDH_OK;  // a blob sized for another (N, shapes, feature_outs): never read
    });
}

extern "C" int idh_matching_stem_sizes(const idh_stem_params *params, int N, const idh_tensor *images, const idh_tensor *out, idh_net_sizes *sizes) {
    return net_entry(MODE_SIZES, nullptr, nullptr, 0, nullptr, sizes, false, [&](Plan &p) { return build_matching_stem(p, params, N, images, out); });
}
extern "C" int idh_matching_stem_pack(const idh_stem_params *params, int N, const idh_tensor *images, const idh_tensor *out, float *blob, void *stream) {
    return net_entry(MODE_PACK, blob, nullptr, 0, stream, nullptr, false, [&](Plan &p) { return build_matching_stem(p, params, N, images, out); });
}
extern "C" int idh_matching_stem_fwd(const idh_stem_params *params, const float *blob, int N, const idh_tensor *images, const idh_tensor *out, float *ws,
                                     size_t ws_floats, void *stream) {
    return net_entry(MODE_RUN, blob, ws, ws_floats, stream, nullptr, false, [&](Plan &p) { return build_matching_stem(p, params, N, images, out); });
}

