// Keyframe feature bank (include/idh_bank.h): a ring of N slots on the device, each one frame's channels-last matching features plus its
// world_T_cam, cam_T_world and K_s1.  commit stores a frame; gather writes, for K slots per batch entry, the inputs of the volume kernels:
// the (B,K,H,W,C) source features, src_K and the two relative poses of bd_model.py:200-204.
//
// Both kernels are copies at 16 bytes a lane.  A view is contiguous in the bank and in the output, so lane l of a wave moves float4 l of a
// 1 KiB run: with C = 16 a pixel is one 64-byte line and a wave moves 16 whole pixels, with C = 32 eight.  A workgroup owns TILE float4 of
// ONE view: its slot number comes out of the launch arguments once (a scalar load), so every address in it is a wave-uniform base plus the
// lane's offset.  The last tile of a view is cut at the view's end.  No LDS, no atomics, vector stores only.
#include "idh_common.h"

#include "../../include/idh_bank.h"

namespace {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;                 // float4 in flight per lane: four loads issued before the first store
constexpr int TILE = THREADS * PER_THREAD;    // float4 per workgroup (16 KiB)

// The slot list of one gather, by value in the kernel arguments: one byte per view (slots < 64), four to a word.
struct SlotList {
    uint32_t packed[IDH_BANK_MAX_VIEWS / 4];
};

// dst[i] = src[i] for the float4 i in [tile * TILE, min((tile + 1) * TILE, n4))
__device__ __forceinline__ void copy_tile(const float4 *__restrict__ src, float4 *__restrict__ dst, unsigned tile, unsigned n4) {
    const unsigned i0 = tile * TILE + threadIdx.x;
    if (tile * TILE + TILE <= n4) {  // a whole tile (workgroup-uniform): four loads in flight, then four stores
        static_assert(PER_THREAD == 4, "the loads below are written out");
        const float4 v0 = src[i0], v1 = src[i0 + THREADS], v2 = src[i0 + 2 * THREADS], v3 = src[i0 + 3 * THREADS];
        dst[i0] = v0;
        dst[i0 + THREADS] = v1;
        dst[i0 + 2 * THREADS] = v2;
        dst[i0 + 3 * THREADS] = v3;
    } else {  // the view's last tile, cut at its end
        for (unsigned i = i0; i < n4; i += THREADS) dst[i] = src[i];
    }
}

// element (r, c) of the row-major 4x4 product a @ b: four fp32 products summed in index order (compiled with -ffp-contract=off)
__device__ __forceinline__ float mat44_elem(const float *__restrict__ a, const float *__restrict__ b, int r, int c) {
    float s = a[4 * r] * b[c];
    s += a[4 * r + 1] * b[4 + c];
    s += a[4 * r + 2] * b[8 + c];
    s += a[4 * r + 3] * b[12 + c];
    return s;
}

// grid (tiles of a frame, 1): the frame's features into the slot; workgroup 0 also stores the three matrices
__global__ __launch_bounds__(THREADS) void bank_commit_k(float4 *__restrict__ slot_feats, float *__restrict__ slot_mats,
                                                         const float4 *__restrict__ feat, const float *__restrict__ world_T_cam,
                                                         const float *__restrict__ cam_T_world, const float *__restrict__ K_s1, unsigned n4) {
    if (blockIdx.x == 0 && threadIdx.x < 48) {
        const int m = threadIdx.x >> 4, e = threadIdx.x & 15;
        const float *src = m == 0 ? world_T_cam : (m == 1 ? cam_T_world : K_s1);
        slot_mats[threadIdx.x] = src[e];
    }
    copy_tile(feat, slot_feats, blockIdx.x, n4);
}

// grid (tiles of a view, B * K): view blockIdx.y = b * K + k
__global__ __launch_bounds__(THREADS) void bank_gather_k(const float4 *__restrict__ feats, const float *__restrict__ mats, SlotList slots,
                                                         const float *__restrict__ cur_world_T_cam, const float *__restrict__ cur_cam_T_world,
                                                         float4 *__restrict__ src_out, float *__restrict__ K_out, float *__restrict__ E_out,
                                                         float *__restrict__ poses_out, unsigned K, unsigned n4) {
    const unsigned view = blockIdx.y;
    const unsigned slot = (slots.packed[view >> 2] >> (8 * (view & 3))) & 0xffu;  // once per workgroup, wave-uniform
    if (blockIdx.x == 0 && threadIdx.x < 48) {
        const unsigned b = view / K;
        const float *m = mats + (size_t)slot * 48;  // world_T_cam, cam_T_world, K_s1
        const int which = threadIdx.x >> 4, e = threadIdx.x & 15, r = e >> 2, c = e & 3;
        if (which == 0)
            E_out[(size_t)view * 16 + e] = mat44_elem(m + 16, cur_world_T_cam + (size_t)b * 16, r, c);
        else if (which == 1)
            poses_out[(size_t)view * 16 + e] = mat44_elem(cur_cam_T_world + (size_t)b * 16, m, r, c);
        else
            K_out[(size_t)view * 16 + e] = m[32 + e];
    }
    copy_tile(feats + (size_t)slot * n4, src_out + (size_t)view * n4, blockIdx.x, n4);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// IDH_OK and the float4 count of one frame, or the error of a bank description
int check_bank(const idh_bank *bank, unsigned *n4) {
    if (!bank || bank->struct_size < (int64_t)sizeof(idh_bank)) return IDH_EINVAL;
    if (!bank->feats || !bank->mats || !aligned16(bank->feats)) return IDH_EINVAL;
    if (bank->N < 1 || bank->N > IDH_BANK_MAX_SLOTS || bank->H <= 0 || bank->W <= 0) return IDH_EINVAL;
    if (bank->C != 16 && bank->C != 32) return IDH_EINVAL;
    const long long floats = (long long)bank->H * bank->W * bank->C;
    if (floats >= (1ll << 31)) return IDH_EUNSUPPORTED;
    *n4 = (unsigned)(floats / 4);
    return IDH_OK;
}

}  // namespace

extern "C" size_t idh_sizeof_bank(void) { return sizeof(idh_bank); }

extern "C" int idh_bank_commit_fwd(const idh_bank *bank, int slot, const float *feat_nhwc, const float *world_T_cam, const float *cam_T_world,
                                   const float *K_s1, void *stream) {
    unsigned n4 = 0;
    if (int e = check_bank(bank, &n4)) return e;
    if (!feat_nhwc || !world_T_cam || !cam_T_world || !K_s1 || !aligned16(feat_nhwc)) return IDH_EINVAL;
    if (slot < 0 || slot >= bank->N) return IDH_EINVAL;
    hipLaunchKernelGGL(bank_commit_k, dim3(idh_cdiv(n4, TILE)), dim3(THREADS), 0, idh_stream(stream),
                       reinterpret_cast<float4 *>(bank->feats) + (size_t)slot * n4, bank->mats + (size_t)slot * 48,
                       reinterpret_cast<const float4 *>(feat_nhwc), world_T_cam, cam_T_world, K_s1, n4);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_bank_gather_fwd(const idh_bank *bank, const int32_t *slots, const float *cur_world_T_cam, const float *cur_cam_T_world,
                                   float *src_nhwc_out, float *src_K_out, float *src_E_out, float *src_poses_out, int B, int K, void *stream) {
    unsigned n4 = 0;
    if (int e = check_bank(bank, &n4)) return e;
    if (B < 0 || K < 0) return IDH_EINVAL;
    if (!slots || !cur_world_T_cam || !cur_cam_T_world || !src_nhwc_out || !src_K_out || !src_E_out || !src_poses_out || !aligned16(src_nhwc_out))
        return IDH_EINVAL;
    const long long views = (long long)B * K;
    if (views > IDH_BANK_MAX_VIEWS) return IDH_EUNSUPPORTED;
    SlotList list = {};
    for (long long v = 0; v < views; ++v) {
        if (slots[v] < 0 || slots[v] >= bank->N) return IDH_EINVAL;
        list.packed[v >> 2] |= (uint32_t)slots[v] << (8 * (v & 3));
    }
    if (views == 0) return IDH_OK;
    hipLaunchKernelGGL(bank_gather_k, dim3(idh_cdiv(n4, TILE), (unsigned)views), dim3(THREADS), 0, idh_stream(stream),
                       reinterpret_cast<const float4 *>(bank->feats), bank->mats, list, cur_world_T_cam, cur_cam_T_world,
                       reinterpret_cast<float4 *>(src_nhwc_out), src_K_out, src_E_out, src_poses_out, (unsigned)K, n4);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
