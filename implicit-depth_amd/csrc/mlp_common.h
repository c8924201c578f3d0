// What the occlusion-MLP kernels share (csrc/mlp.hip: one pixel per column; csrc/mlp_rays.hip: one ray per column): the hidden width,
// nn.ELU and the 128 -> 128 layer on register-resident activations.  The layout is described at the top of csrc/mlp.hip.
#pragma once
#include "idh_common.h"
#include "split_f16.h"

namespace idh_mlp {

using idh_f16::f32x4;

constexpr int kHidden = 128;           // mlp_size (networks.py:88)
constexpr int kNS = kHidden / 16;      // 8 sub-tiles of 16 hidden units

// nn.ELU(alpha = 1): x > 0 ? x : exp(x) - 1, formed exactly as torch's kernel forms it (exp, then subtract), with the
// exponential through v_exp_f32 (1 ulp; exp(x) = exp2(x * log2 e): relative error < 1e-6 for the |x| < 10 that occur)
// instead of ocml's expm1f (~25 VALU per activation against 5 here).  fp32 MFMA and VALU serialise on a SIMD (DESIGN
// 4.3), and the 64 activations per pixel and plane were ~1000 vector instructions against 256 MFMAs: 4.63 -> 4.23 ms
// with a polynomial near 0, -> this form.
__device__ __forceinline__ float elu1(float x) {
#ifdef IDH_ELU_OCML
    return x > 0.f ? x : expm1f(x);
#else
    return x > 0.f ? x : __expf(x) - 1.0f;
#endif
}
// One 128 -> 128 layer on register-resident activations (transposed form), TM pixel sub-tiles.
//   hin[c][t]  : B operands, c = k-block (8), t = pixel sub-tile
//   wfrag      : packed weights [c][i][lane][4]   (i = output sub-tile)
//   acc[i][t]  : results in C/D layout (= next layer's B operands)
template <int TM>
__device__ __forceinline__ void dense128(const f32x4 (&hin)[kNS][TM], const f32x4 *wfrag, int lane,
                                         f32x4 (&acc)[kNS][TM]) {
#pragma unroll
    for (int c = 0; c < kNS; ++c) {
#pragma unroll
        for (int i = 0; i < kNS; ++i) {
            const f32x4 A = wfrag[(c * kNS + i) * 64 + lane];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int t = 0; t < TM; ++t)
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[kk], hin[c][t][kk], acc[i][t], 0, 0, 0);
        }
        // keep the scheduler from hoisting all 64 weight-fragment loads (256 VGPRs) to the top
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace idh_mlp
