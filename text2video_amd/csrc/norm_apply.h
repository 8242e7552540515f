// norm_apply.h -- the norm apply pass, y = [relu](norm(x)) + res1 + res2 (+ the other side of the encoder join), as a device
// function with a store policy: inorm_apply_kernel (elementwise.hip) stores the value, inorm_apply_split_kernel
// (conv_igemm_split.hip) the two bf16 terms of each channel pair.
#pragma once
#include "t2v_internal.h"
#include "transform_common.h"

namespace t2v {

// One side of the encoder join, norm(y) + res per float4 (the arithmetic of an inorm_apply pass with relu 0 and one residual)
__device__ __forceinline__ float4 join_side(const NormJoinSide& s, long im, long n4, int C4, long i, int c4) {
    const float4* mr = reinterpret_cast<const float4*>(s.mean_rstd) + im * 2 * C4;
    const float4 a = mr[2 * c4], b = mr[2 * c4 + 1];
    float4 v = reinterpret_cast<const float4*>(s.y)[im * n4 + i];
    v.x = norm_scale(v.x, a.x, a.y);
    v.y = norm_scale(v.y, a.z, a.w);
    v.z = norm_scale(v.z, b.x, b.y);
    v.w = norm_scale(v.w, b.z, b.w);
    if (s.gamma) {
        const float4 gm = reinterpret_cast<const float4*>(s.gamma)[c4], bt = reinterpret_cast<const float4*>(s.beta)[c4];
        v.x = norm_affine(v.x, gm.x, bt.x);
        v.y = norm_affine(v.y, gm.y, bt.y);
        v.z = norm_affine(v.z, gm.z, bt.z);
        v.w = norm_affine(v.w, gm.w, bt.w);
    }
    const float4 r = reinterpret_cast<const float4*>(s.res)[im * n4 + i];
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    return v;
}

// y = [relu]((x-mean)*rstd*gamma+beta) + res1 + res2 ; float4 over NHWC, C % 4 == 0
// join.y != null: ... + (norm_j(join.y) + join.res), the second sum formed by itself and added last -- the encoder join
// d = (norm_b(yb) + rb) + (norm_a(ya) + ra) in ONE pass: what two apply passes (relu 0, one residual each) and add_kernel
// compute, value by value through the same functions in the same order, without writing and re-reading the two sums
// store(i, v): what becomes of float4 i of the image -- the fp32 kernel stores the value, the split-bf16 one
// (inorm_apply_split_kernel: the input of a T2V_ALGO_DIRECT_BF16X2 layer) the two bf16 terms of each channel pair
template <class Store>
// (x carries no __restrict__ here: the split store writes through it in place; inorm_apply_kernel's own parameter does)
__device__ __forceinline__ void inorm_apply_body(const float4* x, const float4* __restrict__ mean_rstd,
                                                 const float4* __restrict__ gamma, const float4* __restrict__ beta,
                                                 const float4* __restrict__ res1, const float4* __restrict__ res2, long n4, int C4,
                                                 int relu, const NormJoinSide& join, Store&& store) {
    {   // blockIdx.y = image of a batch: maps n4 float4 apart, (mean, rstd) tables 2*C4 float4 apart
        const long im = blockIdx.y;
        x += im * n4;
        mean_rstd += im * 2 * C4;
        if (res1) res1 += im * n4;
        if (res2) res2 += im * n4;
    }
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const int c4 = (int)(i % C4);
        const float4 a = mean_rstd[2 * c4], b = mean_rstd[2 * c4 + 1];  // (m0,r0,m1,r1) (m2,r2,m3,r3)
        float4 v = x[i];
        v.x = norm_scale(v.x, a.x, a.y);
        v.y = norm_scale(v.y, a.z, a.w);
        v.z = norm_scale(v.z, b.x, b.y);
        v.w = norm_scale(v.w, b.z, b.w);
        if (gamma) {
            const float4 gm = gamma[c4], bt = beta[c4];
            v.x = norm_affine(v.x, gm.x, bt.x);
            v.y = norm_affine(v.y, gm.y, bt.y);
            v.z = norm_affine(v.z, gm.z, bt.z);
            v.w = norm_affine(v.w, gm.w, bt.w);
        }
        if (relu == 1) {          // (one uniform branch per float4, the activation a constant inside it)
            v.x = norm_act(v.x, 1);
            v.y = norm_act(v.y, 1);
            v.z = norm_act(v.z, 1);
            v.w = norm_act(v.w, 1);
        } else if (relu == 2) {
            v.x = norm_act(v.x, 2);
            v.y = norm_act(v.y, 2);
            v.z = norm_act(v.z, 2);
            v.w = norm_act(v.w, 2);
        }
        if (res1) {
            const float4 r = res1[i];
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (res2) {
            const float4 r = res2[i];
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (join.y) {
            const float4 r = join_side(join, blockIdx.y, n4, C4, i, c4);
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        store(i, v);
    }
}

}  // namespace t2v
