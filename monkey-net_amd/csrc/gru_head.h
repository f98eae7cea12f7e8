// The output head of modules/prediction_module.py:33-42 for ONE key point: y[0..1] -> mean = tanh, y[2..5] = V (2 x 2, row major)
// -> var = V^T V, and the adjoint of both.  Shared by the head kernels of gru.hip (mnk_gru_head_fwd / _bwd) and the loss-fused
// ones of predict.hip (mnk_gru_head_l1_fwd / _bwd): one expression each, so the forms agree bit for bit.
#pragma once
#include "mnk_common.h"

namespace mnk {

__device__ __forceinline__ void head_mean(const float* __restrict__ v, float& m0, float& m1) {
    m0 = tanhf(v[0]);
    m1 = tanhf(v[1]);
}

// V = [[v2, v3], [v4, v5]], var = V^T V (row major 2 x 2)
__device__ __forceinline__ void head_var(const float* __restrict__ v, float* __restrict__ o) {
    // explicit fused multiply-adds (the form the compiler chose for `a * a + c * c` in gru_head_fwd_kernel): left to the
    // compiler, the contraction depends on the code around it and two kernels round the same product differently -- the loss
    // gradient's sign(gt - var) must see the very bits mnk_gru_head_fwd writes
    const float a = v[2], b = v[3], c = v[4], d = v[5];
    const float ab = fmaf(a, b, c * d);
    o[0] = fmaf(a, a, c * c);
    o[1] = ab;
    o[2] = ab;
    o[3] = fmaf(b, b, d * d);
}

// d(y[0..1]) from d(mean) and the means themselves
__device__ __forceinline__ void head_mean_bwd(float dm0, float dm1, float m0, float m1, float* __restrict__ o) {
    o[0] = dm0 * (1.f - m0 * m0);
    o[1] = dm1 * (1.f - m1 * m1);
}

// d(y[2..5]) = dV = V (G + G^T) from g = d(var) (row major 2 x 2)
__device__ __forceinline__ void head_var_bwd(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ o) {
    const float s00 = 2.f * g[0], s01 = g[1] + g[2], s11 = 2.f * g[3];
    const float a = v[2], b = v[3], c = v[4], d = v[5];
    o[2] = a * s00 + b * s01;
    o[3] = a * s01 + b * s11;
    o[4] = c * s00 + d * s01;
    o[5] = c * s01 + d * s11;
}

}  // namespace mnk
