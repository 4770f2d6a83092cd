// cstr_td_device.h -- the twin TD loss head's arithmetic, stated once (internal, included by cstr_mlp.hip and cstr_iql.hip): the
// float32 block reduction of the single-workgroup loss heads, the TD target and critic differences of ONE row, and the final
// combination of the two batch sums. cstr_td_twin_q_loss_f32 and cstr_iql_loss_f32 promise each other's bits for the critic part and
// keep the promise by calling these. Every TU that includes this is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// 256 threads: 64-lane shuffle tree (offsets 32, 16, ... 1), the four wave sums combine as (s0 + s1) + (s2 + s3)
__device__ __forceinline__ float block_sum_256(float v, float *sm)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    const float r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

// d loss / d q_i = td_q_grad_scale * (q_i - t)
__device__ __forceinline__ float td_q_grad_scale(const float scale, const int batch) { return scale * 2.0f / (float)batch; }

// One row of the twin TD loss: t = rew + (1 - done) * gamma * (min(q1_t, q2_t) - [with_logp] ent_coef * next_logp), d_i = q_i - t.
__device__ __forceinline__ float td_twin_row(const float q1_t, const float q2_t, const bool with_logp, const float ent_coef,
                                             const float next_logp, const float rew, const float done, const float gamma, const float q1,
                                             const float q2, float &d1, float &d2)
{
    float q = fminf(q1_t, q2_t);
    if (with_logp) q = q - ent_coef * next_logp;
    const float t = rew + (1.0f - done) * gamma * q;
    d1 = q1 - t;
    d2 = q2 - t;
    return t;
}

// loss = scale * (mse(q1, t) + mse(q2, t)) from the two block sums of d_i^2
__device__ __forceinline__ float td_twin_loss(const float scale, const float s1, const float s2, const int batch)
{
    return scale * (s1 / (float)batch + s2 / (float)batch);
}

}  // namespace
