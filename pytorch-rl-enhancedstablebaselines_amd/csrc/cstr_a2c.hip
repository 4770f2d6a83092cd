// cstr_a2c.hip -- A2C's own arithmetic and its optimiser (reference core/a2c/a2c.py:132-190), f32, gfx950:
//   * everything between evaluate_actions' outputs and loss.backward() (a2c.py:150-171) in ONE launch: advantage normalisation, the
//     diagonal Gaussian's log-prob and entropy, the policy-gradient and value losses, the four scalars and the gradients w.r.t. the
//     action mean, the value and log_std. The structure is ppo_loss_kernel's: every thread sums its rows in f64, a fixed LDS tree per
//     workgroup, the partials are published and the workgroup that draws the last ticket sums them in workgroup order. No float atomics;
//     the grid is a function of the row count alone.
//   * torch.optim.RMSprop (momentum 0, not centred, no weight decay) over one flat arena with clip_grad_norm_ folded in: launch 1 is
//     the sum-of-squares pass of cstr_grad_clip_f32 (same grid, same partials), launch 2 forms the coefficient from the partials as
//     grad_scale_kernel does, scales each gradient in register, writes it back and takes the step. Without clipping: one launch and
//     the gradient is only read.
// NaN: with normalize_advantage the statistics are taken over any batch, one row included, where the unbiased standard deviation is
// 0 / 0 = NaN (torch.std of one element): the policy loss and its gradients are then NaN, as in the reference, which unlike PPO has
// no `len > 1` guard (a2c.py:155-156).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"

namespace {

constexpr int A2C_PARTS = 8;  // policy sum, value sum, -, -, d log_std[0..3]: the stride of cstr_ppo_loss_f32's partials

// a2c.py:150-171
template <int A>
__global__ __launch_bounds__(256) void a2c_loss_kernel(const cstr_a2c_loss_t p, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[A2C_PARTS];
    const int64_t B = p.batch;
    // advantage statistics over the whole buffer: every workgroup computes them itself, in the same order
    const bool norm = p.normalize_advantage != 0;
    float a_mean = 0.0f, a_den = 1.0f;
    if (norm) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < B; i += 256) s += (double)p.adv[i];
        a_mean = (float)(block_sum_f64(s, red) / (double)B);
        double q = 0.0;
        for (int64_t i = threadIdx.x; i < B; i += 256) {
            const float d = p.adv[i] - a_mean;
            q += (double)(d * d);
        }
        a_den = (float)sqrt(block_sum_f64(q, red) / (double)(B - 1)) + 1e-8f;  // unbiased std, a2c.py:156; B == 1: 0 / 0 = NaN
    }
    float sig[A], var[A];
#pragma unroll
    for (int k = 0; k < A; ++k) {
        sig[k] = expf(p.log_std[k]);
        var[k] = sig[k] * sig[k];
    }
    const float inv_b = 1.0f / (float)B;
    double acc[2 + A];
#pragma unroll
    for (int k = 0; k < 2 + A; ++k) acc[k] = 0.0;
    for (int64_t b = blockIdx.x * 256ll + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256ll) {
        float mu[A], act[A];
        load_row<A>(p.mean + b * p.ldm, mu);
        load_row<A>(p.actions + b * A, act);
        const float logp = diag_log_prob<A>(act, mu, sig);
        if (p.log_prob_out) p.log_prob_out[b] = logp;
        const float advn = norm ? (p.adv[b] - a_mean) / a_den : p.adv[b];
        acc[0] += (double)(advn * logp);
        const float g_logp = -(inv_b * advn);  // d(-mean(adv * log_prob)) / d log_prob
        float gm[A];
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float d = act[k] - mu[k];
            gm[k] = g_logp * (d / var[k]);
            acc[2 + k] += (double)(g_logp * ((d * d) / var[k] - 1.0f));
        }
        store_row<A>(p.g_mean + b * A, gm);
        const float v = p.values[b], ret = p.returns[b];
        const float dr = ret - v;
        acc[1] += (double)(dr * dr);
        p.g_value[b] = p.vf_coef * ((2.0f * inv_b) * (v - ret));
    }
#pragma unroll
    for (int k = 0; k < 2 + A; ++k) {
        const double s = block_sum_f64(acc[k], red);
        const int slot = k < 2 ? k : k + 2;
        if (threadIdx.x == 0) publish_f64(ws + WS_PART0 + (int64_t)blockIdx.x * A2C_PARTS + slot, s);
    }
    __threadfence();  // release: the partials are visible chip-wide before this workgroup's ticket is
    if (!last_block_ticket(ws)) return;
    __threadfence();  // acquire: behind the last ticket every workgroup's partials are read from memory
    if (threadIdx.x < A2C_PARTS) {
        double s = 0.0;
        const bool used = threadIdx.x < 2 || (threadIdx.x >= 4 && threadIdx.x < 4 + A);
        if (used)
            for (unsigned j = 0; j < gridDim.x; ++j) s += consume_f64(ws + WS_PART0 + (int64_t)j * A2C_PARTS + threadIdx.x);
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ent = 0.0f;
#pragma unroll
        for (int k = 0; k < A; ++k) ent += HALF_LOG_2PI_E + logf(sig[k]);
        float out[4];
        out[0] = -(float)(tot[0] / (double)B);  // policy_loss
        out[1] = (float)(tot[1] / (double)B);   // value_loss
        out[2] = -ent;                          // entropy_loss = -mean(entropy); the entropy does not depend on the row
        out[3] = (out[0] + p.ent_coef * out[2]) + p.vf_coef * out[1];  // loss
        if (p.scalars_out) {
#pragma unroll
            for (int k = 0; k < 4; ++k) p.scalars_out[k] = out[k];
        }
#pragma unroll
        for (int k = 0; k < A; ++k) p.g_log_std[k] = (float)tot[4 + k] - p.ent_coef;  // d(ent_coef * entropy_loss) / d log_std = -ent_coef
    }
}

// torch.optim.RMSprop's single-tensor step, every operation rounded to f32 in ATen's order (mul_ / addcmul_ / sqrt / add_ / addcdiv_)
__device__ __forceinline__ void rmsprop1(float &w, float &g, float &sq, const float coef, const float alpha, const float oma,
                                         const float eps, const float nlr)
{
    g = g * coef;
    sq = sq * alpha + (oma * g) * g;
    const float avg = sqrtf(sq) + eps;
    w = w + (nlr * g) / avg;
}

// part != NULL: launch 2 of the clipped step (every workgroup sums the partials of launch 1 in the same order); NULL: the plain step
__global__ __launch_bounds__(512) void rmsprop_kernel(float *__restrict__ param, float *__restrict__ grad, float *__restrict__ square_avg,
                                                      const double *__restrict__ lr, const float alpha, const float oma, const float eps,
                                                      const double *__restrict__ part, const int n_part, const float max_norm,
                                                      float *__restrict__ norm_out, const int64_t n)
{
    float coef = 1.0f;
    if (part) {
        float norm;
        coef = grad_clip_coef(part, n_part, max_norm, norm);
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    }
    const float nlr = (float)(-lr[0]);
    const int64_t nv = n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(param), *g4 = reinterpret_cast<float4 *>(grad), *s4 = reinterpret_cast<float4 *>(square_avg);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < nv; i += stride) {
        float4 w = p4[i], g = g4[i], s = s4[i];
        rmsprop1(w.x, g.x, s.x, coef, alpha, oma, eps, nlr);
        rmsprop1(w.y, g.y, s.y, coef, alpha, oma, eps, nlr);
        rmsprop1(w.z, g.z, s.z, coef, alpha, oma, eps, nlr);
        rmsprop1(w.w, g.w, s.w, coef, alpha, oma, eps, nlr);
        p4[i] = w;
        s4[i] = s;
        if (part) g4[i] = g;
    }
    for (int64_t i = (nv << 2) + tid; i < n; i += stride) {
        float w = param[i], g = grad[i], s = square_avg[i];
        rmsprop1(w, g, s, coef, alpha, oma, eps, nlr);
        param[i] = w;
        square_avg[i] = s;
        if (part) grad[i] = g;
    }
}

}  // namespace

extern "C" int cstr_a2c_loss_f32(const cstr_a2c_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p || !workspace || !p->mean || !p->log_std || !p->actions || !p->values || !p->adv || !p->returns || !p->g_mean || !p->g_value ||
        !p->g_log_std || p->batch <= 0 || p->act_dim <= 0)
        return CSTR_E_BADARG;
    if (p->act_dim != 2 && p->act_dim != 4) return CSTR_E_UNSUPPORTED;
    if (p->batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    const int A = p->act_dim;
    if (p->ldm < A || (p->ldm * 4) % (A == 4 ? 16 : 8)) return CSTR_E_BADARG;
    if (!aligned8(workspace) || !row_aligned(p->mean, A) || !row_aligned(p->actions, A) || !row_aligned(p->g_mean, A) ||
        !aligned4(p->log_std) || !aligned4(p->values) || !aligned4(p->adv) || !aligned4(p->returns) || !aligned4(p->g_value) ||
        !aligned4(p->g_log_std) || (p->scalars_out && !aligned4(p->scalars_out)) || (p->log_prob_out && !aligned4(p->log_prob_out)))
        return CSTR_E_BADARG;
    {
        const int64_t B = p->batch;
        const void *ins[6] = {p->mean, p->log_std, p->actions, p->values, p->adv, p->returns};
        const int64_t in_n[6] = {(B - 1) * p->ldm + A, A, B * A, B, B, B};
        const void *outs[6] = {p->g_mean, p->g_value, p->g_log_std, p->scalars_out, p->log_prob_out, workspace};
        const int64_t out_n[6] = {B * A, B, A, 4, B, 2 * CSTR_PPO_WS_WORDS};
        for (int o = 0; o < 6; ++o) {
            if (!outs[o]) continue;
            for (int i = 0; i < 6; ++i)
                if (overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
            for (int q = o + 1; q < 6; ++q)
                if (outs[q] && overlap(outs[o], out_n[o], outs[q], out_n[q])) return CSTR_E_BADARG;
        }
    }
    const unsigned grid = lane_grid(p->batch, 256, CSTR_PPO_MAX_BLOCKS);
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(workspace);
    if (A == 2) a2c_loss_kernel<2><<<grid, 256, 0, (hipStream_t)stream>>>(*p, ws);
    else a2c_loss_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(*p, ws);
    return (int)hipGetLastError();
}

extern "C" int cstr_rmsprop_f32(float *param, float *grad, float *square_avg, const double *lr, double alpha, double eps, float max_norm,
                                uint64_t *workspace, float *norm_out, int64_t n, cstr_stream_t stream)
{
    if (!param || !grad || !square_avg || !lr || n <= 0 || max_norm != max_norm || !(alpha >= 0.0) || !(eps >= 0.0)) return CSTR_E_BADARG;
    if (!aligned16(param) || !aligned16(grad) || !aligned16(square_avg) || !aligned8(lr)) return CSTR_E_BADARG;
    if (overlap(param, n, grad, n) || overlap(param, n, square_avg, n) || overlap(grad, n, square_avg, n) || overlap(param, n, lr, 2) ||
        overlap(grad, n, lr, 2) || overlap(square_avg, n, lr, 2))
        return CSTR_E_BADARG;
    const bool clip = max_norm > 0.0f;
    if (clip) {
        if (!workspace || !aligned8(workspace) || (norm_out && !aligned4(norm_out))) return CSTR_E_BADARG;
        const void *arenas[3] = {param, grad, square_avg};
        for (int i = 0; i < 3; ++i)
            if (overlap(arenas[i], n, workspace, 2 * CSTR_PPO_WS_WORDS) || (norm_out && overlap(arenas[i], n, norm_out, 1))) return CSTR_E_BADARG;
        if (overlap(lr, 2, workspace, 2 * CSTR_PPO_WS_WORDS) || (norm_out && (overlap(workspace, 2 * CSTR_PPO_WS_WORDS, norm_out, 1) || overlap(lr, 2, norm_out, 1))))
            return CSTR_E_BADARG;
    }
    const double *part = nullptr;
    unsigned n_part = 0;
    if (clip) {  // launch 1: the sum-of-squares pass of cstr_grad_clip_f32
        n_part = lane_grid(n, 256, CSTR_PPO_MAX_BLOCKS);
        double *w = reinterpret_cast<double *>(workspace) + WS_PART0;
        grad_sumsq_kernel<<<n_part, 256, 0, (hipStream_t)stream>>>(grad, n, w);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
        part = w;
    }
    int block, grid;
    flat_launch_shape((n + 3) / 4, block, grid);
    if (block > 512) block = 512;  // the kernel's launch bound
    rmsprop_kernel<<<grid, block, 0, (hipStream_t)stream>>>(param, grad, square_avg, lr, (float)alpha, (float)(1.0 - alpha), (float)eps, part,
                                                           (int)n_part, max_norm, clip ? norm_out : nullptr, n);
    return (int)hipGetLastError();
}
