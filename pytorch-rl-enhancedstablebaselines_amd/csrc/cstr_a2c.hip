// cstr_a2c.hip -- A2C's own arithmetic and its optimiser (reference core/a2c/a2c.py:132-190), f32, gfx950:
//   * everything between evaluate_actions' outputs and loss.backward() (a2c.py:150-171) in ONE launch: advantage normalisation, the
//     diagonal Gaussian's log-prob and entropy, the policy-gradient and value losses, the four scalars and the gradients w.r.t. the
//     action mean, the value and log_std. The kernel is PPO's with the other objective (diag_gaussian_loss_kernel<A, false> of
//     cstr_onpolicy_device.h, where the reduction convention is stated); cstr_a2c_loss_f32 fills its arguments.
//   * torch.optim.RMSprop (momentum 0, not centred, no weight decay) over one flat arena with clip_grad_norm_ folded in: launch 1 is
//     the sum-of-squares pass of cstr_grad_clip_f32 (same grid, same partials), launch 2 forms the coefficient from the partials as
//     grad_scale_kernel does, scales each gradient in register, writes it back and takes the step. Without clipping: one launch and
//     the gradient is only read.
//   * RMSpropTFLike (reference core/common/sb2_compat/rmsprop_tf_like.py:90-135: square_avg starts at ones, epsilon inside the square
//     root; weight decay, centred and momentum forms) with the same launch shape and the same folded clip: rmsprop_tf_kernel<WD,
//     CENTRED, MOMENTUM>, eight instantiations, each reading and writing only the arenas its form has.
// NaN: with normalize_advantage the statistics are taken over any batch, one row included, where the unbiased standard deviation is
// 0 / 0 = NaN (torch.std of one element): the policy loss and its gradients are then NaN, as in the reference, which unlike PPO has
// no `len > 1` guard (a2c.py:155-156).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"

namespace {

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

// RMSpropTFLike's single-tensor step (rmsprop_tf_like.py:112-135), every operation rounded to f32; where the operation is the same the
// order is rmsprop1's. `sq - ga * ga` can round below -eps: the square root is then NaN, as the reference's is.
template <bool WD, bool CENTRED, bool MOMENTUM>
__device__ __forceinline__ void rmsprop_tf1(float &w, float &g, float &sq, float &buf, float &ga, const float coef, const float alpha,
                                            const float oma, const float eps, const float wd, const float mom, const float nlr)
{
    g = g * coef;  // what is written back to grad: the clipped gradient before weight decay, as clip_grad_norm_ leaves it
    float gd = g;
    if (WD) gd = gd + wd * w;
    sq = sq * alpha + (oma * gd) * gd;
    float avg;
    if (CENTRED) {
        ga = ga * alpha + oma * gd;
        avg = sqrtf((sq - ga * ga) + eps);
    } else {
        avg = sqrtf(sq + eps);
    }
    if (MOMENTUM) {
        buf = buf * mom + gd / avg;
        w = w + nlr * buf;
    } else {
        w = w + (nlr * gd) / avg;
    }
}

// part != NULL: launch 2 of the clipped step, as in rmsprop_kernel. momentum_buf / grad_avg are touched only by the forms that have them.
template <bool WD, bool CENTRED, bool MOMENTUM>
__global__ __launch_bounds__(512) void rmsprop_tf_kernel(float *__restrict__ param, float *__restrict__ grad, float *__restrict__ square_avg,
                                                         float *__restrict__ momentum_buf, float *__restrict__ grad_avg,
                                                         const double *__restrict__ lr, const float alpha, const float oma, const float eps,
                                                         const float wd, const float mom, const double *__restrict__ part, const int n_part,
                                                         const float max_norm, float *__restrict__ norm_out, const int64_t n)
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
    float4 *b4 = reinterpret_cast<float4 *>(momentum_buf), *a4 = reinterpret_cast<float4 *>(grad_avg);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < nv; i += stride) {
        float4 w = p4[i], g = g4[i], s = s4[i], b = make_float4(0.f, 0.f, 0.f, 0.f), a = b;
        if (MOMENTUM) b = b4[i];
        if (CENTRED) a = a4[i];
        rmsprop_tf1<WD, CENTRED, MOMENTUM>(w.x, g.x, s.x, b.x, a.x, coef, alpha, oma, eps, wd, mom, nlr);
        rmsprop_tf1<WD, CENTRED, MOMENTUM>(w.y, g.y, s.y, b.y, a.y, coef, alpha, oma, eps, wd, mom, nlr);
        rmsprop_tf1<WD, CENTRED, MOMENTUM>(w.z, g.z, s.z, b.z, a.z, coef, alpha, oma, eps, wd, mom, nlr);
        rmsprop_tf1<WD, CENTRED, MOMENTUM>(w.w, g.w, s.w, b.w, a.w, coef, alpha, oma, eps, wd, mom, nlr);
        p4[i] = w;
        s4[i] = s;
        if (MOMENTUM) b4[i] = b;
        if (CENTRED) a4[i] = a;
        if (part) g4[i] = g;
    }
    for (int64_t i = (nv << 2) + tid; i < n; i += stride) {
        float w = param[i], g = grad[i], s = square_avg[i], b = 0.f, a = 0.f;
        if (MOMENTUM) b = momentum_buf[i];
        if (CENTRED) a = grad_avg[i];
        rmsprop_tf1<WD, CENTRED, MOMENTUM>(w, g, s, b, a, coef, alpha, oma, eps, wd, mom, nlr);
        param[i] = w;
        square_avg[i] = s;
        if (MOMENTUM) momentum_buf[i] = b;
        if (CENTRED) grad_avg[i] = a;
        if (part) grad[i] = g;
    }
}

typedef void (*rmsprop_tf_fn)(float *, float *, float *, float *, float *, const double *, float, float, float, float, float, const double *,
                              int, float, float *, int64_t);
// index: weight decay * 4 + centred * 2 + momentum
const rmsprop_tf_fn RMSPROP_TF_FORMS[8] = {
    rmsprop_tf_kernel<false, false, false>, rmsprop_tf_kernel<false, false, true>, rmsprop_tf_kernel<false, true, false>,
    rmsprop_tf_kernel<false, true, true>,   rmsprop_tf_kernel<true, false, false>, rmsprop_tf_kernel<true, false, true>,
    rmsprop_tf_kernel<true, true, false>,   rmsprop_tf_kernel<true, true, true>};

}  // namespace

extern "C" int cstr_a2c_loss_f32(const cstr_a2c_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p) return CSTR_E_BADARG;
    cstr_ppo_loss_t k = {};  // no old_values, old_log_prob, clip ranges or scalars_sum: the A2C objective reads none of them
    k.mean = p->mean, k.ldm = p->ldm, k.log_std = p->log_std, k.actions = p->actions, k.values = p->values;
    k.adv = p->adv, k.returns = p->returns, k.batch = p->batch, k.act_dim = p->act_dim, k.normalize_advantage = p->normalize_advantage;
    k.ent_coef = p->ent_coef, k.vf_coef = p->vf_coef, k.g_mean = p->g_mean, k.g_value = p->g_value, k.g_log_std = p->g_log_std;
    k.scalars_out = p->scalars_out, k.log_prob_out = p->log_prob_out;
    return diag_gaussian_loss_launch<false>(&k, workspace, stream);
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

extern "C" int cstr_rmsprop_tf_f32(float *param, float *grad, float *square_avg, float *momentum_buf, float *grad_avg, const double *lr,
                                   double alpha, double eps, double weight_decay, double momentum, float max_norm, uint64_t *workspace,
                                   float *norm_out, int64_t n, cstr_stream_t stream)
{
    if (!param || !grad || !square_avg || !lr || n <= 0 || max_norm != max_norm) return CSTR_E_BADARG;
    if (!(alpha >= 0.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) || !(momentum >= 0.0)) return CSTR_E_BADARG;
    if ((momentum_buf != nullptr) != (momentum > 0.0)) return CSTR_E_BADARG;
    const void *arenas[5] = {param, grad, square_avg, momentum_buf, grad_avg};  // the optional two may be NULL
    for (int i = 0; i < 5; ++i) {
        if (!arenas[i]) continue;
        if (!aligned16(arenas[i]) || overlap(arenas[i], n, lr, 2)) return CSTR_E_BADARG;
        for (int j = i + 1; j < 5; ++j)
            if (arenas[j] && overlap(arenas[i], n, arenas[j], n)) return CSTR_E_BADARG;
    }
    if (!aligned8(lr)) return CSTR_E_BADARG;
    const bool clip = max_norm > 0.0f;
    if (clip) {
        if (!workspace || !aligned8(workspace) || (norm_out && !aligned4(norm_out))) return CSTR_E_BADARG;
        for (int i = 0; i < 5; ++i)
            if (arenas[i] && (overlap(arenas[i], n, workspace, 2 * CSTR_PPO_WS_WORDS) || (norm_out && overlap(arenas[i], n, norm_out, 1))))
                return CSTR_E_BADARG;
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
    const int form = (weight_decay != 0.0 ? 4 : 0) + (grad_avg ? 2 : 0) + (momentum > 0.0 ? 1 : 0);
    RMSPROP_TF_FORMS[form]<<<grid, block, 0, (hipStream_t)stream>>>(param, grad, square_avg, momentum_buf, grad_avg, lr, (float)alpha,
                                                                    (float)(1.0 - alpha), (float)eps, (float)weight_decay, (float)momentum,
                                                                    part, (int)n_part, max_norm, clip ? norm_out : nullptr, n);
    return (int)hipGetLastError();
}
