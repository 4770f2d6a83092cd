// cstr_gaussian_device.h -- the actor head's per-element arithmetic, stated once (internal, included by cstr_mlp.hip, cstr_eval.hip and
// cstr_chain.hip): the squashed diagonal Gaussian (core/common/distributions.py:161-260) forward and backward for ONE (row, action),
// and the deterministic head's output activation. Every kernel that samples an action, evaluates its log-prob or differentiates them
// calls these, so launches that promise each other's bits (the head launches, the policy launches, the evaluation kernel, the row
// chains) keep the promise by construction. Each caller keeps its own summation order over the action dimension. Every TU that
// includes this is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2;

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;  // core/sac/policies.py:20-22

// mean, raw log_std, eps -> action: sd = exp(clamp(raw)) (policies.py:173), u = mean + sd * eps (Normal.rsample,
// distributions.py:183), a = tanh(u). sd and u are handed on to the log-prob terms, so a kernel whose critical path needs only the
// action can evaluate them later (or not at all). The mode is e = 0.0f: u = mu + sd * 0.0f, what a sampling launch gives for eps = 0.
__device__ __forceinline__ void sample_action_act(const float mu, const float raw, const float e, float &a, float &sd, float &u)
{
    const float ls = fminf(fmaxf(raw, LOG_STD_MIN), LOG_STD_MAX);
    sd = expf(ls);
    u = mu + sd * e;
    a = tanhf(u);
}

// this action's Normal log-pdf (torch Normal.log_prob) ...
__device__ __forceinline__ float gaussian_logp_term(const float mu, const float sd, const float u)
{
    const float half_log_2pi = 0.91893853320467274178f;  // math.log(math.sqrt(2 * math.pi))
    const float d = u - mu, var = sd * sd;
    return -(d * d) / (2.0f * var) - logf(sd) - half_log_2pi;
}

// ... and its tanh correction (distributions.py:232): logp = sum_j gaussian_logp_term - sum_j tanh_correction_term
__device__ __forceinline__ float tanh_correction_term(const float a) { return logf(1.0f - a * a + 1e-6f); }

// Analytic backward for one (row, action): ga = d/d action, gl = d/d logp of the row. With d = sd * eps the Gaussian term is
// -eps^2/2 - ls - c, so
//   dlogp/du = 2 a (1 - a^2) / (1 - a^2 + 1e-6),  da/du = 1 - a^2
//   gu = d/d mean,  gls = d/d raw log_std = gu * eps * sd - gl inside the clamp range, 0 outside
// (autograd through the reference's expression adds terms that cancel to rounding noise, ~1e-7 relative).
__device__ __forceinline__ void squashed_gaussian_grad(const float a, const float raw, const float eps, const float ga, const float gl,
                                                       float &gu, float &gls)
{
    const float s = expf(fminf(fmaxf(raw, LOG_STD_MIN), LOG_STD_MAX));
    const float one_m = 1.0f - a * a;
    gu = ga * one_m + gl * (2.0f * a * one_m / (one_m + 1e-6f));
    gls = (raw >= LOG_STD_MIN && raw <= LOG_STD_MAX) ? gu * eps * s - gl : 0.0f;
}

// the deterministic head's output activation (TD3 / DDPG actors: out_act is a run-time field of the network)
__device__ __forceinline__ float head_out_act(float v, const int out_act)
{
    if (out_act == ACT_RELU) v = fmaxf(v, 0.0f);
    if (out_act == ACT_TANH) v = tanhf(v);
    return v;
}

}  // namespace
