// cstr_ppo.hip -- PPO's own arithmetic around the Linear layers (reference core/ppo/ppo.py:184-300,
// core/common/on_policy_algorithm.py:162-268, core/common/buffers.py:343-521 RolloutBuffer, core/common/distributions.py
// DiagGaussianDistribution), f32, gfx950:
//   * the rollout head: action = mean + exp(log_std) * eps (stored unclipped), env_action = clip(action, low, high), log_prob;
//   * RolloutBuffer.add at the device-resident position, with the timeout bootstrap reward += gamma * V(terminal observation);
//   * compute_returns_and_advantage (GAE), one lane per env, NumPy's expression order and rounding points (bit-identical);
//   * the minibatch gather by flat swap_and_flatten indices (index i = env i / T, step i % T);
//   * the same add and gather on the goal face's buffer (cstr_goal_rollout_add_f32 / cstr_goal_ppo_gather_f32): the kernels are
//     templated on the row width, a 6-float row [achieved_goal | desired_goal | observation] moves as three float2;
//   * everything between evaluate_actions' outputs and loss.backward() (ppo.py:213-264): advantage normalisation, the diagonal
//     Gaussian's log-prob and entropy, ratio and clipped surrogate, the (clipped) value loss, the six logged scalars and the
//     gradients w.r.t. the action mean, the value and log_std (diag_gaussian_loss_kernel<A, true> of cstr_onpolicy_device.h);
//   * clip_grad_norm_ over the flat gradient arena (the coefficient stays on the device).
// Noise is READ when given and DRAWN otherwise: Philox4x32-10 keyed by rng_ctl[0], counter (rng_ctl[1] + row, 0, PPO tag) -> two
// Box-Muller pairs = the row's (up to four) draws; the last workgroup advances rng_ctl[1] by the row count.
// Batch reductions follow the convention at the top of cstr_onpolicy_device.h (fixed order, no float atomics). The gradient clip is
// two launches (partials, then every workgroup sums the partials in the same order and scales its share), so no workgroup waits for
// another inside a launch.
// NOT a batch reduction, and not order-deterministic: the Monitor-style episode statistics of the add launch (ep_stats: f64
// atomicAdd per finished episode, the convention of cstr_collect_step_f32). The count and the sum of lengths are integers in f64 and
// so exact in any order; the sum of returns, which only feeds the logged rollout/ep_rew_mean, may differ in its last f64 bits.
// NaN: the loss launch propagates a NaN as torch does (policy_term / value_term of cstr_onpolicy_device.h select around fminf /
// fmaxf, which DROP a NaN operand where torch.min / clamp keep it). A NaN log-prob or advantage of a row makes policy_loss, loss,
// d/d log_std and that row's d/d mean NaN (a NaN log-prob also approx_kl; clip_fraction stays finite, the comparison is false). A NaN
// value makes value_loss and loss NaN; its row's d/d value is NaN without the value clip and 0 with it (clamp's mask passes no
// gradient for a NaN step). Every other row's gradient keeps its bits. The rollout head's np.clip of the action (env_action) still
// goes through fminf / fmaxf: a NaN action reaches the env as `low`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t PPO_STREAM_TAG = 0x990A11C7u;  // counter word 3: never shares counters with the other heads' streams
constexpr int GOAL_ROW = 6;  // the goal face's flat row [achieved_goal | desired_goal | observation] (cstr_goal_vec_step_f32)

// on_policy_algorithm.py:199-216: one lane per env
template <int A>
__global__ __launch_bounds__(64) void diag_gaussian_act_kernel(const float *__restrict__ mean, const float *__restrict__ log_std,
                                                               const float *__restrict__ eps_in, uint64_t *__restrict__ rng_ctl,
                                                               const float *__restrict__ low, const float *__restrict__ high,
                                                               const int deterministic, float *__restrict__ action,
                                                               float *__restrict__ env_action, float *__restrict__ log_prob,
                                                               float *__restrict__ eps_out, const int64_t n)
{
    const bool draw = !deterministic && rng_ctl != nullptr;
    const uint64_t seed = draw ? rng_ctl[0] : 0ull, base = draw ? rng_ctl[1] : 0ull;
    float sig[A];
#pragma unroll
    for (int k = 0; k < A; ++k) sig[k] = expf(log_std[k]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float mu[A], e[A], a[A];
        load_row<A>(mean + i * A, mu);
        if (deterministic) {
#pragma unroll
            for (int k = 0; k < A; ++k) e[k] = 0.0f;
        } else if (draw) {
            const uint64_t ctr = base + (uint64_t)i;
            uint32_t r[4];
            float z[4];
            philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, PPO_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), r);
            box_muller(r[0], r[1], z[0], z[1]);
            if (A > 2) box_muller(r[2], r[3], z[2], z[3]);
#pragma unroll
            for (int k = 0; k < A; ++k) e[k] = z[k];
        } else {
            load_row<A>(eps_in + i * A, e);
        }
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = deterministic ? mu[k] : mu[k] + sig[k] * e[k];
        store_row<A>(action + i * A, a);
        if (eps_out) store_row<A>(eps_out + i * A, e);
        if (log_prob) log_prob[i] = diag_log_prob<A>(a, mu, sig);
        if (env_action) {
            float c[A];
#pragma unroll
            for (int k = 0; k < A; ++k) c[k] = low ? fminf(fmaxf(a[k], low[k]), high[k]) : a[k];  // np.clip
            store_row<A>(env_action + i * A, c);
        }
    }
    if (draw && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0)
        rng_ctl[1] = base + (uint64_t)n;
}

// One observation row: float4 pieces where the width is a multiple of four (16-byte-aligned rows), float2 pieces otherwise (the goal
// face's 6-float rows, 8-byte aligned)
template <int D> __device__ __forceinline__ void copy_obs_row(const float *src, float *dst)
{
    constexpr int V = D % 4 == 0 ? 4 : 2;
    static_assert(D % V == 0, "an observation row is a whole number of vector pieces");
#pragma unroll
    for (int c = 0; c < D; c += V) {
        float v[V];
        load_row<V>(src + c, v);
        store_row<V>(dst + c, v);
    }
}

// buffers.py:440-479 + on_policy_algorithm.py:236-245. ctl = { pos, full, ticket, adds }; a full buffer takes no row.
template <int D, int A>
__global__ __launch_bounds__(64) void rollout_add_kernel(const cstr_rollout_t rb, int64_t *__restrict__ ctl, const float *__restrict__ obs,
                                                         const float *__restrict__ act, const float *__restrict__ reward,
                                                         float *episode_start, const float *__restrict__ value,
                                                         const float *__restrict__ log_prob, const float *__restrict__ timeout,
                                                         const float *__restrict__ terminal_value, const float gamma,
                                                         const float *__restrict__ done, float *__restrict__ ep_return,
                                                         int32_t *__restrict__ ep_len, double *__restrict__ ep_stats)
{
    const int64_t pos = ctl[0], n = rb.n_envs;
    const bool room = pos >= 0 && pos < rb.rows;
    if (room) {
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t r = pos * n + i;
            copy_obs_row<D>(obs + i * D, rb.obs + r * D);
            float a[A];
            load_row<A>(act + i * A, a);
            store_row<A>(rb.act + r * A, a);
            float rw = reward[i];
            if (ep_stats) {  // Monitor semantics on the env's own reward: return / length of the episode that ends here
                const float ret = ep_return[i] + rw;
                const int32_t len = ep_len[i] + 1;
                const bool d = done[i] != 0.0f;
                ep_return[i] = d ? 0.0f : ret;
                ep_len[i] = d ? 0 : len;
                if (d) {
                    atomicAdd(ep_stats + 0, 1.0);
                    atomicAdd(ep_stats + 1, (double)ret);
                    atomicAdd(ep_stats + 2, (double)len);
                }
            }
            if (timeout && timeout[i] != 0.0f) rw = rw + gamma * terminal_value[i];
            rb.rew[r] = rw;
            rb.episode_start[r] = episode_start[i];
            if (done) episode_start[i] = done[i];  // _last_episode_starts = dones (on_policy_algorithm.py:256)
            rb.values[r] = value[i];
            rb.log_probs[r] = log_prob[i];
            rb.advantages[r] = 0.0f;
            rb.returns[r] = 0.0f;
        }
    }
    if (last_block_ticket(reinterpret_cast<unsigned long long *>(ctl + 2)) && threadIdx.x == 0 && room) {
        ctl[0] = pos + 1;
        if (pos + 1 == rb.rows) ctl[1] = 1;
        ctl[3] += 1;
    }
}

// buffers.py:403-438 in NumPy's order: delta = r + (g * v_next) * nnt - v;  gae = delta + ((gl * nnt) * gae);  g = f32(gamma),
// gl = f32(gamma * gae_lambda) (the product is formed in double); returns = advantages + values
__global__ __launch_bounds__(64) void gae_kernel(const float *__restrict__ rewards, const float *__restrict__ values,
                                                 const float *__restrict__ episode_starts, const float *__restrict__ last_values,
                                                 const float *__restrict__ dones, const float g, const float gl,
                                                 float *__restrict__ advantages, float *__restrict__ returns, const int64_t T,
                                                 const int64_t N)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        float gae = 0.0f, nnt = 1.0f - dones[i], v_next = last_values[i];
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t r = t * N + i;
            const float v = values[r];
            const float delta = (rewards[r] + (g * v_next) * nnt) - v;
            gae = delta + (gl * nnt) * gae;
            advantages[r] = gae;
            returns[r] = gae + v;
            nnt = 1.0f - episode_starts[r];
            v_next = v;
        }
    }
}

// buffers.py:481-521: flat index i (swap_and_flatten) = env i / T, step i % T; indices are clamped into the buffer
template <int D, int A>
__global__ __launch_bounds__(256) void ppo_gather_kernel(const cstr_rollout_t rb, const int64_t *__restrict__ idx, const int64_t batch,
                                                         float *__restrict__ obs, float *__restrict__ act, float *__restrict__ old_value,
                                                         float *__restrict__ old_log_prob, float *__restrict__ adv, float *__restrict__ ret)
{
    const int64_t T = rb.rows, N = rb.n_envs, total = T * N;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < batch; b += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);
        const int64_t env = i / T, step = i - env * T, r = step * N + env;
        copy_obs_row<D>(rb.obs + r * D, obs + b * D);
        float a[A];
        load_row<A>(rb.act + r * A, a);
        store_row<A>(act + b * A, a);
        old_value[b] = rb.values[r];
        old_log_prob[b] = rb.log_probs[r];
        adv[b] = rb.advantages[r];
        ret[b] = rb.returns[r];
    }
}

// clip_grad_norm_ (torch.nn.utils), launch 2 behind grad_sumsq_kernel: coef = min(1, max_norm / (norm + 1e-6)); grad *= coef (torch
// multiplies also when the coefficient is 1)
__global__ __launch_bounds__(256) void grad_scale_kernel(float *__restrict__ grad, const int64_t n, const double *__restrict__ part,
                                                         const int n_part, const float max_norm, float *__restrict__ norm_out)
{
    float norm;
    const float coef = grad_clip_coef(part, n_part, max_norm, norm);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256ll) grad[i] = grad[i] * coef;
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
}

// The two faces of the rollout buffer's entry points: which widths they take and how an observation row must be aligned.
// BoxFace: act_dim 1 is the Categorical head's action row, the index as one float (cstr_categorical.hip).
struct BoxFace {
    static bool widths_ok(int obs_dim, int act_dim) { return (obs_dim == 4 || obs_dim == 8) && (act_dim == 1 || act_dim == 2 || act_dim == 4); }
    static bool obs_aligned(const void *p) { return aligned16(p); }
};
// GoalFace: the flat row of cstr_goal_vec_step_f32, GOAL_ROW floats, and the valve pair
struct GoalFace {
    static bool widths_ok(int obs_dim, int act_dim) { return obs_dim == GOAL_ROW && act_dim == 2; }
    static bool obs_aligned(const void *p) { return aligned8(p); }
};

template <class Face> inline int rollout_check(const cstr_rollout_t *rb)
{
    if (!rb || !rb->obs || !rb->act || !rb->rew || !rb->episode_start || !rb->values || !rb->log_probs || !rb->advantages ||
        !rb->returns || rb->rows <= 0 || rb->n_envs <= 0 || rb->obs_dim <= 0 || rb->act_dim <= 0)
        return CSTR_E_BADARG;
    if (!Face::widths_ok(rb->obs_dim, rb->act_dim)) return CSTR_E_UNSUPPORTED;
    if (rb->rows > CSTR_PPO_MAX_ROWS / rb->n_envs) return CSTR_E_UNSUPPORTED;
    if (!Face::obs_aligned(rb->obs) || !row_aligned(rb->act, rb->act_dim) || !aligned4(rb->rew) || !aligned4(rb->episode_start) ||
        !aligned4(rb->values) || !aligned4(rb->log_probs) || !aligned4(rb->advantages) || !aligned4(rb->returns))
        return CSTR_E_BADARG;
    return 0;
}

// validation of both add entry points, then the launch of the face's instantiation
template <class Face>
inline int rollout_add(const cstr_rollout_t *rb, int64_t *ctl, const float *obs, const float *act, const float *reward, float *episode_start,
                       const float *value, const float *log_prob, const float *timeout, const float *terminal_value, float gamma,
                       const float *done, float *ep_return, int32_t *ep_len, double *ep_stats, cstr_stream_t stream)
{
    const int rc = rollout_check<Face>(rb);
    if (rc) return rc;
    if (!ctl || !obs || !act || !reward || !episode_start || !value || !log_prob) return CSTR_E_BADARG;
    if ((timeout == nullptr) != (terminal_value == nullptr)) return CSTR_E_BADARG;
    if ((ep_stats == nullptr) != (ep_return == nullptr) || (ep_stats == nullptr) != (ep_len == nullptr) || (ep_stats && !done))
        return CSTR_E_BADARG;  // the episode statistics: all three or none, and they need `done`
    if ((done && (!aligned4(done) || overlap(done, rb->n_envs, episode_start, rb->n_envs))) ||
        (ep_stats && (!aligned8(ep_stats) || !aligned4(ep_return) || !aligned4(ep_len))))
        return CSTR_E_BADARG;
    if (!aligned8(ctl) || !Face::obs_aligned(obs) || !row_aligned(act, rb->act_dim) || !aligned4(reward) || !aligned4(episode_start) ||
        !aligned4(value) || !aligned4(log_prob) || (timeout && (!aligned4(timeout) || !aligned4(terminal_value))))
        return CSTR_E_BADARG;
    const int64_t n = rb->n_envs, cells = rb->rows * n;
    if (overlap(rb->obs, cells * rb->obs_dim, obs, n * rb->obs_dim) || overlap(rb->act, cells * rb->act_dim, act, n * rb->act_dim) ||
        overlap(rb->rew, cells, reward, n) || overlap(rb->episode_start, cells, episode_start, n) || overlap(rb->values, cells, value, n) ||
        overlap(rb->log_probs, cells, log_prob, n))
        return CSTR_E_BADARG;
    const unsigned grid = lane_grid(n, 64, 4096);
    const int d = rb->obs_dim, a = rb->act_dim;
#define ADD_LAUNCH(D, A)                                                                                                              \
    rollout_add_kernel<D, A><<<grid, 64, 0, (hipStream_t)stream>>>(*rb, ctl, obs, act, reward, episode_start, value, log_prob, timeout, \
                                                                  terminal_value, gamma, done, ep_return, ep_len, ep_stats)
    if (d == GOAL_ROW) ADD_LAUNCH(GOAL_ROW, 2);  // GoalFace alone gets here: BoxFace::widths_ok has refused the width
    else if (d == 4 && a == 1) ADD_LAUNCH(4, 1);
    else if (a == 1) ADD_LAUNCH(8, 1);
    else if (d == 4 && a == 2) ADD_LAUNCH(4, 2);
    else if (d == 4) ADD_LAUNCH(4, 4);
    else if (a == 2) ADD_LAUNCH(8, 2);
    else ADD_LAUNCH(8, 4);
#undef ADD_LAUNCH
    return (int)hipGetLastError();
}

// validation of both gather entry points, then the launch of the face's instantiation
template <class Face>
inline int ppo_gather(const cstr_rollout_t *rb, const int64_t *idx, int64_t batch, float *obs, float *act, float *old_value,
                      float *old_log_prob, float *adv, float *ret, cstr_stream_t stream)
{
    const int rc = rollout_check<Face>(rb);
    if (rc) return rc;
    if (!idx || !obs || !act || !old_value || !old_log_prob || !adv || !ret || batch <= 0) return CSTR_E_BADARG;
    if (batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!aligned8(idx) || !Face::obs_aligned(obs) || !row_aligned(act, rb->act_dim) || !aligned4(old_value) || !aligned4(old_log_prob) ||
        !aligned4(adv) || !aligned4(ret))
        return CSTR_E_BADARG;
    const int64_t cells = rb->rows * rb->n_envs;
    const Buf outs[6] = {{obs, batch * rb->obs_dim}, {act, batch * rb->act_dim}, {old_value, batch}, {old_log_prob, batch}, {adv, batch},
                         {ret, batch}};
    const Buf ins[7] = {{rb->obs, cells * rb->obs_dim}, {rb->act, cells * rb->act_dim}, {rb->values, cells}, {rb->log_probs, cells},
                        {rb->advantages, cells}, {rb->returns, cells}, {idx, 2 * batch}};
    if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    const unsigned grid = lane_grid(batch, 256, 2048);
    const int d = rb->obs_dim, a = rb->act_dim;
#define GATHER_LAUNCH(D, A) \
    ppo_gather_kernel<D, A><<<grid, 256, 0, (hipStream_t)stream>>>(*rb, idx, batch, obs, act, old_value, old_log_prob, adv, ret)
    if (d == GOAL_ROW) GATHER_LAUNCH(GOAL_ROW, 2);  // GoalFace alone gets here: BoxFace::widths_ok has refused the width
    else if (d == 4 && a == 1) GATHER_LAUNCH(4, 1);
    else if (a == 1) GATHER_LAUNCH(8, 1);
    else if (d == 4 && a == 2) GATHER_LAUNCH(4, 2);
    else if (d == 4) GATHER_LAUNCH(4, 4);
    else if (a == 2) GATHER_LAUNCH(8, 2);
    else GATHER_LAUNCH(8, 4);
#undef GATHER_LAUNCH
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cstr_diag_gaussian_act_f32(const float *mean, const float *log_std, const float *eps_in, uint64_t *rng_ctl, const float *low,
                                          const float *high, int deterministic, float *action, float *env_action, float *log_prob,
                                          float *eps_out, int64_t n, int act_dim, cstr_stream_t stream)
{
    if (!mean || !log_std || !action || n <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if (!deterministic && (eps_in == nullptr) == (rng_ctl == nullptr)) return CSTR_E_BADARG;  // exactly one noise source
    if ((low == nullptr) != (high == nullptr)) return CSTR_E_BADARG;
    if (act_dim != 2 && act_dim != 4) return CSTR_E_UNSUPPORTED;
    if (n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!row_aligned(mean, act_dim) || !row_aligned(action, act_dim) || (eps_in && !row_aligned(eps_in, act_dim)) ||
        (env_action && !row_aligned(env_action, act_dim)) || (eps_out && !row_aligned(eps_out, act_dim)) || !aligned4(log_std) ||
        (log_prob && !aligned4(log_prob)) || (rng_ctl && !aligned8(rng_ctl)))
        return CSTR_E_BADARG;
    {
        const int64_t na = n * act_dim;
        const Buf ins[3] = {{mean, na}, {deterministic ? nullptr : eps_in, na}, {log_std, act_dim}};
        const Buf outs[4] = {{action, na}, {env_action, na}, {log_prob, n}, {eps_out, na}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    const unsigned grid = lane_grid(n, 64, 4096);
    if (act_dim == 2)
        diag_gaussian_act_kernel<2><<<grid, 64, 0, (hipStream_t)stream>>>(mean, log_std, eps_in, rng_ctl, low, high, deterministic, action,
                                                                         env_action, log_prob, eps_out, n);
    else
        diag_gaussian_act_kernel<4><<<grid, 64, 0, (hipStream_t)stream>>>(mean, log_std, eps_in, rng_ctl, low, high, deterministic, action,
                                                                         env_action, log_prob, eps_out, n);
    return (int)hipGetLastError();
}

extern "C" int cstr_rollout_add_f32(const cstr_rollout_t *rb, int64_t *ctl, const float *obs, const float *act, const float *reward,
                                    float *episode_start, const float *value, const float *log_prob, const float *timeout,
                                    const float *terminal_value, float gamma, const float *done, float *ep_return, int32_t *ep_len,
                                    double *ep_stats, cstr_stream_t stream)
{
    return rollout_add<BoxFace>(rb, ctl, obs, act, reward, episode_start, value, log_prob, timeout, terminal_value, gamma, done, ep_return,
                                ep_len, ep_stats, stream);
}

extern "C" int cstr_goal_rollout_add_f32(const cstr_rollout_t *rb, int64_t *ctl, const float *rows, const float *act, const float *reward,
                                         float *episode_start, const float *value, const float *log_prob, const float *timeout,
                                         const float *terminal_value, float gamma, const float *done, float *ep_return, int32_t *ep_len,
                                         double *ep_stats, cstr_stream_t stream)
{
    return rollout_add<GoalFace>(rb, ctl, rows, act, reward, episode_start, value, log_prob, timeout, terminal_value, gamma, done, ep_return,
                                 ep_len, ep_stats, stream);
}

extern "C" int cstr_gae_f32(const float *rewards, const float *values, const float *episode_starts, const float *last_values,
                            const float *dones, double gamma, double gae_lambda, float *advantages, float *returns, int64_t n_steps,
                            int64_t n_envs, cstr_stream_t stream)
{
    if (!rewards || !values || !episode_starts || !last_values || !dones || !advantages || !returns || n_steps <= 0 || n_envs <= 0)
        return CSTR_E_BADARG;
    if (n_steps > CSTR_PPO_MAX_ROWS / n_envs) return CSTR_E_UNSUPPORTED;
    const void *all[7] = {rewards, values, episode_starts, last_values, dones, advantages, returns};
    for (int i = 0; i < 7; ++i)
        if (!aligned4(all[i])) return CSTR_E_BADARG;
    const int64_t cells = n_steps * n_envs;
    const Buf ins[5] = {{rewards, cells}, {values, cells}, {episode_starts, cells}, {last_values, n_envs}, {dones, n_envs}};
    const Buf outs[2] = {{advantages, cells}, {returns, cells}};
    if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    // NEP 50: a Python float times a float32 array rounds the float to float32; gamma * gae_lambda is a product of two Python floats
    gae_kernel<<<lane_grid(n_envs, 64, 4096), 64, 0, (hipStream_t)stream>>>(rewards, values, episode_starts, last_values, dones, (float)gamma,
                                                                           (float)(gamma * gae_lambda), advantages, returns, n_steps,
                                                                           n_envs);
    return (int)hipGetLastError();
}

extern "C" int cstr_ppo_gather_f32(const cstr_rollout_t *rb, const int64_t *idx, int64_t batch, float *obs, float *act, float *old_value,
                                   float *old_log_prob, float *adv, float *ret, cstr_stream_t stream)
{
    return ppo_gather<BoxFace>(rb, idx, batch, obs, act, old_value, old_log_prob, adv, ret, stream);
}

extern "C" int cstr_goal_ppo_gather_f32(const cstr_rollout_t *rb, const int64_t *idx, int64_t batch, float *rows, float *act,
                                        float *old_value, float *old_log_prob, float *adv, float *ret, cstr_stream_t stream)
{
    return ppo_gather<GoalFace>(rb, idx, batch, rows, act, old_value, old_log_prob, adv, ret, stream);
}

extern "C" int cstr_ppo_loss_f32(const cstr_ppo_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    return p ? diag_gaussian_loss_launch<true>(p, workspace, stream) : CSTR_E_BADARG;
}

extern "C" int cstr_grad_clip_f32(float *grad, int64_t n, float max_norm, uint64_t *workspace, float *norm_out, cstr_stream_t stream)
{
    if (!grad || !workspace || n <= 0 || !(max_norm >= 0.0f)) return CSTR_E_BADARG;
    if (!aligned4(grad) || !aligned8(workspace) || (norm_out && !aligned4(norm_out))) return CSTR_E_BADARG;
    if (overlap(grad, n, workspace, 2 * CSTR_PPO_WS_WORDS) || (norm_out && overlap(grad, n, norm_out, 1)) ||
        (norm_out && overlap(workspace, 2 * CSTR_PPO_WS_WORDS, norm_out, 1)))
        return CSTR_E_BADARG;
    const unsigned grid = lane_grid(n, 256, CSTR_PPO_MAX_BLOCKS);
    double *part = reinterpret_cast<double *>(workspace) + WS_PART0;
    grad_sumsq_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(grad, n, part);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    grad_scale_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(grad, n, part, (int)grid, max_norm, norm_out);
    return (int)hipGetLastError();
}
