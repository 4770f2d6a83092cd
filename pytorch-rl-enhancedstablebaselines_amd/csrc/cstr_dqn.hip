// cstr_dqn.hip -- DQN's own arithmetic around the Q network's Linear layers (reference core/dqn/dqn.py:168-256), gfx950:
//   * one RandomState.random_sample() from the HBM image of NumPy's legacy MT19937 stream and its comparison with the exploration
//     rate (dqn.py:245, `np.random.rand() < self.exploration_rate`): the stream the replay sampler shares advances, twist included;
//   * action selection over a discretised valve pair: greedy (first maximum of the row, torch's argmax; a NaN counts as the
//     greatest value, the first one wins), the reference's all-or-none exploration, or epsilon-greedy per row; the output is the
//     index and the normalised valve pair v(i), v(j), (i, j) = (a / K, a % K), v(q) = -1 + (2 q) / (K - 1) in f32;
//   * everything between the two forward passes and loss.backward() (dqn.py:195-212) in ONE launch: the greedy target, the gather
//     of the taken action's value (its index recovered from the stored valve pair), the Huber loss and its gradient.
// Uniforms are READ when given and DRAWN otherwise: Philox4x32-10 keyed by rng_ctl[0], counter (rng_ctl[1] + row, 0, DQN tag); words
// 0 and 1 give u[row][0] and u[row][1] as (word >> 8) * 2^-24 in [0, 1). The last workgroup advances rng_ctl[1] by the row count,
// in every launch that draws (mode 1 also when the flag is 0: the launch sequence, not the data, decides the stream position).
// The batch reduction follows the convention at the top of cstr_onpolicy_device.h (fixed order, no float atomics), with one slot and
// one workspace word per workgroup.
// One lane per row: a row of at most 256 Q values is scanned by its lane. The launches are latency-bound at the batch sizes DQN
// uses (32 rows by default); nothing here is tuned for bandwidth.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_mt_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t DQN_STREAM_TAG = 0xD09A11C7u;  // counter word 3: never shares counters with the other heads' streams

// first maximum of a row; a NaN is the greatest value (torch.argmax / torch.max)
__device__ __forceinline__ int row_argmax(const float *__restrict__ row, const int M, float &best)
{
    int arg = 0;
    best = row[0];
    for (int c = 1; c < M; ++c) {
        const float v = row[c];
        if (v > best || (v != v && best == best)) { best = v; arg = c; }
    }
    return arg;
}

// dqn.py:245 on the legacy stream image: one wave
__global__ __launch_bounds__(64) void rand_flag_kernel(uint32_t *__restrict__ mt_state, const double *__restrict__ threshold,
                                                       int32_t *__restrict__ flag_out, double *__restrict__ draw_out)
{
    __shared__ uint32_t mt[MT_N];
    const int lane = threadIdx.x;
    for (int i = lane; i < MT_N; i += 64) mt[i] = mt_state[i];
    int pos = (int)mt_state[MT_N];
    if (pos < 0 || pos > MT_N) pos = MT_N;
    __syncthreads();
    bool twisted = false;
    uint32_t w[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (pos == MT_N) {  // wave-uniform
            mt_twist_wave(mt, lane);
            __syncthreads();
            pos = 0;
            twisted = true;
        }
        w[k] = mt_temper(mt[pos]);
        ++pos;
    }
    if (twisted)
        for (int i = lane; i < MT_N; i += 64) mt_state[i] = mt[i];
    if (lane == 0) {
        mt_state[MT_N] = (uint32_t)pos;
        // mt19937_next_double: (a * 2^26 + b) / 2^53 with a = w0 >> 5, b = w1 >> 6
        const double d = ((double)(int)(w[0] >> 5) * 67108864.0 + (double)(int)(w[1] >> 6)) / 9007199254740992.0;
        flag_out[0] = d < threshold[0] ? 1 : 0;
        if (draw_out) draw_out[0] = d;
    }
}

// one lane per row
__global__ __launch_bounds__(64) void dqn_act_kernel(const float *__restrict__ q, const int64_t ldq, const int64_t n, const int M, const int K,
                                                     const int mode, const double *__restrict__ eps, const int32_t *__restrict__ flag,
                                                     const float *__restrict__ u_in, uint64_t *__restrict__ rng_ctl,
                                                     float *__restrict__ valve_out, int64_t *__restrict__ index_out)
{
    const bool draw = mode != 0 && rng_ctl != nullptr;
    const uint64_t seed = draw ? rng_ctl[0] : 0ull, base = draw ? rng_ctl[1] : 0ull;
    const bool all_explore = mode == 1 && flag[0] != 0;
    const double e = mode == 2 ? eps[0] : 0.0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        float u0 = 1.0f, u1 = 0.0f;
        if (draw) {
            const uint64_t ctr = base + (uint64_t)r;
            uint32_t x[4];
            philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, DQN_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            u0 = (float)(x[0] >> 8) * (1.0f / 16777216.0f);
            u1 = (float)(x[1] >> 8) * (1.0f / 16777216.0f);
        } else if (mode != 0) {
            const float2 t = *reinterpret_cast<const float2 *>(u_in + r * 2);
            u0 = t.x;
            u1 = t.y;
        }
        const bool explore = all_explore || (mode == 2 && (double)u0 < e);
        int a;
        if (explore) {
            a = (int)floorf(fminf(fmaxf(u1 * (float)M, 0.0f), (float)(M - 1)));  // min(floor(u M), M - 1); a NaN gives 0
        } else {
            float best;
            a = row_argmax(q + r * ldq, M, best);
        }
        float2 v;
        v.x = valve_of(a / K, K);
        v.y = valve_of(a % K, K);
        *reinterpret_cast<float2 *>(valve_out + r * 2) = v;
        if (index_out) index_out[r] = (int64_t)a;
    }
    if (draw && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0) rng_ctl[1] = base + (uint64_t)n;
}

// dqn.py:195-212
__global__ __launch_bounds__(256) void dqn_loss_kernel(const float *__restrict__ q, const int64_t ldq, const float *__restrict__ next_q,
                                                       const int64_t ldn, const float *__restrict__ valve, const float *__restrict__ reward,
                                                       const float *__restrict__ done, const float gamma, const int64_t B, const int M,
                                                       const int K, float *__restrict__ g_q, float *__restrict__ loss_out,
                                                       float *__restrict__ loss_sum, float *__restrict__ cur_q_out,
                                                       float *__restrict__ target_out, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[1];
    const float fB = (float)B;
    double acc[1] = {0.0};
    for (int64_t b = blockIdx.x * 256ll + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256ll) {
        float best;
        row_argmax(next_q + b * ldn, M, best);                      // next_q_values.max(dim=1)
        const float target = reward[b] + ((1.0f - done[b]) * gamma) * best;
        const float2 v = *reinterpret_cast<const float2 *>(valve + b * 2);
        const int a = level_of(v.x, K) * K + level_of(v.y, K);     // in [0, M) by construction
        const float cur = q[b * ldq + a];                           // th.gather(current_q_values, 1, actions)
        const float d = cur - target, z = fabsf(d);
        acc[0] += (double)(z < 1.0f ? (0.5f * z) * z : z - 0.5f);      // smooth_l1_loss, beta = 1 (a NaN takes the second branch)
        float *g = g_q + b * ldq;
        for (int c = 0; c < M; ++c) g[c] = 0.0f;
        g[a] = d != d ? d : fminf(fmaxf(d, -1.0f), 1.0f) / fB;      // d smooth_l1 / d cur = clamp(d, -1, 1), mean over B; a NaN stays one
        if (cur_q_out) cur_q_out[b] = cur;
        if (target_out) target_out[b] = target;
    }
    if (!reduce_partials<1, 1u, 1>(acc, red, ws, tot)) return;
    if (threadIdx.x == 0) {
        const float loss = (float)(tot[0] / (double)B);
        loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
    }
}

inline int face_check(int n_actions, int levels)
{
    return (levels < 2 || levels > CSTR_DQN_MAX_LEVELS || n_actions != levels * levels) ? CSTR_E_UNSUPPORTED : 0;
}

}  // namespace

extern "C" int cstr_mt19937_rand_flag_f64(uint32_t *mt_state, const double *threshold, int32_t *flag_out, double *draw_out,
                                          cstr_stream_t stream)
{
    if (!mt_state || !threshold || !flag_out) return CSTR_E_BADARG;
    if (!aligned4(mt_state) || !aligned8(threshold) || !aligned4(flag_out) || (draw_out && !aligned8(draw_out))) return CSTR_E_BADARG;
    if (overlap(mt_state, CSTR_MT_STATE_WORDS, threshold, 2) || overlap(mt_state, CSTR_MT_STATE_WORDS, flag_out, 1) ||
        overlap(threshold, 2, flag_out, 1) ||
        (draw_out && (overlap(mt_state, CSTR_MT_STATE_WORDS, draw_out, 2) || overlap(threshold, 2, draw_out, 2) || overlap(flag_out, 1, draw_out, 2))))
        return CSTR_E_BADARG;
    rand_flag_kernel<<<1, 64, 0, (hipStream_t)stream>>>(mt_state, threshold, flag_out, draw_out);
    return (int)hipGetLastError();
}

extern "C" int cstr_dqn_act_f32(const float *q, int64_t ldq, int64_t n, int n_actions, int levels, int mode, const double *eps,
                                const int32_t *flag, const float *u_in, uint64_t *rng_ctl, float *valve_out, int64_t *index_out,
                                cstr_stream_t stream)
{
    if (!q || !valve_out || n <= 0 || n_actions <= 0 || levels <= 0 || ldq < n_actions) return CSTR_E_BADARG;
    if (mode < 0 || mode > 2) return CSTR_E_BADARG;
    if (mode == 1 && !flag) return CSTR_E_BADARG;
    if (mode == 2 && !eps) return CSTR_E_BADARG;
    if (mode != 0 && (u_in == nullptr) == (rng_ctl == nullptr)) return CSTR_E_BADARG;  // exactly one source of uniforms
    const int rc = face_check(n_actions, levels);
    if (rc) return rc;
    if (n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (mode == 0) { eps = nullptr; flag = nullptr; u_in = nullptr; rng_ctl = nullptr; }
    if (mode == 1) eps = nullptr;
    if (mode == 2) flag = nullptr;
    if (!aligned4(q) || !aligned8(valve_out) || (index_out && !aligned8(index_out)) || (eps && !aligned8(eps)) || (flag && !aligned4(flag)) ||
        (u_in && !aligned8(u_in)) || (rng_ctl && !aligned8(rng_ctl)))
        return CSTR_E_BADARG;
    {
        const Buf ins[4] = {{q, span(n, ldq, n_actions)}, {eps, 2}, {flag, 1}, {u_in, 2 * n}};
        const Buf outs[3] = {{valve_out, 2 * n}, {index_out, 2 * n}, {rng_ctl, 2 * CSTR_RNG_CTL_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    dqn_act_kernel<<<lane_grid(n, 64, 4096), 64, 0, (hipStream_t)stream>>>(q, ldq, n, n_actions, levels, mode, eps, flag, u_in, rng_ctl,
                                                                          valve_out, index_out);
    return (int)hipGetLastError();
}

extern "C" int cstr_dqn_loss_f32(const float *q, int64_t ldq, const float *next_q, int64_t ldn, const float *valve, const float *reward,
                                 const float *done, float gamma, int64_t batch, int n_actions, int levels, float *g_q, float *loss_out,
                                 float *loss_sum, float *cur_q_out, float *target_out, uint64_t *workspace, cstr_stream_t stream)
{
    if (!q || !next_q || !valve || !reward || !done || !g_q || !loss_out || !workspace || batch <= 0 || n_actions <= 0 || levels <= 0 ||
        ldq < n_actions || ldn < n_actions || gamma != gamma)
        return CSTR_E_BADARG;
    const int rc = face_check(n_actions, levels);
    if (rc) return rc;
    if (batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!aligned4(q) || !aligned4(next_q) || !aligned8(valve) || !aligned4(reward) || !aligned4(done) || !aligned4(g_q) || !aligned4(loss_out) ||
        (loss_sum && !aligned4(loss_sum)) || (cur_q_out && !aligned4(cur_q_out)) || (target_out && !aligned4(target_out)) ||
        !aligned8(workspace))
        return CSTR_E_BADARG;
    {
        const int64_t B = batch;
        const Buf ins[5] = {{q, span(B, ldq, n_actions)}, {next_q, span(B, ldn, n_actions)}, {valve, 2 * B}, {reward, B}, {done, B}};
        const Buf outs[6] = {{g_q, span(B, ldq, n_actions)}, {loss_out, 1}, {loss_sum, 1}, {cur_q_out, B}, {target_out, B},
                             {workspace, 2 * CSTR_PPO_WS_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    const unsigned grid = lane_grid(batch, 256, CSTR_PPO_MAX_BLOCKS);
    dqn_loss_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(q, ldq, next_q, ldn, valve, reward, done, gamma, batch, n_actions, levels, g_q,
                                                          loss_out, loss_sum, cur_q_out, target_out,
                                                          reinterpret_cast<unsigned long long *>(workspace));
    return (int)hipGetLastError();
}
