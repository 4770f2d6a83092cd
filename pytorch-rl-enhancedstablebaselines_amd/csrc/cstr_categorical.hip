// cstr_categorical.hip -- the Categorical action head of PPO and A2C on the discrete valve face (reference
// core/common/distributions.py:263-311 CategoricalDistribution = torch's Categorical(logits=z), core/ppo/ppo.py:213-264,
// core/a2c/a2c.py:150-171), f32, gfx950:
//   * the rollout / predict head in ONE launch: logp = z - logsumexp(z), the index (first maximum, a teacher-forced index, or the
//     inverse CDF of a given or drawn uniform), its log-prob and the normalised valve pair the env steps with;
//   * everything between evaluate_actions' outputs and loss.backward() in ONE launch for both algorithms (`objective`): the stored
//     action's log-prob, the row entropy, PPO's clipped surrogate or A2C's policy-gradient loss, the value loss, the logged scalars
//     and the gradients w.r.t. the logits and the value.
// Shape: ONE WAVE PER ROW. Lane l holds logits l, l + 64, l + 128, l + 192 (the kernels are instantiated on ceil(n_actions / 64), so
// a face of at most 64 indices carries one register per lane); the row maximum, the sum of exponentials, the entropy and the
// argmax go through xor butterflies, the cumulative probabilities through a shuffle scan per 64-index chunk plus a carry, the first
// index past the uniform through a ballot. No LDS round trip per row. A 256-thread workgroup holds four rows and grid-strides.
// Statement: m = max_j z_j; logp_j = (z_j - m) - logf(sum_j expf(z_j - m)); p_j = expf(logp_j) (log_softmax, then exp, as torch's
// Categorical does). The butterfly sums every lane's partial in a fixed tree: a row always reduces the same way.
// The deterministic index is the first maximum of the LOGITS. The reference takes argmax(probs): the two differ only where two
// distinct logits round to the same probability (there the reference takes the earlier index, this kernel the larger logit). A NaN
// counts as the greatest value, the first one wins (cstr_dqn_act_f32's rule).
// Sampling: a = the first index whose inclusive cumulative probability (f32, index order) exceeds u, n_actions - 1 if none does
// (rounding can leave the total below u; a NaN anywhere also ends there). Uniforms are READ when given and DRAWN otherwise:
// Philox4x32-10 keyed by rng_ctl[0], counter (rng_ctl[1] + row, 0, Categorical tag), word 0 as (word >> 8) * 2^-24 in [0, 1); the
// last workgroup advances rng_ctl[1] by the row count. torch's multinomial stream is not reproduced: parity with the reference is
// teacher-forced through action_in.
// Batch reductions: lane 0 of every wave sums its rows in f64; from there the convention at the top of cstr_onpolicy_device.h.
// Entropy: H = -sum_j p_j * max(logp_j, -FLT_MAX) (torch clamps the logits to the least finite value, so p = 0 contributes 0).
// NaN: the loss launch propagates a NaN log-prob, advantage or value as torch.min / clamp do (stated in cstr_ppo.hip's header).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_discrete_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t CAT_STREAM_TAG = 0xCA7A11C7u;  // counter word 3: never shares counters with the other heads' streams

template <int C> __device__ __forceinline__ void load_logits(const float *__restrict__ row, const int M, const int lane, float (&z)[C])
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = lane + 64 * c;
        z[c] = j < M ? row[j] : -INFINITY;  // a padded lane: probability 0, never a maximum before a real index
    }
}

// logp_j = (z_j - m) - log(sum_j exp(z_j - m))
template <int C> __device__ __forceinline__ void row_log_softmax(const float (&z)[C], float (&lp)[C])
{
    float m = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
    m = seg_max<64>(m);
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += expf(z[c] - m);
    const float lse = logf(seg_sum<64>(s));
#pragma unroll
    for (int c = 0; c < C; ++c) lp[c] = (z[c] - m) - lse;
}

// first maximum of the row over the wave; a NaN is the greatest value, the first one wins
template <int C> __device__ __forceinline__ int row_argmax(const float (&z)[C], const int M, const int lane)
{
    float bv = z[0];
    int bi = lane;
#pragma unroll
    for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (v > bv || (v != v && bv == bv)) { bv = v; bi = lane + 64 * c; }
    }
    return seg_argmax<64>(bv, bi, M);
}

// element `a` of a row held as lane + 64 c
template <int C> __device__ __forceinline__ float row_element(const float (&v)[C], const int a)
{
    float sel = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c)
        if ((a >> 6) == c) sel = v[c];
    return __shfl(sel, a & 63);
}

template <int C>
__global__ __launch_bounds__(256) void categorical_act_kernel(const float *__restrict__ logits, const int64_t ldz, const int64_t n, const int M,
                                                              const int K, const int deterministic, const int64_t *__restrict__ action_in,
                                                              const float *__restrict__ u_in, uint64_t *__restrict__ rng_ctl,
                                                              float *__restrict__ index_f32, int64_t *__restrict__ index_out,
                                                              float *__restrict__ valve_out, float *__restrict__ log_prob,
                                                              float *__restrict__ u_out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool draw = rng_ctl != nullptr;
    const bool sample = draw || u_in != nullptr;
    const uint64_t seed = draw ? rng_ctl[0] : 0ull, base = draw ? rng_ctl[1] : 0ull;
    for (int64_t r = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; r < n; r += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        float z[C], lp[C];
        load_logits<C>(logits + r * ldz, M, lane, z);
        if (sample || log_prob) row_log_softmax<C>(z, lp);
        int a;
        float u = 0.0f;
        if (deterministic) {
            a = row_argmax<C>(z, M, lane);
        } else if (action_in) {
            a = clamp_level(action_in[r], M);
        } else {
            if (draw) {
                uint32_t x[4];
                philox_row(seed, base + (uint64_t)r, CAT_STREAM_TAG, x);
                u = philox_uniform(x[0]);
            } else {
                u = u_in[r];
            }
            a = M - 1;
            bool found = false;
            float carry = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float cum = carry + seg_inclusive_scan<64>(expf(lp[c]), lane);
                const unsigned long long hit = __ballot(lane + 64 * c < M && cum > u);
                if (!found && hit != 0ull) {
                    a = 64 * c + (__ffsll((long long)hit) - 1);
                    found = true;
                }
                carry = __shfl(cum, 63);
            }
        }
        const float la = log_prob ? row_element<C>(lp, a) : 0.0f;
        if (lane == 0) {
            index_f32[r] = (float)a;
            if (index_out) index_out[r] = (int64_t)a;
            if (valve_out) {
                float2 v;
                v.x = valve_of(a / K, K);
                v.y = valve_of(a % K, K);
                *reinterpret_cast<float2 *>(valve_out + r * 2) = v;
            }
            if (log_prob) log_prob[r] = la;
            if (u_out) u_out[r] = u;
        }
    }
    if (draw && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0) rng_ctl[1] = base + (uint64_t)n;
}

// ppo.py:213-264 (objective 0) / a2c.py:150-171 (objective 1) on the Categorical log-prob and entropy
template <int C>
__global__ __launch_bounds__(256) void categorical_loss_kernel(const cstr_categorical_loss_t p, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[DISCRETE_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = p.batch;
    const int M = p.n_actions;
    DiscreteLoss<cstr_categorical_loss_t> core(p, red);
    for (int64_t b = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; b < B; b += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        float z[C], lp[C], pr[C];
        load_logits<C>(p.logits + b * p.ldz, M, lane, z);
        row_log_softmax<C>(z, lp);
        float hs = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            pr[c] = expf(lp[c]);
            lp[c] = fmaxf(lp[c], -FLT_MAX);  // torch's Categorical.entropy clamps the logits; logp_a below is never -inf * 0
            hs += pr[c] * lp[c];
        }
        const float H = -seg_sum<64>(hs);
        const int a = stored_level(p.actions[b], M);
        const float logp = row_element<C>(lp, a);
        const PolicyTerm pt = core.policy(b, logp);
        float *g = p.g_logits + b * p.ldz;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = lane + 64 * c;
            if (j < M) g[j] = pt.g_logp * ((j == a ? 1.0f : 0.0f) - pr[c]) + core.ec_b * (pr[c] * (lp[c] + H));
        }
        if (lane == 0) core.row_done(b, logp, H, pt);
    }
    core.finish(red, ws, tot);
}

inline int face_check(int n_actions, int levels)
{
    return (levels < 2 || levels > CSTR_DQN_MAX_LEVELS || n_actions != levels * levels) ? CSTR_E_UNSUPPORTED : 0;
}

}  // namespace

extern "C" int cstr_categorical_act_f32(const float *logits, int64_t ldz, int64_t n, int n_actions, int levels, int deterministic,
                                        const int64_t *action_in, const float *u_in, uint64_t *rng_ctl, float *index_f32, int64_t *index_out,
                                        float *valve_out, float *log_prob, float *u_out, cstr_stream_t stream)
{
    if (!logits || !index_f32 || n <= 0 || n_actions <= 0 || levels <= 0 || ldz < n_actions) return CSTR_E_BADARG;
    if (!act_sources_ok(deterministic, action_in, u_in, rng_ctl, u_out)) return CSTR_E_BADARG;
    const int rc = face_check(n_actions, levels);
    if (rc) return rc;
    if (n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!act_buffers_ok(1, logits, span(n, ldz, n_actions), n, action_in, u_in, rng_ctl, index_f32, index_out, valve_out, log_prob, u_out))
        return CSTR_E_BADARG;
    const unsigned grid = row_grid(n, ACT_MAX_BLOCKS);
    const int chunks = (n_actions + 63) / 64;
#define ACT_LAUNCH(C)                                                                                                                     \
    categorical_act_kernel<C><<<grid, 256, 0, (hipStream_t)stream>>>(logits, ldz, n, n_actions, levels, deterministic, action_in, u_in, rng_ctl, \
                                                                    index_f32, index_out, valve_out, log_prob, u_out)
    if (chunks == 1) ACT_LAUNCH(1);
    else if (chunks == 2) ACT_LAUNCH(2);
    else if (chunks == 3) ACT_LAUNCH(3);
    else ACT_LAUNCH(4);
#undef ACT_LAUNCH
    return (int)hipGetLastError();
}

extern "C" int cstr_categorical_loss_f32(const cstr_categorical_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p || !p->logits || !p->actions || !p->g_logits || p->n_actions <= 0 || p->levels <= 0 || p->ldz < p->n_actions) return CSTR_E_BADARG;
    if (p->objective != 0 && p->objective != 1) return CSTR_E_BADARG;
    cstr_categorical_loss_t k = *p;
    const LossCommon c = discrete_loss_common(k, workspace);  // nulls what the objective does not read
    const int rc = loss_common_check(c, face_check(p->n_actions, p->levels));
    if (rc) return rc;
    if (!aligned4(p->logits) || !aligned4(p->actions) || !aligned4(p->g_logits)) return CSTR_E_BADARG;
    const int64_t B = p->batch, zs = span(B, p->ldz, p->n_actions);
    const Buf ins[2] = {{p->logits, zs}, {p->actions, B}};
    const Buf outs[1] = {{p->g_logits, zs}};
    if (loss_outputs_overlap(c, ins, outs)) return CSTR_E_BADARG;
    const unsigned grid = row_grid(B, CSTR_PPO_MAX_BLOCKS);
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(workspace);
    const int chunks = (p->n_actions + 63) / 64;
    if (chunks == 1) categorical_loss_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    else if (chunks == 2) categorical_loss_kernel<2><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    else if (chunks == 3) categorical_loss_kernel<3><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    else categorical_loss_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    return (int)hipGetLastError();
}
