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
// Batch reductions (the convention of cstr_ppo.hip): lane 0 of every wave sums its rows in f64, a fixed LDS tree per workgroup, the
// partials are published and the workgroup that draws the last ticket sums them in workgroup order. No float atomics; the grid is
// a function of the row count alone.
// Entropy: H = -sum_j p_j * max(logp_j, -FLT_MAX) (torch clamps the logits to the least finite value, so p = 0 contributes 0).
// NaN: fminf / fmaxf in the clips DROP a NaN operand where torch.min / clamp propagate it (as in cstr_ppo.hip).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t CAT_STREAM_TAG = 0xCA7A11C7u;  // counter word 3: never shares counters with the other heads' streams
constexpr int CAT_PARTS = 8;       // the stride of cstr_ppo_loss_f32's partials
constexpr int CAT_USED = 5;        // policy sum, value sum, kl sum, clipped count, entropy sum
constexpr int ROWS_PER_BLOCK = 4;  // one wave per row
constexpr int ACT_MAX_BLOCKS = 256;

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// xor butterfly: both partners form the same commutative sum at every level, so every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float wave_inclusive_scan(float v, const int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

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
    m = wave_max(m);
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += expf(z[c] - m);
    const float lse = logf(wave_sum(s));
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        const bool greater = ov > bv || (ov != ov && bv == bv);
        const bool tie = ov == bv || (ov != ov && bv != bv);
        if (greater || (tie && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi < M ? bi : M - 1;
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
            const int64_t t = action_in[r];
            a = t < 0 ? 0 : (t >= M ? M - 1 : (int)t);
        } else {
            if (draw) {
                const uint64_t ctr = base + (uint64_t)r;
                uint32_t x[4];
                philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, CAT_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), x);
                u = (float)(x[0] >> 8) * (1.0f / 16777216.0f);
            } else {
                u = u_in[r];
            }
            a = M - 1;
            bool found = false;
            float carry = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float cum = carry + wave_inclusive_scan(expf(lp[c]), lane);
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

// ppo.py:213-264 (objective 0: ppo_loss_kernel's statements on the Categorical log-prob) / a2c.py:150-171 (objective 1)
template <int C>
__global__ __launch_bounds__(256) void categorical_loss_kernel(const cstr_categorical_loss_t p, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[CAT_USED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = p.batch;
    const int M = p.n_actions;
    const bool ppo = p.objective == 0;
    // advantage statistics over the whole minibatch: every workgroup computes them itself, in the same order. PPO skips them for a
    // single row (ppo.py:217); A2C has no such guard (a2c.py:155-156): one row gives 0 / 0 = NaN
    const bool norm = p.normalize_advantage && (!ppo || B > 1);
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
        a_den = (float)sqrt(block_sum_f64(q, red) / (double)(B - 1)) + 1e-8f;  // unbiased std
    }
    const float lo = (float)(1.0 - p.clip_range), hi = (float)(1.0 + p.clip_range), cr = (float)p.clip_range;
    const bool vclip = ppo && p.clip_range_vf > 0.0;
    const float cv = (float)p.clip_range_vf;
    const float inv_b = 1.0f / (float)B;
    const float ec_b = p.ent_coef * inv_b;
    double acc[CAT_USED] = {0.0, 0.0, 0.0, 0.0, 0.0};
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
        const float H = -wave_sum(hs);
        const float af = p.actions[b];  // rollout_data.actions.long().flatten(); outside the face: the caller's bug, clamped
        const int a = af >= 0.0f ? (af < (float)M ? (int)af : M - 1) : 0;
        const float logp = row_element<C>(lp, a);
        const float advn = norm ? (p.adv[b] - a_mean) / a_den : p.adv[b];
        float g_logp;
        double part0, part2 = 0.0, part3 = 0.0;
        if (ppo) {
            const float lr = logp - p.old_log_prob[b];
            const float ratio = expf(lr);
            const float pl1 = advn * ratio, pl2 = advn * fminf(fmaxf(ratio, lo), hi);
            part0 = (double)fminf(pl1, pl2);
            part2 = (double)((ratio - 1.0f) - lr);
            part3 = fabsf(ratio - 1.0f) > cr ? 1.0 : 0.0;
            // d min(pl1, pl2) / d ratio: the closed-interval rule of ppo_loss_kernel
            const float dmin = ((ratio >= lo && ratio <= hi) || pl1 < pl2) ? advn : 0.0f;
            g_logp = -(inv_b * dmin) * ratio;
        } else {
            part0 = (double)(advn * logp);
            g_logp = -(inv_b * advn);  // d(-mean(adv * log_prob)) / d log_prob
        }
        float *g = p.g_logits + b * p.ldz;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = lane + 64 * c;
            if (j < M) g[j] = g_logp * ((j == a ? 1.0f : 0.0f) - pr[c]) + ec_b * (pr[c] * (lp[c] + H));
        }
        if (lane == 0) {
            if (p.log_prob_out) p.log_prob_out[b] = logp;
            const float v = p.values[b], ret = p.returns[b];
            float vp = v;
            bool pass = true;
            if (vclip) {
                const float vo = p.old_values[b], dv = v - vo;
                vp = vo + fminf(fmaxf(dv, -cv), cv);
                pass = dv >= -cv && dv <= cv;
            }
            const float dr = ret - vp;
            p.g_value[b] = pass ? p.vf_coef * ((2.0f * inv_b) * (vp - ret)) : 0.0f;
            acc[0] += part0;
            acc[1] += (double)(dr * dr);
            acc[2] += part2;
            acc[3] += part3;
            acc[4] += (double)H;
        }
    }
#pragma unroll
    for (int k = 0; k < CAT_USED; ++k) {
        const double s = block_sum_f64(acc[k], red);
        if (threadIdx.x == 0) publish_f64(ws + WS_PART0 + (int64_t)blockIdx.x * CAT_PARTS + k, s);
    }
    __threadfence();  // release: the partials are visible chip-wide before this workgroup's ticket is
    if (!last_block_ticket(ws)) return;
    __threadfence();  // acquire: behind the last ticket every workgroup's partials are read from memory
    if (threadIdx.x < CAT_USED) {
        double s = 0.0;
        for (unsigned j = 0; j < gridDim.x; ++j) s += consume_f64(ws + WS_PART0 + (int64_t)j * CAT_PARTS + threadIdx.x);
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float out[6];
        out[0] = -(float)(tot[0] / (double)B);  // policy_gradient_loss / policy_loss
        out[1] = (float)(tot[1] / (double)B);   // value_loss
        out[2] = -(float)(tot[4] / (double)B);  // entropy_loss = -mean(entropy)
        out[3] = (out[0] + p.ent_coef * out[2]) + p.vf_coef * out[1];  // loss
        out[4] = (float)(tot[2] / (double)B);   // approx_kl (PPO)
        out[5] = (float)(tot[3] / (double)B);   // clip_fraction (PPO)
        const int n_out = ppo ? 6 : 4;
        for (int k = 0; k < n_out; ++k) {
            if (p.scalars_out) p.scalars_out[k] = out[k];
            if (p.scalars_sum) p.scalars_sum[k] += out[k];
        }
    }
}

inline int face_check(int n_actions, int levels)
{
    return (levels < 2 || levels > CSTR_DQN_MAX_LEVELS || n_actions != levels * levels) ? CSTR_E_UNSUPPORTED : 0;
}

// floats spanned by `rows` rows of `width` floats with row stride ld
inline int64_t span(int64_t rows, int64_t ld, int64_t width) { return (rows - 1) * ld + width; }

inline unsigned row_grid(int64_t rows, int64_t cap) { return lane_grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, 1, cap); }

}  // namespace

extern "C" int cstr_categorical_act_f32(const float *logits, int64_t ldz, int64_t n, int n_actions, int levels, int deterministic,
                                        const int64_t *action_in, const float *u_in, uint64_t *rng_ctl, float *index_f32, int64_t *index_out,
                                        float *valve_out, float *log_prob, float *u_out, cstr_stream_t stream)
{
    if (!logits || !index_f32 || n <= 0 || n_actions <= 0 || levels <= 0 || ldz < n_actions) return CSTR_E_BADARG;
    const int sources = (deterministic != 0) + (action_in != nullptr) + (u_in != nullptr) + (rng_ctl != nullptr);
    if (sources != 1) return CSTR_E_BADARG;  // the index comes from exactly one source
    if (u_out && !u_in && !rng_ctl) return CSTR_E_BADARG;  // no uniform to keep
    const int rc = face_check(n_actions, levels);
    if (rc) return rc;
    if (n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!aligned4(logits) || !aligned4(index_f32) || (index_out && !aligned8(index_out)) || (valve_out && !aligned8(valve_out)) ||
        (log_prob && !aligned4(log_prob)) || (u_out && !aligned4(u_out)) || (action_in && !aligned8(action_in)) || (u_in && !aligned4(u_in)) ||
        (rng_ctl && !aligned8(rng_ctl)))
        return CSTR_E_BADARG;
    {
        const void *ins[4] = {logits, action_in, u_in, rng_ctl};
        const int64_t in_n[4] = {span(n, ldz, n_actions), 2 * n, n, 2 * CSTR_RNG_CTL_WORDS};
        const void *outs[5] = {index_f32, index_out, valve_out, log_prob, u_out};
        const int64_t out_n[5] = {n, 2 * n, 2 * n, n, n};
        for (int o = 0; o < 5; ++o) {
            if (!outs[o]) continue;
            for (int i = 0; i < 4; ++i)
                if (ins[i] && overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
            for (int q = o + 1; q < 5; ++q)
                if (outs[q] && overlap(outs[o], out_n[o], outs[q], out_n[q])) return CSTR_E_BADARG;
        }
        if (rng_ctl && overlap(rng_ctl, 2 * CSTR_RNG_CTL_WORDS, logits, in_n[0])) return CSTR_E_BADARG;
    }
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
    if (!p || !workspace || !p->logits || !p->actions || !p->values || !p->adv || !p->returns || !p->g_logits || !p->g_value ||
        p->batch <= 0 || p->n_actions <= 0 || p->levels <= 0 || p->ldz < p->n_actions)
        return CSTR_E_BADARG;
    if (p->objective != 0 && p->objective != 1) return CSTR_E_BADARG;
    const bool ppo = p->objective == 0;
    if (ppo && (!p->old_log_prob || !(p->clip_range >= 0.0) || (p->clip_range_vf > 0.0 && !p->old_values))) return CSTR_E_BADARG;
    const int rc = face_check(p->n_actions, p->levels);
    if (rc) return rc;
    if (p->batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    const float *old_values = ppo && p->clip_range_vf > 0.0 ? p->old_values : nullptr;  // read only by the value clip
    const float *old_log_prob = ppo ? p->old_log_prob : nullptr;
    if (!aligned8(workspace) || !aligned4(p->logits) || !aligned4(p->actions) || !aligned4(p->values) || !aligned4(p->adv) ||
        !aligned4(p->returns) || !aligned4(p->g_logits) || !aligned4(p->g_value) || (old_values && !aligned4(old_values)) ||
        (old_log_prob && !aligned4(old_log_prob)) || (p->scalars_out && !aligned4(p->scalars_out)) ||
        (p->scalars_sum && !aligned4(p->scalars_sum)) || (p->log_prob_out && !aligned4(p->log_prob_out)))
        return CSTR_E_BADARG;
    {
        const int64_t B = p->batch, zs = span(B, p->ldz, p->n_actions), ns = ppo ? 6 : 4;
        const void *ins[7] = {p->logits, p->actions, p->values, old_values, old_log_prob, p->adv, p->returns};
        const int64_t in_n[7] = {zs, B, B, B, B, B, B};
        const void *outs[6] = {p->g_logits, p->g_value, p->scalars_out, p->scalars_sum, p->log_prob_out, workspace};
        const int64_t out_n[6] = {zs, B, ns, ns, B, 2 * CSTR_PPO_WS_WORDS};
        for (int o = 0; o < 6; ++o) {
            if (!outs[o]) continue;
            for (int i = 0; i < 7; ++i)
                if (ins[i] && overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
            for (int q = o + 1; q < 6; ++q)
                if (outs[q] && overlap(outs[o], out_n[o], outs[q], out_n[q])) return CSTR_E_BADARG;
        }
    }
    cstr_categorical_loss_t k = *p;
    k.old_values = old_values;
    k.old_log_prob = old_log_prob;
    const unsigned grid = row_grid(p->batch, CSTR_PPO_MAX_BLOCKS);
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(workspace);
    const int chunks = (p->n_actions + 63) / 64;
    if (chunks == 1) categorical_loss_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    else if (chunks == 2) categorical_loss_kernel<2><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    else if (chunks == 3) categorical_loss_kernel<3><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    else categorical_loss_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(k, ws);
    return (int)hipGetLastError();
}
