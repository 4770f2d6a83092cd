// cstr_multicategorical.hip -- the MultiCategorical action head of PPO and A2C on the MultiDiscrete valve face (reference
// core/common/distributions.py:314-368 MultiCategoricalDistribution = one torch Categorical per th.split of the logits,
// core/ppo/ppo.py:213-264, core/a2c/a2c.py:150-171), f32, gfx950:
//   * the rollout / predict head in ONE launch: per valve logp = z - logsumexp(z), the level pair (first maxima, a teacher-forced
//     pair, or the inverse CDFs of two given or drawn uniforms), the pair's log-prob and the normalised valve pair the env steps with;
//   * everything between evaluate_actions' outputs and loss.backward() in ONE launch for both algorithms (`objective`).
// Layout: logits [rows][ldz]; columns 0 .. K0-1 are valve 0's, K0 .. K0+K1-1 valve 1's (th.split order), 2 <= K_g <= 32.
// Shape: ONE WAVE PER ROW, BOTH VALVES AT ONCE. Lanes 0-31 hold valve 0, lanes 32-63 valve 1 (lane & 31 = the level, padded lanes
// hold -inf: probability 0, never a maximum before a real level). Maxima, sums of exponentials, entropies and argmaxes go through xor
// butterflies with offsets 16 .. 1, which never cross the half; the cumulative probabilities through a width-32 shuffle scan; the
// first level past the uniform through one ballot, split into its two halves. No LDS round trip per row. A 256-thread workgroup
// holds four rows and grid-strides. The butterfly sums every lane's partial in a fixed tree: a row always reduces the same way.
// Statement per valve g (cstr_categorical.hip's): m_g = max_j z_j; logp_j = (z_j - m_g) - logf(sum_j expf(z_j - m_g));
// p_j = expf(logp_j); H_g = -sum_j p_j * max(logp_j, -FLT_MAX). Row: logp = logp_0[a_0] + logp_1[a_1], H = H_0 + H_1.
// The deterministic level is the first maximum of the valve's LOGITS; a NaN counts as the greatest value, the first one wins.
// Sampling: a_g = the first level whose inclusive cumulative probability (f32, index order) exceeds u_g, K_g - 1 if none does.
// Uniforms are READ when given and DRAWN otherwise: Philox4x32-10 keyed by rng_ctl[0], counter (rng_ctl[1] + row, 0, tag), words 0
// and 1 of the one block as (word >> 8) * 2^-24 for valves 0 and 1; the last workgroup advances rng_ctl[1] by the row count.
// Batch reductions (the convention of cstr_ppo.hip): lane 0 of every wave sums its rows in f64, a fixed LDS tree per workgroup, the
// partials are published and the workgroup that draws the last ticket sums them in workgroup order. No float atomics.
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

constexpr uint32_t MCAT_STREAM_TAG = 0x3CA7A11Cu;  // counter word 3: never shares counters with the other heads' streams
constexpr int MCAT_PARTS = 8;      // the stride of cstr_ppo_loss_f32's partials
constexpr int MCAT_USED = 5;       // policy sum, value sum, kl sum, clipped count, entropy sum
constexpr int ROWS_PER_BLOCK = 4;  // one wave per row
constexpr int ACT_MAX_BLOCKS = 256;

__device__ __forceinline__ float half_max(float v)
{
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// xor butterfly inside the 32-lane half: both partners form the same commutative sum at every level
__device__ __forceinline__ float half_sum(float v)
{
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float half_inclusive_scan(float v, const int j)
{
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const float t = __shfl_up(v, o, 32);
        if (j >= o) v += t;
    }
    return v;
}

// the lane's logit: level j of its valve, -inf on a padded lane
__device__ __forceinline__ float load_logit(const float *__restrict__ row, const int col, const bool valid) { return valid ? row[col] : -INFINITY; }

// logp_j = (z_j - m_g) - log(sum_j exp(z_j - m_g)) over the lane's half
__device__ __forceinline__ float half_log_softmax(const float z)
{
    const float m = half_max(z);
    const float lse = logf(half_sum(expf(z - m)));
    return (z - m) - lse;
}

// first maximum of the lane's half; a NaN is the greatest value, the first one wins
__device__ __forceinline__ int half_argmax(const float z, const int j, const int K)
{
    float bv = z;
    int bi = j;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        const bool greater = ov > bv || (ov != ov && bv == bv);
        const bool tie = ov == bv || (ov != ov && bv != bv);
        if (greater || (tie && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi < K ? bi : K - 1;
}

__device__ __forceinline__ int clamp_level(const int64_t t, const int K) { return t < 0 ? 0 : (t >= K ? K - 1 : (int)t); }

__global__ __launch_bounds__(256) void multicategorical_act_kernel(const float *__restrict__ logits, const int64_t ldz, const int64_t n,
                                                                   const int K0, const int K1, const int deterministic,
                                                                   const int64_t *__restrict__ action_in, const float *__restrict__ u_in,
                                                                   uint64_t *__restrict__ rng_ctl, float *__restrict__ action_f32,
                                                                   int64_t *__restrict__ action_out, float *__restrict__ valve_out,
                                                                   float *__restrict__ log_prob, float *__restrict__ u_out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31;
    const int K = half ? K1 : K0, col = half ? K0 + j : j;
    const bool valid = j < K;
    const bool draw = rng_ctl != nullptr;
    const bool sample = draw || u_in != nullptr;
    const uint64_t seed = draw ? rng_ctl[0] : 0ull, base = draw ? rng_ctl[1] : 0ull;
    for (int64_t r = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; r < n; r += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        const float z = load_logit(logits + r * ldz, col, valid);
        float lp = 0.0f;
        if (sample || log_prob) lp = half_log_softmax(z);
        int a0, a1;
        float u0 = 0.0f, u1 = 0.0f;
        if (deterministic) {
            const int a = half_argmax(z, j, K);
            a0 = __shfl(a, 0);
            a1 = __shfl(a, 32);
        } else if (action_in) {
            a0 = clamp_level(action_in[2 * r], K0);
            a1 = clamp_level(action_in[2 * r + 1], K1);
        } else {
            if (draw) {
                const uint64_t ctr = base + (uint64_t)r;
                uint32_t x[4];
                philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, MCAT_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), x);
                u0 = (float)(x[0] >> 8) * (1.0f / 16777216.0f);
                u1 = (float)(x[1] >> 8) * (1.0f / 16777216.0f);
            } else {
                const float2 t = *reinterpret_cast<const float2 *>(u_in + 2 * r);
                u0 = t.x;
                u1 = t.y;
            }
            const float cum = half_inclusive_scan(expf(lp), j);
            const unsigned long long hit = __ballot(valid && cum > (half ? u1 : u0));
            const unsigned h0 = (unsigned)(hit & 0xFFFFFFFFull), h1 = (unsigned)(hit >> 32);
            a0 = h0 ? __ffs((int)h0) - 1 : K0 - 1;
            a1 = h1 ? __ffs((int)h1) - 1 : K1 - 1;
        }
        float la = 0.0f;
        if (log_prob) la = __shfl(lp, a0) + __shfl(lp, 32 + a1);
        if (lane == 0) {
            float2 af;
            af.x = (float)a0;
            af.y = (float)a1;
            *reinterpret_cast<float2 *>(action_f32 + 2 * r) = af;
            if (action_out) {
                action_out[2 * r] = (int64_t)a0;
                action_out[2 * r + 1] = (int64_t)a1;
            }
            if (valve_out) {
                float2 v;
                v.x = valve_of(a0, K0);
                v.y = valve_of(a1, K1);
                *reinterpret_cast<float2 *>(valve_out + 2 * r) = v;
            }
            if (log_prob) log_prob[r] = la;
            if (u_out) {
                float2 uu;
                uu.x = u0;
                uu.y = u1;
                *reinterpret_cast<float2 *>(u_out + 2 * r) = uu;
            }
        }
    }
    if (draw && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0) rng_ctl[1] = base + (uint64_t)n;
}

// ppo.py:213-264 (objective 0) / a2c.py:150-171 (objective 1): categorical_loss_kernel's statements on the pair's log-prob and entropy
__global__ __launch_bounds__(256) void multicategorical_loss_kernel(const cstr_multicategorical_loss_t p, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[MCAT_USED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31;
    const int K0 = p.levels0, K1 = p.levels1;
    const int K = half ? K1 : K0, col = half ? K0 + j : j;
    const bool valid = j < K;
    const int64_t B = p.batch;
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
    double acc[MCAT_USED] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t b = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; b < B; b += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        const float z = load_logit(p.logits + b * p.ldz, col, valid);
        float lp = half_log_softmax(z);
        const float pr = expf(lp);
        lp = fmaxf(lp, -FLT_MAX);  // torch's Categorical.entropy clamps the logits; the pair's log-prob below is never -inf * 0
        const float Hg = -half_sum(pr * lp);  // this lane's valve
        const float H = __shfl(Hg, 0) + __shfl(Hg, 32);
        // rollout_data.actions.long(); a level outside the face: the caller's bug, clamped
        const float2 af = *reinterpret_cast<const float2 *>(p.actions + 2 * b);
        const int a0 = af.x >= 0.0f ? (af.x < (float)K0 ? (int)af.x : K0 - 1) : 0;
        const int a1 = af.y >= 0.0f ? (af.y < (float)K1 ? (int)af.y : K1 - 1) : 0;
        const float logp = __shfl(lp, a0) + __shfl(lp, 32 + a1);
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
        if (valid) {
            const int a = half ? a1 : a0;
            p.g_logits[b * p.ldz + col] = g_logp * ((j == a ? 1.0f : 0.0f) - pr) + ec_b * (pr * (lp + Hg));  // the valve's own entropy
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
    for (int k = 0; k < MCAT_USED; ++k) {
        const double s = block_sum_f64(acc[k], red);
        if (threadIdx.x == 0) publish_f64(ws + WS_PART0 + (int64_t)blockIdx.x * MCAT_PARTS + k, s);
    }
    __threadfence();  // release: the partials are visible chip-wide before this workgroup's ticket is
    if (!last_block_ticket(ws)) return;
    __threadfence();  // acquire: behind the last ticket every workgroup's partials are read from memory
    if (threadIdx.x < MCAT_USED) {
        double s = 0.0;
        for (unsigned k = 0; k < gridDim.x; ++k) s += consume_f64(ws + WS_PART0 + (int64_t)k * MCAT_PARTS + threadIdx.x);
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

inline int face_check(int levels0, int levels1)
{
    return (levels0 < 2 || levels0 > CSTR_MCAT_MAX_LEVELS || levels1 < 2 || levels1 > CSTR_MCAT_MAX_LEVELS) ? CSTR_E_UNSUPPORTED : 0;
}

// floats spanned by `rows` rows of `width` floats with row stride ld
inline int64_t span(int64_t rows, int64_t ld, int64_t width) { return (rows - 1) * ld + width; }

inline unsigned row_grid(int64_t rows, int64_t cap) { return lane_grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, 1, cap); }

}  // namespace

extern "C" int cstr_multicategorical_act_f32(const float *logits, int64_t ldz, int64_t n, int levels0, int levels1, int deterministic,
                                             const int64_t *action_in, const float *u_in, uint64_t *rng_ctl, float *action_f32,
                                             int64_t *action_out, float *valve_out, float *log_prob, float *u_out, cstr_stream_t stream)
{
    if (!logits || !action_f32 || n <= 0 || levels0 <= 0 || levels1 <= 0) return CSTR_E_BADARG;
    const int sources = (deterministic != 0) + (action_in != nullptr) + (u_in != nullptr) + (rng_ctl != nullptr);
    if (sources != 1) return CSTR_E_BADARG;  // the pair comes from exactly one source
    if (u_out && !u_in && !rng_ctl) return CSTR_E_BADARG;  // no uniforms to keep
    const int rc = face_check(levels0, levels1);
    if (rc) return rc;
    const int M = levels0 + levels1;
    if (ldz < M) return CSTR_E_BADARG;
    if (n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!aligned4(logits) || !aligned8(action_f32) || (action_out && !aligned8(action_out)) || (valve_out && !aligned8(valve_out)) ||
        (log_prob && !aligned4(log_prob)) || (u_out && !aligned8(u_out)) || (action_in && !aligned8(action_in)) || (u_in && !aligned8(u_in)) ||
        (rng_ctl && !aligned8(rng_ctl)))
        return CSTR_E_BADARG;
    {
        const void *ins[4] = {logits, action_in, u_in, rng_ctl};
        const int64_t in_n[4] = {span(n, ldz, M), 4 * n, 2 * n, 2 * CSTR_RNG_CTL_WORDS};
        const void *outs[5] = {action_f32, action_out, valve_out, log_prob, u_out};
        const int64_t out_n[5] = {2 * n, 4 * n, 2 * n, n, 2 * n};
        for (int o = 0; o < 5; ++o) {
            if (!outs[o]) continue;
            for (int i = 0; i < 4; ++i)
                if (ins[i] && overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
            for (int q = o + 1; q < 5; ++q)
                if (outs[q] && overlap(outs[o], out_n[o], outs[q], out_n[q])) return CSTR_E_BADARG;
        }
        if (rng_ctl && overlap(rng_ctl, 2 * CSTR_RNG_CTL_WORDS, logits, in_n[0])) return CSTR_E_BADARG;
    }
    multicategorical_act_kernel<<<row_grid(n, ACT_MAX_BLOCKS), 256, 0, (hipStream_t)stream>>>(
        logits, ldz, n, levels0, levels1, deterministic, action_in, u_in, rng_ctl, action_f32, action_out, valve_out, log_prob, u_out);
    return (int)hipGetLastError();
}

extern "C" int cstr_multicategorical_loss_f32(const cstr_multicategorical_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p || !workspace || !p->logits || !p->actions || !p->values || !p->adv || !p->returns || !p->g_logits || !p->g_value ||
        p->batch <= 0 || p->levels0 <= 0 || p->levels1 <= 0)
        return CSTR_E_BADARG;
    if (p->objective != 0 && p->objective != 1) return CSTR_E_BADARG;
    const bool ppo = p->objective == 0;
    if (ppo && (!p->old_log_prob || !(p->clip_range >= 0.0) || (p->clip_range_vf > 0.0 && !p->old_values))) return CSTR_E_BADARG;
    const int rc = face_check(p->levels0, p->levels1);
    if (rc) return rc;
    const int M = p->levels0 + p->levels1;
    if (p->ldz < M) return CSTR_E_BADARG;
    if (p->batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    const float *old_values = ppo && p->clip_range_vf > 0.0 ? p->old_values : nullptr;  // read only by the value clip
    const float *old_log_prob = ppo ? p->old_log_prob : nullptr;
    if (!aligned8(workspace) || !aligned4(p->logits) || !aligned8(p->actions) || !aligned4(p->values) || !aligned4(p->adv) ||
        !aligned4(p->returns) || !aligned4(p->g_logits) || !aligned4(p->g_value) || (old_values && !aligned4(old_values)) ||
        (old_log_prob && !aligned4(old_log_prob)) || (p->scalars_out && !aligned4(p->scalars_out)) ||
        (p->scalars_sum && !aligned4(p->scalars_sum)) || (p->log_prob_out && !aligned4(p->log_prob_out)))
        return CSTR_E_BADARG;
    {
        const int64_t B = p->batch, zs = span(B, p->ldz, M), ns = ppo ? 6 : 4;
        const void *ins[7] = {p->logits, p->actions, p->values, old_values, old_log_prob, p->adv, p->returns};
        const int64_t in_n[7] = {zs, 2 * B, B, B, B, B, B};
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
    cstr_multicategorical_loss_t k = *p;
    k.old_values = old_values;
    k.old_log_prob = old_log_prob;
    multicategorical_loss_kernel<<<row_grid(p->batch, CSTR_PPO_MAX_BLOCKS), 256, 0, (hipStream_t)stream>>>(
        k, reinterpret_cast<unsigned long long *>(workspace));
    return (int)hipGetLastError();
}
