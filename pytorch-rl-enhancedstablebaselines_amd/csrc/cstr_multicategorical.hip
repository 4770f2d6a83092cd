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
// Batch reductions: lane 0 of every wave sums its rows in f64; from there the convention at the top of cstr_onpolicy_device.h.
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

constexpr uint32_t MCAT_STREAM_TAG = 0x3CA7A11Cu;  // counter word 3: never shares counters with the other heads' streams

// the lane's logit: level j of its valve, -inf on a padded lane
__device__ __forceinline__ float load_logit(const float *__restrict__ row, const int col, const bool valid) { return valid ? row[col] : -INFINITY; }

// logp_j = (z_j - m_g) - log(sum_j exp(z_j - m_g)) over the lane's half
__device__ __forceinline__ float half_log_softmax(const float z)
{
    const float m = seg_max<32>(z);
    const float lse = logf(seg_sum<32>(expf(z - m)));
    return (z - m) - lse;
}

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
            const int a = seg_argmax<32>(z, j, K);  // first maximum of the lane's half
            a0 = __shfl(a, 0);
            a1 = __shfl(a, 32);
        } else if (action_in) {
            a0 = clamp_level(action_in[2 * r], K0);
            a1 = clamp_level(action_in[2 * r + 1], K1);
        } else {
            if (draw) {
                uint32_t x[4];
                philox_row(seed, base + (uint64_t)r, MCAT_STREAM_TAG, x);
                u0 = philox_uniform(x[0]);
                u1 = philox_uniform(x[1]);
            } else {
                const float2 t = *reinterpret_cast<const float2 *>(u_in + 2 * r);
                u0 = t.x;
                u1 = t.y;
            }
            const float cum = seg_inclusive_scan<32>(expf(lp), j);
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

// ppo.py:213-264 (objective 0) / a2c.py:150-171 (objective 1) on the pair's log-prob and entropy
__global__ __launch_bounds__(256) void multicategorical_loss_kernel(const cstr_multicategorical_loss_t p, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[DISCRETE_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31;
    const int K0 = p.levels0, K1 = p.levels1;
    const int K = half ? K1 : K0, col = half ? K0 + j : j;
    const bool valid = j < K;
    const int64_t B = p.batch;
    DiscreteLoss<cstr_multicategorical_loss_t> core(p, red);
    for (int64_t b = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; b < B; b += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        const float z = load_logit(p.logits + b * p.ldz, col, valid);
        float lp = half_log_softmax(z);
        const float pr = expf(lp);
        lp = fmaxf(lp, -FLT_MAX);  // torch's Categorical.entropy clamps the logits; the pair's log-prob below is never -inf * 0
        const float Hg = -seg_sum<32>(pr * lp);  // this lane's valve
        const float H = __shfl(Hg, 0) + __shfl(Hg, 32);
        const float2 af = *reinterpret_cast<const float2 *>(p.actions + 2 * b);
        const int a0 = stored_level(af.x, K0), a1 = stored_level(af.y, K1);
        const float logp = __shfl(lp, a0) + __shfl(lp, 32 + a1);
        const PolicyTerm pt = core.policy(b, logp);
        if (valid) {
            const int a = half ? a1 : a0;
            p.g_logits[b * p.ldz + col] = pt.g_logp * ((j == a ? 1.0f : 0.0f) - pr) + core.ec_b * (pr * (lp + Hg));  // the valve's own entropy
        }
        if (lane == 0) core.row_done(b, logp, H, pt);
    }
    core.finish(red, ws, tot);
}

// the face's verdict and, behind it, the row stride's
inline int face_check(int levels0, int levels1, int64_t ldz)
{
    if (levels0 < 2 || levels0 > CSTR_MCAT_MAX_LEVELS || levels1 < 2 || levels1 > CSTR_MCAT_MAX_LEVELS) return CSTR_E_UNSUPPORTED;
    return ldz < levels0 + levels1 ? CSTR_E_BADARG : 0;
}

}  // namespace

extern "C" int cstr_multicategorical_act_f32(const float *logits, int64_t ldz, int64_t n, int levels0, int levels1, int deterministic,
                                             const int64_t *action_in, const float *u_in, uint64_t *rng_ctl, float *action_f32,
                                             int64_t *action_out, float *valve_out, float *log_prob, float *u_out, cstr_stream_t stream)
{
    if (!logits || !action_f32 || n <= 0 || levels0 <= 0 || levels1 <= 0) return CSTR_E_BADARG;
    if (!act_sources_ok(deterministic, action_in, u_in, rng_ctl, u_out)) return CSTR_E_BADARG;
    const int rc = face_check(levels0, levels1, ldz);
    if (rc) return rc;
    if (n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!act_buffers_ok(2, logits, span(n, ldz, levels0 + levels1), n, action_in, u_in, rng_ctl, action_f32, action_out, valve_out, log_prob,
                        u_out))
        return CSTR_E_BADARG;
    multicategorical_act_kernel<<<row_grid(n, ACT_MAX_BLOCKS), 256, 0, (hipStream_t)stream>>>(
        logits, ldz, n, levels0, levels1, deterministic, action_in, u_in, rng_ctl, action_f32, action_out, valve_out, log_prob, u_out);
    return (int)hipGetLastError();
}

extern "C" int cstr_multicategorical_loss_f32(const cstr_multicategorical_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p || !p->logits || !p->actions || !p->g_logits || p->levels0 <= 0 || p->levels1 <= 0) return CSTR_E_BADARG;
    if (p->objective != 0 && p->objective != 1) return CSTR_E_BADARG;
    cstr_multicategorical_loss_t k = *p;
    const LossCommon c = discrete_loss_common(k, workspace);  // nulls what the objective does not read
    const int rc = loss_common_check(c, face_check(p->levels0, p->levels1, p->ldz));
    if (rc) return rc;
    if (!aligned4(p->logits) || !aligned8(p->actions) || !aligned4(p->g_logits)) return CSTR_E_BADARG;
    const int64_t B = p->batch, zs = span(B, p->ldz, p->levels0 + p->levels1);
    const Buf ins[2] = {{p->logits, zs}, {p->actions, 2 * B}};
    const Buf outs[1] = {{p->g_logits, zs}};
    if (loss_outputs_overlap(c, ins, outs)) return CSTR_E_BADARG;
    multicategorical_loss_kernel<<<row_grid(B, CSTR_PPO_MAX_BLOCKS), 256, 0, (hipStream_t)stream>>>(
        k, reinterpret_cast<unsigned long long *>(workspace));
    return (int)hipGetLastError();
}
