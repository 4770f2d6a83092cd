// cstr_discrete_device.h -- what the two discrete action heads share (cstr_categorical.hip: one categorical over a 64-lane wave;
// cstr_multicategorical.hip: one per 32-lane half; internal, not part of the ABI): the segmented wave primitives, the index sources
// of the act launches and their host-side argument checks.
// A segment is W consecutive lanes, W = 64 or 32. The xor butterflies start at offset W / 2 and so never leave the segment; both
// partners form the same commutative result at every level, so every lane of the segment ends with the same bits and a row always
// reduces the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // one wave per row, 256-thread workgroups
constexpr int ACT_MAX_BLOCKS = 256;
constexpr int DISCRETE_SLOTS = 5;  // SLOT_POLICY .. SLOT_ENTROPY

template <int W> __device__ __forceinline__ float seg_max(float v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

template <int W> __device__ __forceinline__ float seg_sum(float v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// j: the lane's position in its segment
template <int W> __device__ __forceinline__ float seg_inclusive_scan(float v, const int j)
{
#pragma unroll
    for (int o = 1; o < W; o <<= 1) {
        const float t = __shfl_up(v, o, W);
        if (j >= o) v += t;
    }
    return v;
}

// index of the first maximum over the segment of the lanes' candidates (bv, bi), clamped below n (padded lanes hold -inf); a NaN is
// the greatest value, the first one wins (torch.argmax, cstr_dqn_act_f32's rule)
template <int W> __device__ __forceinline__ int seg_argmax(float bv, int bi, const int n)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        const bool greater = ov > bv || (ov != ov && bv == bv);
        const bool tie = ov == bv || (ov != ov && bv != bv);
        if (greater || (tie && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi < n ? bi : n - 1;
}

// the row's Philox4x32-10 block: keyed by the stream's seed, counter (offset + row, 0, the head's tag)
__device__ __forceinline__ void philox_row(const uint64_t seed, const uint64_t ctr, const uint32_t tag, uint32_t (&x)[4])
{
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, tag, (uint32_t)seed, (uint32_t)(seed >> 32), x);
}

// a teacher-forced level; outside the face: the caller's bug, clamped
__device__ __forceinline__ int clamp_level(const int64_t t, const int K) { return t < 0 ? 0 : (t >= K ? K - 1 : (int)t); }

// the same for a level stored as a float (rollout_data.actions.long())
__device__ __forceinline__ int stored_level(const float af, const int K) { return af >= 0.0f ? (af < (float)K ? (int)af : K - 1) : 0; }

// What a discrete loss kernel needs beside its head: P is cstr_categorical_loss_t or cstr_multicategorical_loss_t, whose shared
// fields carry the same names. PPO skips the advantage statistics for a single row, A2C does not (advantage_stats).
template <class P> struct DiscreteLoss {
    const P &p;
    const bool ppo, norm, vclip;
    const float lo, hi, cr, cv, inv_b, ec_b;
    float a_mean = 0.0f, a_den = 1.0f;
    double acc[DISCRETE_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0};

    __device__ __forceinline__ DiscreteLoss(const P &p_, double *red)
        : p(p_), ppo(p_.objective == 0), norm(p_.normalize_advantage && (!ppo || p_.batch > 1)), vclip(ppo && p_.clip_range_vf > 0.0),
          lo((float)(1.0 - p_.clip_range)), hi((float)(1.0 + p_.clip_range)), cr((float)p_.clip_range), cv((float)p_.clip_range_vf),
          inv_b(1.0f / (float)p_.batch), ec_b(p_.ent_coef * inv_b)
    {
        if (norm) advantage_stats(p.adv, p.batch, red, a_mean, a_den);
    }

    // every lane of the row's wave: the row's share of the policy objective
    __device__ __forceinline__ PolicyTerm policy(const int64_t b, const float logp) const
    {
        const float advn = norm ? (p.adv[b] - a_mean) / a_den : p.adv[b];
        return policy_term(ppo, logp, p.old_log_prob, b, advn, lo, hi, cr, inv_b);
    }

    // lane 0 of the row's wave: the per-row outputs and the row's summands (H: the row's entropy)
    __device__ __forceinline__ void row_done(const int64_t b, const float logp, const float H, const PolicyTerm &pt)
    {
        if (p.log_prob_out) p.log_prob_out[b] = logp;
        const ValueTerm vt = value_term(p.values[b], p.returns[b], p.old_values, b, vclip, cv, p.vf_coef, inv_b);
        p.g_value[b] = vt.g_value;
        acc[SLOT_POLICY] += pt.part0;
        acc[SLOT_VALUE] += (double)vt.sq;
        acc[SLOT_KL] += pt.part2;
        acc[SLOT_CLIPPED] += pt.part3;
        acc[SLOT_ENTROPY] += (double)H;
    }

    // the batch reduction and, in the last workgroup, the scalars; entropy_loss = -mean(entropy)
    __device__ __forceinline__ void finish(double *red, unsigned long long *__restrict__ ws, double *tot) const
    {
        if (!reduce_partials<DISCRETE_SLOTS>(acc, red, ws, tot)) return;
        if (threadIdx.x == 0)
            write_scalars(ppo, tot, p.batch, -(float)(tot[SLOT_ENTROPY] / (double)p.batch), p.ent_coef, p.vf_coef, p.scalars_out, p.scalars_sum);
    }
};

// The shared arguments of a discrete loss struct (objective 0 or 1) for loss_common_check. old_values (read only by PPO's value
// clip) and old_log_prob (read only by PPO) are nulled in `k`, the copy the kernel gets, where the launch does not read them: a
// stale pointer there is neither checked nor an error. cstr_ppo_loss_f32 differs: it checks old_values whenever it is given.
template <class P> inline LossCommon discrete_loss_common(P &k, const uint64_t *workspace)
{
    const bool ppo = k.objective == 0;
    if (!(ppo && k.clip_range_vf > 0.0)) k.old_values = nullptr;
    if (!ppo) k.old_log_prob = nullptr;
    return {ppo,           k.values,      k.adv,          k.returns, k.old_values, k.old_log_prob, k.g_value,
            k.scalars_out, k.scalars_sum, k.log_prob_out, workspace, k.batch,      k.clip_range,   k.clip_range_vf};
}

inline unsigned row_grid(int64_t rows, int64_t cap) { return lane_grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, 1, cap); }

// the act launches' index comes from exactly one source: deterministic, action_in, u_in or rng_ctl; u_out keeps a uniform that exists
inline bool act_sources_ok(int deterministic, const int64_t *action_in, const float *u_in, const uint64_t *rng_ctl, const float *u_out)
{
    const int sources = (deterministic != 0) + (action_in != nullptr) + (u_in != nullptr) + (rng_ctl != nullptr);
    return sources == 1 && !(u_out && !u_in && !rng_ctl);
}

// alignment and aliasing of an act launch's buffers; the action row is W floats wide (1: the index, 2: the level pair), `zs` the
// floats spanned by the logits
inline bool act_buffers_ok(const int W, const float *logits, const int64_t zs, const int64_t n, const int64_t *action_in, const float *u_in,
                           uint64_t *rng_ctl, float *action_f32, int64_t *action_out, float *valve_out, float *log_prob, float *u_out)
{
    if (!aligned4(logits) || !row_aligned(action_f32, W) || (action_out && !aligned8(action_out)) || (valve_out && !aligned8(valve_out)) ||
        (log_prob && !aligned4(log_prob)) || (u_out && !row_aligned(u_out, W)) || (action_in && !aligned8(action_in)) ||
        (u_in && !row_aligned(u_in, W)) || (rng_ctl && !aligned8(rng_ctl)))
        return false;
    const Buf ins[3] = {{logits, zs}, {action_in, 2 * W * n}, {u_in, W * n}};
    const Buf outs[6] = {{action_f32, W * n}, {action_out, 2 * W * n}, {valve_out, 2 * n}, {log_prob, n}, {u_out, W * n},
                         {rng_ctl, 2 * CSTR_RNG_CTL_WORDS}};
    return !outputs_overlap(ins, outs);
}

}  // namespace
