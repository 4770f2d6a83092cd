// cstr_onpolicy_device.h -- what the on-policy kernels share (cstr_ppo.hip, cstr_a2c.hip, cstr_dqn.hip, cstr_qrdqn.hip,
// cstr_categorical.hip, cstr_multicategorical.hip; internal, not part of the ABI):
//   * row loads and stores, the diagonal Gaussian's log-prob, the discrete faces' valve values;
//   * the loss core between a head's log-prob and the logged scalars: advantage_stats, policy_term, value_term, reduce_partials,
//     write_scalars, and the one loss kernel of the diagonal Gaussian head (PPO and A2C are its two instantiations);
//   * the sum-of-squares pass and the coefficient of clip_grad_norm_;
//   * the host-side argument checks: alignment, outputs_overlap, loss_common_check.
// THE REDUCTION CONVENTION, stated here once. Batch reductions have a fixed order and no float atomics: every thread sums its rows in
// f64, a fixed LDS tree per workgroup (block_sum_f64), the per-workgroup partials are published (agent-scope stores, release fence,
// ticket) and the workgroup that draws the last ticket sums them in workgroup order behind an acquire fence (reduce_partials). The
// grid is a function of the row count alone, so a given batch always reduces the same way.
// Everything sits in an anonymous namespace: each translation unit gets its own copy, nothing is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"

namespace {

constexpr float LOG_SQRT_2PI = 0.918938533204672742f;  // math.log(math.sqrt(2 * math.pi)) (torch Normal.log_prob)
constexpr double LOG_SQRT_2PI_F64 = 0.918938533204672742;  // rounds to LOG_SQRT_2PI
constexpr float HALF_LOG_2PI_E = 1.418938533204672742f;  // 0.5 + 0.5 * math.log(2 * math.pi) (torch Normal.entropy)
constexpr int WS_PART0 = 8;    // workspace word of the first partial (word 0: the ticket; 64-byte offset keeps it on its own line)
constexpr int WS_STRIDE = 8;   // partial words per workgroup of the PPO / A2C loss launches (8 + 64 * 8 words fit CSTR_PPO_WS_WORDS)
// the partial slots: the discrete heads use 0 .. 4, the Gaussian head 0 .. 3 and one slot per action dimension from SLOT_LOG_STD
constexpr int SLOT_POLICY = 0, SLOT_VALUE = 1, SLOT_KL = 2, SLOT_CLIPPED = 3, SLOT_ENTROPY = 4, SLOT_LOG_STD = 4;

template <int W> struct VecOf;
template <> struct VecOf<1> { typedef float type; };
template <> struct VecOf<2> { typedef float2 type; };
template <> struct VecOf<4> { typedef float4 type; };

template <int W> __device__ __forceinline__ void load_row(const float *p, float (&v)[W])
{
    const typename VecOf<W>::type t = *reinterpret_cast<const typename VecOf<W>::type *>(p);
    const float *f = reinterpret_cast<const float *>(&t);
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = f[k];
}

template <int W> __device__ __forceinline__ void store_row(float *p, const float (&v)[W])
{
    typename VecOf<W>::type t;
    float *f = reinterpret_cast<float *>(&t);
#pragma unroll
    for (int k = 0; k < W; ++k) f[k] = v[k];
    *reinterpret_cast<typename VecOf<W>::type *>(p) = t;
}

// distributions.py DiagGaussianDistribution.log_prob = sum over the action dimensions of torch's Normal.log_prob:
// -((a - mu)^2) / (2 sigma^2) - log(sigma) - log(sqrt(2 pi)), sigma = exp(log_std)
// T: float (every rollout head and loss launch) or double (cstr_trpo.hip, whose batch scalars are checked against float64 statements)
template <int A, typename T = float> __device__ __forceinline__ T diag_log_prob(const T (&act)[A], const T (&mu)[A], const T (&sig)[A])
{
    T lp = (T)0;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const T d = act[k] - mu[k];
        lp += (-(d * d) / ((T)2 * (sig[k] * sig[k])) - log(sig[k])) - (T)LOG_SQRT_2PI_F64;
    }
    return lp;
}

// v(q) of the discrete valve face (core/common/vec_env/cstr_vec_env.py): f32(-1) + f32(2 q) / f32(K - 1), in that order
__device__ __forceinline__ float valve_of(const int q, const int K) { return -1.0f + (float)(2 * q) / (float)(K - 1); }

// its inverse on a stored valve value: rint((v + 1) (K - 1) / 2), clamped into [0, K - 1] (a NaN gives 0)
__device__ __forceinline__ int level_of(const float v, const int K)
{
    const float x = ((v + 1.0f) * (float)(K - 1)) / 2.0f;
    return (int)rintf(fminf(fmaxf(x, 0.0f), (float)(K - 1)));
}

// sum of v over the workgroup's 256 threads in a fixed tree; every thread gets the result
__device__ __forceinline__ double block_sum_f64(double v, double *red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void publish_f64(unsigned long long *w, double v)
{
    __hip_atomic_store(w, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double consume_f64(unsigned long long *w)
{
    return __longlong_as_double((long long)__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Mean and unbiased standard deviation (+ 1e-8) of the advantages over the whole minibatch (ppo.py:219, a2c.py:156): every workgroup
// computes them itself, in the same order. The caller owns the guard: PPO skips the call for a single row (ppo.py:217), A2C has no
// such guard (a2c.py:155-156) and one row gives 0 / 0 = NaN, as torch.std of one element does.
// T: the type the statistics are formed and returned in, float (PPO, A2C) or double (cstr_trpo.hip).
template <typename T = float>
__device__ __forceinline__ void advantage_stats(const float *__restrict__ adv, const int64_t B, double *red, T &a_mean, T &a_den)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += 256) s += (double)adv[i];
    a_mean = (T)(block_sum_f64(s, red) / (double)B);
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += 256) {
        const T d = (T)adv[i] - a_mean;
        q += (double)(d * d);
    }
    a_den = (T)sqrt(block_sum_f64(q, red) / (double)(B - 1)) + (T)1e-8;
}

// one row's share of the policy objective: the summands of slots SLOT_POLICY, SLOT_KL and SLOT_CLIPPED and d loss / d log_prob
struct PolicyTerm {
    double part0, part2, part3;
    float g_logp;
};

// ppo = true: ratio, clipped surrogate, the approx_kl and clip_fraction terms (ppo.py:224-240), old_log_prob[b] is read;
// ppo = false: A2C's -adv * log_prob (a2c.py:159), old_log_prob is not touched. lo / hi / cr = f32(1 - clip), f32(1 + clip), f32(clip).
__device__ __forceinline__ PolicyTerm policy_term(const bool ppo, const float logp, const float *__restrict__ old_log_prob, const int64_t b,
                                                  const float advn, const float lo, const float hi, const float cr, const float inv_b)
{
    PolicyTerm t;
    t.part2 = 0.0;
    t.part3 = 0.0;
    if (ppo) {
        const float lr = logp - old_log_prob[b];
        const float ratio = expf(lr);
        const float pl1 = advn * ratio, pl2 = advn * fminf(fmaxf(ratio, lo), hi);
        // fminf / fmaxf drop a NaN operand where torch.clamp / torch.min propagate it: a NaN ratio stays one (pl1 carries a NaN
        // advantage by itself, and fminf of two NaNs is NaN)
        t.part0 = (double)(ratio != ratio ? ratio : fminf(pl1, pl2));
        t.part2 = (double)((ratio - 1.0f) - lr);
        t.part3 = fabsf(ratio - 1.0f) > cr ? 1.0 : 0.0;
        // d min(pl1, pl2) / d ratio: the clamp passes the gradient on the closed interval (there pl1 == pl2, torch splits the
        // gradient between the two equal operands and both halves arrive); outside it only pl1 carries one. torch.min zeroes
        // pl1's share only where pl1 > pl2, so a NaN product (of a NaN advantage or a NaN ratio) keeps it and the gradient is NaN
        const float dmin = ((ratio >= lo && ratio <= hi) || !(pl1 >= pl2)) ? advn : 0.0f;
        t.g_logp = -(inv_b * dmin) * ratio;
    } else {
        t.part0 = (double)(advn * logp);
        t.g_logp = -(inv_b * advn);  // d(-mean(adv * log_prob)) / d log_prob
    }
    return t;
}

struct ValueTerm {
    float sq, g_value;  // (returns - value)^2 and d loss / d value
};

// mse(returns, values) (ppo.py:242-254, a2c.py:162); vclip: the value moves at most cv from old_values[b], which is read only then,
// and a clamped row passes no gradient
__device__ __forceinline__ ValueTerm value_term(const float v, const float ret, const float *__restrict__ old_values, const int64_t b,
                                                const bool vclip, const float cv, const float vf_coef, const float inv_b)
{
    float vp = v;
    bool pass = true;
    if (vclip) {
        const float vo = old_values[b], dv = v - vo;
        vp = vo + (dv != dv ? dv : fminf(fmaxf(dv, -cv), cv));  // torch.clamp: a NaN step stays one, the value loss goes NaN
        pass = dv >= -cv && dv <= cv;                           // ... and its mask passes no gradient for it: g_value = 0
    }
    const float dr = ret - vp;
    ValueTerm t;
    t.sq = dr * dr;
    t.g_value = pass ? vf_coef * ((2.0f * inv_b) * (vp - ret)) : 0.0f;
    return t;
}

// The batch reduction of every loss launch. Slot k of acc (bit k of USED set; the others cost nothing and leave tot[k] unwritten) goes
// through the workgroup's tree and is published at ws[WS_PART0 + workgroup * STRIDE + k]; release fence, ticket on ws[0] (which
// resets itself), acquire fence; the workgroup that drew the last ticket sums every slot in workgroup order into tot (LDS, N
// doubles). Returns true in that workgroup alone, for all its threads, behind a barrier: tot is ready to read.
template <int N, unsigned USED = (1u << N) - 1u, int STRIDE = WS_STRIDE>
__device__ __forceinline__ bool reduce_partials(const double (&acc)[N], double *red, unsigned long long *__restrict__ ws, double *tot)
{
    static_assert(N <= STRIDE && N <= 32, "a workgroup's partials fit its stride");
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (!((USED >> k) & 1u)) continue;
        const double s = block_sum_f64(acc[k], red);
        if (threadIdx.x == 0) publish_f64(ws + WS_PART0 + (int64_t)blockIdx.x * STRIDE + k, s);
    }
    __threadfence();  // release: the partials are visible chip-wide before this workgroup's ticket is
    if (!last_block_ticket(ws)) return false;
    __threadfence();  // acquire: behind the last ticket every workgroup's partials are read from memory
    if (threadIdx.x < N && ((USED >> threadIdx.x) & 1u)) {
        double s = 0.0;
        for (unsigned j = 0; j < gridDim.x; ++j) s += consume_f64(ws + WS_PART0 + (int64_t)j * STRIDE + threadIdx.x);
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    return true;
}

// The logged scalars, by one thread of the last workgroup: PPO_SCALARS' six or A2C_SCALARS' four (hip_ops.py), written to
// scalars_out and added to scalars_sum where given. entropy_loss = -mean(entropy) is the head's own.
__device__ __forceinline__ void write_scalars(const bool ppo, const double *tot, const int64_t B, const float entropy_loss, const float ent_coef,
                                              const float vf_coef, float *__restrict__ scalars_out, float *__restrict__ scalars_sum)
{
    float out[6];
    out[0] = -(float)(tot[SLOT_POLICY] / (double)B);  // policy_gradient_loss / policy_loss
    out[1] = (float)(tot[SLOT_VALUE] / (double)B);    // value_loss
    out[2] = entropy_loss;
    out[3] = (out[0] + ent_coef * out[2]) + vf_coef * out[1];  // loss
    out[4] = (float)(tot[SLOT_KL] / (double)B);       // approx_kl (PPO)
    out[5] = (float)(tot[SLOT_CLIPPED] / (double)B);  // clip_fraction (PPO)
    const int n_out = ppo ? 6 : 4;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k < n_out) {
            if (scalars_out) scalars_out[k] = out[k];
            if (scalars_sum) scalars_sum[k] += out[k];
        }
    }
}

// ppo.py:213-264 (PPO) / a2c.py:150-171 (!PPO) on the diagonal Gaussian head in ONE launch, one lane per row: advantage normalisation,
// the log-prob and entropy, the policy and value losses, the scalars and the gradients w.r.t. the action mean, the value and log_std.
// cstr_a2c_loss_f32 fills a cstr_ppo_loss_t; without PPO, old_values, old_log_prob and the clip ranges are never read and slots
// SLOT_KL and SLOT_CLIPPED are skipped at compile time.
template <int A, bool PPO>
__global__ __launch_bounds__(256) void diag_gaussian_loss_kernel(const cstr_ppo_loss_t p, unsigned long long *__restrict__ ws)
{
    constexpr unsigned LOG_STD_SLOTS = ((1u << A) - 1u) << SLOT_LOG_STD;
    constexpr unsigned USED = (PPO ? 0xFu : 0x3u) | LOG_STD_SLOTS;
    __shared__ double red[256];
    __shared__ double tot[WS_STRIDE];
    const int64_t B = p.batch;
    const bool norm = p.normalize_advantage && (!PPO || B > 1);
    float a_mean = 0.0f, a_den = 1.0f;
    if (norm) advantage_stats(p.adv, B, red, a_mean, a_den);
    float sig[A], var[A];
#pragma unroll
    for (int k = 0; k < A; ++k) {
        sig[k] = expf(p.log_std[k]);
        var[k] = sig[k] * sig[k];
    }
    const float lo = (float)(1.0 - p.clip_range), hi = (float)(1.0 + p.clip_range), cr = (float)p.clip_range;
    const bool vclip = PPO && p.clip_range_vf > 0.0;
    const float cv = (float)p.clip_range_vf;
    const float inv_b = 1.0f / (float)B;
    double acc[WS_STRIDE];
#pragma unroll
    for (int k = 0; k < WS_STRIDE; ++k) acc[k] = 0.0;
    for (int64_t b = blockIdx.x * 256ll + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256ll) {
        float mu[A], act[A];
        load_row<A>(p.mean + b * p.ldm, mu);
        load_row<A>(p.actions + b * A, act);
        const float logp = diag_log_prob<A>(act, mu, sig);
        if (p.log_prob_out) p.log_prob_out[b] = logp;
        const float advn = norm ? (p.adv[b] - a_mean) / a_den : p.adv[b];
        const PolicyTerm pt = policy_term(PPO, logp, p.old_log_prob, b, advn, lo, hi, cr, inv_b);
        acc[SLOT_POLICY] += pt.part0;
        if (PPO) {
            acc[SLOT_KL] += pt.part2;
            acc[SLOT_CLIPPED] += pt.part3;
        }
        float gm[A];
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float d = act[k] - mu[k];
            gm[k] = pt.g_logp * (d / var[k]);
            acc[SLOT_LOG_STD + k] += (double)(pt.g_logp * ((d * d) / var[k] - 1.0f));
        }
        store_row<A>(p.g_mean + b * A, gm);
        const ValueTerm vt = value_term(p.values[b], p.returns[b], p.old_values, b, vclip, cv, p.vf_coef, inv_b);
        acc[SLOT_VALUE] += (double)vt.sq;
        p.g_value[b] = vt.g_value;
    }
    if (!reduce_partials<WS_STRIDE, USED>(acc, red, ws, tot)) return;
    if (threadIdx.x == 0) {
        float ent = 0.0f;
#pragma unroll
        for (int k = 0; k < A; ++k) ent += HALF_LOG_2PI_E + logf(sig[k]);
        // entropy_loss = -mean(entropy); the entropy does not depend on the row
        write_scalars(PPO, tot, B, -ent, p.ent_coef, p.vf_coef, p.scalars_out, p.scalars_sum);
#pragma unroll
        for (int k = 0; k < A; ++k) p.g_log_std[k] = (float)tot[SLOT_LOG_STD + k] - p.ent_coef;  // d(ent_coef * entropy_loss) / d log_std = -ent_coef
    }
}

// clip_grad_norm_ (torch.nn.utils): launch 1, per-workgroup sums of squares
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ grad, const int64_t n, double *__restrict__ part)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256ll) {
        const float g = grad[i];
        s += (double)(g * g);
    }
    const double t = block_sum_f64(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// the partials of launch 1 summed in workgroup order: coef = min(1, max_norm / (norm + 1e-6))
__device__ __forceinline__ float grad_clip_coef(const double *__restrict__ part, const int n_part, const float max_norm, float &norm)
{
    double s = 0.0;
    for (int j = 0; j < n_part; ++j) s += part[j];
    norm = (float)sqrt(s);
    return fminf(max_norm / (norm + 1e-6f), 1.0f);
}

inline bool overlap(const void *a, int64_t a_floats, const void *b, int64_t b_floats)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 4u * (uintptr_t)b_floats && b0 < a0 + 4u * (uintptr_t)a_floats;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool row_aligned(const void *p, int width) { return width == 4 ? aligned16(p) : (width == 1 ? aligned4(p) : aligned8(p)); }

inline unsigned lane_grid(int64_t n, int block, int64_t cap)
{
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}

// floats spanned by `rows` rows of `width` floats with row stride ld
inline int64_t span(int64_t rows, int64_t ld, int64_t width) { return (rows - 1) * ld + width; }

// a launch argument as the aliasing check sees it: `floats` 4-byte words from p; a NULL (optional, absent) buffer overlaps nothing
struct Buf {
    const void *p;
    int64_t floats;
};

// does any output overlap an input or another output? A buffer the launch both reads and writes (a workspace, an rng_ctl) is an output.
template <int NI, int NO> inline bool outputs_overlap(const Buf (&ins)[NI], const Buf (&outs)[NO])
{
    for (int o = 0; o < NO; ++o) {
        if (!outs[o].p) continue;
        for (int i = 0; i < NI; ++i)
            if (ins[i].p && overlap(outs[o].p, outs[o].floats, ins[i].p, ins[i].floats)) return true;
        for (int q = o + 1; q < NO; ++q)
            if (outs[q].p && overlap(outs[o].p, outs[o].floats, outs[q].p, outs[q].floats)) return true;
    }
    return false;
}

// the arguments the four loss structs share, as the entry point hands them over (old_values, old_log_prob, scalars_sum: NULL where
// the struct has none or the entry point decides the launch does not read them)
struct LossCommon {
    bool ppo;  // objective: PPO (six scalars, the clip rule) or A2C (four)
    const float *values, *adv, *returns, *old_values, *old_log_prob;
    float *g_value, *scalars_out, *scalars_sum, *log_prob_out;
    const uint64_t *workspace;
    int64_t batch;
    double clip_range, clip_range_vf;
};

// The shared part of a loss entry point's validation, in the order all four report it: a missing required pointer, a row count < 1
// or a broken PPO rule (old_log_prob, clip_range >= 0, old_values with a value clip) -> CSTR_E_BADARG; then `head_rc`, the head's own
// verdict on its shape (0, or what the entry point returns for it); then more than CSTR_PPO_MAX_ROWS rows -> CSTR_E_UNSUPPORTED;
// then a misaligned buffer -> CSTR_E_BADARG.
inline int loss_common_check(const LossCommon &c, const int head_rc)
{
    if (!c.workspace || !c.values || !c.adv || !c.returns || !c.g_value || c.batch <= 0) return CSTR_E_BADARG;
    if (c.ppo && (!c.old_log_prob || !(c.clip_range >= 0.0) || (c.clip_range_vf > 0.0 && !c.old_values))) return CSTR_E_BADARG;
    if (head_rc) return head_rc;
    if (c.batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    const void *f32[9] = {c.values, c.adv, c.returns, c.old_values, c.old_log_prob, c.g_value, c.scalars_out, c.scalars_sum, c.log_prob_out};
    for (int i = 0; i < 9; ++i)
        if (f32[i] && !aligned4(f32[i])) return CSTR_E_BADARG;
    return aligned8(c.workspace) ? 0 : CSTR_E_BADARG;
}

// outputs_overlap over the head's own buffers and the shared ones
template <int NI, int NO> inline bool loss_outputs_overlap(const LossCommon &c, const Buf (&head_ins)[NI], const Buf (&head_outs)[NO])
{
    const int64_t B = c.batch, ns = c.ppo ? 6 : 4;
    Buf ins[NI + 5] = {{c.values, B}, {c.old_values, B}, {c.old_log_prob, B}, {c.adv, B}, {c.returns, B}};
    Buf outs[NO + 5] = {{c.g_value, B}, {c.scalars_out, ns}, {c.scalars_sum, ns}, {c.log_prob_out, B}, {c.workspace, 2 * CSTR_PPO_WS_WORDS}};
    for (int i = 0; i < NI; ++i) ins[5 + i] = head_ins[i];
    for (int o = 0; o < NO; ++o) outs[5 + o] = head_outs[o];
    return outputs_overlap(ins, outs);
}

// cstr_ppo_loss_f32 (PPO) and cstr_a2c_loss_f32 (!PPO, on the struct it filled): validation and launch of diag_gaussian_loss_kernel
template <bool PPO> inline int diag_gaussian_loss_launch(const cstr_ppo_loss_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p->mean || !p->log_std || !p->actions || !p->g_mean || !p->g_log_std || p->act_dim <= 0) return CSTR_E_BADARG;
    // old_values goes to the shared check as the caller gave it: cstr_ppo_loss_f32 has its alignment and aliasing checked even when
    // the value clip is off and the launch does not read it, where the discrete entry points null it first
    const LossCommon c = {PPO,           p->values,      p->adv,         p->returns,      p->old_values, p->old_log_prob, p->g_value,
                          p->scalars_out, p->scalars_sum, p->log_prob_out, workspace,       p->batch,      p->clip_range,   p->clip_range_vf};
    const int A = p->act_dim;
    const int rc = loss_common_check(c, (A != 2 && A != 4) ? CSTR_E_UNSUPPORTED : 0);
    if (rc) return rc;
    if (p->ldm < A || (p->ldm * 4) % (A == 4 ? 16 : 8)) return CSTR_E_BADARG;
    if (!row_aligned(p->mean, A) || !row_aligned(p->actions, A) || !row_aligned(p->g_mean, A) || !aligned4(p->log_std) ||
        !aligned4(p->g_log_std))
        return CSTR_E_BADARG;
    const int64_t B = p->batch;
    const Buf ins[3] = {{p->mean, span(B, p->ldm, A)}, {p->log_std, A}, {p->actions, B * A}};
    const Buf outs[2] = {{p->g_mean, B * A}, {p->g_log_std, A}};
    if (loss_outputs_overlap(c, ins, outs)) return CSTR_E_BADARG;
    const unsigned grid = lane_grid(B, 256, CSTR_PPO_MAX_BLOCKS);
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(workspace);
    if (A == 2) diag_gaussian_loss_kernel<2, PPO><<<grid, 256, 0, (hipStream_t)stream>>>(*p, ws);
    else diag_gaussian_loss_kernel<4, PPO><<<grid, 256, 0, (hipStream_t)stream>>>(*p, ws);
    return (int)hipGetLastError();
}

}  // namespace
