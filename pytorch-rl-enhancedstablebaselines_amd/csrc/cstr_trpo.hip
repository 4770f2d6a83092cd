// cstr_trpo.hip -- TRPO's own arithmetic around the Linear layers (the published trust-region step: natural gradient by conjugate
// gradient on Fisher-vector products, a backtracking line search against a hard KL bound, a separate critic), f32 storage, gfx950:
//   * the tangent (forward-mode) pass of one Linear + activation layer on the f32 matrix cores (cstr_linear_tangent_fwd_f32): the first
//     forward-mode kernel of the library;
//   * everything between the actor's outputs and its backward in ONE launch, templated on the three heads (trpo_objective_kernel):
//     advantage normalisation, log-prob, ratio, objective, KL against the distribution at theta0, the objective's gradients; in
//     line-search mode the accept decision and the shrinking of the device-resident coefficient instead of the gradients;
//   * the head's Fisher metric times a tangent (cstr_trpo_fisher_head_f32);
//   * one single-workgroup conjugate-gradient launch per iteration, with an init and a finishing form (cstr_trpo_cg_step_f32);
//   * theta = theta0 + coeff * step * s over the actor's tensors (cstr_trpo_apply_step_f32);
//   * the critic minibatch's loss launch and the conjugate gradient's start vector on TRPO's own Philox stream.
// WHY THE FISHER FORM: at theta0 the new and the old distribution coincide, d kl / d (distribution parameters) = 0, and the Hessian of
// the mean KL is (1/R) sum_r J_r^T M_r J_r exactly -- a tangent pass, the metric M_r of the head, and the ordinary backward.
// Batch sums follow the convention at the top of cstr_onpolicy_device.h (f64, fixed tree, ticket, no float atomics); the per-row terms of
// the objective launch are formed in double from the float inputs by the SAME device functions the PPO / A2C launches instantiate in
// float (diag_log_prob, advantage_stats), so the launch can be held to the kernel-against-fp64 bar. The discrete heads run one wave per
// row: a categorical over the 64 lanes, a multi-categorical with one valve per 32-lane half (the mapping of cstr_multicategorical.hip).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_discrete_device.h"
#include "cstr_onpolicy_device.h"
#include "cstr_policy_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t TRPO_STREAM_TAG = 0x7290C6A5u;  // counter word 3: never shares counters with the other streams
constexpr int CG_THREADS = 1024;

// ---- the tangent of a Linear + activation layer ---------------------------------------------------------------------------------------
// One wave per 16 x 16 output tile, operands straight from L2 as 16-byte vectors (the structure of cstr_mlp.hip's linear_act_fwd_kernel):
// lane (r = lane & 15, h = lane >> 4) loads [row r][16 c + 4 h .. + 3] of all four operands per 16-wide K chunk and feeds element e to
// MFMA step e; acc0 sums x . w_dot, acc1 sums x_dot . w -- two independent accumulator chains, which is what the 16x16x4 f32 MFMA
// needs to reach its issue rate -- and they meet in the epilogue; without x_dot (the first layer) the one product alternates between
// the two chains. Rows >= M / N and k >= K are loaded as zeros (guarded loads); 16-wide chunks at or beyond K are skipped.
template <int ACT, bool VEC, bool XDOT>
__global__ __launch_bounds__(64) void linear_tangent_fwd_kernel(const float *__restrict__ x, const float *__restrict__ xd,
                                                                const float *__restrict__ w, const float *__restrict__ wd, const int ldx,
                                                                const int ldxd, const int M, const int N, const int K,
                                                                const float *__restrict__ bd, const float *__restrict__ y,
                                                                float *__restrict__ zd)
{
    const int lane = threadIdx.x, r = lane & 15, h = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const bool row_ok = m0 + r < M, col_ok = n0 + r < N;
    const float *xr = x + (int64_t)(row_ok ? m0 + r : 0) * ldx;
    const float *xdr = XDOT ? xd + (int64_t)(row_ok ? m0 + r : 0) * ldxd : nullptr;
    const float *wr = w + (int64_t)(col_ok ? n0 + r : 0) * K;
    const float *wdr = wd + (int64_t)(col_ok ? n0 + r : 0) * K;
    const float bv = bd[min(n0 + r, N - 1)];
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int UNROLL = 4;  // K = 64: every load of the tile in flight at once
    for (int c0 = 0; c0 < K; c0 += 16 * UNROLL) {
        float4 a[UNROLL], b[UNROLL], ad[UNROLL], bw[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (c0 + 16 * u >= K) break;  // wave-uniform: the first layer (K = 4) is one chunk
            const int k = c0 + 16 * u + 4 * h;
            a[u] = load_k4<VEC>(xr, k, K, row_ok);
            b[u] = load_k4<VEC>(wdr, k, K, col_ok);
            if (XDOT) {
                ad[u] = load_k4<VEC>(xdr, k, K, row_ok);
                bw[u] = load_k4<VEC>(wr, k, K, col_ok);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (c0 + 16 * u >= K) break;
            if (XDOT) {  // one chain per product
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[u].x, bw[u].x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u].y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[u].y, bw[u].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[u].z, bw[u].z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u].w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[u].w, bw[u].w, acc1, 0, 0, 0);
            } else {  // the one product alternates between the two chains, as linear_act_fwd_kernel's does
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u].w, acc1, 0, 0, 0);
            }
        }
    }
    const f32x4 acc = acc0 + acc1;
    // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 * (lane >> 4) + register
    const int col = n0 + r;
    if (col < N) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = m0 + 4 * h + e;
            if (row < M) {
                const int64_t o = (int64_t)row * N + col;
                float v = acc[e] + bv;
                if (ACT == ACT_TANH) {
                    const float yv = y[o];
                    v = v * (1.0f - yv * yv);
                }
                if (ACT == ACT_RELU) v = y[o] > 0.0f ? v : 0.0f;
                zd[o] = v;
            }
        }
    }
}

// ---- the objective launch ------------------------------------------------------------------------------------------------------------
constexpr int SLOT_OBJ = 0, SLOT_KLD = 1, SLOT_GLS = 2;  // the partial slots: objective, kl, d objective / d log_std[0 .. 3]
constexpr int TRPO_SLOTS = 6;

struct ObjectiveCore {
    bool norm;
    double a_mean, a_den, inv_r;
};

__device__ __forceinline__ ObjectiveCore objective_core(const cstr_trpo_objective_t &p, double *red)
{
    ObjectiveCore c;
    c.norm = p.normalize_advantage != 0;
    c.a_mean = 0.0;
    c.a_den = 1.0;
    c.inv_r = 1.0 / (double)p.batch;
    if (c.norm) advantage_stats<double>(p.adv, p.batch, red, c.a_mean, c.a_den);
    return c;
}

// the batch reduction and, in the workgroup that finishes last, the scalars, the control block and the line search's decision
template <unsigned USED>
__device__ __forceinline__ void objective_finish(const cstr_trpo_objective_t &p, const double (&acc)[TRPO_SLOTS], double *red,
                                                 unsigned long long *__restrict__ ws, double *tot, const int n_log_std)
{
    if (!reduce_partials<TRPO_SLOTS, USED>(acc, red, ws, tot)) return;
    if (threadIdx.x != 0) return;
    const double objective = tot[SLOT_OBJ] / (double)p.batch, kl = tot[SLOT_KLD] / (double)p.batch;
    if (p.scalars_out) {
        p.scalars_out[0] = (float)objective;
        p.scalars_out[1] = (float)kl;
    }
    if (!p.line_search) {
        p.ctl[CSTR_TRPO_CTL_OBJECTIVE] = objective;
        p.ctl[CSTR_TRPO_CTL_KL] = kl;
        p.ctl[CSTR_TRPO_CTL_COEFF] = 1.0;
        for (int k = 0; k < n_log_std; ++k) p.g_log_std[k] = (float)tot[SLOT_GLS + k];
    } else {
        const bool ok = kl < p.target_kl && objective > p.ctl[CSTR_TRPO_CTL_OBJECTIVE];
        p.ctl[CSTR_TRPO_CTL_LS_OBJECTIVE] = objective;
        p.ctl[CSTR_TRPO_CTL_LS_KL] = kl;
        if (!ok) p.ctl[CSTR_TRPO_CTL_COEFF] = p.ctl[CSTR_TRPO_CTL_COEFF] * p.shrink;
        p.accepted[0] = ok ? 1 : 0;
    }
}

// the diagonal Gaussian head, one lane per row. KL(new || old) per dimension, torch's _kl_normal_normal:
// 0.5 * ((s / s0)^2 + ((mu - mu0) / s0)^2 - 1 - log((s / s0)^2))
template <int A>
__global__ __launch_bounds__(256) void trpo_objective_gaussian_kernel(const cstr_trpo_objective_t p, unsigned long long *__restrict__ ws)
{
    constexpr unsigned USED = 0x3u | (((1u << A) - 1u) << SLOT_GLS);
    __shared__ double red[256];
    __shared__ double tot[TRPO_SLOTS];
    const int64_t B = p.batch;
    const ObjectiveCore c = objective_core(p, red);
    double sig[A], sig0[A], kl_const = 0.0;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        sig[k] = exp((double)p.log_std[k]);
        sig0[k] = exp((double)p.old_log_std[k]);
        const double vr = (sig[k] / sig0[k]) * (sig[k] / sig0[k]);
        kl_const += 0.5 * (vr - 1.0 - log(vr));  // the row-independent part
    }
    double acc[TRPO_SLOTS];
#pragma unroll
    for (int k = 0; k < TRPO_SLOTS; ++k) acc[k] = 0.0;
    for (int64_t b = blockIdx.x * 256ll + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256ll) {
        float muf[A], mu0f[A], actf[A];
        load_row<A>(p.dist + b * p.ld, muf);
        load_row<A>(p.old_dist + b * p.old_ld, mu0f);
        load_row<A>(p.actions + b * A, actf);
        double mu[A], act[A];
#pragma unroll
        for (int k = 0; k < A; ++k) {
            mu[k] = (double)muf[k];
            act[k] = (double)actf[k];
        }
        const double logp = diag_log_prob<A, double>(act, mu, sig);
        const double advn = c.norm ? ((double)p.adv[b] - c.a_mean) / c.a_den : (double)p.adv[b];
        const double ratio = exp(logp - (double)p.old_log_prob[b]);
        acc[SLOT_OBJ] += advn * ratio;
        double kl = kl_const;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const double t = (mu[k] - (double)mu0f[k]) / sig0[k];
            kl += 0.5 * (t * t);
        }
        acc[SLOT_KLD] += kl;
        if (!p.line_search) {
            const double g_logp = (advn * ratio) * c.inv_r;  // d objective / d log_prob of this row
            float gm[A];
#pragma unroll
            for (int k = 0; k < A; ++k) {
                const double d = act[k] - mu[k], var = sig[k] * sig[k];
                gm[k] = (float)(g_logp * (d / var));
                acc[SLOT_GLS + k] += g_logp * ((d * d) / var - 1.0);
            }
            store_row<A>(p.g_dist + b * A, gm);
        }
    }
    objective_finish<USED>(p, acc, red, ws, tot, A);
}

template <int W> __device__ __forceinline__ double seg_max_f64(double v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

template <int W> __device__ __forceinline__ double seg_sum_f64(double v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// log-softmax over the lane's segment (a padded lane holds -inf)
template <int W> __device__ __forceinline__ double seg_log_softmax_f64(const double z)
{
    const double m = seg_max_f64<W>(z);
    return (z - m) - log(seg_sum_f64<W>(exp(z - m)));
}

// the discrete heads, one wave per row: W = 64, one categorical over k0 logits; W = 32, one categorical per half (k0 | k1 logits).
// KL(new || old) per block = sum_j p_j (logp_j - logq_j) (torch's _kl_categorical_categorical on finite logits)
template <int W>
__global__ __launch_bounds__(256) void trpo_objective_discrete_kernel(const cstr_trpo_objective_t p, unsigned long long *__restrict__ ws)
{
    __shared__ double red[256];
    __shared__ double tot[TRPO_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = lane / W, j = lane % W;  // W = 64: seg = 0
    const int K = seg ? p.k1 : p.k0, col = seg ? p.k0 + j : j, width = W == 64 ? p.k0 : p.k0 + p.k1;
    const bool valid = j < K;
    const int64_t B = p.batch;
    const ObjectiveCore c = objective_core(p, red);
    double acc[TRPO_SLOTS];
#pragma unroll
    for (int k = 0; k < TRPO_SLOTS; ++k) acc[k] = 0.0;
    for (int64_t b = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; b < B; b += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        const double z = valid ? (double)p.dist[b * p.ld + col] : -INFINITY;
        const double z0 = valid ? (double)p.old_dist[b * p.old_ld + col] : -INFINITY;
        const double lp = seg_log_softmax_f64<W>(z), lq = seg_log_softmax_f64<W>(z0);
        const double pr = valid ? exp(lp) : 0.0;
        const double klg = seg_sum_f64<W>(valid ? pr * (lp - lq) : 0.0);
        int a;
        double logp, kl;
        if (W == 64) {
            a = stored_level(p.actions[b], p.k0);
            logp = __shfl(lp, a);
            kl = klg;
        } else {
            const float2 af = *reinterpret_cast<const float2 *>(p.actions + 2 * b);
            const int a0 = stored_level(af.x, p.k0), a1 = stored_level(af.y, p.k1);
            a = seg ? a1 : a0;
            logp = __shfl(lp, a0) + __shfl(lp, 32 + a1);
            kl = __shfl(klg, 0) + __shfl(klg, 32);
        }
        const double advn = c.norm ? ((double)p.adv[b] - c.a_mean) / c.a_den : (double)p.adv[b];
        const double ratio = exp(logp - (double)p.old_log_prob[b]);
        if (!p.line_search && valid) p.g_dist[b * width + col] = (float)(((advn * ratio) * c.inv_r) * ((j == a ? 1.0 : 0.0) - pr));
        if (lane == 0) {
            acc[SLOT_OBJ] += advn * ratio;
            acc[SLOT_KLD] += kl;
        }
    }
    objective_finish<0x3u>(p, acc, red, ws, tot, 0);
}

// ---- the head's Fisher metric times a tangent -------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(256) void fisher_head_gaussian_kernel(const float *__restrict__ dd, const int64_t ldd,
                                                                   const float *__restrict__ log_std, const float *__restrict__ v_log_std,
                                                                   const int64_t B, float *__restrict__ up, float *__restrict__ g_log_std)
{
    float m[A];
    const float rows = (float)B;
#pragma unroll
    for (int k = 0; k < A; ++k) m[k] = expf(-2.0f * log_std[k]);
    for (int64_t b = blockIdx.x * 256ll + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256ll) {
        float t[A], u[A];
        load_row<A>(dd + b * ldd, t);
#pragma unroll
        for (int k = 0; k < A; ++k) u[k] = (t[k] * m[k]) / rows;
        store_row<A>(up + b * A, u);
    }
    if (blockIdx.x == 0 && threadIdx.x < A) g_log_std[threadIdx.x] = 2.0f * v_log_std[threadIdx.x];
}

template <int W>
__global__ __launch_bounds__(256) void fisher_head_discrete_kernel(const float *__restrict__ dd, const int64_t ldd, const float *__restrict__ dist,
                                                                   const int64_t ld, const int k0, const int k1, const int64_t B,
                                                                   float *__restrict__ up)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = lane / W, j = lane % W;
    const int K = seg ? k1 : k0, col = seg ? k0 + j : j, width = W == 64 ? k0 : k0 + k1;
    const bool valid = j < K;
    const float rows = (float)B;
    for (int64_t b = blockIdx.x * (int64_t)ROWS_PER_BLOCK + wave; b < B; b += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
        const float z = valid ? dist[b * ld + col] : -INFINITY;
        const float zd = valid ? dd[b * ldd + col] : 0.0f;
        const float mx = seg_max<W>(z);
        const float e = expf(z - mx);  // a padded lane: expf(-inf) = 0
        const float pr = e / seg_sum<W>(e);
        const float pz = pr * zd;
        const float dot = seg_sum<W>(pz);
        if (valid) up[b * width + col] = (pz - pr * dot) / rows;
    }
}

// ---- conjugate gradient: one single-workgroup launch per iteration ----------------------------------------------------------------------
__device__ __forceinline__ double cg_block_sum(double v, double *red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = CG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(CG_THREADS) void trpo_cg_kernel(const int mode, float *__restrict__ x, float *__restrict__ r, float *__restrict__ p,
                                                             const float *__restrict__ ap, const float *__restrict__ g, const int64_t n,
                                                             const double damping, const double tol, const double target_kl, const int last,
                                                             double *__restrict__ ctl)
{
    __shared__ double red[CG_THREADS];
    const int64_t t = threadIdx.x;
    if (mode == CSTR_TRPO_CG_INIT) {
        double s = 0.0;
        for (int64_t i = t; i < n; i += CG_THREADS) {
            const float rv = (float)((double)g[i] - ((double)ap[i] + damping * (double)x[i]));
            r[i] = rv;
            p[i] = rv;
            s += (double)rv * (double)rv;
        }
        const double rr = cg_block_sum(s, red);
        if (t == 0) {
            ctl[CSTR_TRPO_CTL_RR] = rr;
            ctl[CSTR_TRPO_CTL_DONE] = rr < tol ? 1.0 : 0.0;
            ctl[CSTR_TRPO_CTL_ITERS] = 0.0;
        }
        return;
    }
    if (mode == CSTR_TRPO_CG_FINISH) {
        double s = 0.0;
        for (int64_t i = t; i < n; i += CG_THREADS) s += (double)x[i] * ((double)ap[i] + damping * (double)x[i]);
        const double sfs = cg_block_sum(s, red);
        if (t == 0) {
            ctl[CSTR_TRPO_CTL_SFS] = sfs;
            ctl[CSTR_TRPO_CTL_STEP] = sqrt(2.0 * target_kl / sfs);
            ctl[CSTR_TRPO_CTL_COEFF] = 1.0;
        }
        return;
    }
    if (ctl[CSTR_TRPO_CTL_DONE] != 0.0) return;  // uniform over the workgroup: nobody has written the block yet
    const double rr = ctl[CSTR_TRPO_CTL_RR];
    double s = 0.0;
    for (int64_t i = t; i < n; i += CG_THREADS) s += (double)p[i] * ((double)ap[i] + damping * (double)p[i]);
    const double pap = cg_block_sum(s, red);  // behind its barriers every thread has read DONE and RR
    const double alpha = rr / pap;
    double q = 0.0;
    for (int64_t i = t; i < n; i += CG_THREADS) {
        const double pv = (double)p[i];
        x[i] = (float)((double)x[i] + alpha * pv);
        if (!last) {
            const float rv = (float)((double)r[i] - alpha * ((double)ap[i] + damping * pv));
            r[i] = rv;
            q += (double)rv * (double)rv;
        }
    }
    if (last) {
        if (t == 0) {
            ctl[CSTR_TRPO_CTL_PAP] = pap;
            ctl[CSTR_TRPO_CTL_ALPHA] = alpha;
            ctl[CSTR_TRPO_CTL_DONE] = 1.0;
            ctl[CSTR_TRPO_CTL_ITERS] += 1.0;
        }
        return;
    }
    const double new_rr = cg_block_sum(q, red);
    const bool stop = new_rr < tol;
    const double beta = new_rr / rr;
    if (!stop)
        for (int64_t i = t; i < n; i += CG_THREADS) p[i] = (float)((double)r[i] + beta * (double)p[i]);
    if (t == 0) {
        ctl[CSTR_TRPO_CTL_PAP] = pap;
        ctl[CSTR_TRPO_CTL_ALPHA] = alpha;
        ctl[CSTR_TRPO_CTL_ITERS] += 1.0;
        if (stop) {
            ctl[CSTR_TRPO_CTL_DONE] = 1.0;
        } else {
            ctl[CSTR_TRPO_CTL_BETA] = beta;
            ctl[CSTR_TRPO_CTL_RR] = new_rr;
        }
    }
}

__global__ __launch_bounds__(256) void trpo_apply_step_kernel(float *__restrict__ theta, const float *__restrict__ theta0,
                                                              const float *__restrict__ s, const float *__restrict__ mask, const int64_t n,
                                                              const double *__restrict__ ctl)
{
    const double cs = ctl[CSTR_TRPO_CTL_COEFF] * ctl[CSTR_TRPO_CTL_STEP];
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256ll)
        if (mask[i] != 0.0f) theta[i] = (float)((double)theta0[i] + cs * (double)s[i]);
}

__global__ __launch_bounds__(256) void trpo_value_loss_kernel(const float *__restrict__ values, const float *__restrict__ returns, const int64_t B,
                                                              float *__restrict__ g_value, float *__restrict__ loss_out,
                                                              float *__restrict__ loss_sum)
{
    __shared__ double red[256];
    const double inv_b = 1.0 / (double)B;
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += 256) {
        const double d = (double)values[b] - (double)returns[b];
        g_value[b] = (float)((2.0 * d) * inv_b);
        s += d * d;
    }
    const double tot = block_sum_f64(s, red);
    if (threadIdx.x == 0) {
        const float loss = (float)(tot * inv_b);
        if (loss_out) loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
    }
}

__global__ __launch_bounds__(256) void trpo_x0_kernel(float *__restrict__ x, const float *__restrict__ mask, const int64_t n, const float scale,
                                                      uint64_t *__restrict__ rng_ctl)
{
    const uint64_t seed = rng_ctl[0], base = rng_ctl[1];
    const int64_t pairs = (n + 1) / 2;
    for (int64_t j = blockIdx.x * 256ll + threadIdx.x; j < pairs; j += (int64_t)gridDim.x * 256ll) {
        const uint64_t ctr = base + (uint64_t)j;
        uint32_t w[4];
        float z0, z1;
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, TRPO_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        box_muller(w[0], w[1], z0, z1);
        x[2 * j] = mask[2 * j] != 0.0f ? scale * z0 : 0.0f;
        if (2 * j + 1 < n) x[2 * j + 1] = mask[2 * j + 1] != 0.0f ? scale * z1 : 0.0f;
    }
    if (last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0) rng_ctl[1] = base + (uint64_t)pairs;
}

// the heads' shapes: 0 when taken. Gaussian: k0 = A in {2, 4}; categorical: 2 <= k0 <= 64; multi-categorical: 2 <= k0, k1 <= 32
inline int head_check(const int head, const int k0, const int k1)
{
    if (head == CSTR_TRPO_HEAD_GAUSSIAN) return (k0 == 2 || k0 == 4) ? 0 : CSTR_E_UNSUPPORTED;
    if (head == CSTR_TRPO_HEAD_CATEGORICAL) return (k0 >= 2 && k0 <= CSTR_TRPO_MAX_LOGITS) ? 0 : CSTR_E_UNSUPPORTED;
    if (head == CSTR_TRPO_HEAD_MULTICATEGORICAL) return (k0 >= 2 && k0 <= 32 && k1 >= 2 && k1 <= 32) ? 0 : CSTR_E_UNSUPPORTED;
    return CSTR_E_UNSUPPORTED;
}

inline int head_width(const int head, const int k0, const int k1) { return head == CSTR_TRPO_HEAD_MULTICATEGORICAL ? k0 + k1 : k0; }

// a [rows][width] matrix with row stride ld read by the head's loads: the Gaussian rows move as one vector
inline bool dist_rows_ok(const int head, const float *p, const int64_t ld, const int width)
{
    if (ld < width) return false;
    if (head != CSTR_TRPO_HEAD_GAUSSIAN) return aligned4(p);
    return row_aligned(p, width) && (ld * 4) % (width == 4 ? 16 : 8) == 0;
}

}  // namespace

extern "C" int cstr_linear_tangent_fwd_f32(const float *x, int64_t ldx, const float *x_dot, int64_t ldxd, const float *w, const float *w_dot,
                                           const float *b_dot, const float *y, int act, float *z_dot, int64_t m, int64_t n, int64_t k,
                                           cstr_stream_t stream)
{
    if (!x || !w || !w_dot || !b_dot || !z_dot || m <= 0 || n <= 0 || k <= 0 || ldx < k || (x_dot && ldxd < k)) return CSTR_E_BADARG;
    if (act < 0 || act > 2) return CSTR_E_UNSUPPORTED;
    if (act != 0 && !y) return CSTR_E_BADARG;
    if (m > 0x7fffff || n > 0x7fffff || k > 0x7fffff || (m + 15) / 16 > 65535) return CSTR_E_UNSUPPORTED;
    if (ldx > 0x7fffffff || (x_dot && ldxd > 0x7fffffff)) return CSTR_E_UNSUPPORTED;  // the kernel carries the row strides as int
    const void *all[7] = {x, x_dot, w, w_dot, b_dot, y, z_dot};
    for (int i = 0; i < 7; ++i)
        if (all[i] && !aligned4(all[i])) return CSTR_E_BADARG;
    {
        const Buf ins[6] = {{x, span(m, ldx, k)}, {x_dot, x_dot ? span(m, ldxd, k) : 0}, {w, n * k}, {w_dot, n * k}, {b_dot, n},
                            {act ? y : nullptr, m * n}};
        const Buf outs[1] = {{z_dot, m * n}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    const dim3 grid((unsigned)((n + 15) / 16), (unsigned)((m + 15) / 16));
    const bool vec = (k & 3) == 0 && (ldx & 3) == 0 && aligned16(x) && aligned16(w) && aligned16(w_dot) &&
                     (!x_dot || ((ldxd & 3) == 0 && aligned16(x_dot)));
    hipStream_t s = (hipStream_t)stream;
#define TAN(A, V, X) linear_tangent_fwd_kernel<A, V, X><<<grid, 64, 0, s>>>(x, x_dot, w, w_dot, (int)ldx, (int)ldxd, (int)m, (int)n, (int)k, b_dot, y, z_dot)
#define TAN_X(A, V) do { if (x_dot) TAN(A, V, true); else TAN(A, V, false); } while (0)
#define TAN_ACT(V) do { if (act == 0) TAN_X(0, V); else if (act == 1) TAN_X(1, V); else TAN_X(2, V); } while (0)
    if (vec) TAN_ACT(true); else TAN_ACT(false);
#undef TAN_ACT
#undef TAN_X
#undef TAN
    return (int)hipGetLastError();
}

extern "C" int cstr_trpo_objective_f32(const cstr_trpo_objective_t *p, uint64_t *workspace, cstr_stream_t stream)
{
    if (!p || !workspace) return CSTR_E_BADARG;
    if (!p->dist || !p->old_dist || !p->actions || !p->old_log_prob || !p->adv || !p->ctl || p->batch <= 0) return CSTR_E_BADARG;
    const bool gauss = p->head == CSTR_TRPO_HEAD_GAUSSIAN;
    if (gauss && (!p->log_std || !p->old_log_std)) return CSTR_E_BADARG;
    if (p->line_search) {
        if (!p->accepted || !(p->target_kl > 0.0) || !(p->shrink > 0.0 && p->shrink < 1.0)) return CSTR_E_BADARG;
    } else if (!p->g_dist || (gauss && !p->g_log_std)) {
        return CSTR_E_BADARG;
    }
    const int rc = head_check(p->head, p->k0, p->k1);
    if (rc) return rc;
    if (p->batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    const int width = head_width(p->head, p->k0, p->k1);
    const int aw = gauss ? p->k0 : (p->head == CSTR_TRPO_HEAD_CATEGORICAL ? 1 : 2);  // floats per action row
    if (!dist_rows_ok(p->head, p->dist, p->ld, width) || !dist_rows_ok(p->head, p->old_dist, p->old_ld, width)) return CSTR_E_BADARG;
    if (!row_aligned(p->actions, aw) || !aligned4(p->old_log_prob) || !aligned4(p->adv) || !aligned8(p->ctl) || !aligned8(workspace) ||
        (p->scalars_out && !aligned4(p->scalars_out)))
        return CSTR_E_BADARG;
    if (gauss && (!aligned4(p->log_std) || !aligned4(p->old_log_std))) return CSTR_E_BADARG;
    const int64_t B = p->batch;
    float *g_dist = p->line_search ? nullptr : p->g_dist, *g_log_std = (p->line_search || !gauss) ? nullptr : p->g_log_std;
    if (g_dist && !(gauss ? row_aligned(g_dist, width) : aligned4(g_dist))) return CSTR_E_BADARG;
    if (g_log_std && !aligned4(g_log_std)) return CSTR_E_BADARG;
    if (p->line_search && !aligned4(p->accepted)) return CSTR_E_BADARG;
    {
        const Buf ins[7] = {{p->dist, span(B, p->ld, width)}, {p->old_dist, span(B, p->old_ld, width)}, {gauss ? p->log_std : nullptr, width},
                            {gauss ? p->old_log_std : nullptr, width}, {p->actions, B * aw}, {p->old_log_prob, B}, {p->adv, B}};
        const Buf outs[6] = {{g_dist, B * width}, {g_log_std, width}, {p->scalars_out, 2}, {p->ctl, 2 * CSTR_TRPO_CTL_WORDS},
                             {p->line_search ? p->accepted : nullptr, 1}, {workspace, 2 * CSTR_PPO_WS_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    cstr_trpo_objective_t k = *p;
    k.g_dist = g_dist;
    k.g_log_std = g_log_std;
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (gauss) {
        const unsigned grid = lane_grid(B, 256, CSTR_PPO_MAX_BLOCKS);
        if (p->k0 == 2) trpo_objective_gaussian_kernel<2><<<grid, 256, 0, s>>>(k, ws);
        else trpo_objective_gaussian_kernel<4><<<grid, 256, 0, s>>>(k, ws);
    } else {
        const unsigned grid = row_grid(B, CSTR_PPO_MAX_BLOCKS);
        if (p->head == CSTR_TRPO_HEAD_CATEGORICAL) trpo_objective_discrete_kernel<64><<<grid, 256, 0, s>>>(k, ws);
        else trpo_objective_discrete_kernel<32><<<grid, 256, 0, s>>>(k, ws);
    }
    return (int)hipGetLastError();
}

extern "C" int cstr_trpo_fisher_head_f32(int head, int k0, int k1, const float *dist_dot, int64_t ldd, const float *dist, int64_t ld,
                                         const float *log_std, const float *v_log_std, int64_t batch, float *upstream, float *g_log_std,
                                         cstr_stream_t stream)
{
    if (!dist_dot || !upstream || batch <= 0) return CSTR_E_BADARG;
    const bool gauss = head == CSTR_TRPO_HEAD_GAUSSIAN;
    if (gauss ? (!log_std || !v_log_std || !g_log_std) : !dist) return CSTR_E_BADARG;
    const int rc = head_check(head, k0, k1);
    if (rc) return rc;
    if (batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    const int width = head_width(head, k0, k1);
    if (!dist_rows_ok(head, dist_dot, ldd, width) || (!gauss && !dist_rows_ok(head, dist, ld, width))) return CSTR_E_BADARG;
    if (!(gauss ? row_aligned(upstream, width) : aligned4(upstream))) return CSTR_E_BADARG;
    if (gauss && (!aligned4(log_std) || !aligned4(v_log_std) || !aligned4(g_log_std))) return CSTR_E_BADARG;
    {
        const Buf ins[4] = {{dist_dot, span(batch, ldd, width)}, {gauss ? nullptr : dist, gauss ? 0 : span(batch, ld, width)},
                            {gauss ? log_std : nullptr, width}, {gauss ? v_log_std : nullptr, width}};
        const Buf outs[2] = {{upstream, batch * width}, {gauss ? g_log_std : nullptr, width}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (gauss) {
        const unsigned grid = lane_grid(batch, 256, 1024);
        if (k0 == 2) fisher_head_gaussian_kernel<2><<<grid, 256, 0, s>>>(dist_dot, ldd, log_std, v_log_std, batch, upstream, g_log_std);
        else fisher_head_gaussian_kernel<4><<<grid, 256, 0, s>>>(dist_dot, ldd, log_std, v_log_std, batch, upstream, g_log_std);
    } else {
        const unsigned grid = row_grid(batch, 4096);
        if (head == CSTR_TRPO_HEAD_CATEGORICAL) fisher_head_discrete_kernel<64><<<grid, 256, 0, s>>>(dist_dot, ldd, dist, ld, k0, k1, batch, upstream);
        else fisher_head_discrete_kernel<32><<<grid, 256, 0, s>>>(dist_dot, ldd, dist, ld, k0, k1, batch, upstream);
    }
    return (int)hipGetLastError();
}

extern "C" int cstr_trpo_cg_step_f32(int mode, float *x, float *r, float *p, const float *ap, const float *g, int64_t n, double damping,
                                     double residual_tol, double target_kl, int last, double *ctl, cstr_stream_t stream)
{
    if (mode != CSTR_TRPO_CG_INIT && mode != CSTR_TRPO_CG_STEP && mode != CSTR_TRPO_CG_FINISH) return CSTR_E_BADARG;
    if (!x || !ap || !ctl || n <= 0 || !(damping >= 0.0) || !(residual_tol >= 0.0)) return CSTR_E_BADARG;
    if (mode != CSTR_TRPO_CG_FINISH && (!r || !p)) return CSTR_E_BADARG;
    if (mode == CSTR_TRPO_CG_INIT && !g) return CSTR_E_BADARG;
    if (mode == CSTR_TRPO_CG_FINISH && !(target_kl > 0.0)) return CSTR_E_BADARG;
    if (n > CSTR_TRPO_MAX_VECTOR) return CSTR_E_UNSUPPORTED;
    if (mode == CSTR_TRPO_CG_FINISH) r = p = nullptr;
    if (mode != CSTR_TRPO_CG_INIT) g = nullptr;
    const void *f32[5] = {x, r, p, ap, g};
    for (int i = 0; i < 5; ++i)
        if (f32[i] && !aligned4(f32[i])) return CSTR_E_BADARG;
    if (!aligned8(ctl)) return CSTR_E_BADARG;
    {
        const Buf ins[2] = {{ap, n}, {g, n}};
        const Buf outs[4] = {{x, n}, {r, n}, {p, n}, {ctl, 2 * CSTR_TRPO_CTL_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    trpo_cg_kernel<<<1, CG_THREADS, 0, (hipStream_t)stream>>>(mode, x, r, p, ap, g, n, damping, residual_tol, target_kl, last ? 1 : 0, ctl);
    return (int)hipGetLastError();
}

extern "C" int cstr_trpo_apply_step_f32(float *theta, const float *theta0, const float *s, const float *mask, int64_t n, const double *ctl,
                                        cstr_stream_t stream)
{
    if (!theta || !theta0 || !s || !mask || !ctl || n <= 0) return CSTR_E_BADARG;
    if (n > CSTR_TRPO_MAX_VECTOR) return CSTR_E_UNSUPPORTED;
    if (!aligned4(theta) || !aligned4(theta0) || !aligned4(s) || !aligned4(mask) || !aligned8(ctl)) return CSTR_E_BADARG;
    {
        const Buf ins[4] = {{theta0, n}, {s, n}, {mask, n}, {ctl, 2 * CSTR_TRPO_CTL_WORDS}};
        const Buf outs[1] = {{theta, n}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    trpo_apply_step_kernel<<<lane_grid(n, 256, 1024), 256, 0, (hipStream_t)stream>>>(theta, theta0, s, mask, n, ctl);
    return (int)hipGetLastError();
}

extern "C" int cstr_trpo_value_loss_f32(const float *values, const float *returns, int64_t batch, float *g_value, float *loss_out,
                                        float *loss_sum, cstr_stream_t stream)
{
    if (!values || !returns || !g_value || batch <= 0) return CSTR_E_BADARG;
    if (batch > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!aligned4(values) || !aligned4(returns) || !aligned4(g_value) || (loss_out && !aligned4(loss_out)) || (loss_sum && !aligned4(loss_sum)))
        return CSTR_E_BADARG;
    {
        const Buf ins[2] = {{values, batch}, {returns, batch}};
        const Buf outs[3] = {{g_value, batch}, {loss_out, 1}, {loss_sum, 1}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    trpo_value_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(values, returns, batch, g_value, loss_out, loss_sum);
    return (int)hipGetLastError();
}

extern "C" int cstr_trpo_x0_f32(float *x, const float *mask, int64_t n, float scale, uint64_t *rng_ctl, cstr_stream_t stream)
{
    if (!x || !mask || !rng_ctl || n <= 0) return CSTR_E_BADARG;
    if (n > CSTR_TRPO_MAX_VECTOR) return CSTR_E_UNSUPPORTED;
    if (!aligned4(x) || !aligned4(mask) || !aligned8(rng_ctl)) return CSTR_E_BADARG;
    {
        const Buf ins[1] = {{mask, n}};
        const Buf outs[2] = {{x, n}, {rng_ctl, 2 * CSTR_RNG_CTL_WORDS}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    trpo_x0_kernel<<<lane_grid((n + 1) / 2, 256, 1024), 256, 0, (hipStream_t)stream>>>(x, mask, n, scale, rng_ctl);
    return (int)hipGetLastError();
}
