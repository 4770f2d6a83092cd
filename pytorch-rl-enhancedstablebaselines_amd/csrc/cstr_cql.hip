// cstr_cql.hip -- CQL's own arithmetic around SAC's gradient step (Kumar et al. 2020, the importance-sampled CQL(H) term of the
// published SAC-based implementation; core/cql/cql.py), f32, gfx950:
//   * the candidate actions of the conservative term: per state N uniform actions, N samples of pi(.|s) and N samples of pi(.|s'), from
//     the actor's distribution parameters of s and s' (ONE trunk pass per state, no repeated rows), written next to the state's
//     observation into 3N contiguous critic-input rows, with the three importance corrections (A log 0.5, log pi(a|s), log pi(a|s'));
//   * everything between the critic's forward on [data rows | candidate rows] and its backward: the TD target (the twin TD loss head's
//     statement and rounding points, csrc/cstr_mlp.hip td_twin_q_loss_kernel), the Bellman term, T * logsumexp(c / T) over a state's
//     3N (+1) entries with its softmax gradient, the logged scalars.
// A sampled action and its log-prob are the device functions of cstr_gaussian_device.h summed over the action dimension in
// gaussian_head_fwd_kernel's order (ascending j, the Gaussian terms and the tanh corrections in two sums, logp = lp - corr), so a
// candidate drawn with eps = e has the bits a SAC head launch gives for the same (mean, raw, e).
// Noise is READ when given and DRAWN otherwise: Philox4x32-10 keyed by rng_ctl[0], counter (rng_ctl[1] + b N + k, sub, CQL tag); the
// last workgroup advances rng_ctl[1] by B N, so a graph replay draws fresh noise. No float atomics: the loss launch is ONE 1024-thread
// workgroup whose sixteen waves stride over the states, a wave holds a state's entries in its lanes, both critics side by side (maximum,
// sum and broadcast through xor-shuffles: the launch waits for shuffle chains, so the two critics' chains are interleaved), and
// accumulates the batch sums in float64 in a fixed order. Nothing here allocates, synchronises or keeps host state.
// Access width: rows of D + A = 6 floats leave most of them off 16-byte boundaries and both launches are launch-latency bound at the
// learner's sizes (<= 31 * 256 rows), so the loops are scalar; a state's candidate rows and its 3N q values are contiguous, which is
// what the loss reads with one coalesced request per critic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_gaussian_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t CQL_STREAM_TAG = 0xC0175E4Au;  // counter word 3: never shares counters with the other heads' streams

// One thread per output row r = b * 3N + j: kind = j / N (0 uniform, 1 pi(.|s_b), 2 pi(.|s'_b)), sample k = j % N.
// Drawn noise, counter c = offset + b N + k: (c, sub 0) words 0..3 -> the uniform action's columns 0..3 as 2 * ((w >> 8) * 2^-24) - 1;
// (c, sub 1 + p) -> Box-Muller(words 0, 1) = eps of pi(.|s)'s columns 2p, 2p + 1 and Box-Muller(words 2, 3) = eps of pi(.|s')'s.
__global__ __launch_bounds__(256) void cql_candidates_kernel(const float *__restrict__ obs, const int64_t ldo,
                                                             const float *__restrict__ params_cur, const float *__restrict__ params_next,
                                                             const int64_t ldp, const float *__restrict__ u_in,
                                                             const float *__restrict__ eps_in, uint64_t *__restrict__ rng_ctl,
                                                             const float log_unif, float *__restrict__ x, const int64_t ldx,
                                                             float *__restrict__ corr, const int64_t batch, const int N, const int D,
                                                             const int A)
{
    const uint64_t seed = rng_ctl ? rng_ctl[0] : 0ull, base = rng_ctl ? rng_ctl[1] : 0ull;
    const int n3 = 3 * N;
    const int64_t rows = batch * n3;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = r / n3;
        const int j = (int)(r - b * n3);
        const int kind = j / N, k = j - kind * N;
        float *xr = x + r * ldx;
        const float *o = obs + b * ldo;
        for (int c = 0; c < D; ++c) xr[c] = o[c];
        const uint64_t ctr = base + (uint64_t)(b * N + k);
        if (kind == 0) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (rng_ctl) philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, CQL_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), w);
            for (int c = 0; c < A; ++c)
                xr[D + c] = rng_ctl ? 2.0f * philox_uniform(w[c]) - 1.0f : u_in[(b * N + k) * A + c];
            if (corr) corr[r] = log_unif;
            continue;
        }
        const float *pr = (kind == 1 ? params_cur : params_next) + b * ldp;
        const float *er = eps_in ? eps_in + ((b * 2 * N) + (kind - 1) * N + k) * A : nullptr;
        float lp = 0.0f, tc = 0.0f;
        for (int c0 = 0; c0 < A; c0 += 2) {
            float e[2] = {0.0f, 0.0f};
            if (rng_ctl) {
                uint32_t w[4];
                philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 1u + (uint32_t)(c0 >> 1), CQL_STREAM_TAG, (uint32_t)seed,
                              (uint32_t)(seed >> 32), w);
                if (kind == 1) box_muller(w[0], w[1], e[0], e[1]);
                else box_muller(w[2], w[3], e[0], e[1]);
            }
            for (int cc = 0; cc < 2 && c0 + cc < A; ++cc) {
                const int c = c0 + cc;
                if (!rng_ctl) e[cc] = er[c];
                const float mu = pr[c], raw = pr[A + c];
                float a, s, u;
                sample_action_act(mu, raw, e[cc], a, s, u);
                xr[D + c] = a;
                lp += gaussian_logp_term(mu, s, u);
                tc += tanh_correction_term(a);
            }
        }
        if (corr) corr[r] = lp - tc;
    }
    if (rng_ctl && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0)
        rng_ctl[1] = base + (uint64_t)(batch * N);
}

constexpr int QL_WAVES = 16, QL_THREADS = 64 * QL_WAVES;  // the loss launch's one workgroup

// both critics' butterflies side by side: two independent shuffle chains per step instead of one after the other
__device__ __forceinline__ void wave_max_all_2(float &a, float &b)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ta = __shfl_xor(a, o, 64), tb = __shfl_xor(b, o, 64);
        a = fmaxf(a, ta);
        b = fmaxf(b, tb);
    }
}

__device__ __forceinline__ void wave_sum_all_2(float &a, float &b)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ta = __shfl_xor(a, o, 64), tb = __shfl_xor(b, o, 64);
        a += ta;
        b += tb;
    }
}

// the sixteen wave sums of one quantity in a fixed binary tree: neighbours, then pairs of pairs, ... ((s0 + s1) + (s2 + s3)) + ...
__device__ __forceinline__ double tree_16(const double *v)
{
    double t[QL_WAVES];
#pragma unroll
    for (int i = 0; i < QL_WAVES; ++i) t[i] = v[i];
#pragma unroll
    for (int w = 1; w < QL_WAVES; w <<= 1)
#pragma unroll
        for (int i = 0; i < QL_WAVES; i += 2 * w) t[i] = t[i] + t[i + w];
    return t[0];
}

// Wave v of 16 takes the states v, v + 16, ... in ascending order, both critics of a state side by side. The n = 3N (+1 with_data)
// entries of a (state, critic) sit in lanes 0 .. n-1: c_j = q_cand[j] - corr[j] (no correction without corr), the last one Q(s, a) itself
// when with_data. z = c / T; m = max_j z (an infinite m is replaced by 0, as torch.logsumexp); e_j = exp(z_j - m); s = sum_j e_j
// (xor-shuffle butterfly, offsets 32 .. 1: every lane ends with the same bits); lse = T * (log(s) + m); softmax_j = e_j / s. A NaN entry
// leaves the maximum (fmaxf drops it) and enters the sum, so lse, every softmax share of that state and the loss are NaN.
__global__ __launch_bounds__(QL_THREADS) void cql_q_loss_kernel(const float *__restrict__ q, const int64_t q_stride,
                                                                const float *__restrict__ corr, const int with_data,
                                                                const float *__restrict__ q1_t, const float *__restrict__ q2_t,
                                                                const float *__restrict__ next_logp, const float *__restrict__ rew,
                                                                const float *__restrict__ done, const float *__restrict__ ent_coef,
                                                                const float gamma, const float w, const float temp,
                                                                float *__restrict__ target_out, float *__restrict__ gq,
                                                                float *__restrict__ loss_out, float *__restrict__ loss_sum,
                                                                float *__restrict__ aux, const int batch, const int N)
{
    __shared__ double sm[6][QL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n3 = 3 * N, n = n3 + (with_data ? 1 : 0);
    const int64_t rows = (int64_t)batch * (1 + n3);
    const float ec = ent_coef ? ent_coef[0] : 0.0f;
    const float k = 0.5f * 2.0f / (float)batch;  // the twin TD loss head's scale * 2 / B at SAC's scale 0.5
    const float hw = (0.5f * w) / (float)batch;
    const float *q0p = q, *q1p = q + q_stride;
    float *g0p = gq, *g1p = gq + rows;
    double a_bell[2] = {0.0, 0.0}, a_lse[2] = {0.0, 0.0}, a_q[2] = {0.0, 0.0};
    for (int b = wave; b < batch; b += QL_WAVES) {
        const int64_t row = (int64_t)batch + (int64_t)b * n3 + lane;
        // every load of the state in front of the arithmetic
        const float t1 = q1_t[b], t2 = q2_t[b], nl = next_logp ? next_logp[b] : 0.0f, r = rew[b], dn = done[b];
        const float cr = (corr && lane < n3) ? corr[(int64_t)b * n3 + lane] : 0.0f;
        const float qd0 = q0p[b], qd1 = q1p[b];
        const float qc0 = lane < n3 ? q0p[row] : 0.0f, qc1 = lane < n3 ? q1p[row] : 0.0f;
        float qn = fminf(t1, t2);
        if (next_logp) qn = qn - ec * nl;
        const float t = r + (1.0f - dn) * gamma * qn;
        if (target_out && lane == 0) target_out[b] = t;
        float c0 = -INFINITY, c1 = -INFINITY;
        if (lane < n3) { c0 = qc0 - cr; c1 = qc1 - cr; }
        else if (lane < n) { c0 = qd0; c1 = qd1; }
        const float z0 = c0 / temp, z1 = c1 / temp;
        float m0 = z0, m1 = z1;
        wave_max_all_2(m0, m1);
        if (isinf(m0)) m0 = 0.0f;
        if (isinf(m1)) m1 = 0.0f;
        const float e0 = lane < n ? expf(z0 - m0) : 0.0f, e1 = lane < n ? expf(z1 - m1) : 0.0f;
        float s0 = e0, s1 = e1;
        wave_sum_all_2(s0, s1);
        const float lse0 = temp * (logf(s0) + m0), lse1 = temp * (logf(s1) + m1);
        const float p0 = e0 / s0, p1 = e1 / s1;
        if (lane < n3) { g0p[row] = hw * p0; g1p[row] = hw * p1; }
        const float d0 = qd0 - t, d1 = qd1 - t;
        // the appended entry's share (read by every lane: no divergent shuffle)
        const float pd0 = __shfl(p0, n3 & 63, 64), pd1 = __shfl(p1, n3 & 63, 64);
        if (lane == 0) {
            g0p[b] = with_data ? (k * d0 - hw) + hw * pd0 : k * d0 - hw;
            g1p[b] = with_data ? (k * d1 - hw) + hw * pd1 : k * d1 - hw;
        }
        a_bell[0] += (double)d0 * (double)d0;
        a_bell[1] += (double)d1 * (double)d1;
        a_lse[0] += (double)lse0;
        a_lse[1] += (double)lse1;
        a_q[0] += (double)qd0;
        a_q[1] += (double)qd1;
    }
    // every lane of a wave carries the wave's sums (the butterflies left all lanes with the same values)
    if (lane == 0) {
        sm[0][wave] = a_bell[0]; sm[1][wave] = a_bell[1];
        sm[2][wave] = a_lse[0];  sm[3][wave] = a_lse[1];
        sm[4][wave] = a_q[0];    sm[5][wave] = a_q[1];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double fb = (double)batch;
        const double bell0 = tree_16(sm[0]), bell1 = tree_16(sm[1]), lse0 = tree_16(sm[2]), lse1 = tree_16(sm[3]);
        const double q0 = tree_16(sm[4]), q1 = tree_16(sm[5]);
        const double bell = 0.5 * (bell0 / fb + bell1 / fb);
        const double cons = 0.5 * (double)w * ((lse0 / fb - q0 / fb) + (lse1 / fb - q1 / fb));
        const float loss = (float)(bell + cons);
        if (loss_out) loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
        if (aux) {
            aux[0] = (float)bell;
            aux[1] = (float)cons;
            aux[2] = (float)(0.5 * (lse0 / fb + lse1 / fb));
            aux[3] = (float)(0.5 * (q0 / fb + q1 / fb));
        }
    }
}

inline bool overlap(const void *a, int64_t a_floats, const void *b, int64_t b_floats)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 4u * (uintptr_t)b_floats && b0 < a0 + 4u * (uintptr_t)a_floats;
}

// floats spanned by `rows` rows of `width` floats with row stride ld
inline int64_t span(int64_t rows, int64_t ld, int64_t width) { return (rows - 1) * ld + width; }

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// every output against every input and every other output
inline bool any_overlap(const void *const *ins, const int64_t *in_n, int n_in, const void *const *outs, const int64_t *out_n, int n_out)
{
    for (int o = 0; o < n_out; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < n_in; ++i)
            if (ins[i] && overlap(outs[o], out_n[o], ins[i], in_n[i])) return true;
        for (int p = o + 1; p < n_out; ++p)
            if (outs[p] && overlap(outs[o], out_n[o], outs[p], out_n[p])) return true;
    }
    return false;
}

}  // namespace

extern "C" int cstr_cql_candidates_f32(const float *obs, int64_t ldo, const float *params_cur, const float *params_next, int64_t ldp,
                                       int64_t batch, int n_actions, int obs_dim, int act_dim, const float *u_in, const float *eps_in,
                                       uint64_t *rng_ctl, float log_unif, float *x, int64_t ldx, float *corr, cstr_stream_t stream)
{
    if (!obs || !params_cur || !params_next || !x || batch <= 0 || n_actions <= 0 || obs_dim <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if (ldo < obs_dim || ldp < 2 * (int64_t)act_dim || ldx < (int64_t)obs_dim + act_dim) return CSTR_E_BADARG;
    const bool given = u_in || eps_in;
    if ((given && rng_ctl) || (!given && !rng_ctl) || (given && (!u_in || !eps_in))) return CSTR_E_BADARG;  // exactly one noise source
    if (act_dim > CSTR_MAX_HEAD_ACT || n_actions > CSTR_CQL_MAX_ACTIONS) return CSTR_E_UNSUPPORTED;
    if (batch > CSTR_BCQ_MAX_ROWS / (3 * (int64_t)n_actions)) return CSTR_E_UNSUPPORTED;
    if (!aligned4(obs) || !aligned4(params_cur) || !aligned4(params_next) || !aligned4(u_in) || !aligned4(eps_in) || !aligned4(x) ||
        !aligned4(corr) || (rng_ctl && !aligned8(rng_ctl)))
        return CSTR_E_BADARG;
    const int64_t n3 = 3 * (int64_t)n_actions, rows = batch * n3;
    const void *ins[6] = {obs, params_cur, params_next, u_in, eps_in, rng_ctl};
    const int64_t in_n[6] = {span(batch, ldo, obs_dim), span(batch, ldp, 2 * act_dim), span(batch, ldp, 2 * act_dim),
                             batch * n_actions * act_dim, batch * 2 * n_actions * act_dim, 2 * CSTR_RNG_CTL_WORDS};
    const void *outs[2] = {x, corr};
    const int64_t out_n[2] = {span(rows, ldx, obs_dim + act_dim), rows};
    if (any_overlap(ins, in_n, 6, outs, out_n, 2)) return CSTR_E_BADARG;
    const int64_t g = (rows + 255) / 256;
    cql_candidates_kernel<<<(unsigned)(g < 4096 ? g : 4096), 256, 0, (hipStream_t)stream>>>(obs, ldo, params_cur, params_next, ldp, u_in, eps_in,
                                                                                           rng_ctl, log_unif, x, ldx, corr, batch, n_actions,
                                                                                           obs_dim, act_dim);
    return (int)hipGetLastError();
}

extern "C" int cstr_cql_q_loss_f32(const float *q, int64_t q_stride, const float *corr, int with_data, const float *q1_t, const float *q2_t,
                                   const float *next_logp, const float *rew, const float *done, const float *ent_coef, float gamma, float w,
                                   float temp, float *target_out, float *gq, float *loss_out, float *loss_sum, float *aux, int64_t batch,
                                   int n_actions, cstr_stream_t stream)
{
    if (!q || !q1_t || !q2_t || !rew || !done || !gq || batch <= 0 || n_actions <= 0) return CSTR_E_BADARG;
    if ((with_data != 0 && with_data != 1) || (!corr && !with_data)) return CSTR_E_BADARG;  // the published variants: corrections, or Q(s, a) appended
    if (next_logp && !ent_coef) return CSTR_E_BADARG;
    if (!(w >= 0.0f) || !(temp > 0.0f) || gamma != gamma) return CSTR_E_BADARG;  // negative / non-positive or NaN
    if (n_actions > CSTR_CQL_MAX_ACTIONS || batch > CSTR_MAX_SAMPLE_BATCH) return CSTR_E_UNSUPPORTED;
    const int64_t n3 = 3 * (int64_t)n_actions, rows = batch * (1 + n3);
    if (q_stride < rows) return CSTR_E_BADARG;
    if (!aligned4(q) || !aligned4(corr) || !aligned4(q1_t) || !aligned4(q2_t) || !aligned4(next_logp) || !aligned4(rew) || !aligned4(done) ||
        !aligned4(ent_coef) || !aligned4(target_out) || !aligned4(gq) || !aligned4(loss_out) || !aligned4(loss_sum) || !aligned4(aux))
        return CSTR_E_BADARG;
    const void *ins[8] = {q, corr, q1_t, q2_t, next_logp, rew, done, ent_coef};
    const int64_t in_n[8] = {q_stride + rows, batch * n3, batch, batch, batch, batch, batch, 1};
    const void *outs[5] = {target_out, gq, loss_out, loss_sum, aux};
    const int64_t out_n[5] = {batch, 2 * rows, 1, 1, 4};
    if (any_overlap(ins, in_n, 8, outs, out_n, 5)) return CSTR_E_BADARG;
    cql_q_loss_kernel<<<1, QL_THREADS, 0, (hipStream_t)stream>>>(q, q_stride, corr, with_data, q1_t, q2_t, next_logp, rew, done, ent_coef, gamma, w, temp,
                                                          target_out, gq, loss_out, loss_sum, aux, (int)batch, n_actions);
    return (int)hipGetLastError();
}
