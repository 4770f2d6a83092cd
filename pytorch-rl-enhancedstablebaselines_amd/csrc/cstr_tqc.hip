// cstr_tqc.hip -- TQC's own arithmetic (Kuznetsov et al. 2020, "Controlling Overestimation Bias with Truncated Mixture of Continuous
// Distributional Quantile Critics"; core/tqc/tqc.py), f32 in and out, gfx950: what lies between the critics' forward passes of a
// gradient step and its backward passes. G critics of Nq atoms each, M = G * Nq <= 256 atoms per state, k atoms dropped per critic,
// n_keep = M - k * G. Atom tensors are [G][B][Nq], the layout the stacked GEMM of the critics' last layer leaves.
//
// cstr_tqc_critic_loss_f32, two launches behind one entry point:
//   rows kernel, ONE workgroup per batch row, one lane per atom (64, 128, 192 or 256 lanes):
//     * the row's M target atoms go to LDS; lane m counts rank_m = #{j : z'_j < z'_m or (z'_j == z'_m and j < m)}, a permutation of
//       0 .. M-1 whatever ties there are, so `rank < n_keep` keeps exactly n_keep atoms (float32 comparisons are exact);
//     * a kept atom's target y = r + (1 - d) gamma (z' - alpha logp') is evaluated in float64 and stored at LDS slot `rank`: the
//       targets lie ascending there (y is non-decreasing in z' for (1 - d) gamma >= 0) without a sorting pass;
//     * lane m walks the n_keep targets in ascending order: delta = y_j - z_m, the Huber term, the weight |tau_i - 1[delta < 0]| and the
//       two sums (loss, gradient) in float64. An f32 difference of atoms of size 100 would carry 1e-5 into a gradient term of size
//       <= 1 and can flip the |delta| <= 1 branch;
//     * three row sums (loss, kept targets, atoms) leave through a float64 shuffle tree and the wave sums in wave order.
//   finish kernel, one 256-lane workgroup: lane t adds the row sums of rows t, t + 256, ... in ascending order, the same tree, then
//     lane 0 writes the loss and the two logged means. SAC's entropy-coefficient part (cstr_alpha_part_t) rides here, in float64.
//   No float atomics and no workgroup that waits for another: a relaunch gives the same bits.
// cstr_tqc_actor_loss_f32, one 256-lane workgroup: loss = mean_b(alpha logp_b - mean_{g,i} z_pi), float64 row means and batch sum in
//   the finish kernel's order; the two gradients are constants.
// Nothing here allocates, synchronises or keeps host state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"

namespace {

constexpr int TQC_MAX_ATOMS = CSTR_TQC_MAX_ATOMS;

struct TqcCriticArgs {
    const float *z, *z_next, *next_logp, *rew, *done, *ent_coef, *log_alpha;
    double gamma;
    float *gz, *target_out;
    double *ws;
    int G, Nq, k, batch;
};

// Sum over the workgroup (1 to 4 waves of 64 lanes): shuffle tree with offsets 32, 16, ... 1, then the wave sums in wave order.
// Every lane of the workgroup calls it; the result is valid in lane 0.
__device__ __forceinline__ double block_sum_f64(double v, double *sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    double r = sm[0];
    for (int w = 1; w < waves; ++w) r += sm[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void tqc_critic_rows_kernel(const TqcCriticArgs a)
{
    __shared__ float s_zn[TQC_MAX_ATOMS];
    __shared__ double s_y[TQC_MAX_ATOMS];
    __shared__ double s_red[4];
    const int b = blockIdx.x, t = threadIdx.x, G = a.G, Nq = a.Nq, M = G * Nq, n_keep = M - a.k * G;
    const bool live = t < M;
    int i = 0;
    int64_t at = 0;
    float zc = 0.0f, zn = 0.0f;
    if (live) {
        const int g = t / Nq;
        i = t - g * Nq;
        at = ((int64_t)g * a.batch + b) * Nq + i;
        zc = a.z[at];
        zn = a.z_next[at];
        s_zn[t] = zn;
    }
    __syncthreads();
    int rank = 0;
    if (live)
        for (int j = 0; j < M; ++j) {
            const float v = s_zn[j];  // one address per wave: an LDS broadcast
            rank += (v < zn || (v == zn && j < t)) ? 1 : 0;
        }
    const double ec = a.log_alpha ? exp((double)a.log_alpha[0]) : (double)a.ent_coef[0];
    const double r = (double)a.rew[b], coef = (1.0 - (double)a.done[b]) * a.gamma, lp = (double)a.next_logp[b];
    const bool kept = live && rank < n_keep;
    double yv = 0.0;
    if (kept) {
        yv = r + coef * ((double)zn - ec * lp);
        s_y[rank] = yv;
        if (a.target_out) a.target_out[(int64_t)b * n_keep + rank] = (float)yv;
    }
    __syncthreads();
    double lsum = 0.0, gsum = 0.0;
    if (live) {
        const double tau = ((double)i + 0.5) / (double)Nq, w_neg = 1.0 - tau, zd = (double)zc;
        for (int j = 0; j < n_keep; ++j) {
            const double d = s_y[j] - zd, ad = fabs(d);
            const double w = d < 0.0 ? w_neg : tau;                 // |tau_i - 1[delta < 0]|
            const double h = ad <= 1.0 ? 0.5 * d * d : ad - 0.5;    // Huber, kappa = 1
            const double c = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d); // its derivative
            lsum += w * h;
            gsum += w * c;
        }
        a.gz[at] = (float)(-(gsum / ((double)a.batch * (double)M * (double)n_keep)));
    }
    const double s0 = block_sum_f64(lsum, s_red), s1 = block_sum_f64(yv, s_red), s2 = block_sum_f64(live ? (double)zc : 0.0, s_red);
    if (t == 0) {
        double *w = a.ws + 3 * (int64_t)b;
        w[0] = s0;
        w[1] = s1;
        w[2] = s2;
    }
}

struct TqcFinishArgs {
    const double *ws;
    float *loss_out, *loss_sum, *means_out, *means_sum;
    cstr_alpha_part_t ap;
    int M, n_keep, batch;
};

__global__ __launch_bounds__(256) void tqc_critic_finish_kernel(const TqcFinishArgs a)
{
    __shared__ double s_red[4];
    const bool with_alpha = a.ap.log_alpha != nullptr;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < a.batch; b += 256) {
        const double *w = a.ws + 3 * (int64_t)b;
        acc[0] += w[0];
        acc[1] += w[1];
        acc[2] += w[2];
        if (with_alpha) acc[3] += (double)a.ap.logp_pi[b] + (double)a.ap.target_entropy;
    }
    double s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = block_sum_f64(acc[i], s_red);
    if (threadIdx.x == 0) {
        const double db = (double)a.batch, dm = (double)a.M, dk = (double)a.n_keep;
        const float loss = (float)(s[0] / (db * dm * dk)), tmean = (float)(s[1] / (db * dk)), amean = (float)(s[2] / (db * dm));
        if (a.loss_out) a.loss_out[0] = loss;
        if (a.loss_sum) a.loss_sum[0] += loss;
        if (a.means_out) { a.means_out[0] = tmean; a.means_out[1] = amean; }
        if (a.means_sum) { a.means_sum[0] += tmean; a.means_sum[1] += amean; }
        if (with_alpha) {  // core/sac/sac.py: ent_coef = exp(log_alpha) before its update; loss = -mean(log_alpha * (logp + H))
            const double la = (double)a.ap.log_alpha[0], mean = s[3] / db;
            const float ec = (float)exp(la), el = (float)(-(la * mean));
            a.ap.grad_out[0] = (float)(-mean);
            a.ap.ent_coef_out[0] = ec;
            if (a.ap.loss_out) a.ap.loss_out[0] = el;
            if (a.ap.loss_sum) a.ap.loss_sum[0] += el;
            if (a.ap.ent_coef_sum) a.ap.ent_coef_sum[0] += ec;
        }
    }
}

struct TqcActorArgs {
    const float *z_pi, *logp, *ent_coef;
    float *gz_pi, *g_logp, *loss_out, *loss_sum, *z_pi_mean;
    int G, Nq, batch;
};

__global__ __launch_bounds__(256) void tqc_actor_loss_kernel(const TqcActorArgs a)
{
    __shared__ double s_red[4];
    const int G = a.G, Nq = a.Nq, batch = a.batch;
    const double ec = (double)a.ent_coef[0], db = (double)batch, dm = (double)(G * Nq);
    const float g_lp = (float)(ec / db), g_z = (float)(-(1.0 / (db * dm)));
    double acc = 0.0;
    for (int b = threadIdx.x; b < batch; b += 256) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) {
            const float *row = a.z_pi + ((int64_t)g * batch + b) * Nq;
            for (int i = 0; i < Nq; ++i) s += (double)row[i];
        }
        const double zm = s / dm;
        if (a.z_pi_mean) a.z_pi_mean[b] = (float)zm;
        a.g_logp[b] = g_lp;
        acc += ec * (double)a.logp[b] - zm;
    }
    const int64_t n = (int64_t)G * batch * Nq;
    for (int64_t e = threadIdx.x; e < n; e += 256) a.gz_pi[e] = g_z;
    const double s = block_sum_f64(acc, s_red);
    if (threadIdx.x == 0) {
        const float loss = (float)(s / db);
        if (a.loss_out) a.loss_out[0] = loss;
        if (a.loss_sum) a.loss_sum[0] += loss;
    }
}

inline bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

inline bool aligned(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0; }

// outputs against inputs and against each other; absent (NULL) buffers are skipped
inline bool any_overlap(const void *const *ins, const int64_t *in_bytes, int n_in, const void *const *outs, const int64_t *out_bytes, int n_out)
{
    for (int o = 0; o < n_out; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < n_in; ++i)
            if (ins[i] && overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return true;
        for (int p = o + 1; p < n_out; ++p)
            if (outs[p] && overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return true;
    }
    return false;
}

}  // namespace

extern "C" int cstr_tqc_supported(int n_critics, int n_quantiles, int drop_per_net)
{
    return n_critics >= 1 && n_critics <= CSTR_MAX_ENS_CRITICS && n_quantiles >= 1 && (int64_t)n_critics * n_quantiles <= CSTR_TQC_MAX_ATOMS
           && drop_per_net >= 0 && drop_per_net < n_quantiles;
}

extern "C" int cstr_tqc_critic_loss_f32(const float *z, const float *z_next, const float *next_logp, const float *rew, const float *done,
                                        const float *ent_coef, double gamma, int n_critics, int n_quantiles, int drop_per_net, float *gz,
                                        float *loss_out, float *loss_sum, float *target_out, float *means_out, float *means_sum, double *ws,
                                        const cstr_alpha_part_t *alpha, int64_t batch, cstr_stream_t stream)
{
    if (!z || !z_next || !next_logp || !rew || !done || !gz || !ws || batch <= 0) return CSTR_E_BADARG;
    if (n_critics <= 0 || n_quantiles <= 0 || drop_per_net < 0 || drop_per_net >= n_quantiles) return CSTR_E_BADARG;
    if (!(gamma >= 0.0)) return CSTR_E_BADARG;  // NaN fails too; a negative one would leave the targets descending
    cstr_alpha_part_t ap = {};
    if (alpha && alpha->log_alpha) {
        if (!alpha->logp_pi || !alpha->grad_out || !alpha->ent_coef_out) return CSTR_E_BADARG;
        ap = *alpha;
    }
    if (!ap.log_alpha && !ent_coef) return CSTR_E_BADARG;  // the entropy term needs its coefficient
    if (!cstr_tqc_supported(n_critics, n_quantiles, drop_per_net) || batch > CSTR_MAX_SAMPLE_BATCH) return CSTR_E_UNSUPPORTED;
    const int M = n_critics * n_quantiles, n_keep = M - drop_per_net * n_critics;
    const int64_t atoms = 4 * batch * M, col = 4 * batch;
    const void *ins[8] = {z, z_next, next_logp, rew, done, ap.log_alpha ? nullptr : ent_coef, ap.log_alpha, ap.logp_pi};
    const int64_t in_b[8] = {atoms, atoms, col, col, col, 4, 4, col};
    const void *outs[11] = {gz, loss_out, loss_sum, target_out, means_out, means_sum, ws, ap.grad_out, ap.ent_coef_out, ap.loss_out, ap.loss_sum};
    const int64_t out_b[11] = {atoms, 4, 4, 4 * batch * n_keep, 8, 8, 24 * batch, 4, 4, 4, 4};
    for (int i = 0; i < 8; ++i)
        if (!aligned(ins[i], 4)) return CSTR_E_BADARG;
    for (int o = 0; o < 11; ++o)
        if (!aligned(outs[o], o == 6 ? 8 : 4)) return CSTR_E_BADARG;
    if (!aligned(ap.ent_coef_sum, 4)) return CSTR_E_BADARG;
    if (any_overlap(ins, in_b, 8, outs, out_b, 11)) return CSTR_E_BADARG;
    TqcCriticArgs a;
    a.z = z; a.z_next = z_next; a.next_logp = next_logp; a.rew = rew; a.done = done; a.ent_coef = ent_coef; a.log_alpha = ap.log_alpha;
    a.gamma = gamma; a.gz = gz; a.target_out = target_out; a.ws = ws;
    a.G = n_critics; a.Nq = n_quantiles; a.k = drop_per_net; a.batch = (int)batch;
    const int lanes = ((M + 63) / 64) * 64;  // one lane per atom, whole waves
    tqc_critic_rows_kernel<<<(unsigned)batch, lanes, 0, (hipStream_t)stream>>>(a);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    TqcFinishArgs f;
    f.ws = ws; f.loss_out = loss_out; f.loss_sum = loss_sum; f.means_out = means_out; f.means_sum = means_sum; f.ap = ap;
    f.M = M; f.n_keep = n_keep; f.batch = (int)batch;
    tqc_critic_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(f);
    return (int)hipGetLastError();
}

extern "C" int cstr_tqc_actor_loss_f32(const float *z_pi, const float *logp, const float *ent_coef, int n_critics, int n_quantiles, float *gz_pi,
                                       float *g_logp, float *loss_out, float *loss_sum, float *z_pi_mean, int64_t batch, cstr_stream_t stream)
{
    if (!z_pi || !logp || !ent_coef || !gz_pi || !g_logp || batch <= 0 || n_critics <= 0 || n_quantiles <= 0) return CSTR_E_BADARG;
    if (!cstr_tqc_supported(n_critics, n_quantiles, 0) || batch > CSTR_MAX_SAMPLE_BATCH) return CSTR_E_UNSUPPORTED;
    const int64_t atoms = 4 * batch * n_critics * n_quantiles, col = 4 * batch;
    const void *ins[3] = {z_pi, logp, ent_coef};
    const int64_t in_b[3] = {atoms, col, 4};
    const void *outs[5] = {gz_pi, g_logp, loss_out, loss_sum, z_pi_mean};
    const int64_t out_b[5] = {atoms, col, 4, 4, col};
    for (int i = 0; i < 3; ++i)
        if (!aligned(ins[i], 4)) return CSTR_E_BADARG;
    for (int o = 0; o < 5; ++o)
        if (!aligned(outs[o], 4)) return CSTR_E_BADARG;
    if (any_overlap(ins, in_b, 3, outs, out_b, 5)) return CSTR_E_BADARG;
    TqcActorArgs a;
    a.z_pi = z_pi; a.logp = logp; a.ent_coef = ent_coef; a.gz_pi = gz_pi; a.g_logp = g_logp; a.loss_out = loss_out; a.loss_sum = loss_sum;
    a.z_pi_mean = z_pi_mean; a.G = n_critics; a.Nq = n_quantiles; a.batch = (int)batch;
    tqc_actor_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
