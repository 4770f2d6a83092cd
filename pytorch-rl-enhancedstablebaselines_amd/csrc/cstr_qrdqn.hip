// cstr_qrdqn.hip -- QR-DQN's own arithmetic (Dabney et al. 2018, "Distributional Reinforcement Learning with Quantile Regression";
// sb3_contrib.QRDQN; core/qrdqn/qrdqn.py) around the quantile network's Linear layers, f32 in and out, gfx950. The face is DQN's
// (M = K * K indices over two valves of K levels), a state has Nq atoms per action, and a row of atoms is [Nq][M]: atom i of action
// a at i * M + a, what the last Linear layer leaves and what `quantiles.view(-1, Nq, M)` reads.
//
// cstr_qrdqn_fold_head_f32: the rollout and `predict` need argmax_a mean_i z[i][a] only, and the mean is linear in the last layer,
//   so they run on the FOLDED head w_mean[a][:] = mean_i w[i * M + a][:], b_mean[a] = mean_i bias[i * M + a]: an [M, H] layer the
//   Linear kernel and cstr_dqn_act_f32 take as they are, instead of writing and re-reading [rows][Nq * M] atoms per vec-step.
//   With e = a * H + k the source of output element e is w[i * M * H + e]: both folds are the mean of Nq consecutive chunks of a
//   flat vector. One lane per output element, so a wave's load of chunk i is 64 consecutive floats; eight loads are issued before
//   the first is consumed (the launch is a chain of Nq dependent-latency loads per lane and nothing else). Sum over i ascending
//   in float64, one division, one rounding.
// cstr_qrdqn_loss_f32, two launches behind one entry point:
//   rows kernel, ONE workgroup per batch row (64 .. 256 lanes, whole waves covering max(M, Nq)):
//     * lane a < M sums z_next[b][i][a] over i ascending in float64 (a wave reads consecutive floats of each atom row); the greedy
//       next action a* is the first maximum of these sums, a NaN the greatest value and the first one winning (row_argmax's order in
//       cstr_dqn.hip), found by a shuffle tree and the wave winners in wave order: the order is total, so the tree's shape is free;
//     * lane j < Nq gathers z_next[b][j][a*] and puts y_j = r + (1 - d) gamma z'_j (float64) into LDS;
//     * lane i < Nq reads z[b][i][a] (a from the stored valve pair, DQN's level_of) and walks the Nq targets in ascending j: delta =
//       y_j - z_i, the Huber term, the weight |tau_i - 1[delta < 0]| and the two sums (loss, gradient) in float64, as in cstr_tqc.hip;
//     * the row of gz is zero-filled by the whole workgroup with consecutive stores, the Nq entries of the taken action left to their
//       lanes; the row's loss sum leaves through the float64 shuffle tree of cstr_tqc.hip.
//   finish kernel, one 256-lane workgroup: lane t adds the row sums of rows t, t + 256, ... in ascending order, the same tree, then
//     lane 0 writes loss = sum / (B Nq) (sum over the current quantile, mean over batch and target quantile).
//   No float atomics and no workgroup that waits for another: a relaunch gives the same bits.
// Nothing here allocates, synchronises or keeps host state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"

namespace {

constexpr int QR_MAX_QUANTILES = CSTR_QRDQN_MAX_QUANTILES;
constexpr int FOLD_LANES = 64, FOLD_IN_FLIGHT = 8;

// out[e] = (sum_i src[i * n + e]) / Nq for e < n: one lane per element
__device__ __forceinline__ float fold_mean(const float *__restrict__ src, const int64_t n, const int64_t e, const int Nq)
{
    const float *p = src + e;
    double s = 0.0;
    int i = 0;
    for (; i + FOLD_IN_FLIGHT <= Nq; i += FOLD_IN_FLIGHT) {
        float v[FOLD_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < FOLD_IN_FLIGHT; ++u) v[u] = p[(int64_t)(i + u) * n];
#pragma unroll
        for (int u = 0; u < FOLD_IN_FLIGHT; ++u) s += (double)v[u];
    }
    for (; i < Nq; ++i) s += (double)p[(int64_t)i * n];
    return (float)(s / (double)Nq);
}

__global__ __launch_bounds__(FOLD_LANES) void qrdqn_fold_head_kernel(const float *__restrict__ w, const float *__restrict__ bias, const int64_t MH,
                                                                     const int M, const int Nq, float *__restrict__ w_mean,
                                                                     float *__restrict__ b_mean)
{
    const int64_t e = (int64_t)blockIdx.x * FOLD_LANES + threadIdx.x;
    if (e < MH)
        w_mean[e] = fold_mean(w, MH, e, Nq);
    else if (e < MH + M)
        b_mean[e - MH] = fold_mean(bias, M, e - MH, Nq);
}

struct QrLossArgs {
    const float *z, *z_next, *valve, *rew, *done;
    int64_t ldz, ldn;
    double gamma;
    float *gz, *cur_out, *target_out;
    int64_t *next_index_out;
    double *ws;
    int M, K, Nq, batch;
};

// cstr_tqc.hip's block_sum_f64: sum over the workgroup (1 to 4 waves of 64 lanes), shuffle tree with offsets 32, 16, ... 1, then the
// wave sums in wave order. Every lane of the workgroup calls it; the result is valid in lane 0. (cstr_onpolicy_device.h's function of
// that name is the 256-entry LDS tree of the batch reductions.)
__device__ __forceinline__ double wave_tree_sum_f64(double v, double *sm)
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

// does (v1, i1) come before (v2, i2) in the greedy order? A NaN is the greatest value, equal values (and two NaNs) go by the index.
__device__ __forceinline__ bool greedy_before(const double v1, const int i1, const double v2, const int i2)
{
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 != n2) return n1;
    if (!n1 && v1 != v2) return v1 > v2;
    return i1 < i2;
}

__global__ __launch_bounds__(256) void qrdqn_loss_rows_kernel(const QrLossArgs a)
{
    __shared__ double s_y[QR_MAX_QUANTILES];
    __shared__ double s_red[4];
    __shared__ int s_idx[4];
    const int b = blockIdx.x, t = threadIdx.x, M = a.M, Nq = a.Nq, K = a.K;
    const float *zn_row = a.z_next + (int64_t)b * a.ldn;
    const float *z_row = a.z + (int64_t)b * a.ldz;
    float *g_row = a.gz + (int64_t)b * a.ldz;

    // the atom sums of the next state and their first maximum
    double best = -__builtin_inf();
    int arg = 0x7fffffff;  // a lane without an action loses against every action, whatever its sum
    if (t < M) {
        double s = 0.0;
        for (int i = 0; i < Nq; ++i) s += (double)zn_row[(int64_t)i * M + t];
        best = s;
        arg = t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_down(best, o, 64);
        const int j = __shfl_down(arg, o, 64);
        if (greedy_before(v, j, best, arg)) { best = v; arg = j; }
    }
    const int lane = t & 63, wave = t >> 6, waves = blockDim.x >> 6;
    if (lane == 0) { s_red[wave] = best; s_idx[wave] = arg; }
    __syncthreads();
    best = s_red[0];
    arg = s_idx[0];
    for (int w = 1; w < waves; ++w)
        if (greedy_before(s_red[w], s_idx[w], best, arg)) { best = s_red[w]; arg = s_idx[w]; }
    const int a_next = arg;  // in [0, M): lane 0 always holds an action
    __syncthreads();

    const double r = (double)a.rew[b], coef = (1.0 - (double)a.done[b]) * a.gamma;
    const float2 v = *reinterpret_cast<const float2 *>(a.valve + (int64_t)b * 2);
    const int a_cur = level_of(v.x, K) * K + level_of(v.y, K);  // in [0, M) by construction
    const bool live = t < Nq;
    float zc = 0.0f;
    if (live) {
        const double y = r + coef * (double)zn_row[(int64_t)t * M + a_next];
        s_y[t] = y;
        zc = z_row[(int64_t)t * M + a_cur];
        if (a.target_out) a.target_out[(int64_t)b * Nq + t] = (float)y;
        if (a.cur_out) a.cur_out[(int64_t)b * Nq + t] = zc;
    }
    if (t == 0 && a.next_index_out) a.next_index_out[b] = (int64_t)a_next;
    // the gradient row: zeros everywhere but at the taken action's Nq atoms, which their lanes store below
    for (int e = t; e < Nq * M; e += blockDim.x)
        if (e % M != a_cur) g_row[e] = 0.0f;
    __syncthreads();
    double lsum = 0.0, gsum = 0.0;
    if (live) {
        const double tau = ((double)t + 0.5) / (double)Nq, w_neg = 1.0 - tau, zd = (double)zc;
        for (int j = 0; j < Nq; ++j) {
            const double d = s_y[j] - zd, ad = fabs(d);  // one address per wave: an LDS broadcast
            const double w = d < 0.0 ? w_neg : tau;                 // |tau_i - 1[delta < 0]|
            const double h = ad <= 1.0 ? 0.5 * d * d : ad - 0.5;    // Huber, kappa = 1
            const double c = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d); // its derivative
            lsum += w * h;
            gsum += w * c;
        }
        g_row[(int64_t)t * M + a_cur] = (float)(-(gsum / ((double)a.batch * (double)Nq)));
    }
    const double s0 = wave_tree_sum_f64(lsum, s_red);
    if (t == 0) a.ws[b] = s0;
}

__global__ __launch_bounds__(256) void qrdqn_loss_finish_kernel(const double *__restrict__ ws, const int batch, const int Nq,
                                                                float *__restrict__ loss_out, float *__restrict__ loss_sum)
{
    __shared__ double s_red[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < batch; b += 256) acc += ws[b];
    const double s = wave_tree_sum_f64(acc, s_red);
    if (threadIdx.x == 0) {
        const float loss = (float)(s / ((double)batch * (double)Nq));
        if (loss_out) loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
    }
}

}  // namespace

extern "C" int cstr_qrdqn_supported(int n_actions, int levels, int n_quantiles)
{
    return levels >= 2 && levels <= CSTR_DQN_MAX_LEVELS && n_actions == levels * levels && n_quantiles >= 1 &&
           n_quantiles <= CSTR_QRDQN_MAX_QUANTILES;
}

extern "C" int cstr_qrdqn_fold_head_f32(const float *w, const float *bias, int n_actions, int n_quantiles, int64_t H, float *w_mean,
                                        float *b_mean, cstr_stream_t stream)
{
    if (!w || !bias || !w_mean || !b_mean || n_actions <= 0 || n_quantiles <= 0 || H <= 0) return CSTR_E_BADARG;
    if (!aligned4(w) || !aligned4(bias) || !aligned4(w_mean) || !aligned4(b_mean)) return CSTR_E_BADARG;
    const int64_t M = n_actions, MH = M * H, n_out = MH + M;
    if (H > ((int64_t)1 << 30) || n_out > ((int64_t)1 << 30)) return CSTR_E_UNSUPPORTED;
    {
        const Buf ins[2] = {{w, (int64_t)n_quantiles * MH}, {bias, (int64_t)n_quantiles * M}};
        const Buf outs[2] = {{w_mean, MH}, {b_mean, M}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    const unsigned grid = (unsigned)((n_out + FOLD_LANES - 1) / FOLD_LANES);
    qrdqn_fold_head_kernel<<<grid, FOLD_LANES, 0, (hipStream_t)stream>>>(w, bias, MH, n_actions, n_quantiles, w_mean, b_mean);
    return (int)hipGetLastError();
}

extern "C" int cstr_qrdqn_loss_f32(const float *z, int64_t ldz, const float *z_next, int64_t ldn, const float *valve, const float *reward,
                                   const float *done, double gamma, int64_t batch, int n_actions, int levels, int n_quantiles, float *gz,
                                   float *loss_out, float *loss_sum, float *cur_out, float *target_out, int64_t *next_index_out, double *ws,
                                   cstr_stream_t stream)
{
    if (!z || !z_next || !valve || !reward || !done || !gz || !ws || batch <= 0 || n_actions <= 0 || levels <= 0 || n_quantiles <= 0)
        return CSTR_E_BADARG;
    if (!(gamma >= 0.0)) return CSTR_E_BADARG;  // NaN fails too
    if (!cstr_qrdqn_supported(n_actions, levels, n_quantiles) || batch > CSTR_MAX_SAMPLE_BATCH) return CSTR_E_UNSUPPORTED;
    const int64_t B = batch, NM = (int64_t)n_quantiles * n_actions;
    if (ldz < NM || ldn < NM) return CSTR_E_BADARG;
    if (!aligned4(z) || !aligned4(z_next) || !aligned8(valve) || !aligned4(reward) || !aligned4(done) || !aligned4(gz) ||
        (loss_out && !aligned4(loss_out)) || (loss_sum && !aligned4(loss_sum)) || (cur_out && !aligned4(cur_out)) ||
        (target_out && !aligned4(target_out)) || (next_index_out && !aligned8(next_index_out)) || !aligned8(ws))
        return CSTR_E_BADARG;
    {
        const Buf ins[5] = {{z, span(B, ldz, NM)}, {z_next, span(B, ldn, NM)}, {valve, 2 * B}, {reward, B}, {done, B}};
        const Buf outs[7] = {{gz, span(B, ldz, NM)}, {loss_out, 1}, {loss_sum, 1}, {cur_out, B * n_quantiles}, {target_out, B * n_quantiles},
                             {next_index_out, 2 * B}, {ws, 2 * B}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    QrLossArgs a;
    a.z = z; a.z_next = z_next; a.valve = valve; a.rew = reward; a.done = done; a.ldz = ldz; a.ldn = ldn; a.gamma = gamma;
    a.gz = gz; a.cur_out = cur_out; a.target_out = target_out; a.next_index_out = next_index_out; a.ws = ws;
    a.M = n_actions; a.K = levels; a.Nq = n_quantiles; a.batch = (int)batch;
    const int widest = n_actions > n_quantiles ? n_actions : n_quantiles;
    const int lanes = ((widest + 63) / 64) * 64;  // whole waves over max(M, Nq) <= 256
    qrdqn_loss_rows_kernel<<<(unsigned)batch, lanes, 0, (hipStream_t)stream>>>(a);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    qrdqn_loss_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(ws, (int)batch, n_quantiles, loss_out, loss_sum);
    return (int)hipGetLastError();
}
