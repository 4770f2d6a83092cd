// cstr_td3bc.hip -- TD3+BC's own arithmetic around TD3's gradient step (Fujimoto & Gu 2021; core/td3bc/td3bc.py), f32, gfx950:
//   * the actor loss -lam * mean(q) + mean((pi - a)^2) with lam = alpha / mean|q| a CONSTANT of the batch (no gradient through it):
//     the loss value, lam, the two terms and d(loss)/dq = -lam / B in one single-workgroup launch, where TD3 launches
//     neg_mean_loss_kernel (csrc/cstr_mlp.hip);
//   * the backward of the actor's last layer with the behaviour-cloning gradient 2 (pi - a) / (B A) added where the Q-path gradient
//     of the action columns is read: bias_act_bwd_kernel's walk (csrc/cstr_mlp.hip) with one more strided operand.
// Reductions have a fixed order (per-thread strided partial sums in float64, 64-lane shuffle tree, (s0 + s1) + (s2 + s3) over the
// four waves): no atomics, a relaunch gives the same bits. Nothing here allocates, synchronises or keeps host state.
// Access width: pi / act are the action columns of packed critic inputs (row stride obs_dim + act_dim = 6 floats, column offset
// obs_dim), so rows sit on 4-byte boundaries only and the loops are scalar; both launches are launch-latency bound at batch size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"

namespace {

constexpr int ACT_RELU = CSTR_ACT_RELU, ACT_TANH = CSTR_ACT_TANH;

// The three batch sums are accumulated in float64 (exact products of float32 inputs, a fixed tree) and every output is rounded to
// float32 ONCE, where a float32 evaluation carries one rounding per operation and per addend. Against the fp64 statement on the same
// float32 inputs: lam and bc within 0.5 ulp; the Q term, which follows from the float32 lam, about 1 ulp; the loss, their sum, about
// 2 ulp of its own (smaller) value. One workgroup of 256 lanes at batch <= 16384: the fp64 adds are not what it waits for.
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the loss heads' tree (csrc/cstr_mlp.hip block_sum_256) on float64 partial sums
__device__ __forceinline__ double block_sum_256(double v, double *sm)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    const double r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

// loss = -lam * mean_b(q_b) + mean_{b,j}((pi_bj - a_bj)^2),  lam = alpha / mean_b|q_b|  (not differentiated);  gq_b = -lam / B.
// mean|q| == 0 is not guarded: lam = alpha / 0 (inf, or NaN for alpha == 0) and the loss follows (NaN), as the float32 torch statement.
__global__ __launch_bounds__(256) void td3bc_actor_loss_kernel(const float *__restrict__ q, const float *__restrict__ pi, const int64_t ldpi,
                                                               const float *__restrict__ act, const int64_t ldact, const float alpha,
                                                               float *__restrict__ gq, float *__restrict__ loss_out,
                                                               float *__restrict__ loss_sum, float *__restrict__ aux, const int batch,
                                                               const int A)
{
    __shared__ double sm[4];
    double a_abs = 0.0, a_q = 0.0, a_bc = 0.0;
    for (int b = threadIdx.x; b < batch; b += 256) a_abs += (double)fabsf(q[b]);
    const double s_abs = block_sum_256(a_abs, sm);  // first reduction: the normaliser
    for (int b = threadIdx.x; b < batch; b += 256) {
        a_q += (double)q[b];
        const float *p = pi + (int64_t)b * ldpi, *a = act + (int64_t)b * ldact;
        for (int j = 0; j < A; ++j) {
            const double d = (double)p[j] - (double)a[j];
            a_bc += d * d;
        }
    }
    const double s_q = block_sum_256(a_q, sm), s_bc = block_sum_256(a_bc, sm);
    const double fb = (double)batch;
    // float32 lam first: a float32 statement overflows to inf where the quotient leaves the float32 range, and so does this one
    const float lam = (float)((double)alpha / (s_abs / fb));
    const float g = (float)(-((double)lam / fb));
    for (int b = threadIdx.x; b < batch; b += 256) gq[b] = g;
    if (threadIdx.x == 0) {
        const double q_term = -((double)lam * (s_q / fb)), bc = s_bc / (fb * (double)A);
        const float loss = (float)(q_term + bc);
        if (loss_out) loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
        if (aux) {
            aux[0] = lam;
            aux[1] = (float)q_term;
            aux[2] = (float)bc;
        }
    }
}

// gz[m][n] = (gy[m][n] + coef * (y[m][n] - act[m][n])) * act'(y[m][n]): bias_act_bwd_kernel's ownership (a workgroup owns 64 columns,
// its WAVES waves stride over the rows, FLY rows of loads in flight per wave) and its expressions for act'. coef == 0 adds nothing
// (not even a signed zero), so the result is bias_act_bwd_kernel's bit for bit.
template <int ACT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void td3bc_act_bwd_rows_kernel(const float *__restrict__ gy, const int64_t ldg,
                                                                        const float *__restrict__ y, const int64_t ldy,
                                                                        const float *__restrict__ act, const int64_t lda, const float coef,
                                                                        float *__restrict__ gz, const int m, const int n)
{
    constexpr int FLY = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    if (col >= n) return;
    for (int r0 = wave; r0 < m; r0 += FLY * WAVES) {
        float g[FLY], t[FLY], a[FLY];
#pragma unroll
        for (int k = 0; k < FLY; ++k) {
            const int r = r0 + k * WAVES;
            g[k] = r < m ? gy[(int64_t)r * ldg + col] : 0.0f;
            t[k] = r < m ? y[(int64_t)r * ldy + col] : 0.0f;
            a[k] = r < m ? act[(int64_t)r * lda + col] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < FLY; ++k) {
            const int r = r0 + k * WAVES;
            if (coef != 0.0f) g[k] = g[k] + coef * (t[k] - a[k]);
            if (ACT == ACT_RELU) g[k] = t[k] > 0.0f ? g[k] : 0.0f;
            if (ACT == ACT_TANH) g[k] = g[k] * (1.0f - t[k] * t[k]);
            if (r < m) gz[(int64_t)r * n + col] = g[k];
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

extern "C" int cstr_td3bc_actor_loss_f32(const float *q, const float *pi, int64_t ldpi, const float *act, int64_t ldact, float alpha,
                                         float *gq, float *loss_out, float *loss_sum, float *aux, int64_t batch, int act_dim,
                                         cstr_stream_t stream)
{
    if (!q || !pi || !act || !gq || batch <= 0 || act_dim <= 0 || ldpi < act_dim || ldact < act_dim) return CSTR_E_BADARG;
    if (!(alpha >= 0.0f)) return CSTR_E_BADARG;  // negative or NaN
    if (batch > CSTR_TD3BC_MAX_BATCH || act_dim > CSTR_TD3BC_MAX_ACT) return CSTR_E_UNSUPPORTED;
    if (!aligned4(q) || !aligned4(pi) || !aligned4(act) || !aligned4(gq) || !aligned4(loss_out) || !aligned4(loss_sum) || !aligned4(aux))
        return CSTR_E_BADARG;
    const void *ins[3] = {q, pi, act};
    const int64_t in_n[3] = {batch, span(batch, ldpi, act_dim), span(batch, ldact, act_dim)};
    const void *outs[4] = {gq, loss_out, loss_sum, aux};
    const int64_t out_n[4] = {batch, 1, 1, 3};
    if (any_overlap(ins, in_n, 3, outs, out_n, 4)) return CSTR_E_BADARG;
    td3bc_actor_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(q, pi, ldpi, act, ldact, alpha, gq, loss_out, loss_sum, aux, (int)batch,
                                                                act_dim);
    return (int)hipGetLastError();
}

extern "C" int cstr_td3bc_act_bwd_rows_f32(const float *gy, int64_t ldgy, const float *y, int64_t ldy, const float *act, int64_t ldact,
                                           float coef, int act_kind, float *gz, int64_t m, int64_t n, cstr_stream_t stream)
{
    if (!gy || !y || !act || !gz || m <= 0 || n <= 0 || ldgy < n || ldy < n || ldact < n) return CSTR_E_BADARG;
    if (act_kind < 0 || act_kind > 2 || m > 0x7fffffff || n > 0x7fffffff) return CSTR_E_UNSUPPORTED;
    if (!aligned4(gy) || !aligned4(y) || !aligned4(act) || !aligned4(gz)) return CSTR_E_BADARG;
    const void *ins[3] = {gy, y, act};
    const int64_t in_n[3] = {span(m, ldgy, n), span(m, ldy, n), span(m, ldact, n)};
    const void *outs[1] = {gz};
    const int64_t out_n[1] = {m * n};
    if (any_overlap(ins, in_n, 3, outs, out_n, 1)) return CSTR_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + 63) / 64), 1u);
#define TBR(A, W) td3bc_act_bwd_rows_kernel<A, W><<<grid, 64 * W, 0, s>>>(gy, ldgy, y, ldy, act, ldact, coef, gz, (int)m, (int)n)
    if (m >= 64) { if (act_kind == 0) TBR(0, 16); else if (act_kind == 1) TBR(1, 16); else TBR(2, 16); }  // bias_act_bwd_rows' shapes
    else { if (act_kind == 0) TBR(0, 4); else if (act_kind == 1) TBR(1, 4); else TBR(2, 4); }
#undef TBR
    return (int)hipGetLastError();
}
