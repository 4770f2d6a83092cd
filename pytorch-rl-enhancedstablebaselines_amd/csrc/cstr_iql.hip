// cstr_iql.hip -- IQL's own arithmetic (Kostrikov, Nair & Levine 2021, "Offline Reinforcement Learning with Implicit Q-Learning";
// core/iql/iql.py), f32, gfx950: everything between the four forward passes of a gradient step (target critics, V on s and s', the
// critics, the actor's distribution parameters) and its three backward passes, in ONE single-workgroup launch:
//   * the expectile value loss |tau_e - 1[u < 0]| u^2 with u = min(Qt_1, Qt_2) - V(s), and its gradient into V(s);
//   * the critic loss against y = r + (1 - d) gamma V(s'): the twin TD loss head's statement, rounding points and float32 reduction
//     (cstr_td_device.h, shared with cstr_td_twin_q_loss_f32 in csrc/cstr_mlp.hip), so the critic outputs have that launch's bits;
//   * advantage-weighted regression of the actor onto the dataset action: w = min(exp(beta u), M) a constant, log pi(a | s) of the
//     squashed diagonal Gaussian at the DATASET action (atanh of the clamped action, the tanh correction of the unclamped one), and
//     its gradient into the head's [mean | raw log_std] rows, the log-std clamp's closed-interval mask included;
//   * the logged scalars.
// The per-(row, action) Gaussian terms are the device functions of cstr_gaussian_device.h, summed over the action dimension in ascending
// order in two sums (logp = sum of Gaussian terms - sum of corrections), as the head kernels do.
// Reductions have a fixed order: thread t of 256 takes rows t, t + 256, ... in ascending order; the critic's two sums are float32 (the
// twin TD loss head's, bit for bit), every other batch sum is float64; each goes through a 64-lane shuffle tree (offsets 32, 16, ... 1)
// and the four wave sums combine as (s0 + s1) + (s2 + s3). No atomics: a relaunch gives the same bits. Nothing here allocates,
// synchronises or keeps host state.
// Launch shape: one row per lane at the learner's batch of 256. The launch is latency-bound there (about 2 A log1p, A exp and 2 A log
// per row: a few dozen transcendental instructions per wave at 8 cycles of issue each, a fraction of a microsecond, against a kernel
// boundary of 1.1 to 1.9 us), so more rows per lane would only put transcendentals behind each other, and fewer lanes would leave
// the float32 critic tree different from the twin TD loss head's; 256 lanes = four waves, one per SIMD of a CU. Rows of 2A <= 8
// floats off 16-byte boundaries: the loops are scalar.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_gaussian_device.h"
#include "cstr_td_device.h"

namespace {

constexpr int IQL_SUMS = 8;  // value, actor, u, w, clipped, logp, v, y

struct IqlArgs {
    const float *qt1, *qt2, *v, *v_next, *q1, *q2, *params, *act, *rew, *done;
    int64_t ldp, ldact;
    float gamma, expectile, beta, exp_adv_max;
    float *g_v, *gq1, *gq2, *g_params, *loss_out, *loss_sum, *aux, *target_out, *adv_out, *logp_out;
    int batch, A;
};

// torch.clamp: a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_nan(const float x, const float lo, const float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(256) void iql_loss_kernel(const IqlArgs a)
{
    __shared__ float smf[4];
    __shared__ double smd[IQL_SUMS][4];
    const int batch = a.batch, A = a.A;
    const float fb = (float)batch;
    const float k = td_q_grad_scale(0.5f, batch);
    const float w_neg = fabsf(a.expectile - 1.0f);  // |tau_e - 1[u < 0]| for u < 0
    const float eps32 = 1.1920928955078125e-07f;    // float32 eps (distributions.py TanhBijector.inverse)
    float a1 = 0.0f, a2 = 0.0f;
    double acc[IQL_SUMS];
#pragma unroll
    for (int i = 0; i < IQL_SUMS; ++i) acc[i] = 0.0;
    for (int b = threadIdx.x; b < batch; b += 256) {
        // every scalar load of the row in front of the arithmetic
        const float qa = a.qt1[b], qb = a.qt2[b], vb = a.v[b], vn = a.v_next[b], q1 = a.q1[b], q2 = a.q2[b], r = a.rew[b], dn = a.done[b];
        const float *p = a.params + (int64_t)b * a.ldp, *ac = a.act + (int64_t)b * a.ldact;
        // value: u = min(Qt_1, Qt_2) - V(s); a NaN u takes weight tau_e (1[NaN < 0] = 0) and stays NaN in u^2
        const float u = fminf(qa, qb) - vb;
        const float we = u < 0.0f ? w_neg : a.expectile;
        if (a.g_v) a.g_v[b] = -(2.0f * we * u) / fb;
        if (a.adv_out) a.adv_out[b] = u;
        // critic: the twin TD loss head with V(s') as both target values, no entropy term
        float d1, d2;
        const float y = td_twin_row(vn, vn, false, 0.0f, 0.0f, r, dn, a.gamma, q1, q2, d1, d2);
        if (a.target_out) a.target_out[b] = y;
        if (a.gq1) { a.gq1[b] = k * d1; a.gq2[b] = k * d2; }
        a1 += d1 * d1;
        a2 += d2 * d2;
        // actor: w = min(exp(beta u), M), NaN kept (a comparison with NaN is false)
        const float e = expf(a.beta * u);
        const bool clipped = e > a.exp_adv_max;
        const float w = clipped ? a.exp_adv_max : e;
        const float c = w / fb;
        float lp = 0.0f, tc = 0.0f;
        for (int j = 0; j < A; ++j) {
            const float mu = p[j], raw = p[A + j], aj = ac[j];
            const float x = clamp_nan(aj, -1.0f + eps32, 1.0f - eps32);
            const float g = 0.5f * (log1pf(x) - log1pf(-x));
            const float ls = clamp_nan(raw, LOG_STD_MIN, LOG_STD_MAX);
            const float sd = expf(ls);
            lp += gaussian_logp_term(mu, sd, g);
            tc += tanh_correction_term(aj);  // the UNclamped action: |a| > 1 is the log of a negative number, torch's NaN
            if (a.g_params) {
                const float d = g - mu, var = sd * sd;
                float *gp = a.g_params + (int64_t)b * (2 * A);
                gp[j] = -(c * (d / var));
                gp[A + j] = (raw >= LOG_STD_MIN && raw <= LOG_STD_MAX) ? -(c * (d * d / var - 1.0f)) : 0.0f;
            }
        }
        const float logp = lp - tc;
        if (a.logp_out) a.logp_out[b] = logp;
        acc[0] += (double)we * (double)u * (double)u;
        acc[1] += -((double)w * (double)logp);
        acc[2] += (double)u;
        acc[3] += (double)w;
        acc[4] += clipped ? 1.0 : 0.0;
        acc[5] += (double)logp;
        acc[6] += (double)vb;
        acc[7] += (double)y;
    }
    const float s1 = block_sum_256(a1, smf), s2 = block_sum_256(a2, smf);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < IQL_SUMS; ++i) {
        double t = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
        if (lane == 0) smd[i][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double db = (double)batch;
        double s[IQL_SUMS];
#pragma unroll
        for (int i = 0; i < IQL_SUMS; ++i) s[i] = (smd[i][0] + smd[i][1]) + (smd[i][2] + smd[i][3]);
        const float loss[3] = {(float)(s[0] / db), td_twin_loss(0.5f, s1, s2, batch), (float)(s[1] / db)};
        for (int i = 0; i < 3; ++i) {
            if (a.loss_out) a.loss_out[i] = loss[i];
            if (a.loss_sum) a.loss_sum[i] += loss[i];
        }
        if (a.aux)
            for (int i = 0; i < 6; ++i) a.aux[i] = (float)(s[2 + i] / db);
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

}  // namespace

extern "C" int cstr_iql_loss_f32(const float *qt1, const float *qt2, const float *v, const float *v_next, const float *q1, const float *q2,
                                 const float *params, int64_t ldp, const float *act, int64_t ldact, const float *rew, const float *done,
                                 float gamma, float expectile, float beta, float exp_adv_max, float *g_v, float *gq1, float *gq2,
                                 float *g_params, float *loss_out, float *loss_sum, float *aux, float *target_out, float *adv_out,
                                 float *logp_out, int64_t batch, int act_dim, cstr_stream_t stream)
{
    if (!qt1 || !qt2 || !v || !v_next || !q1 || !q2 || !params || !act || !rew || !done || batch <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if ((gq1 == nullptr) != (gq2 == nullptr)) return CSTR_E_BADARG;  // the critic's two gradients are one group
    if (ldp < 2 * (int64_t)act_dim || ldact < act_dim) return CSTR_E_BADARG;
    if (!(expectile > 0.0f && expectile < 1.0f) || !(beta >= 0.0f) || !(exp_adv_max > 0.0f)) return CSTR_E_BADARG;  // NaN fails each
    if (batch > CSTR_IQL_MAX_BATCH || act_dim > CSTR_MAX_HEAD_ACT) return CSTR_E_UNSUPPORTED;
    const int64_t a2 = 2 * (int64_t)act_dim;
    const void *ins[10] = {qt1, qt2, v, v_next, q1, q2, params, act, rew, done};
    const int64_t in_n[10] = {batch, batch, batch, batch, batch, batch, span(batch, ldp, a2), span(batch, ldact, act_dim), batch, batch};
    const void *outs[10] = {g_v, gq1, gq2, g_params, loss_out, loss_sum, aux, target_out, adv_out, logp_out};
    const int64_t out_n[10] = {batch, batch, batch, batch * a2, 3, 3, 6, batch, batch, batch};
    for (int i = 0; i < 10; ++i)
        if (!aligned4(ins[i]) || !aligned4(outs[i])) return CSTR_E_BADARG;
    for (int o = 0; o < 10; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 10; ++i)
            if (overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
        for (int p = o + 1; p < 10; ++p)
            if (outs[p] && overlap(outs[o], out_n[o], outs[p], out_n[p])) return CSTR_E_BADARG;
    }
    IqlArgs a;
    a.qt1 = qt1; a.qt2 = qt2; a.v = v; a.v_next = v_next; a.q1 = q1; a.q2 = q2; a.params = params; a.act = act; a.rew = rew; a.done = done;
    a.ldp = ldp; a.ldact = ldact;
    a.gamma = gamma; a.expectile = expectile; a.beta = beta; a.exp_adv_max = exp_adv_max;
    a.g_v = g_v; a.gq1 = gq1; a.gq2 = gq2; a.g_params = g_params; a.loss_out = loss_out; a.loss_sum = loss_sum; a.aux = aux;
    a.target_out = target_out; a.adv_out = adv_out; a.logp_out = logp_out;
    a.batch = (int)batch; a.A = act_dim;
    iql_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
