// cstr_sde.hip -- generalized State-Dependent Exploration (gSDE) for SAC's actor (reference core/sac/policies.py:89-175,
// core/common/distributions.py:421-617), f32, gfx950:
//   * the exploration matrices M = z * std(log_std) (exp or expln, full or [L, 1] std), z drawn in the kernel from a Philox stream
//     whose offset the last workgroup advances (graph replays draw fresh matrices) or given (teacher-forced tests);
//   * the gSDE head forward from the latent h [B, L]: mean = Hardtanh(h W^T + b), noise = h M (one shared matrix or one per row),
//     variance = (h^2)(std^2), action = tanh(mean + noise), and the reference's log-prob through atanh(clamp(action));
//   * its backward: d/dh through mean, noise and variance times the latent's last activation gradient (one launch), then dW, db and
//     d log_std reduced over the batch (one launch, a workgroup per 64 latent columns + one for db; no atomics).
// One wave per row in the row kernels; every reduction has a fixed order, so results are deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2;
constexpr float SDE_EPS = 1e-6f;                  // StateDependentNoiseDistribution.epsilon (distributions.py:450)
constexpr float TANH_CLAMP = 1.0f - 1.1920929e-07f;  // TanhBijector.inverse: clamp to +-(1 - finfo(float32).eps)
constexpr uint32_t SDE_STREAM_TAG = 0x5DE5DE5Du;  // counter word 3: the gSDE draws never share counters with the action heads

// get_std (distributions.py:473-497): exp, or expln = exp(x) for x <= 0 and log1p(x + eps) + 1 above
__device__ __forceinline__ float sde_std(const float ls, const int expln)
{
    if (!expln) return expf(ls);
    const float pos = ls > 0.0f ? 1.0f : 0.0f;
    const float below = expf(ls) * (ls <= 0.0f ? 1.0f : 0.0f);
    const float above = (log1pf(ls * pos + SDE_EPS) + 1.0f) * pos;
    return below + above;
}

// d std / d log_std of the same expression (autograd's: exp' = exp, log1p' = 1 / (1 + x), the masks are constants)
__device__ __forceinline__ float sde_dstd(const float ls, const int expln)
{
    if (!expln) return expf(ls);
    if (ls <= 0.0f) return expf(ls);
    return 1.0f / (1.0f + (ls + SDE_EPS));
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// mats[i] = z[i] * std[(i % (L A))] for i < n_mats L A (Normal(0, std).rsample, distributions.py:507-512); std_out [L, A] = get_std.
// z: read, or drawn (Philox4x32-10 keyed by rng_ctl[0], counter = (rng_ctl[1] + pair, 0, tag) -> Box-Muller, element 2p + k) and
// stored for the first z_keep matrices.
__global__ __launch_bounds__(256) void sde_draw_kernel(const float *__restrict__ log_std, const int ls_cols, const int L, const int A,
                                                       const int expln, const int64_t n_mats, float *__restrict__ std_out,
                                                       float *__restrict__ z, const int64_t z_keep, float *__restrict__ mats,
                                                       uint64_t *__restrict__ rng_ctl)
{
    const int64_t per = (int64_t)L * A, total = n_mats * per, pairs = (total + 1) >> 1, z_end = z_keep * per;
    const uint64_t seed = rng_ctl ? rng_ctl[0] : 0ull, base = rng_ctl ? rng_ctl[1] : 0ull;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * blockDim.x) {
        float e[2] = {0.0f, 0.0f};
        if (rng_ctl) {
            const uint64_t ctr = base + (uint64_t)p;
            uint32_t r[4];
            philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, SDE_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), r);
            box_muller(r[0], r[1], e[0], e[1]);
        }
        for (int k = 0; k < 2; ++k) {
            const int64_t i = 2 * p + k;
            if (i >= total) break;
            const int64_t la = i % per;
            const int l = (int)(la / A), a = (int)(la % A);
            const float s = sde_std(log_std[(int64_t)l * ls_cols + (ls_cols == 1 ? 0 : a)], expln);
            float zz;
            if (rng_ctl) {
                zz = e[k];
                if (i < z_end) z[i] = zz;  // only the matrices whose z a backward needs are stored
            }
            else zz = z[i];
            mats[i] = zz * s;
            if (std_out && i < per) std_out[i] = s;
        }
    }
    if (rng_ctl && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0)
        rng_ctl[1] = base + (uint64_t)pairs;
}

// Forward, one wave per row. aux [B][2A] keeps (pre-clip mean, variance) for the backward.
__global__ __launch_bounds__(256) void sde_head_fwd_kernel(const float *__restrict__ h, const int64_t ldh, const int64_t batch, const int L,
                                                           const int A, const float *__restrict__ w, const float *__restrict__ bias,
                                                           const float clip, const float *__restrict__ mats, const int64_t mat_stride,
                                                           const float *__restrict__ stdm, float *__restrict__ action, const int64_t act_stride,
                                                           float *__restrict__ logp, float *__restrict__ aux)
{
    const float half_log_2pi = 0.91893853320467274178f;
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (row >= batch) return;
    const float *hr = h + row * ldh;
    const float *M = mats ? mats + row * mat_stride : nullptr;
    float sm[CSTR_MAX_HEAD_ACT], sn[CSTR_MAX_HEAD_ACT], sv[CSTR_MAX_HEAD_ACT];
#pragma unroll
    for (int a = 0; a < CSTR_MAX_HEAD_ACT; ++a) sm[a] = sn[a] = sv[a] = 0.0f;
    for (int l = lane; l < L; l += 64) {
        const float hv = hr[l], h2 = hv * hv;
#pragma unroll
        for (int a = 0; a < CSTR_MAX_HEAD_ACT; ++a) {
            if (a >= A) break;
            sm[a] += hv * w[(int64_t)a * L + l];
            if (M) sn[a] += hv * M[(int64_t)l * A + a];
            const float s = stdm[(int64_t)l * A + a];
            sv[a] += h2 * (s * s);
        }
    }
#pragma unroll
    for (int a = 0; a < CSTR_MAX_HEAD_ACT; ++a) {
        if (a >= A) break;
        sm[a] = wave_sum(sm[a]);
        sn[a] = wave_sum(sn[a]);
        sv[a] = wave_sum(sv[a]);
    }
    if (lane != 0) return;
    float lp = 0.0f, corr = 0.0f;
    for (int a = 0; a < A; ++a) {
        const float pre = sm[a] + bias[a];
        const float mean = clip > 0.0f ? fminf(fmaxf(pre, -clip), clip) : pre;  // nn.Hardtanh(-clip_mean, clip_mean)
        const float x = M ? mean + sn[a] : mean;                                  // sample() / mode()
        const float act = tanhf(x);
        action[row * act_stride + a] = act;
        const float scale = sqrtf(sv[a] + SDE_EPS);
        const float c = fminf(fmaxf(act, -TANH_CLAMP), TANH_CLAMP);
        const float ga = 0.5f * (log1pf(c) - log1pf(-c));  // TanhBijector.atanh
        const float d = ga - mean, v2 = scale * scale;
        lp += -(d * d) / (2.0f * v2) - logf(scale) - half_log_2pi;  // torch Normal.log_prob
        const float t = tanhf(ga);
        corr += logf(1.0f - t * t + SDE_EPS);  // log_prob_correction
        if (aux) { aux[row * 2 * A + a] = pre; aux[row * 2 * A + A + a] = sv[a]; }
    }
    if (logp) logp[row] = lp - corr;
}

// Backward, one wave per row: per-row gradients w.r.t. the pre-clip mean (g_pre), x = mean + noise (g_x) and the variance (g_var),
// and dh = g_pre W + g_x M^T + 2 h (g_var (std^2)^T), times the activation gradient of the layer that produced h.
__global__ __launch_bounds__(256) void sde_head_bwd_kernel(const float *__restrict__ g_action, const int64_t ga_stride,
                                                           const float *__restrict__ g_logp, const float *__restrict__ action,
                                                           const int64_t act_stride, const float *__restrict__ aux,
                                                           const float *__restrict__ h, const int64_t ldh, const int64_t batch, const int L,
                                                           const int A, const float *__restrict__ w, const float clip,
                                                           const float *__restrict__ mats, const int64_t mat_stride,
                                                           const float *__restrict__ stdm, const int below, float *__restrict__ g_pre_out,
                                                           float *__restrict__ g_x_out, float *__restrict__ g_var_out, float *__restrict__ dh)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (row >= batch) return;
    float gp[CSTR_MAX_HEAD_ACT], gx[CSTR_MAX_HEAD_ACT], gv[CSTR_MAX_HEAD_ACT];
    const float gl = g_logp ? g_logp[row] : 0.0f;
    for (int a = 0; a < CSTR_MAX_HEAD_ACT; ++a) {
        gp[a] = gx[a] = gv[a] = 0.0f;
        if (a >= A) continue;
        const float act = action[row * act_stride + a];
        const float pre = aux[row * 2 * A + a], var = aux[row * 2 * A + A + a];
        const float mean = clip > 0.0f ? fminf(fmaxf(pre, -clip), clip) : pre;
        const float scale = sqrtf(var + SDE_EPS), v2 = scale * scale;
        const float c = fminf(fmaxf(act, -TANH_CLAMP), TANH_CLAMP);
        const float ga = 0.5f * (log1pf(c) - log1pf(-c));
        const float d = ga - mean, t = tanhf(ga), omt = 1.0f - t * t;
        // d logp / d ga: the Gaussian term and the squash correction evaluated at ga (autograd through tanh(ga))
        const float g_ga = gl * (-d / v2 + 2.0f * t * omt / (omt + SDE_EPS));
        const float g_c = g_ga * 0.5f * (1.0f / (1.0f + c) + 1.0f / (1.0f - c));
        const bool inside = act >= -TANH_CLAMP && act <= TANH_CLAMP;  // clamp passes the gradient inside [min, max]
        const float g_act = (g_action ? g_action[row * ga_stride + a] : 0.0f) + (inside ? g_c : 0.0f);
        const float g_x = g_act * (1.0f - act * act);  // tanh backward
        const float g_mean = g_x + gl * (d / v2);
        const float g_scale = gl * ((d * d) / (scale * v2) - 1.0f / scale);
        gv[a] = g_scale * 0.5f / scale;  // sqrt backward
        gx[a] = mats ? g_x : 0.0f;
        gp[a] = (clip > 0.0f && !(pre > -clip && pre < clip)) ? 0.0f : g_mean;  // hardtanh_backward: zero at and beyond the bounds
    }
    if (lane == 0) {
        for (int a = 0; a < A; ++a) {
            if (g_pre_out) g_pre_out[row * A + a] = gp[a];
            if (g_x_out) g_x_out[row * A + a] = gx[a];
            if (g_var_out) g_var_out[row * A + a] = gv[a];
        }
    }
    if (!dh) return;
    const float *hr = h + row * ldh;
    const float *M = mats ? mats + row * mat_stride : nullptr;
    for (int l = lane; l < L; l += 64) {
        const float hv = hr[l];
        float acc = 0.0f, accv = 0.0f;
        for (int a = 0; a < A; ++a) {
            acc += w[(int64_t)a * L + l] * gp[a];
            if (M) acc += M[(int64_t)l * A + a] * gx[a];
            const float s = stdm[(int64_t)l * A + a];
            accv += gv[a] * (s * s);
        }
        acc += 2.0f * hv * accv;
        if (below == ACT_RELU) acc = hv > 0.0f ? acc : 0.0f;
        else if (below == ACT_TANH) acc *= 1.0f - hv * hv;
        dh[row * L + l] = acc;
    }
}

// dW [A][L] = g_pre^T h, d log_std = std'(log_std) * (z * h^T g_x + 2 std * (h^2)^T g_var) (summed over A for a [L, 1] log_std),
// db [A] = column sums of g_pre. Workgroup j < ceil(L / 64) owns latent columns [64 j, 64 j + 64) (lane = column, its four waves
// stride over the rows, LDS combines them); the last workgroup reduces db. Every output element is written once.
__global__ __launch_bounds__(256) void sde_param_grad_kernel(const float *__restrict__ h, const int64_t ldh, const int64_t batch, const int L,
                                                             const int A, const float *__restrict__ g_pre, const float *__restrict__ g_x,
                                                             const float *__restrict__ g_var, const float *__restrict__ z,
                                                             const float *__restrict__ stdm, const float *__restrict__ log_std,
                                                             const int ls_cols, const int expln, float *__restrict__ dw,
                                                             float *__restrict__ db, float *__restrict__ dlog_std)
{
    __shared__ float part[4][3 * CSTR_MAX_HEAD_ACT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblk_l = (L + 63) / 64;
    if ((int)blockIdx.x == nblk_l) {  // db
        __shared__ float red[CSTR_MAX_HEAD_ACT][256];
        for (int a = 0; a < A; ++a) {
            float s = 0.0f;
            for (int64_t b = threadIdx.x; b < batch; b += 256) s += g_pre[b * A + a];
            red[a][threadIdx.x] = s;
        }
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o)
                for (int a = 0; a < A; ++a) red[a][threadIdx.x] += red[a][threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0 && db)
            for (int a = 0; a < A; ++a) db[a] = red[a][0];
        return;
    }
    const int l = blockIdx.x * 64 + lane;
    float sw[CSTR_MAX_HEAD_ACT], sx[CSTR_MAX_HEAD_ACT], sv[CSTR_MAX_HEAD_ACT];
#pragma unroll
    for (int a = 0; a < CSTR_MAX_HEAD_ACT; ++a) sw[a] = sx[a] = sv[a] = 0.0f;
    if (l < L) {
        for (int64_t b = wave; b < batch; b += 4) {
            const float hv = h[b * ldh + l], h2 = hv * hv;
#pragma unroll
            for (int a = 0; a < CSTR_MAX_HEAD_ACT; ++a) {
                if (a >= A) break;
                sw[a] += hv * g_pre[b * A + a];
                sx[a] += hv * g_x[b * A + a];
                sv[a] += h2 * g_var[b * A + a];
            }
        }
    }
    for (int a = 0; a < A; ++a) {
        part[wave][a][lane] = sw[a];
        part[wave][CSTR_MAX_HEAD_ACT + a][lane] = sx[a];
        part[wave][2 * CSTR_MAX_HEAD_ACT + a][lane] = sv[a];
    }
    __syncthreads();
    if (wave != 0 || l >= L) return;
    float dls_sum = 0.0f;
    for (int a = 0; a < A; ++a) {
        const float w_ = ((part[0][a][lane] + part[1][a][lane]) + part[2][a][lane]) + part[3][a][lane];
        const int kx = CSTR_MAX_HEAD_ACT + a, kv = 2 * CSTR_MAX_HEAD_ACT + a;
        const float x_ = ((part[0][kx][lane] + part[1][kx][lane]) + part[2][kx][lane]) + part[3][kx][lane];
        const float v_ = ((part[0][kv][lane] + part[1][kv][lane]) + part[2][kv][lane]) + part[3][kv][lane];
        if (dw) dw[(int64_t)a * L + l] = w_;
        const float s = stdm[(int64_t)l * A + a];
        const float dstd = (z ? z[(int64_t)l * A + a] * x_ : 0.0f) + 2.0f * s * v_;
        const float ls = log_std[(int64_t)l * ls_cols + (ls_cols == 1 ? 0 : a)];
        const float dls = dstd * sde_dstd(ls, expln);
        if (ls_cols == 1) dls_sum += dls;
        else if (dlog_std) dlog_std[(int64_t)l * A + a] = dls;
    }
    if (ls_cols == 1 && dlog_std) dlog_std[l] = dls_sum;
}

inline bool sde_dims_bad(int64_t batch, int L, int A) { return batch <= 0 || L <= 0 || A <= 0; }
inline bool sde_dims_unsupported(int L, int A) { return L > CSTR_SDE_MAX_LATENT || A > CSTR_MAX_HEAD_ACT; }

}  // namespace

extern "C" int cstr_sde_draw_f32(const float *log_std, int log_std_cols, int latent, int act_dim, int use_expln, int64_t n_mats,
                                 float *std_out, float *z, int64_t z_keep, float *mats, uint64_t *rng_ctl, cstr_stream_t stream)
{
    if (!log_std || !z || !mats || n_mats <= 0 || latent <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if (z_keep < 0 || z_keep > n_mats) return CSTR_E_BADARG;
    if (log_std_cols != 1 && log_std_cols != act_dim) return CSTR_E_BADARG;
    if (sde_dims_unsupported(latent, act_dim) || n_mats > CSTR_SDE_MAX_MATS) return CSTR_E_UNSUPPORTED;
    const int64_t pairs = (n_mats * latent * act_dim + 1) / 2;
    const int64_t g = (pairs + 255) / 256;
    sde_draw_kernel<<<(unsigned)(g < 2048 ? g : 2048), 256, 0, (hipStream_t)stream>>>(log_std, log_std_cols, latent, act_dim, use_expln != 0,
                                                                                      n_mats, std_out, z, z_keep, mats, rng_ctl);
    return (int)hipGetLastError();
}

extern "C" int cstr_sde_head_fwd_f32(const float *h, int64_t ldh, int64_t batch, int latent, int act_dim, const float *w_mu,
                                     const float *b_mu, float clip_mean, const float *mats, int64_t mat_stride, const float *std_mat,
                                     float *action, int64_t action_stride, float *logp, float *aux, cstr_stream_t stream)
{
    if (!h || !w_mu || !b_mu || !std_mat || !action || sde_dims_bad(batch, latent, act_dim)) return CSTR_E_BADARG;
    if (ldh < latent || action_stride < act_dim || mat_stride < 0 || (mats && mat_stride != 0 && mat_stride < (int64_t)latent * act_dim))
        return CSTR_E_BADARG;
    if (sde_dims_unsupported(latent, act_dim)) return CSTR_E_UNSUPPORTED;
    sde_head_fwd_kernel<<<(unsigned)((batch + 3) / 4), 256, 0, (hipStream_t)stream>>>(h, ldh, batch, latent, act_dim, w_mu, b_mu, clip_mean, mats,
                                                                                       mat_stride, std_mat, action, action_stride, logp, aux);
    return (int)hipGetLastError();
}

extern "C" int cstr_sde_head_bwd_f32(const float *g_action, int64_t g_action_stride, const float *g_logp, const float *action,
                                     int64_t action_stride, const float *aux, const float *h, int64_t ldh, int64_t batch, int latent,
                                     int act_dim, const float *w_mu, float clip_mean, const float *mats, int64_t mat_stride,
                                     const float *std_mat, int below_act, float *g_pre, float *g_x, float *g_var, float *dh,
                                     cstr_stream_t stream)
{
    if (!action || !aux || !h || !w_mu || !std_mat || sde_dims_bad(batch, latent, act_dim)) return CSTR_E_BADARG;
    if (!g_action && !g_logp) return CSTR_E_BADARG;
    if (ldh < latent || action_stride < act_dim || (g_action && g_action_stride < act_dim) || mat_stride < 0 ||
        (mats && mat_stride != 0 && mat_stride < (int64_t)latent * act_dim))
        return CSTR_E_BADARG;
    if (below_act < ACT_NONE || below_act > ACT_TANH) return CSTR_E_BADARG;
    if (sde_dims_unsupported(latent, act_dim)) return CSTR_E_UNSUPPORTED;
    sde_head_bwd_kernel<<<(unsigned)((batch + 3) / 4), 256, 0, (hipStream_t)stream>>>(g_action, g_action_stride, g_logp, action, action_stride,
                                                                                       aux, h, ldh, batch, latent, act_dim, w_mu, clip_mean,
                                                                                       mats, mat_stride, std_mat, below_act, g_pre, g_x, g_var, dh);
    return (int)hipGetLastError();
}

extern "C" int cstr_sde_param_grad_f32(const float *h, int64_t ldh, int64_t batch, int latent, int act_dim, const float *g_pre,
                                       const float *g_x, const float *g_var, const float *z, const float *std_mat, const float *log_std,
                                       int log_std_cols, int use_expln, float *dw_mu, float *db_mu, float *dlog_std, cstr_stream_t stream)
{
    if (!h || !g_pre || !g_x || !g_var || !std_mat || !log_std || sde_dims_bad(batch, latent, act_dim)) return CSTR_E_BADARG;
    if (ldh < latent || (log_std_cols != 1 && log_std_cols != act_dim)) return CSTR_E_BADARG;
    if (sde_dims_unsupported(latent, act_dim)) return CSTR_E_UNSUPPORTED;
    sde_param_grad_kernel<<<(unsigned)((latent + 63) / 64 + 1), 256, 0, (hipStream_t)stream>>>(h, ldh, batch, latent, act_dim, g_pre, g_x, g_var, z,
                                                                                                std_mat, log_std, log_std_cols, use_expln != 0,
                                                                                                dw_mu, db_mu, dlog_std);
    return (int)hipGetLastError();
}
