// cstr_bcq.hip -- BCQ's own arithmetic around the Linear layers (reference core/bcq/bcq.py:137-213, core/bcq/policies.py:67-124,
// :157-166, :244-253, :426-435), f32, gfx950:
//   * the VAE latent from the merged head output [mean | log_std_raw]: clamp(-4, 15), exp, z = mean + std * eps, written next to the
//     observation into the decoder input; its backward with the KL gradients added;
//   * the VAE loss mse(recon, act) + 0.5 * (-0.5 * mean(1 + log(std^2) - mean^2 - std^2)) with its three gradients;
//   * the candidate expansion [state[r % n] | clamp(randn, -0.5, 0.5)] (the reference's repeat + cat + randn + clamp);
//   * the perturbation a = clamp(a_vae + max_perturbation * p, -1, 1) and its backward;
//   * the target: min over the target critics, max over groups of S candidates (the reference's grouping or a state's own), TD target;
//   * predict's selection: per state the first maximum of q1 over its candidates and the gathered action.
// Noise is READ when given and DRAWN otherwise: Philox4x32-10 keyed by rng_ctl[0], counter (rng_ctl[1] + pair, 0, BCQ tag) ->
// Box-Muller, element 2 pair + k; the last workgroup advances rng_ctl[1], so a graph replay draws fresh noise. Every reduction has
// a fixed order (no float atomics). Nothing here allocates, synchronises or keeps host state.
// Access width: the expansion's state rows move as 16-byte vectors where pointers and strides allow. The other loops are scalar with
// one index division per element on purpose: their operands are column blocks of rows whose strides (D + A = 6, D + L = 36 floats) and
// column offsets (D, D + L) leave most rows off 16-byte boundaries, and at the learner's sizes (<= 2560 x 32 floats) every launch here
// is launch-latency bound; a vector path for the aligned special case was judged not worth its extra instantiations.
// NaN: the target / selection reductions use fminf / fmaxf and `>`, which DROP a NaN operand where torch.min / max / argmax propagate it:
// a diverged critic shows as NaN on the torch-statement path and as the remaining finite values here (the losses still go NaN through
// the current Q values of the same critic).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr float LOG_STD_MIN = -4.0f, LOG_STD_MAX = 15.0f;  // policies.py:78
constexpr uint32_t BCQ_STREAM_TAG = 0xBC0BC0B1u;           // counter word 3: never shares counters with the action heads / gSDE

__device__ __forceinline__ void bcq_pair(const uint64_t seed, const uint64_t ctr, float &e0, float &e1)
{
    uint32_t r[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, BCQ_STREAM_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    box_muller(r[0], r[1], e0, e1);
}

// policies.py:76-85: xdec[row] = [obs[row] | mean + exp(clamp(log_std_raw)) * eps]; std and eps are kept for the backward.
__global__ __launch_bounds__(256) void bcq_latent_fwd_kernel(const float *__restrict__ params, const int64_t ldp,
                                                             const float *__restrict__ obs, const int64_t ldo,
                                                             const float *__restrict__ eps_in, uint64_t *__restrict__ rng_ctl,
                                                             float *__restrict__ xdec, const int64_t ldx, float *__restrict__ std_out,
                                                             float *__restrict__ eps_out, const int64_t batch, const int D, const int L)
{
    const int64_t total = batch * L, pairs = (total + 1) >> 1;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const uint64_t seed = rng_ctl ? rng_ctl[0] : 0ull, base = rng_ctl ? rng_ctl[1] : 0ull;
    for (int64_t p = tid; p < pairs; p += nthr) {
        float e[2] = {0.0f, 0.0f};
        if (rng_ctl) bcq_pair(seed, base + (uint64_t)p, e[0], e[1]);
        for (int k = 0; k < 2; ++k) {
            const int64_t i = 2 * p + k;
            if (i >= total) break;
            const int64_t row = i / L;
            const int c = (int)(i - row * L);
            const float mean = params[row * ldp + c];
            const float ls = fminf(fmaxf(params[row * ldp + L + c], LOG_STD_MIN), LOG_STD_MAX);
            const float s = expf(ls);
            const float ev = rng_ctl ? e[k] : eps_in[i];
            const float se = s * ev;
            xdec[row * ldx + D + c] = mean + se;
            std_out[i] = s;
            if (eps_out) eps_out[i] = ev;
        }
    }
    const int64_t ncopy = batch * D;
    for (int64_t j = tid; j < ncopy; j += nthr) {
        const int64_t row = j / D;
        const int c = (int)(j - row * D);
        xdec[row * ldx + c] = obs[row * ldo + c];
    }
    if (rng_ctl && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0)
        rng_ctl[1] = base + (uint64_t)pairs;
}

// bcq.py:145-149. Every workgroup writes its share of the three gradients; workgroup 0 alone reduces the loss (thread t sums the
// elements t, t + 256, ... in f64, then a fixed LDS tree).
__global__ __launch_bounds__(256) void bcq_vae_loss_kernel(const float *__restrict__ recon, const int64_t ldr, const float *__restrict__ act,
                                                           const int64_t lda, const float *__restrict__ params, const int64_t ldp,
                                                           const float *__restrict__ stdv, const int64_t batch, const int A, const int L,
                                                           float *__restrict__ g_recon, float *__restrict__ g_mean, float *__restrict__ g_std,
                                                           float *__restrict__ loss_out, float *__restrict__ loss_sum)
{
    __shared__ double red[2][256];
    const int64_t n_rec = batch * A, n_lat = batch * L;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const float inv_rec = 1.0f / (float)n_rec, inv_lat = 1.0f / (float)n_lat;
    // d(loss)/d(kl sum element): 0.5 (weight) * -0.5 / (B L)
    const float c_kl = (0.5f * -0.5f) * inv_lat;
    if (g_recon)
        for (int64_t i = tid; i < n_rec; i += nthr) {
            const int64_t row = i / A;
            const int c = (int)(i - row * A);
            g_recon[i] = (2.0f * (recon[row * ldr + c] - act[row * lda + c])) * inv_rec;
        }
    if (g_mean || g_std)
        for (int64_t i = tid; i < n_lat; i += nthr) {
            const int64_t row = i / L;
            const int c = (int)(i - row * L);
            const float m = params[row * ldp + c], s = stdv[i];
            if (g_mean) g_mean[i] = c_kl * (-(2.0f * m));
            if (g_std) g_std[i] = c_kl * ((2.0f * s) / (s * s) - 2.0f * s);  // d log(s^2) = 2 s / s^2, d(-s^2) = -2 s
        }
    if (blockIdx.x != 0 || (!loss_out && !loss_sum)) return;
    double a_rec = 0.0, a_kl = 0.0;
    for (int64_t i = threadIdx.x; i < n_rec; i += 256) {
        const int64_t row = i / A;
        const int c = (int)(i - row * A);
        const float d = recon[row * ldr + c] - act[row * lda + c];
        a_rec += (double)(d * d);
    }
    for (int64_t i = threadIdx.x; i < n_lat; i += 256) {
        const int64_t row = i / L;
        const int c = (int)(i - row * L);
        const float m = params[row * ldp + c], s = stdv[i];
        a_kl += (double)(((1.0f + logf(s * s)) - m * m) - s * s);
    }
    red[0][threadIdx.x] = a_rec;
    red[1][threadIdx.x] = a_kl;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float rec = (float)(red[0][0] / (double)n_rec);
        const float kl = -0.5f * (float)(red[1][0] / (double)n_lat);
        const float loss = rec + 0.5f * kl;
        if (loss_out) loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
    }
}

// Backward of the latent: g_mean = g_z + dKL/dmean; g_log_std_raw = (g_z * eps + dKL/dstd) * std where -4 <= raw <= 15 (clamp's
// gradient is 1 on the closed interval), 0 elsewhere.
__global__ __launch_bounds__(256) void bcq_latent_bwd_kernel(const float *__restrict__ g_z, const int64_t ldg, const float *__restrict__ gkl_mean,
                                                             const float *__restrict__ gkl_std, const float *__restrict__ params,
                                                             const int64_t ldp, const float *__restrict__ stdv, const float *__restrict__ eps,
                                                             float *__restrict__ g_params, const int64_t batch, const int L)
{
    const int64_t total = batch * L;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / L;
        const int c = (int)(i - row * L);
        const float gz = g_z ? g_z[row * ldg + c] : 0.0f;
        const float raw = params[row * ldp + L + c];
        const float gs = gz * eps[i] + (gkl_std ? gkl_std[i] : 0.0f);
        const bool pass = raw >= LOG_STD_MIN && raw <= LOG_STD_MAX;
        g_params[row * 2 * L + c] = gz + (gkl_mean ? gkl_mean[i] : 0.0f);
        g_params[row * 2 * L + L + c] = pass ? gs * stdv[i] : 0.0f;
    }
}

// policies.py:122-124 / :247: row r = [state[r % n] | clamp(randn, -clip, clip)]; the state columns of up to two more row-major
// buffers (the perturbation net's and the critics' inputs) are filled by the same launch. VEC: the state rows are loaded and
// written into xdec as 16-byte vectors; va / vb: so are the rows of xa / xb (their row stride allows it).
template <bool VEC>
__global__ __launch_bounds__(256) void bcq_expand_kernel(const float *__restrict__ state, const int64_t lds, const int64_t n, const int64_t rows,
                                                         const int D, const int L, const float *__restrict__ noise,
                                                         uint64_t *__restrict__ rng_ctl, const float clip, float *__restrict__ xdec,
                                                         const int64_t ldx, float *__restrict__ xa, const int64_t lda, float *__restrict__ xb,
                                                         const int64_t ldb, const bool va, const bool vb)
{
    const int64_t total = rows * L, pairs = (total + 1) >> 1;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const uint64_t seed = rng_ctl ? rng_ctl[0] : 0ull, base = rng_ctl ? rng_ctl[1] : 0ull;
    for (int64_t p = tid; p < pairs; p += nthr) {
        float e[2] = {0.0f, 0.0f};
        if (rng_ctl) bcq_pair(seed, base + (uint64_t)p, e[0], e[1]);
        for (int k = 0; k < 2; ++k) {
            const int64_t i = 2 * p + k;
            if (i >= total) break;
            const int64_t row = i / L;
            const int c = (int)(i - row * L);
            const float v = rng_ctl ? e[k] : noise[i];
            xdec[row * ldx + D + c] = fminf(fmaxf(v, -clip), clip);
        }
    }
    if (VEC) {
        const int dv = D >> 2;
        const int64_t ncopy = rows * dv;
        for (int64_t j = tid; j < ncopy; j += nthr) {
            const int64_t row = j / dv;
            const int c = (int)(j - row * dv);
            const float4 v = reinterpret_cast<const float4 *>(state + (row % n) * lds)[c];
            reinterpret_cast<float4 *>(xdec + row * ldx)[c] = v;
            if (xa) {
                float *o = xa + row * lda + 4 * c;
                if (va) *reinterpret_cast<float4 *>(o) = v;
                else { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
            }
            if (xb) {
                float *o = xb + row * ldb + 4 * c;
                if (vb) *reinterpret_cast<float4 *>(o) = v;
                else { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
            }
        }
    } else {
        const int64_t ncopy = rows * D;
        for (int64_t j = tid; j < ncopy; j += nthr) {
            const int64_t row = j / D;
            const int c = (int)(j - row * D);
            const float v = state[(row % n) * lds + c];
            xdec[row * ldx + c] = v;
            if (xa) xa[row * lda + c] = v;
            if (xb) xb[row * ldb + c] = v;
        }
    }
    if (rng_ctl && last_block_ticket(reinterpret_cast<unsigned long long *>(rng_ctl + 2)) && threadIdx.x == 0)
        rng_ctl[1] = base + (uint64_t)pairs;
}

// policies.py:165-166
__global__ __launch_bounds__(256) void bcq_perturb_fwd_kernel(const float *__restrict__ a_vae, const int64_t lda, const float *__restrict__ p,
                                                              const int64_t ldp, const float mp, float *__restrict__ out, const int64_t ldo,
                                                              const int64_t rows, const int A)
{
    const int64_t total = rows * A;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / A;
        const int c = (int)(i - row * A);
        const float t = p[row * ldp + c] * mp;
        const float x = a_vae[row * lda + c] + t;
        out[row * ldo + c] = fminf(fmaxf(x, -1.0f), 1.0f);
    }
}

__global__ __launch_bounds__(256) void bcq_perturb_bwd_kernel(const float *__restrict__ g_out, const int64_t ldg, const float *__restrict__ a_vae,
                                                              const int64_t lda, const float *__restrict__ p, const int64_t ldp, const float mp,
                                                              float *__restrict__ g_p, const int64_t rows, const int A)
{
    const int64_t total = rows * A;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / A;
        const int c = (int)(i - row * A);
        const float t = p[row * ldp + c] * mp;
        const float x = a_vae[row * lda + c] + t;
        g_p[i] = (x >= -1.0f && x <= 1.0f) ? g_out[row * ldg + c] * mp : 0.0f;
    }
}

// bcq.py:167-173. grouping 0 = the reference's reshape(B, S): target row i takes flat entries S i ... S i + S - 1 of the
// [sample][state] layout; grouping 1 = state i's own candidates i, i + n, ..., i + n (S - 1).
__global__ __launch_bounds__(256) void bcq_target_kernel(const float *__restrict__ q, const int64_t q_stride, const int N, const int64_t n,
                                                         const int S, const int grouping, const float *__restrict__ rew,
                                                         const float *__restrict__ done, const float gamma, float *__restrict__ target,
                                                         float *__restrict__ max_q)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float best = 0.0f;
        for (int s = 0; s < S; ++s) {
            const int64_t idx = grouping == 0 ? i * S + s : i + n * s;
            float v = q[idx];
            for (int k = 1; k < N; ++k) v = fminf(v, q[k * q_stride + idx]);
            best = s == 0 ? v : fmaxf(best, v);
        }
        if (max_q) max_q[i] = best;
        if (target) target[i] = rew[i] + (1.0f - done[i]) * gamma * best;
    }
}

// policies.py:429-435 per state: first maximum of q1 over the candidates i, i + n, ...; the chosen row's action.
__global__ __launch_bounds__(256) void bcq_select_kernel(const float *__restrict__ q1, const float *__restrict__ cand, const int64_t ldc,
                                                         const int64_t n, const int S, const int A, int64_t *__restrict__ index_out,
                                                         float *__restrict__ action_out)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t arg = i;
        float best = q1[i];
        for (int s = 1; s < S; ++s) {
            const float v = q1[i + n * s];
            if (v > best) { best = v; arg = i + n * s; }
        }
        if (index_out) index_out[i] = arg;
        for (int c = 0; c < A; ++c) action_out[i * A + c] = cand[arg * ldc + c];
    }
}

inline bool overlap(const void *a, int64_t a_floats, const void *b, int64_t b_floats)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 4u * (uintptr_t)b_floats && b0 < a0 + 4u * (uintptr_t)a_floats;
}

// floats spanned by `rows` rows of `width` floats with row stride ld
inline int64_t span(int64_t rows, int64_t ld, int64_t width) { return (rows - 1) * ld + width; }

inline unsigned flat_grid(int64_t work)
{
    int64_t g = (work + 255) / 256;
    if (g < 1) g = 1;
    return (unsigned)(g < 2048 ? g : 2048);
}

}  // namespace

extern "C" int cstr_bcq_latent_fwd_f32(const float *params, int64_t ldp, const float *obs, int64_t ldo, const float *eps_in,
                                       uint64_t *rng_ctl, float *xdec, int64_t ldx, float *std_out, float *eps_out, int64_t batch,
                                       int obs_dim, int latent, cstr_stream_t stream)
{
    if (!params || !obs || !xdec || !std_out || batch <= 0 || obs_dim <= 0 || latent <= 0) return CSTR_E_BADARG;
    if ((eps_in == nullptr) == (rng_ctl == nullptr) || (rng_ctl && !eps_out)) return CSTR_E_BADARG;
    if (latent > CSTR_BCQ_MAX_LATENT || batch > CSTR_BCQ_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (ldp < 2 * (int64_t)latent || ldo < obs_dim || ldx < (int64_t)obs_dim + latent) return CSTR_E_BADARG;
    {
        // every output against every input and against every other output
        const int64_t sx = span(batch, ldx, obs_dim + latent), sp = span(batch, ldp, 2 * latent), so = span(batch, ldo, obs_dim);
        const int64_t bl = batch * latent;
        const void *ins[3] = {params, obs, eps_in};
        const int64_t in_n[3] = {sp, so, bl};
        const void *outs[3] = {xdec, std_out, eps_out};
        const int64_t out_n[3] = {sx, bl, bl};
        for (int o = 0; o < 3; ++o) {
            if (!outs[o]) continue;
            for (int i = 0; i < 3; ++i)
                if (ins[i] && overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
            for (int q = o + 1; q < 3; ++q)
                if (outs[q] && overlap(outs[o], out_n[o], outs[q], out_n[q])) return CSTR_E_BADARG;
        }
    }
    bcq_latent_fwd_kernel<<<flat_grid(batch * (latent > obs_dim ? latent : obs_dim)), 256, 0, (hipStream_t)stream>>>(
        params, ldp, obs, ldo, eps_in, rng_ctl, xdec, ldx, std_out, eps_out, batch, obs_dim, latent);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_vae_loss_f32(const float *recon, int64_t ldr, const float *act, int64_t lda, const float *params, int64_t ldp,
                                     const float *std, int64_t batch, int act_dim, int latent, float *g_recon, float *g_mean, float *g_std,
                                     float *loss_out, float *loss_sum, cstr_stream_t stream)
{
    if (!recon || !act || !params || !std || batch <= 0 || act_dim <= 0 || latent <= 0) return CSTR_E_BADARG;
    if (!g_recon && !g_mean && !g_std && !loss_out && !loss_sum) return CSTR_E_BADARG;
    if (latent > CSTR_BCQ_MAX_LATENT || act_dim > CSTR_BCQ_MAX_ACT || batch > CSTR_BCQ_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (ldr < act_dim || lda < act_dim || ldp < 2 * (int64_t)latent) return CSTR_E_BADARG;
    {
        const int64_t ba = batch * act_dim, bl = batch * latent;
        const void *ins[4] = {recon, act, params, std};
        const int64_t in_n[4] = {span(batch, ldr, act_dim), span(batch, lda, act_dim), span(batch, ldp, 2 * latent), bl};
        const void *outs[5] = {g_recon, g_mean, g_std, loss_out, loss_sum};
        const int64_t out_n[5] = {ba, bl, bl, 1, 1};
        for (int o = 0; o < 5; ++o) {
            if (!outs[o]) continue;
            for (int i = 0; i < 4; ++i)
                if (overlap(outs[o], out_n[o], ins[i], in_n[i])) return CSTR_E_BADARG;
            for (int q = o + 1; q < 5; ++q)
                if (outs[q] && overlap(outs[o], out_n[o], outs[q], out_n[q])) return CSTR_E_BADARG;
        }
    }
    bcq_vae_loss_kernel<<<flat_grid(batch * (latent > act_dim ? latent : act_dim)), 256, 0, (hipStream_t)stream>>>(
        recon, ldr, act, lda, params, ldp, std, batch, act_dim, latent, g_recon, g_mean, g_std, loss_out, loss_sum);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_latent_bwd_f32(const float *g_z, int64_t ldg, const float *g_mean_kl, const float *g_std_kl, const float *params,
                                       int64_t ldp, const float *std, const float *eps, float *g_params, int64_t batch, int latent,
                                       cstr_stream_t stream)
{
    if (!params || !std || !eps || !g_params || batch <= 0 || latent <= 0) return CSTR_E_BADARG;
    if (!g_z && !g_mean_kl && !g_std_kl) return CSTR_E_BADARG;
    if (latent > CSTR_BCQ_MAX_LATENT || batch > CSTR_BCQ_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (ldp < 2 * (int64_t)latent || (g_z && ldg < latent)) return CSTR_E_BADARG;
    if (overlap(g_params, batch * 2 * latent, params, span(batch, ldp, 2 * latent)) ||
        (g_z && overlap(g_params, batch * 2 * latent, g_z, span(batch, ldg, latent))))
        return CSTR_E_BADARG;
    bcq_latent_bwd_kernel<<<flat_grid(batch * latent), 256, 0, (hipStream_t)stream>>>(g_z, ldg, g_mean_kl, g_std_kl, params, ldp, std, eps,
                                                                                     g_params, batch, latent);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_expand_f32(const float *state, int64_t lds, int64_t n_states, int samples, int obs_dim, int latent,
                                   const float *noise, uint64_t *rng_ctl, float clip, float *xdec, int64_t ldx, float *xa, int64_t lda,
                                   float *xb, int64_t ldb, cstr_stream_t stream)
{
    if (!state || !xdec || n_states <= 0 || samples <= 0 || obs_dim <= 0 || latent <= 0) return CSTR_E_BADARG;
    if ((noise == nullptr) == (rng_ctl == nullptr) || !(clip >= 0.0f)) return CSTR_E_BADARG;
    if (latent > CSTR_BCQ_MAX_LATENT || samples > CSTR_BCQ_MAX_SAMPLES || n_states > CSTR_BCQ_MAX_ROWS / samples) return CSTR_E_UNSUPPORTED;
    if (lds < obs_dim || ldx < (int64_t)obs_dim + latent || (xa && lda < obs_dim) || (xb && ldb < obs_dim)) return CSTR_E_BADARG;
    const int64_t rows = n_states * samples;
    const int64_t sx = span(rows, ldx, obs_dim + latent), ss = span(n_states, lds, obs_dim), sa = span(rows, lda, obs_dim), sb = span(rows, ldb, obs_dim);
    if (overlap(xdec, sx, state, ss) || (xa && overlap(xa, sa, state, ss)) || (xb && overlap(xb, sb, state, ss)) ||
        (xa && overlap(xa, sa, xdec, sx)) || (xb && overlap(xb, sb, xdec, sx)) || (xa && xb && overlap(xa, sa, xb, sb)))
        return CSTR_E_BADARG;
    const bool vec = obs_dim % 4 == 0 && aligned16(state) && aligned16(xdec) && lds % 4 == 0 && ldx % 4 == 0;
    const bool va = xa && aligned16(xa) && lda % 4 == 0, vb = xb && aligned16(xb) && ldb % 4 == 0;
    const unsigned grid = flat_grid(rows * (latent > obs_dim ? latent : obs_dim));
    if (vec)
        bcq_expand_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(state, lds, n_states, rows, obs_dim, latent, noise, rng_ctl, clip, xdec, ldx,
                                                                        xa, lda, xb, ldb, va, vb);
    else
        bcq_expand_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(state, lds, n_states, rows, obs_dim, latent, noise, rng_ctl, clip, xdec, ldx,
                                                                         xa, lda, xb, ldb, va, vb);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_perturb_fwd_f32(const float *a_vae, int64_t lda, const float *p, int64_t ldp, float max_perturbation, float *out,
                                        int64_t ldo, int64_t rows, int act_dim, cstr_stream_t stream)
{
    if (!a_vae || !p || !out || rows <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if (act_dim > CSTR_BCQ_MAX_ACT || rows > CSTR_BCQ_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (lda < act_dim || ldp < act_dim || ldo < act_dim) return CSTR_E_BADARG;
    if (overlap(out, span(rows, ldo, act_dim), a_vae, span(rows, lda, act_dim)) || overlap(out, span(rows, ldo, act_dim), p, span(rows, ldp, act_dim))) return CSTR_E_BADARG;
    bcq_perturb_fwd_kernel<<<flat_grid(rows * act_dim), 256, 0, (hipStream_t)stream>>>(a_vae, lda, p, ldp, max_perturbation, out, ldo, rows,
                                                                                      act_dim);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_perturb_bwd_f32(const float *g_out, int64_t ldg, const float *a_vae, int64_t lda, const float *p, int64_t ldp,
                                        float max_perturbation, float *g_p, int64_t rows, int act_dim, cstr_stream_t stream)
{
    if (!g_out || !a_vae || !p || !g_p || rows <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if (act_dim > CSTR_BCQ_MAX_ACT || rows > CSTR_BCQ_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (ldg < act_dim || lda < act_dim || ldp < act_dim) return CSTR_E_BADARG;
    if (overlap(g_p, rows * act_dim, g_out, span(rows, ldg, act_dim)) || overlap(g_p, rows * act_dim, a_vae, span(rows, lda, act_dim)) ||
        overlap(g_p, rows * act_dim, p, span(rows, ldp, act_dim)))
        return CSTR_E_BADARG;
    bcq_perturb_bwd_kernel<<<flat_grid(rows * act_dim), 256, 0, (hipStream_t)stream>>>(g_out, ldg, a_vae, lda, p, ldp, max_perturbation, g_p, rows,
                                                                                      act_dim);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_target_f32(const float *q, int64_t q_stride, int n_critics, int64_t n_states, int samples, int grouping,
                                   const float *rew, const float *done, float gamma, float *target_out, float *max_q_out,
                                   cstr_stream_t stream)
{
    if (!q || n_critics <= 0 || n_states <= 0 || samples <= 0 || (!target_out && !max_q_out)) return CSTR_E_BADARG;
    if (target_out && (!rew || !done)) return CSTR_E_BADARG;
    if (grouping != 0 && grouping != 1) return CSTR_E_BADARG;
    if (n_critics > CSTR_MAX_ENS_CRITICS || samples > CSTR_BCQ_MAX_SAMPLES || n_states > CSTR_BCQ_MAX_ROWS / samples) return CSTR_E_UNSUPPORTED;
    const int64_t rows = n_states * samples;
    if (n_critics > 1 && q_stride < rows) return CSTR_E_BADARG;
    const int64_t q_floats = (n_critics - 1) * q_stride + rows;
    if ((target_out && overlap(target_out, n_states, q, q_floats)) || (max_q_out && overlap(max_q_out, n_states, q, q_floats)))
        return CSTR_E_BADARG;
    bcq_target_kernel<<<flat_grid(n_states), 256, 0, (hipStream_t)stream>>>(q, q_stride, n_critics, n_states, samples, grouping, rew, done, gamma,
                                                                            target_out, max_q_out);
    return (int)hipGetLastError();
}

extern "C" int cstr_bcq_select_f32(const float *q1, const float *cand, int64_t ldc, int64_t n_states, int samples, int act_dim,
                                   int64_t *index_out, float *action_out, cstr_stream_t stream)
{
    if (!q1 || !cand || !action_out || n_states <= 0 || samples <= 0 || act_dim <= 0) return CSTR_E_BADARG;
    if (act_dim > CSTR_BCQ_MAX_ACT || samples > CSTR_BCQ_MAX_SAMPLES || n_states > CSTR_BCQ_MAX_ROWS / samples) return CSTR_E_UNSUPPORTED;
    if (ldc < act_dim) return CSTR_E_BADARG;
    if (overlap(action_out, n_states * act_dim, cand, span(n_states * samples, ldc, act_dim)) || overlap(action_out, n_states * act_dim, q1, n_states * samples))
        return CSTR_E_BADARG;
    bcq_select_kernel<<<flat_grid(n_states), 256, 0, (hipStream_t)stream>>>(q1, cand, ldc, n_states, samples, act_dim, index_out, action_out);
    return (int)hipGetLastError();
}
