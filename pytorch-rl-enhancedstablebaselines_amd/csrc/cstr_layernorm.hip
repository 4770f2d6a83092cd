// cstr_layernorm.hip -- layer-normalised, dropout-regularised Q networks (DroQ, Hiraoka et al. 2022; the layer_norm / dropout_rate
// critics of SBX, RLPD, BRO): one hidden layer  y = act(LN(drop(x W^T + b)) * gamma + beta)  and its backward, f32 in and out, gfx950.
//
// How the work is split. LayerNorm's statistics belong to ONE row, so a workgroup (4 waves) owns 16 batch rows of one Q network
// (group g of the stacked [G, ...] operands) across ALL N <= 512 columns of the layer: a row's sums never leave the workgroup, no
// workgroup waits for another, and everything between two GEMMs is an epilogue on the accumulators.
//   * GEMM: v_mfma_f32_16x16x4_f32 (exact f32 fma chains). The 16-wide column tiles are dealt to the waves round-robin (tile t to wave
//     t & 3, at most 8 per wave, possibly one or none); the [16, K] left operand is staged ONCE in LDS for all four waves in chunks of
//     128 k (zero-filled past M and K), the right operand streams from L2. A lane feeds element e of a 4-float group to MFMA step e for
//     both operands: the k order inside a 16-wide chunk is permuted identically, which a sum over k does not see.
//   * forward epilogue, in the C/D layout (column = lane & 15, row = 4 * (lane >> 4) + register): bias, dropout, then two-pass
//     statistics in float32 from the accumulators -- the row mean first, then the CENTRED sum of squares, never E[x^2] - E[x]^2.
//     A row sum = the lane's tiles in order, an xor tree over the 16 lanes of a row, the four waves' partials from LDS in wave order.
//     Tail columns (N not a multiple of 16) and tail rows take no part in any sum. It writes y, the normalised pre-affine xhat and
//     rstd: the backward never recomputes the forward.
//   * backward (cstr_ln_linear_bwd_input_f32), the mirror image: g_y = gz_next W_next gives complete [16, N] rows (a scalar Q head,
//     N_next = 1, is an outer product on the VALU), and the epilogue is the layer's own backward
//         g_ln = g_y act'(y);  g_xhat = g_ln gamma;  gz = rstd (g_xhat - mean(g_xhat) - xhat mean(g_xhat xhat)) keep / (1 - p)
//     It leaves per-workgroup column partials of d gamma = sum g_ln xhat and d beta = sum g_ln in float64; a second, tiny launch behind
//     the same entry point adds them in workgroup order into the gradient arena (a launch of its own, not a finishing workgroup: no
//     ticket, no hand-over inside a launch). No float atomics anywhere: a relaunch gives the same bits.
//   * dropout: keep = u >= p with u = philox_uniform of Philox4x32-10 keyed by rng_ctl[0], counter words (row, column / 4 | group << 8 |
//     layer << 16, lo32(pass), tag ^ hi32(pass)), word column & 3. The pass counter is rng_ctl[1], read on the device; the launch that
//     ends a pass advances it (last workgroup out), so a captured graph replays fresh masks. The forward records the counter it used
//     (pass_out); the backward regenerates the mask from that word: no mask is stored. The 16 x N uniforms of a workgroup are drawn
//     once, one Philox call per four columns, into LDS; u_in [G, M, N] replaces the stream, and cstr_ln_dropout_uniform_f32 writes the
//     stream's uniforms with the same device function. p = 0 is a compile-time variant without any of it.
// Nothing here allocates, synchronises or keeps host state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_rng_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ACT_RELU = CSTR_ACT_RELU, ACT_TANH = CSTR_ACT_TANH;
constexpr int LN_MAX_N = CSTR_LN_MAX_WIDTH;  // 512 columns = 32 tiles
constexpr int TPW = LN_MAX_N / 64;           // tiles per wave
constexpr int KC = 128, LDA = KC + 4;        // staged k chunk of the left operand and its padded LDS row
constexpr int LDU = LN_MAX_N + 4;            // LDS row of the uniforms
constexpr int DROP_NONE = 0, DROP_STREAM = 1, DROP_GIVEN = 2;
constexpr uint32_t LN_TAG = CSTR_LN_TAG;
constexpr float LN_EPS = 1e-5f;  // torch.nn.LayerNorm's default

// the four uniforms of (pass, layer, group, row, columns 4j .. 4j + 3)
__device__ __forceinline__ float4 ln_uniform4(const uint64_t seed, const uint64_t pass, const int layer, const int g, const int row, const int j)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)row, (uint32_t)j | ((uint32_t)g << 8) | ((uint32_t)layer << 16), (uint32_t)pass, LN_TAG ^ (uint32_t)(pass >> 32),
                  (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return make_float4(philox_uniform(w[0]), philox_uniform(w[1]), philox_uniform(w[2]), philox_uniform(w[3]));
}

// The workgroup's 16 x N uniforms into LDS (rows past M: 1, kept): drawn (DROP_STREAM) or copied from u_in (DROP_GIVEN).
template <int DROP>
__device__ __forceinline__ void stage_uniforms(float (*s_u)[LDU], const float *u_in, const uint64_t seed, const uint64_t pass, const int layer,
                                               const int g, const int m0, const int M, const int N)
{
    if (DROP == DROP_STREAM) {
        const int nj = (N + 3) >> 2;
        for (int i = threadIdx.x; i < 16 * nj; i += 256) {
            const int r = i / nj, j = i - r * nj;
            const float4 u = m0 + r < M ? ln_uniform4(seed, pass, layer, g, m0 + r, j) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            *reinterpret_cast<float4 *>(&s_u[r][4 * j]) = u;
        }
    } else if (DROP == DROP_GIVEN) {
        for (int i = threadIdx.x; i < 16 * N; i += 256) {
            const int r = i / N, c = i - r * N;
            s_u[r][c] = m0 + r < M ? u_in[((int64_t)g * M + m0 + r) * N + c] : 1.0f;
        }
    }
}

// Sums of v[e] (e = the lane's four rows) over a row's columns: xor tree over the 16 lanes of a row, the waves' partials in wave order.
// Every lane of the workgroup calls it; every lane gets the sums of its own four rows. `sm` is used by this call alone.
__device__ __forceinline__ void row_sums(float (&v)[4], float (*sm)[16])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v[e] += __shfl_xor(v[e], o, 64);
        if (r == 0) sm[wave][4 * h + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((sm[0][4 * h + e] + sm[1][4 * h + e]) + sm[2][4 * h + e]) + sm[3][4 * h + e];
}

// last workgroup out (2-D grid): every workgroup has consumed the control words it read before it takes a ticket
__device__ __forceinline__ bool last_block_2d(unsigned long long *ticket)
{
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y, t = atomicAdd(ticket, 1ULL);
        is_last = t == total - 1ULL;
        if (is_last) *ticket = 0ULL;  // self-reset for the next launch
    }
    __syncthreads();
    return is_last != 0;
}

struct LnFwdArgs {
    const float *x, *w, *bias, *gamma, *beta, *u_in;
    int64_t x_group_stride;
    int ldx, M, N, K;
    float p, keep_div;  // keep_div = 1 - p: kept values are DIVIDED by it, as the statement x * mask / (1 - p) does
    uint64_t *rng_ctl, *pass_out;
    int advance, layer;
    float *y, *xhat, *rstd;
};

template <int ACT, int DROP>
__global__ __launch_bounds__(256) void linear_ln_act_fwd_kernel(const LnFwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_a[16][LDA];
    __shared__ __attribute__((aligned(16))) float s_u[DROP != DROP_NONE ? 16 : 1][LDU];
    __shared__ float s_r0[4][16], s_r1[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    const int M = a.M, N = a.N, K = a.K, m0 = blockIdx.x * 16, g = blockIdx.y;
    const int ntiles = (N + 15) >> 4;
    const float *xg = a.x + (int64_t)g * a.x_group_stride;
    const float *wg = a.w + (int64_t)g * N * K;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(wg) & 15u) == 0;
    uint64_t seed = 0, pass = 0;
    if (DROP == DROP_STREAM) {
        seed = a.rng_ctl[0];
        pass = a.rng_ctl[1];
    }
    f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kb = 0; kb < K; kb += KC) {
        if (kb > 0) __syncthreads();  // the previous chunk has been read
        for (int i = tid; i < 16 * KC; i += 256) {
            const int rr = i / KC, kk = i - rr * KC;
            s_a[rr][kk] = (m0 + rr < M && kb + kk < K) ? xg[(int64_t)(m0 + rr) * a.ldx + kb + kk] : 0.0f;
        }
        __syncthreads();
        const int kend = min(KC, K - kb);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = wave + 4 * i;
            if (t < ntiles) {
                const int n = min(16 * t + r, N - 1);  // a tail column reads the last row of W: its products are never used
                const float *wr = wg + (int64_t)n * K + kb;
                for (int c = 0; c < kend; c += 16) {
                    const int k = c + 4 * h;
                    const float4 av = *reinterpret_cast<const float4 *>(&s_a[r][k]);
                    float4 bv;
                    if (vec) {
                        bv = k < kend ? *reinterpret_cast<const float4 *>(wr + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    } else {
                        bv.x = k < kend ? wr[k] : 0.0f;
                        bv.y = k + 1 < kend ? wr[k + 1] : 0.0f;
                        bv.z = k + 2 < kend ? wr[k + 2] : 0.0f;
                        bv.w = k + 3 < kend ? wr[k + 3] : 0.0f;
                    }
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[i], 0, 0, 0);
                }
            }
        }
    }
    if (DROP != DROP_NONE) {
        stage_uniforms<DROP>(s_u, a.u_in, seed, pass, a.layer, g, m0, M, N);
        __syncthreads();
    }
    // bias and dropout; the row mean
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int col = 16 * (wave + 4 * i) + r;
        if (col < N) {
            const float bv = a.bias[(int64_t)g * N + col];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d = acc[i][e] + bv;
                if (DROP != DROP_NONE) d = s_u[4 * h + e][col] >= a.p ? d / a.keep_div : 0.0f;
                acc[i][e] = d;
                s[e] += d;
            }
        }
    }
    row_sums(s, s_r0);
    float mean[4], q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e) mean[e] = s[e] / (float)N;
    // the centred sum of squares
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        if (16 * (wave + 4 * i) + r < N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c = acc[i][e] - mean[e];
                acc[i][e] = c;
                q[e] += c * c;
            }
        }
    }
    row_sums(q, s_r1);
    float rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) rs[e] = 1.0f / sqrtf(q[e] / (float)N + LN_EPS);
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int col = 16 * (wave + 4 * i) + r;
        if (col < N) {
            const float gm = a.gamma[(int64_t)g * N + col], bt = a.beta[(int64_t)g * N + col];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + 4 * h + e;
                if (row < M) {
                    const float xh = acc[i][e] * rs[e];
                    float v = xh * gm + bt;
                    if (ACT == ACT_RELU) v = fmaxf(v, 0.0f);
                    if (ACT == ACT_TANH) v = tanhf(v);
                    const int64_t at = ((int64_t)g * M + row) * N + col;
                    a.xhat[at] = xh;
                    a.y[at] = v;
                }
            }
        }
    }
    if (wave == 0 && r == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (m0 + 4 * h + e < M) a.rstd[(int64_t)g * M + m0 + 4 * h + e] = rs[e];
    }
    if (DROP == DROP_STREAM) {
        if (a.pass_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.pass_out[0] = pass;
        if (a.advance && last_block_2d(reinterpret_cast<unsigned long long *>(a.rng_ctl + 2)) && tid == 0) a.rng_ctl[1] = pass + 1;
    }
}

struct LnBwdArgs {
    const float *gz_next, *w_next, *y, *xhat, *rstd, *gamma, *u_in;
    int M, N, Nn;
    float p, keep_div;  // keep_div = 1 - p: kept values are DIVIDED by it, as the statement x * mask / (1 - p) does
    const uint64_t *rng_ctl, *pass_ctr;
    int layer;
    float *gz;
    double *parts;  // [G][row blocks][2][N] or NULL (frozen parameters)
};

// HEAD: the consumer is the scalar Q head (Nn = 1): g_y = gq (outer) w_head on the VALU
template <int ACT, int DROP, bool HEAD>
__global__ __launch_bounds__(256) void ln_linear_bwd_input_kernel(const LnBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_a[HEAD ? 1 : 16][LDA];
    __shared__ __attribute__((aligned(16))) float s_u[DROP != DROP_NONE ? 16 : 1][LDU];
    __shared__ float s_r0[4][16], s_r1[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    const int M = a.M, N = a.N, Nn = a.Nn, m0 = blockIdx.x * 16, g = blockIdx.y;
    const int ntiles = (N + 15) >> 4;
    const float *wn = a.w_next + (int64_t)g * Nn * N;
    const float *gn = a.gz_next + (int64_t)g * M * Nn;
    f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (HEAD) {
        float gq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) gq[e] = m0 + 4 * h + e < M ? gn[m0 + 4 * h + e] : 0.0f;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int col = 16 * (wave + 4 * i) + r;
            if (col < N) {
                const float wv = wn[col];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][e] = gq[e] * wv;
            }
        }
    } else {
        for (int kb = 0; kb < Nn; kb += KC) {
            if (kb > 0) __syncthreads();
            for (int i = tid; i < 16 * KC; i += 256) {
                const int rr = i / KC, kk = i - rr * KC;
                s_a[rr][kk] = (m0 + rr < M && kb + kk < Nn) ? gn[(int64_t)(m0 + rr) * Nn + kb + kk] : 0.0f;
            }
            __syncthreads();
            const int kend = min(KC, Nn - kb);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int t = wave + 4 * i;
                if (t < ntiles) {
                    const int col = min(16 * t + r, N - 1);  // a tail column repeats the last one: never used
                    const float *wc = wn + (int64_t)kb * N + col;
                    for (int c = 0; c < kend; c += 16) {
                        const int k = c + 4 * h;
                        const float4 av = *reinterpret_cast<const float4 *>(&s_a[r][k]);
                        const float b0 = k < kend ? wc[(int64_t)k * N] : 0.0f;
                        const float b1 = k + 1 < kend ? wc[(int64_t)(k + 1) * N] : 0.0f;
                        const float b2 = k + 2 < kend ? wc[(int64_t)(k + 2) * N] : 0.0f;
                        const float b3 = k + 3 < kend ? wc[(int64_t)(k + 3) * N] : 0.0f;
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc[i], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (DROP != DROP_NONE) {
        uint64_t seed = 0, pass = 0;
        if (DROP == DROP_STREAM) {
            seed = a.rng_ctl[0];
            pass = a.pass_ctr[0];
        }
        stage_uniforms<DROP>(s_u, a.u_in, seed, pass, a.layer, g, m0, M, N);
        __syncthreads();
    }
    // g_ln = g_y act'(y) (kept in acc), xhat, the two row sums of g_xhat and g_xhat xhat
    f32x4 xh[TPW];
    float gam[TPW];
    float s1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int col = 16 * (wave + 4 * i) + r;
        xh[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        gam[i] = 0.0f;
        if (col < N) {
            gam[i] = a.gamma[(int64_t)g * N + col];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + 4 * h + e;
                float gl = 0.0f;
                if (row < M) {
                    const int64_t at = ((int64_t)g * M + row) * N + col;
                    const float yv = a.y[at];
                    xh[i][e] = a.xhat[at];
                    gl = ACT == ACT_RELU ? (yv > 0.0f ? acc[i][e] : 0.0f) : acc[i][e] * (1.0f - yv * yv);
                }
                acc[i][e] = gl;
                const float gx = gl * gam[i];
                s1[e] += gx;
                s2[e] += gx * xh[i][e];
            }
        } else {
            acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    row_sums(s1, s_r0);
    row_sums(s2, s_r1);
    float rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s1[e] = s1[e] / (float)N;
        s2[e] = s2[e] / (float)N;
        rs[e] = m0 + 4 * h + e < M ? a.rstd[(int64_t)g * M + m0 + 4 * h + e] : 0.0f;
    }
    const int nblk = gridDim.x;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int col = 16 * (wave + 4 * i) + r;
        if (16 * (wave + 4 * i) < N) {  // the whole wave: the shuffles below need every lane of the tile
            double pg = 0.0, pb = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + 4 * h + e;
                const float gl = acc[i][e], xv = xh[i][e];
                if (row < M && col < N) {
                    float v = rs[e] * ((gl * gam[i] - s1[e]) - xv * s2[e]);
                    if (DROP != DROP_NONE) v = s_u[4 * h + e][col] >= a.p ? v / a.keep_div : 0.0f;
                    a.gz[((int64_t)g * M + row) * N + col] = v;
                }
                pg += (double)gl * (double)xv;  // rows past M and tail columns hold zeros
                pb += (double)gl;
            }
            if (a.parts) {  // the 16 rows of the workgroup: the lane's four, then the four lane groups
                pg += __shfl_xor(pg, 16, 64);
                pb += __shfl_xor(pb, 16, 64);
                pg += __shfl_xor(pg, 32, 64);
                pb += __shfl_xor(pb, 32, 64);
                if (h == 0 && col < N) {
                    double *o = a.parts + (((int64_t)g * nblk + blockIdx.x) * 2) * N + col;
                    o[0] = pg;
                    o[N] = pb;
                }
            }
        }
    }
}

// d gamma, d beta [G][N]: the workgroups' partials in workgroup order, float64
__global__ __launch_bounds__(256) void ln_param_grad_finish_kernel(const double *parts, float *dgamma, float *dbeta, const int nblk, const int N)
{
    const int col = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (col >= N) return;
    const double *p = parts + (int64_t)g * nblk * 2 * N + col;
    double sg = 0.0, sb = 0.0;
    for (int b = 0; b < nblk; ++b) {
        sg += p[(int64_t)b * 2 * N];
        sb += p[(int64_t)b * 2 * N + N];
    }
    dgamma[(int64_t)g * N + col] = (float)sg;
    dbeta[(int64_t)g * N + col] = (float)sb;
}

__global__ __launch_bounds__(256) void ln_dropout_uniform_kernel(float *u, const uint64_t *rng_ctl, const uint64_t *pass_ctr, const int layer,
                                                                 const int M, const int N)
{
    const uint64_t seed = rng_ctl[0], pass = pass_ctr ? pass_ctr[0] : rng_ctl[1];
    const int nj = (N + 3) >> 2, g = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)M * nj) return;
    const int row = (int)(i / nj), j = (int)(i - (int64_t)row * nj);
    const float4 v = ln_uniform4(seed, pass, layer, g, row, j);
    const float e[4] = {v.x, v.y, v.z, v.w};
    float *o = u + ((int64_t)g * M + row) * N;
    for (int c = 0; c < 4; ++c)
        if (4 * j + c < N) o[4 * j + c] = e[c];
}

inline bool aligned(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0; }

inline bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

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

// which dropout variant a call asks for; -1: a contradiction
inline int drop_mode(double p, const void *u_in, const void *rng_ctl)
{
    if (p == 0.0) return (u_in || rng_ctl) ? -1 : DROP_NONE;
    if ((u_in != nullptr) == (rng_ctl != nullptr)) return -1;
    return u_in ? DROP_GIVEN : DROP_STREAM;
}

inline bool shape_ok(int64_t groups, int64_t m, int64_t n) { return groups <= CSTR_MAX_ENS_CRITICS && m <= (1 << 20) && groups * m * n < (1ll << 31); }

template <int ACT>
void launch_fwd(int drop, dim3 grid, hipStream_t st, const LnFwdArgs &a)
{
    if (drop == DROP_NONE) linear_ln_act_fwd_kernel<ACT, DROP_NONE><<<grid, 256, 0, st>>>(a);
    else if (drop == DROP_STREAM) linear_ln_act_fwd_kernel<ACT, DROP_STREAM><<<grid, 256, 0, st>>>(a);
    else linear_ln_act_fwd_kernel<ACT, DROP_GIVEN><<<grid, 256, 0, st>>>(a);
}

template <int ACT, bool HEAD>
void launch_bwd(int drop, dim3 grid, hipStream_t st, const LnBwdArgs &a)
{
    if (drop == DROP_NONE) ln_linear_bwd_input_kernel<ACT, DROP_NONE, HEAD><<<grid, 256, 0, st>>>(a);
    else if (drop == DROP_STREAM) ln_linear_bwd_input_kernel<ACT, DROP_STREAM, HEAD><<<grid, 256, 0, st>>>(a);
    else ln_linear_bwd_input_kernel<ACT, DROP_GIVEN, HEAD><<<grid, 256, 0, st>>>(a);
}

}  // namespace

extern "C" int cstr_ln_supported(int64_t k, int64_t n, double p, int act)
{
    return k >= 1 && n >= 1 && n <= CSTR_LN_MAX_WIDTH && p >= 0.0 && p < 1.0 && (act == CSTR_ACT_RELU || act == CSTR_ACT_TANH);
}

extern "C" int cstr_linear_ln_act_fwd_f32(const float *x, int64_t x_group_stride, int64_t ldx, const float *w, const float *bias,
                                          const float *gamma, const float *beta, int act, double p, const float *u_in, uint64_t *rng_ctl,
                                          int advance, uint64_t *pass_out, int layer, float *y, float *xhat, float *rstd, int64_t groups,
                                          int64_t m, int64_t n, int64_t k, cstr_stream_t stream)
{
    if (!x || !w || !bias || !gamma || !beta || !y || !xhat || !rstd || groups <= 0 || m <= 0 || n <= 0 || k <= 0) return CSTR_E_BADARG;
    if (ldx < k || x_group_stride < 0 || layer < 0 || layer > 0xFFFF || !(p >= 0.0)) return CSTR_E_BADARG;
    const int drop = drop_mode(p, u_in, rng_ctl);
    if (drop < 0) return CSTR_E_BADARG;
    if (!cstr_ln_supported(k, n, p, act) || !shape_ok(groups, m, n) || ldx >= (1ll << 31)) return CSTR_E_UNSUPPORTED;
    const int64_t x_bytes = 4 * ((groups - 1) * x_group_stride + (m - 1) * ldx + k), out_bytes = 4 * groups * m * n, vec = 4 * groups * n;
    const void *ins[7] = {x, w, bias, gamma, beta, u_in, rng_ctl};
    const int64_t in_b[7] = {x_bytes, 4 * groups * n * k, vec, vec, vec, out_bytes, 8 * CSTR_RNG_CTL_WORDS};
    const void *outs[4] = {y, xhat, rstd, pass_out};
    const int64_t out_b[4] = {out_bytes, out_bytes, 4 * groups * m, 8};
    for (int i = 0; i < 6; ++i)
        if (!aligned(ins[i], 4)) return CSTR_E_BADARG;
    if (!aligned(rng_ctl, 8) || !aligned(pass_out, 8) || !aligned(y, 4) || !aligned(xhat, 4) || !aligned(rstd, 4)) return CSTR_E_BADARG;
    if (any_overlap(ins, in_b, 7, outs, out_b, 4)) return CSTR_E_BADARG;
    LnFwdArgs a;
    a.x = x; a.w = w; a.bias = bias; a.gamma = gamma; a.beta = beta; a.u_in = u_in; a.x_group_stride = x_group_stride;
    a.ldx = (int)ldx; a.M = (int)m; a.N = (int)n; a.K = (int)k; a.p = (float)p; a.keep_div = (float)(1.0 - p);
    a.rng_ctl = rng_ctl; a.pass_out = pass_out; a.advance = advance; a.layer = layer; a.y = y; a.xhat = xhat; a.rstd = rstd;
    const dim3 grid((unsigned)((m + 15) / 16), (unsigned)groups);
    if (act == CSTR_ACT_RELU) launch_fwd<ACT_RELU>(drop, grid, (hipStream_t)stream, a);
    else launch_fwd<ACT_TANH>(drop, grid, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int cstr_ln_linear_bwd_input_f32(const float *gz_next, const float *w_next, int64_t n_next, const float *y, const float *xhat,
                                            const float *rstd, const float *gamma, int act, double p, const float *u_in,
                                            const uint64_t *rng_ctl, const uint64_t *pass_ctr, int layer, float *gz, double *parts,
                                            float *dgamma, float *dbeta, int64_t groups, int64_t m, int64_t n, cstr_stream_t stream)
{
    if (!gz_next || !w_next || !y || !xhat || !rstd || !gamma || !gz || groups <= 0 || m <= 0 || n <= 0 || n_next <= 0) return CSTR_E_BADARG;
    if (layer < 0 || layer > 0xFFFF || !(p >= 0.0)) return CSTR_E_BADARG;
    if ((dgamma != nullptr) != (dbeta != nullptr) || (dgamma != nullptr) != (parts != nullptr)) return CSTR_E_BADARG;
    const int drop = drop_mode(p, u_in, rng_ctl);
    if (drop < 0 || (drop == DROP_STREAM && !pass_ctr)) return CSTR_E_BADARG;
    if (!cstr_ln_supported(n_next, n, p, act) || !shape_ok(groups, m, n) || !shape_ok(groups, m, n_next)) return CSTR_E_UNSUPPORTED;
    const int64_t nblk = (m + 15) / 16, full = 4 * groups * m * n, vec = 4 * groups * n;
    const void *ins[9] = {gz_next, w_next, y, xhat, rstd, gamma, u_in, rng_ctl, pass_ctr};
    const int64_t in_b[9] = {4 * groups * m * n_next, 4 * groups * n_next * n, full, full, 4 * groups * m, vec, full, 8 * CSTR_RNG_CTL_WORDS, 8};
    const void *outs[4] = {gz, parts, dgamma, dbeta};
    const int64_t out_b[4] = {full, 16 * groups * nblk * n, vec, vec};
    for (int i = 0; i < 7; ++i)
        if (!aligned(ins[i], 4)) return CSTR_E_BADARG;
    if (!aligned(rng_ctl, 8) || !aligned(pass_ctr, 8) || !aligned(parts, 8) || !aligned(gz, 4) || !aligned(dgamma, 4) || !aligned(dbeta, 4))
        return CSTR_E_BADARG;
    if (any_overlap(ins, in_b, 9, outs, out_b, 4)) return CSTR_E_BADARG;
    LnBwdArgs a;
    a.gz_next = gz_next; a.w_next = w_next; a.y = y; a.xhat = xhat; a.rstd = rstd; a.gamma = gamma; a.u_in = u_in;
    a.M = (int)m; a.N = (int)n; a.Nn = (int)n_next; a.p = (float)p; a.keep_div = (float)(1.0 - p);
    a.rng_ctl = rng_ctl; a.pass_ctr = pass_ctr; a.layer = layer; a.gz = gz; a.parts = parts;
    const dim3 grid((unsigned)nblk, (unsigned)groups);
    hipStream_t st = (hipStream_t)stream;
    if (n_next == 1) {
        if (act == CSTR_ACT_RELU) launch_bwd<ACT_RELU, true>(drop, grid, st, a);
        else launch_bwd<ACT_TANH, true>(drop, grid, st, a);
    } else {
        if (act == CSTR_ACT_RELU) launch_bwd<ACT_RELU, false>(drop, grid, st, a);
        else launch_bwd<ACT_TANH, false>(drop, grid, st, a);
    }
    int rc = (int)hipGetLastError();
    if (rc != 0 || !parts) return rc;
    ln_param_grad_finish_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)groups), 256, 0, st>>>(parts, dgamma, dbeta, (int)nblk, (int)n);
    return (int)hipGetLastError();
}

extern "C" int cstr_ln_dropout_uniform_f32(float *u_out, const uint64_t *rng_ctl, const uint64_t *pass_ctr, int layer, int64_t groups,
                                           int64_t m, int64_t n, cstr_stream_t stream)
{
    if (!u_out || !rng_ctl || groups <= 0 || m <= 0 || n <= 0 || layer < 0 || layer > 0xFFFF) return CSTR_E_BADARG;
    if (!aligned(u_out, 4) || !aligned(rng_ctl, 8) || !aligned(pass_ctr, 8)) return CSTR_E_BADARG;
    if (n > CSTR_LN_MAX_WIDTH || !shape_ok(groups, m, n)) return CSTR_E_UNSUPPORTED;
    if (overlap(u_out, 4 * groups * m * n, rng_ctl, 8 * CSTR_RNG_CTL_WORDS) || (pass_ctr && overlap(u_out, 4 * groups * m * n, pass_ctr, 8)))
        return CSTR_E_BADARG;
    const int64_t quads = m * ((n + 3) / 4);
    ln_dropout_uniform_kernel<<<dim3((unsigned)((quads + 255) / 256), (unsigned)groups), 256, 0, (hipStream_t)stream>>>(u_out, rng_ctl, pass_ctr, layer,
                                                                                                                   (int)m, (int)n);
    return (int)hipGetLastError();
}
