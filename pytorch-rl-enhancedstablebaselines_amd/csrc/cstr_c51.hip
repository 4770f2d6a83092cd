// cstr_c51.hip -- categorical DQN's own arithmetic (Bellemare, Dabney & Munos 2017, "A Distributional Perspective on Reinforcement
// Learning"; core/c51/c51.py) around the categorical network's Linear layers, f32 in and out, gfx950. The face is DQN's (M = K * K
// indices over two valves of K levels); a state has a softmax over N atoms per action on the fixed support z_i = v_min + i * dz,
// dz = (v_max - v_min) / (N - 1). A row of logits is [M][N]: atom i of action a at a * N + i (`logits.view(-1, M, N)`), ACTION-major,
// so the N rows of the last layer's weight that belong to one action are contiguous.
//
// cstr_c51_head_q_f32: the rollout and `predict` need q[r][a] = sum_i z_i softmax_i(h[r] . w[a * N + i] + bias[a * N + i]) only. The
//   expectation is not linear in the last layer (QR-DQN's fold does not apply), so the head GEMM, the softmax and the expectation run
//   in ONE launch and the [rows][M * N] logits never exist, not even in LDS:
//     * a 256-lane workgroup owns 16 rows; their hidden tile [16][H] sits in LDS (row stride H + 4 floats; registers cannot hold it:
//       H is a run-time size up to 512 and MFMA operands cannot be indexed dynamically). Rows beyond n are read on the clamped last
//       row and never stored.
//     * its four waves split the M actions round-robin (wave v: a = v, v + 4, ...). For one action a wave walks the ceil(N / 16)
//       column tiles, HEAD_TILES = 4 of them per pass over H (N = 51: one pass), with __builtin_amdgcn_mfma_f32_16x16x4f32: the A
//       operand (lane = row lr, k = lq) is one float4 of the LDS tile per 16 contraction columns, the B operand (k = lq, column lr)
//       one float4 of weight row a * N + column straight from memory, so the four tiles' accumulators form four independent MFMA
//       chains on one A load. H % 16 in {4, 8, 12} leaves one to three 4-wide steps on scalar loads. Columns beyond N read the
//       clamped row a * N + N - 1 and count as -inf.
//     * the accumulator layout gives lane (lr, lq) the rows 4 lq .. 4 lq + 3 of column lr, so a row's 16 columns of a tile sit on
//       the 16 lanes of one quarter: bias added, the pass's maximum, sum e and sum z e go through xor butterflies (offsets 8 .. 1:
//       they stay inside the quarter, and every lane ends with the same bits) and fold into the row's running maximum m, the
//       rescaled running s = sum e^(x - m) and t = sum z e^(x - m). expf, not the fast intrinsic. q = t / s.
//     * a NaN logit is dropped by the maximum and turns e, s and q of that (row, action) into NaN; +inf does the same, as torch's
//       softmax. cstr_dqn_act_f32 takes a NaN as the greatest value.
//     * the wave's q values collect in an LDS tile [16][M + 1]; after one barrier the workgroup stores them with consecutive lanes
//       on consecutive columns.
// cstr_c51_loss_f32, two launches behind one entry point (the QR-DQN block's shape):
//   rows kernel, ONE workgroup per batch row (64 .. 256 lanes, whole waves covering max(M, N)), float64 throughout:
//     * lane a < M: the maximum of z_next[b][a][:], then se = sum_i e_i and sz = sum_i z_i e_i (e_i = exp(x_i - max), i ascending);
//       Q'_a = sz / se. The greedy a* is the first maximum of Q', a NaN the greatest and the first one winning, found by
//       cstr_qrdqn.hip's shuffle tree (the order is total, the tree's shape is free);
//     * lane j < N: p_j = exp(z_next[b][a*][j] - max) / se and b_j = clamp((clamp(r + (1 - d) gamma z_j, v_min, v_max) - v_min) / dz,
//       0, N - 1) into LDS;
//     * lane i < N: m_i = sum_j p_j max(0, 1 - |b_j - i|), j ascending over all N (an LDS broadcast per term): the paper's
//       projection as a gather, no atomics, no special case for an integer b_j;
//     * lane i < N reads z[b][a][i] (a from the stored valve pair, DQN's level_of): the maximum, sum of exponentials, sum m and
//       sum m lp through the 64-lane shuffle tree and the wave sums in wave order; lp_i = (x_i - max) - log(sum e),
//       gz = ((e_i / sum e) * (sum m) - m_i) / B;
//     * the row of gz is zero-filled by the whole workgroup, the N entries of the taken action left to their lanes.
//   finish kernel, one 256-lane workgroup: lane t adds the row sums of rows t, t + 256, ... in ascending order, the same tree, then
//     lane 0 writes loss = sum / B.
//   No float atomics and no workgroup that waits for another: a relaunch gives the same bits.
// Nothing here allocates, synchronises or keeps host state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_onpolicy_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int C51_MAX_ATOMS = CSTR_C51_MAX_ATOMS, C51_MAX_H = 512;
constexpr int HEAD_THREADS = 256, HEAD_WAVES = 4, HEAD_ROWS = 16, HEAD_TILES = 4, HEAD_PAD = 4;

struct C51HeadArgs {
    const float *h, *w, *bias;
    float *q;
    int64_t ldh, ldq, n;
    double v_min, dz;
    int M, N, H;
};

// over the 16 lanes of a quarter (the 16 columns of a row's tile); every lane ends with the same bits
__device__ __forceinline__ float quarter_max(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float quarter_sum(float v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(HEAD_THREADS) void c51_head_q_kernel(const C51HeadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float c51_lds[];
    const int H = a.H, N = a.N, M = a.M, ldt = H + HEAD_PAD, ldo = M + 1;
    float *ht = c51_lds;                   // [16][ldt]: the hidden tile
    float *qt = c51_lds + HEAD_ROWS * ldt;  // [16][ldo]: the workgroup's q values
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;

    for (int idx = tid; idx < HEAD_ROWS * H; idx += HEAD_THREADS) {
        const int r = idx / H, k = idx - r * H;
        const int64_t row = row0 + r < a.n ? row0 + r : a.n - 1;
        ht[r * ldt + k] = a.h[row * a.ldh + k];
    }
    __syncthreads();

    const float *hr = ht + lr * ldt;
    const int h16 = H & ~15;
    const float ninf = -__builtin_inff();
    for (int act = wave; act < M; act += HEAD_WAVES) {
        const float *wa = a.w + (int64_t)act * N * H, *ba = a.bias + (int64_t)act * N;
        float m[4], s[4], t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { m[i] = ninf; s[i] = 0.0f; t[i] = 0.0f; }
        for (int c0 = 0; c0 < N; c0 += 16 * HEAD_TILES) {
            const int nt = (N - c0 + 15) >> 4;  // tiles of this pass that hold a column (wave-uniform), HEAD_TILES or fewer at the end
            const float *wr[HEAD_TILES];
            f32x4 acc[HEAD_TILES];
#pragma unroll
            for (int u = 0; u < HEAD_TILES; ++u) {
                const int col = c0 + 16 * u + lr;
                wr[u] = wa + (int64_t)(col < N ? col : N - 1) * H;
                acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            // 16 contraction columns per step, lane quarter lq takes columns 4 lq .. 4 lq + 3 of them as one float4 on both operands
            for (int kb = 0; kb < h16; kb += 16) {
                const float4 av = *reinterpret_cast<const float4 *>(hr + kb + 4 * lq);
#pragma unroll
                for (int u = 0; u < HEAD_TILES; ++u) {
                    if (u < nt) {
                        const float4 bv = *reinterpret_cast<const float4 *>(wr[u] + kb + 4 * lq);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[u], 0, 0, 0);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[u], 0, 0, 0);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[u], 0, 0, 0);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[u], 0, 0, 0);
                    }
                }
            }
            for (int k0 = h16; k0 < H; k0 += 4) {  // H % 16: 4-wide steps
                const float ax = hr[k0 + lq];
#pragma unroll
                for (int u = 0; u < HEAD_TILES; ++u)
                    if (u < nt) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, wr[u][k0 + lq], acc[u], 0, 0, 0);
            }
            // the pass's logits: acc[u][i] is row 4 lq + i, column c0 + 16 u + lr
            float zc[HEAD_TILES];
#pragma unroll
            for (int u = 0; u < HEAD_TILES; ++u) {
                const int col = c0 + 16 * u + lr;
                const bool in = col < N;
                const float bc = in ? ba[col] : 0.0f;
                zc[u] = (float)(a.v_min + (double)col * a.dz);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[u][i] = in ? acc[u][i] + bc : ninf;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float pm = acc[0][i];
#pragma unroll
                for (int u = 1; u < HEAD_TILES; ++u) pm = fmaxf(pm, acc[u][i]);
                const float mn = fmaxf(m[i], quarter_max(pm));
                const float ref = mn == ninf ? 0.0f : mn;                      // a row of -inf so far: e = 0, nothing to subtract
                const float scale = m[i] == ninf ? 0.0f : expf(m[i] - mn);  // s = t = 0 before the first finite logit
                float se = 0.0f, te = 0.0f;
#pragma unroll
                for (int u = 0; u < HEAD_TILES; ++u) {
                    const float e = expf(acc[u][i] - ref);
                    se += e;
                    te += zc[u] * e;
                }
                s[i] = s[i] * scale + quarter_sum(se);
                t[i] = t[i] * scale + quarter_sum(te);
                m[i] = mn;
            }
        }
        if (lr == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) qt[(4 * lq + i) * ldo + act] = t[i] / s[i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < HEAD_ROWS * M; idx += HEAD_THREADS) {
        const int r = idx / M, c = idx - r * M;
        if (row0 + r < a.n) a.q[(row0 + r) * a.ldq + c] = qt[r * ldo + c];
    }
}

struct C51LossArgs {
    const float *z, *z_next, *valve, *rew, *done;
    int64_t ldz, ldn;
    double gamma, v_min, v_max;
    float *gz, *m_out, *logp_out, *row_loss_out;
    int64_t *next_index_out;
    double *ws;
    int M, K, N, batch;
};

// cstr_qrdqn.hip's wave_tree_sum_f64: sum over the workgroup (1 to 4 waves of 64 lanes), shuffle tree with offsets 32, 16, ... 1, then
// the wave sums in wave order. Every lane of the workgroup calls it and gets the result.
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

// the same for the maximum; fmax drops a NaN operand
__device__ __forceinline__ double wave_tree_max_f64(double v, double *sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    double r = sm[0];
    for (int w = 1; w < waves; ++w) r = fmax(r, sm[w]);
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

// numpy.clip: a NaN stays one
__device__ __forceinline__ double clip_f64(const double x, const double lo, const double hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(256) void c51_loss_rows_kernel(const C51LossArgs a)
{
    __shared__ double s_p[C51_MAX_ATOMS], s_b[C51_MAX_ATOMS];
    __shared__ double s_red[4], s_stat[2];
    __shared__ int s_idx[4];
    const int b = blockIdx.x, t = threadIdx.x, M = a.M, N = a.N, K = a.K;
    const float *zn_row = a.z_next + (int64_t)b * a.ldn;
    const float *z_row = a.z + (int64_t)b * a.ldz;
    float *g_row = a.gz + (int64_t)b * a.ldz;
    const double v_min = a.v_min, v_max = a.v_max, dz = (v_max - v_min) / (double)(N - 1);
    const double ninf = -__builtin_inf();

    // the expected value of every action of the next state and their first maximum
    double best = ninf, mx = ninf, se = 0.0;
    int arg = 0x7fffffff;  // a lane without an action loses against every action, whatever its value
    if (t < M) {
        const float *p = zn_row + (int64_t)t * N;
        for (int i = 0; i < N; ++i) mx = fmax(mx, (double)p[i]);
        double sz = 0.0;
        for (int i = 0; i < N; ++i) {
            const double e = exp((double)p[i] - mx);
            se += e;
            sz += (v_min + (double)i * dz) * e;
        }
        best = sz / se;
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
    if (t == a_next) { s_stat[0] = mx; s_stat[1] = se; }
    __syncthreads();

    // its probabilities and the positions of the shifted atoms on the support
    const bool live = t < N;
    if (live) {
        s_p[t] = exp((double)zn_row[(int64_t)a_next * N + t] - s_stat[0]) / s_stat[1];
        const double coef = (1.0 - (double)a.done[b]) * a.gamma;
        const double tz = clip_f64((double)a.rew[b] + coef * (v_min + (double)t * dz), v_min, v_max);
        s_b[t] = clip_f64((tz - v_min) / dz, 0.0, (double)(N - 1));
    }
    if (t == 0 && a.next_index_out) a.next_index_out[b] = (int64_t)a_next;
    const float2 v = *reinterpret_cast<const float2 *>(a.valve + (int64_t)b * 2);
    const int a_cur = level_of(v.x, K) * K + level_of(v.y, K);  // in [0, M) by construction
    // the gradient row: zeros everywhere but at the taken action's N atoms, which their lanes store below
    for (int e = t; e < M * N; e += blockDim.x)
        if (e / N != a_cur) g_row[e] = 0.0f;
    __syncthreads();

    // the projected target: atom i gathers from every shifted atom within one spacing of it
    double mi = 0.0;
    if (live) {
        const double pos = (double)t;
        for (int j = 0; j < N; ++j) {
            const double hat = 1.0 - fabs(s_b[j] - pos);  // one address per wave: an LDS broadcast
            if (!(hat <= 0.0)) mi += s_p[j] * hat;         // a NaN position reaches the sum
        }
    }
    // the log-softmax of the taken action's logits, the row's loss and gradient
    const double x = live ? (double)z_row[(int64_t)a_cur * N + t] : ninf;
    const double xm = x - wave_tree_max_f64(x, s_red);
    const double ex = live ? exp(xm) : 0.0;
    const double sum_e = wave_tree_sum_f64(ex, s_red);
    const double lp = xm - log(sum_e);
    const double sum_m = wave_tree_sum_f64(mi, s_red);
    const double row_loss = -wave_tree_sum_f64(live ? mi * lp : 0.0, s_red);
    if (live) {
        g_row[(int64_t)a_cur * N + t] = (float)(((ex / sum_e) * sum_m - mi) / (double)a.batch);
        if (a.m_out) a.m_out[(int64_t)b * N + t] = (float)mi;
        if (a.logp_out) a.logp_out[(int64_t)b * N + t] = (float)lp;
    }
    if (t == 0) {
        a.ws[b] = row_loss;
        if (a.row_loss_out) a.row_loss_out[b] = (float)row_loss;
    }
}

__global__ __launch_bounds__(256) void c51_loss_finish_kernel(const double *__restrict__ ws, const int batch, float *__restrict__ loss_out,
                                                              float *__restrict__ loss_sum)
{
    __shared__ double s_red[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < batch; b += 256) acc += ws[b];
    const double s = wave_tree_sum_f64(acc, s_red);
    if (threadIdx.x == 0) {
        const float loss = (float)(s / (double)batch);
        if (loss_out) loss_out[0] = loss;
        if (loss_sum) loss_sum[0] += loss;
    }
}

inline bool support_ok(double v_min, double v_max) { return std::isfinite(v_min) && std::isfinite(v_max) && v_max > v_min; }

}  // namespace

extern "C" int cstr_c51_supported(int n_actions, int levels, int n_atoms, int64_t H)
{
    return levels >= 2 && levels <= CSTR_DQN_MAX_LEVELS && n_actions == levels * levels && n_atoms >= 2 && n_atoms <= CSTR_C51_MAX_ATOMS &&
           H > 0 && H % 4 == 0 && H <= C51_MAX_H;
}

extern "C" int cstr_c51_head_q_f32(const float *h, int64_t ldh, const float *w, const float *bias, int64_t n, int n_actions, int levels,
                                   int n_atoms, int64_t H, double v_min, double v_max, float *q, int64_t ldq, cstr_stream_t stream)
{
    if (!h || !w || !bias || !q || n <= 0 || n_actions <= 0 || levels <= 0 || n_atoms <= 0 || H <= 0) return CSTR_E_BADARG;
    if (ldh < H || ldq < n_actions || !support_ok(v_min, v_max)) return CSTR_E_BADARG;
    if (!cstr_c51_supported(n_actions, levels, n_atoms, H) || n > CSTR_PPO_MAX_ROWS) return CSTR_E_UNSUPPORTED;
    if (!aligned4(h) || !aligned16(w) || !aligned4(bias) || !aligned4(q)) return CSTR_E_BADARG;
    const int64_t MN = (int64_t)n_actions * n_atoms;
    {
        const Buf ins[3] = {{h, span(n, ldh, H)}, {w, MN * H}, {bias, MN}};
        const Buf outs[1] = {{q, span(n, ldq, n_actions)}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    C51HeadArgs a;
    a.h = h; a.w = w; a.bias = bias; a.q = q; a.ldh = ldh; a.ldq = ldq; a.n = n;
    a.v_min = v_min; a.dz = (v_max - v_min) / (double)(n_atoms - 1);
    a.M = n_actions; a.N = n_atoms; a.H = (int)H;
    const unsigned grid = (unsigned)((n + HEAD_ROWS - 1) / HEAD_ROWS);
    const size_t lds = sizeof(float) * (size_t)(HEAD_ROWS * ((int)H + HEAD_PAD) + HEAD_ROWS * (n_actions + 1));  // at most 49 KiB
    c51_head_q_kernel<<<grid, HEAD_THREADS, lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

extern "C" int cstr_c51_loss_f32(const float *z, int64_t ldz, const float *z_next, int64_t ldn, const float *valve, const float *reward,
                                 const float *done, double gamma, double v_min, double v_max, int64_t batch, int n_actions, int levels,
                                 int n_atoms, float *gz, float *loss_out, float *loss_sum, float *m_out, float *logp_out,
                                 int64_t *next_index_out, float *row_loss_out, double *ws, cstr_stream_t stream)
{
    if (!z || !z_next || !valve || !reward || !done || !gz || !ws || batch <= 0 || n_actions <= 0 || levels <= 0 || n_atoms <= 0)
        return CSTR_E_BADARG;
    if (!(gamma >= 0.0) || !support_ok(v_min, v_max)) return CSTR_E_BADARG;  // NaN fails too
    if (!cstr_c51_supported(n_actions, levels, n_atoms, 4) || batch > CSTR_MAX_SAMPLE_BATCH) return CSTR_E_UNSUPPORTED;
    const int64_t B = batch, N = n_atoms, MN = (int64_t)n_actions * n_atoms;
    if (ldz < MN || ldn < MN) return CSTR_E_BADARG;
    if (!aligned4(z) || !aligned4(z_next) || !aligned8(valve) || !aligned4(reward) || !aligned4(done) || !aligned4(gz) ||
        (loss_out && !aligned4(loss_out)) || (loss_sum && !aligned4(loss_sum)) || (m_out && !aligned4(m_out)) ||
        (logp_out && !aligned4(logp_out)) || (next_index_out && !aligned8(next_index_out)) || (row_loss_out && !aligned4(row_loss_out)) ||
        !aligned8(ws))
        return CSTR_E_BADARG;
    {
        const Buf ins[5] = {{z, span(B, ldz, MN)}, {z_next, span(B, ldn, MN)}, {valve, 2 * B}, {reward, B}, {done, B}};
        const Buf outs[8] = {{gz, span(B, ldz, MN)}, {loss_out, 1}, {loss_sum, 1}, {m_out, B * N}, {logp_out, B * N},
                             {next_index_out, 2 * B}, {row_loss_out, B}, {ws, 2 * B}};
        if (outputs_overlap(ins, outs)) return CSTR_E_BADARG;
    }
    C51LossArgs a;
    a.z = z; a.z_next = z_next; a.valve = valve; a.rew = reward; a.done = done; a.ldz = ldz; a.ldn = ldn;
    a.gamma = gamma; a.v_min = v_min; a.v_max = v_max;
    a.gz = gz; a.m_out = m_out; a.logp_out = logp_out; a.row_loss_out = row_loss_out; a.next_index_out = next_index_out; a.ws = ws;
    a.M = n_actions; a.K = levels; a.N = n_atoms; a.batch = (int)batch;
    const int widest = n_actions > n_atoms ? n_actions : n_atoms;
    const int lanes = ((widest + 63) / 64) * 64;  // whole waves over max(M, N) <= 256
    c51_loss_rows_kernel<<<(unsigned)batch, lanes, 0, (hipStream_t)stream>>>(a);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    c51_loss_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(ws, (int)batch, loss_out, loss_sum);
    return (int)hipGetLastError();
}
