// cstr_lstm.hip -- a single-layer LSTM over ragged segments, forward and backward through time, f32 on gfx950 (RecurrentPPO).
//
// Semantics: torch.nn.LSTM (gate order i, f, g, o; weight_ih [4H, K], weight_hh [4H, H], bias_ih, bias_hh) with sb3_contrib's reset
// multiply: before step t of a sequence, h and c are multiplied by 1 - episode_start[t].
//
// Work split. A SEGMENT is a run of consecutive rows (time steps of one env) with its own initial (h, c). A workgroup of four waves owns
// up to 16 segments -- the 16 rows of v_mfma_f32_16x16x4_f32 -- and ALL 4H gate columns, so the state never leaves the workgroup and no
// workgroup waits for another inside the launch. It walks time to the longest length of its group; shorter segments are masked per
// row. Loop bounds and barriers depend on group values only, never on a segment's own length.
//
// Data movement, forward. Wave w owns the hidden tiles j = w, w + 4, ... (16 hidden units each) and, for each, the four gate tiles at
// columns g * H + 16 j. In the MFMA result layout a lane holds D[4 (lane / 16) + i][lane % 16], i = 0..3: the four gates of one
// (segment, hidden unit) pair sit in the same lane, so the activations and the update of c are lane-local and c lives in registers
// for the whole sequence. h is the A operand of the next step: it goes through a double-buffered LDS tile [16][H + 4] (one barrier
// per step), already multiplied by the next step's reset mask -- that masked tile is also what the backward's weight gradient needs,
// so the training mode stores it. x_t (K floats per row) rides in a second small tile and its projection is folded into the step.
// W_hh stays in LDS ([4H][H + 4], read as float4 along k) when it fits beside the tiles; otherwise every step streams it through L2.
//
// Backward. Same ownership, time reversed. The lane that owned (segment, hidden unit) in the forward computes the four gate gradients
// from the stored activations, c_t and c_{t-1}, writes them to dgates [R, 4H] and into an LDS tile; dh_carry = dgates W_hh runs on
// MFMA in two halves of 2H contraction columns each ([i | f], then [g | o]: the tile stays under 64 KB at H = 256), with W_hh
// transposed in LDS ([H][4H + 4]) or streamed. Both carries are multiplied by 1 - episode_start[t] before they reach step t - 1.
// dW_hh, dW_ih and db are cstr_linear_bwd_weight_f32 on dgates against the stored masked h_{t-1} and x: no kernel of their own.
//
// No float atomics anywhere: every output element has one writer and a fixed summation order, so a repeated launch is bit-identical.
#include "cstr_device.h"

namespace {

constexpr int LSTM_SEGS = 16;        // segments per workgroup = rows of the MFMA tile
constexpr int LSTM_THREADS = 256;    // four waves
constexpr int LSTM_TILES = 4;        // hidden tiles per wave at H = CSTR_LSTM_MAX_HIDDEN
constexpr int64_t LSTM_LDS_CAP = 160 * 1024;
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LstmFwdArgs {
    const float *x, *es, *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0;
    const int32_t *seg;
    float *out, *hn, *cn, *gates, *cseq, *hprev;
    int n_seg, K, Kp, H;
};

struct LstmBwdArgs {
    const float *dout, *gates, *cseq, *c0, *es, *w_hh;
    const int32_t *seg;
    float *dgates, *dh0, *dc0;
    int n_seg, H;
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// the lane's four segments (rows 4 (lane / 16) + i of the group) and the group's longest length (the same value in every lane)
__device__ __forceinline__ int load_segments(const int32_t *seg, int n_seg, int seg0, int lq, int (&first)[4], int (&len)[4], int (&init)[4])
{
    int maxlen = 0;
    for (int s = 0; s < LSTM_SEGS; ++s) {
        const int l = seg0 + s < n_seg ? seg[3 * (seg0 + s) + 1] : 0;
        maxlen = l > maxlen ? l : maxlen;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sidx = seg0 + 4 * lq + i;
        const bool ok = sidx < n_seg;
        first[i] = ok ? seg[3 * sidx] : 0;
        len[i] = ok ? seg[3 * sidx + 1] : 0;
        init[i] = ok ? seg[3 * sidx + 2] : 0;
    }
    return maxlen;
}

template <bool RESIDENT, bool TRAIN>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_fwd_kernel(const LstmFwdArgs a)
{
    extern __shared__ float4 lstm_lds4[];
    float *lds = reinterpret_cast<float *>(lstm_lds4);
    const int H = a.H, ldh = H + 4, K = a.K, Kp = a.Kp, ldx = Kp + 4, nt = H >> 4;
    float *hbuf = lds;                      // [2][16][ldh]
    float *xbuf = hbuf + 2 * LSTM_SEGS * ldh;  // [2][16][ldx]
    float *wl = xbuf + 2 * LSTM_SEGS * ldx;    // RESIDENT: [4H][ldh]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int seg0 = blockIdx.x * LSTM_SEGS;
    int first[4], len[4], init[4];
    const int maxlen = load_segments(a.seg, a.n_seg, seg0, lq, first, len, init);

    if (RESIDENT) {
        const int h4 = H >> 2;
        for (int idx = tid; idx < 4 * H * h4; idx += LSTM_THREADS) {
            const int row = idx / h4, c4 = idx - row * h4;
            *reinterpret_cast<float4 *>(wl + row * ldh + 4 * c4) = *reinterpret_cast<const float4 *>(a.w_hh + (int64_t)row * H + 4 * c4);
        }
    }
    // step 0's operands: the initial h times the first row's reset mask, and x_0
    for (int idx = tid; idx < LSTM_SEGS * H; idx += LSTM_THREADS) {
        const int s = idx / H, col = idx - s * H, sidx = seg0 + s;
        float v = 0.0f;
        if (sidx < a.n_seg) {
            const int f = a.seg[3 * sidx], in = a.seg[3 * sidx + 2];
            v = a.h0[(int64_t)in * H + col] * (1.0f - a.es[f]);
            if (TRAIN) a.hprev[(int64_t)f * H + col] = v;
        }
        hbuf[s * ldh + col] = v;
    }
    for (int idx = tid; idx < LSTM_SEGS * Kp; idx += LSTM_THREADS) {
        const int s = idx / Kp, k = idx - s * Kp, sidx = seg0 + s;
        xbuf[s * ldx + k] = (sidx < a.n_seg && k < K) ? a.x[(int64_t)a.seg[3 * sidx] * K + k] : 0.0f;
    }
    float c_reg[LSTM_TILES][4], bias[LSTM_TILES][4];
#pragma unroll
    for (int u = 0; u < LSTM_TILES; ++u) {
        const int j = wave + 4 * u, col = 16 * j + lr;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            c_reg[u][i] = (j < nt && len[i] > 0) ? a.c0[(int64_t)init[i] * H + col] * (1.0f - a.es[first[i]]) : 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) bias[u][g] = j < nt ? a.b_ih[g * H + col] + a.b_hh[g * H + col] : 0.0f;
    }
    __syncthreads();

    for (int t = 0; t < maxlen; ++t) {
        const int p = t & 1;
        const float *hb = hbuf + p * LSTM_SEGS * ldh, *xb = xbuf + p * LSTM_SEGS * ldx;
        float *hnext = hbuf + (1 - p) * LSTM_SEGS * ldh, *xnext = xbuf + (1 - p) * LSTM_SEGS * ldx;
        f32x4 acc[LSTM_TILES][4];
#pragma unroll
        for (int u = 0; u < LSTM_TILES; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[u][g] = f32x4{bias[u][g], bias[u][g], bias[u][g], bias[u][g]};
        // gates += h W_hh^T: 16 contraction columns per pass, lane quarter lq takes columns 4 lq .. 4 lq + 3 of them as one float4
        for (int kb = 0; kb < H; kb += 16) {
            const float4 av = *reinterpret_cast<const float4 *>(hb + lr * ldh + kb + 4 * lq);
#pragma unroll
            for (int u = 0; u < LSTM_TILES; ++u) {
                const int j = wave + 4 * u;
                if (j < nt) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int wrow = g * H + 16 * j + lr;
                        const float4 bv = RESIDENT ? *reinterpret_cast<const float4 *>(wl + wrow * ldh + kb + 4 * lq)
                                                   : *reinterpret_cast<const float4 *>(a.w_hh + (int64_t)wrow * H + kb + 4 * lq);
                        acc[u][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[u][g], 0, 0, 0);
                        acc[u][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[u][g], 0, 0, 0);
                        acc[u][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[u][g], 0, 0, 0);
                        acc[u][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[u][g], 0, 0, 0);
                    }
                }
            }
        }
        // gates += x_t W_ih^T (the x tile is zero beyond K and beyond a segment's end)
        for (int k0 = 0; k0 < Kp; k0 += 4) {
            const float ax = xb[lr * ldx + k0 + lq];
            const bool kin = k0 + lq < K;
#pragma unroll
            for (int u = 0; u < LSTM_TILES; ++u) {
                const int j = wave + 4 * u;
                if (j < nt) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float bx = kin ? a.w_ih[(int64_t)(g * H + 16 * j + lr) * K + k0 + lq] : 0.0f;
                        acc[u][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, bx, acc[u][g], 0, 0, 0);
                    }
                }
            }
        }
        float mnext[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) mnext[i] = t + 1 < len[i] ? 1.0f - a.es[first[i] + t + 1] : 0.0f;
#pragma unroll
        for (int u = 0; u < LSTM_TILES; ++u) {
            const int j = wave + 4 * u, col = 16 * j + lr;
            if (j < nt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int s = 4 * lq + i;
                    float hm = 0.0f;
                    if (t < len[i]) {
                        const float gi = sigmoidf_(acc[u][0][i]), gf = sigmoidf_(acc[u][1][i]), gg = tanhf(acc[u][2][i]), go = sigmoidf_(acc[u][3][i]);
                        const float c = gf * c_reg[u][i] + gi * gg;
                        const float h = go * tanhf(c);
                        const int64_t r = (int64_t)first[i] + t;
                        if (a.out) a.out[r * H + col] = h;
                        if (TRAIN) {
                            float *gr = a.gates + r * 4 * H + col;
                            gr[0] = gi; gr[H] = gf; gr[2 * H] = gg; gr[3 * H] = go;
                            a.cseq[r * H + col] = c;
                        }
                        if (t + 1 == len[i]) {
                            a.hn[(int64_t)(seg0 + s) * H + col] = h;
                            a.cn[(int64_t)(seg0 + s) * H + col] = c;
                        } else {
                            hm = h * mnext[i];
                            if (TRAIN) a.hprev[(r + 1) * H + col] = hm;
                        }
                        c_reg[u][i] = c * mnext[i];
                    }
                    hnext[s * ldh + col] = hm;
                }
            }
        }
        for (int idx = tid; idx < LSTM_SEGS * Kp; idx += LSTM_THREADS) {
            const int s = idx / Kp, k = idx - s * Kp, sidx = seg0 + s;
            float v = 0.0f;
            if (sidx < a.n_seg && k < K && t + 1 < a.seg[3 * sidx + 1]) v = a.x[((int64_t)a.seg[3 * sidx] + t + 1) * K + k];
            xnext[s * ldx + k] = v;
        }
        __syncthreads();
    }
}

template <bool RESIDENT>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_bwd_kernel(const LstmBwdArgs a)
{
    extern __shared__ float4 lstm_lds4[];
    float *lds = reinterpret_cast<float *>(lstm_lds4);
    const int H = a.H, H2 = 2 * H, ldg = H2 + 4, ldt = 4 * H + 4, nt = H >> 4;
    float *dgl = lds;                   // [16][ldg]: one half ([i | f] or [g | o]) of the step's gate gradients
    float *wt = dgl + LSTM_SEGS * ldg;  // RESIDENT: W_hh transposed, [H][ldt]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int seg0 = blockIdx.x * LSTM_SEGS;
    int first[4], len[4], init[4];
    const int maxlen = load_segments(a.seg, a.n_seg, seg0, lq, first, len, init);

    if (RESIDENT) {
        for (int idx = tid; idx < 4 * H * H; idx += LSTM_THREADS) {
            const int kk = idx / H, n = idx - kk * H;
            wt[n * ldt + kk] = a.w_hh[idx];
        }
    }
    float dh_c[LSTM_TILES][4], dc_c[LSTM_TILES][4];
#pragma unroll
    for (int u = 0; u < LSTM_TILES; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) dh_c[u][i] = dc_c[u][i] = 0.0f;
    __syncthreads();

    for (int t = maxlen - 1; t >= 0; --t) {
        float da[LSTM_TILES][4][4];  // [tile][gate][row]
        float mask[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) mask[i] = t < len[i] ? 1.0f - a.es[first[i] + t] : 0.0f;
#pragma unroll
        for (int u = 0; u < LSTM_TILES; ++u) {
            const int j = wave + 4 * u, col = 16 * j + lr;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
                if (j < nt && t < len[i]) {
                    const int64_t r = (int64_t)first[i] + t;
                    const float *gr = a.gates + r * 4 * H + col;
                    const float gi = gr[0], gf = gr[H], gg = gr[2 * H], go = gr[3 * H];
                    const float c = a.cseq[r * H + col];
                    const float cprev = (t > 0 ? a.cseq[(r - 1) * H + col] : a.c0[(int64_t)init[i] * H + col]) * mask[i];
                    const float dh = a.dout[r * H + col] + dh_c[u][i];
                    const float tc = tanhf(c);
                    const float dc = dc_c[u][i] + dh * go * (1.0f - tc * tc);
                    d0 = dc * gg * (gi * (1.0f - gi));
                    d1 = dc * cprev * (gf * (1.0f - gf));
                    d2 = dc * gi * (1.0f - gg * gg);
                    d3 = dh * tc * (go * (1.0f - go));
                    float *dg = a.dgates + r * 4 * H + col;
                    dg[0] = d0; dg[H] = d1; dg[2 * H] = d2; dg[3 * H] = d3;
                    dc_c[u][i] = dc * gf * mask[i];
                }
                da[u][0][i] = d0; da[u][1][i] = d1; da[u][2][i] = d2; da[u][3][i] = d3;
            }
        }
        f32x4 acc[LSTM_TILES];
#pragma unroll
        for (int u = 0; u < LSTM_TILES; ++u) acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // dh_carry = dgates W_hh over the 4H gate columns, two halves through the LDS tile (rows past a segment's end hold zeros)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int u = 0; u < LSTM_TILES; ++u) {
                const int j = wave + 4 * u, col = 16 * j + lr;
                if (j < nt) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dgl[(4 * lq + i) * ldg + col] = da[u][2 * half][i];
                        dgl[(4 * lq + i) * ldg + H + col] = da[u][2 * half + 1][i];
                    }
                }
            }
            __syncthreads();
            for (int kb = 0; kb < H2; kb += 16) {
                const float4 av = *reinterpret_cast<const float4 *>(dgl + lr * ldg + kb + 4 * lq);
                const int kk = half * H2 + kb + 4 * lq;  // the gate column (row of W_hh) of av.x
#pragma unroll
                for (int u = 0; u < LSTM_TILES; ++u) {
                    const int j = wave + 4 * u, n = 16 * j + lr;
                    if (j < nt) {
                        float4 bv;
                        if (RESIDENT) {
                            bv = *reinterpret_cast<const float4 *>(wt + n * ldt + kk);
                        } else {
                            const float *wp = a.w_hh + (int64_t)kk * H + n;
                            bv = make_float4(wp[0], wp[H], wp[2 * H], wp[3 * H]);
                        }
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[u], 0, 0, 0);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[u], 0, 0, 0);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[u], 0, 0, 0);
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[u], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < LSTM_TILES; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dh_c[u][i] = acc[u][i] * mask[i];
        }
    }
#pragma unroll
    for (int u = 0; u < LSTM_TILES; ++u) {
        const int j = wave + 4 * u, col = 16 * j + lr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (j < nt && len[i] > 0) {
                a.dh0[(int64_t)(seg0 + 4 * lq + i) * H + col] = dh_c[u][i];
                a.dc0[(int64_t)(seg0 + 4 * lq + i) * H + col] = dc_c[u][i];
            }
        }
    }
}

inline bool al(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0; }

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

// every segment inside [0, n_rows), in ascending order without a shared row (each row has one writer), its state row inside the state buffer
inline bool segments_ok(const int32_t *seg, int64_t n_seg, int64_t n_rows, int64_t n_state_rows)
{
    int64_t next = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        const int64_t first = seg[3 * s], len = seg[3 * s + 1], init = seg[3 * s + 2];
        if (first < next || len < 1 || first + len > n_rows || init < 0 || init >= n_state_rows) return false;
        next = first + len;
    }
    return true;
}

inline int64_t fwd_lds_bytes(int64_t k, int64_t h, bool resident)
{
    const int64_t kp = (k + 3) / 4 * 4;
    return 4 * (2 * LSTM_SEGS * (h + 4) + 2 * LSTM_SEGS * (kp + 4) + (resident ? 4 * h * (h + 4) : 0));
}

inline int64_t bwd_lds_bytes(int64_t h, bool resident) { return 4 * (LSTM_SEGS * (2 * h + 4) + (resident ? h * (4 * h + 4) : 0)); }

// the LDS a workgroup of the current device may ask for, at most the 160 KB of a gfx950 compute unit
int64_t lds_limit()
{
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
        v = 64 * 1024;
    return v < LSTM_LDS_CAP ? v : LSTM_LDS_CAP;
}

template <typename Kern>
void allow_lds(Kern kern, int64_t bytes)
{
    if (bytes > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

inline int shape_rc(int64_t k, int64_t h)
{
    if (k < 1 || h < 1) return CSTR_E_BADARG;
    if (h % 16 != 0 || h > CSTR_LSTM_MAX_HIDDEN || k > CSTR_LSTM_MAX_INPUT) return CSTR_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int cstr_lstm_supported(int64_t k, int64_t h) { return shape_rc(k, h) == 0; }

extern "C" int cstr_lstm_resident(int64_t k, int64_t h, int backward)
{
    if (shape_rc(k, h) != 0) return 0;
    return (backward ? bwd_lds_bytes(h, true) : fwd_lds_bytes(k, h, true)) <= LSTM_LDS_CAP;
}

extern "C" int cstr_lstm_seq_fwd_f32(const float *x, const float *episode_start, int64_t n_rows, const float *w_ih, const float *w_hh,
                                     const float *b_ih, const float *b_hh, const float *state_h, const float *state_c, int64_t n_state_rows,
                                     const int32_t *seg_host, const int32_t *seg_dev, int64_t n_seg, float *out, float *hn, float *cn,
                                     float *gates, float *c_seq, float *h_prev, int64_t k, int64_t h, int force_stream, cstr_stream_t stream)
{
    if (!x || !episode_start || !w_ih || !w_hh || !b_ih || !b_hh || !state_h || !state_c || !seg_host || !seg_dev || !hn || !cn)
        return CSTR_E_BADARG;
    if (n_rows <= 0 || n_state_rows <= 0 || n_seg <= 0) return CSTR_E_BADARG;
    if (int rc = shape_rc(k, h)) return rc;
    if (n_rows >= (1ll << 31) || n_state_rows >= (1ll << 31) || n_seg >= (1ll << 31) - LSTM_SEGS) return CSTR_E_UNSUPPORTED;
    const bool train = gates || c_seq || h_prev;
    if (train && (!gates || !c_seq || !h_prev || !out)) return CSTR_E_BADARG;
    const int64_t rows_h = 4 * n_rows * h, segs_h = 4 * n_seg * h, st = 4 * n_state_rows * h;
    const void *ins[9] = {x, episode_start, w_ih, w_hh, b_ih, b_hh, state_h, state_c, seg_dev};
    const int64_t in_b[9] = {4 * n_rows * k, 4 * n_rows, 16 * h * k, 16 * h * h, 16 * h, 16 * h, st, st, 12 * n_seg};
    const void *outs[6] = {out, hn, cn, gates, c_seq, h_prev};
    const int64_t out_b[6] = {rows_h, segs_h, segs_h, 4 * rows_h, rows_h, rows_h};
    for (int i = 0; i < 9; ++i)
        if (!al(ins[i], 4)) return CSTR_E_BADARG;
    for (int i = 0; i < 6; ++i)
        if (!al(outs[i], 4)) return CSTR_E_BADARG;
    if (!al(w_hh, 16)) return CSTR_E_BADARG;
    if (any_overlap(ins, in_b, 9, outs, out_b, 6)) return CSTR_E_BADARG;
    if (!segments_ok(seg_host, n_seg, n_rows, n_state_rows)) return CSTR_E_BADARG;

    const int64_t limit = lds_limit();
    const bool resident = !force_stream && fwd_lds_bytes(k, h, true) <= limit;
    const int64_t lds = fwd_lds_bytes(k, h, resident);
    if (lds > limit) return CSTR_E_UNSUPPORTED;
    LstmFwdArgs a;
    a.x = x; a.es = episode_start; a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh; a.h0 = state_h; a.c0 = state_c; a.seg = seg_dev;
    a.out = out; a.hn = hn; a.cn = cn; a.gates = gates; a.cseq = c_seq; a.hprev = h_prev;
    a.n_seg = (int)n_seg; a.K = (int)k; a.Kp = (int)((k + 3) / 4 * 4); a.H = (int)h;
    const dim3 grid((unsigned)((n_seg + LSTM_SEGS - 1) / LSTM_SEGS));
    hipStream_t s = (hipStream_t)stream;
    if (resident && train) { allow_lds(lstm_seq_fwd_kernel<true, true>, lds); lstm_seq_fwd_kernel<true, true><<<grid, LSTM_THREADS, lds, s>>>(a); }
    else if (resident) { allow_lds(lstm_seq_fwd_kernel<true, false>, lds); lstm_seq_fwd_kernel<true, false><<<grid, LSTM_THREADS, lds, s>>>(a); }
    else if (train) { allow_lds(lstm_seq_fwd_kernel<false, true>, lds); lstm_seq_fwd_kernel<false, true><<<grid, LSTM_THREADS, lds, s>>>(a); }
    else { allow_lds(lstm_seq_fwd_kernel<false, false>, lds); lstm_seq_fwd_kernel<false, false><<<grid, LSTM_THREADS, lds, s>>>(a); }
    return (int)hipGetLastError();
}

extern "C" int cstr_lstm_seq_bwd_f32(const float *dout, const float *gates, const float *c_seq, const float *state_c, int64_t n_state_rows,
                                     const float *episode_start, int64_t n_rows, const float *w_hh, const int32_t *seg_host,
                                     const int32_t *seg_dev, int64_t n_seg, float *dgates, float *dh0, float *dc0, int64_t h, int force_stream,
                                     cstr_stream_t stream)
{
    if (!dout || !gates || !c_seq || !state_c || !episode_start || !w_hh || !seg_host || !seg_dev || !dgates || !dh0 || !dc0) return CSTR_E_BADARG;
    if (n_rows <= 0 || n_state_rows <= 0 || n_seg <= 0) return CSTR_E_BADARG;
    if (int rc = shape_rc(1, h)) return rc;
    if (n_rows >= (1ll << 31) || n_state_rows >= (1ll << 31) || n_seg >= (1ll << 31) - LSTM_SEGS) return CSTR_E_UNSUPPORTED;
    const int64_t rows_h = 4 * n_rows * h, segs_h = 4 * n_seg * h;
    const void *ins[7] = {dout, gates, c_seq, state_c, episode_start, w_hh, seg_dev};
    const int64_t in_b[7] = {rows_h, 4 * rows_h, rows_h, 4 * n_state_rows * h, 4 * n_rows, 16 * h * h, 12 * n_seg};
    const void *outs[3] = {dgates, dh0, dc0};
    const int64_t out_b[3] = {4 * rows_h, segs_h, segs_h};
    for (int i = 0; i < 7; ++i)
        if (!al(ins[i], 4)) return CSTR_E_BADARG;
    for (int i = 0; i < 3; ++i)
        if (!al(outs[i], 4)) return CSTR_E_BADARG;
    if (any_overlap(ins, in_b, 7, outs, out_b, 3)) return CSTR_E_BADARG;
    if (!segments_ok(seg_host, n_seg, n_rows, n_state_rows)) return CSTR_E_BADARG;

    const int64_t limit = lds_limit();
    const bool resident = !force_stream && bwd_lds_bytes(h, true) <= limit;
    const int64_t lds = bwd_lds_bytes(h, resident);
    if (lds > limit) return CSTR_E_UNSUPPORTED;
    LstmBwdArgs a;
    a.dout = dout; a.gates = gates; a.cseq = c_seq; a.c0 = state_c; a.es = episode_start; a.w_hh = w_hh; a.seg = seg_dev;
    a.dgates = dgates; a.dh0 = dh0; a.dc0 = dc0; a.n_seg = (int)n_seg; a.H = (int)h;
    const dim3 grid((unsigned)((n_seg + LSTM_SEGS - 1) / LSTM_SEGS));
    hipStream_t s = (hipStream_t)stream;
    if (resident) { allow_lds(lstm_seq_bwd_kernel<true>, lds); lstm_seq_bwd_kernel<true><<<grid, LSTM_THREADS, lds, s>>>(a); }
    else { allow_lds(lstm_seq_bwd_kernel<false>, lds); lstm_seq_bwd_kernel<false><<<grid, LSTM_THREADS, lds, s>>>(a); }
    return (int)hipGetLastError();
}
