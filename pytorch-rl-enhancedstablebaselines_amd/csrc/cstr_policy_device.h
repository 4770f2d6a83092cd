// cstr_policy_device.h -- device functions of the rollout policy network shared by its kernels (internal, included by cstr_mlp.hip
// and cstr_eval.hip): the 16-row hidden layer on the f32 matrix cores and its operand loads, the two head forms of
// cstr_policy_rows_fwd_f32 (shuffle tree, split-K tile) and the host-side choice between that launch's two kernels. Every TU that
// includes this is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_gaussian_device.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

template <bool VEC>
__device__ __forceinline__ float4 load_k4(const float *__restrict__ row, const int k, const int K, const bool valid)
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!valid || k >= K) return v;
    if (VEC) return *reinterpret_cast<const float4 *>(row + k);  // K % 4 == 0 and 16-byte aligned rows
    v.x = row[k];
    if (k + 1 < K) v.y = row[k + 1];
    if (k + 2 < K) v.z = row[k + 2];
    if (k + 3 < K) v.w = row[k + 3];
    return v;
}

// The same values from an UNCONDITIONAL 16-byte load at a clamped address (VEC: K % 4 == 0, K >= 4), zeroed afterwards: hipcc
// scalarises a float4 load under a condition into four branchy dword loads.
template <bool VEC>
__device__ __forceinline__ float4 load_k4_clamped(const float *__restrict__ row, const int k, const int K, const bool valid)
{
    if (!VEC) return load_k4<false>(row, k, K, valid);
    float4 v = *reinterpret_cast<const float4 *>(row + min(k, K - 4));
    const bool ok = valid && k < K;
    v.x = ok ? v.x : 0.0f; v.y = ok ? v.y : 0.0f; v.z = ok ? v.z : 0.0f; v.w = ok ? v.w : 0.0f;
    return v;
}

constexpr int POLICY_ROWS = 16, POLICY_WAVES = 8;

// One hidden layer for the workgroup's 16 rows: out[16][N] (LDS, row stride so) = act(in[16][K] W^T + b). The waves take the
// 16-column tiles round robin, TWO per pass: every lane issues ALL of its loads for both tiles (up to 256 k values each) at
// once (A = input rows, shared by the two tiles: global memory for the first layer, LDS after it; B = weight rows from L2), so
// a layer of up to 16 x POLICY_WAVES columns costs one memory round trip.
template <int ACT, bool A_GLOBAL, bool VEC, bool SWZ = false, int UNROLL = 16>
__device__ __forceinline__ void policy_layer(const float *__restrict__ in, const int64_t in_stride, const bool in_row_ok, const int K,
                                             const float *__restrict__ w, const float *__restrict__ bias, const int N,
                                             float *__restrict__ out, const int so, const int wave = threadIdx.x >> 6,
                                             const int n_waves = POLICY_WAVES)
{
    const int lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
    const int tiles = (N + 15) >> 4;
    const float *ar = in + r * in_stride;
    const float4 *wsw = reinterpret_cast<const float4 *>(w);
    const int kc = (K + 15) >> 4;
    for (int t = wave; t < tiles; t += 2 * n_waves) {
        const int n0 = t * 16, n1 = n0 + 16 * n_waves;
        const bool ok0 = n0 + r < N, ok1 = n1 + r < N;
        const bool second = t + n_waves < tiles;  // wave-uniform
        const float *wr0 = w + (int64_t)(n0 + r) * K, *wr1 = w + (int64_t)(n1 + r) * K;
        f32x4 c00 = {0.0f, 0.0f, 0.0f, 0.0f}, c01 = c00, c10 = c00, c11 = c00;
        for (int c0 = 0; c0 < K; c0 += 16 * UNROLL) {
            float4 av[UNROLL], b0[UNROLL], b1[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int k = c0 + 16 * u + 4 * h;
                // SWZ: `w` is the tile-major copy [tile][k chunk][lane] of float4 (cstr_policy_swizzle_f32): a wave's load
                // instruction reads 1 KB of consecutive bytes instead of sixteen 64-byte row pieces (7.2 -> ~2 us per 256 KB)
                b0[u] = SWZ ? (k < K ? wsw[((int64_t)t * kc + (c0 >> 4) + u) * 64 + lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f))
                            : load_k4<VEC>(wr0, k, K, ok0);
                av[u] = A_GLOBAL ? load_k4<VEC>(ar, k, K, in_row_ok) : load_k4<true>(ar, k, K, true);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                b1[u] = SWZ ? ((second && c0 + 16 * u + 4 * h < K) ? wsw[((int64_t)(t + n_waves) * kc + (c0 >> 4) + u) * 64 + lane]
                                                                    : make_float4(0.0f, 0.0f, 0.0f, 0.0f))
                            : load_k4<VEC>(wr1, c0 + 16 * u + 4 * h, K, ok1 && second);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (c0 + 16 * u >= K) break;  // wave-uniform: no matrix-core passes on all-zero chunks (K = 4: one chunk)
                c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].x, b0[u].x, c00, 0, 0, 0);
                c01 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].y, b0[u].y, c01, 0, 0, 0);
                c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].z, b0[u].z, c00, 0, 0, 0);
                c01 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].w, b0[u].w, c01, 0, 0, 0);
            }
            if (second) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (c0 + 16 * u >= K) break;
                    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].x, b1[u].x, c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].y, b1[u].y, c11, 0, 0, 0);
                    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].z, b1[u].z, c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].w, b1[u].w, c11, 0, 0, 0);
                }
            }
        }
        // column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = (half ? n1 : n0) + r;
            if (half ? (ok1 && second) : ok0) {
                const f32x4 acc = half ? c10 + c11 : c00 + c01;
                const float bb = bias[col];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = acc[e] + bb;
                    if (ACT == ACT_RELU) v = fmaxf(v, 0.0f);
                    if (ACT == ACT_TANH) v = tanhf(v);
                    out[(4 * h + e) * so + col] = v;
                }
            }
        }
    }
}

// ---- the head (n_out <= 8 outputs per row) in the two summation orders of cstr_policy_rows_fwd_f32 ----------------------------------
// Both leave (or read) the head outputs as an image [16 rows][8 slots] in LDS.
static_assert(2 * CSTR_MAX_HEAD_ACT == 8, "the head images are 8 slots wide");

// Shuffle-tree form, the dots: RPW rows per wave (row q at row0 + q * row_step, LDS or global memory, 16-byte aligned), per-lane partial
// dots over the row's K values against the n_out rows of w3 [n_out][K], then a 64-lane xor tree: every lane ends with the sums in p.
template <int RPW>
__device__ __forceinline__ void head_tree_dots(const float *row0, const int row_step, const int K, const float *w3,
                                               const int n_out, const int lane, float (&p)[RPW][2 * CSTR_MAX_HEAD_ACT])
{
#pragma unroll
    for (int q = 0; q < RPW; ++q)
#pragma unroll
        for (int j = 0; j < 2 * CSTR_MAX_HEAD_ACT; ++j) p[q][j] = 0.0f;
    for (int c = lane * 4; c < K; c += 256) {
        float4 hv[RPW];
#pragma unroll
        for (int q = 0; q < RPW; ++q) hv[q] = *reinterpret_cast<const float4 *>(row0 + q * row_step + c);
#pragma unroll
        for (int j = 0; j < 2 * CSTR_MAX_HEAD_ACT; ++j) {
            if (j >= n_out) break;
            const float4 wv = *reinterpret_cast<const float4 *>(w3 + (int64_t)j * K + c);
#pragma unroll
            for (int q = 0; q < RPW; ++q) p[q][j] += (hv[q].x * wv.x + hv[q].y * wv.y) + (hv[q].z * wv.z + hv[q].w * wv.w);
        }
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
#pragma unroll
        for (int j = 0; j < 2 * CSTR_MAX_HEAD_ACT; ++j) {
            if (j >= n_out) break;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) p[q][j] += __shfl_xor(p[q][j], o, 64);
        }
    }
}

// Shuffle-tree head of the workgroup's 16 rows of h2s (LDS, row stride S2): wave w takes rows w, w + 8, ...; ps[row][slot] = dot + b3
template <int RPW>
__device__ __forceinline__ void policy_head_tree(const float *h2s, const int S2, const int H2, const float *w3,
                                                 const float *b3, const int n_out, float *ps, const int wave, const int lane)
{
    float p[RPW][2 * CSTR_MAX_HEAD_ACT];
    head_tree_dots<RPW>(h2s + wave * S2, POLICY_WAVES * S2, H2, w3, n_out, lane, p);
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
#pragma unroll
        for (int j = 0; j < 2 * CSTR_MAX_HEAD_ACT; ++j) {
            if (j >= n_out) break;
            if (lane == 0) ps[(wave + q * POLICY_WAVES) * 8 + j] = p[q][j] + b3[j];
        }
    }
}

// Split-K form: ONE 16 x 16 tile (rows x outputs, outputs >= n_out are zero columns), K split over the waves: wave w takes the k chunks
// w, w + 8, ...; the partial tiles meet in LDS (part [8 waves][16 rows][8]) and are added in wave order.
// One k chunk: hr = this lane's four h2 values of the chunk (LDS), wv = its four w3 values (zeros for r >= n_out). The LOOP over the
// chunks stays with its kernel: the pipelined kernel holds its w3 quads in registers, requested before layer 1, and walks them fully
// unrolled; the evaluation kernel, which runs the network once per vec-step, loads them in the loop.
__device__ __forceinline__ void split_k_head_chunk(const float *hr, const float4 wv, f32x4 &p0, f32x4 &p1)
{
    const float4 av = *reinterpret_cast<const float4 *>(hr);
    p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv.x, p0, 0, 0, 0);
    p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv.y, p1, 0, 0, 0);
    p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv.z, p0, 0, 0, 0);
    p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv.w, p1, 0, 0, 0);
}

// the wave's partial tile p (column = r, row = 4 * h + register) into its slice of part. The lane's coordinates are derived HERE, not
// passed in: handed the pipelined kernel's own `wave`, `r`, `h`, two rollout instantiations came out with a vmcnt(0) behind their first
// ring requests (profiles/actor_head_shared_ab.txt)
__device__ __forceinline__ void split_k_head_store(float *part, const f32x4 p)
{
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, h = (threadIdx.x & 63) >> 4;
    if (r < 8) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(wave * POLICY_ROWS + 4 * h + e) * 8 + r] = p[e];
    }
}

// (behind a workgroup barrier) head output `slot` of row `row`: the partial tiles in wave order, then the bias
__device__ __forceinline__ float split_k_head_out(const float *part, const int row, const int slot, const float bias)
{
    float sum = 0.0f;
#pragma unroll
    for (int w = 0; w < POLICY_WAVES; ++w) sum += part[(w * POLICY_ROWS + row) * 8 + slot];
    return sum + bias;
}

// ---- which kernel cstr_policy_rows_fwd_f32 runs (host) -------------------------------------------------------------------------------
constexpr int V2_MAX_WIDTH = 512;  // widths up to which the pipelined kernel is instantiated

// dynamic LDS of the pipelined kernel: h1 | h2 images (k padded to 16, + 4 floats per row), part, then eps, 2 x term, cos | sin [16][8] each
static inline size_t policy_v2_lds(const cstr_policy_mlp_t &n)
{
    const int kc1 = (n.h1 + 15) / 16, kc2 = (n.h2 + 15) / 16;
    return (size_t)(POLICY_ROWS * (16 * kc1 + 4 + 16 * kc2 + 4) + POLICY_WAVES * POLICY_ROWS * 8 + 4 * POLICY_ROWS * 8) * sizeof(float);
}

// the pipelined kernel can run this network: tile-major W2 given, widths and LDS inside its instantiations (cstr_rollout_step_f32 needs it)
static inline bool policy_v2_fits(const cstr_policy_mlp_t &n)
{
    return n.w2_swizzled && n.h1 <= V2_MAX_WIDTH && n.h2 <= V2_MAX_WIDTH && policy_v2_lds(n) <= 64 * 1024;
}

// cstr_policy_rows_fwd_f32 runs its pipelined kernel, i.e. the split-K head, for this network (else the first kernel and its shuffle-tree
// head). The evaluation launches ask the same question and run the same head. CSTR_POLICY_V1: development A/B knob (tools/policy_ab.py),
// read once per translation unit.
static inline bool policy_runs_split_k_head(const cstr_policy_mlp_t &n)
{
    static const bool force_v1 = getenv("CSTR_POLICY_V1") != nullptr;
    return policy_v2_fits(n) && !force_v1;
}

}  // namespace
