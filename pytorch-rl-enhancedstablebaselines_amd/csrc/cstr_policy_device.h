// cstr_policy_device.h -- device functions of the rollout policy network shared by its kernels (internal, included by cstr_mlp.hip
// and cstr_eval.hip): the 16-row hidden layer on the f32 matrix cores and its operand loads. Every TU that includes this is built
// with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2;

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;  // core/sac/policies.py:20-22

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

}  // namespace
