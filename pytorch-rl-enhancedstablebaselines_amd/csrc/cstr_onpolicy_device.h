// cstr_onpolicy_device.h -- what the on-policy kernels share (cstr_ppo.hip, cstr_a2c.hip, cstr_dqn.hip, cstr_categorical.hip; internal, not part of the ABI): row loads
// and stores, the diagonal Gaussian's log-prob, the discrete face's valve values, the fixed-order f64 batch reduction (LDS tree per workgroup, published partials,
// last-workgroup ticket), the sum-of-squares pass and the coefficient of clip_grad_norm_, and the host-side argument checks.
// Everything sits in an anonymous namespace: each translation unit gets its own copy, nothing is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"

namespace {

constexpr float LOG_SQRT_2PI = 0.918938533204672742f;  // math.log(math.sqrt(2 * math.pi)) (torch Normal.log_prob)
constexpr float HALF_LOG_2PI_E = 1.418938533204672742f;  // 0.5 + 0.5 * math.log(2 * math.pi) (torch Normal.entropy)
constexpr int WS_PART0 = 8;    // workspace word of the first partial (word 0: the ticket; 64-byte offset keeps it on its own line)

template <int W> struct VecOf;
template <> struct VecOf<1> { typedef float type; };
template <> struct VecOf<2> { typedef float2 type; };
template <> struct VecOf<4> { typedef float4 type; };

template <int W> __device__ __forceinline__ void load_row(const float *p, float (&v)[W])
{
    const typename VecOf<W>::type t = *reinterpret_cast<const typename VecOf<W>::type *>(p);
    const float *f = reinterpret_cast<const float *>(&t);
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = f[k];
}

template <int W> __device__ __forceinline__ void store_row(float *p, const float (&v)[W])
{
    typename VecOf<W>::type t;
    float *f = reinterpret_cast<float *>(&t);
#pragma unroll
    for (int k = 0; k < W; ++k) f[k] = v[k];
    *reinterpret_cast<typename VecOf<W>::type *>(p) = t;
}

// distributions.py DiagGaussianDistribution.log_prob = sum over the action dimensions of torch's Normal.log_prob:
// -((a - mu)^2) / (2 sigma^2) - log(sigma) - log(sqrt(2 pi)), sigma = exp(log_std)
template <int A> __device__ __forceinline__ float diag_log_prob(const float (&act)[A], const float (&mu)[A], const float (&sig)[A])
{
    float lp = 0.0f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float d = act[k] - mu[k];
        lp += (-(d * d) / (2.0f * (sig[k] * sig[k])) - logf(sig[k])) - LOG_SQRT_2PI;
    }
    return lp;
}

// v(q) of the discrete valve face (core/common/vec_env/cstr_vec_env.py): f32(-1) + f32(2 q) / f32(K - 1), in that order
__device__ __forceinline__ float valve_of(const int q, const int K) { return -1.0f + (float)(2 * q) / (float)(K - 1); }

// sum of v over the workgroup's 256 threads in a fixed tree; every thread gets the result
__device__ __forceinline__ double block_sum_f64(double v, double *red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void publish_f64(unsigned long long *w, double v)
{
    __hip_atomic_store(w, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double consume_f64(unsigned long long *w)
{
    return __longlong_as_double((long long)__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// clip_grad_norm_ (torch.nn.utils): launch 1, per-workgroup sums of squares
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ grad, const int64_t n, double *__restrict__ part)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256ll) {
        const float g = grad[i];
        s += (double)(g * g);
    }
    const double t = block_sum_f64(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// the partials of launch 1 summed in workgroup order: coef = min(1, max_norm / (norm + 1e-6))
__device__ __forceinline__ float grad_clip_coef(const double *__restrict__ part, const int n_part, const float max_norm, float &norm)
{
    double s = 0.0;
    for (int j = 0; j < n_part; ++j) s += part[j];
    norm = (float)sqrt(s);
    return fminf(max_norm / (norm + 1e-6f), 1.0f);
}

inline bool overlap(const void *a, int64_t a_floats, const void *b, int64_t b_floats)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 4u * (uintptr_t)b_floats && b0 < a0 + 4u * (uintptr_t)a_floats;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool row_aligned(const void *p, int width) { return width == 4 ? aligned16(p) : (width == 1 ? aligned4(p) : aligned8(p)); }

inline unsigned lane_grid(int64_t n, int block, int64_t cap)
{
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}

}  // namespace
