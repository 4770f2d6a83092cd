// cstr_ars.hip -- Augmented Random Search (Mania, Guy & Recht 2018; sb3_contrib.ARS) for gfx950: a whole population of perturbed
// policies evaluated in ONE launch (cstr_ars_population_f32), selection and the parameter step in a second one (cstr_ars_update_f32),
// and the host-only shape predicate cstr_ars_supported. Two launches per update whatever n_delta is.
//
// THE DELTAS ARE NEVER STORED. delta[k][p] (direction k = 0 .. n_delta - 1, parameter p = 0 .. P - 1 in parameters() order) is a pure
// function of (seed, update index, k, p): with q = p >> 2 and e = p & 3,
//     words = Philox4x32-10(counter = (q, k, (uint32)update_index, ARS_TAG = 0xA4500D17), key = ((uint32)seed, (uint32)(seed >> 32)))
//     (z0, z1) = box_muller(words[0], words[1]);  (z2, z3) = box_muller(words[2], words[3]);  delta[k][p] = z_e
// (philox4x32_10 / box_muller of cstr_rng_device.h: u = ((w >> 8) + 0.5) * 2^-24, radius sqrt(-2 log u1), angle 2 pi u2, cos then sin).
// The tag in counter word 3 keeps the stream apart from every other Philox stream of the library. Both launches regenerate the
// deltas from these counters: the population launch to form the candidates, the update launch for the step.
//
// Candidates: theta + s * delta_k is job c = k, theta - s * delta_k is job c = n_delta + k (f32: the product is rounded, then the sum).
//
// JOB MODEL. Job c runs on env slot c % n_envs; a slot handles its jobs in increasing c, one after another, inside the launch. A job:
// the reset draw of its slot (reset_draw_env: the slot's PCG64 stream and static_init entry, the arithmetic of cstr_reset_draw_f32),
// then n_eval_episodes episodes -- per step the policy's deterministic output, predict()'s unscale (squashed) or clip, the env step of
// cstr_env_device.h; each episode is followed by the auto-reset draw -- and R_c = sum over its episodes of (f64 sum of the f32 step
// rewards) + alive_bonus_offset * (its step count). With n_envs = 1 the launch consumes the env's random stream exactly as a
// sequential host loop over the candidates does; with n_envs >= 2 n_delta every candidate runs in parallel. Slots beyond the job
// count do nothing and their state is untouched; a slot's state after the launch is what its last job left.
//
// TWO MAPPINGS. A linear policy (no hidden layer: at most 8 * 4 + 4 = 36 parameters) runs one slot per LANE with the candidate's
// weights in registers. A policy with hidden layers runs one slot per WAVE: lane j owns hidden unit j of both layers (and output j
// of the last layer) with its weight rows in registers, the hidden vector is exchanged with v_readlane (a uniform lane index: no
// LDS round trip, no bank conflicts; the 64 values are consumed in index order so the dot products have ONE summation order), and
// every lane steps the env redundantly so that the next observation needs no broadcast. The candidate's parameters are generated
// once per job by the whole wave into an LDS row and read back as rows.
// Dot products: acc = 0; acc += w[i] * x[i] for i ascending; then + bias (when the layer has one); then the activation.
//
// NO CROSS-WAVE BARRIER: every workgroup is ONE wave (64 lanes), so the __syncthreads() behind the candidate's LDS row orders that
// wave alone; trip counts differ between waves (jobs per slot, episodes that end on the env's NaN path) and nothing waits on them.
// BOUNDED LOOPS: jobs_per_slot * n_eval_episodes * max(coef.max_steps, 1) steps at most, whatever the data does.
// The statistics block is summed by the workgroup that draws the last ticket (an integer atomic; no float atomics), in a fixed order:
// lane l adds jobs l, l + 64, ... and the 64 partial sums meet in a shuffle tree.
//
// cstr_ars_update_f32: every workgroup ranks the directions by counting (top_k = max(R+_k, R-_k), a NaN counts as the greatest, ties go
// to the lower k), keeps the n_top first, computes the unbiased standard deviation of the 2 n_top kept returns and
// step_size = lr / (n_top * std + 1e-6) in f64 (fixed-order sums), and a thread per four parameters adds
// step_size * sum over the kept directions, in rank order, of (R+_k - R-_k) * delta[k][p] (f64 accumulate, one f32 rounding) to theta.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_env_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr uint32_t ARS_TAG = 0xA4500D17u;  // counter word 3 of the delta stream
constexpr int ARS_W = CSTR_ARS_MAX_WIDTH;  // 64: one lane per hidden unit
constexpr int ARS_MAX_PARAMS = ARS_W * 8 + ARS_W + ARS_W * ARS_W + ARS_W + 4 * ARS_W + 4;  // [64, 64] on the (8, 4) layout: 4996
constexpr int ARS_UPDATE_BLOCK = 256;

struct ArsArgs {
    cstr_ars_policy_t p;
    const float *theta; float delta_std; uint64_t seed; uint32_t update; int n_delta, n_episodes; double alive_bonus;
    cstr_coef_t k; int integrator;
    float *env_obs; int32_t *step_count; uint64_t *pcg; double *static_init;
    ActBounds ab; int64_t n;
    double *returns; int32_t *lengths; double *stats;
};

__device__ __forceinline__ void ars_delta_block(const uint64_t seed, const uint32_t update, const uint32_t k, const uint32_t q, float z[4])
{
    uint32_t r[4];
    philox4x32_10(q, k, update, ARS_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
}

// the four parameters 4 q .. 4 q + 3 of candidate (k, sign): theta +- delta_std * delta (entries at and beyond n_params: 0)
__device__ __forceinline__ void ars_candidate_block(const ArsArgs &a, const int n_params, const uint32_t k, const bool minus, const int q, float w[4])
{
    float z[4];
    ars_delta_block(a.seed, a.update, k, (uint32_t)q, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = 4 * q + e;
        const float sd = a.delta_std * z[e];
        w[e] = p < n_params ? (minus ? a.theta[p] - sd : a.theta[p] + sd) : 0.0f;
    }
}

__device__ __forceinline__ float ars_act(const float v, const int act) { return act == 2 ? tanhf(v) : ((v < 0.0f) ? 0.0f : v); }  // NaN stays NaN

__device__ __forceinline__ float lane_bcast(const float v, const int src)  // src: a compile-time constant after unrolling
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

__host__ __device__ inline int ars_n_params(const cstr_ars_policy_t &p)
{
    const int b = p.with_bias ? 1 : 0;
    if (p.n_hidden == 0) return p.act_dim * (p.obs_dim + b);
    if (p.n_hidden == 1) return p.h1 * (p.obs_dim + b) + p.act_dim * (p.h1 + b);
    return p.h1 * (p.obs_dim + b) + p.h2 * (p.h1 + b) + p.act_dim * (p.h2 + b);
}

// ---- the policies --------------------------------------------------------------------------------------------------------------------

// no hidden layer, a lane per slot: K [A][D] (+ b [A]) in registers
template <int L>
struct LinearPolicy {
    static constexpr int D = Lay<L>::D, A = Lay<L>::A;
    float w[A][D], b[A];

    __device__ __forceinline__ void load(const ArsArgs &a, const uint32_t k, const bool minus)
    {
        const int P = A * D + (a.p.with_bias ? A : 0);
        constexpr int NB = (A * D + A + 3) / 4;
        float flat[4 * NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) ars_candidate_block(a, P, k, minus, q, flat + 4 * q);
#pragma unroll
        for (int r = 0; r < A; ++r) {
#pragma unroll
            for (int d = 0; d < D; ++d) w[r][d] = flat[r * D + d];
            b[r] = flat[A * D + r];  // 0 without bias (beyond n_params)
        }
    }

    __device__ __forceinline__ void operator()(const ArsArgs &a, const float o[2][4], float out[4]) const
    {
#pragma unroll
        for (int r = 0; r < A; ++r) {
            float acc = 0.0f;
#pragma unroll
            for (int d = 0; d < D; ++d) acc += w[r][d] * o[d >> 2][d & 3];
            if (a.p.with_bias) acc += b[r];
            out[r] = a.p.squash ? tanhf(acc) : acc;
        }
    }
};

// one or two hidden layers, a wave per slot: lane j owns unit j of every layer
template <int L>
struct WavePolicy {
    static constexpr int D = Lay<L>::D, A = Lay<L>::A;
    float w1[D], b1, w2[ARS_W], b2, w3[ARS_W], b3;

    // the whole wave writes the candidate into `row` (LDS, n_params floats rounded up to 4), then every lane takes its rows
    __device__ __forceinline__ void load(const ArsArgs &a, const uint32_t k, const bool minus, float *row, const int lane)
    {
        const int P = ars_n_params(a.p), H1 = a.p.h1, H2 = a.p.h2, nb = a.p.with_bias ? 1 : 0, two = a.p.n_hidden == 2;
        __syncthreads();  // one wave per workgroup: the rows of the previous job have been read
        for (int q = lane; 4 * q < P; q += 64) {
            float v[4];
            ars_candidate_block(a, P, k, minus, q, v);
            *reinterpret_cast<float4 *>(row + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        const int o_b1 = H1 * D, o_w2 = o_b1 + nb * H1, o_b2 = o_w2 + (two ? H2 * H1 : 0), o_w3 = o_b2 + (two ? nb * H2 : 0);
        const int HL = two ? H2 : H1, o_b3 = o_w3 + A * HL;
#pragma unroll
        for (int d = 0; d < D; ++d) w1[d] = lane < H1 ? row[lane * D + d] : 0.0f;
        b1 = (nb && lane < H1) ? row[o_b1 + lane] : 0.0f;
#pragma unroll
        for (int i = 0; i < ARS_W; ++i) w2[i] = (two && lane < H2 && i < H1) ? row[o_w2 + lane * H1 + i] : 0.0f;
        b2 = (two && nb && lane < H2) ? row[o_b2 + lane] : 0.0f;
#pragma unroll
        for (int i = 0; i < ARS_W; ++i) w3[i] = (lane < A && i < HL) ? row[o_w3 + lane * HL + i] : 0.0f;
        b3 = (nb && lane < A) ? row[o_b3 + lane] : 0.0f;
    }

    __device__ __forceinline__ void operator()(const ArsArgs &a, const float o[2][4], float out[4]) const
    {
        const int H1 = a.p.h1, H2 = a.p.h2, nb = a.p.with_bias, two = a.p.n_hidden == 2, HL = two ? H2 : H1;
        const int lane = threadIdx.x;
        float acc = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) acc += w1[d] * o[d >> 2][d & 3];
        if (nb) acc += b1;
        float h = lane < H1 ? ars_act(acc, a.p.act) : 0.0f;
        if (two) {
            acc = 0.0f;
#pragma unroll
            for (int i = 0; i < ARS_W; ++i) {
                if (i < H1) acc += w2[i] * lane_bcast(h, i);  // wave-uniform guard
            }
            if (nb) acc += b2;
            h = lane < H2 ? ars_act(acc, a.p.act) : 0.0f;
        }
        acc = 0.0f;
#pragma unroll
        for (int i = 0; i < ARS_W; ++i) {
            if (i < HL) acc += w3[i] * lane_bcast(h, i);  // wave-uniform guard
        }
        if (nb) acc += b3;
        const float y = a.p.squash ? tanhf(acc) : acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = r < A ? lane_bcast(y, r) : 0.0f;
    }
};

// ---- one job: reset draw, n_episodes episodes, R_c ---------------------------------------------------------------------------------
template <int L, typename Policy>
__device__ __forceinline__ void ars_run_job(const ArsArgs &a, const Policy &pol, float o[2][4], int32_t &st, uint64_t pst[4], double *sinit,
                                            double &ret, int32_t &len)
{
    constexpr int A = Lay<L>::A;
    reset_draw_env<L>(a.k, pst, sinit, 0, o);  // evaluate_policy's env.reset()
    st = 0;
    double total = 0.0;
    len = 0;
    const int max_t = a.k.max_steps > 1 ? a.k.max_steps : 1;
    for (int ep = 0; ep < a.n_episodes; ++ep) {
        double cur = 0.0;  // current_rewards: float64
        for (int t = 0; t < max_t; ++t) {  // the env truncates at max_steps: the bound holds whatever the data does
            float y[4], ea[4] = {0.0f, 0.0f, 0.0f, 0.0f}, on[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}}, rew;
            pol(a, o, y);
#pragma unroll
            for (int j = 0; j < A; ++j)
                ea[j] = a.p.squash ? unscale_action(y[j], a.ab.lo[j], a.ab.hi[j]) : clip_keep_nan(y[j], a.ab.lo[j], a.ab.hi[j]);
            const bool done = a.integrator == CSTR_INTEGRATOR_EULER ? env_step_lane<L, CSTR_INTEGRATOR_EULER>(a.k, o, ea, st, on, rew)
                                                                    : env_step_lane<L, CSTR_INTEGRATOR_RK4>(a.k, o, ea, st, on, rew);
            cur += (double)rew;
            len += 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j >> 2][j & 3] = on[j >> 2][j & 3];
            if (done) break;
        }
        total += cur;
        reset_draw_env<L>(a.k, pst, sinit, 0, o);  // auto-reset (dummy_vec_env.py:68-72)
        st = 0;
    }
    ret = total + a.alive_bonus * (double)len;
}

template <int L>
struct SlotState {
    float o[2][4]; int32_t st; uint64_t pst[4]; double sloc[8]; double *sinit;

    __device__ __forceinline__ void load(const ArsArgs &a, const int64_t slot)
    {
        constexpr int TR = Lay<L>::TR;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j >> 2][j & 3] = 0.0f;
        load_obs<L>(a.env_obs, slot, o);
        st = a.step_count[slot];
        load_pcg(a.pcg, slot, pst);
        sinit = nullptr;
        if (a.static_init) {
#pragma unroll
            for (int j = 0; j < 4 * TR; ++j) sloc[j] = a.static_init[4 * TR * slot + j];
            sinit = sloc;
        }
    }

    __device__ __forceinline__ void store(const ArsArgs &a, const int64_t slot) const
    {
        constexpr int TR = Lay<L>::TR;
        store_obs<L>(a.env_obs, slot, o);
        a.step_count[slot] = st;
        *reinterpret_cast<ulonglong2 *>(a.pcg + 4 * slot) = make_ulonglong2(pst[0], pst[1]);
        if (a.static_init) {
#pragma unroll
            for (int j = 0; j < 4 * TR; ++j) a.static_init[4 * TR * slot + j] = sloc[j];
        }
    }
};

// The statistics block, by the workgroup that finishes last: stats = {sum of lengths, sum of returns, NaN returns, ticket}. Word 3 is a
// 64-bit ticket counter (zero on entry, zero again on exit). Every workgroup is one wave.
__device__ __forceinline__ void ars_finish(const ArsArgs &a, const int lane)
{
    unsigned long long *ticket = reinterpret_cast<unsigned long long *>(a.stats + 3);
    __threadfence();  // this wave's returns / lengths are visible device-wide before its ticket is
    int last = 0;
    if (lane == 0) last = atomicAdd(ticket, 1ULL) == (unsigned long long)gridDim.x - 1ULL;
    last = __shfl(last, 0);
    if (!last) return;
    __threadfence();
    const int jobs = 2 * a.n_delta;
    double rs = 0.0;
    long long ls = 0;
    int nn = 0;
    for (int c = lane; c < jobs; c += 64) {
        const double r = __hip_atomic_load(a.returns + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ls += __hip_atomic_load(a.lengths + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rs += r;
        nn += (r != r) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        rs += __shfl_down(rs, off);
        ls += __shfl_down(ls, off);
        nn += __shfl_down(nn, off);
    }
    if (lane == 0) {
        a.stats[0] = (double)ls;
        a.stats[1] = rs;
        a.stats[2] = (double)nn;
        *ticket = 0ULL;
    }
}

// a lane per slot (linear policies)
template <int L>
__global__ __launch_bounds__(64) void ars_population_lane_kernel(const ArsArgs a)
{
    const int lane = threadIdx.x, jobs = 2 * a.n_delta;
    const int64_t slot = (int64_t)blockIdx.x * 64 + lane;
    if (slot < a.n && slot < jobs) {
        SlotState<L> s;
        s.load(a, slot);
        for (int64_t c = slot; c < jobs; c += a.n) {
            const bool minus = c >= a.n_delta;
            LinearPolicy<L> pol;
            pol.load(a, (uint32_t)(minus ? c - a.n_delta : c), minus);
            double ret;
            int32_t len;
            ars_run_job<L>(a, pol, s.o, s.st, s.pst, s.sinit, ret, len);
            a.returns[c] = ret;
            a.lengths[c] = len;
        }
        s.store(a, slot);
    }
    ars_finish(a, lane);
}

// a wave per slot (policies with hidden layers)
template <int L>
__global__ __launch_bounds__(64) void ars_population_wave_kernel(const ArsArgs a)
{
    __shared__ __attribute__((aligned(16))) float row[(ARS_MAX_PARAMS + 3) / 4 * 4];
    const int lane = threadIdx.x, jobs = 2 * a.n_delta;
    const int64_t slot = blockIdx.x;  // the grid has min(n_envs, jobs) workgroups
    SlotState<L> s;
    s.load(a, slot);
    for (int64_t c = slot; c < jobs; c += a.n) {  // wave-uniform
        const bool minus = c >= a.n_delta;
        WavePolicy<L> pol;
        pol.load(a, (uint32_t)(minus ? c - a.n_delta : c), minus, row, lane);
        double ret;
        int32_t len;
        ars_run_job<L>(a, pol, s.o, s.st, s.pst, s.sinit, ret, len);  // every lane steps the env: the same values in all of them
        if (lane == 0) {
            a.returns[c] = ret;
            a.lengths[c] = len;
        }
    }
    if (lane == 0) s.store(a, slot);
    ars_finish(a, lane);
}

// ---- the update launch -----------------------------------------------------------------------------------------------------------------
struct ArsUpdateArgs {
    float *theta; int n_params; const double *returns; int n_delta, n_top; double lr; uint64_t seed; uint32_t update;
    double *out; int32_t *kept;
};

// a beats b in the descending order: NaN is the greatest, equal values (two NaNs included) go to the lower index
__device__ __forceinline__ bool ars_beats(const double a, const int ia, const double b, const int ib)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ia < ib);
    return a > b || (a == b && ia < ib);
}

// fixed-order block sum: thread t adds elements t, t + B, ...; the B partial sums meet in a tree in LDS
__device__ __forceinline__ double ars_block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = ARS_UPDATE_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(ARS_UPDATE_BLOCK) void ars_update_kernel(const ArsUpdateArgs a)
{
    extern __shared__ double ars_lds[];
    double *top = ars_lds, *red = top + a.n_delta;                  // [n_delta], [ARS_UPDATE_BLOCK]
    int32_t *kept = reinterpret_cast<int32_t *>(red + ARS_UPDATE_BLOCK);  // [n_top]
    const int t = threadIdx.x, nd = a.n_delta, nt = a.n_top;
    for (int k = t; k < nd; k += ARS_UPDATE_BLOCK) {
        const double rp = a.returns[k], rm = a.returns[nd + k];
        top[k] = (rp != rp || rm != rm) ? (rp != rp ? rp : rm) : (rp > rm ? rp : rm);  // torch.maximum: NaN propagates
    }
    __syncthreads();
    for (int k = t; k < nd; k += ARS_UPDATE_BLOCK) {  // rank by counting
        const double v = top[k];
        int rank = 0;
        for (int j = 0; j < nd; ++j) rank += ars_beats(top[j], j, v, k) ? 1 : 0;
        if (rank < nt) kept[rank] = k;
    }
    __syncthreads();
    // unbiased standard deviation of cat(R+[kept], R-[kept]) (2 n_top values), f64
    double s = 0.0;
    for (int i = t; i < 2 * nt; i += ARS_UPDATE_BLOCK) s += i < nt ? a.returns[kept[i]] : a.returns[nd + kept[i - nt]];
    const double mean = ars_block_sum(s, red) / (double)(2 * nt);
    s = 0.0;
    for (int i = t; i < 2 * nt; i += ARS_UPDATE_BLOCK) {
        const double d = (i < nt ? a.returns[kept[i]] : a.returns[nd + kept[i - nt]]) - mean;
        s += d * d;
    }
    const double ret_std = sqrt(ars_block_sum(s, red) / (double)(2 * nt - 1));
    const double step = a.lr / ((double)nt * ret_std + 1e-6);
    if (blockIdx.x == 0) {
        if (t == 0) { a.out[0] = step; a.out[1] = ret_std; }
        for (int i = t; i < nt; i += ARS_UPDATE_BLOCK) a.kept[i] = kept[i];
    }
    // theta += step * sum over the kept directions, in rank order, of (R+ - R-) * delta: a thread per four parameters
    const int q = blockIdx.x * ARS_UPDATE_BLOCK + t;
    if (4 * q < a.n_params) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < nt; ++i) {
            const int k = kept[i];
            const double d = a.returns[k] - a.returns[nd + k];
            float z[4];
            ars_delta_block(a.seed, a.update, (uint32_t)k, (uint32_t)q, z);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += d * (double)z[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * q + e < a.n_params) a.theta[4 * q + e] = (float)((double)a.theta[4 * q + e] + step * acc[e]);
    }
}

struct Span { const char *lo, *hi; };

static inline Span span_of(const void *p, int64_t bytes) { return Span{static_cast<const char *>(p), static_cast<const char *>(p) + bytes}; }
static inline bool overlaps(const Span &x, const Span &y) { return x.lo && y.lo && x.lo < y.hi && y.lo < x.hi; }
static inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

static int policy_ok(int obs_dim, int act_dim, int n_hidden, int h1, int h2, int act, int with_bias, int squash)
{
    if (layout_of(obs_dim, act_dim) < 0) return 0;
    if (n_hidden < 0 || n_hidden > 2 || (with_bias & ~1) || (squash & ~1)) return 0;
    if (n_hidden >= 1 && (h1 < 1 || h1 > ARS_W || (act != 1 && act != 2))) return 0;
    if (n_hidden == 2 && (h2 < 1 || h2 > ARS_W)) return 0;
    return 1;
}

}  // namespace

extern "C" int cstr_ars_supported(int obs_dim, int act_dim, int n_hidden_layers, int h1, int h2, int act, int with_bias, int squash, int n_delta,
                                  int n_top)
{
    if (!policy_ok(obs_dim, act_dim, n_hidden_layers, h1, h2, act, with_bias, squash)) return 0;
    return (n_delta >= 1 && n_delta <= CSTR_ARS_MAX_DELTA && n_top >= 1 && n_top <= n_delta) ? 1 : 0;
}

extern "C" int cstr_ars_population_f32(const cstr_ars_policy_t *policy, const float *theta, float delta_std, uint64_t seed, int64_t update_index,
                                       int n_delta, int n_eval_episodes, double alive_bonus_offset, const cstr_coef_t *coef, int integrator,
                                       float *env_obs, int32_t *step_count, uint64_t *pcg_state, double *static_init, const float *act_low,
                                       const float *act_high, int64_t n_envs, double *returns, int32_t *lengths, double *stats,
                                       cstr_stream_t stream)
{
    if (!policy || !theta || !coef || !env_obs || !step_count || !pcg_state || !act_low || !act_high || !returns || !lengths || !stats)
        return CSTR_E_BADARG;
    if (n_envs <= 0 || n_delta < 1 || n_eval_episodes < 1 || !(delta_std > 0.0f) || update_index < 0 || update_index > 0xffffffffLL ||
        alive_bonus_offset != alive_bonus_offset)
        return CSTR_E_BADARG;
    const cstr_ars_policy_t &p = *policy;
    if (!policy_ok(p.obs_dim, p.act_dim, p.n_hidden, p.h1, p.h2, p.act, p.with_bias, p.squash) || n_delta > CSTR_ARS_MAX_DELTA ||
        (integrator != CSTR_INTEGRATOR_EULER && integrator != CSTR_INTEGRATOR_RK4))
        return CSTR_E_UNSUPPORTED;
    if (!aligned16(env_obs) || !aligned16(pcg_state) || !aligned4(theta) || !aligned4(step_count) || !aligned4(lengths) || !aligned8(returns) ||
        !aligned8(stats) || (static_init && !aligned8(static_init)))
        return CSTR_E_BADARG;
    const int lay = layout_of(p.obs_dim, p.act_dim), A = p.act_dim, TR = lay == 2 ? 2 : 1, jobs = 2 * n_delta;
    ArsArgs a;
    for (int j = 0; j < 4; ++j) {
        a.ab.lo[j] = j < A ? act_low[j] : -1.0f;
        a.ab.hi[j] = j < A ? act_high[j] : 1.0f;
        if (!(a.ab.hi[j] > a.ab.lo[j])) return CSTR_E_BADARG;
    }
    {   // nothing the launch writes may overlap anything it reads or anything else it writes (the env state is read and written)
        constexpr int NW = 7;
        const Span wr[NW] = {span_of(returns, 8LL * jobs), span_of(lengths, 4LL * jobs), span_of(stats, 32), span_of(env_obs, 4 * n_envs * p.obs_dim),
                             span_of(step_count, 4 * n_envs), span_of(pcg_state, 32 * n_envs), span_of(static_init, 32 * TR * n_envs)};
        const Span rd = span_of(theta, 4LL * ars_n_params(p));
        for (int i = 0; i < NW; ++i) {
            if (overlaps(wr[i], rd)) return CSTR_E_BADARG;
            for (int j = i + 1; j < NW; ++j)
                if (overlaps(wr[i], wr[j])) return CSTR_E_BADARG;
        }
    }
    a.p = p;
    a.theta = theta; a.delta_std = delta_std; a.seed = seed; a.update = (uint32_t)update_index; a.n_delta = n_delta; a.n_episodes = n_eval_episodes;
    a.alive_bonus = alive_bonus_offset;
    a.k = *coef; a.integrator = integrator;
    a.env_obs = env_obs; a.step_count = step_count; a.pcg = pcg_state; a.static_init = static_init;
    a.n = n_envs;
    a.returns = returns; a.lengths = lengths; a.stats = stats;
    const int64_t slots = n_envs < jobs ? n_envs : jobs;
    hipStream_t s = (hipStream_t)stream;
    if (p.n_hidden == 0) {
        const unsigned grid = (unsigned)((slots + 63) / 64);
        if (lay == 0) ars_population_lane_kernel<0><<<grid, 64, 0, s>>>(a);
        else if (lay == 1) ars_population_lane_kernel<1><<<grid, 64, 0, s>>>(a);
        else ars_population_lane_kernel<2><<<grid, 64, 0, s>>>(a);
    } else {
        const unsigned grid = (unsigned)slots;
        if (lay == 0) ars_population_wave_kernel<0><<<grid, 64, 0, s>>>(a);
        else if (lay == 1) ars_population_wave_kernel<1><<<grid, 64, 0, s>>>(a);
        else ars_population_wave_kernel<2><<<grid, 64, 0, s>>>(a);
    }
    return (int)hipGetLastError();
}

extern "C" int cstr_ars_update_f32(float *theta, int64_t n_params, const double *returns, int n_delta, int n_top, double learning_rate,
                                   uint64_t seed, int64_t update_index, double *out, int32_t *kept, cstr_stream_t stream)
{
    if (!theta || !returns || !out || !kept) return CSTR_E_BADARG;
    if (n_params < 1 || n_delta < 1 || n_top < 1 || n_top > n_delta || update_index < 0 || update_index > 0xffffffffLL ||
        learning_rate != learning_rate)
        return CSTR_E_BADARG;
    if (n_delta > CSTR_ARS_MAX_DELTA || n_params > ARS_MAX_PARAMS) return CSTR_E_UNSUPPORTED;
    if (!aligned4(theta) || !aligned8(returns) || !aligned8(out) || !aligned4(kept)) return CSTR_E_BADARG;
    {
        const Span wr[3] = {span_of(theta, 4 * n_params), span_of(out, 16), span_of(kept, 4LL * n_top)};
        const Span rd = span_of(returns, 16LL * n_delta);
        for (int i = 0; i < 3; ++i) {
            if (overlaps(wr[i], rd)) return CSTR_E_BADARG;
            for (int j = i + 1; j < 3; ++j)
                if (overlaps(wr[i], wr[j])) return CSTR_E_BADARG;
        }
    }
    const ArsUpdateArgs a = {theta, (int)n_params, returns, n_delta, n_top, learning_rate, seed, (uint32_t)update_index, out, kept};
    const unsigned grid = (unsigned)(((n_params + 3) / 4 + ARS_UPDATE_BLOCK - 1) / ARS_UPDATE_BLOCK);
    const size_t lds = sizeof(double) * ((size_t)n_delta + ARS_UPDATE_BLOCK) + sizeof(int32_t) * (size_t)n_top;
    ars_update_kernel<<<grid, ARS_UPDATE_BLOCK, lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
