// cstr_her.hip -- Hindsight Experience Replay on the goal-conditioned face of the CSTR env, for gfx950 (MI355X):
//   cstr_goal_vec_step_f32  VecEnv.step on the goal face: the env step of cstr_env_device.h, the goal reward with the lane's own
//                           target, auto-reset from the env's PCG64 stream, the Philox target redraw, flat [ag | dg | obs] rows;
//   cstr_her_add_f32        HerReplayBuffer.add + _compute_episode_length (core/her/her_replay_buffer.py:135-184), a lane per env;
//   cstr_goal_collect_step_f32  the rollout's vec-step on the goal face in one launch: the action scaling chain of cstr_collect_step_f32, the
//                           two launches above (their bodies, as shared device functions) and Monitor's episode statistics;
//   cstr_her_sample_f32     HerReplayBuffer.sample (:186-384) in one launch on NumPy's legacy MT19937 stream.
// The goal has one dimension: achieved_goal = observation[2] (normalised C2), so the ring stores no achieved goals.
//
// The sampler is ONE workgroup. Wave 0 owns the MT19937 stream (one-wave twist and index draw of cstr_mt_device.h); the goal
// draw of `future` / `episode` is NumPy's array-form randint, i.e. one scalar masked-rejection draw per element in order, each
// with its own mask: wave 0 walks it with wave-uniform control flow (every lane reads the same LDS word). Selecting the k-th valid
// transition and the gather are a lane per sample. Valid transitions are found through two summaries that cstr_her_add_f32 keeps
// current: row_valid[r] (valid envs of ring row r) and valid_bits[r][w] (bit e of word w: env 64 w + e is valid).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"

#include "cstr_env_device.h"
#include "cstr_goal_device.h"
#include "cstr_mt_device.h"
#include "cstr_rng_device.h"

namespace {

constexpr int HER_TPB = 256;
// ---- VecEnv.step on the goal face (dummy_vec_env.py:56-73 over TwoSeriesCSTREnv.step) ------------------------------------------
// What env i's step leaves in registers for the launch around it: the true next observation (terminal where done) with the OLD goal,
// reward, done / truncated and the step count the episode has reached (before the auto-reset zeroes it).
struct GoalStep { float on[4], dg, r; int32_t st; bool d, trunc; };

// Env i of VecEnv.step on the goal face: the env step on action a[0..1], the goal reward on the lane's own target (NaN action or state:
// old state, -10, truncated), auto-reset from the env's PCG64 stream, the Philox target redraw with episode[i] += 1, step_count, the
// env state and the row VecEnv.step returns (rows_after). Shared by goal_step_kernel and goal_collect_step_kernel.
template <int INTEG>
__device__ __forceinline__ void goal_step_lane(const cstr_coef_t &k, float *env_obs, const float a[4], int32_t *step_count, uint64_t *pcg,
                                               double *static_init, float *target, const GoalDraw &gd, float *rows_after, const int64_t i,
                                               GoalStep &s)
{
    float o[2][4], raw[4], r;
    load_obs<0>(env_obs, i, o);
    int32_t st = step_count[i];
    float tg = target[i];
    bool bad = (a[0] != a[0]) || (a[1] != a[1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= (o[0][j] != o[0][j]);
    const bool trunc = cstr_step_lane<INTEG>(k, o[0], a[0], a[1], st, s.on, raw, r);
    const float dg = goal_of_target(k, tg);
    if (!bad) r = goal_reward(k.s_lo[2], k.s_span[2], k.conc_span, s.on[2], dg);  // NaN path: old state, -10, truncated
    const bool d = trunc;
    s.dg = dg; s.r = r; s.st = st; s.d = d; s.trunc = trunc;
    if (d) {  // dummy_vec_env.py:68-72: the env's own reset stream, as cstr_reset_draw_f32 consumes it
        uint64_t pst[4];
        load_pcg(pcg, i, pst);
        float ro[2][4];
        reset_draw_env<0>(k, pst, static_init, i, ro);
        *reinterpret_cast<ulonglong2 *>(pcg + 4 * i) = make_ulonglong2(pst[0], pst[1]);
        store_obs<0>(env_obs, i, ro);
        float dg2 = dg;
        if (gd.episode) {  // target of the episode that starts now: counter (env index, episode ordinal, tag), key = goal seed
            const int32_t e = gd.episode[i];
            tg = goal_draw_target(gd, i, e);
            target[i] = tg;
            gd.episode[i] = e + 1;
            dg2 = goal_of_target(k, tg);
        }
        store_row6(rows_after, i, dg2, ro[0]);
        st = 0;
    } else {
        float oo[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) oo[0][j] = s.on[j];
        store_obs<0>(env_obs, i, oo);
        store_row6(rows_after, i, dg, s.on);
    }
    step_count[i] = st;
}

template <int INTEG>
__global__ void goal_step_kernel(const cstr_coef_t k, float *__restrict__ env_obs, const float *__restrict__ act, int32_t *__restrict__ step_count,
                                 uint64_t *__restrict__ pcg, double *__restrict__ static_init, float *__restrict__ target, const GoalDraw gd,
                                 float *__restrict__ next_rows, float *__restrict__ rows_after, float *__restrict__ reward,
                                 float *__restrict__ done, float *__restrict__ timeout, const int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float a[4];
        GoalStep s;
        load_act<2>(act, i, a);
        goal_step_lane<INTEG>(k, env_obs, a, step_count, pcg, static_init, target, gd, rows_after, i, s);
        store_row6(next_rows, i, s.dg, s.on);
        reward[i] = s.r;
        done[i] = s.d ? 1.0f : 0.0f;
        timeout[i] = s.trunc ? 1.0f : 0.0f;
    }
}

// ---- HerReplayBuffer.add -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void her_set_valid(const cstr_her_t &h, const int64_t words, const int64_t r, const int64_t i, const bool valid)
{
    unsigned long long *w = reinterpret_cast<unsigned long long *>(h.valid_bits) + r * words + (i >> 6);
    const unsigned long long bit = 1ULL << (i & 63);
    if (valid) {
        if (!(atomicOr(w, bit) & bit)) atomicAdd(h.row_valid + r, 1);
    } else {
        if (atomicAnd(w, ~bit) & bit) atomicSub(h.row_valid + r, 1);
    }
}

// Env i of HerReplayBuffer.add at ring row `pos`: x / y = observation / next observation (columns 2..5 of the flat rows), dg = column 1
// of the observation row, a = the buffer action. Shared by her_add_kernel and goal_collect_step_kernel.
__device__ __forceinline__ void her_add_lane(const cstr_ring_t &ring, const cstr_her_t &h, const int64_t pos, const int64_t words, const int64_t i,
                                             const float4 x, const float4 y, const float dg, const float2 a, const float rw, const float dn,
                                             const float to)
{
    const int64_t n = ring.n_envs, rows = ring.rows, o = pos * n + i;
    // her_replay_buffer.py:148-154: writing onto an old episode deletes the whole of it
    const int32_t len0 = h.ep_length[o];
    if (len0 > 0) {
        const int64_t end = (int64_t)h.ep_start[o] + len0;
        for (int64_t j = pos; j < end; ++j) {  // np.arange(pos, episode_end) % buffer_size
            const int64_t r = j % rows;
            if (h.ep_length[r * n + i] > 0) her_set_valid(h, words, r, i, false);
            h.ep_length[r * n + i] = 0;
        }
    }
    const int32_t cs = h.cur_ep_start[i];
    h.ep_start[o] = cs;  // :157
    // :162, DictReplayBuffer.add: the row; achieved_goal is column 2 of the observation and is not stored
    *reinterpret_cast<float4 *>(ring.obs + o * 4) = x;
    *reinterpret_cast<float4 *>(ring.next_obs + o * 4) = y;
    *reinterpret_cast<float2 *>(ring.act + o * 2) = a;
    h.desired_goal[o] = dg;
    ring.rew[o] = rw;
    ring.done[o] = dn;
    ring.timeout[o] = to;
    if (dn != 0.0f) {  // :165-184, _compute_episode_length with self.pos already advanced by the add
        const int64_t new_pos = (pos + 1 == rows) ? 0 : pos + 1;
        int64_t end = new_pos;
        if (end < cs) end += rows;
        const int32_t len = (int32_t)(end - cs);
        for (int64_t j = cs; j < end; ++j) {  // np.arange(episode_start, episode_end) % buffer_size
            const int64_t r = j % rows;
            h.ep_length[r * n + i] = len;
            her_set_valid(h, words, r, i, true);
        }
        h.cur_ep_start[i] = (int32_t)new_pos;
    }
}

__global__ void her_add_kernel(const cstr_ring_t ring, const cstr_her_t h, int64_t *__restrict__ ring_ctl, const float *__restrict__ obs_rows,
                               const float *__restrict__ next_rows, const float *__restrict__ act, const float *__restrict__ rew,
                               const float *__restrict__ done, const float *__restrict__ timeout)
{
    const int64_t n = ring.n_envs, pos = ring_ctl[0], words = (n + 63) >> 6;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float2 g = *reinterpret_cast<const float2 *>(obs_rows + 6 * i);
        const float2 x01 = *reinterpret_cast<const float2 *>(obs_rows + 6 * i + 2), x23 = *reinterpret_cast<const float2 *>(obs_rows + 6 * i + 4);
        const float2 y01 = *reinterpret_cast<const float2 *>(next_rows + 6 * i + 2), y23 = *reinterpret_cast<const float2 *>(next_rows + 6 * i + 4);
        her_add_lane(ring, h, pos, words, i, make_float4(x01.x, x01.y, x23.x, x23.y), make_float4(y01.x, y01.y, y23.x, y23.y), g.y,
                     *reinterpret_cast<const float2 *>(act + 2 * i), rew[i], done[i], timeout[i]);
    }
    ring_advance_last_block(ring_ctl, ring.rows);
}

// ---- the goal face's collect step: action chain + VecEnv.step + HerReplayBuffer.add + Monitor statistics, ONE launch ------------------
// (off_policy_algorithm.py:364-411, :564, :580 on the goal face.) A lane per env; N x ~100 bytes, launch-latency-bound. Everything an env
// needs besides its own rows is wave-uniform (kernarg segment); the ring position is read once in front of the arithmetic.
struct GoalCollectArgs {
    cstr_ring_t ring;
    cstr_her_t her;
    float *env_obs, *rows; int32_t *step_count; uint64_t *pcg; double *static_init; float *target;
    GoalDraw gd;
    int squashed; ActBounds ab;
    const float *noise;
    float *reward_out, *done_out, *timeout_out, *next_rows_out, *ep_return; double *ep_stats;
};

template <int INTEG>
__global__ void goal_collect_step_kernel(const cstr_coef_t k, const GoalCollectArgs c, int64_t *__restrict__ ring_ctl,
                                         const float *__restrict__ policy_out, uint64_t *__restrict__ policy_rng_ctl,
                                         const uint64_t policy_rng_advance)
{
    const int64_t n = c.ring.n_envs, words = (n + 63) >> 6;
    const int64_t pos = ring_ctl[0];  // wave-uniform scalar load
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float u[4], z[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sa[4], ea[4];
        load_act<2>(policy_out, i, u);
        if (c.noise) load_act<2>(c.noise, i, z);
        // _last_obs: the env's own row is the transition's observation row; the step below writes what VecEnv.step returns over it
        const float2 g = *reinterpret_cast<const float2 *>(c.rows + 6 * i);
        const float2 x01 = *reinterpret_cast<const float2 *>(c.rows + 6 * i + 2), x23 = *reinterpret_cast<const float2 *>(c.rows + 6 * i + 4);
        const float ep_ret = c.ep_return ? c.ep_return[i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) action_scale_chain(c.squashed, c.ab.lo[j], c.ab.hi[j], u[j], c.noise != nullptr, z[j], sa[j], ea[j]);
        ea[2] = ea[3] = 0.0f;
        GoalStep s;
        goal_step_lane<INTEG>(k, c.env_obs, ea, c.step_count, c.pcg, c.static_init, c.target, c.gd, c.rows, i, s);
        const float dn = s.d ? 1.0f : 0.0f, to = s.trunc ? 1.0f : 0.0f;
        if (c.next_rows_out) store_row6(c.next_rows_out, i, s.dg, s.on);
        if (c.reward_out) c.reward_out[i] = s.r;
        if (c.done_out) c.done_out[i] = dn;
        if (c.timeout_out) c.timeout_out[i] = to;
        her_add_lane(c.ring, c.her, pos, words, i, make_float4(x01.x, x01.y, x23.x, x23.y), make_float4(s.on[0], s.on[1], s.on[2], s.on[3]), g.y,
                     make_float2(sa[0], sa[1]), s.r, dn, to);
        if (c.ep_return) {  // Monitor semantics: return / length of the episode that ends here (the convention of cstr_collect_step_f32)
            const float ret = ep_ret + s.r;
            c.ep_return[i] = s.d ? 0.0f : ret;
            if (s.d) {
                atomicAdd(c.ep_stats + 0, 1.0);
                atomicAdd(c.ep_stats + 1, (double)ret);
                atomicAdd(c.ep_stats + 2, (double)s.st);
            }
        }
    }
    ring_advance_last_block(ring_ctl, c.ring.rows, policy_rng_ctl, policy_rng_advance);
}

// ---- HerReplayBuffer.sample --------------------------------------------------------------------------------------------------
struct HerSampleArgs {
    cstr_ring_t ring;
    cstr_her_t her;
    uint32_t *mt_state;
    int batch, nb_virtual, strategy;
    float s_lo2, s_span2, conc_span;
    const int64_t *forced_row, *forced_env, *forced_goal;
    float *out_obs, *out_act, *out_next_obs, *out_done, *out_rew;
    int64_t *out_row_idx, *out_env_idx, *out_goal_row;
    int32_t *status;
};

__device__ __forceinline__ int64_t clamp_index(const int64_t v, const int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__global__ __launch_bounds__(HER_TPB) void her_sample_kernel(const HerSampleArgs a)
{
    __shared__ uint32_t mt[MT_N];
    __shared__ int part[HER_TPB];
    extern __shared__ __align__(16) int32_t dyn[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, B = a.batch, nbv = a.nb_virtual;
    const int64_t rows = a.ring.rows, n = a.ring.n_envs, words = (n + 63) >> 6;
    int32_t *pre = dyn;                    // [rows] inclusive prefix sum of row_valid
    int32_t *s_row = dyn + rows;           // [B] per sample, in draw order
    int32_t *s_env = s_row + B, *s_lo = s_env + B, *s_hi = s_lo + B, *s_start = s_hi + B;
    const bool forced = a.forced_row != nullptr;

    for (int i = t; i < MT_N; i += HER_TPB) mt[i] = a.mt_state[i];
    int pos = (int)min(a.mt_state[MT_N], (uint32_t)MT_N);  // used by wave 0 only; never past the LDS image
    // inclusive prefix sum of the valid counts: a contiguous chunk of rows per lane, then the 256 chunk totals
    const int64_t chunk = (rows + HER_TPB - 1) / HER_TPB, r0 = (int64_t)t * chunk, r1 = (r0 + chunk < rows) ? r0 + chunk : rows;
    int acc = 0;
    for (int64_t r = r0; r < r1; ++r) { acc += a.her.row_valid[r]; pre[r] = acc; }
    part[t] = acc;
    __syncthreads();
    int before = 0, n_valid = 0;
    for (int i = 0; i < HER_TPB; ++i) { const int c = part[i]; if (i < t) before += c; n_valid += c; }
    for (int64_t r = r0; r < r1; ++r) pre[r] += before;
    if (!forced && n_valid <= 0) {  // her_replay_buffer.py:197-201; workgroup-uniform: nothing has been written
        if (t == 0) a.status[0] = 1;
        return;
    }
    if (t == 0) a.status[0] = 0;
    __syncthreads();
    // :210-212: np.random.choice(valid_indices, B, replace=True) draws randint(0, n_valid, B); s_row holds k for now
    if (!forced && wave == 0) pos = mt_randint_fill_wave(mt, pos, (uint32_t)(n_valid - 1), B, s_row, lane);
    __syncthreads();
    for (int s = t; s < B; s += HER_TPB) {
        int64_t row, env;
        if (forced) {
            row = clamp_index(a.forced_row[s], rows);
            env = clamp_index(a.forced_env[s], n);
        } else {  // :215, the k-th valid (row, env) in row-major order
            int k = s_row[s];
            int64_t lo = 0, hi = rows - 1;
            while (lo < hi) {  // smallest row whose inclusive prefix exceeds k
                const int64_t mid = (lo + hi) >> 1;
                if (pre[mid] > k) hi = mid; else lo = mid + 1;
            }
            row = lo;
            if (row > 0) k -= pre[row - 1];
            env = 0;
            const unsigned long long *bits = reinterpret_cast<const unsigned long long *>(a.her.valid_bits) + row * words;
            bool found = false;
            for (int64_t w0 = 0; w0 < words && !found; w0 += 8) {  // eight independent word loads in flight, then the in-order count
                unsigned long long v8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v8[j] = (w0 + j < words) ? bits[w0 + j] : 0ULL;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    unsigned long long v = v8[j];
                    const int c = __popcll(v);
                    if (!found && k < c) {
                        for (; k > 0; --k) v &= v - 1;  // drop the k lowest set bits
                        env = (w0 + j) * 64 + (int64_t)__builtin_ctzll(v);
                        found = true;
                    }
                    if (!found) k -= c;
                }
            }
            env = clamp_index(env, n);
        }
        const int64_t o = row * n + env;
        const int32_t es = a.her.ep_start[o], el = a.her.ep_length[o];
        s_row[s] = (int32_t)row;
        s_env[s] = (int32_t)env;
        s_start[s] = es;
        int32_t lo = el - 1, hi = el;  // final: batch_ep_length - 1, no draw (:366-368)
        if (a.strategy == CSTR_HER_FUTURE) lo = (int32_t)((((row - es) % rows) + rows) % rows);  // :373-374
        else if (a.strategy == CSTR_HER_EPISODE) lo = 0;                                            // :378
        s_lo[s] = lo;
        s_hi[s] = hi;
    }
    __syncthreads();
    if (wave == 0) {
        if (nbv > 0 && a.strategy != CSTR_HER_FINAL && !a.forced_goal) {
            // np.random.randint(low[], high[]): one masked-rejection draw per element, in order, none where high - low == 1
            for (int s = 0; s < nbv; ++s) {  // wave-uniform
                const int32_t lo = s_lo[s], span = s_hi[s] - lo;
                uint32_t v = 0;
                if (span > 1) {
                    const uint32_t rng = (uint32_t)(span - 1);
                    uint32_t mask = rng;
                    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
                    do {
                        if (pos == MT_N) { mt_twist_wave(mt, lane); pos = 0; }
                        v = mt_temper(mt[pos]) & mask;
                        pos += 1;
                    } while (v > rng);
                }
                if (lane == 0) s_lo[s] = lo + (int32_t)v;
            }
        }
        if (!forced || (nbv > 0 && a.strategy != CSTR_HER_FINAL && !a.forced_goal)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int i = lane; i < MT_N; i += 64) a.mt_state[i] = mt[i];
            if (lane == 0) a.mt_state[MT_N] = (uint32_t)pos;
        }
    }
    __syncthreads();
    // the five outputs: real transitions first, then the virtual ones (:228-238)
    for (int s = t; s < B; s += HER_TPB) {
        const bool virt = s < nbv;
        const int64_t b = virt ? (int64_t)(B - nbv) + s : (int64_t)s - nbv;
        const int64_t row = s_row[s], env = s_env[s], o = row * n + env;
        const float4 x = *reinterpret_cast<const float4 *>(a.ring.obs + o * 4), y = *reinterpret_cast<const float4 *>(a.ring.next_obs + o * 4);
        float dg = a.her.desired_goal[o], rw = a.ring.rew[o];
        int64_t grow = -1;
        if (virt) {
            if (a.forced_goal) grow = clamp_index(a.forced_goal[s], rows);
            else grow = ((((int64_t)s_lo[s] + s_start[s]) % rows) + rows) % rows;  // :383
            dg = a.ring.next_obs[(grow * n + env) * 4 + 2];                        // :384, next achieved goal of that transition
            rw = goal_reward(a.s_lo2, a.s_span2, a.conc_span, y.z, dg);           // :320-335
        }
        float2 *po = reinterpret_cast<float2 *>(a.out_obs + 6 * b), *pn = reinterpret_cast<float2 *>(a.out_next_obs + 6 * b);
        po[0] = make_float2(x.z, dg); po[1] = make_float2(x.x, x.y); po[2] = make_float2(x.z, x.w);
        pn[0] = make_float2(y.z, dg); pn[1] = make_float2(y.x, y.y); pn[2] = make_float2(y.z, y.w);
        *reinterpret_cast<float2 *>(a.out_act + 2 * b) = *reinterpret_cast<const float2 *>(a.ring.act + o * 2);
        a.out_done[b] = a.ring.done[o] * (1.0f - a.ring.timeout[o]);  // :281-283
        a.out_rew[b] = rw;
        if (a.out_row_idx) a.out_row_idx[b] = row;
        if (a.out_env_idx) a.out_env_idx[b] = env;
        if (a.out_goal_row) a.out_goal_row[b] = grow;
    }
}

inline bool spans_overlap(const void *p, int64_t p_bytes, const void *q, int64_t q_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p), b0 = reinterpret_cast<uintptr_t>(q);
    return a0 < b0 + (uintptr_t)q_bytes && b0 < a0 + (uintptr_t)p_bytes;
}

inline bool aligned4p(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int check_her(const cstr_ring_t *ring, const cstr_her_t *her)
{
    if (!ring || !her) return CSTR_E_BADARG;
    if (!ring->obs || !ring->next_obs || !ring->act || !ring->rew || !ring->done || !ring->timeout || ring->rows <= 0 || ring->n_envs <= 0)
        return CSTR_E_BADARG;
    if (!her->desired_goal || !her->ep_start || !her->ep_length || !her->cur_ep_start || !her->row_valid || !her->valid_bits) return CSTR_E_BADARG;
    if (ring->obs_dim != 4 || ring->act_dim != 2) return CSTR_E_UNSUPPORTED;
    if (ring->rows > CSTR_HER_MAX_ROWS || ring->n_envs > CSTR_HER_MAX_ENVS) return CSTR_E_UNSUPPORTED;
    if (ring->rows * ring->n_envs >= (1LL << 31)) return CSTR_E_UNSUPPORTED;  // the count of valid transitions is an int32
    if (!aligned16(ring->obs) || !aligned16(ring->next_obs) || !aligned8(ring->act) || !aligned8(her->valid_bits)) return CSTR_E_BADARG;
    if (!aligned4p(her->desired_goal) || !aligned4p(her->ep_start) || !aligned4p(her->ep_length) || !aligned4p(her->cur_ep_start) ||
        !aligned4p(her->row_valid))
        return CSTR_E_BADARG;
    return CSTR_OK;
}

}  // namespace

extern "C" int cstr_goal_vec_step_f32(const cstr_coef_t *coef, int integrator, int obs_dim, float *env_obs, const float *act,
                                      int32_t *step_count, uint64_t *pcg_state, double *static_init, float *target, int32_t *episode,
                                      uint64_t goal_seed, int64_t goal_index_offset, float goal_lo, float goal_hi, float *next_rows,
                                      float *rows_after, float *reward, float *done, float *timeout, int64_t n_envs, cstr_stream_t stream)
{
    if (!coef || !env_obs || !act || !step_count || !pcg_state || !target || !next_rows || !rows_after || !reward || !done || !timeout ||
        n_envs <= 0)
        return CSTR_E_BADARG;
    if (obs_dim != 4 || (integrator != CSTR_INTEGRATOR_EULER && integrator != CSTR_INTEGRATOR_RK4)) return CSTR_E_UNSUPPORTED;
    if (!aligned16(env_obs) || !aligned8(act) || !aligned16(pcg_state) || !aligned8(next_rows) || !aligned8(rows_after) || !aligned4p(target) ||
        !aligned4p(step_count) || (episode && !aligned4p(episode)))
        return CSTR_E_BADARG;
    if (episode && !(goal_lo <= goal_hi)) return CSTR_E_BADARG;
    const int64_t row_bytes = 24 * n_envs;
    if (spans_overlap(next_rows, row_bytes, rows_after, row_bytes) || spans_overlap(next_rows, row_bytes, env_obs, 16 * n_envs) ||
        spans_overlap(rows_after, row_bytes, env_obs, 16 * n_envs))
        return CSTR_E_BADARG;
    const GoalDraw gd{goal_seed, goal_index_offset, goal_lo, goal_hi, episode};
    int block, grid;
    env_launch_shape(n_envs, block, grid);
    hipStream_t s = (hipStream_t)stream;
    if (integrator == CSTR_INTEGRATOR_EULER)
        goal_step_kernel<CSTR_INTEGRATOR_EULER><<<grid, block, 0, s>>>(*coef, env_obs, act, step_count, pcg_state, static_init, target, gd, next_rows,
                                                                        rows_after, reward, done, timeout, n_envs);
    else
        goal_step_kernel<CSTR_INTEGRATOR_RK4><<<grid, block, 0, s>>>(*coef, env_obs, act, step_count, pcg_state, static_init, target, gd, next_rows,
                                                                      rows_after, reward, done, timeout, n_envs);
    return (int)hipGetLastError();
}

extern "C" int cstr_her_add_f32(const cstr_ring_t *ring, const cstr_her_t *her, int64_t *ring_ctl, const float *obs_rows, const float *next_rows,
                                const float *act, const float *rew, const float *done, const float *timeout, cstr_stream_t stream)
{
    const int rc = check_her(ring, her);
    if (rc) return rc;
    if (!ring_ctl || !obs_rows || !next_rows || !act || !rew || !done || !timeout) return CSTR_E_BADARG;
    if (!aligned8(obs_rows) || !aligned8(next_rows) || !aligned8(act) || !aligned4p(rew) || !aligned4p(done) || !aligned4p(timeout)) return CSTR_E_BADARG;
    const int64_t cells = ring->rows * ring->n_envs, n = ring->n_envs;
    if (spans_overlap(ring->obs, 16 * cells, obs_rows, 24 * n) || spans_overlap(ring->next_obs, 16 * cells, obs_rows, 24 * n) ||
        spans_overlap(ring->obs, 16 * cells, next_rows, 24 * n) || spans_overlap(ring->next_obs, 16 * cells, next_rows, 24 * n))
        return CSTR_E_BADARG;
    int block, grid;
    env_launch_shape(n, block, grid);
    her_add_kernel<<<grid, block, 0, (hipStream_t)stream>>>(*ring, *her, ring_ctl, obs_rows, next_rows, act, rew, done, timeout);
    return (int)hipGetLastError();
}

extern "C" int cstr_goal_collect_step_f32(const cstr_coef_t *coef, int integrator, int obs_dim, const cstr_ring_t *ring, const cstr_her_t *her,
                                          int64_t *ring_ctl, float *env_obs, float *rows, int32_t *step_count, uint64_t *pcg_state,
                                          double *static_init, float *target, int32_t *episode, uint64_t goal_seed, int64_t goal_index_offset,
                                          float goal_lo, float goal_hi, const float *policy_out, int squashed, const float *act_low,
                                          const float *act_high, const float *noise, float *reward_out, float *done_out, float *timeout_out,
                                          float *next_rows_out, float *ep_return, double *ep_stats, uint64_t *policy_rng_ctl,
                                          uint64_t policy_rng_advance, cstr_stream_t stream)
{
    const int rc = check_her(ring, her);
    if (rc) return rc;
    if (!coef || !ring_ctl || !env_obs || !rows || !step_count || !pcg_state || !target || !policy_out || !act_low || !act_high) return CSTR_E_BADARG;
    if ((ep_return == nullptr) != (ep_stats == nullptr)) return CSTR_E_BADARG;
    if (obs_dim != 4 || (squashed & ~1) || (integrator != CSTR_INTEGRATOR_EULER && integrator != CSTR_INTEGRATOR_RK4)) return CSTR_E_UNSUPPORTED;
    if (!aligned16(env_obs) || !aligned8(rows) || !aligned8(policy_out) || !aligned16(pcg_state) || !aligned4p(target) || !aligned4p(step_count) ||
        !aligned8(ring_ctl) || (noise && !aligned8(noise)) || (episode && !aligned4p(episode)) || (static_init && !aligned8(static_init)) ||
        (next_rows_out && !aligned8(next_rows_out)) || (reward_out && !aligned4p(reward_out)) || (done_out && !aligned4p(done_out)) ||
        (timeout_out && !aligned4p(timeout_out)) || (ep_return && !aligned4p(ep_return)) || (ep_stats && !aligned8(ep_stats)) ||
        (policy_rng_ctl && !aligned8(policy_rng_ctl)))
        return CSTR_E_BADARG;
    if (episode && !(goal_lo <= goal_hi)) return CSTR_E_BADARG;
    ActBounds ab;
    for (int j = 0; j < 4; ++j) {
        ab.lo[j] = j < 2 ? act_low[j] : -1.0f;
        ab.hi[j] = j < 2 ? act_high[j] : 1.0f;
        if (!(ab.hi[j] > ab.lo[j])) return CSTR_E_BADARG;
    }
    // nothing the launch writes may overlap anything else it touches: state arrays, outputs, the ring and its side arrays
    const int64_t n = ring->n_envs, cells = ring->rows * n, words = (n + 63) >> 6;
    struct Span { const void *p; int64_t bytes; bool written; };
    const Span spans[] = {
        {policy_out, 8 * n, false}, {noise, 8 * n, false},
        {env_obs, 16 * n, true}, {rows, 24 * n, true}, {step_count, 4 * n, true}, {pcg_state, 32 * n, true}, {static_init, 32 * n, true},
        {target, 4 * n, true}, {episode, 4 * n, true}, {reward_out, 4 * n, true}, {done_out, 4 * n, true}, {timeout_out, 4 * n, true},
        {next_rows_out, 24 * n, true}, {ep_return, 4 * n, true}, {ep_stats, 32, true}, {ring_ctl, 32, true}, {policy_rng_ctl, 16, true},
        {ring->obs, 16 * cells, true}, {ring->next_obs, 16 * cells, true}, {ring->act, 8 * cells, true}, {ring->rew, 4 * cells, true},
        {ring->done, 4 * cells, true}, {ring->timeout, 4 * cells, true}, {her->desired_goal, 4 * cells, true}, {her->ep_start, 4 * cells, true},
        {her->ep_length, 4 * cells, true}, {her->cur_ep_start, 4 * n, true}, {her->row_valid, 4 * ring->rows, true},
        {her->valid_bits, 8 * ring->rows * words, true}};
    constexpr int n_spans = (int)(sizeof(spans) / sizeof(spans[0]));
    for (int i = 0; i < n_spans; ++i)
        for (int j = i + 1; j < n_spans; ++j)
            if (spans[i].p && spans[j].p && (spans[i].written || spans[j].written) &&
                spans_overlap(spans[i].p, spans[i].bytes, spans[j].p, spans[j].bytes))
                return CSTR_E_BADARG;
    GoalCollectArgs c;
    c.ring = *ring; c.her = *her;
    c.env_obs = env_obs; c.rows = rows; c.step_count = step_count; c.pcg = pcg_state; c.static_init = static_init; c.target = target;
    c.gd = GoalDraw{goal_seed, goal_index_offset, goal_lo, goal_hi, episode};
    c.squashed = squashed; c.ab = ab; c.noise = noise;
    c.reward_out = reward_out; c.done_out = done_out; c.timeout_out = timeout_out; c.next_rows_out = next_rows_out;
    c.ep_return = ep_return; c.ep_stats = ep_stats;
    int block, grid;
    env_launch_shape(n, block, grid);
    hipStream_t s = (hipStream_t)stream;
    if (integrator == CSTR_INTEGRATOR_EULER)
        goal_collect_step_kernel<CSTR_INTEGRATOR_EULER><<<grid, block, 0, s>>>(*coef, c, ring_ctl, policy_out, policy_rng_ctl, policy_rng_advance);
    else
        goal_collect_step_kernel<CSTR_INTEGRATOR_RK4><<<grid, block, 0, s>>>(*coef, c, ring_ctl, policy_out, policy_rng_ctl, policy_rng_advance);
    return (int)hipGetLastError();
}

extern "C" int cstr_her_sample_f32(const cstr_coef_t *coef, const cstr_ring_t *ring, const cstr_her_t *her, uint32_t *mt_state, int64_t batch,
                                   int64_t nb_virtual, int strategy, const int64_t *forced_row, const int64_t *forced_env,
                                   const int64_t *forced_goal, float *out_obs, float *out_act, float *out_next_obs, float *out_done,
                                   float *out_rew, int64_t *out_row_idx, int64_t *out_env_idx, int64_t *out_goal_row, int32_t *status,
                                   cstr_stream_t stream)
{
    const int rc = check_her(ring, her);
    if (rc) return rc;
    if (!coef || !mt_state || !out_obs || !out_act || !out_next_obs || !out_done || !out_rew || !status || batch <= 0) return CSTR_E_BADARG;
    if (nb_virtual < 0 || nb_virtual > batch) return CSTR_E_BADARG;
    if (strategy != CSTR_HER_FUTURE && strategy != CSTR_HER_FINAL && strategy != CSTR_HER_EPISODE) return CSTR_E_BADARG;
    if ((forced_row == nullptr) != (forced_env == nullptr) || (forced_goal && !forced_row)) return CSTR_E_BADARG;
    if (batch > CSTR_HER_MAX_BATCH) return CSTR_E_UNSUPPORTED;
    if (!aligned8(out_obs) || !aligned8(out_next_obs) || !aligned8(out_act) || !aligned4p(out_done) || !aligned4p(out_rew) || !aligned4p(mt_state) ||
        !aligned4p(status))
        return CSTR_E_BADARG;
    const void *outs[5] = {out_obs, out_next_obs, out_act, out_done, out_rew};
    const int64_t out_bytes[5] = {24 * batch, 24 * batch, 8 * batch, 4 * batch, 4 * batch};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (spans_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return CSTR_E_BADARG;
    HerSampleArgs a;
    a.ring = *ring; a.her = *her; a.mt_state = mt_state;
    a.batch = (int)batch; a.nb_virtual = (int)nb_virtual; a.strategy = strategy;
    a.s_lo2 = coef->s_lo[2]; a.s_span2 = coef->s_span[2]; a.conc_span = coef->conc_span;
    a.forced_row = forced_row; a.forced_env = forced_env; a.forced_goal = forced_goal;
    a.out_obs = out_obs; a.out_act = out_act; a.out_next_obs = out_next_obs; a.out_done = out_done; a.out_rew = out_rew;
    a.out_row_idx = out_row_idx; a.out_env_idx = out_env_idx; a.out_goal_row = out_goal_row; a.status = status;
    const size_t dyn = sizeof(int32_t) * ((size_t)ring->rows + 5 * (size_t)batch);
    her_sample_kernel<<<1, HER_TPB, dyn, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
