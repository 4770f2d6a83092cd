// cstr_eval.hip -- whole evaluation episodes in ONE launch for gfx950 (cstr_eval_episodes_f32, cstr_eval_goal_episodes_f32).
//
// evaluate_policy (core/common/evaluation.py:11-140) is a host loop: per vec-step the actor's launch, the env step, a few element-wise
// ops and two flags read back. Here a workgroup owns 16 envs and walks their vec-steps inside the launch:
//   policy network on the 16 observation rows (policy_layer of cstr_policy_device.h, the stages of cstr_policy_rows_fwd_f32: layer 1
//   and layer 2 on the f32 matrix cores, W2 streamed from L2 every step -- 256 x 256 f32 is 256 KB and does not fit in LDS -- as rows or
//   from the tile-major copy when the caller has one), the head in the summation order of the launch it stands for (below), predict()'s
//   post-processing, the env step (cstr_env_device.h), the episode accounting and the PCG64 reset draw of an env whose episode ended.
// Observations, activations and the head's partial sums live in LDS for the whole launch; a lane of wave 0 per env carries the
// running return (f64 sum of the f32 step rewards), the length and the episode count. Workgroups never exchange anything: no ticket, no
// hand-over, results leave through ordinary stores.
//
// Bit-level contract: for the counted episodes, ep_return / ep_len / ep_done and the env's pcg_state equal what the step-by-step
// launches give: cstr_policy_rows_fwd_f32 (head 0: with eps = 0, i.e. the squashed Gaussian at its mode), predict()'s post-processing,
// cstr_vec_step_f32 with the reset observations of cstr_reset_draw_f32. cstr_policy_rows_fwd_f32 has two head forms with different
// summation orders (per-lane partial dots + shuffle tree; split-K matrix-core tile when the tile-major W2 is given and the widths are
// <= 512): this kernel runs the one that launch would run for the same cstr_policy_mlp_t. Both sides of the contract are the same code:
// the layers (policy_layer), the two heads (policy_head_tree; split_k_head_chunk / _store / _out) and the host's choice between them
// (policy_runs_split_k_head) live in cstr_policy_device.h, the element arithmetic (sample_action_act at eps = 0, head_out_act) in
// cstr_gaussian_device.h, predict()'s unscale / clip (unscale_action, clip_keep_nan) in cstr_env_device.h.
// An env stops when it has met its target: its state after its last counted episode (the reset draw behind that episode included) is
// what the launch leaves; the host loop would keep stepping it until every env is done, which is NOT reproduced.
//
// cstr_eval_goal_episodes_f32 is the same kernel on the goal-conditioned face (GOAL instantiations): the network reads the flat row
// [achieved_goal | desired_goal | observation] (k0 = 6), the reward is goal_reward on the env's own setpoint, an episode's end redraws the
// setpoint from Philox exactly as cstr_goal_vec_step_f32 does, and three optional per-episode outputs carry the setpoint, the terminal
// gap and the f64 sum of |achieved - desired| -- the numbers a lane has in registers when its episode ends. Its contract is bit-level
// against cstr_policy_rows_fwd_f32 on the flat rows, predict()'s post-processing and cstr_goal_vec_step_f32.
//
// cstr_collect_episodes_f32 is the recording form on the (4, 2) layout (REC instantiations): no targets -- every env runs exactly n_steps
// vec-steps -- and each step leaves the replay-ring row cstr_collect_step_f32 would write (action_scale_chain on the head value, the
// stores of collect_env_lane), optionally with a uniform action drawn from Philox in place of the policy's (COLLECT_TAG). Its contract is
// bit-level against cstr_policy_rows_fwd_f32, the draw's statement in the header and cstr_collect_step_f32.
//
// Termination: the loop over vec-steps is bounded by max_vec_steps whatever the data does; it ends earlier once the workgroup's 16 envs
// have met their targets (REC: the trip count is n_steps, fixed).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cstr_rl_hip.h"
#include "cstr_device.h"
#include "cstr_env_device.h"
#include "cstr_goal_device.h"
#include "cstr_policy_device.h"

namespace {

// k chunks of layer 2 whose operands a wave requests at once (the accumulation order does not depend on it): 8 keeps the kernel, which
// also holds the env lanes' episode state, inside its register budget (200 VGPRs; the goal instantiations, whose env lanes also hold the
// setpoint, the episode ordinal and the gap sum, 216; no scratch in either: profiles/goal_eval_kernel_resources.txt)
constexpr int EVAL_UNROLL = 8;

struct EvalArgs {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w2s;
    int k0, h1, h2, act_dim, out_act, split_k_head;
    cstr_coef_t k;
    float *env_obs; int32_t *step_count; uint64_t *pcg; double *static_init;
    int squashed, integrator; ActBounds ab;
    double *ep_return; int32_t *ep_len, *ep_done;  // ep_done: targets on entry, episodes counted on exit
    int64_t ep_stride, n, max_vec_steps;
};

// the goal face (cstr_eval_goal_episodes_f32): the Box arguments, then the per-env setpoints, their redraw and the tracking outputs
struct GoalEvalArgs : EvalArgs {
    float *target; GoalDraw gd;
    float *ep_goal, *ep_gap; double *ep_abs_gap;  // each optional
};

// the recording form (cstr_collect_episodes_f32): the Box arguments (max_vec_steps = n_steps, ep_done written only), then the ring rows the
// launch fills and the exploration stream
struct CollectEpArgs : EvalArgs {
    cstr_ring_t ring; int64_t row0;
    float explore_prob; uint64_t seed; int64_t index_offset; uint32_t step_offset;
    uint8_t *explored;  // optional, [ring rows][n_envs]
};

template <bool GOAL, bool REC = false> struct EvalArgsOf { using type = EvalArgs; };
template <> struct EvalArgsOf<true, false> { using type = GoalEvalArgs; };
template <> struct EvalArgsOf<false, true> { using type = CollectEpArgs; };

constexpr uint32_t COLLECT_TAG = 0xC011EC7Du;  // counter word 3 of the exploration draw: shares no counters with the other streams

// GOAL = false: the Box faces, L = the env layout. GOAL = true (L = 0): the network reads the flat row [achieved | desired | observation]
// (k0 = 6; the env state is columns 2..5 of the LDS row), the reward is goal_reward on the lane's own setpoint, and an episode's end
// redraws the setpoint as cstr_goal_vec_step_f32 does.
// REC = true (GOAL = false, L = 0; cstr_collect_episodes_f32): every env runs exactly max_vec_steps vec-steps -- no targets, no early end --
// and each of them leaves ring row row0 + t with the stores of collect_env_lane; the deterministic head value may be replaced by a
// uniform draw over the action space (explore_prob) and goes through the collect step's action_scale_chain.
template <int ACT, int HEAD, int L, bool GOAL = false, bool REC = false>
__global__ __launch_bounds__(64 * POLICY_WAVES) void eval_episodes_kernel(const typename EvalArgsOf<GOAL, REC>::type a)
{
    static_assert(!GOAL || L == 0, "the goal face is the (4, 2) layout");
    static_assert(!REC || (!GOAL && L == 0), "the recording form is the Box face's (4, 2) layout");
    constexpr int D = Lay<L>::D, A = Lay<L>::A, XS = 8;  // XS: row stride of the observation image
    constexpr int X0 = GOAL ? 2 : 0;                     // column of the env state in a row of the image
    extern __shared__ float eval_lds[];
    __shared__ int go_s;
    const int H1 = a.h1, H2 = a.h2, kc1 = (H1 + 15) >> 4, kc2 = (H2 + 15) >> 4, S1 = 16 * kc1 + 4, S2 = 16 * kc2 + 4;
    float *h1s = eval_lds, *h2s = h1s + POLICY_ROWS * S1, *part = h2s + POLICY_ROWS * S2;  // part [8 waves][16 rows][8]
    float *ps = part + POLICY_WAVES * POLICY_ROWS * 8, *xs = ps + POLICY_ROWS * 8;         // head outputs [16][8], observations [16][XS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * POLICY_ROWS;
    const int n_out = HEAD == 0 ? 2 * A : A;

    // the env lanes: lane e < 16 of wave 0 owns env m0 + e for the whole launch
    const int64_t env = m0 + lane;
    const bool env_lane = wave == 0 && lane < POLICY_ROWS && env < a.n;
    int32_t target = 0, count = 0, cur_len = 0, st = 0;
    double cur_ret = 0.0;
    float tg = 0.0f, dg = 0.0f;  // GOAL: the env's raw setpoint and its desired_goal, constant within an episode
    int32_t ordinal = 0;         // GOAL: ordinal of the env's next episode (the redraw's counter word)
    double abs_gap = 0.0;        // GOAL: f64 sum of |achieved - desired| over the episode's next rows
    if (tid < POLICY_ROWS * XS) xs[tid] = 0.0f;  // rows past n_envs and columns past obs_dim stay zero
    {   // zero the k padding of both activation images (widths that are not multiples of 16: the split-K head reads whole chunks)
        const int p1 = 16 * kc1 - H1, p2 = 16 * kc2 - H2;
        if (p1 > 0 && tid < POLICY_ROWS * p1) h1s[(tid / max(p1, 1)) * S1 + H1 + tid % max(p1, 1)] = 0.0f;
        if (p2 > 0 && tid < POLICY_ROWS * p2) h2s[(tid / max(p2, 1)) * S2 + H2 + tid % max(p2, 1)] = 0.0f;
    }
    __syncthreads();
    if (env_lane) {
        float o[2][4];
        load_obs<L>(a.env_obs, env, o);
#pragma unroll
        for (int j = 0; j < D; ++j) xs[lane * XS + X0 + j] = o[j >> 2][j & 3];
        st = a.step_count[env];
        if constexpr (!REC) target = a.ep_done[env];
        if constexpr (GOAL) {
            tg = a.target[env];
            dg = goal_of_target(a.k, tg);
            if (a.gd.episode) ordinal = a.gd.episode[env];
            xs[lane * XS + 0] = o[0][2];  // achieved_goal = observation[2]
            xs[lane * XS + 1] = dg;
        }
    }
    if constexpr (!REC) {
        if (wave == 0) {
            const unsigned long long any = __ballot(env_lane && count < target);
            if (lane == 0) go_s = any != 0ull;
        }
    }
    __syncthreads();

    for (int64_t it = 0; it < a.max_vec_steps; ++it) {
        if constexpr (!REC) {
            if (!go_s) break;  // workgroup-uniform: written before the barrier that ends the previous trip
        }
        // ---- the policy network on the 16 observation rows (the stages of cstr_policy_rows_fwd_f32) ----
        // k0 <= 8: one k chunk. GOAL: W1's rows are 6 floats (24 bytes), so its operand loads are per element, bounded by k0 -- the
        // first-layer staging cstr_policy_rows_fwd_f32 takes for k0 = 6 (no 16-byte loads); columns 6, 7 of the image are zero
        policy_layer<ACT, false, !GOAL, false, 1>(xs, XS, true, a.k0, a.w1, a.b1, H1, h1s, S1);
        __syncthreads();
        if (a.w2s) policy_layer<ACT, false, true, true, EVAL_UNROLL>(h1s, S1, true, H1, a.w2s, a.b2, H2, h2s, S2);
        else policy_layer<ACT, false, true, false, EVAL_UNROLL>(h1s, S1, true, H1, a.w2, a.b2, H2, h2s, S2);
        __syncthreads();
        if (a.split_k_head) {
            // the split-K tile of the pipelined policy kernel (cstr_policy_device.h); here the w3 quads are loaded in the loop
            f32x4 p0 = {0.0f, 0.0f, 0.0f, 0.0f}, p1 = p0;
            const float *hr = h2s + r * S2 + 4 * h;
            const float *w3r = a.w3 + (int64_t)min(r, n_out - 1) * H2;
            for (int c = wave; c < kc2; c += POLICY_WAVES)
                split_k_head_chunk(hr + 16 * c, load_k4_clamped<true>(w3r, 16 * c + 4 * h, H2, r < n_out), p0, p1);
            split_k_head_store(part, p0 + p1);
            __syncthreads();
            if (tid < POLICY_ROWS * 8 && (tid & 7) < n_out)  // thread = 8 * row + output slot
                ps[tid] = split_k_head_out(part, tid >> 3, tid & 7, a.b3[tid & 7]);
        } else {
            policy_head_tree<POLICY_ROWS / POLICY_WAVES>(h2s, S2, H2, a.w3, a.b3, n_out, ps, wave, lane);  // the first policy kernel's head
        }
        __syncthreads();

        // ---- predict()'s post-processing, env step, episode accounting, reset draw: a lane per env ----
        const bool active = REC ? env_lane : (env_lane && count < target);
        if (active) {
            const float *pr = ps + lane * 8;
            float ea[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            float sa[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // REC: the buffer action
            uint32_t xw[4] = {0u, 0u, 0u, 0u};       // REC: the step's Philox block (word 0: the flag, words 1..A: the uniform action)
            bool explore = false;
            if constexpr (REC) {
                if (a.explore_prob > 0.0f) {
                    const uint64_t idx = (uint64_t)(a.index_offset + env);
                    philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), a.step_offset + (uint32_t)it, COLLECT_TAG, (uint32_t)a.seed,
                                  (uint32_t)(a.seed >> 32), xw);
                    explore = philox_uniform(xw[0]) < a.explore_prob;
                }
            }
#pragma unroll
            for (int j = 0; j < A; ++j) {
                float v, sd, u;
                if (HEAD == 1) v = head_out_act(pr[j], a.out_act);
                else sample_action_act(pr[j], pr[A + j], 0.0f, v, sd, u);  // the squashed Gaussian at its mode: what eps = 0 gives
                const float lo = a.ab.lo[j], hi = a.ab.hi[j];
                if constexpr (REC) {
                    if (explore) {  // a uniform draw over the action space in place of the head value (the TU is built without contraction)
                        const float uj = philox_uniform(xw[1 + j]);
                        v = (a.squashed & 1) ? 2.0f * uj - 1.0f : lo + uj * (hi - lo);
                    }
                    if (!(a.squashed & 1)) v = clip_keep_nan(v, lo, hi);        // predict()'s clip (policies.py:386)
                    action_scale_chain(a.squashed, lo, hi, v, false, 0.0f, sa[j], ea[j]);  // the statement of cstr_collect_step_f32
                } else {
                    ea[j] = (a.squashed & 1) ? unscale_action(v, lo, hi) : clip_keep_nan(v, lo, hi);  // policies.py:375, :413 | :386
                }
            }
            float o[2][4], on[2][4], rew;
#pragma unroll
            for (int j = 0; j < (GOAL ? 4 : 8); ++j) o[j >> 2][j & 3] = xs[lane * XS + X0 + j];
            bool bad = false;
            if constexpr (GOAL) {  // goal_step_kernel's own NaN test: the goal reward does not replace the NaN path's -10
                bad = (ea[0] != ea[0]) || (ea[1] != ea[1]);
#pragma unroll
                for (int j = 0; j < 4; ++j) bad |= (o[0][j] != o[0][j]);
            }
            const bool done = a.integrator == CSTR_INTEGRATOR_EULER ? env_step_lane<L, CSTR_INTEGRATOR_EULER>(a.k, o, ea, st, on, rew)
                                                                    : env_step_lane<L, CSTR_INTEGRATOR_RK4>(a.k, o, ea, st, on, rew);
            float gap = 0.0f;
            if constexpr (GOAL) {  // the next row's columns 0, 1: achieved goal of the next state, the OLD desired goal
                if (!bad) rew = goal_reward(a.k.s_lo[2], a.k.s_span[2], a.k.conc_span, on[0][2], dg);
                gap = on[0][2] - dg;
                abs_gap += (double)fabsf(gap);
            }
            if constexpr (REC) {  // ring row row0 + it: obs = the observation before the step, next_obs = the terminal one (collect_env_lane)
                const int64_t e = (a.row0 + it) * a.n + env;
                store_ring_obs<L>(a.ring.obs, e, o);
                store_ring_obs<L>(a.ring.next_obs, e, on);
                store_ring_act<A>(a.ring.act, e, sa);
                store_ring_f32(a.ring.rew, e, rew);
                store_ring_f32(a.ring.done, e, done ? 1.0f : 0.0f);
                store_ring_f32(a.ring.timeout, e, done ? 1.0f : 0.0f);
                if (a.explored) a.explored[e] = explore ? 1 : 0;
            }
            cur_ret += (double)rew;  // current_rewards: float64 (evaluation.py:84, :97)
            cur_len += 1;
            if (done) {
                if (!REC || count < a.ep_stride) {  // REC: episodes beyond ep_stride are counted, not stored
                    a.ep_return[env * a.ep_stride + count] = cur_ret;
                    a.ep_len[env * a.ep_stride + count] = cur_len;
                }
                if constexpr (GOAL) {
                    if (a.ep_goal) a.ep_goal[env * a.ep_stride + count] = dg;
                    if (a.ep_gap) a.ep_gap[env * a.ep_stride + count] = gap;
                    if (a.ep_abs_gap) a.ep_abs_gap[env * a.ep_stride + count] = abs_gap;
                    abs_gap = 0.0;
                }
                count += 1;
                cur_ret = 0.0;
                cur_len = 0;
                uint64_t pst[4];  // auto-reset (dummy_vec_env.py:68-72)
                load_pcg(a.pcg, env, pst);
                reset_draw_env<L>(a.k, pst, a.static_init, env, on);
                *reinterpret_cast<ulonglong2 *>(a.pcg + 4 * env) = make_ulonglong2(pst[0], pst[1]);
                st = 0;
                if constexpr (GOAL) {
                    if (a.gd.episode) {  // the setpoint of the episode that starts now
                        tg = goal_draw_target(a.gd, env, ordinal);
                        ordinal += 1;
                        dg = goal_of_target(a.k, tg);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) xs[lane * XS + X0 + j] = on[j >> 2][j & 3];
            if constexpr (GOAL) {
                xs[lane * XS + 0] = on[0][2];
                xs[lane * XS + 1] = dg;
            }
        }
        if constexpr (!REC) {
            if (wave == 0) {
                const unsigned long long any = __ballot(env_lane && count < target);
                if (lane == 0) go_s = any != 0ull;
            }
        }
        __syncthreads();
    }

    if (env_lane) {
        float o[2][4];
#pragma unroll
        for (int j = 0; j < (GOAL ? 4 : 8); ++j) o[j >> 2][j & 3] = xs[lane * XS + X0 + j];
        store_obs<L>(a.env_obs, env, o);
        a.step_count[env] = st;
        a.ep_done[env] = count;
        if constexpr (GOAL) {
            a.target[env] = tg;
            if (a.gd.episode) a.gd.episode[env] = ordinal;
        }
    }
}

struct Span { const char *lo, *hi; };

static inline Span span_of(const void *p, int64_t bytes) { return Span{static_cast<const char *>(p), static_cast<const char *>(p) + bytes}; }
static inline bool overlaps(const Span &x, const Span &y) { return x.lo && y.lo && x.lo < y.hi && y.lo < x.hi; }

}  // namespace

static size_t eval_lds_bytes(const cstr_policy_mlp_t &n)
{
    const int kc1 = (n.h1 + 15) / 16, kc2 = (n.h2 + 15) / 16;
    return (size_t)(POLICY_ROWS * (16 * kc1 + 4 + 16 * kc2 + 4) + POLICY_WAVES * POLICY_ROWS * 8 + 2 * POLICY_ROWS * 8) * sizeof(float);
}

extern "C" int cstr_eval_episodes_f32(const cstr_policy_mlp_t *net, const cstr_coef_t *coef, int integrator, int obs_dim, float *env_obs,
                                      int32_t *step_count, uint64_t *pcg_state, double *static_init, int squashed, const float *act_low,
                                      const float *act_high, const int32_t *targets, int64_t n_envs, int64_t max_vec_steps,
                                      double *ep_return, int32_t *ep_len, int32_t *ep_done, cstr_stream_t stream)
{
    if (!net || !coef || !env_obs || !step_count || !pcg_state || !act_low || !act_high || !targets || !ep_done) return CSTR_E_BADARG;
    if (n_envs <= 0 || max_vec_steps <= 0 || (squashed & ~1)) return CSTR_E_BADARG;
    const cstr_policy_mlp_t &n = *net;
    if (!n.w1 || !n.b1 || !n.w2 || !n.b2 || !n.w3 || !n.b3 || n.k0 <= 0 || n.h1 <= 0 || n.h2 <= 0 || n.act_dim <= 0 || n.reserved) return CSTR_E_BADARG;
    const int lay = layout_of(obs_dim, n.act_dim);
    if (lay < 0 || (integrator != CSTR_INTEGRATOR_EULER && integrator != CSTR_INTEGRATOR_RK4)) return CSTR_E_UNSUPPORTED;
    if (n.k0 != obs_dim) return CSTR_E_BADARG;  // the policy reads the env's observation rows
    // the shapes of cstr_policy_rows_fwd_f32
    if (n.act < 0 || n.act > 2 || n.out_act < 0 || n.out_act > 2 || n.head < 0 || n.head > 1 || (n.h1 & 3) || (n.h2 & 3) ||
        (size_t)POLICY_ROWS * (n.h1 + 4 + n.h2 + 4) * sizeof(float) > 64 * 1024 || eval_lds_bytes(n) > 64 * 1024 ||
        (n_envs + POLICY_ROWS - 1) / POLICY_ROWS > 0x7fffffff)
        return CSTR_E_UNSUPPORTED;
    if (!aligned16(env_obs) || !aligned16(pcg_state) || !aligned16(n.w1) || !aligned16(n.w2) || !aligned16(n.w3) ||
        (n.w2_swizzled && !aligned16(n.w2_swizzled)) || !aligned8(ep_return) || (static_init && !aligned8(static_init)) ||
        (reinterpret_cast<uintptr_t>(step_count) & 3u) || (reinterpret_cast<uintptr_t>(ep_len) & 3u) || (reinterpret_cast<uintptr_t>(ep_done) & 3u))
        return CSTR_E_BADARG;
    const int A = n.act_dim;
    ActBounds ab;
    for (int j = 0; j < 4; ++j) {
        ab.lo[j] = j < A ? act_low[j] : -1.0f;
        ab.hi[j] = j < A ? act_high[j] : 1.0f;
        if (!(ab.hi[j] > ab.lo[j])) return CSTR_E_BADARG;
    }
    int64_t ep_stride = 0;  // targets is a HOST array (like act_low / act_high): checked here, staged into ep_done below
    for (int64_t i = 0; i < n_envs; ++i) {
        if (targets[i] < 0) return CSTR_E_BADARG;
        if (targets[i] > ep_stride) ep_stride = targets[i];
    }
    if (ep_stride > 0 && (!ep_return || !ep_len)) return CSTR_E_BADARG;  // (no slot exists when every target is 0)
    if (ep_stride > 0 && n_envs > INT64_MAX / (8 * ep_stride)) return CSTR_E_UNSUPPORTED;
    {   // outputs must not overlap what the launch reads, or each other
        const int TR = lay == 2 ? 2 : 1, n_out = (n.head == 0 ? 2 : 1) * A, kc1 = (n.h1 + 15) / 16, kc2 = (n.h2 + 15) / 16;
        const Span outs[3] = {span_of(ep_return, 8 * n_envs * ep_stride), span_of(ep_len, 4 * n_envs * ep_stride), span_of(ep_done, 4 * n_envs)};
        const Span ins[11] = {span_of(env_obs, 4 * n_envs * obs_dim), span_of(step_count, 4 * n_envs), span_of(pcg_state, 32 * n_envs),
                              span_of(static_init, 32 * TR * n_envs), span_of(n.w1, 4LL * n.h1 * n.k0), span_of(n.b1, 4LL * n.h1),
                              span_of(n.w2, 4LL * n.h2 * n.h1), span_of(n.b2, 4LL * n.h2), span_of(n.w3, 4LL * n_out * n.h2),
                              span_of(n.b3, 4LL * n_out), span_of(n.w2_swizzled, 1024LL * kc1 * kc2)};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 11; ++j)
                if (overlaps(outs[i], ins[j])) return CSTR_E_BADARG;
            for (int j = i + 1; j < 3; ++j)
                if (overlaps(outs[i], outs[j])) return CSTR_E_BADARG;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const hipError_t cp = hipMemcpyAsync(ep_done, targets, sizeof(int32_t) * (size_t)n_envs, hipMemcpyHostToDevice, s);
    if (cp != hipSuccess) return (int)cp;
    if (ep_stride == 0) return CSTR_OK;  // nothing to run: ep_done = targets = 0
    EvalArgs a = {n.w1, n.b1, n.w2, n.b2, n.w3, n.b3, n.w2_swizzled, n.k0, n.h1, n.h2, A, n.out_act, policy_runs_split_k_head(n) ? 1 : 0, *coef,
                  env_obs, step_count, pcg_state, static_init, squashed, integrator, ab, ep_return, ep_len, ep_done, ep_stride, n_envs, max_vec_steps};
    const unsigned grid = (unsigned)((n_envs + POLICY_ROWS - 1) / POLICY_ROWS);
    const size_t lds = eval_lds_bytes(n);
#define EV3(A_, H_, L_) eval_episodes_kernel<A_, H_, L_><<<grid, 64 * POLICY_WAVES, lds, s>>>(a)
#define EV2(A_, H_) do { if (lay == 0) EV3(A_, H_, 0); else if (lay == 1) EV3(A_, H_, 1); else EV3(A_, H_, 2); } while (0)
    if (n.head == 0) { if (n.act == 0) EV2(0, 0); else if (n.act == 1) EV2(1, 0); else EV2(2, 0); }
    else { if (n.act == 0) EV2(0, 1); else if (n.act == 1) EV2(1, 1); else EV2(2, 1); }
#undef EV2
#undef EV3
    return (int)hipGetLastError();
}

extern "C" int cstr_eval_goal_episodes_f32(const cstr_policy_mlp_t *net, const cstr_coef_t *coef, int integrator, float *env_obs,
                                           int32_t *step_count, uint64_t *pcg_state, double *static_init, float *target, int32_t *episode,
                                           uint64_t goal_seed, int64_t goal_index_offset, float goal_lo, float goal_hi, int squashed,
                                           const float *act_low, const float *act_high, const int32_t *targets, int64_t n_envs,
                                           int64_t max_vec_steps, double *ep_return, int32_t *ep_len, int32_t *ep_done, float *ep_goal,
                                           float *ep_gap, double *ep_abs_gap, cstr_stream_t stream)
{
    constexpr int K0 = 6;  // the flat row [achieved_goal | desired_goal | observation]
    if (!net || !coef || !env_obs || !step_count || !pcg_state || !target || !act_low || !act_high || !targets || !ep_done) return CSTR_E_BADARG;
    if (n_envs <= 0 || max_vec_steps <= 0 || (squashed & ~1)) return CSTR_E_BADARG;
    const cstr_policy_mlp_t &n = *net;
    if (!n.w1 || !n.b1 || !n.w2 || !n.b2 || !n.w3 || !n.b3 || n.k0 <= 0 || n.h1 <= 0 || n.h2 <= 0 || n.act_dim <= 0 || n.reserved) return CSTR_E_BADARG;
    if (n.act_dim != 2 || (integrator != CSTR_INTEGRATOR_EULER && integrator != CSTR_INTEGRATOR_RK4)) return CSTR_E_UNSUPPORTED;
    if (n.k0 != K0) return CSTR_E_BADARG;  // the policy reads the goal face's flat rows
    if (episode && !(goal_lo <= goal_hi)) return CSTR_E_BADARG;
    // the shapes of cstr_policy_rows_fwd_f32
    if (n.act < 0 || n.act > 2 || n.out_act < 0 || n.out_act > 2 || n.head < 0 || n.head > 1 || (n.h1 & 3) || (n.h2 & 3) ||
        (size_t)POLICY_ROWS * (n.h1 + 4 + n.h2 + 4) * sizeof(float) > 64 * 1024 || eval_lds_bytes(n) > 64 * 1024 ||
        (n_envs + POLICY_ROWS - 1) / POLICY_ROWS > 0x7fffffff)
        return CSTR_E_UNSUPPORTED;
    const auto aligned4 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; };
    if (!aligned16(env_obs) || !aligned16(pcg_state) || !aligned4(n.w1) || !aligned16(n.w2) || !aligned16(n.w3) ||
        (n.w2_swizzled && !aligned16(n.w2_swizzled)) || !aligned8(ep_return) || !aligned8(ep_abs_gap) || (static_init && !aligned8(static_init)) ||
        !aligned4(step_count) || !aligned4(target) || !aligned4(episode) || !aligned4(ep_len) || !aligned4(ep_done) || !aligned4(ep_goal) ||
        !aligned4(ep_gap))
        return CSTR_E_BADARG;
    ActBounds ab;
    for (int j = 0; j < 4; ++j) {
        ab.lo[j] = j < 2 ? act_low[j] : -1.0f;
        ab.hi[j] = j < 2 ? act_high[j] : 1.0f;
        if (!(ab.hi[j] > ab.lo[j])) return CSTR_E_BADARG;
    }
    int64_t ep_stride = 0;  // targets is a HOST array (like act_low / act_high): checked here, staged into ep_done below
    for (int64_t i = 0; i < n_envs; ++i) {
        if (targets[i] < 0) return CSTR_E_BADARG;
        if (targets[i] > ep_stride) ep_stride = targets[i];
    }
    if (ep_stride > 0 && (!ep_return || !ep_len)) return CSTR_E_BADARG;  // (no slot exists when every target is 0)
    if (ep_stride > 0 && n_envs > INT64_MAX / (8 * ep_stride)) return CSTR_E_UNSUPPORTED;
    {   // outputs must not overlap what the launch reads, or each other
        const int n_out = (n.head == 0 ? 2 : 1) * 2, kc1 = (n.h1 + 15) / 16, kc2 = (n.h2 + 15) / 16;
        const int64_t slots = n_envs * ep_stride;
        const Span outs[6] = {span_of(ep_return, 8 * slots), span_of(ep_len, 4 * slots), span_of(ep_done, 4 * n_envs),
                              span_of(ep_goal, 4 * slots), span_of(ep_gap, 4 * slots), span_of(ep_abs_gap, 8 * slots)};
        const Span ins[13] = {span_of(env_obs, 16 * n_envs), span_of(step_count, 4 * n_envs), span_of(pcg_state, 32 * n_envs),
                              span_of(static_init, 32 * n_envs), span_of(target, 4 * n_envs), span_of(episode, 4 * n_envs),
                              span_of(n.w1, 4LL * n.h1 * K0), span_of(n.b1, 4LL * n.h1), span_of(n.w2, 4LL * n.h2 * n.h1),
                              span_of(n.b2, 4LL * n.h2), span_of(n.w3, 4LL * n_out * n.h2), span_of(n.b3, 4LL * n_out),
                              span_of(n.w2_swizzled, 1024LL * kc1 * kc2)};
        for (int i = 0; i < 6; ++i) {
            for (int j = 0; j < 13; ++j)
                if (overlaps(outs[i], ins[j])) return CSTR_E_BADARG;
            for (int j = i + 1; j < 6; ++j)
                if (overlaps(outs[i], outs[j])) return CSTR_E_BADARG;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const hipError_t cp = hipMemcpyAsync(ep_done, targets, sizeof(int32_t) * (size_t)n_envs, hipMemcpyHostToDevice, s);
    if (cp != hipSuccess) return (int)cp;
    if (ep_stride == 0) return CSTR_OK;  // nothing to run: ep_done = targets = 0
    GoalEvalArgs a;
    static_cast<EvalArgs &>(a) = EvalArgs{n.w1, n.b1, n.w2, n.b2, n.w3, n.b3, n.w2_swizzled, n.k0, n.h1, n.h2, 2, n.out_act, policy_runs_split_k_head(n) ? 1 : 0,
                                          *coef, env_obs, step_count, pcg_state, static_init, squashed, integrator, ab, ep_return, ep_len, ep_done,
                                          ep_stride, n_envs, max_vec_steps};
    a.target = target;
    a.gd = GoalDraw{goal_seed, goal_index_offset, goal_lo, goal_hi, episode};
    a.ep_goal = ep_goal; a.ep_gap = ep_gap; a.ep_abs_gap = ep_abs_gap;
    const unsigned grid = (unsigned)((n_envs + POLICY_ROWS - 1) / POLICY_ROWS);
    const size_t lds = eval_lds_bytes(n);
#define EVG(A_, H_) eval_episodes_kernel<A_, H_, 0, true><<<grid, 64 * POLICY_WAVES, lds, s>>>(a)
    if (n.head == 0) { if (n.act == 0) EVG(0, 0); else if (n.act == 1) EVG(1, 0); else EVG(2, 0); }
    else { if (n.act == 0) EVG(0, 1); else if (n.act == 1) EVG(1, 1); else EVG(2, 1); }
#undef EVG
    return (int)hipGetLastError();
}

extern "C" int cstr_collect_episodes_f32(const cstr_policy_mlp_t *net, const cstr_coef_t *coef, int integrator, int obs_dim, float *env_obs,
                                         int32_t *step_count, uint64_t *pcg_state, double *static_init, int squashed, const float *act_low,
                                         const float *act_high, const cstr_ring_t *ring, int64_t row0, int64_t n_envs, int64_t n_steps,
                                         float explore_prob, uint64_t seed, int64_t index_offset, int64_t step_offset, double *ep_return,
                                         int32_t *ep_len, int64_t ep_stride, int32_t *ep_done, uint8_t *explored, cstr_stream_t stream)
{
    if (!net || !coef || !env_obs || !step_count || !pcg_state || !act_low || !act_high || !ring || !ep_done) return CSTR_E_BADARG;
    if (n_envs <= 0 || n_steps <= 0 || (squashed & ~1)) return CSTR_E_BADARG;
    const cstr_policy_mlp_t &n = *net;
    if (!n.w1 || !n.b1 || !n.w2 || !n.b2 || !n.w3 || !n.b3 || n.k0 <= 0 || n.h1 <= 0 || n.h2 <= 0 || n.act_dim <= 0 || n.reserved) return CSTR_E_BADARG;
    const cstr_ring_t &rg = *ring;
    if (!rg.obs || !rg.next_obs || !rg.act || !rg.rew || !rg.done || !rg.timeout || rg.rows <= 0) return CSTR_E_BADARG;
    if (layout_of(obs_dim, n.act_dim) < 0 || (integrator != CSTR_INTEGRATOR_EULER && integrator != CSTR_INTEGRATOR_RK4)) return CSTR_E_UNSUPPORTED;
    if (n.k0 != obs_dim) return CSTR_E_BADARG;  // the policy reads the env's observation rows
    if (rg.n_envs != n_envs || rg.obs_dim != obs_dim || rg.act_dim != n.act_dim) return CSTR_E_BADARG;  // the ring is this env's
    if (layout_of(obs_dim, n.act_dim) != 0) return CSTR_E_UNSUPPORTED;  // the recording form exists for the (4, 2) layout
    if (row0 < 0 || n_steps > rg.rows || row0 > rg.rows - n_steps) return CSTR_E_BADARG;
    if (!(explore_prob >= 0.0f && explore_prob <= 1.0f)) return CSTR_E_BADARG;  // NaN included
    if (step_offset < 0 || n_steps > (int64_t)1 << 32 || step_offset > ((int64_t)1 << 32) - n_steps) return CSTR_E_BADARG;  // counter word 2
    if (ep_stride < 0 || (ep_stride > 0 && (!ep_return || !ep_len))) return CSTR_E_BADARG;
    // the shapes of cstr_policy_rows_fwd_f32
    if (n.act < 0 || n.act > 2 || n.out_act < 0 || n.out_act > 2 || n.head < 0 || n.head > 1 || (n.h1 & 3) || (n.h2 & 3) ||
        (size_t)POLICY_ROWS * (n.h1 + 4 + n.h2 + 4) * sizeof(float) > 64 * 1024 || eval_lds_bytes(n) > 64 * 1024 ||
        (n_envs + POLICY_ROWS - 1) / POLICY_ROWS > 0x7fffffff)
        return CSTR_E_UNSUPPORTED;
    if (rg.rows > INT64_MAX / (64 * n_envs) || (ep_stride > 0 && n_envs > INT64_MAX / (8 * ep_stride))) return CSTR_E_UNSUPPORTED;  // byte extents
    const auto aligned4 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; };
    if (!aligned16(env_obs) || !aligned16(pcg_state) || !aligned16(n.w1) || !aligned16(n.w2) || !aligned16(n.w3) ||
        (n.w2_swizzled && !aligned16(n.w2_swizzled)) || !aligned8(ep_return) || (static_init && !aligned8(static_init)) ||
        !aligned4(step_count) || !aligned4(ep_len) || !aligned4(ep_done) || !aligned16(rg.obs) || !aligned16(rg.next_obs) || !aligned8(rg.act) ||
        !aligned4(rg.rew) || !aligned4(rg.done) || !aligned4(rg.timeout))
        return CSTR_E_BADARG;
    constexpr int A = 2, D = 4;
    ActBounds ab;
    for (int j = 0; j < 4; ++j) {
        ab.lo[j] = j < A ? act_low[j] : -1.0f;
        ab.hi[j] = j < A ? act_high[j] : 1.0f;
        if (!(ab.hi[j] > ab.lo[j])) return CSTR_E_BADARG;
    }
    {   // nothing the launch writes may overlap anything it reads or anything else it writes (the env state is read and written)
        const int n_out = (n.head == 0 ? 2 : 1) * A, kc1 = (n.h1 + 15) / 16, kc2 = (n.h2 + 15) / 16;
        const int64_t cells = rg.rows * n_envs, slots = n_envs * ep_stride;
        constexpr int NW = 14, NR = 7;
        const Span wr[NW] = {span_of(rg.obs, 4 * D * cells), span_of(rg.next_obs, 4 * D * cells), span_of(rg.act, 4 * A * cells),
                             span_of(rg.rew, 4 * cells), span_of(rg.done, 4 * cells), span_of(rg.timeout, 4 * cells), span_of(explored, cells),
                             span_of(ep_return, 8 * slots), span_of(ep_len, 4 * slots), span_of(ep_done, 4 * n_envs),
                             span_of(env_obs, 4 * D * n_envs), span_of(step_count, 4 * n_envs), span_of(pcg_state, 32 * n_envs),
                             span_of(static_init, 32 * n_envs)};
        const Span rd[NR] = {span_of(n.w1, 4LL * n.h1 * n.k0), span_of(n.b1, 4LL * n.h1), span_of(n.w2, 4LL * n.h2 * n.h1), span_of(n.b2, 4LL * n.h2),
                             span_of(n.w3, 4LL * n_out * n.h2), span_of(n.b3, 4LL * n_out), span_of(n.w2_swizzled, 1024LL * kc1 * kc2)};
        for (int i = 0; i < NW; ++i) {
            for (int j = 0; j < NR; ++j)
                if (overlaps(wr[i], rd[j])) return CSTR_E_BADARG;
            for (int j = i + 1; j < NW; ++j)
                if (overlaps(wr[i], wr[j])) return CSTR_E_BADARG;
        }
    }
    CollectEpArgs a;
    static_cast<EvalArgs &>(a) = EvalArgs{n.w1, n.b1, n.w2, n.b2, n.w3, n.b3, n.w2_swizzled, n.k0, n.h1, n.h2, A, n.out_act, policy_runs_split_k_head(n) ? 1 : 0,
                                          *coef, env_obs, step_count, pcg_state, static_init, squashed, integrator, ab, ep_return, ep_len, ep_done,
                                          ep_stride, n_envs, n_steps};
    a.ring = rg; a.row0 = row0;
    a.explore_prob = explore_prob; a.seed = seed; a.index_offset = index_offset; a.step_offset = (uint32_t)step_offset;
    a.explored = explored;
    const unsigned grid = (unsigned)((n_envs + POLICY_ROWS - 1) / POLICY_ROWS);
    const size_t lds = eval_lds_bytes(n);
    hipStream_t s = (hipStream_t)stream;
#define EVR(A_, H_) eval_episodes_kernel<A_, H_, 0, false, true><<<grid, 64 * POLICY_WAVES, lds, s>>>(a)
    if (n.head == 0) { if (n.act == 0) EVR(0, 0); else if (n.act == 1) EVR(1, 0); else EVR(2, 0); }
    else { if (n.act == 0) EVR(0, 1); else if (n.act == 1) EVR(1, 1); else EVR(2, 1); }
#undef EVR
    return (int)hipGetLastError();
}
