/*
 * include/cstr_rl_hip.h -- C ABI of libcstr_rl_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the hot path of CHAINNEVERLIU/Pytorch-RL-EnhancedStableBaselines named by
 * BASELINE.json:north_star: core.{SAC,TD3,MADDPG}("MlpPolicy", env).learn() on the two-series
 * CSTR environment. The reference is 100 % Python and has no FFI of its own, so
 * each entry point below names the Python statements it replaces (file:line relative to the
 * reference root). INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (HBM) + sizes; no torch / C++ types. `stream` is a hipStream_t
 *     passed as void* (torch: torch.cuda.current_stream().cuda_stream).
 *   - every function only enqueues work on `stream`: no allocation, no host sync, graph-capturable.
 *   - return value: 0 = ok; < 0 = cstr error (CSTR_E_*); > 0 = hipError_t of the failed launch.
 *   - all floating point is IEEE fp32, compiled with -ffp-contract=off; fused ops are explicit.
 *   - control words that change every call (ring position, Adam step) live in HBM (`*_ctl`), so a
 *     captured hipGraph replays correctly; the last workgroup of a launch advances them.
 */
#ifndef CSTR_RL_HIP_H
#define CSTR_RL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSTR_ABI_VERSION 5

#define CSTR_OK 0
#define CSTR_E_BADARG (-1)      /* null pointer / non-positive size / misaligned buffer */
#define CSTR_E_UNSUPPORTED (-2) /* (obs_dim, act_dim) not in {(4,2), (8,2), (8,4)}, batch too large, 64-bit index range */

#define CSTR_INTEGRATOR_EULER 0 /* the reference: forward Euler, dt = 0.1 (twoseriescstr.py:493-496) */
#define CSTR_INTEGRATOR_RK4 1   /* north_star's ask; no reference counterpart */

typedef void *cstr_stream_t; /* hipStream_t */

/* f32-folded coefficients of TwoSeriesCSTREnv (twoseriescstr.py:37-61, :99, :103-106), folded with
 * NumPy >= 2 (NEP 50) semantics: Python-float products are formed in double, then rounded to f32
 * at their first contact with an f32 operand. Passed BY VALUE to the kernels (kernarg -> SGPRs). */
typedef struct cstr_coef {
    float q_v1, q_v2, cf, tf, tcf, k0, neg_e, r_gas, hk, rho_cp, cool1, cool2, neg_ua1, neg_ua2, rho_c, c_pc, dt;
    float s_lo[4], s_hi[4], s_span[4]; /* raw_state_low/high, high-low    (:56-57) */
    float a_lo[2], a_hi[2], a_span[2]; /* raw_action_low/high, high-low   (:60-61) */
    float target_c2, conc_span;        /* target_C2, max_conc - min_conc  (:103-106, :290) */
    int32_t max_steps;                 /* 400 (:99) */
} cstr_coef_t;

/* Replay ring in HBM, field-level SoA with the reference's array shapes (core/common/buffers.py:212-234):
 * observations/next_observations [rows][n_envs][obs_dim], actions [rows][n_envs][act_dim],
 * rewards/dones/timeouts [rows][n_envs]; all f32; obs rows 16-byte aligned. */
typedef struct cstr_ring {
    float *obs, *next_obs, *act, *rew, *done, *timeout;
    int64_t rows, n_envs;
    int32_t obs_dim, act_dim; /* (4,2) | (8,2) | (8,4) */
} cstr_ring_t;

/* ring_ctl: int64[4] in HBM = { pos, full, ticket, adds }  (buffers.py:101-104 `pos`, `full`) */
#define CSTR_RING_CTL_WORDS 4
/* adam_ctl: 4 x 64-bit words in HBM = { int64 step, int64 ticket, double beta1^step, double beta2^step }
 * (torch.optim.Adam state["step"]; the powers are the running products the bias corrections need) */
#define CSTR_ADAM_CTL_WORDS 4
/* mt_state: uint32[628] in HBM = { key[624], pos, has_gauss, gauss (f64, lo word first) } (numpy legacy RandomState) */
#define CSTR_MT_STATE_WORDS 628
#define CSTR_MAX_NOISE_PERIOD 8
/* pcg_state: uint64[4] per env in HBM = { state_hi, state_lo, inc_hi, inc_lo } (numpy PCG64) */
#define CSTR_PCG_STATE_WORDS 4
#define CSTR_MAX_SAMPLE_BATCH 16384

int cstr_abi_version(void);
const char *cstr_error_string(int code);

/* Host helper: fold the class constants of TwoSeriesCSTREnv (twoseriescstr.py:37-61) and the ctor
 * arguments default_target / min_concentration / max_concentration (:63-68) into f32 coefficients. */
void cstr_default_coef(cstr_coef_t *coef, double target_c2, double min_conc, double max_conc, int32_t max_steps);

/* VecEnv.step for N CSTR envs in one launch. Replaces the Python loop of
 * DummyVecEnv.step_wait (core/common/vec_env/dummy_vec_env.py:56-73) over
 * TwoSeriesCSTREnv.step/_dynamics/compute_reward (twoseriescstr.py:394-503, :271-392).
 *   (obs_dim, act_dim) selects the layout: (4,2) the reference's observation; (8,2) [normalised | raw];
 *   (8,4) TWO reactor trains side by side -- [train A | train B] normalised, actions [F1A,F2A,F1B,F2B], reward rA + rB,
 *   one step counter and one reset stream per env: the 8-obs / 4-act environment a 4-agent MADDPG needs.
 *   obs        [N][obs_dim] in : current observations
 *   act        [N][act_dim] in : env actions (normalised, clipped to [-1,1] inside, :399)
 *   step_count [N]          i/o: TwoSeriesCSTREnv.current_step
 *   reset_obs  [N][obs_dim] in : observation an env restarts from when it finishes this step
 *   next_obs   [N][obs_dim] out: true next observation (= infos[i]["terminal_observation"] when done)
 *   obs_after  [N][obs_dim] out: what VecEnv.step returns (reset obs when done); may alias obs
 *   reward/done/timeout [N] out: f32; timeout = infos[i]["TimeLimit.truncated"] */
int cstr_vec_step_f32(const cstr_coef_t *coef, int integrator, int obs_dim, int act_dim, const float *obs, const float *act,
                      int32_t *step_count, const float *reset_obs, float *next_obs, float *obs_after, float *reward,
                      float *done, float *timeout, int64_t n_envs, cstr_stream_t stream);

/* TwoSeriesCSTREnv.reset draws for envs with mask[i] != 0 (mask NULL = all) from per-env numpy-PCG64 states that the
 * host seeds exactly like gymnasium.utils.seeding.np_random(seed + i) (twoseriescstr.py:162):
 *   static_init NULL: init_mode="random", generate_initial_state (twoseriescstr.py:187-224, :267);
 *   static_init double[N][4 per train] i/o: init_mode="static" (:94-96, :246-255) -- the env's f64 `init_state`
 *   (constructed as {0.45, 310, 0.25, 290}) takes an in-place uniform step at every reset, like the reference's. */
int cstr_reset_draw_f32(uint64_t *pcg_state, const uint8_t *mask, double *static_init, int obs_dim, int act_dim,
                        float *obs_out, int64_t n_envs, cstr_stream_t stream);

/* ReplayBuffer.add (core/common/buffers.py:247-283) at the device-resident ring position; the last
 * workgroup advances ring_ctl (pos, full). */
int cstr_replay_add_f32(const cstr_ring_t *ring, int64_t *ring_ctl, const float *obs, const float *next_obs,
                        const float *act, const float *rew, const float *done, const float *timeout,
                        cstr_stream_t stream);

/* One fused collect step = _sample_action's scaling chain + VecEnv.step + _store_transition + ReplayBuffer.add
 * (core/common/off_policy_algorithm.py:396-406, :564, :477-496; buffers.py:247-283) in ONE pass over the envs:
 * reads state + policy output once, writes the ring row once, updates the env state in place.
 *   env_obs    [N][obs_dim] i/o: VecEnv state (_last_obs); replaced by the post-reset observation
 *   policy_out [N][act_dim] in : actor output. `squashed` is a bit field: bit 0 set = tanh output in [-1,1] that
 *                                predict() first unscales (core/common/policies.py:375), clear = an action already in
 *                                [low, high] (warm-up sample); bit 1 set = the multi-agent algorithms' behaviour
 *                                (core/common/multiagent_policy_algorithm.py:369, :391-392): no scale/unscale round
 *                                trip and no noise, buffer_action = env action = that value
 *   act_low/act_high [act_dim] in : HOST pointers, bounds of the algorithm-facing action space
 *   noise [N][act_dim] or NULL : added to the scaled action, then clip [-1,1] (off_policy_algorithm.py:401-402)
 *   reset_obs  [N][obs_dim] or NULL, pcg_state [N][4] or NULL: reset source (exactly one non-NULL)
 *   static_init double[N][4 per train] or NULL: with pcg_state, init_mode="static" (see cstr_reset_draw_f32)
 *   reward_out/done_out [N] or NULL: per-env copies (what VecEnv.step would have returned)
 *   ep_return [N] + ep_stats double[4] = {episodes, sum of returns, sum of lengths, -} or both NULL: device-side
 *                                episode statistics (Monitor's info["episode"], core/common/monitor.py:96-109; the
 *                                counters behind _episode_num / rollout/ep_rew_mean) accumulated without a host sync */
int cstr_collect_step_f32(const cstr_coef_t *coef, int integrator, const cstr_ring_t *ring, int64_t *ring_ctl,
                          float *env_obs, int32_t *step_count, const float *policy_out, int squashed,
                          const float *act_low, const float *act_high, const float *noise, const float *reset_obs,
                          uint64_t *pcg_state, double *static_init, float *reward_out, float *done_out, float *ep_return,
                          double *ep_stats, cstr_stream_t stream);
/* The same launch additionally advancing a Philox stream offset: policy_rng_ctl (may be NULL) is the control block of the
 * cstr_policy_rows_fwd_f32 launch that produced policy_out with cstr_policy_mlp_t.reserved bit 0 set ("the caller advances the
 * offset"); this launch's last workgroup adds policy_rng_advance (= that launch's row count) to its offset word -- the rollout's
 * _sample_action (core/common/off_policy_algorithm.py:364-411) and env step then share ONE control-word ticket. */
int cstr_collect_step_rng_f32(const cstr_coef_t *coef, int integrator, const cstr_ring_t *ring, int64_t *ring_ctl,
                              float *env_obs, int32_t *step_count, const float *policy_out, int squashed,
                              const float *act_low, const float *act_high, const float *noise, const float *reset_obs,
                              uint64_t *pcg_state, double *static_init, float *reward_out, float *done_out, float *ep_return,
                              double *ep_stats, uint64_t *policy_rng_ctl, uint64_t policy_rng_advance, cstr_stream_t stream);

/* np.random.seed(seed) for the device-resident legacy MT19937 state (core/common/utils.py:46;
 * twoseriescstr.py:164 reseeds the same global stream). */
int cstr_mt19937_seed(uint32_t *mt_state, uint32_t seed, cstr_stream_t stream);

/* ---- VecNormalize (core/common/vec_env/vec_normalize.py:174-290; core/common/running_mean_std.py:34-55) ----
 * vn_state: double[CSTR_VECNORM_STATE_WORDS] in HBM = { obs mean[8], obs var[8], obs count, ret mean, ret var, ret count }
 * (the reference's obs_rms / ret_rms, f64); returns: double[N] discounted returns (VecNormalize.returns). */
#define CSTR_VECNORM_STATE_WORDS 20
typedef struct {
    int32_t training, norm_obs, norm_reward, obs_dim; /* obs_dim <= 8 */
    double clip_obs, clip_reward, gamma, epsilon;
} cstr_vecnorm_cfg_t;

/* RunningMeanStd.__init__ for both statistics: mean 0, var 1, count 1e-4 (running_mean_std.py:5-15). */
int cstr_vecnorm_init_f64(double *vn_state, cstr_stream_t stream);

/* VecNormalize.step_wait (vec_normalize.py:174-204) on the raw outputs of the inner VecEnv, in the reference's order:
 * obs_rms.update(obs) [training && norm_obs], norm_obs_out = clip((obs - mean) / sqrt(var + eps)), returns = returns*gamma
 * + reward and ret_rms.update(returns) [training], norm_reward_out = clip(reward / sqrt(ret var + eps)), returns[done] = 0.
 * reward == NULL is VecNormalize.reset (:291-307): observation part only and returns = 0.
 *   obs [N][obs_dim] f32 raw; reward/done [N] f32 or NULL; norm_obs_out [N][obs_dim] / norm_reward_out [N] or NULL. */
int cstr_vecnorm_step_f64(const cstr_vecnorm_cfg_t *cfg, double *vn_state, double *returns, const float *obs,
                          const float *reward, const float *done, float *norm_obs_out, float *norm_reward_out,
                          int64_t n_envs, cstr_stream_t stream);

/* ReplayBuffer._get_samples(env=VecNormalize) (core/common/buffers.py:143-155, :312-323): normalize_obs on the sampled
 * observations / next_observations [B][obs_dim] and normalize_reward on rewards [B], in place, with the current
 * statistics. Each of obs / next_obs / reward may be NULL (at least one is not). */
int cstr_vecnorm_apply_f32(const cstr_vecnorm_cfg_t *cfg, const double *vn_state, float *obs, float *next_obs,
                           float *reward, int64_t batch, cstr_stream_t stream);

/* Exploration noise from the SAME legacy stream as the replay sampler: the reference's
 * VectorizedActionNoise.__call__ -> n_envs x NormalActionNoise.__call__ = np.random.normal(mu, sigma).astype(float32)
 * (core/common/noise.py:44-45, :141-142; OU noise draws np.random.normal(size=) the same way, :85-89).
 * out[j] = (float)(loc[j % period] + scale[j % period] * legacy_gauss()), j < count, in numpy's draw order (polar
 * Box-Muller, second deviate first, odd tail cached in mt_state). loc / scale: HOST double[period], period <= 8. */
int cstr_mt19937_normal_f32(uint32_t *mt_state, const double *loc, const double *scale, int32_t period, float *out,
                            int64_t count, cstr_stream_t stream);
/* The same draws kept in double precision: np.random.normal(size=...) as OrnsteinUhlenbeckActionNoise.__call__ uses it
 * (core/common/noise.py:85-89) before its own float64 arithmetic. */
int cstr_mt19937_normal_f64(uint32_t *mt_state, const double *loc, const double *scale, int32_t period, double *out,
                            int64_t count, cstr_stream_t stream);

/* ReplayBuffer.sample (core/common/buffers.py:106-115, :285-325): upper = rows if full else pos;
 * batch_inds = np.random.randint(0, upper, batch); env_indices = np.random.randint(0, n_envs, batch)
 * (legacy MT19937, masked rejection, bit-exact) fused with the gather of the five fields.
 *   out_obs [B][obs_dim], out_act [B][act_dim], out_next_obs [B][obs_dim], out_done [B] (= dones*(1-timeouts)),
 *   out_rew [B]; out_row_idx/out_env_idx int64 [B] or NULL. */
int cstr_replay_sample_mt19937_f32(const cstr_ring_t *ring, const int64_t *ring_ctl, uint32_t *mt_state, int64_t batch,
                                   float *out_obs, float *out_act, float *out_next_obs, float *out_done,
                                   float *out_rew, int64_t *out_row_idx, int64_t *out_env_idx, cstr_stream_t stream);

/* The same draw, gathered straight into the critics' input rows -- ReplayBuffer.sample + the th.cat([obs, actions], dim=1)
 * of ContinuousCritic.forward (core/common/policies.py:975-981) without the cat launches. Row width W = obs_dim + act_dim:
 *   x_data [B][W] <- (observations | actions)          the critic input of the Bellman error
 *   x_next [B][W] <- (next_observations | untouched)   the target critic's input; the actor head writes the action columns
 *   x_pi   [B][W] <- (observations | untouched)        the critic input of the actor loss; may be NULL */
int cstr_replay_sample_packed_mt19937_f32(const cstr_ring_t *ring, const int64_t *ring_ctl, uint32_t *mt_state, int64_t batch,
                                          float *x_data, float *x_next, float *x_pi, float *out_done, float *out_rew,
                                          int64_t *out_row_idx, int64_t *out_env_idx, cstr_stream_t stream);

/* The gather half of that call for index pairs drawn earlier in the iteration (cstr_rollout_step_f32): sample_idx int32
 * [2][batch] = { batch_inds, env_indices } (core/common/buffers.py:113, :309). ONE workgroup, which also performs the
 * control-word updates the rollout launch leaves to its successor: advance_ring != 0 = ReplayBuffer.add's epilogue on
 * ring_ctl (pos, full, adds; core/common/buffers.py:280-283), rng_ctl (may be NULL) = the rollout policy's Philox control
 * block, whose offset grows by rng_advance. Both happen after the gather, so the gather reads the ring by the given indices only. */
int cstr_replay_gather_packed_f32(const cstr_ring_t *ring, int64_t *ring_ctl, int advance_ring, uint64_t *rng_ctl,
                                  uint64_t rng_advance, const int32_t *sample_idx, int64_t batch, float *x_data, float *x_next,
                                  float *x_pi, float *out_done, float *out_rew, int64_t *out_row_idx, int64_t *out_env_idx,
                                  cstr_stream_t stream);

/* ReplayBuffer.sample's gather FUSED INTO ITS FIRST CONSUMER: y [M][n] = act(x W^T + b) where the input rows x are the sampled
 * transitions themselves, read from the ring by the index pairs of cstr_rollout_step_f32 (sample_idx as in
 * cstr_replay_gather_packed_f32). both != 0: M = 2 batch, rows [0, batch) = observations, rows [batch, 2 batch) = next
 * observations (SAC's two actor passes of a gradient step as one 2B-row pass, core/sac/sac.py:222, :247); both == 0: M = batch
 * rows of next observations (a target actor's first layer, core/td3/td3.py:173). w [n][obs_dim], bias [n]; act 0 none / 1 ReLU /
 * 2 Tanh. The launch also writes the packed batch of cstr_replay_sample_packed_mt19937_f32 (x_data, x_next, x_pi or NULL,
 * out_done, out_rew) for the launches behind it and performs the control-word updates of cstr_replay_gather_packed_f32
 * (advance_ring, rng_ctl / rng_advance): one launch and one dependent launch boundary less per gradient step. Results are
 * bit-identical to cstr_replay_gather_packed_f32 followed by cstr_linear_act_fwd_f32. */
int cstr_linear_act_fwd_gather_f32(const cstr_ring_t *ring, int64_t *ring_ctl, int advance_ring, uint64_t *rng_ctl, uint64_t rng_advance,
                                   const int32_t *sample_idx, int64_t batch, int both, const float *w, const float *bias, int act, float *y,
                                   int64_t n, float *x_data, float *x_next, float *x_pi, float *out_done, float *out_rew,
                                   cstr_stream_t stream);

/* Target-Q: SAC core/sac/sac.py:250-254 (logp, ent_coef non-NULL), TD3 core/td3/td3.py:174-176 (both NULL):
 * out = rew + (1 - done) * gamma * (min(q1, q2) - ent_coef[0] * logp). ent_coef is a DEVICE scalar. */
int cstr_td_target_min_f32(const float *q1, const float *q2, const float *logp, const float *rew, const float *done,
                           const float *ent_coef, float gamma, float *out, int64_t n, cstr_stream_t stream);

/* polyak_update over one flat parameter arena (core/common/utils.py:457-481):
 * target = fma(tau, param, target * (1 - tau)), bit-identical to torch's mul_ + add(alpha=). */
int cstr_polyak_f32(const float *param, float *target, double tau, int64_t n, cstr_stream_t stream);

/* torch.optim.Adam step (defaults of core/common/policies.py:96-117) over one flat arena; the step
 * counter lives in adam_ctl and is advanced by the last workgroup. lr is a DEVICE scalar (f64) so
 * _update_learning_rate (core/common/base_class.py:303-317) needs no re-capture. */
int cstr_adam_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t *adam_ctl,
                  const double *lr, double beta1, double beta2, double eps, float grad_scale, int64_t n,
                  cstr_stream_t stream);

/* Several flat-arena updates in ONE launch (SAC: the entropy coefficient -- one parameter -- next to the critic,
 * core/sac/sac.py:240-243 and :266-268; the actor's step next to the critic's soft target update, :281 and :284-287). A
 * segment is a cstr_adam_f32 call's argument list, or -- polyak_source != NULL -- a cstr_polyak_f32 call with param = the
 * TARGET arena (the other Adam fields are ignored). Segments must not depend on each other. */
#define CSTR_MAX_ADAM_SEGS 4
typedef struct {
    float *param; const float *grad; float *exp_avg; float *exp_avg_sq; int64_t *adam_ctl; const double *lr;
    double beta1, beta2, eps; float grad_scale; int64_t n;
    const float *polyak_source; double tau;
    /* optional (NULL = none): a tile-major shadow copy (cstr_policy_swizzle_f32) of the [shadow_n][shadow_k] weight matrix that
     * starts shadow_begin floats into `param` -- rewritten by the same threads that update those weights, so the policy
     * kernel's copy never lags the parameters. shadow_begin and shadow_k are multiples of 4. */
    float *shadow; int64_t shadow_begin, shadow_n, shadow_k;
    /* optional (NULL = none), Adam segments only: the soft-update target OF THESE PARAMETERS. The thread that has just computed
     * param_new[i] also writes own_target[i] = fma(tau, param_new[i], own_target[i] * (1 - tau)) -- a cstr_polyak_f32(param,
     * own_target, tau) that would otherwise need its own launch BEHIND this one (TD3 / MADDPG: the actor's step followed by the
     * actor target's soft update, core/td3/td3.py:199-205, core/maddpg/maddpg.py:179-185). Uses the segment's `tau`. */
    float *own_target;
} cstr_adam_seg_t;
int cstr_adam_multi_f32(const cstr_adam_seg_t *segs, int n_segs, cstr_stream_t stream);

/* ---- learner glue around the PyTorch-ROCm GEMMs (csrc/cstr_mlp.hip) --------------------------------------------- */

#define CSTR_ACT_NONE 0
#define CSTR_ACT_RELU 1
#define CSTR_ACT_TANH 2

/* nn.Linear's bias add + the activation create_mlp puts behind it (core/common/torch_layers.py:110-183), in place on
 * the GEMM output. Grouped form for batched GEMMs (twin critics): y [groups][m][n], bias [groups][n]. */
int cstr_bias_act_fwd_f32(float *y, const float *bias, int act, int64_t groups, int64_t m, int64_t n, cstr_stream_t stream);

/* Backward of the same: gz = gy * act'(y) and gbias[n] = sum_m gz[m][n] (autograd's threshold/tanh backward + the
 * bias gradient's batch sum). gbias may be NULL; with act == NONE and gz == gy nothing is copied. */
int cstr_bias_act_bwd_f32(const float *gy, const float *y, int act, float *gz, float *gbias, int64_t groups, int64_t m, int64_t n,
                          cstr_stream_t stream);
/* The same for ONE group whose gy / y are column blocks of wider row-major matrices (row strides ldg / ldy >= n): the action columns of
 * d(loss)/d(critic input) and of the critic input itself in the deterministic actors' backward (core/td3/td3.py:194-200,
 * core/maddpg/maddpg.py:167-185) -- no gather copies. gz is contiguous [m][n]. */
int cstr_bias_act_bwd_rows_f32(const float *gy, int64_t ldg, const float *y, int64_t ldy, int act, float *gz, float *gbias, int64_t m,
                               int64_t n, cstr_stream_t stream);

/* nn.Linear + the activation create_mlp puts behind it (core/common/torch_layers.py:110-183), forward, in ONE launch for the
 * learners' small shapes: y[g][m][n] = act(sum_k x[g][m][k] * w[g][n][k] + bias[g][n]) on the f32 matrix cores (exact f32 fma
 * chains). x rows are ldx floats apart and groups x_group_stride floats apart (0 = every group reads the same input); w
 * [groups][n][k], bias [groups][n], y [groups][m][n] contiguous. The backward keeps the rocBLAS GEMMs + cstr_bias_act_bwd_f32. */
int cstr_linear_act_fwd_f32(const float *x, int64_t x_group_stride, int64_t ldx, const float *w, const float *bias, int act, float *y,
                            int64_t groups, int64_t m, int64_t n, int64_t k, cstr_stream_t stream);

/* cstr_linear_act_fwd_f32 for up to 8 INDEPENDENT layers of one shape in one launch (every agent's actor layer in MADDPG /
 * IDDPG: core/maddpg/policies.py builds one MLP per agent; the reference evaluates them one after the other). Each set:
 * y[m][n] = act(x[m] . w[n] + bias[n]) with x rows ldx apart and y rows ldy apart (y may be the agent's column block of the
 * joint action). */
#define CSTR_MAX_LINEAR_SETS 16
typedef struct { const float *x; int64_t ldx; const float *w; const float *bias; float *y; int64_t ldy; } cstr_linear_set_t;
int cstr_linear_act_fwd_sets_f32(const cstr_linear_set_t *sets, int n_sets, int act, int64_t m, int64_t n, int64_t k,
                                 cstr_stream_t stream);

/* Backward of a Linear w.r.t. its input, fused with the activation gradient of the layer BELOW it (autograd's mm backward +
 * threshold/tanh backward of core/common/torch_layers.py:110-183's Linear -> ReLU -> Linear):
 *   dz[g][m][k] = (sum_n gz[g][m][n] * w[g][n][k]) * act'(y[g][m][k])
 * gz: gradient w.r.t. this layer's pre-activation [groups][m][n]; w [groups][n][k]; y [groups][m][k]: the lower layer's
 * OUTPUT (this layer's input), NULL with act == NONE; all contiguous. sum_groups != 0: the groups share ONE input
 * (stacked critics): dz [m][k] = sum_g gz[g] @ w[g] (and y [m][k]) -- the batched product and the sum over groups at once. */
int cstr_linear_bwd_input_f32(const float *gz, const float *w, const float *y, int act, float *dz, int64_t groups, int sum_groups,
                              int64_t m, int64_t n, int64_t k, cstr_stream_t stream);

/* Weight and bias gradient of a Linear in one launch (autograd's mm backward for the weight + the bias sum over the batch):
 *   dw[g][n][k] = sum_m dz[g][m][n] * x[g][m][k],   db[g][n] = sum_m dz[g][m][n]   (db may be NULL)
 * dz [groups][m][n] contiguous (gradient w.r.t. the pre-activation); x rows ldx floats apart, groups x_group_stride apart
 * (0 = shared input); dw [groups][n][k] and db [groups][n] contiguous -- views of the gradient arena. */
int cstr_linear_bwd_weight_f32(const float *dz, const float *x, int64_t x_group_stride, int64_t ldx, float *dw, float *db,
                               int64_t groups, int64_t m, int64_t n, int64_t k, cstr_stream_t stream);

/* The same for up to CSTR_MAX_LINEAR_SETS independent Linears (each with its own shape) in ONE launch: the parameter gradients
 * of an MLP's layers once its backward chain has produced every dz. db may be NULL per set. */
typedef struct cstr_wgrad_set {
    const float *dz; /* [m][n] contiguous */
    const float *x;  /* [m][k], rows ldx floats apart */
    int64_t ldx;
    float *dw;       /* [n][k] */
    float *db;       /* [n] or NULL */
    int64_t m, n, k;
} cstr_wgrad_set_t;
int cstr_linear_bwd_weight_sets_f32(const cstr_wgrad_set_t *sets, int n_sets, cstr_stream_t stream);

/* Last hidden layer + scalar head of a Q network: create_mlp(..., output_dim = 1) (core/common/torch_layers.py:110-183;
 * ContinuousCritic.forward, core/common/policies.py:960-987) ends in y = act(z + b1), q = y . w2 + b2. The head is a
 * matrix-vector product, done in the epilogue of the previous GEMM: z [groups][m][k] is replaced by y IN PLACE and
 * q [groups][m] is written. b1, w2 [groups][k]; b2 [groups]. */
int cstr_hidden_head_fwd_f32(float *z, const float *b1, int act, const float *w2, const float *b2, float *q, int64_t groups,
                             int64_t m, int64_t k, cstr_stream_t stream);

/* Backward of the pair given gq = d(loss)/dq [groups][m]: dz = gq * w2 * act'(y) [groups][m][k] and, when the three
 * parameter-gradient pointers are given (all or none), gb1[k] = sum_m dz, gw2[k] = sum_m gq * y, gb2 = sum_m gq. */
int cstr_hidden_head_bwd_f32(const float *gq, const float *y, int act, const float *w2, float *dz, float *gb1, float *gw2,
                             float *gb2, int64_t groups, int64_t m, int64_t k, cstr_stream_t stream);

/* SquashedDiagGaussianDistribution (core/common/distributions.py:161-260) with SAC's log_std clamp
 * (core/sac/policies.py:20-22, :162-164): u = mean + exp(clamp(log_std_raw, -20, 2)) * eps, action = tanh(u),
 * logp = sum_j Normal.log_prob(u_j) - sum_j log(1 - action_j^2 + 1e-6). logp may be NULL (acting only).
 * in_stride = row stride of mean / log_std_raw: act_dim for separate tensors, 2*act_dim when they are the two halves of
 * one merged mu|log_std GEMM output. */
int cstr_squashed_gaussian_fwd_f32(const float *mean, const float *log_std_raw, const float *eps, float *action, float *logp,
                                   int64_t batch, int act_dim, int in_stride, cstr_stream_t stream);
/* Its analytic backward: (g_action rows of stride g_action_stride or NULL, g_logp [B] or NULL) -> g_mean, g_log_std_raw
 * (rows of stride in_stride). */
int cstr_squashed_gaussian_bwd_f32(const float *g_action, const float *g_logp, const float *action, const float *log_std_raw,
                                   const float *eps, float *g_mean, float *g_log_std_raw, int64_t batch, int act_dim,
                                   int in_stride, int g_action_stride, cstr_stream_t stream);

/* The SAC actor's merged (mu | log_std) head in one pass (core/sac/policies.py:162-175; core/common/distributions.py:161-260):
 * params [B][2A] = the head GEMM's output, gets `bias` [2A] added in place (NULL: already biased); eps [B][A] ~ N(0,1) is READ
 * when rng_ctl is NULL and DRAWN (and written, for the backward) when rng_ctl is given; action = tanh(mean + exp(clamp(
 * log_std)) * eps) with row stride `action_stride` (>= A: it may be a column block of the critic's input); logp [B] or NULL.
 * rng_ctl: uint64[CSTR_RNG_CTL_WORDS] in HBM = { seed, offset, ticket, -, sub-tickets[8] (cstr_policy_rows_fwd_f32), - }:
 * Philox4x32-10 counter RNG + Box-Muller, the offset advances by B per launch on the device (graph-replay safe). */
#define CSTR_RNG_CTL_WORDS 16
#define CSTR_MAX_HEAD_ACT 4
int cstr_gaussian_head_fwd_f32(float *params, const float *bias, float *eps, uint64_t *rng_ctl, float *action,
                               int64_t action_stride, float *logp, int64_t batch, int act_dim, cstr_stream_t stream);

/* The same head INCLUDING its Linear: params[b][j] = hidden[b] . w[j] + bias[j] (2A <= 8 dot products per row -- a matrix-
 * vector shaped product, one wave per row) followed by the sampling above. hidden rows ldh floats apart (k and ldh multiples
 * of 4, 16-byte aligned); w [2A][k], bias [2A]; params [B][2A] is an OUTPUT here (kept for the backward). */
int cstr_gaussian_head_gemm_fwd_f32(const float *hidden, int64_t ldh, const float *w, const float *bias, float *params, float *eps,
                                    uint64_t *rng_ctl, float *action, int64_t action_stride, float *logp, int64_t batch, int act_dim,
                                    int64_t k, cstr_stream_t stream);

/* Backward: g_params [B][2A] = d/d(mean | log_std_raw) from g_action (row stride ga_stride, or NULL) and g_logp ([B] or
 * NULL); g_bias [2A] = column sums over the batch (or NULL). */
int cstr_gaussian_head_bwd_f32(const float *g_action, int64_t ga_stride, const float *g_logp, const float *action,
                               int64_t action_stride, const float *params, const float *eps, float *g_params, float *g_bias,
                               int64_t batch, int act_dim, cstr_stream_t stream);

/* The same backward carried one layer further when the head's Linear (w [2A][width], core/sac/policies.py:100-104) sits on
 * a hidden layer with activation `act` (0 none, 1 ReLU, 2 Tanh) whose OUTPUT is `hidden` (rows ldh floats apart):
 * g_params as above and dz [B][width] = (g_params . w) * act'(hidden) = d(loss)/d(that layer's pre-activation), the input
 * of cstr_linear_bwd_weight_f32 / cstr_linear_bwd_input_f32. The head's dW / db: cstr_linear_bwd_weight_f32(g_params, hidden). */
int cstr_gaussian_head_bwd_input_f32(const float *g_action, int64_t ga_stride, const float *g_logp, const float *action,
                                     int64_t action_stride, const float *params, const float *eps, const float *w,
                                     const float *hidden, int64_t ldh, int act, float *g_params, float *dz, int64_t batch,
                                     int act_dim, int64_t width, cstr_stream_t stream);

/* A whole policy network for MANY rows, inference only (no activations kept, no backward): create_mlp(k0, ., [h1, h2]) with
 * activation `act` on both hidden layers (core/common/torch_layers.py:110-183) + the action head, ONE launch.
 * head 0: SAC's squashed Gaussian (core/sac/policies.py:147-175): w3 [2A][h2] = (mu | log_std) weights, b3 [2A]; the action
 *         (rows action_stride apart, e.g. the action columns of a critic input) = tanh(mu + exp(clamp(log_std)) * eps), eps
 *         read ([m][A]) or drawn from the Philox stream `rng_ctl` (same stream positions as cstr_gaussian_head_fwd_f32:
 *         counter = offset + row; the offset advances by m); logp [m] optional.
 * head 1: deterministic actor (core/td3/policies.py:75-78): w3 [A][h2], b3 [A], action = out_act(h2 w3^T + b3); eps, rng_ctl
 *         and logp must be NULL.
 * h1, h2 multiples of 4, k0 <= 256, 16 * (h1 + h2 + 8) floats of LDS <= 64 KB.
 * reserved: bit 0 set = the caller advances the Philox offset by m before the stream's next consumer
 * (cstr_collect_step_rng_f32 does): the launch then ends without its 256-workgroup "last one out" ticket; other bits 0.
 * With w2_swizzled and h1, h2 <= 512 the software-pipelined kernel runs. */
typedef struct cstr_policy_mlp {
    int32_t k0, h1, h2, act_dim;
    int32_t act, head, out_act, reserved;
    const float *w1, *b1; /* [h1][k0], [h1] */
    const float *w2, *b2; /* [h2][h1], [h2] */
    const float *w3, *b3; /* head */
    const float *w2_swizzled; /* NULL, or w2 in the tile-major layout of cstr_policy_swizzle_f32 (full-line loads) */
} cstr_policy_mlp_t;
/* Tile-major copy of a weight matrix w [n][k] (k a multiple of 4) for the matrix-core operand loads of
 * cstr_policy_rows_fwd_f32: out[((tile * ceil(k/16) + chunk) * 64 + lane) * 4 + e] = w[16 tile + (lane & 15)][16 chunk +
 * 4 (lane >> 4) + e], zeros outside the matrix; out holds ceil(n/16) * ceil(k/16) * 256 floats. A wave's operand load then
 * reads 1 KB of consecutive bytes instead of sixteen 64-byte row pieces. */
int cstr_policy_swizzle_f32(const float *w, int64_t n, int64_t k, float *out, cstr_stream_t stream);
int cstr_policy_rows_fwd_f32(const cstr_policy_mlp_t *net, const float *x, int64_t ldx, const float *eps, uint64_t *rng_ctl,
                             float *action, int64_t action_stride, float *logp, int64_t m, cstr_stream_t stream);

/* One vec-step of collect_rollouts in ONE launch (core/common/off_policy_algorithm.py:510-605 for a device-resident vec-env):
 * the policy network + sampling of cstr_policy_rows_fwd_f32 on x [n_envs][k0] (the policy's view of the observations: env_obs
 * itself, or its normalised image), then -- on the sampling tail's lanes, the action never leaving registers -- the fused
 * collect step of cstr_collect_step_f32 for the workgroup's 16 envs (same operands, same arithmetic), and, when mt_state is
 * given, ReplayBuffer.sample's two index draws for the gradient step behind it (core/common/buffers.py:112-113, :309; numpy
 * legacy MT19937, masked rejection, bit-exact) on one otherwise idle wave: sample_idx int32 [2][batch] = { batch_inds,
 * env_indices }, drawn against the ring AS THE ADD OF THIS LAUNCH LEAVES IT (upper = rows if full else pos + 1), mt_state
 * advanced. No control word is written here: ring_ctl is only read (the row goes to position pos), the Philox offset of
 * rng_ctl stays; the next launch must be cstr_replay_gather_packed_f32(advance_ring = 1, rng_ctl, rng_advance = n_envs), or
 * the caller advances them another way. Needs the tile-major W2 copy (net->w2_swizzled), hidden widths <= 512, k0 <= 16 in
 * 16-byte-aligned rows (CSTR_E_UNSUPPORTED otherwise: use the separate launches). head 0: rng_ctl required; head 1: NULL.
 * action_out [n_envs][act_dim] or NULL: the policy output (what cstr_policy_rows_fwd_f32 would have written). */
int cstr_rollout_step_f32(const cstr_policy_mlp_t *net, const float *x, int64_t ldx, uint64_t *rng_ctl, const cstr_coef_t *coef,
                          int integrator, const cstr_ring_t *ring, const int64_t *ring_ctl, float *env_obs, int32_t *step_count,
                          int squashed, const float *act_low, const float *act_high, const float *noise, const float *reset_obs,
                          uint64_t *pcg_state, double *static_init, float *reward_out, float *done_out, float *ep_return,
                          double *ep_stats, float *action_out, uint32_t *mt_state, int64_t batch, int32_t *sample_idx,
                          cstr_stream_t stream);

/* Whole evaluation episodes in ONE launch: evaluate_policy's loop (core/common/evaluation.py:84-131) for a device-resident vec-env and
 * a policy that cstr_policy_mlp_t describes. A workgroup owns 16 envs and walks their vec-steps inside the launch; per step: the policy
 * network on the 16 observation rows (k0 = obs_dim; the shapes of cstr_policy_rows_fwd_f32, W2 streamed from L2 as rows or, when
 * net->w2_swizzled is given, from the tile-major copy), the head (head 0: the squashed Gaussian at its mode, tanh(mu), exactly what
 * eps = 0 gives; head 1: the deterministic actor), predict()'s post-processing (`squashed` 1: low + 0.5 (a + 1)(high - low), 0: clip into
 * [low, high]; core/common/policies.py:379-386), the env step, the episode accounting and the PCG64 reset draw of an env whose episode
 * ended. Workgroups exchange nothing; the launch writes no control word.
 *   env_obs [N][obs_dim] i/o, step_count int32[N] i/o, pcg_state [N][4] i/o, static_init double[N][4 per train] i/o or NULL (as in
 *   cstr_collect_step_f32); act_low / act_high [act_dim]: HOST pointers
 *   targets int32[N]: HOST pointer (validated before anything is enqueued, then copied into ep_done on `stream`, which is why this entry
 *                     point is not graph-capturable from pageable memory): episodes wanted per env, 0 allowed. The copy is asynchronous:
 *                     the caller keeps the array alive and unmodified until `stream` has passed it (e.g. until it has read ep_done back)
 *   max_vec_steps: bound of the loop over vec-steps whatever the data does; the caller passes max(targets) * coef->max_steps, which a
 *                  correct run never reaches (every episode is truncated by max_steps)
 *   ep_return double[N][ep_stride], ep_len int32[N][ep_stride] with ep_stride = max(targets): episode j of env i in slot [i][j] -- the f64
 *                  sum of the f32 step rewards and the step count; slots at and beyond targets[i] are not written (both may be NULL
 *                  when every target is 0)
 *   ep_done int32[N]: episodes counted; ep_done[i] < targets[i] after the launch means max_vec_steps cut the run short (the caller's error)
 * For the counted episodes ep_return / ep_len / ep_done and pcg_state are bit-identical to the step-by-step launches:
 * cstr_policy_rows_fwd_f32 on the same net (head 0: eps = 0), the post-processing, cstr_vec_step_f32 with reset observations from
 * cstr_reset_draw_f32. An env stops once it has met its target: its state after its last counted episode (the reset draw behind that
 * episode included) is what the launch leaves -- the host loop keeps stepping finished envs until all are done, this launch does not.
 * CSTR_E_UNSUPPORTED: (obs_dim, net->act_dim) not a layout, unknown integrator, a network shape cstr_policy_rows_fwd_f32 does not take
 * or more than 64 KB of LDS; CSTR_E_BADARG: NULL pointers, n_envs <= 0, a negative target, max_vec_steps <= 0, net->k0 != obs_dim,
 * misaligned rows, outputs overlapping inputs or each other. */
int cstr_eval_episodes_f32(const cstr_policy_mlp_t *net, const cstr_coef_t *coef, int integrator, int obs_dim, float *env_obs,
                           int32_t *step_count, uint64_t *pcg_state, double *static_init, int squashed, const float *act_low,
                           const float *act_high, const int32_t *targets, int64_t n_envs, int64_t max_vec_steps, double *ep_return,
                           int32_t *ep_len, int32_t *ep_done, cstr_stream_t stream);

/* The recording form of cstr_eval_episodes_f32 on the (4, 2) layout: a trained policy rolled out into replay-ring rows in ONE launch,
 * optionally epsilon-uniform -- the collection loop behind an offline dataset and behind closed-loop response curves. Every env of a
 * workgroup's 16 runs exactly n_steps vec-steps (a fixed trip count: no targets, no early end). At vec-step t the lane of env i
 *   a. forms the deterministic head value v_j of cstr_eval_episodes_f32 (head 0: tanh(mu), what eps = 0 gives; head 1: out_act(.));
 *   b. when explore_prob > 0 takes ONE Philox4x32-10 block, key = (seed lo, seed hi), counter = (idx lo, idx hi, step_offset + t,
 *      0xC011EC7D) with idx = index_offset + i; with u(w) = (w >> 8) * 2^-24: explore = u(w0) < explore_prob (float32 compare), and an
 *      exploring row replaces v_j by a uniform draw over the action space -- squashed & 1: v_j = 2 u(w[1+j]) - 1; otherwise
 *      v_j = low_j + u(w[1+j]) * (high_j - low_j), the product and the sum rounded separately (no FMA). explore_prob == 0 evaluates no block;
 *   c. unsquashed actors (squashed == 0; PPO / A2C): v_j = clip(v_j, low_j, high_j), NaN kept -- predict()'s clip;
 *   d. runs the action scaling chain of cstr_collect_step_f32 on v (no noise): sa = the buffer action, ea = the env's action;
 *   e. steps the env and writes ring row row0 + t with the stores and values of cstr_collect_step_f32: obs = the observation before the
 *      step, next_obs = the TERMINAL observation (never the reset one), act = sa, rew, done = timeout = truncated; explored (optional,
 *      uint8 [ring rows][N]) gets the flag at [row0 + t][i];
 *   f. adds the f32 reward to an f64 running return and counts the step; where the episode ends: if the env's episode count is below
 *      ep_stride, ep_return[i][count] / ep_len[i][count] are stored; the count is incremented either way (episodes beyond ep_stride are
 *      counted, not stored); then the PCG64 auto-reset draw of cstr_collect_step_f32, step_count = 0.
 * After the loop env_obs / step_count / pcg_state (/ static_init) hold the env's state and ep_done[i] the count. The launch touches no
 * control word: pos / full of a ring_ctl are the caller's. Arguments as in cstr_eval_episodes_f32, plus
 *   ring: its n_envs / obs_dim / act_dim must be N / 4 / 2; rows row0 .. row0 + n_steps - 1 are written, all others left alone
 *   ep_return double[N][ep_stride], ep_len int32[N][ep_stride] (both may be NULL when ep_stride is 0), ep_done int32[N] out.
 * Bit-level contract: ring rows, env state and episode outputs equal what the step-by-step launches give -- cstr_policy_rows_fwd_f32
 * (head 0: eps = 0), the statement of b. and c. on its output, cstr_collect_step_f32 without noise.
 * CSTR_E_BADARG: NULL required pointers, n_envs <= 0, n_steps <= 0, row0 < 0 or row0 + n_steps > ring->rows, a ring whose n_envs / obs_dim /
 * act_dim disagree with the env's, explore_prob outside [0, 1] or NaN, step_offset < 0 or step_offset + n_steps > 2^32, ep_stride < 0 or
 * ep_stride > 0 without ep_return / ep_len, net->k0 != obs_dim, misaligned arrays, anything written (ring fields, explored, episode outputs,
 * env state) overlapping anything read or anything else written. CSTR_E_UNSUPPORTED: what cstr_eval_episodes_f32 declines, and the (8, 2) /
 * (8, 4) layouts. All checked before anything is enqueued. */
int cstr_collect_episodes_f32(const cstr_policy_mlp_t *net, const cstr_coef_t *coef, int integrator, int obs_dim, float *env_obs,
                              int32_t *step_count, uint64_t *pcg_state, double *static_init, int squashed, const float *act_low,
                              const float *act_high, const cstr_ring_t *ring, int64_t row0, int64_t n_envs, int64_t n_steps,
                              float explore_prob, uint64_t seed, int64_t index_offset, int64_t step_offset, double *ep_return,
                              int32_t *ep_len, int64_t ep_stride, int32_t *ep_done, uint8_t *explored, cstr_stream_t stream);

/* TD3 / MADDPG target policy smoothing (core/td3/td3.py:167-173; core/maddpg/maddpg.py:131-142) in one launch:
 * noise = clamp(N(0, sigma), -clip, clip); out = clamp(action + noise, -1, 1). action [B][A] contiguous (the target
 * actor's output); `noise` [B][A] (already scaled by sigma) is read when rng_ctl is NULL, otherwise sigma * N(0,1) is drawn
 * from the Philox stream rng_ctl (see cstr_gaussian_head_fwd_f32). out rows are out_stride floats apart. */
int cstr_target_smooth_f32(const float *action, const float *noise, uint64_t *rng_ctl, float sigma, float clip, float *out,
                           int64_t out_stride, int64_t batch, int act_dim, cstr_stream_t stream);

/* A deterministic target actor's LAST Linear with that smoothing inside (core/td3/td3.py:167-173: actor_target(next_obs), then
 * noise, clamp, add, clamp): out[row][j] = clamp(act(x W^T + b)[row][j] + clamp(z, -clip, clip), -1, 1), z as in
 * cstr_target_smooth_f32 (noise [m][n] read, or sigma * N(0,1) drawn from rng_ctl with the same counters; the offset advances by
 * m). One launch instead of two; bit-identical to cstr_linear_act_fwd_f32 followed by cstr_target_smooth_f32. w [n][k], n <= 16,
 * k > 32, m <= 32768 (CSTR_E_UNSUPPORTED otherwise: use the two launches). */
int cstr_linear_smooth_fwd_f32(const float *x, int64_t ldx, const float *w, const float *bias, int act, const float *noise,
                               uint64_t *rng_ctl, float sigma, float clip, float *out, int64_t out_stride, int64_t m, int64_t n,
                               int64_t k, cstr_stream_t stream);

/* SAC entropy coefficient (core/sac/sac.py:230-243): ent_coef_out = exp(log_alpha); grad_out = d/dlog_alpha of
 * -mean(log_alpha * (logp + target_entropy)) = -mean(logp + target_entropy). loss_out (stored) and loss_sum /
 * ent_coef_sum (accumulated) are device scalars, each may be NULL: the values train() logs (:232, :236), no host sync. */
int cstr_sac_alpha_f32(const float *log_alpha, const float *logp, float target_entropy, float *grad_out, float *ent_coef_out,
                       float *loss_out, float *loss_sum, float *ent_coef_sum, int64_t batch, cstr_stream_t stream);

/* Twin-critic loss as a backward root: loss = scale * (mse(q1, t) + mse(q2, t)) (scale 0.5: core/sac/sac.py:261;
 * scale 1: core/td3/td3.py:182, core/maddpg/maddpg.py:157); gq_k = d loss / d q_k. */
int cstr_twin_q_loss_f32(const float *q1, const float *q2, const float *target, float scale, float *gq1, float *gq2,
                         float *loss_out, float *loss_sum, int64_t batch, cstr_stream_t stream);

/* TD target + twin-critic loss (+ optionally SAC's entropy-coefficient loss) in ONE launch: cstr_td_target_min_f32,
 * cstr_twin_q_loss_f32 and cstr_sac_alpha_f32 back to back, bit for bit (core/sac/sac.py:230-261; core/td3/td3.py:167-182).
 * q1_t / q2_t: the target critics on the next state; next_logp NULL for TD3; `alpha` NULL (or log_alpha NULL) = no
 * entropy-coefficient part, then the target uses ent_coef[0]; with it the target uses exp(log_alpha[0]) and ent_coef is
 * ignored. target_out [B] may be NULL. */
typedef struct cstr_alpha_part {
    const float *log_alpha; /* [1] */
    const float *logp_pi;   /* [B] log pi(a|s) of the actor pass on the sampled observations */
    float target_entropy;
    float *grad_out;        /* [1] d loss / d log_alpha */
    float *ent_coef_out;    /* [1] exp(log_alpha) */
    float *loss_out;        /* [1] or NULL: stored */
    float *loss_sum;        /* [1] or NULL: accumulated */
    float *ent_coef_sum;    /* [1] or NULL: accumulated */
} cstr_alpha_part_t;
int cstr_td_twin_q_loss_f32(const float *q1_t, const float *q2_t, const float *next_logp, const float *rew, const float *done,
                            const float *ent_coef, float gamma, const float *q1, const float *q2, float scale, float *target_out,
                            float *gq1, float *gq2, float *loss_out, float *loss_sum, const cstr_alpha_part_t *alpha,
                            int64_t batch, cstr_stream_t stream);

/* cstr_hidden_head_bwd_f32 with the loss root INSIDE: d(loss)/dq of the twin Q networks (groups = 2) is computed per row in
 * the kernel instead of being read from gq, and one extra workgroup performs the batch reductions of the separate loss
 * launch (logged loss, entropy-coefficient part, g_logp) with that launch's arithmetic and reduction order -- the critic
 * backward's / the actor backward's first launch and its loss launch become ONE.
 *   mode 1 (critic loss, core/sac/sac.py:245-261, core/td3/td3.py:174-182) = cstr_td_twin_q_loss_f32's fields;
 *   mode 2 (SAC actor loss, core/sac/sac.py:273-275)                       = cstr_sac_actor_loss_f32's fields (q1/q2 = Q(s, pi(s)));
 *   mode 3 (deterministic actors' loss -mean(Q1(s, pi(s))), core/td3/td3.py:194, core/maddpg/maddpg.py:177) = cstr_neg_mean_loss_f32's
 *          fields (q1, loss_out, loss_sum), through the FIRST Q network alone: y / dz [1][m][k], w2 [k], gb1 / gw2 / gb2 of that network.
 * Unused pointers NULL; gq1 / gq2 of the separate launches are not produced (nothing else reads them). m <= 1024 rows. */
typedef struct cstr_head_root {
    int32_t mode, batch;
    float gamma, scale;
    const float *q1_t, *q2_t, *next_logp, *rew, *done; /* mode 1 */
    const float *ent_coef;                             /* [1]: mode 1 without alpha part, mode 2 */
    const float *q1, *q2;                              /* [batch] each */
    float *target_out;                                 /* mode 1, [batch] or NULL */
    const float *logp;                                 /* mode 2 */
    float *g_logp;                                     /* mode 2 out [batch] */
    float *loss_out, *loss_sum;                        /* [1] or NULL */
    cstr_alpha_part_t alpha;                           /* mode 1: log_alpha NULL = absent */
} cstr_head_root_t;
int cstr_hidden_head_bwd_root_f32(const cstr_head_root_t *root, const float *y, int act, const float *w2, float *dz, float *gb1,
                                  float *gw2, float *gb2, int64_t m, int64_t k, cstr_stream_t stream);

/* SAC actor loss as a backward root (core/sac/sac.py:273-275): loss = mean(ent_coef * logp - min(q1, q2)). */
int cstr_sac_actor_loss_f32(const float *logp, const float *q1, const float *q2, const float *ent_coef, float *g_logp, float *gq1,
                            float *gq2, float *loss_out, float *loss_sum, int64_t batch, cstr_stream_t stream);

/* Critic ensembles (policy_kwargs n_critics = N, 1 <= N <= CSTR_MAX_ENS_CRITICS; reference core/common/policies.py:934-965): the
 * N-critic forms of cstr_td_twin_q_loss_f32 and cstr_sac_actor_loss_f32, one single-workgroup launch each (batch <= 16384). Q values
 * are [N][batch] with a row stride (the stacked critic output [G, B, 1]; unused for N = 1), gq is [N][batch] contiguous. Per critic
 * the twin kernels' expressions and block-sum tree: at N = 2 both are bit-identical to their twin counterparts.
 * cstr_td_ens_q_loss_f32 (core/sac/sac.py:249-261, core/td3/td3.py:174-182): t = rew + (1 - done) * gamma * (min_i q_t[i] - alpha *
 *   next_logp); gq[i] = scale * 2 / B * (q[i] - t); loss = scale * (((s_0 / B + s_1 / B) + s_2 / B) + ...), s_i = sum_b (q[i] - t)^2
 *   in critic order. next_logp, ent_coef, alpha, target_out as in cstr_td_twin_q_loss_f32.
 * cstr_sac_actor_ens_loss_f32 (core/sac/sac.py:273-275): loss = mean(ent_coef * logp - min_i q_i); g_logp = ent_coef / B; gq[i][b] =
 *   -1/B for the FIRST index attaining the minimum (th.min's convention), 0 for the others. */
#define CSTR_MAX_ENS_CRITICS 16
int cstr_td_ens_q_loss_f32(const float *q_t, int64_t q_t_stride, const float *next_logp, const float *rew, const float *done,
                           const float *ent_coef, float gamma, const float *q, int64_t q_stride, float scale, float *target_out, float *gq,
                           float *loss_out, float *loss_sum, const cstr_alpha_part_t *alpha, int n_critics, int64_t batch,
                           cstr_stream_t stream);
int cstr_sac_actor_ens_loss_f32(const float *logp, const float *q, int64_t q_stride, const float *ent_coef, float *g_logp, float *gq,
                                float *loss_out, float *loss_sum, int n_critics, int64_t batch, cstr_stream_t stream);

/* gSDE: generalized State-Dependent Exploration of SAC's actor (csrc/cstr_sde.hip; reference core/sac/policies.py:89-175,
 * core/common/distributions.py:421-617). latent = L (last hidden width, <= CSTR_SDE_MAX_LATENT), act_dim = A (<= CSTR_MAX_HEAD_ACT).
 * std [L][A] = get_std(log_std): exp, or expln when use_expln; log_std is [L][log_std_cols] with log_std_cols = A (full_std) or 1.
 * cstr_sde_draw_f32: mats[k][L][A] = z[k][L][A] * std for k < n_mats (Normal(0, std).rsample); z is drawn when rng_ctl is given
 *   (Philox4x32-10 stream of cstr_gaussian_head_fwd_f32's layout, the last workgroup advances rng_ctl[1]) and read otherwise; a drawn z
 *   is stored for the first z_keep (0..n_mats) matrices only (the rollout's per-env matrices need no z).
 *   std_out [L][A] is optional.
 * cstr_sde_head_fwd_f32: per row of h [batch][ldh]: pre = h W^T + b, mean = Hardtanh(pre, +-clip_mean) (none when clip_mean <= 0),
 *   x = mean + h M (M = mats + row * mat_stride: mat_stride 0 = one shared matrix; mats NULL = the mode), action = tanh(x),
 *   logp = sum Normal(mean, sqrt((h^2)(std^2) + 1e-6)).log_prob(atanh(clamp(action))) - sum log(1 - tanh(.)^2 + 1e-6).
 *   aux [batch][2A] (pre, variance) is what the backward needs; logp and aux are optional.
 * cstr_sde_head_bwd_f32: the autograd gradient of the forward (through the atanh round trip): g_pre / g_x / g_var [batch][A] (each
 *   optional) and dh [batch][L] (optional) times the activation gradient below_act (0 none, 1 ReLU, 2 tanh) of the layer that made h.
 * cstr_sde_param_grad_f32: dw_mu [A][L] = g_pre^T h, db_mu [A], dlog_std [L][log_std_cols] = std' * (z * h^T g_x + 2 std * (h^2)^T g_var)
 *   for a shared matrix M = z * std (z NULL: no noise term). */
#define CSTR_SDE_MAX_LATENT 4096
#define CSTR_SDE_MAX_MATS 65537
int cstr_sde_draw_f32(const float *log_std, int log_std_cols, int latent, int act_dim, int use_expln, int64_t n_mats, float *std_out,
                      float *z, int64_t z_keep, float *mats, uint64_t *rng_ctl, cstr_stream_t stream);
int cstr_sde_head_fwd_f32(const float *h, int64_t ldh, int64_t batch, int latent, int act_dim, const float *w_mu, const float *b_mu,
                          float clip_mean, const float *mats, int64_t mat_stride, const float *std_mat, float *action, int64_t action_stride,
                          float *logp, float *aux, cstr_stream_t stream);
int cstr_sde_head_bwd_f32(const float *g_action, int64_t g_action_stride, const float *g_logp, const float *action, int64_t action_stride,
                          const float *aux, const float *h, int64_t ldh, int64_t batch, int latent, int act_dim, const float *w_mu,
                          float clip_mean, const float *mats, int64_t mat_stride, const float *std_mat, int below_act, float *g_pre,
                          float *g_x, float *g_var, float *dh, cstr_stream_t stream);
int cstr_sde_param_grad_f32(const float *h, int64_t ldh, int64_t batch, int latent, int act_dim, const float *g_pre, const float *g_x,
                            const float *g_var, const float *z, const float *std_mat, const float *log_std, int log_std_cols, int use_expln,
                            float *dw_mu, float *db_mu, float *dlog_std, cstr_stream_t stream);

/* Deterministic-policy actor loss (core/td3/td3.py:194, core/maddpg/maddpg.py:174): loss = -mean(q), gq = -1/B. */
int cstr_neg_mean_loss_f32(const float *q, float *gq, float *loss_out, float *loss_sum, int64_t batch, cstr_stream_t stream);

/* ---- TD3+BC (csrc/cstr_td3bc.hip; core/td3bc/td3bc.py; Fujimoto & Gu 2021) -------------------------------------------------------
 * TD3's gradient step on a fixed dataset with one more term in the actor loss. Both entry points validate on the host without
 * dereferencing anything and then only enqueue; f32; deterministic and bit-identical on relaunch (no float atomics).
 *
 * cstr_td3bc_actor_loss_f32 (one launch, one 256-thread workgroup; it stands where TD3 launches cstr_neg_mean_loss_f32):
 *   lam  = alpha / (sum_b |q_b| / B)                         a constant of the batch: no gradient flows through it
 *   loss = -(lam * (sum_b q_b / B)) + sum_{b,j} (pi_bj - act_bj)^2 / (B * A)
 *   gq[b] = -(lam / B) for every row;  aux (3 floats, may be NULL) = {lam, -(lam * mean q), the second term}
 *   loss_out (may be NULL) is stored, loss_sum (may be NULL) accumulated: the loss heads' convention.
 * d(loss)/d(pi) = 2 (pi - act) / (B A) is NOT written here: cstr_td3bc_act_bwd_rows_f32 adds it where the gradient is consumed.
 * Reduction order: thread t of 256 sums rows t, t + 256, ... in ascending order (sum |q| in a first pass; sum q and, row by row with
 * the columns ascending, sum (pi - act)^2 in a second); each partial goes through a 64-lane shuffle tree (offsets 32, 16, ... 1),
 * the four wave sums combine as (s0 + s1) + (s2 + s3). The sums are accumulated in float64 (pi - act and its square are exact
 * there) and lam, gq, the two terms and the loss are each rounded to float32 once, lam first: the others follow from the float32
 * lam. sum |q| == 0 is not guarded: lam = alpha / 0 = inf (NaN for alpha == 0), gq = -inf, the Q term and the loss NaN -- what
 * the float32 torch statement gives (the published code's behaviour).
 * q [batch] contiguous; pi / act [batch][act_dim] with row strides ldpi / ldact >= act_dim floats (the action columns of packed critic
 * inputs), 4-byte aligned. CSTR_E_BADARG: NULL q / pi / act / gq, batch <= 0, act_dim <= 0, ld* < act_dim, a pointer off a 4-byte
 * boundary, alpha negative or NaN, an output overlapping an input or another output. CSTR_E_UNSUPPORTED: batch >
 * CSTR_TD3BC_MAX_BATCH, act_dim > CSTR_TD3BC_MAX_ACT.
 *
 * cstr_td3bc_act_bwd_rows_f32 (one launch; it stands where the deterministic actor's last layer launches cstr_bias_act_bwd_rows_f32):
 *   gz[m][n] = (gy[m][n] + coef * (y[m][n] - act[m][n])) * act'(y[m][n]),   coef = 2 / (B * A) for the loss above
 * with cstr_bias_act_bwd_rows_f32's expressions for act' (NONE: 1; RELU: y > 0; TANH: 1 - y * y) and its rounding points (the build
 * does not contract). coef == 0 adds nothing and is bit-identical to cstr_bias_act_bwd_rows_f32. gy / y / act are column blocks of
 * row-major matrices (row strides ldgy / ldy / ldact >= n floats, 4-byte aligned), gz is contiguous [m][n]; y is needed for every
 * act_kind. CSTR_E_BADARG: NULL pointers, m or n <= 0, ld* < n, a pointer off a 4-byte boundary, gz overlapping an input.
 * CSTR_E_UNSUPPORTED: an unknown act_kind, m or n beyond 32 bits. */
#define CSTR_TD3BC_MAX_BATCH CSTR_MAX_SAMPLE_BATCH /* 16384, as the other single-workgroup loss heads */
#define CSTR_TD3BC_MAX_ACT (2 * CSTR_MAX_HEAD_ACT)  /* 8: the widest row the action-head kernels handle (mean | log_std) */
int cstr_td3bc_actor_loss_f32(const float *q, const float *pi, int64_t ldpi, const float *act, int64_t ldact, float alpha, float *gq,
                              float *loss_out, float *loss_sum, float *aux, int64_t batch, int act_dim, cstr_stream_t stream);
int cstr_td3bc_act_bwd_rows_f32(const float *gy, int64_t ldgy, const float *y, int64_t ldy, const float *act, int64_t ldact, float coef,
                                int act_kind, float *gz, int64_t m, int64_t n, cstr_stream_t stream);

/* ---- CQL (csrc/cstr_cql.hip; core/cql/cql.py; Kumar et al. 2020, the importance-sampled CQL(H) term on SAC) -------------------------
 * SAC's gradient step on a fixed dataset with a conservative term in the critic loss. Both entry points validate on the host without
 * dereferencing anything and then only enqueue; f32; deterministic and bit-identical on relaunch (no float atomics). B = batch,
 * N = n_actions (<= CSTR_CQL_MAX_ACTIONS, so that a state's 3N + 1 entries fit the 64 lanes of a wave), D = obs_dim, A = act_dim.
 *
 * cstr_cql_candidates_f32 (one launch, one thread per output row): from obs [B][ldo] and the actor's distribution parameters
 * params_cur / params_next [B][ldp] = [mean | raw log_std] of s and s' it writes the critic-input rows
 *   x [B * 3N][ldx], row b * 3N + j = [obs_b | a_bj]:  j in [0, N) uniform in [-1, 1)^A, [N, 2N) ~ pi(.|s_b), [2N, 3N) ~ pi(.|s'_b)
 * (all three at the CURRENT state's observation) and, unless corr is NULL, the importance corrections
 *   corr [B][3N] = log_unif (= A * logf(0.5f), evaluated by the caller) | log pi(a_bj | s_b) | log pi(a_bj | s'_b).
 * A sampled action is sample_action_act(mean, raw, eps) and its log-prob sum_c gaussian_logp_term - sum_c tanh_correction_term
 * (csrc/cstr_gaussian_device.h), both sums over the action dimension in ascending c: the bits of cstr_gaussian_head_fwd_f32 for the
 * same (mean, raw, eps). Noise, exactly one source:
 *   u_in [B][N][A] (uniforms in [-1, 1), copied) AND eps_in [B][2N][A] (rows [0, N) for pi(.|s), [N, 2N) for pi(.|s')), or
 *   rng_ctl [CSTR_RNG_CTL_WORDS]: Philox4x32-10 keyed by rng_ctl[0] on CQL's own stream, counter words
 *     (lo32(c), hi32(c), sub, 0xC0175E4A) with c = rng_ctl[1] + b * N + k for sample k of state b (a 64-bit sum: carries into word 1):
 *     sub 0:     output word j -> column j of the uniform action, 2 * ((word >> 8) * 2^-24) - 1
 *                (cstr_collect_episodes_f32's conversion);
 *     sub 1 + p: Box-Muller(words 0, 1) -> eps of columns 2p, 2p + 1 of the pi(.|s) sample,
 *                Box-Muller(words 2, 3) -> eps of columns 2p, 2p + 1 of the pi(.|s') sample (cstr_gaussian_head_fwd_f32's Box-Muller).
 *   The last workgroup advances rng_ctl[1] by B * N (cstr_bcq_expand_f32's ticket), so a graph replay continues the stream.
 * CSTR_E_BADARG: NULL obs / params / x, sizes <= 0, ldo < D, ldp < 2A, ldx < D + A, a pointer off a 4-byte boundary (rng_ctl: 8),
 * both or neither noise source (u_in without eps_in counts as neither), an output overlapping an input or the other output.
 * CSTR_E_UNSUPPORTED: A > CSTR_MAX_HEAD_ACT, N > CSTR_CQL_MAX_ACTIONS, more than CSTR_BCQ_MAX_ROWS output rows.
 *
 * cstr_cql_q_loss_f32 (one launch, one 1024-thread workgroup; everything between the critic forward and its backward):
 *   q [2][q_stride]: each critic's output over the (1 + 3N) B rows [B data rows | B * 3N candidate rows in x's order].
 *   t_b      = rew_b + (1 - done_b) * gamma * (min(q1_t_b, q2_t_b) - ent_coef[0] * next_logp_b)   (no entropy term when next_logp is
 *              NULL): cstr_td_twin_q_loss_f32's statement and rounding points, target_out [B] (may be NULL) has its bits
 *   c_i[b,j] = q_i[B + b 3N + j] - corr[b][j]   (corr NULL: no correction; with_data = 1 appends c_i[b,3N] = q_i[b]; corr NULL needs it)
 *   lse_i[b] = temp * (log(sum_j exp(c_i[b,j] / temp - m)) + m),  m = max_j c_i[b,j] / temp  (an infinite m counts as 0; a NaN entry
 *              makes that state's lse, its softmax shares and the loss NaN, as torch.logsumexp)
 *   loss     = 0.5 * sum_i [ mean_b (q_i[b] - t_b)^2 + w * (mean_b lse_i[b] - mean_b q_i[b]) ]
 *   gq [2][(1 + 3N) B] = d loss / d q:  data rows (0.5 * 2 / B) * (q_i[b] - t_b) - (0.5 w) / B (+ ((0.5 w) / B) * softmax share of the
 *              appended entry when with_data), candidate rows ((0.5 w) / B) * softmax_j(c_i[b,:] / temp). No batch mean enters a
 *              gradient; w == 0 leaves exact zeros on the candidate rows and cstr_td_twin_q_loss_f32's bits (scale 0.5) on the data rows.
 *   loss_out (may be NULL) is stored, loss_sum (may be NULL) accumulated: the loss heads' convention.
 *   aux [4] (may be NULL) = {0.5 sum_i mean_b (q_i - t)^2,  0.5 w sum_i (mean_b lse_i - mean_b q_i),  mean_b mean_i lse_i,
 *              mean_b mean_i q_i[b]}: loss = aux[0] + aux[1] up to the final rounding.
 * Reduction order: wave v of the sixteen takes the states v, v + 16, ... in ascending order, both critics side by side; a state's entries
 * sit in lanes 0 .. 3N (maximum and sum through xor-shuffle butterflies, offsets 32, 16, ... 1); each wave adds (q_i - t)^2, lse_i and q_i
 * of its states to float64 sums; the sixteen wave sums of a quantity combine in a binary tree (neighbours s0 + s1, s2 + s3, ..., then
 * pairs of pairs, ...), and loss / aux are rounded to float32 once.
 * CSTR_E_BADARG: NULL q / q1_t / q2_t / rew / done / gq, batch or n_actions <= 0, with_data not 0 / 1, corr NULL with with_data 0,
 * next_logp without ent_coef, w negative or NaN, temp <= 0 or NaN, gamma NaN, q_stride < (1 + 3N) B, a pointer off a 4-byte
 * boundary, an output overlapping an input or another output. CSTR_E_UNSUPPORTED: N > CSTR_CQL_MAX_ACTIONS, batch >
 * CSTR_MAX_SAMPLE_BATCH. */
#define CSTR_CQL_MAX_ACTIONS 21 /* 3 * 21 + 1 = 64 entries: one wave */
int cstr_cql_candidates_f32(const float *obs, int64_t ldo, const float *params_cur, const float *params_next, int64_t ldp, int64_t batch,
                            int n_actions, int obs_dim, int act_dim, const float *u_in, const float *eps_in, uint64_t *rng_ctl,
                            float log_unif, float *x, int64_t ldx, float *corr, cstr_stream_t stream);
int cstr_cql_q_loss_f32(const float *q, int64_t q_stride, const float *corr, int with_data, const float *q1_t, const float *q2_t,
                        const float *next_logp, const float *rew, const float *done, const float *ent_coef, float gamma, float w,
                        float temp, float *target_out, float *gq, float *loss_out, float *loss_sum, float *aux, int64_t batch,
                        int n_actions, cstr_stream_t stream);

/* ---- IQL (csrc/cstr_iql.hip; core/iql/iql.py; Kostrikov, Nair & Levine 2021, implicit Q-learning) ---------------------------------
 * cstr_iql_loss_f32 (one launch, one 256-thread workgroup): everything between the forward passes of an IQL gradient step and its
 * three backward passes. It validates on the host without dereferencing anything and then only enqueues; f32; deterministic and
 * bit-identical on relaunch (no float atomics). B = batch, A = act_dim, tau_e = expectile, M = exp_adv_max. Per row b:
 *   u      = min(qt1_b, qt2_b) - v_b                                  (the target critics at (s, a), V(s)); adv_out [B]
 *   value  : we = |tau_e - 1[u < 0]| (u == 0 and a NaN u take tau_e);  term we * u^2;  g_v[b] = -(2 we u) / B
 *   critic : y = rew_b + (1 - done_b) * gamma * v_next_b;  gq_i[b] = (0.5 * 2 / B) * (q_i[b] - y);  target_out [B] = y.
 *            This is cstr_td_twin_q_loss_f32's statement, rounding points and float32 reduction (csrc/cstr_td_device.h is the one
 *            place that states them): fed v_next as both target values, no next_logp and scale 0.5, that launch's gq1, gq2,
 *            target_out and loss have this launch's bits.
 *   actor  : w = min(exp(beta * u), M), a constant of the actor step (an overflowing exp is clipped to M, a NaN stays a NaN);
 *            params [B][ldp] = [mean | raw log_std], ls = clamp(raw, -20, 2), sd = exp(ls);  act [B][ldact] the dataset action;
 *            g_j = atanh(clamp(act_j, -1 + eps32, 1 - eps32)) = 0.5 * (log1p(x) - log1p(-x)), eps32 = 2^-23;
 *            logp = sum_j [-(g_j - mean_j)^2 / (2 sd_j^2) - log(sd_j) - 0.5 log(2 pi)] - sum_j log(1 - act_j^2 + 1e-6)
 *            (csrc/cstr_gaussian_device.h's terms, two sums in ascending j; the correction takes the UNclamped action, so |act_j| > 1
 *            gives NaN in that row's logp, as torch; it is not guarded); logp_out [B];
 *            g_params [B][2A] (contiguous): mean columns -(w / B) * ((g_j - mean_j) / sd_j^2), raw log_std columns
 *            -(w / B) * ((g_j - mean_j)^2 / sd_j^2 - 1) where -20 <= raw <= 2 (torch's clamp passes the gradient on the closed
 *            interval), else 0 (a NaN raw included).
 *   loss_out [3] (stored) / loss_sum [3] (accumulated) = {mean_b we u^2,  0.5 sum_i mean_b (q_i - y)^2,  mean_b -(w logp)}
 *   aux [6] = {mean u, mean w, share of rows with exp(beta u) > M, mean logp, mean v, mean y}
 * Optional, each group as a whole (NULL = not written): g_v; (gq1, gq2) together; g_params; loss_out; loss_sum; aux; target_out;
 * adv_out; logp_out. Every input is required: the three losses and aux are always evaluated.
 * v and v_next may be the two halves of one [2B] array (V's ONE forward on [s; s']).
 * Reduction order: thread t of 256 sums rows t, t + 256, ... in ascending order; each partial goes through a 64-lane shuffle tree
 * (offsets 32, 16, ... 1), the four wave sums combine as (s0 + s1) + (s2 + s3). The critic's two sums of (q_i - y)^2 are float32 (the
 * twin TD loss head's bits); all others are float64 sums of float32 values (products of float32 factors formed in float64), each
 * result rounded to float32 once.
 * All vectors [B] contiguous; params / act rows on 4-byte boundaries with ldp >= 2A, ldact >= A floats.
 * CSTR_E_BADARG: a NULL input, batch or act_dim <= 0, ldp < 2A, ldact < A, one of gq1 / gq2 without the other, a pointer off a
 * 4-byte boundary, an output overlapping an input or another output, expectile outside (0, 1) or NaN, beta negative or NaN,
 * exp_adv_max <= 0 or NaN. CSTR_E_UNSUPPORTED: batch > CSTR_IQL_MAX_BATCH, act_dim > CSTR_MAX_HEAD_ACT. */
#define CSTR_IQL_MAX_BATCH CSTR_MAX_SAMPLE_BATCH /* 16384, as the other single-workgroup loss heads */
int cstr_iql_loss_f32(const float *qt1, const float *qt2, const float *v, const float *v_next, const float *q1, const float *q2,
                      const float *params, int64_t ldp, const float *act, int64_t ldact, const float *rew, const float *done, float gamma,
                      float expectile, float beta, float exp_adv_max, float *g_v, float *gq1, float *gq2, float *g_params,
                      float *loss_out, float *loss_sum, float *aux, float *target_out, float *adv_out, float *logp_out, int64_t batch,
                      int act_dim, cstr_stream_t stream);

/* ---- TQC (csrc/cstr_tqc.hip; core/tqc/tqc.py; Kuznetsov et al. 2020, truncated quantile critics) ----------------------------------
 * What lies between the critics' forward passes of a TQC gradient step and its backward passes. Both entry points validate on the
 * host without dereferencing anything and then only enqueue; f32 in and out, float64 inside; deterministic and bit-identical on
 * relaunch (no float atomics, no workgroup waiting for another). G = n_critics, Nq = n_quantiles, k = drop_per_net, B = batch,
 * M = G * Nq atoms per state, n_keep = M - k * G, tau_i = (i + 0.5) / Nq. Atom tensors are [G][B][Nq] contiguous (the stacked critic
 * output).
 * cstr_tqc_supported: 1 <= G <= CSTR_MAX_ENS_CRITICS, Nq >= 1, M <= CSTR_TQC_MAX_ATOMS, 0 <= k < Nq.
 * cstr_tqc_critic_loss_f32 (two launches: one workgroup per row, then one workgroup over the per-row sums in ws):
 *   per row b: the M atoms of z_next are ranked, rank_m = #{j : z'_j < z'_m or (z'_j == z'_m and j < m)} with j, m = g * Nq + i; the
 *   n_keep atoms of rank < n_keep are kept (exactly n_keep, whatever ties there are), and
 *     y_rank = rew_b + (1 - done_b) * gamma * (z' - alpha * next_logp_b);   target_out [B][n_keep] = y, ascending in each row;
 *   alpha = exp(log_alpha[0]) when the entropy-coefficient part rides along (its value BEFORE this step's update), else ent_coef[0].
 *   For every atom z_m of the row and every y_j: delta = y_j - z_m, H = 0.5 delta^2 if |delta| <= 1 else |delta| - 0.5,
 *     rho = |tau_i - 1[delta < 0]| * H;   loss = mean over (b, m, j) of rho;
 *     gz[m] = -(1 / (B M n_keep)) * sum_j |tau_i - 1[delta < 0]| * clamp(delta, -1, 1)       (j ascending)
 *   loss_out [1] (stored) / loss_sum [1] (accumulated); means_out [2] (stored) / means_sum [2] (accumulated) = {mean over (b, j) of y,
 *   mean over (b, m) of z}. Every difference, Huber term and sum is float64 on the float32 inputs; each output is rounded to
 *   float32 once. ws: double [3 * B] scratch (the per-row sums), 8-byte aligned. `alpha` (NULL or log_alpha NULL = absent): SAC's
 *   entropy-coefficient part as in cstr_td_twin_q_loss_f32, here with a float64 mean and exp.
 *   Reduction order: a row's lanes through a 64-lane shuffle tree (offsets 32 .. 1), wave sums in wave order; rows t, t + 256, ...
 *   in ascending order on lane t of the finishing workgroup, the same tree.
 *   Optional (NULL = not written): loss_out, loss_sum, target_out, means_out, means_sum, alpha.
 *   CSTR_E_BADARG: a NULL required pointer, batch <= 0, G or Nq <= 0, k < 0 or k >= Nq, gamma negative or NaN, neither ent_coef nor
 *   the alpha part, an incomplete alpha part, a pointer off a 4-byte (ws: 8-byte) boundary, an output overlapping an input or another
 *   output. CSTR_E_UNSUPPORTED: not cstr_tqc_supported, batch > CSTR_MAX_SAMPLE_BATCH.
 * cstr_tqc_actor_loss_f32 (one launch, one 256-thread workgroup): loss = mean_b(ent_coef * logp_b - mean_{g,i} z_pi[g][b][i]);
 *   gz_pi [G][B][Nq] = -1 / (B M), g_logp [B] = ent_coef / B, z_pi_mean [B] (optional) the row means; loss_out / loss_sum [1] optional.
 *   Lane t sums rows t, t + 256, ... (each row's atoms in (g, i) order), then the tree above. Errors as above. */
#define CSTR_TQC_MAX_ATOMS 256
int cstr_tqc_supported(int n_critics, int n_quantiles, int drop_per_net);
int cstr_tqc_critic_loss_f32(const float *z, const float *z_next, const float *next_logp, const float *rew, const float *done,
                             const float *ent_coef, double gamma, int n_critics, int n_quantiles, int drop_per_net, float *gz,
                             float *loss_out, float *loss_sum, float *target_out, float *means_out, float *means_sum, double *ws,
                             const cstr_alpha_part_t *alpha, int64_t batch, cstr_stream_t stream);
int cstr_tqc_actor_loss_f32(const float *z_pi, const float *logp, const float *ent_coef, int n_critics, int n_quantiles, float *gz_pi,
                            float *g_logp, float *loss_out, float *loss_sum, float *z_pi_mean, int64_t batch, cstr_stream_t stream);

/* cstr_linear_bwd_weight_sets_f32 with the OPTIMISER STEP inside (single-GPU training: no collective sits between a gradient and
 * its Adam step; torch.optim.Adam's arithmetic, core/sac/sac.py:266-268, :279-281): the workgroup that has reduced a 16 x 16 tile of
 * dW (and db) applies Adam to exactly those parameters -- parameter / moment quads requested at entry, one launch instead of two.
 * dw / db are still written (the gradient arena stays inspectable). `flat` (n_flat <= 4): segments WITHOUT a weight-gradient tile
 * in the same launch -- Adam over a flat range (SAC's entropy coefficient, whose gradient an earlier launch wrote) or a soft target
 * update (polyak_source set) of parameters this launch does not change.
 * Every step counter must have been advanced by an EARLIER launch (cstr_chain_root_t.adam_advance: state["step"] += 1 and the
 * running beta powers): this launch only reads adam_ctl and writes no control word (no last-workgroup ticket). m > 32 rows. */
typedef struct cstr_adam_opt {
    const int64_t *adam_ctl; /* {step, ticket, beta1^step, beta2^step (f64 bits)} AFTER this step's increment */
    const double *lr;        /* [1] */
    double beta1, beta2, eps;
    float grad_scale;
    int32_t reserved;
} cstr_adam_opt_t;
typedef struct cstr_wgrad_adam_set {
    cstr_wgrad_set_t g;      /* the gradient part: dz, x, ldx, dw, db, m, n, k */
    float *w, *w_m, *w_v;    /* the weight [n][k] and its exp_avg / exp_avg_sq */
    float *b, *b_m, *b_v;    /* the bias [n] and its moments (with g.db) */
    float *shadow;           /* tile-major copy of w kept current (cstr_policy_swizzle_f32's layout) or NULL */
    int32_t opt, reserved;   /* index into opts */
    float *w_target, *b_target; /* these parameters' OWN target (soft update with the values just computed,
                                   core/common/utils.py:478-481: target = tau * p + (1 - tau) * target) or NULL */
    float tau, reserved2;
} cstr_wgrad_adam_set_t;
int cstr_linear_bwd_weight_adam_sets_f32(const cstr_wgrad_adam_set_t *sets, int n_sets, const cstr_adam_opt_t *opts, int n_opts,
                                         const cstr_adam_seg_t *flat, int n_flat, cstr_stream_t stream);
/* Test hooks of that launch. It has two kernels that write the same bits: a lean one (slice lookup from preloaded registers, one
 * record per set, every wave a share of the tile's optimiser step, a body chosen per workgroup) and the one it replaced.
 * cstr_wgrad_adam_lean(on): on = 0 launches the earlier kernel from now on, on > 0 the lean one (the default), on < 0 changes
 * nothing; returns the setting before the call. A launch of 65535 workgroups or more always takes the earlier kernel.
 * cstr_wgrad_adam_tile_body: the body the lean kernel runs for tile (tile_n, tile_k) of an [n][k] gradient reduced over m rows:
 * 0 full (m = 256, tile complete in n and k), 1 k-narrow (k <= 16, complete in n), 2 n-narrow (n <= 16, complete in k),
 * 3 generic (every other tile: the earlier kernel's tile body). */
int cstr_wgrad_adam_lean(int on);
int cstr_wgrad_adam_tile_body(int64_t m, int64_t n, int64_t k, int64_t tile_n, int64_t tile_k);

/* ---- row-chain kernels: a gradient step's forward / backward chains with FEWER launch boundaries ------------------------------
 * A chain of Linear layers is row-local (row r of layer l+1 needs row r of layer l only), but a launch boundary is the cheapest
 * way on this chip to hand data between workgroups (an in-kernel cross-workgroup barrier costs 4-17 us, an empty dependent launch
 * 1.6 us: tools/probes/cluster_chain_probe.hip, profiles/r03_notes.md). These kernels cut boundaries WITHOUT any hand-over inside a
 * launch: a workgroup owns 16 batch rows x one column group of the chain's WIDE layer (one f32-MFMA tile pass over K), RECOMPUTES
 * the cheap layer in front of it (K = obs_dim (+ act_dim) <= 12 inputs, or an element-wise function of stored activations), and
 * leaves the NARROW layer behind it (a Q head's H2 -> 1 dot product, the actor head's H2 -> 2A, the first layer's input gradient
 * H1 -> act_dim) as per-column-group PARTIAL sums that the next launch adds up in a fixed order in its prologue.
 * SAC.train (core/sac/sac.py:215-287) = 10 launches instead of 20; everything is deterministic (no float atomics).
 * Networks: create_mlp(in, out, [H1, H2], ReLU) (core/common/torch_layers.py:110-183); H1, H2 multiples of 4, <= 512; batch a
 * multiple of 16, <= 1024; (obs_dim, act_dim) as the ring's layouts. `tiles` = 16-column tiles per workgroup (1, 2 or 4). */
#define CSTR_CHAIN_MAX_NETS 16
#define CSTR_CHAIN_MAX_WIDTH 512

/* One Q network Linear(W, H1)-ReLU-Linear(H1, H2)-ReLU-Linear(H2, 1) (core/common/policies.py:960-987) of a chain launch. */
typedef struct cstr_chain_net {
    const float *w1, *b1, *w2, *b2, *w3, *b3; /* [H1][W], [H1], [H2][H1], [H2], [H2], [1] */
    const float *x;                            /* forward: this network's input rows [batch][W] (ld = W) */
    float *h1, *h2;                            /* [batch][H1], [batch][H2] post-activation: forward = written when not NULL (kept for
                                                  the backward); backward = read */
    float *q_part;                             /* [n_colgroups][batch] partial head sums (forward: out; backward: in) */
    int32_t role, reserved;                    /* forward, see CSTR_CHAIN_ROLE_* */
} cstr_chain_net_t;
#define CSTR_CHAIN_ROLE_PLAIN 0      /* x is complete */
#define CSTR_CHAIN_ROLE_STORE_PI 1   /* x is complete; the column-group-0 workgroups ALSO finalise the actor head of the pi(obs) rows
                                        and store x_pi's action columns, params, logp_pi (a side job: nothing here reads them) */
#define CSTR_CHAIN_ROLE_NEXT 2       /* x = x_next whose ACTION columns are not written yet: every workgroup finalises the actor head
                                        of its pi(next_obs) rows for itself */
#define CSTR_CHAIN_ROLE_NEXT_STORE 3 /* ... and the column-group-0 workgroups store them (x_next action columns, logp_next) */
#define CSTR_CHAIN_ROLE_PI 4         /* x = x_pi whose ACTION columns are not written yet (a deterministic actor's loss pass): finalised
                                        by every workgroup for itself, stored by the column-group-0 workgroups */
/* rows of an actor chain pass */
#define CSTR_CHAIN_ROWS_PAIR 0 /* [obs rows | next_obs rows], 2B rows: SAC's pi(obs) and pi(next_obs) */
#define CSTR_CHAIN_ROWS_NEXT 1 /* next_obs rows, B rows: a target actor (core/td3/td3.py:171) */
#define CSTR_CHAIN_ROWS_OBS 2  /* obs rows, B rows, activations kept: the deterministic actors' loss pass (core/td3/td3.py:194) */
/* head of the actor */
#define CSTR_CHAIN_HEAD_GAUSSIAN 0      /* [mu | log_std] (H2, 2A) + squashed-Gaussian sampling (core/sac/policies.py:147-175) */
#define CSTR_CHAIN_HEAD_DETERMINISTIC 1 /* Linear(H2, A) + Tanh (core/td3/policies.py:57-83) */

/* SAC actor Linear(D, H1)-ReLU-Linear(H1, H2)-ReLU-[mu | log_std](H2, 2A) (core/sac/policies.py:84-175), heads merged. */
typedef struct cstr_sac_actor {
    int32_t obs_dim, act_dim, h1, h2;
    const float *w1, *b1, *w2, *b2, *hw, *hb; /* hw [head_n][H2], hb [head_n]: head_n = 2A (Gaussian) or A (deterministic) */
} cstr_sac_actor_t;

/* SAC.train's actor passes pi(obs) (core/sac/sac.py:222) and pi(next_obs) (:247) as ONE launch over 2B rows (rows [0, B) = obs,
 * [B, 2B) = next_obs): ReplayBuffer.sample's gather (sample_idx = the (row, env) pairs drawn by cstr_rollout_step_f32, or NULL:
 * the observation columns of x_pi / x_next are already filled) + layer 1 (recomputed per workgroup) + layer 2 (one MFMA column
 * group per workgroup) + PARTIAL head sums head_part [n_colgroups][2B][2A] (n_colgroups = ceil(H2 / (16 * tiles))). With sample_idx
 * the column-group-0 workgroups also materialise the packed batch (cstr_linear_act_fwd_gather_f32's contract: x_data, the
 * observation columns of x_pi / x_next, rewards, dones * (1 - timeouts)) and thread 0 advances the ring position.
 * a_h1 [B][H1], a_h2 [B][H2]: the pi(obs) rows' activations, kept for cstr_sac_actor_chain_bwd_f32.
 * eps_all [2B][A] (or NULL): the sampling head's noise, drawn HERE by an otherwise idle wave (Philox4x32-10 / Box-Muller, key =
 * head_rng_ctl[0], counter = head_rng_ctl[1] + head_rng_offset + row, row in [0, 2B): the stream positions of
 * cstr_gaussian_head_gemm_fwd_f32 on the 2B-row pass) -- it does not depend on the network, and the launch that finalises the head has
 * a long enough prologue without it. head_rng_offset: draws of an earlier launch on the same stream whose offset advance is still
 * pending (cstr_rollout_step_f32 leaves it to the launches behind it). head_rng_ctl is only READ in this launch; the backward chain
 * launch advances the offset by everything that is pending (cstr_chain_root_t.rng_ctl). */
int cstr_sac_actor_chain_fwd_f32(const cstr_sac_actor_t *actor, const cstr_ring_t *ring, int64_t *ring_ctl, int advance_ring,
                                 const int32_t *sample_idx, int64_t batch, float *x_data, float *x_pi, float *x_next, float *out_done,
                                 float *out_rew, float *a_h1, float *a_h2, float *head_part, const uint64_t *head_rng_ctl,
                                 uint64_t head_rng_offset, float *eps_all, int rows_mode, int head_n, int tiles, cstr_stream_t stream);

/* How a consumer launch turns the actor's head partials into actions (core/common/distributions.py:207-260, the arithmetic of
 * cstr_gaussian_head_gemm_fwd_f32): params = sum of partials + hb; u = mean + exp(clamp(log_std)) * eps; a = tanh(u); log-prob.
 * eps [2B][A]: the actor chain launch's eps_all, or teacher-forced draws. */
typedef struct cstr_sac_head_fin {
    const float *head_part; /* [n_parts][part_rows][head_n] */
    const float *hb;        /* [head_n] */
    const float *eps;       /* [part_rows][A] standard normal draws (or teacher-forced noise); deterministic head: may be NULL (no noise) */
    int32_t n_parts, act_dim, obs_dim, kind; /* kind: CSTR_CHAIN_HEAD_* */
    int32_t part_rows, next_offset;          /* rows of the actor pass; row of batch element b: pi rows b, next rows next_offset + b */
    float sigma, clip;      /* deterministic head, next rows: a' = clamp(tanh(.) + clamp(sigma * eps, -clip, clip), -1, 1)
                               (target policy smoothing, core/td3/td3.py:167-171) */
    float *x_pi, *x_next;   /* [B][D + A]: action columns written by the STORE roles */
    float *params, *logp_pi, *logp_next; /* Gaussian head: [B][2A], [B], [B] */
} cstr_sac_head_fin_t;

/* Forward of n_nets <= 16 Q networks on `batch` rows each in ONE launch (16: every agent's critic and target critic of a 4-agent MADDPG
 * step without a policy update, core/maddpg/maddpg.py:146-164): layer 1 recomputed per workgroup (K = W <= 12), layer 2 one
 * MFMA column group per workgroup, head as partial sums q_part [n_colgroups][batch]. SAC / TD3 critic step: nets 0, 1 = the critic on
 * x_data, nets 2, 3 = the target on x_next (core/sac/sac.py:250, :258; core/td3/td3.py:173, :179); actor loss: the critic on x_pi
 * (:273). `fin` (or NULL): the SAC actor's pending head (roles above). */
int cstr_q_chain_fwd_f32(const cstr_chain_net_t *nets, int n_nets, int w_in, int obs_dim, int h1, int h2, int64_t batch,
                         const cstr_sac_head_fin_t *fin, int tiles, cstr_stream_t stream);

/* Loss root + backward of the twin Q networks in ONE launch (what cstr_hidden_head_bwd_root_f32 + cstr_linear_bwd_input_f32 did in
 * two or three): per workgroup q = sum of partials + b3, d(loss)/dq of its 16 rows (cstr_head_root_t's modes and arithmetic:
 * 1 = TD critic loss, 2 = SAC actor loss, 3 = -mean(Q1)), dz2 = dq * w3 * relu'(h2) recomputed (element-wise), one MFMA column group
 * of dz1 = (dz2 W2) * relu'(h1), and -- when gact_part is given (the actor loss: the critic is frozen) -- partial sums of
 * d(loss)/d(action) = dz1 W1[:, obs_dim:], gact_part [n_nets][n_colgroups][batch][A]. ONE extra workgroup does the batch reductions
 * (logged loss, entropy-coefficient part) and advances the actor's Philox offset. */
typedef struct cstr_chain_root {
    int32_t mode, batch;
    float gamma, scale;
    const float *q_part[4]; /* nets 0, 1: q1 / q2 (the differentiated networks); 2, 3: q1_t / q2_t (mode 1) */
    const float *b3[4];
    int32_t n_parts, reserved;
    const float *next_logp, *rew, *done;  /* mode 1 */
    const float *ent_coef;                /* [1]: mode 1 without alpha part, mode 2 */
    const float *logp;                    /* mode 2: log pi(a|obs) */
    float *target_out;                    /* mode 1, [batch] or NULL */
    float *q_out;                         /* [2][batch] finalised q1 / q2 (mode 3: [1][batch]) or NULL */
    float *gq_out;                        /* [2][batch] d(loss)/dq (the head's dW3 / db3 operand) or NULL */
    float *loss_out, *loss_sum;           /* [1] or NULL */
    cstr_alpha_part_t alpha;              /* mode 1: log_alpha NULL = absent */
    uint64_t *rng_ctl;                    /* or NULL: rng_ctl[1] += rng_advance by the loss workgroup */
    uint64_t rng_advance;
    /* Adam control words the loss workgroup advances on behalf of the optimiser launch behind this one (state["step"] += 1,
     * beta^step *= beta: cstr_linear_bwd_weight_adam_sets_f32 reads them pre-advanced); NULL = none */
    int64_t *adam_advance[2];
    double adam_beta1[2], adam_beta2[2];
} cstr_chain_root_t;
int cstr_q_chain_bwd_f32(const cstr_chain_net_t *nets, int n_nets, const cstr_chain_root_t *root, int w_in, int obs_dim, int h1, int h2,
                         float *dz2, float *dz1, float *gact_part, int tiles, cstr_stream_t stream);
/* Test hook of the two Q launches above. Each has two kernels that write the same bits: the generic one (run-time widths, loss mode,
 * head kind and partial-sum count) and a lean one for 256 x 256 networks on the (4, 2) and (8, 2) layouts whose partial-sum requests
 * run on arguments that arrive with the wave, whose remaining arguments are one batch of scalar reads, and whose loss mode, head kind,
 * store set and partial-sum bucket are fixed at compile time. Lean instantiations exist for what the learners dispatch -- forward:
 * no pending head, Gaussian, deterministic; backward: mode 1 with the alpha part and next_logp, with next_logp and ent_coef, with
 * neither (each storing dz1 and dz2), modes 2 and 3 (storing gact_part) -- with at most 16 partial sums; every other launch runs the
 * generic kernel whatever the switch says.
 * cstr_chain_lean(on): on = 0 launches the generic kernels from now on, on > 0 the lean ones where they exist (the default), on < 0
 * changes nothing; returns the setting before the call. */
int cstr_chain_lean(int on);

/* out[row * out_stride + col] = sum over p < n_parts of part[p][row][col] (p ascending): the finalisation of a chain launch's partial
 * sums for a consumer that is not a chain kernel -- MADDPG's per-layer actor backward (core/maddpg/maddpg.py:174-179) reads
 * d(loss)/d(action) from the action columns of a critic-input gradient. */
int cstr_chain_sum_parts_f32(const float *part, int n_parts, int64_t rows, int cols, float *out, int64_t out_stride, cstr_stream_t stream);

/* Backward of the SAC actor from the critic's action-gradient partials in ONE launch (cstr_gaussian_head_bwd_input_f32 +
 * cstr_linear_bwd_input_f32): d(loss)/d(action) = sum of gact_part over networks and column groups; d(loss)/d(logp) = ent_coef / B
 * (core/sac/sac.py:275); the squashed-Gaussian head's analytic backward -> g_params [B][2A]; dz2 = (g_params hw) * relu'(a_h2)
 * recomputed (2A terms per element); one MFMA column group of dz1 = (dz2 W2) * relu'(a_h1).
 * kind = CSTR_CHAIN_HEAD_DETERMINISTIC (core/td3/td3.py:194-199): g_params [B][A] = d(loss)/d(action) * (1 - a^2) (the Tanh); ent_coef,
 * params and eps are not read. */
int cstr_sac_actor_chain_bwd_f32(const cstr_sac_actor_t *actor, const float *gact_part, int n_nets, int n_parts, const float *ent_coef,
                                 const float *x_pi, const float *params, const float *eps, const float *a_h1, const float *a_h2,
                                 float *g_params, float *dz2, float *dz1, int64_t batch, int kind, int tiles, cstr_stream_t stream);

/* ---- BCQ: the arithmetic around the Linear layers of an offline gradient step (core/bcq/bcq.py:137-213) ---------------------------
 * Row-major f32 operands; `ld*` = row stride in floats (a column block of a wider matrix is fine). Each entry point validates on the
 * host (NULL, sizes, strides, overlapping input / output rows -> CSTR_E_BADARG; latent > CSTR_BCQ_MAX_LATENT, act_dim >
 * CSTR_BCQ_MAX_ACT, samples > CSTR_BCQ_MAX_SAMPLES, more than CSTR_BCQ_MAX_ROWS rows -> CSTR_E_UNSUPPORTED), then only enqueues.
 * Noise: exactly one of a noise array (read) or rng_ctl [CSTR_RNG_CTL_WORDS] (drawn: Philox4x32-10 + Box-Muller on BCQ's own
 * stream tag, element pair p uses counter rng_ctl[1] + p; the last workgroup advances rng_ctl[1] by the pairs drawn).
 * cstr_bcq_latent_fwd_f32 (core/bcq/policies.py:76-85): params [batch][ldp] = [mean | log_std_raw] (2 latent columns);
 *   std = exp(clamp(log_std_raw, -4, 15)); xdec [batch][ldx] = [obs | mean + std * eps]; std_out, eps_out [batch][latent] for the
 *   backward (eps_out optional when eps_in is given).
 * cstr_bcq_vae_loss_f32 (bcq.py:145-149): loss = mse(recon, act) + 0.5 * (-0.5 * mean(1 + log(std * std) - mean^2 - std^2));
 *   g_recon [batch][act_dim], g_mean / g_std [batch][latent] (the KL term's gradients) -- each optional; loss_out[0] = loss,
 *   loss_sum[0] += loss (each optional).
 * cstr_bcq_latent_bwd_f32: g_params [batch][2 latent] = [g_z + g_mean_kl | (g_z * eps + g_std_kl) * std where -4 <= log_std_raw <= 15,
 *   else 0]; g_z [batch][ldg] (the latent columns of the decoder input's gradient), g_mean_kl, g_std_kl: each optional, not all NULL.
 * cstr_bcq_expand_f32 (policies.py:122-124, :247; bcq.py:164): rows = n_states * samples; xdec row r = [state[r % n_states] |
 *   clamp(noise, -clip, clip)]; xa / xb (optional, [rows][ld]): their first obs_dim columns = state[r % n_states].
 * cstr_bcq_perturb_fwd_f32 (policies.py:165-166): out = clamp(a_vae + p * max_perturbation, -1, 1).
 * cstr_bcq_perturb_bwd_f32: g_p [rows][act_dim] = g_out * max_perturbation where the clamp is inactive (closed interval), else 0.
 * cstr_bcq_target_f32 (bcq.py:167-173): q [n_critics][q_stride], rows = n_states * samples in [sample][state] order; per row the min
 *   over the critics, then per state i the max over a group of `samples` rows: grouping 0 = rows samples * i ... samples * i +
 *   samples - 1 (the reference's reshape(B, samples)), grouping 1 = rows i + n_states * s (the state's own candidates);
 *   max_q_out[i] = that (optional), target_out[i] = rew[i] + (1 - done[i]) * gamma * that (optional; needs rew, done).
 * cstr_bcq_select_f32 (policies.py:429-435, per state): index_out[i] (optional) = the row i + n_states * s with the largest q1
 *   (first maximum wins), action_out [n_states][act_dim] = cand[that row]. */
#define CSTR_BCQ_MAX_LATENT 256
#define CSTR_BCQ_MAX_ACT 64
#define CSTR_BCQ_MAX_SAMPLES 4096
#define CSTR_BCQ_MAX_ROWS 16777216
int cstr_bcq_latent_fwd_f32(const float *params, int64_t ldp, const float *obs, int64_t ldo, const float *eps_in, uint64_t *rng_ctl,
                            float *xdec, int64_t ldx, float *std_out, float *eps_out, int64_t batch, int obs_dim, int latent,
                            cstr_stream_t stream);
int cstr_bcq_vae_loss_f32(const float *recon, int64_t ldr, const float *act, int64_t lda, const float *params, int64_t ldp,
                          const float *std, int64_t batch, int act_dim, int latent, float *g_recon, float *g_mean, float *g_std,
                          float *loss_out, float *loss_sum, cstr_stream_t stream);
int cstr_bcq_latent_bwd_f32(const float *g_z, int64_t ldg, const float *g_mean_kl, const float *g_std_kl, const float *params, int64_t ldp,
                            const float *std, const float *eps, float *g_params, int64_t batch, int latent, cstr_stream_t stream);
int cstr_bcq_expand_f32(const float *state, int64_t lds, int64_t n_states, int samples, int obs_dim, int latent, const float *noise,
                        uint64_t *rng_ctl, float clip, float *xdec, int64_t ldx, float *xa, int64_t lda, float *xb, int64_t ldb,
                        cstr_stream_t stream);
int cstr_bcq_perturb_fwd_f32(const float *a_vae, int64_t lda, const float *p, int64_t ldp, float max_perturbation, float *out, int64_t ldo,
                             int64_t rows, int act_dim, cstr_stream_t stream);
int cstr_bcq_perturb_bwd_f32(const float *g_out, int64_t ldg, const float *a_vae, int64_t lda, const float *p, int64_t ldp,
                             float max_perturbation, float *g_p, int64_t rows, int act_dim, cstr_stream_t stream);
int cstr_bcq_target_f32(const float *q, int64_t q_stride, int n_critics, int64_t n_states, int samples, int grouping, const float *rew,
                        const float *done, float gamma, float *target_out, float *max_q_out, cstr_stream_t stream);
int cstr_bcq_select_f32(const float *q1, const float *cand, int64_t ldc, int64_t n_states, int samples, int act_dim, int64_t *index_out,
                        float *action_out, cstr_stream_t stream);

/* ---- PPO: the arithmetic around the Linear layers of an on-policy rollout step and minibatch step (core/ppo/ppo.py:184-300,
 * core/common/on_policy_algorithm.py:162-268, core/common/buffers.py:343-521) ------------------------------------------------------
 * All f32; obs_dim in {4, 8}, act_dim in {2, 4} (CSTR_E_UNSUPPORTED otherwise, as for more than CSTR_PPO_MAX_ROWS rows); any row
 * count >= 1. cstr_rollout_add_f32 and cstr_ppo_gather_f32 also take act_dim 1: the Categorical head's action row, the index as one
 * float (4-byte-aligned rows; see the Categorical block below). Every entry point validates on the host (NULL, non-positive sizes, misaligned rows -- 4 * width bytes for [.][width]
 * matrices, 16 for observations --, overlapping input / output rows -> CSTR_E_BADARG), then only enqueues. Batch reductions are
 * deterministic (per-workgroup f64 partials summed in workgroup order; no float atomics).
 * cstr_rollout_t: the RolloutBuffer's field arrays, [rows][n_envs][.] row-major. rollout ctl: int64[CSTR_ROLLOUT_CTL_WORDS] in HBM
 * = { pos, full, ticket, adds }, the convention of ring_ctl, except that pos stops at rows (a full buffer takes no further row).
 * workspace: uint64[CSTR_PPO_WS_WORDS] in HBM, zero before the first use (word 0 is a ticket that resets itself), private to one
 * stream.
 * cstr_diag_gaussian_act_f32: action [n][act_dim] = mean + exp(log_std) * eps (deterministic != 0: = mean), env_action (optional) =
 * clip(action, low, high) (low / high both NULL: = action), log_prob [n] (optional) = sum_a -(a - mu)^2 / (2 sigma^2) - log sigma -
 * log sqrt(2 pi). Noise unless deterministic: exactly one of eps_in [n][act_dim] (read) or rng_ctl [CSTR_RNG_CTL_WORDS] (drawn:
 * Philox4x32-10 + Box-Muller on PPO's own stream, offset advanced by n by the last workgroup); eps_out (optional) keeps the draws.
 * cstr_rollout_add_f32: writes row ctl[0] of all eight fields (advantages / returns: 0) and advances ctl; reward + gamma * terminal_value
 * where timeout != 0 (both NULL: no bootstrap), gamma as given (the caller rounds to f32). done [n_envs] (optional): episode_start is
 * overwritten with it after it was stored (the next step's episode starts). Episode statistics (all three or none, they need done):
 * ep_return [n_envs] / ep_len int32[n_envs] accumulate the env's own reward (before the bootstrap) and the step count,
 * and ep_stats double[4] = { episodes, sum of returns, sum of lengths, - } += { 1, return, length } for every env whose episode ends (the convention of cstr_collect_step_f32).
 * cstr_gae_f32: per env, t = n_steps - 1 ... 0: delta = r + (g * v_next) * nnt - v; gae = delta + ((gl * nnt) * gae); g = (float)gamma,
 * gl = (float)(gamma * gae_lambda); nnt = 1 - dones (last step) / 1 - episode_starts[t + 1]; returns = advantages + values.
 * Bit-identical to NumPy's evaluation of buffers.py:423-438.
 * cstr_ppo_gather_f32: idx int64[batch], flat index i = env i / rows, step i % rows (swap_and_flatten); indices outside
 * [0, rows * n_envs) are the caller's bug and are clamped into it.
 * cstr_ppo_loss_f32 (ppo.py:213-264): see cstr_ppo_loss_t. scalars = { policy_gradient_loss, value_loss, entropy_loss, loss, approx_kl,
 * clip_fraction }; g_mean [batch][act_dim] / g_value [batch] / g_log_std [act_dim] = d loss / d (action mean, value, log_std).
 * cstr_grad_clip_f32 (torch.nn.utils.clip_grad_norm_): grad[0..n) *= min(1, max_norm / (||grad||_2 + 1e-6)), two launches; norm_out
 * (optional) receives the norm before clipping. */
#define CSTR_ROLLOUT_CTL_WORDS 4
#define CSTR_PPO_WS_WORDS 1024
#define CSTR_PPO_MAX_BLOCKS 64
#define CSTR_PPO_MAX_ROWS 1073741824
typedef struct {
    float *obs, *act, *rew, *episode_start, *values, *log_probs, *advantages, *returns;
    int64_t rows, n_envs;
    int32_t obs_dim, act_dim;
} cstr_rollout_t;
typedef struct {
    const float *mean;         /* [batch][ldm], act_dim columns used */
    int64_t ldm;
    const float *log_std;      /* [act_dim] */
    const float *actions;      /* [batch][act_dim] */
    const float *values;       /* [batch]: the value net's output */
    const float *old_values;   /* [batch]; may be NULL when clip_range_vf <= 0 */
    const float *old_log_prob; /* [batch] */
    const float *adv;          /* [batch] */
    const float *returns;      /* [batch] */
    int64_t batch;
    int32_t act_dim;
    int32_t normalize_advantage; /* != 0: (adv - mean) / (unbiased std + 1e-8) over the batch, skipped when batch == 1 */
    double clip_range;
    double clip_range_vf;        /* <= 0: no value clipping */
    float ent_coef, vf_coef;
    float *g_mean, *g_value, *g_log_std;
    float *scalars_out;          /* [6] or NULL */
    float *scalars_sum;          /* [6] or NULL: += */
    float *log_prob_out;         /* [batch] or NULL: the new log-prob */
} cstr_ppo_loss_t;
int cstr_diag_gaussian_act_f32(const float *mean, const float *log_std, const float *eps_in, uint64_t *rng_ctl, const float *low,
                               const float *high, int deterministic, float *action, float *env_action, float *log_prob, float *eps_out,
                               int64_t n, int act_dim, cstr_stream_t stream);
int cstr_rollout_add_f32(const cstr_rollout_t *rb, int64_t *ctl, const float *obs, const float *act, const float *reward,
                         float *episode_start, const float *value, const float *log_prob, const float *timeout,
                         const float *terminal_value, float gamma, const float *done, float *ep_return, int32_t *ep_len, double *ep_stats,
                         cstr_stream_t stream);
int cstr_gae_f32(const float *rewards, const float *values, const float *episode_starts, const float *last_values, const float *dones,
                 double gamma, double gae_lambda, float *advantages, float *returns, int64_t n_steps, int64_t n_envs, cstr_stream_t stream);
int cstr_ppo_gather_f32(const cstr_rollout_t *rb, const int64_t *idx, int64_t batch, float *obs, float *act, float *old_value,
                        float *old_log_prob, float *adv, float *ret, cstr_stream_t stream);
int cstr_ppo_loss_f32(const cstr_ppo_loss_t *p, uint64_t *workspace, cstr_stream_t stream);
/* The rollout buffer of the GOAL face (PPO / A2C on a Dict observation space; reference core/common/buffers.py:696-840
 * DictRolloutBuffer): rb->obs is [rows][n_envs][6], the flat row [achieved_goal | desired_goal | observation] that
 * cstr_goal_vec_step_f32 writes. rb->obs_dim must be 6 and rb->act_dim 2, the goal face's (4, 2) layout (anything else:
 * CSTR_E_UNSUPPORTED). Observation rows (rb->obs, rows) are 8-byte aligned and move as three float2. Everything else is the statement
 * of cstr_rollout_add_f32 / cstr_ppo_gather_f32 above -- the same kernel bodies, instantiated on the row width: the timeout bootstrap,
 * episode_start overwritten with done after it was stored, the episode statistics, ctl, the swap-and-flatten index order and the
 * clamped indices, and the host-side validation (CSTR_E_BADARG) before anything is enqueued. The Box-face entry points keep refusing
 * obs_dim 6. */
int cstr_goal_rollout_add_f32(const cstr_rollout_t *rb, int64_t *ctl, const float *rows, const float *act, const float *reward,
                              float *episode_start, const float *value, const float *log_prob, const float *timeout,
                              const float *terminal_value, float gamma, const float *done, float *ep_return, int32_t *ep_len,
                              double *ep_stats, cstr_stream_t stream);
int cstr_goal_ppo_gather_f32(const cstr_rollout_t *rb, const int64_t *idx, int64_t batch, float *rows, float *act, float *old_value,
                             float *old_log_prob, float *adv, float *ret, cstr_stream_t stream);
int cstr_grad_clip_f32(float *grad, int64_t n, float max_norm, uint64_t *workspace, float *norm_out, cstr_stream_t stream);

/* ---- A2C: the loss launch and the optimiser of core/a2c/a2c.py:132-190 ---------------------------------------------------------------
 * Same conventions as the PPO block above: f32, act_dim in {2, 4} (CSTR_E_UNSUPPORTED otherwise, as for more than CSTR_PPO_MAX_ROWS
 * rows), any row count >= 1, host-side validation (NULL, non-positive sizes, misaligned rows, overlapping input / output ->
 * CSTR_E_BADARG), then only enqueues; deterministic batch reductions; the workspace is a uint64[CSTR_PPO_WS_WORDS] as above.
 * cstr_a2c_loss_f32 (a2c.py:150-171, one launch): see cstr_a2c_loss_t. policy_loss = -mean(adv * log_prob), value_loss =
 * mse(returns, values), entropy_loss = -mean(entropy), loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss; g_mean
 * [batch][act_dim] / g_value [batch] / g_log_std [act_dim] = d loss / d (action mean, value, log_std). normalize_advantage != 0:
 * (adv - mean) / (unbiased std + 1e-8) over the batch WITHOUT a batch > 1 guard (the reference has none): batch == 1 gives NaN, as
 * torch.std of one element does.
 * cstr_rmsprop_f32: torch.optim.RMSprop (momentum 0, not centred, no weight decay) over one flat arena (16-byte-aligned, param /
 * grad / square_avg disjoint) with clip_grad_norm_ folded in. Per element, every operation rounded to f32:
 *   g' = g * coef;  sq = sq * (float)alpha + ((float)(1 - alpha) * g') * g';  param = param + ((float)(-lr) * g') / (sqrtf(sq) + (float)eps)
 * lr is a DEVICE scalar (f64), as for cstr_adam_f32. max_norm > 0: two launches -- the sum-of-squares pass of cstr_grad_clip_f32
 * (same grid, same partials), then coef = min(1, max_norm / (norm + 1e-6)), the clipped gradient written back to grad and the step;
 * the result is bit-identical to cstr_grad_clip_f32 followed by the unclipped call. workspace is required, norm_out (optional)
 * receives the norm before clipping. max_norm <= 0: coef = 1, one launch, grad is not written, workspace and norm_out may be NULL.
 * cstr_rmsprop_tf_f32: RMSpropTFLike (core/common/sb2_compat/rmsprop_tf_like.py:90-135; square_avg is initialised to ONES by the
 * caller, epsilon is added inside the square root) over one flat arena, same launch shape, same folded clip, same lr / workspace /
 * norm_out conventions as cstr_rmsprop_f32. momentum_buf is given iff momentum > 0, grad_avg iff the centred form is wanted; the up
 * to five arenas are 16-byte-aligned and disjoint; alpha, eps, weight_decay, momentum >= 0. The form (weight decay != 0, centred,
 * momentum > 0) selects one of eight kernel bodies, each touching only the arenas it has. Per element, every operation rounded to
 * f32, the scalars converted once ((float)alpha, (float)(1 - alpha), (float)eps, (float)weight_decay, (float)momentum, (float)(-lr)):
 *   g' = g * coef                                  (written back to grad when max_norm > 0, before weight decay)
 *   weight decay:  g' = g' + wd * param
 *                  sq = sq * alpha + ((1 - alpha) * g') * g'
 *   centred:       ga = ga * alpha + (1 - alpha) * g';  avg = sqrtf((sq - ga * ga) + eps)     (NaN where that sum is negative)
 *   otherwise:     avg = sqrtf(sq + eps)
 *   momentum:      buf = buf * momentum + g' / avg;     param = param + (-lr) * buf
 *   otherwise:     param = param + ((-lr) * g') / avg */
typedef struct {
    const float *mean;         /* [batch][ldm], act_dim columns used */
    int64_t ldm;
    const float *log_std;      /* [act_dim] */
    const float *actions;      /* [batch][act_dim] */
    const float *values;       /* [batch]: the value net's output */
    const float *adv;          /* [batch] */
    const float *returns;      /* [batch] */
    int64_t batch;
    int32_t act_dim;
    int32_t normalize_advantage;
    float ent_coef, vf_coef;
    float *g_mean, *g_value, *g_log_std;
    float *scalars_out;        /* [4] = { policy_loss, value_loss, entropy_loss, loss } or NULL */
    float *log_prob_out;       /* [batch] or NULL: the log-prob of the actions */
} cstr_a2c_loss_t;
int cstr_a2c_loss_f32(const cstr_a2c_loss_t *p, uint64_t *workspace, cstr_stream_t stream);
int cstr_rmsprop_f32(float *param, float *grad, float *square_avg, const double *lr, double alpha, double eps, float max_norm,
                     uint64_t *workspace, float *norm_out, int64_t n, cstr_stream_t stream);
int cstr_rmsprop_tf_f32(float *param, float *grad, float *square_avg, float *momentum_buf /* NULL iff momentum == 0 */,
                        float *grad_avg /* NULL iff !centered */, const double *lr, double alpha, double eps, double weight_decay,
                        double momentum, float max_norm, uint64_t *workspace, float *norm_out, int64_t n, cstr_stream_t stream);

/* ---- DQN on the discrete valve face: exploration draw, action selection, target + gather + Huber loss (core/dqn/dqn.py:168-256) -----
 * Same conventions as the PPO block: f32 data, host-side validation (NULL, non-positive sizes, misaligned or overlapping rows ->
 * CSTR_E_BADARG), then only enqueues; a deterministic batch reduction; the workspace is a uint64[CSTR_PPO_WS_WORDS] as above.
 * The face: n_actions = levels * levels indices over two valves with `levels` settings each, 2 <= levels <= CSTR_DQN_MAX_LEVELS
 * (anything else, or more than CSTR_PPO_MAX_ROWS rows: CSTR_E_UNSUPPORTED). Index a = i * levels + j stands for the normalised valve
 * pair (v(i), v(j)), v(q) = (float)-1 + (float)(2 q) / (float)(levels - 1); a stored valve value gives its level back as
 * rint((v + 1) * (levels - 1) / 2), clamped into the face.
 * cstr_mt19937_rand_flag_f64: one RandomState.random_sample() from the legacy stream image mt_state [CSTR_MT_STATE_WORDS] (two words,
 * ((a >> 5) * 2^26 + (b >> 6)) / 2^53; the stream advances, twist included): flag_out[0] = draw < threshold[0] in f64, threshold a
 * DEVICE double; draw_out (optional) keeps the draw. `np.random.rand() < self.exploration_rate` of dqn.py:245.
 * cstr_dqn_act_f32: q [n][ldq], n_actions columns used. Greedy index = first maximum of the row (torch.argmax; a NaN counts as the
 * greatest value). mode 0: greedy. mode 1 (the reference): every row takes a uniform random index iff flag[0] != 0 (device int32),
 * else greedy. mode 2: row r explores iff u[r][0] < eps[0] (device double, compared in f64). The random index is
 * min(floor(u[r][1] * n_actions), n_actions - 1). Uniforms in modes 1 and 2: exactly one of u_in [n][2] (read) or rng_ctl
 * [CSTR_RNG_CTL_WORDS] (drawn: Philox4x32-10 on DQN's own stream, (word >> 8) * 2^-24; the last workgroup advances the offset by n in
 * every such launch). valve_out [n][2] = (v(a / levels), v(a % levels)); index_out int64[n] (optional) = a.
 * cstr_dqn_loss_f32 (dqn.py:195-212, one launch): target = reward + ((1 - done) * gamma) * max_a next_q[b][a] (a NaN propagates),
 * cur = q[b][index(valve[b])], loss_out[0] = mean(smooth_l1(cur - target)) with beta 1, loss_sum[0] (optional) += it; g_q [batch][ldq]
 * = d loss / d q: zero except g_q[b][index] = clamp(cur - target, -1, 1) / batch. cur_q_out / target_out [batch] (optional). */
#define CSTR_DQN_MAX_LEVELS 16
int cstr_mt19937_rand_flag_f64(uint32_t *mt_state, const double *threshold, int32_t *flag_out, double *draw_out, cstr_stream_t stream);
int cstr_dqn_act_f32(const float *q, int64_t ldq, int64_t n, int n_actions, int levels, int mode, const double *eps, const int32_t *flag,
                     const float *u_in, uint64_t *rng_ctl, float *valve_out, int64_t *index_out, cstr_stream_t stream);
int cstr_dqn_loss_f32(const float *q, int64_t ldq, const float *next_q, int64_t ldn, const float *valve, const float *reward,
                      const float *done, float gamma, int64_t batch, int n_actions, int levels, float *g_q, float *loss_out,
                      float *loss_sum, float *cur_q_out, float *target_out, uint64_t *workspace, cstr_stream_t stream);

/* ---- QR-DQN on the discrete valve face (csrc/cstr_qrdqn.hip; core/qrdqn/qrdqn.py; Dabney et al. 2018, quantile-regression DQN) -------
 * What QR-DQN adds to DQN's launches: the folded head its action selection runs on, and everything between the two forward passes of
 * a gradient step and loss.backward(). Both entry points validate on the host without dereferencing anything and then only enqueue;
 * f32 in and out, float64 inside; deterministic and bit-identical on relaunch (no float atomics, no workgroup waiting for another).
 * The face is the DQN block's: M = n_actions = levels * levels, 2 <= levels <= CSTR_DQN_MAX_LEVELS. Nq = n_quantiles, B = batch,
 * tau_i = (i + 0.5) / Nq. ATOM LAYOUT: a row holds Nq * M floats, atom i of action a at i * M + a (`quantiles.view(-1, Nq, M)`, what
 * the network's last Linear layer leaves).
 * cstr_qrdqn_supported: the DQN face check and 1 <= Nq <= CSTR_QRDQN_MAX_QUANTILES.
 * cstr_qrdqn_fold_head_f32 (one launch): the mean over the atoms is linear, so greedy action selection needs only the FOLDED last
 *   layer: w_mean[a][k] = (sum_i w[i * M + a][k]) / Nq, b_mean[a] = (sum_i bias[i * M + a]) / Nq; w [Nq * M][H] and w_mean [M][H]
 *   contiguous. Each sum runs over i ascending in float64, is divided by Nq and rounded to float32 once. One lane per output element,
 *   consecutive lanes on consecutive k: each of a wave's Nq loads is one contiguous 256-byte run; eight loads are in flight per lane.
 *   The folded layer feeds cstr_linear_act_fwd_f32 and cstr_dqn_act_f32 unchanged: there is no act kernel over full atom rows.
 *   No cap on Nq. CSTR_E_BADARG: a NULL pointer, n_actions, Nq or H <= 0, a pointer off a 4-byte boundary, an output overlapping an
 *   input or the other output. CSTR_E_UNSUPPORTED: more than 2^30 output elements.
 * cstr_qrdqn_loss_f32 (two launches: one workgroup per row, then one workgroup over the per-row sums in ws). z [B][ldz] the online
 *   network's atoms at s, z_next [B][ldn] the target network's at s', ldz, ldn >= Nq * M; valve [B][2] the stored valve pair. Per row b:
 *     S_a = sum_i z_next[b][i][a] (i ascending, float64);  a* = the first maximum of S (a NaN counts as the greatest value, the first
 *     one wins: cstr_dqn_act_f32's convention);  y_j = reward_b + (1 - done_b) * gamma * z_next[b][j][a*]           j = 0 .. Nq - 1
 *     a = level(valve[b][0]) * levels + level(valve[b][1]) (the DQN block's inverse);  z_i = z[b][i][a];  delta = y_j - z_i,
 *     H = 0.5 delta^2 if |delta| <= 1 else |delta| - 0.5,  rho = |tau_i - 1[delta < 0]| * H
 *     gz[b][i][a] = -(1 / (B Nq)) * sum_j |tau_i - 1[delta < 0]| * clamp(delta, -1, 1)   (j ascending); every other entry of the
 *     row's Nq * M is stored as 0. gz has z's shape and row stride.
 *   loss = (sum over (b, i, j) of rho) / (B Nq): the sum over the current quantile, the mean over batch and target quantile
 *   (`quantile_huber_loss(current, target, sum_over_quantiles=True)`). loss_out [1] (stored) / loss_sum [1] (+= loss, one float32
 *   addition). cur_out [B][Nq] = z_i, target_out [B][Nq] = y_j, next_index_out int64 [B] = a*. Every difference, Huber term and sum is
 *   float64 on the float32 inputs; each output is rounded to float32 once. ws: double [B] scratch (the per-row sums), 8-byte aligned.
 *   Reduction order: a row's lanes through a 64-lane shuffle tree (offsets 32 .. 1), wave sums in wave order; rows t, t + 256, ...
 *   in ascending order on lane t of the finishing workgroup, the same tree (the TQC block's).
 *   Optional (NULL = not written): loss_out, loss_sum, cur_out, target_out, next_index_out.
 *   CSTR_E_BADARG: a NULL required pointer, batch, n_actions, levels or Nq <= 0, ldz or ldn < Nq * M, gamma negative or NaN, a pointer
 *   off a 4-byte (valve, next_index_out, ws: 8-byte) boundary, an output overlapping an input or another output.
 *   CSTR_E_UNSUPPORTED: not cstr_qrdqn_supported, batch > CSTR_MAX_SAMPLE_BATCH. */
#define CSTR_QRDQN_MAX_QUANTILES 256
int cstr_qrdqn_supported(int n_actions, int levels, int n_quantiles);
int cstr_qrdqn_fold_head_f32(const float *w, const float *bias, int n_actions, int n_quantiles, int64_t H, float *w_mean, float *b_mean,
                             cstr_stream_t stream);
int cstr_qrdqn_loss_f32(const float *z, int64_t ldz, const float *z_next, int64_t ldn, const float *valve, const float *reward,
                        const float *done, double gamma, int64_t batch, int n_actions, int levels, int n_quantiles, float *gz,
                        float *loss_out, float *loss_sum, float *cur_out, float *target_out, int64_t *next_index_out, double *ws,
                        cstr_stream_t stream);

/* ---- Categorical head of PPO / A2C on the discrete valve face (core/common/distributions.py:263-311, core/ppo/ppo.py:213-264,
 * core/a2c/a2c.py:150-171) ---------------------------------------------------------------------------------------------------------
 * Same conventions as the PPO block: f32 data, host-side validation (NULL, non-positive sizes, misaligned or overlapping rows ->
 * CSTR_E_BADARG), then only enqueues; deterministic batch reductions; the workspace is a uint64[CSTR_PPO_WS_WORDS] as above. The face
 * is the DQN block's: n_actions = levels * levels, 2 <= levels <= CSTR_DQN_MAX_LEVELS (anything else, or more than CSTR_PPO_MAX_ROWS
 * rows: CSTR_E_UNSUPPORTED). logits [rows][ldz], ldz >= n_actions, n_actions columns used, rows 4-byte aligned.
 * Per row: logp_j = (z_j - max z) - log sum_j exp(z_j - max z) (torch's Categorical(logits = z)), p_j = exp(logp_j).
 * cstr_categorical_act_f32 (one launch): the index a comes from exactly one source (two at once, or none: CSTR_E_BADARG):
 *   deterministic != 0: the first maximum of the row's logits (a NaN counts as the greatest value). The reference takes argmax(probs);
 *     the two differ only where two distinct logits round to the same probability;
 *   action_in int64[n]: teacher-forced indices; values outside the face are the caller's bug and are clamped into it;
 *   u_in [n]: a given uniform in [0, 1);
 *   rng_ctl [CSTR_RNG_CTL_WORDS]: the uniform is drawn, Philox4x32-10 on the head's own stream, counter (offset + row, 0, tag), word 0
 *     as (word >> 8) * 2^-24; the last workgroup advances the offset by n.
 * With a uniform u, a is the first index whose inclusive cumulative probability (f32, index order) exceeds u, n_actions - 1 if none
 * does. Outputs: index_f32 [n] = a as a float (what the rollout buffer stores); optional index_out int64[n], valve_out [n][2] =
 * (v(a / levels), v(a % levels)), log_prob [n] = logp_a, u_out [n] = the uniforms (only with u_in or rng_ctl).
 * cstr_categorical_loss_f32 (one launch): see cstr_categorical_loss_t. Per row the stored action is a = (long)actions[b] (clamped
 * into the face), H_b = -sum_j p_j logp_j. objective 0 (PPO): cstr_ppo_loss_f32's statements with logp_a as the log-prob, the same six
 * scalars in the same order, entropy_loss = -mean_b H_b; objective 1 (A2C): cstr_a2c_loss_f32's four scalars, the advantage
 * normalisation without a batch > 1 guard (batch 1: NaN). Any other objective: CSTR_E_BADARG.
 * g_logits[b][j] = g_logp_b * ((j == a) - p_j) + (ent_coef / batch) * p_j * (logp_j + H_b), g_logp_b = d loss / d logp_a (PPO:
 * -(dmin * ratio) / batch with the closed-interval clamp rule; A2C: -adv_b / batch); columns n_actions .. ldz of g_logits are not
 * written. g_value [batch] as in the two blocks above. */
typedef struct {
    const float *logits;       /* [batch][ldz], n_actions columns used */
    int64_t ldz;
    const float *actions;      /* [batch]: the stored index as a float */
    const float *values;       /* [batch]: the value net's output */
    const float *old_values;   /* [batch]; may be NULL when clip_range_vf <= 0 or objective 1 */
    const float *old_log_prob; /* [batch]; may be NULL for objective 1 */
    const float *adv;          /* [batch] */
    const float *returns;      /* [batch] */
    int64_t batch;
    int32_t n_actions, levels;
    int32_t objective;           /* 0: PPO, 1: A2C */
    int32_t normalize_advantage; /* != 0: (adv - mean) / (unbiased std + 1e-8); PPO skips it when batch == 1 */
    double clip_range;           /* PPO */
    double clip_range_vf;        /* PPO; <= 0: no value clipping */
    float ent_coef, vf_coef;
    float *g_logits;             /* [batch][ldz] */
    float *g_value;              /* [batch] */
    float *scalars_out;          /* [6] (PPO) / [4] (A2C) or NULL */
    float *scalars_sum;          /* same size or NULL: += */
    float *log_prob_out;         /* [batch] or NULL: logp_a */
} cstr_categorical_loss_t;
int cstr_categorical_act_f32(const float *logits, int64_t ldz, int64_t n, int n_actions, int levels, int deterministic,
                             const int64_t *action_in, const float *u_in, uint64_t *rng_ctl, float *index_f32, int64_t *index_out,
                             float *valve_out, float *log_prob, float *u_out, cstr_stream_t stream);
int cstr_categorical_loss_f32(const cstr_categorical_loss_t *p, uint64_t *workspace, cstr_stream_t stream);

/* ---- MultiCategorical head of PPO / A2C on the MultiDiscrete valve face (core/common/distributions.py:314-368, core/ppo/ppo.py:213-264,
 * core/a2c/a2c.py:150-171) ---------------------------------------------------------------------------------------------------------
 * Same conventions as the Categorical block: f32 data, host-side validation (NULL, non-positive sizes, ldz < levels0 + levels1,
 * misaligned or overlapping rows -> CSTR_E_BADARG), then only enqueues; deterministic batch reductions; the workspace is a
 * uint64[CSTR_PPO_WS_WORDS] as above. The face: one categorical per valve, 2 <= levels_g <= CSTR_MCAT_MAX_LEVELS (anything else, or
 * more than CSTR_PPO_MAX_ROWS rows: CSTR_E_UNSUPPORTED). logits [rows][ldz], ldz >= levels0 + levels1, rows 4-byte aligned: columns
 * 0 .. levels0 - 1 are valve 0's, levels0 .. levels0 + levels1 - 1 valve 1's (th.split order). Level q of valve g stands for the
 * normalised valve action v_g(q) = f32(-1) + f32(2 q) / f32(levels_g - 1). Rows of pairs ([.][2]) are 8-byte aligned.
 * Per valve g: logp_j = (z_j - m_g) - log sum_j exp(z_j - m_g), p_j = exp(logp_j), H_g = -sum_j p_j max(logp_j, -FLT_MAX).
 * Per row: logp = logp_0[a_0] + logp_1[a_1], H = H_0 + H_1 (f32).
 * cstr_multicategorical_act_f32 (one launch): the pair (a_0, a_1) comes from exactly one source (two at once, or none: CSTR_E_BADARG):
 *   deterministic != 0: the first maximum of each valve's logits (a NaN counts as the greatest value, the first one wins);
 *   action_in int64[n][2]: teacher-forced pairs; levels outside the face are the caller's bug and are clamped per valve;
 *   u_in [n][2]: given uniforms in [0, 1);
 *   rng_ctl [CSTR_RNG_CTL_WORDS]: the uniforms are drawn, Philox4x32-10 on the head's own stream, counter (offset + row, 0, tag), words
 *     0 and 1 of the one block as (word >> 8) * 2^-24 for valves 0 and 1; the last workgroup advances the offset by n.
 * With uniforms, a_g is the first level of valve g whose inclusive cumulative probability (f32, index order) exceeds u_g, levels_g - 1
 * if none does. Outputs: action_f32 [n][2] = the pair as floats (what the rollout buffer stores); optional action_out int64[n][2],
 * valve_out [n][2] = (v_0(a_0), v_1(a_1)), log_prob [n], u_out [n][2] = the uniforms (only with u_in or rng_ctl).
 * cstr_multicategorical_loss_f32 (one launch): cstr_categorical_loss_f32's objectives, scalars and order on the row's logp and H; the
 * stored pair is (long)actions[b][g], clamped per valve. For a column j of valve g:
 *   g_logits[b][j] = g_logp_b * ((j == a_g) - p_j) + (ent_coef / batch) * p_j * (logp_j + H_g)      (the valve's own H_g);
 * columns levels0 + levels1 .. ldz of g_logits are not written. g_value, scalars_out, scalars_sum, log_prob_out, the value clip, the
 * advantage normalisation and the NaN behaviour are the Categorical loss's. */
#define CSTR_MCAT_MAX_LEVELS 32
typedef struct {
    const float *logits;       /* [batch][ldz], levels0 + levels1 columns used */
    int64_t ldz;
    const float *actions;      /* [batch][2]: the stored level pair as floats */
    const float *values;       /* [batch]: the value net's output */
    const float *old_values;   /* [batch]; may be NULL when clip_range_vf <= 0 or objective 1 */
    const float *old_log_prob; /* [batch]; may be NULL for objective 1 */
    const float *adv;          /* [batch] */
    const float *returns;      /* [batch] */
    int64_t batch;
    int32_t levels0, levels1;
    int32_t objective;           /* 0: PPO, 1: A2C */
    int32_t normalize_advantage; /* != 0: (adv - mean) / (unbiased std + 1e-8); PPO skips it when batch == 1 */
    double clip_range;           /* PPO */
    double clip_range_vf;        /* PPO; <= 0: no value clipping */
    float ent_coef, vf_coef;
    float *g_logits;             /* [batch][ldz] */
    float *g_value;              /* [batch] */
    float *scalars_out;          /* [6] (PPO) / [4] (A2C) or NULL */
    float *scalars_sum;          /* same size or NULL: += */
    float *log_prob_out;         /* [batch] or NULL: the pair's log-prob */
} cstr_multicategorical_loss_t;
int cstr_multicategorical_act_f32(const float *logits, int64_t ldz, int64_t n, int levels0, int levels1, int deterministic,
                                  const int64_t *action_in, const float *u_in, uint64_t *rng_ctl, float *action_f32, int64_t *action_out,
                                  float *valve_out, float *log_prob, float *u_out, cstr_stream_t stream);
int cstr_multicategorical_loss_f32(const cstr_multicategorical_loss_t *p, uint64_t *workspace, cstr_stream_t stream);

/* ---- Hindsight Experience Replay on the goal-conditioned face of the env (core/her/her_replay_buffer.py) ---------------------------
 * The goal face (constructed here; the reference's env has none): achieved_goal = observation[2] (normalised C2), desired_goal = the
 * env's own target through the same affine map, g = 2 (target - s_lo[2]) / s_span[2] - 1. A flat row is six floats in key order,
 * [achieved_goal | desired_goal | observation], rows 8-byte aligned. The reward is the reference's concentration term
 * (twoseriescstr.py:288-291) on (achieved, desired), in f32 and in this order:
 *   C2 = s_lo2 + (ag + 1) * s_span2 / 2;  T = s_lo2 + (dg + 1) * s_span2 / 2;  ne = |C2 - T| / conc_span;  r = -5 (ne ne) - 2 ne.
 * All four entry points validate on the host (NULL, non-positive sizes, a ring that is not (4, 2), misaligned or overlapping rows ->
 * CSTR_E_BADARG / CSTR_E_UNSUPPORTED) and then only enqueue. */
#define CSTR_HER_FUTURE 0  /* GoalSelectionStrategy (core/her/goal_selection_strategy.py:12-17) */
#define CSTR_HER_FINAL 1
#define CSTR_HER_EPISODE 2
#define CSTR_HER_MAX_BATCH 1024
#define CSTR_HER_MAX_ROWS 8192         /* ring rows: the sampler keeps a prefix sum over them in LDS */
#define CSTR_HER_MAX_ENVS (1 << 24)    /* and rows * n_envs < 2^31: the count of valid transitions is an int32 */

/* Side arrays of the HER ring, beside a cstr_ring_t with (obs_dim, act_dim) = (4, 2). W = ceil(n_envs / 64). */
typedef struct cstr_her {
    float *desired_goal;   /* [rows][n_envs]: observations["desired_goal"]; next_observations' is the same within an episode */
    int32_t *ep_start;     /* [rows][n_envs] (:97) */
    int32_t *ep_length;    /* [rows][n_envs] (:98); > 0 = the transition can be sampled */
    int32_t *cur_ep_start; /* [n_envs] (:99) */
    int32_t *row_valid;    /* [rows]: number of envs with ep_length > 0 in the row; kept current by cstr_her_add_f32 */
    uint64_t *valid_bits;  /* [rows][W]: bit e of word w set = env 64 w + e of the row has ep_length > 0; likewise */
} cstr_her_t;

/* VecEnv.step on the goal face, one launch: TwoSeriesCSTREnv.step (the dynamics of cstr_vec_step_f32, bit for bit) with the reward
 * above on the lane's own target (NaN action or state: old state, -10, truncated, as there), truncation, auto-reset from the env's
 * own PCG64 stream exactly as cstr_reset_draw_f32 draws it, and the target of the next episode.
 *   env_obs [N][4] i/o: the env state, replaced by the reset observation where done;  act [N][2];  step_count [N] i/o
 *   pcg_state [N][4] i/o, static_init double[N][4] or NULL: the reset source
 *   target [N] i/o: raw setpoint (mol/L) per env
 *   episode int32[N] i/o or NULL: NULL = targets stay; else an env that finishes redraws target = goal_lo + (goal_hi - goal_lo) * u,
 *     u = (x >> 8) * 2^-24 with x = word 0 of Philox4x32-10, key = goal_seed, counter = (goal_index_offset + env index [64 bit],
 *     episode[env], tag 0x90A17A67), and episode[env] += 1: counter-based, no other state
 *   next_rows [N][6] out: the true next observation (terminal observation where done) with the OLD target
 *   rows_after [N][6] out: what VecEnv.step returns (reset observation and new target where done)
 *   reward / done / timeout [N] out. obs_dim must be 4. */
int cstr_goal_vec_step_f32(const cstr_coef_t *coef, int integrator, int obs_dim, float *env_obs, const float *act, int32_t *step_count,
                           uint64_t *pcg_state, double *static_init, float *target, int32_t *episode, uint64_t goal_seed,
                           int64_t goal_index_offset, float goal_lo, float goal_hi, float *next_rows, float *rows_after, float *reward,
                           float *done, float *timeout, int64_t n_envs, cstr_stream_t stream);

/* HerReplayBuffer.add + _compute_episode_length (her_replay_buffer.py:135-184) at the device-resident ring position, a lane per env:
 * an old episode that the row overwrites is invalidated as a whole (np.arange(pos, ep_start + ep_length) % rows, the reference's
 * modulo), ep_start[pos] = cur_ep_start, the ring row and the goal are written (obs_rows / next_rows [N][6] flat rows; columns 2..5
 * go to the ring, column 1 of obs_rows to desired_goal), and where done != 0 the episode's rows get ep_length = end - start with
 * end = the advanced position (+ rows when it wrapped) and cur_ep_start = the advanced position. row_valid / valid_bits follow every
 * change. The last workgroup advances ring_ctl like cstr_replay_add_f32. */
int cstr_her_add_f32(const cstr_ring_t *ring, const cstr_her_t *her, int64_t *ring_ctl, const float *obs_rows, const float *next_rows,
                     const float *act, const float *rew, const float *done, const float *timeout, cstr_stream_t stream);

/* The rollout's vec-step on the goal face in ONE launch, a lane per env: what cstr_collect_step_rng_f32 is on the Box face. Per env, in
 * this order:
 *   1. the action scaling chain of cstr_collect_step_f32 on policy_out [N][2] (squashed bit 0 set: tanh output, unscaled first; clear: a
 *      warm-up action already in [act_low, act_high], both HOST pointers to 2 floats); noise [N][2] or NULL is added to the scaled action
 *      and clipped to [-1, 1] (fminf / fmaxf as there: a NaN action with noise is clipped, without noise it reaches the env); the buffer
 *      action is the scaled action, the env's action its unscale;
 *   2. the body of cstr_goal_vec_step_f32 (the same device function): env step, goal reward on the lane's own target, the NaN path,
 *      truncation, auto-reset from the env's PCG64 stream, the Philox target redraw with episode[i] += 1, step_count;
 *   3. the body of cstr_her_add_f32 (the same device function) at ring_ctl[0]: the invalidation loop, the ring row (observation = the
 *      env's own flat row as it stood before the step, next observation = the terminal observation where done, the buffer action),
 *      ep_start / ep_length / cur_ep_start, row_valid / valid_bits;
 *   4. Monitor's statistics as in cstr_collect_step_f32: ep_return [N] accumulates the reward; where an episode ends, ep_stats double[4]
 *      += {1, return, step count the episode reached} by f64 atomicAdd (count and length sum exact in any order; the return sum may
 *      differ in its last f64 bits between runs); both NULL or both given;
 *   5. the last workgroup advances ring_ctl and, if policy_rng_ctl != NULL, adds policy_rng_advance to its offset word.
 * State: env_obs [N][4] i/o; rows [N][6] i/o, the env's flat rows: each lane reads its own row as the transition's observation before
 * it writes what VecEnv.step returns over it; step_count, pcg_state, static_init (or NULL), target, episode (or NULL: targets stay),
 * goal_seed, goal_index_offset, goal_lo, goal_hi as in cstr_goal_vec_step_f32. N = ring->n_envs.
 * Outputs, each may be NULL: reward_out / done_out / timeout_out [N], next_rows_out [N][6] (the next_rows of cstr_goal_vec_step_f32).
 * Every array above and every ring / side array is bit-identical to: the chain's f32 statements, cstr_goal_vec_step_f32, cstr_her_add_f32.
 * CSTR_E_BADARG: NULL required pointers, n_envs <= 0, act_high <= act_low, goal_lo > goal_hi with episode, misaligned rows, anything the
 * launch writes overlapping anything else it touches, ep_return / ep_stats not given together. CSTR_E_UNSUPPORTED: a ring that is not
 * (4, 2), obs_dim != 4, squashed with any bit but bit 0 (bit 1 = multi-agent), an unknown integrator, sizes beyond CSTR_HER_MAX_*.
 * All checked before anything is enqueued. */
int cstr_goal_collect_step_f32(const cstr_coef_t *coef, int integrator, int obs_dim, const cstr_ring_t *ring, const cstr_her_t *her,
                               int64_t *ring_ctl, float *env_obs, float *rows, int32_t *step_count, uint64_t *pcg_state, double *static_init,
                               float *target, int32_t *episode, uint64_t goal_seed, int64_t goal_index_offset, float goal_lo, float goal_hi,
                               const float *policy_out, int squashed, const float *act_low, const float *act_high, const float *noise,
                               float *reward_out, float *done_out, float *timeout_out, float *next_rows_out, float *ep_return,
                               double *ep_stats, uint64_t *policy_rng_ctl, uint64_t policy_rng_advance, cstr_stream_t stream);

/* HerReplayBuffer.sample (her_replay_buffer.py:186-384) in one launch on the legacy MT19937 stream:
 *   k = randint(0, n_valid, batch) (what np.random.choice(valid_indices, batch) draws) -> the k-th valid (row, env), row-major;
 *   the first nb_virtual samples are virtual: goal index final = len - 1 (no draw) | future = randint(cur, len) per element,
 *   cur = (row - ep_start) % rows | episode = randint(0, len) per element (array-form randint: one masked-rejection draw per element
 *   in order, none where high - low == 1); new goal = next_observations[(index + ep_start) % rows, env][2]; virtual reward = the
 *   statement above on (next achieved, new goal); real rewards and goals are the stored ones; done = dones * (1 - timeouts).
 * Outputs hold the real transitions first, then the virtual ones: out_obs / out_next_obs [B][6] flat rows, out_act [B][2], out_done /
 * out_rew [B]; out_row_idx / out_env_idx / out_goal_row int64[B] or NULL, in output order (goal row -1 for real transitions).
 * forced_row / forced_env int64[B] (both or neither; draw order, the first nb_virtual are virtual): the index draw is skipped;
 * forced_goal int64[B] (needs the pair): ring rows of the goals, the goal draw is skipped too. Forced indices are clamped into the ring.
 * status int32[1] out: 0 = sampled; 1 = no valid transition, nothing else was written and the stream is where it was.
 * nb_virtual > batch or an unknown strategy: CSTR_E_BADARG; batch > CSTR_HER_MAX_BATCH, rows > CSTR_HER_MAX_ROWS: CSTR_E_UNSUPPORTED. */
int cstr_her_sample_f32(const cstr_coef_t *coef, const cstr_ring_t *ring, const cstr_her_t *her, uint32_t *mt_state, int64_t batch,
                        int64_t nb_virtual, int strategy, const int64_t *forced_row, const int64_t *forced_env, const int64_t *forced_goal,
                        float *out_obs, float *out_act, float *out_next_obs, float *out_done, float *out_rew, int64_t *out_row_idx,
                        int64_t *out_env_idx, int64_t *out_goal_row, int32_t *status, cstr_stream_t stream);

/* Whole evaluation episodes on the GOAL face in ONE launch: cstr_eval_episodes_f32's structure (a workgroup owns 16 envs and walks
 * their vec-steps inside the launch, a lane of wave 0 per env carries the episode state, workgroups exchange nothing) with, per vec-step:
 *   network input: the flat row [achieved_goal | desired_goal | observation] (6 floats, net->k0 = 6) that cstr_goal_vec_step_f32 writes:
 *     achieved_goal = observation[2], desired_goal = 2 (target - s_lo[2]) / s_span[2] - 1, constant within an episode; network stages,
 *     both head forms and predict()'s post-processing as in cstr_eval_episodes_f32;
 *   env step: the dynamics of cstr_vec_step_f32 on the (4, 2) layout, reward = the goal reward on (achieved goal of the next state, the
 *     OLD desired goal); NaN action or state: old state, -10, truncated, as in cstr_goal_vec_step_f32;
 *   episode end, in this order: the accounting slot, the PCG64 reset draw, and -- if episode != NULL -- the target redraw of
 *     cstr_goal_vec_step_f32 (Philox4x32-10 word 0, key goal_seed, counter (goal_index_offset + env index [64 bit], episode[env], tag
 *     0x90A17A67), u = (x >> 8) * 2^-24, target = goal_lo + (goal_hi - goal_lo) * u) followed by episode[env] += 1.
 * Arguments as in cstr_eval_episodes_f32 (obs_dim = 4 implied: env_obs [N][4]) plus
 *   target float[N] i/o: raw setpoint per env;  episode int32[N] i/o or NULL (NULL: targets stay)
 *   three OPTIONAL per-episode outputs laid out like ep_return ([N][ep_stride], slots at and beyond targets[i] not written):
 *     ep_goal float: the episode's desired_goal (normalised)
 *     ep_gap float: achieved_goal - desired_goal of the episode's TERMINAL row (columns 0 and 1 of the next_rows row that
 *                   cstr_goal_vec_step_f32 would have written on the last step), one f32 subtraction
 *     ep_abs_gap double: the f64 sum, in step order, of (double)fabsf(achieved - desired) over the next_rows of all the episode's steps
 * For the counted episodes every output, pcg_state, env_obs, step_count, target and episode are bit-identical to the step-by-step
 * launches: cstr_policy_rows_fwd_f32 on the flat rows (head 0: eps = 0), the post-processing, cstr_goal_vec_step_f32. An env stops once
 * it has met its target: its state after its last counted episode (the reset draw and the target redraw behind that episode included)
 * is what the launch leaves.
 * CSTR_E_BADARG: NULL required pointers, n_envs <= 0, a negative target, max_vec_steps <= 0, net->k0 != 6, goal_lo > goal_hi when
 * episode is given, misaligned rows, outputs overlapping inputs or each other; CSTR_E_UNSUPPORTED: net->act_dim != 2, unknown
 * integrator, a network shape cstr_policy_rows_fwd_f32 does not take or more than 64 KB of LDS. All checked before anything is enqueued. */
int cstr_eval_goal_episodes_f32(const cstr_policy_mlp_t *net, const cstr_coef_t *coef, int integrator, float *env_obs, int32_t *step_count,
                                uint64_t *pcg_state, double *static_init, float *target, int32_t *episode, uint64_t goal_seed,
                                int64_t goal_index_offset, float goal_lo, float goal_hi, int squashed, const float *act_low,
                                const float *act_high, const int32_t *targets, int64_t n_envs, int64_t max_vec_steps, double *ep_return,
                                int32_t *ep_len, int32_t *ep_done, float *ep_goal, float *ep_gap, double *ep_abs_gap, cstr_stream_t stream);

/* ---- Augmented Random Search (csrc/cstr_ars.hip; Mania, Guy & Recht 2018, sb3_contrib.ARS) ----------------------------------------
 * One update = 2 n_delta whole-episode evaluations of perturbed copies of a small deterministic policy (one launch), then selection
 * and the parameter step (a second launch). No backward pass, no optimiser state.
 *
 * The policy: nn.Sequential(create_mlp(obs_dim, act_dim, net_arch, activation, with_bias, squash_output)), its parameters one flat
 * float vector `theta` in parameters() order without padding: per layer W [out][in] row-major, then b [out] when with_bias.
 *   n_hidden 0 (u = K x (+ b)), 1 or 2; h1, h2 in 1 .. CSTR_ARS_MAX_WIDTH (ignored where the layer does not exist);
 *   act 1 = ReLU, 2 = Tanh (CSTR_ACT_*; ignored with n_hidden = 0); squash: a Tanh behind the last layer, and predict() un-scales
 *   low + 0.5 (y + 1) (high - low); without it predict() clips into [low, high] (NaN passes).
 * A dot product is acc = 0, acc += w[i] * x[i] for i ascending, then + bias, then the activation: one summation order.
 *
 * THE DELTAS ARE NEVER STORED: delta[k][p] (k < n_delta, p < P) is, with q = p >> 2 and e = p & 3,
 *   words = Philox4x32-10(counter words (q, k, (uint32_t)update_index, 0xA4500D17), key words ((uint32_t)seed, (uint32_t)(seed >> 32)))
 *   z0 = r(words[0]) cos(a(words[1])), z1 = r(words[0]) sin(a(words[1])), z2, z3 likewise from words[2], words[3];  delta[k][p] = z_e
 *   r(w) = sqrtf(-2 logf(((w >> 8) + 0.5) * 2^-24)),  a(w) = 2 pi ((w >> 8) + 0.5) * 2^-24     (float arithmetic)
 * Counter word 3 is this stream's own tag. Both launches regenerate the deltas from (seed, update_index).
 * Candidates (float: product rounded, then the sum): job c = k is theta + delta_std * delta_k, job c = n_delta + k is theta - ... . */
#define CSTR_ARS_MAX_WIDTH 64   /* hidden units per layer: one lane each */
#define CSTR_ARS_MAX_DELTA 4096 /* n_delta: the update launch ranks by counting inside one workgroup */

typedef struct {
    int32_t obs_dim, act_dim, n_hidden, h1, h2, act, with_bias, squash;
} cstr_ars_policy_t;

/* Host only, touches no GPU: 1 when the two launches take this policy, n_delta in 1 .. CSTR_ARS_MAX_DELTA and n_top in 1 .. n_delta;
 * else 0. (obs_dim, act_dim) must be a CSTR layout. */
int cstr_ars_supported(int obs_dim, int act_dim, int n_hidden_layers, int h1, int h2, int act, int with_bias, int squash, int n_delta,
                       int n_top);

/* The population launch. Job c (0 .. 2 n_delta - 1) runs on env slot c % n_envs; a slot handles its jobs in increasing c, one after
 * another. A job: the slot's reset draw (its PCG64 stream and static_init entry, the arithmetic of cstr_reset_draw_f32; step_count = 0),
 * then n_eval_episodes episodes: per step the policy, predict()'s un-scale / clip against act_low / act_high (host arrays [act_dim]), the
 * env step of cstr_vec_step_f32; an episode ends when the step truncates (max_steps, or the NaN path) and is followed by the auto-reset
 * draw.  returns[c] = sum over the job's episodes, in order, of (the f64 sum of the episode's f32 step rewards)
 *                     + alive_bonus_offset * (double)lengths[c];  lengths[c] = the job's steps over all its episodes.
 * n_envs = 1: the env's random stream is consumed as by a sequential loop over the candidates; slots >= 2 n_delta do nothing and
 * their state is untouched; env_obs [N][obs_dim], step_count [N], pcg_state [N][4], static_init f64 [N][4 or 8] or NULL are left as
 * each slot's last job left them.
 * stats double[4] i/o: [0] sum of lengths, [1] sum of returns, [2] number of NaN returns -- fixed-order sums, written by the workgroup
 * that finishes last; [3] is the launch's 64-bit ticket: ZERO on entry, zero again on exit.
 * Mappings: n_hidden = 0: a slot per lane; otherwise a slot per wave (lane j owns unit j; one wave per workgroup, no cross-wave
 * barrier). At most ceil(2 n_delta / n_envs) * n_eval_episodes * max(coef->max_steps, 1) steps per slot whatever the data does.
 * CSTR_E_BADARG: NULL required pointers, n_envs <= 0, n_delta < 1, n_eval_episodes < 1, delta_std <= 0 or NaN, NaN alive_bonus_offset,
 * update_index outside 0 .. 2^32 - 1, act_high <= act_low, misaligned buffers (env_obs, pcg_state 16; returns, stats, static_init 8;
 * others 4), anything written overlapping theta or anything else written; CSTR_E_UNSUPPORTED: a policy cstr_ars_supported declines,
 * n_delta > CSTR_ARS_MAX_DELTA, unknown integrator. All checked before anything is enqueued. */
int cstr_ars_population_f32(const cstr_ars_policy_t *policy, const float *theta, float delta_std, uint64_t seed, int64_t update_index,
                            int n_delta, int n_eval_episodes, double alive_bonus_offset, const cstr_coef_t *coef, int integrator,
                            float *env_obs, int32_t *step_count, uint64_t *pcg_state, double *static_init, const float *act_low,
                            const float *act_high, int64_t n_envs, double *returns, int32_t *lengths, double *stats,
                            cstr_stream_t stream);

/* The update launch, on returns double[2 n_delta] (R+_k = returns[k], R-_k = returns[n_delta + k]):
 *   top_k = max(R+_k, R-_k), NaN if either is; directions in descending top_k, a NaN counting as the greatest and ties (two NaNs
 *   included) going to the lower k; the first n_top are kept: kept int32[n_top], in that order;
 *   return_std = unbiased standard deviation over the 2 n_top kept returns (R+ of the kept in order, then R-), float64;
 *   step_size = learning_rate / (n_top * return_std + 1e-6), float64;
 *   theta[p] = (float)((double)theta[p] + step_size * sum over the kept k, in order, of (R+_k - R-_k) * (double)delta[k][p]).
 * out double[2] = {step_size, return_std}. A kept NaN return makes step_size and every theta[p] NaN, as published. Sums have a fixed
 * order; no float atomics.
 * CSTR_E_BADARG: NULL pointers, n_params < 1, n_delta < 1, n_top outside 1 .. n_delta, update_index outside 0 .. 2^32 - 1, NaN
 * learning_rate, misaligned buffers, outputs overlapping returns or each other; CSTR_E_UNSUPPORTED: n_delta > CSTR_ARS_MAX_DELTA,
 * n_params > 4996 (net_arch [64, 64] on the (8, 4) layout). */
int cstr_ars_update_f32(float *theta, int64_t n_params, const double *returns, int n_delta, int n_top, double learning_rate, uint64_t seed,
                        int64_t update_index, double *out, int32_t *kept, cstr_stream_t stream);

/* ---- TRPO: trust-region policy steps on Fisher-vector products (csrc/cstr_trpo.hip) --------------------------------------------
 * At theta0 the new and the old distribution coincide, so the Hessian of the mean KL is the Fisher matrix and
 *   Fvp(v) = (1/R) sum_r J_r^T M_r J_r v + damping v
 * is a tangent (forward-mode) pass through the actor's Linear layers (cstr_linear_tangent_fwd_f32), the head's metric
 * (cstr_trpo_fisher_head_f32), the per-layer backward (cstr_linear_bwd_input_f32 / cstr_linear_bwd_weight_sets_f32) and one
 * conjugate-gradient launch (cstr_trpo_cg_step_f32), which folds the damping term in. Vectors over the parameters (g, x, r, p, s)
 * are ARENA-sized float arrays whose entries outside the actor's tensors are exactly zero.
 * Batch sums and dot products are float64 in a fixed order (no float atomics); a given shape always reduces the same way.
 * The control block, double[CSTR_TRPO_CTL_WORDS], lives on the device; the host reads none of it while train() runs. */
#define CSTR_TRPO_HEAD_GAUSSIAN 0         /* diagonal Gaussian, state-independent log_std: k0 = act_dim (2 or 4) */
#define CSTR_TRPO_HEAD_CATEGORICAL 1      /* k0 logits, 2 .. CSTR_TRPO_MAX_LOGITS */
#define CSTR_TRPO_HEAD_MULTICATEGORICAL 2 /* k0 + k1 logits in th.split order, 2 .. 32 each */
#define CSTR_TRPO_MAX_LOGITS 64
#define CSTR_TRPO_CTL_WORDS 16
#define CSTR_TRPO_CTL_RR 0        /* r . r of the conjugate-gradient iteration */
#define CSTR_TRPO_CTL_ALPHA 1
#define CSTR_TRPO_CTL_BETA 2
#define CSTR_TRPO_CTL_PAP 3       /* p . (F p + damping p) */
#define CSTR_TRPO_CTL_DONE 4      /* 1.0 once the iteration has returned: later step launches do nothing */
#define CSTR_TRPO_CTL_ITERS 5     /* step launches that did something */
#define CSTR_TRPO_CTL_SFS 6       /* s . (F s + damping s) */
#define CSTR_TRPO_CTL_STEP 7      /* sqrt(2 target_kl / sFs) */
#define CSTR_TRPO_CTL_COEFF 8     /* the line search's coefficient */
#define CSTR_TRPO_CTL_OBJECTIVE 9 /* the objective and the KL of the gradient-mode launch (the base of the line search) */
#define CSTR_TRPO_CTL_KL 10
#define CSTR_TRPO_CTL_LS_OBJECTIVE 11 /* ... of the last line-search launch */
#define CSTR_TRPO_CTL_LS_KL 12
#define CSTR_TRPO_CG_INIT 0
#define CSTR_TRPO_CG_STEP 1
#define CSTR_TRPO_CG_FINISH 2
#define CSTR_TRPO_MAX_VECTOR (1 << 24) /* floats of an arena-sized vector */

/* z_dot[m][n] = f'(y) * (x w_dot^T + x_dot w^T + b_dot): the tangent of one Linear + activation layer. f: CSTR_ACT_NONE, CSTR_ACT_TANH
 * (1 - y^2 from the stored output y[m][n]) or CSTR_ACT_RELU (y > 0). x [m][ldx >= k], x_dot [m][ldxd >= k] or NULL (the first layer: an
 * observation has no tangent), w, w_dot [n][k], b_dot [n], y and z_dot contiguous. One wave per 16 x 16 output tile on the f32 matrix
 * cores (v_mfma_f32_16x16x4_f32); the two products run in two independent accumulators that meet in the epilogue.
 * CSTR_E_BADARG: NULL pointers (y only with an activation), sizes < 1, a row stride below k, buffers not 4-byte aligned, z_dot
 * overlapping an input; CSTR_E_UNSUPPORTED: unknown activation, m, n or k above 2^23 - 1, more than 65535 row tiles, a row stride
 * above 2^31 - 1. */
int cstr_linear_tangent_fwd_f32(const float *x, int64_t ldx, const float *x_dot, int64_t ldxd, const float *w, const float *w_dot,
                                const float *b_dot, const float *y, int act, float *z_dot, int64_t m, int64_t n, int64_t k,
                                cstr_stream_t stream);

typedef struct {
    const float *dist;        /* the action mean [R][ld] or the logits [R][ld] at the current parameters */
    int64_t ld;
    const float *log_std;     /* Gaussian head: [k0] at the current parameters; NULL otherwise */
    const float *old_dist;    /* the same two at theta0, held constant (may be the very same buffers) */
    int64_t old_ld;
    const float *old_log_std;
    const float *actions;     /* [R][k0] (Gaussian), [R] the index as a float, [R][2] the level pair as floats */
    const float *old_log_prob;/* [R], the rollout buffer's */
    const float *adv;         /* [R] */
    int64_t batch;            /* R */
    int32_t head, k0, k1, normalize_advantage;
    int32_t line_search, reserved;
    double target_kl, shrink; /* line-search mode */
    float *g_dist;            /* gradient mode: d objective / d dist, [R][width] contiguous */
    float *g_log_std;         /* gradient mode, Gaussian head: d objective / d log_std [k0] */
    float *scalars_out;       /* [2]: objective, kl; may be NULL */
    double *ctl;              /* the control block */
    int32_t *accepted;        /* line-search mode: 1 iff kl' < target_kl and objective' > objective */
} cstr_trpo_objective_t;

/* One launch for everything between the actor's outputs and the backward: adv = (adv - mean) / (std + 1e-8) over the R rows (with
 * normalize_advantage; std unbiased), log_prob (the heads' shared device functions, in double), ratio = exp(log_prob - old_log_prob),
 * objective = mean(adv ratio), kl = mean_r KL(new_r || old_r) summed over action dimensions or sub-distributions.
 * Gradient mode (line_search = 0): also d objective / d (mean, log_std) or d objective / d logits; ctl[OBJECTIVE], ctl[KL] are
 * written and ctl[COEFF] = 1. Line-search mode: no gradients; *accepted = kl < target_kl && objective > ctl[OBJECTIVE];
 * ctl[LS_OBJECTIVE], ctl[LS_KL] are written and ctl[COEFF] *= shrink when the step was not accepted.
 * Every per-row quantity is formed in double from the float inputs; stores are float. Any R up to CSTR_PPO_MAX_ROWS: the grid is
 * capped at CSTR_PPO_MAX_BLOCKS workgroups, which stride over the rows. workspace: uint64[CSTR_PPO_WS_WORDS], zero before first use.
 * CSTR_E_BADARG: NULL struct or required pointers, R < 1, strides below the width, misaligned buffers, an output overlapping an input or
 * another output, target_kl <= 0 or shrink outside (0, 1) in line-search mode; CSTR_E_UNSUPPORTED: a head or width outside the list. */
int cstr_trpo_objective_f32(const cstr_trpo_objective_t *p, uint64_t *workspace, cstr_stream_t stream);

/* The Fisher metric of the head in distribution-parameter space, times the tangent, over R: upstream [R][width] contiguous is what the
 * per-layer backward takes as d / d (mean | logits).
 *   Gaussian: upstream[r][a] = dist_dot[r][a] * exp(-2 log_std[a]) / R, and g_log_std[a] = 2 v_log_std[a] (no cross terms);
 *   (Multi)Categorical, per block of logits with p = softmax(dist[r]): upstream[r] = (p * dist_dot[r] - p (p . dist_dot[r])) / R.
 * dist_dot [R][ldd]: the tangent of the mean / logits. dist [R][ld]: the logits at theta0 (discrete heads; NULL for the Gaussian).
 * CSTR_E_BADARG / CSTR_E_UNSUPPORTED as for cstr_trpo_objective_f32. */
int cstr_trpo_fisher_head_f32(int head, int k0, int k1, const float *dist_dot, int64_t ldd, const float *dist, int64_t ld,
                              const float *log_std, const float *v_log_std, int64_t batch, float *upstream, float *g_log_std,
                              cstr_stream_t stream);

/* One conjugate-gradient launch (a single workgroup) over n-float vectors; ap = F v WITHOUT the damping term, as the backward left
 * it; the launch adds damping * v itself. Scalars and dot products are double in ctl.
 *   CSTR_TRPO_CG_INIT   (ap = F x): r = g - (ap + damping x); p = r; rr = r . r; done = rr < residual_tol; iters = 0.
 *   CSTR_TRPO_CG_STEP   (ap = F p): nothing when done. Otherwise Ap = ap + damping p; alpha = rr / (p . Ap); x += alpha p; with
 *                       `last` (the iteration max_iter - 1) done = 1 and return; r -= alpha Ap; new_rr = r . r; if new_rr <
 *                       residual_tol done = 1 and return; beta = new_rr / rr; rr = new_rr; p = r + beta p.
 *   CSTR_TRPO_CG_FINISH (ap = F x): sFs = x . (ap + damping x); step = sqrt(2 target_kl / sFs); coeff = 1. r, p, g may be NULL.
 * CSTR_E_BADARG: NULL or misaligned pointers, overlapping vectors, n < 1, unknown mode, negative or NaN damping / residual_tol,
 * target_kl <= 0 in the finishing form; CSTR_E_UNSUPPORTED: n > CSTR_TRPO_MAX_VECTOR. */
int cstr_trpo_cg_step_f32(int mode, float *x, float *r, float *p, const float *ap, const float *g, int64_t n, double damping,
                          double residual_tol, double target_kl, int last, double *ctl, cstr_stream_t stream);

/* theta[i] = theta0[i] + (ctl[COEFF] * ctl[STEP]) * s[i] where mask[i] != 0 (the actor's tensors); every other float of theta is left
 * untouched. CSTR_E_BADARG: NULL / misaligned pointers, n < 1, theta overlapping an input; CSTR_E_UNSUPPORTED: n > CSTR_TRPO_MAX_VECTOR. */
int cstr_trpo_apply_step_f32(float *theta, const float *theta0, const float *s, const float *mask, int64_t n, const double *ctl,
                             cstr_stream_t stream);

/* The critic minibatch's loss launch (a single workgroup): loss = mean((returns - values)^2), g_value[b] = 2 (values[b] - returns[b]) /
 * batch; loss_out[0] = loss and loss_sum[0] += loss where given. CSTR_E_BADARG: NULL / misaligned pointers, batch < 1, overlaps. */
int cstr_trpo_value_loss_f32(const float *values, const float *returns, int64_t batch, float *g_value, float *loss_out, float *loss_sum,
                             cstr_stream_t stream);

/* x[i] = scale * N(0, 1) where mask[i] != 0, 0 elsewhere: the conjugate gradient's start. Philox4x32-10 keyed by rng_ctl[0], counter
 * (rng_ctl[1] + i / 2, 0, 0x7290C6A5), one Box-Muller pair per counter for the floats 2j and 2j + 1; the last workgroup advances
 * rng_ctl[1] by (n + 1) / 2. CSTR_E_BADARG: NULL / misaligned pointers, n < 1, overlaps; CSTR_E_UNSUPPORTED: n > CSTR_TRPO_MAX_VECTOR. */
int cstr_trpo_x0_f32(float *x, const float *mask, int64_t n, float scale, uint64_t *rng_ctl, cstr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CSTR_RL_HIP_H */
