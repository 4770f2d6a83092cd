"""RecurrentPPO (sb3_contrib's algorithm: PPO with an LSTM actor and an LSTM critic) on the HIP path.

Rollout step (device env, no host synchronisation): the two LSTM steps (csrc/cstr_lstm.hip in its rollout mode: one length-1 segment per
env, the new state written straight into the buffer's next state slot), both MLPs on the per-layer Linear kernels, the Gaussian head, the
env step, the critic once more on the terminal observations with its POST-step state and no reset (the bootstrap value of a truncated
episode), the buffer's add launch.

Minibatch step: see core/ppo_recurrent/buffers.py for the chunks and their segments. Both LSTM forwards in training mode, the extractor /
head / cstr_ppo_loss_f32 launches of PPO, their backwards down to d loss / d (LSTM outputs), the two LSTM backwards, ONE
cstr_linear_bwd_weight_sets_f32 launch for dW_ih, dW_hh and db of both LSTMs (bias_ih and bias_hh receive the same gradient), the
global-norm clip and the flat Adam step. Loss means and the advantage normalisation run over the chunk's rows, which equals sb3_contrib's
padded-sequence form up to rounding.

`fused_learner` False -- set by hand, a non-default optimiser, a width cstr_lstm_supported declines, enable_critic_lstm=False or
shared_lstm=True -- runs the same algorithm as torch statements on the same buffer and segment tables.

Refused at construction: n_lstm_layers != 1, gSDE, the Discrete / MultiDiscrete / goal faces, VecNormalize, data-parallel runs; an env that
is not a CSTRVecEnv; hipGraph replay (enable_graph_capture)."""
from typing import Optional, Union

import numpy as np
import torch as th

from core.common import fused, hip_ops
from core.common.logger import DeviceMean
from core.common.spaces import Discrete, MultiDiscrete
from core.ppo.ppo import PPO
from core.ppo_recurrent.buffers import STATE_NAMES, RecurrentRolloutBuffer
from core.ppo_recurrent.policies import MlpLstmPolicy, lstm_weights


class RecurrentPPO(PPO):
    policy_aliases = {"MlpLstmPolicy": MlpLstmPolicy}
    goal_face_support = False

    def __init__(self, policy, env, learning_rate=3e-4, n_steps: int = 128, batch_size: int = 128, n_epochs: int = 10, gamma: float = 0.99,
                 gae_lambda: float = 0.95, clip_range=0.2, clip_range_vf=None, normalize_advantage: bool = True, ent_coef: float = 0.0,
                 vf_coef: float = 0.5, max_grad_norm: float = 0.5, use_sde: bool = False, sde_sample_freq: int = -1,
                 target_kl: Optional[float] = None, stats_window_size: int = 100, tensorboard_log: Optional[str] = None,
                 policy_kwargs: Optional[dict] = None, verbose: int = 0, seed: Optional[int] = None, device: Union[th.device, str] = "auto",
                 _init_setup_model: bool = True):
        if (policy_kwargs or {}).get("n_lstm_layers", 1) != 1:
            raise ValueError(f"RecurrentPPO is built for n_lstm_layers=1, got {policy_kwargs['n_lstm_layers']}")
        super().__init__(policy, env, learning_rate=learning_rate, n_steps=n_steps, batch_size=batch_size, n_epochs=n_epochs, gamma=gamma,
                         gae_lambda=gae_lambda, clip_range=clip_range, clip_range_vf=clip_range_vf, normalize_advantage=normalize_advantage,
                         ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, use_sde=use_sde, sde_sample_freq=sde_sample_freq,
                         target_kl=target_kl, stats_window_size=stats_window_size, tensorboard_log=tensorboard_log,
                         policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device, _init_setup_model=False)
        if isinstance(self.action_space, (Discrete, MultiDiscrete)):
            raise ValueError("RecurrentPPO is built for the Box valve face: the Discrete and MultiDiscrete faces are not")
        if self.env is not None and self._denv is None:
            raise NotImplementedError("RecurrentPPO steps a device-resident CSTRVecEnv; other VecEnvs are not built")
        if _init_setup_model:
            self._setup_model()

    # ---- setup ----------------------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        hidden = int(self.policy_kwargs.get("lstm_hidden_size", 256))
        self.rollout_buffer_class = RecurrentRolloutBuffer
        self.rollout_buffer_kwargs = dict(self.rollout_buffer_kwargs, hidden_size=hidden)
        super()._setup_model()  # OnPolicyAlgorithm: buffer, policy in one arena; PPO: schedules, loss workspace
        pol, dev, n = self.policy, self.device, self.n_envs
        k = pol.features_dim
        self._fast = None
        if (pol.flat_optimizers() and pol.lstm_critic is not None and hip_ops.lstm_supported(k, hidden)
                and hip_ops.ppo_supported(k, pol.action_net.out_features) and fused.FastMLP.supported(pol.mlp_extractor.policy_net)
                and fused.FastMLP.supported(pol.mlp_extractor.value_net) and all(p.grad is not None for p in pol.parameters())):
            self._fast = fused.FastActorCritic(pol, self._device_rng())
        self._fused_learner = self._fast is not None
        pol.fast = None  # the policy's own entry points are not used: this class steps it
        with th.cuda.device(dev):
            self._step_segs = hip_ops.LstmSegments([(i, 1, i) for i in range(n)], dev)
        z = lambda *s: th.zeros(*s, dtype=th.float32, device=dev)  # noqa: E731
        self._no_start = z(n)
        self._term = {k_: z(n, hidden) for k_ in ("h", "c")}
        self._act_bufs = dict(action=z(n, pol.action_net.out_features), env_action=z(n, pol.action_net.out_features), log_prob=z(n))
        low, high = (th.as_tensor(getattr(pol.action_space, a), dtype=th.float32).reshape(-1).to(dev).contiguous() for a in ("low", "high"))
        self._bounds = (low, high)
        self._lstm_bufs: dict = {}
        self.last_rollout_debug: list = []

    def _device_rollout(self) -> bool:
        return True

    def _setup_learn(self, total_timesteps, callback=None, reset_num_timesteps=True, tb_log_name="run", progress_bar=False):
        resetting = reset_num_timesteps or self._last_obs is None
        out = super()._setup_learn(total_timesteps, callback, reset_num_timesteps, tb_log_name, progress_bar)
        if resetting:  # fresh episodes: the states the next rollout starts from are zero
            for v in self.rollout_buffer.hidden.values():
                v[self.n_steps].zero_()
        return out

    # ---- one LSTM step for all envs ---------------------------------------------------------------------------------
    def _lstm_step(self, lstm, x, episode_start, h, c, hn, cn) -> None:
        """(h, c) [n, H] -> (hn, cn) [n, H] for one observation per env"""
        if self._fused_learner:
            segs = self._step_segs if x.shape[0] == self.n_envs else hip_ops.LstmSegments([(i, 1, i) for i in range(x.shape[0])], x.device)
            hip_ops.lstm_seq_fwd(x, episode_start, *(w.detach() for w in lstm_weights(lstm)), h, c, segs, hn, cn)
            return
        w_ih, w_hh, b_ih, b_hh = lstm_weights(lstm)
        m = (1.0 - episode_start)[:, None]
        z = th.nn.functional.linear(x, w_ih, b_ih) + th.nn.functional.linear(h * m, w_hh, b_hh)
        i, f, g, o = z.chunk(4, dim=1)
        cn.copy_(th.sigmoid(f) * (c * m) + th.sigmoid(i) * th.tanh(g))
        hn.copy_(th.sigmoid(o) * th.tanh(cn))

    def _mean(self, latent_pi):
        return self._fast.mean(latent_pi) if self._fused_learner else self.policy.action_net(self.policy.mlp_extractor.forward_actor(latent_pi))

    def _values(self, latent_vf):
        pol = self.policy
        return self._fast.values(latent_vf) if self._fused_learner else pol.value_net(pol.mlp_extractor.forward_critic(latent_vf))

    def _critic_latent(self, x, episode_start, t_from: int, hn, cn, pi_latent=None):
        """the critic's features for one observation per env from the state in slot t_from (its own LSTM, the actor's, or a Linear)"""
        pol, hid = self.policy, self.rollout_buffer.hidden
        if pol.lstm_critic is not None:
            self._lstm_step(pol.lstm_critic, x, episode_start, hid["vf_h"][t_from], hid["vf_c"][t_from], hn, cn)
            return hn
        if pol.shared_lstm:
            if pi_latent is None:
                self._lstm_step(pol.lstm_actor, x, episode_start, hid["pi_h"][t_from], hid["pi_c"][t_from], hn, cn)
                return hn
            return pi_latent
        return pol.critic(x)

    # ---- rollouts ---------------------------------------------------------------------------------------------------
    def collect_rollouts(self, env, callback, rollout_buffer, n_rollout_steps: int) -> bool:
        assert self._last_obs is not None, "No previous observation was provided"
        self.policy.set_training_mode(False)
        rollout_buffer.reset()
        rollout_buffer.carry_over()
        callback.on_rollout_start()
        noop_cb = getattr(callback, "is_noop", False)
        denv, hid, pol = self._denv, rollout_buffer.hidden, self.policy
        self.last_rollout_debug = []
        self._starts_on = "device"
        with th.no_grad(), th.cuda.device(self.device):
            for t in range(n_rollout_steps):
                self._obs_prev.copy_(denv.obs)
                es = self._episode_starts_dev
                self._lstm_step(pol.lstm_actor, self._obs_prev, es, hid["pi_h"][t], hid["pi_c"][t], hid["pi_h"][t + 1], hid["pi_c"][t + 1])
                latent_vf = self._critic_latent(self._obs_prev, es, t, hid["vf_h"][t + 1], hid["vf_c"][t + 1], pi_latent=hid["pi_h"][t + 1])
                mean, values = self._mean(hid["pi_h"][t + 1]), self._values(latent_vf)
                b = self._act_bufs
                eps = self._fast.eps_queue.pop(0).to(self.device, th.float32).contiguous() if (self._fast and self._fast.eps_queue) else None
                hip_ops.diag_gaussian_act(mean.contiguous(), pol.log_std.detach(), eps, None if eps is not None else self._device_rng(),
                                          *self._bounds, False, b["action"], b["env_action"], b["log_prob"])
                new_obs, rewards, dones, timeouts, terminal_obs = denv.step_device(b["env_action"])
                # the bootstrap value of a truncated episode: the critic on the terminal observation, its state AFTER this step, no reset
                term_latent = self._critic_latent(terminal_obs, self._no_start, t + 1, self._term["h"], self._term["c"])
                terminal_values = self._values(term_latent)
                if self.debug_capture:
                    self.last_rollout_debug.append(dict(terminal_obs=terminal_obs.clone(), terminal_values=terminal_values.reshape(-1).clone(),
                                                        timeouts=timeouts.clone()))
                self.num_timesteps += env.num_envs
                if not noop_cb:
                    callback.update_locals(locals())
                if not callback.on_step():
                    return False
                rollout_buffer.add_device(self._obs_prev, b["action"], rewards, es, values.reshape(-1), b["log_prob"], timeouts,
                                          terminal_values.reshape(-1), dones, self._ep_return, self._ep_len, self._ep_stats)
                self._last_obs = new_obs
            # the value behind the last step: episode starts are the last dones (the add launch left them in place)
            last_latent = self._critic_latent(new_obs, self._episode_starts_dev, n_rollout_steps, self._term["h"], self._term["c"])
            rollout_buffer.compute_returns_and_advantage(last_values=self._values(last_latent).reshape(-1), dones=dones)
        if not noop_cb:
            callback.update_locals(locals())
        callback.on_rollout_end()
        return True

    # ---- train ------------------------------------------------------------------------------------------------------
    def _net_bufs(self, rows: int, n_seg: int) -> dict:
        key = (rows, n_seg)
        b = self._lstm_bufs.get(key)
        if b is None:
            h = self.rollout_buffer.hidden_size
            e = lambda *s: th.empty(*s, dtype=th.float32, device=self.device)  # noqa: E731
            b = self._lstm_bufs[key] = {net: dict(out=e(rows, h), gates=e(rows, 4 * h), c_seq=e(rows, h), h_prev=e(rows, h), dgates=e(rows, 4 * h),
                                                  hn=e(n_seg, h), cn=e(n_seg, h), dh0=e(n_seg, h), dc0=e(n_seg, h)) for net in ("pi", "vf")}
        return b

    def _chunk_fused(self, rd, es, segs, clip_range, clip_range_vf, sums):
        pol, rb = self.policy, self.rollout_buffer
        rows = rd.observations.shape[0]
        nets = self._net_bufs(rows, segs.n)
        b = self._bufs(rows)
        feats = {}
        for net, lstm in (("pi", pol.lstm_actor), ("vf", pol.lstm_critic)):
            nb = nets[net]
            hip_ops.lstm_seq_fwd(rd.observations, es, *(w.detach() for w in lstm_weights(lstm)), rb.state_rows(net + "_h"),
                                 rb.state_rows(net + "_c"), segs, nb["hn"], nb["cn"], out=nb["out"], gates=nb["gates"], c_seq=nb["c_seq"],
                                 h_prev=nb["h_prev"])
            feats[net] = nb["out"].detach().requires_grad_(True)
        mean = self._fast.mean(feats["pi"], train_params=True)
        values = self._fast.values(feats["vf"], train_params=True)
        hip_ops.ppo_loss(mean.detach(), pol.log_std.detach(), rd.actions, values.detach(), rd.old_values, rd.old_log_prob, rd.advantages,
                         rd.returns, clip_range, clip_range_vf, self.normalize_advantage, self.ent_coef, self.vf_coef, b["g_mean"],
                         b["g_value"], pol.log_std.grad, self._ws, scalars_out=self._scalars, scalars_sum=sums,
                         log_prob_out=b["log_prob"] if self.debug_capture else None)
        return mean, values, b, feats, nets

    def _update_fused(self, rd, es, segs, mean, values, b, feats, nets) -> None:
        pol, rb = self.policy, self.rollout_buffer
        with fused.deferred_weight_grads():
            th.autograd.backward([mean, values], [b["g_mean"], b["g_value"]])
        sets = []
        for net, lstm in (("pi", pol.lstm_actor), ("vf", pol.lstm_critic)):
            nb = nets[net]
            w_ih, w_hh, b_ih, _ = lstm_weights(lstm)
            hip_ops.lstm_seq_bwd(feats[net].grad.contiguous(), nb["gates"], nb["c_seq"], rb.state_rows(net + "_c"), es, w_hh.detach(), segs,
                                 nb["dgates"], nb["dh0"], nb["dc0"])  # dh0 / dc0: the stored states are constants, the gradient is dropped
            sets += [(nb["dgates"], nb["h_prev"], w_hh.grad, None), (nb["dgates"], rd.observations, w_ih.grad, b_ih.grad)]
        hip_ops.linear_bwd_weight_sets(sets)
        for lstm in (pol.lstm_actor, pol.lstm_critic):
            lstm.bias_hh_l0.grad.copy_(lstm.bias_ih_l0.grad)
        hip_ops.grad_clip(pol.arena.grad, self.max_grad_norm, self._ws, self._grad_norm)
        pol.optimizer.step()

    def _chunk_torch(self, rd, es, segs, clip_range, clip_range_vf, sums):
        pol, rb = self.policy, self.rollout_buffer
        states = {k: rb.state_rows(k) for k in STATE_NAMES}
        values, log_prob, entropy = pol.evaluate_actions_torch(rd.observations, rd.actions, es, states, segs.host)
        values = values.flatten()
        adv = rd.advantages
        if self.normalize_advantage and len(adv) > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = th.exp(log_prob - rd.old_log_prob)
        policy_loss = -th.min(adv * ratio, adv * th.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
        clip_fraction = th.mean((th.abs(ratio - 1) > clip_range).float())
        pred = values if clip_range_vf is None else rd.old_values + th.clamp(values - rd.old_values, -clip_range_vf, clip_range_vf)
        value_loss = th.nn.functional.mse_loss(rd.returns, pred)
        entropy_loss = -th.mean(entropy)
        loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss
        with th.no_grad():
            log_ratio = log_prob - rd.old_log_prob
            approx_kl = th.mean((th.exp(log_ratio) - 1) - log_ratio)
            self._scalars.copy_(th.stack([policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction]).detach())
            sums += self._scalars
        return loss, values.detach(), log_prob.detach()

    def train(self) -> None:
        self.policy.set_training_mode(True)
        self._update_learning_rate(self.policy.optimizer)
        clip_range = self.clip_range(self._current_progress_remaining)
        clip_range_vf = None if self.clip_range_vf is None else self.clip_range_vf(self._current_progress_remaining)
        if self._sums.shape[0] != max(self.n_epochs, 1):
            self._sums = th.zeros(max(self.n_epochs, 1), 6, dtype=th.float32, device=self.device)
        self._sums.zero_()
        self.last_train_minibatches = []
        n_minibatches, n_last_epoch, last_epoch = 0, 0, 0
        continue_training = True
        with th.cuda.device(self.device):
            for epoch in range(self.n_epochs):
                n_last_epoch, last_epoch = 0, epoch
                sums = self._sums[epoch]
                for rd, es, segs in self.rollout_buffer.get(self.batch_size):
                    if self._fused_learner:
                        step = self._chunk_fused(rd, es, segs, clip_range, clip_range_vf, sums)
                    else:
                        loss, values, log_prob = self._chunk_torch(rd, es, segs, clip_range, clip_range_vf, sums)
                    n_minibatches += 1
                    n_last_epoch += 1
                    if self.debug_capture:
                        self.last_train_minibatches.append(dict(scalars=self._scalars.clone(), epoch=epoch, rows=rd.observations.shape[0]))
                    if self.target_kl is not None and float(self._scalars[4]) > 1.5 * self.target_kl:
                        continue_training = False
                        if self.verbose >= 1:
                            print(f"Early stopping at step {epoch} due to reaching max kl: {float(self._scalars[4]):.2f}")
                        break
                    if self._fused_learner:
                        self._update_fused(rd, es, segs, *step)
                    else:
                        self.policy.optimizer.zero_grad()
                        loss.backward()
                        norm = th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
                        self._grad_norm.copy_(norm.detach().reshape(1))
                        self.policy.optimizer.step()
                self._n_updates += 1
                if not continue_training:
                    break
            rb = self.rollout_buffer
            with th.no_grad():
                totals = self._sums.sum(dim=0)
                kl_sum, last_loss = self._sums[last_epoch, 4].clone(), self._scalars[3].clone()
                y_pred, y_true = rb.values.flatten(), rb.returns.flatten()
                var_y = y_true.var(unbiased=False)
                explained_var = th.where(var_y == 0, th.full_like(var_y, float("nan")), 1 - (y_true - y_pred).var(unbiased=False) / var_y)
                std = th.exp(self.policy.log_std.detach()).mean()
        count = max(n_minibatches, 1)
        for key, value in (("entropy_loss", DeviceMean(totals[2], count)), ("policy_gradient_loss", DeviceMean(totals[0], count)),
                           ("value_loss", DeviceMean(totals[1], count)), ("approx_kl", DeviceMean(kl_sum, max(n_last_epoch, 1))),
                           ("clip_fraction", DeviceMean(totals[5], count)), ("loss", DeviceMean(last_loss, 1)),
                           ("explained_variance", DeviceMean(explained_var, 1)), ("std", DeviceMean(std, 1))):
            self.logger.record("train/" + key, value)
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/clip_range", clip_range)
        if self.clip_range_vf is not None:
            self.logger.record("train/clip_range_vf", clip_range_vf)

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 1, tb_log_name: str = "RecurrentPPO",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps=total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                             reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)

    @classmethod
    def _construct_for_load(cls, env, device, ctor: dict):
        return cls("MlpLstmPolicy", env, device=device, **ctor)

    # ---- predict ----------------------------------------------------------------------------------------------------
    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """-> (actions, state): state = (h, c) of the actor LSTM, [1, n_envs, H] each (NumPy), as sb3_contrib returns it"""
        pol = self.policy
        pol.set_training_mode(False)
        obs, vectorized = pol.obs_to_tensor(observation)
        n, hidden, dev = obs.shape[0], self.rollout_buffer.hidden_size, self.device
        with th.no_grad(), th.cuda.device(dev):
            to = lambda a: th.as_tensor(np.asarray(a, dtype=np.float32)).reshape(n, -1).to(dev).contiguous()  # noqa: E731
            h, c = (th.zeros(n, hidden, device=dev), th.zeros(n, hidden, device=dev)) if state is None else (to(state[0]), to(state[1]))
            es = th.zeros(n, device=dev) if episode_start is None else to(episode_start).reshape(n)
            hn, cn = th.empty_like(h), th.empty_like(c)
            self._lstm_step(pol.lstm_actor, obs.float().contiguous(), es, h, c, hn, cn)
            mean = self._mean(hn)
            actions = mean if deterministic else mean + th.exp(pol.log_std) * th.randn_like(mean)
        actions = np.clip(actions.cpu().numpy().reshape((-1, *pol.action_space.shape)), pol.action_space.low, pol.action_space.high)
        return (actions if vectorized else actions.squeeze(axis=0)), (hn.cpu().numpy()[None], cn.cpu().numpy()[None])
