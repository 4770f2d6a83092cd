"""`MlpLstmPolicy` (sb3_contrib's RecurrentActorCriticPolicy on a flat Box observation): features -> lstm_actor / lstm_critic (each
nn.LSTM(K, H), one layer) -> mlp_extractor on H inputs -> action_net / value_net, a state-independent log_std.

Construction order: the parent ActorCriticPolicy (mlp_extractor, action_net, log_std, value_net, orthogonal initialisation), then
lstm_actor, then lstm_critic (or `critic`, a Linear(K, H), with enable_critic_lstm=False and no shared LSTM), then ONE optimiser over all
parameters in one flat arena. The LSTMs keep nn.LSTM's own initialisation. Seeded-initialisation parity with sb3_contrib is not claimed.

The nn.LSTM modules own the parameters and give the state_dict its keys; they are never called on the device (MIOpen's weight
flattening would move the parameters out of the arena): the kernel path runs csrc/cstr_lstm.hip, the torch path `lstm_torch` below."""
import numpy as np
import torch as th
from torch import nn
from torch.nn import functional as F

from core.common.policies import ActorCriticPolicy


def lstm_weights(lstm: nn.LSTM) -> tuple:
    return lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0


def lstm_torch(lstm: nn.LSTM, x: th.Tensor, episode_start: th.Tensor, state_h: th.Tensor, state_c: th.Tensor, table: np.ndarray):
    """The kernels' statement as torch statements (differentiable): every segment of `table` [n_seg, 3] walked step by step, h and c
    multiplied by 1 - episode_start first. -> (out [R, H], hn [n_seg, H], cn [n_seg, H])"""
    w_ih, w_hh, b_ih, b_hh = lstm_weights(lstm)
    dev = x.device
    first, lens = table[:, 0].astype(np.int64), table[:, 1].astype(np.int64)
    init = th.from_numpy(table[:, 2].astype(np.int64)).to(dev)
    h, c = state_h[init], state_c[init]
    rows_all, outs = [], []
    for t in range(int(lens.max())):
        live = np.flatnonzero(lens > t)
        act = th.from_numpy(live).to(dev)
        rows = th.from_numpy(first[live] + t).to(dev)
        m = (1.0 - episode_start[rows])[:, None]
        hh, cc = h[act] * m, c[act] * m
        z = F.linear(x[rows], w_ih, b_ih) + F.linear(hh, w_hh, b_hh)
        i, f, g, o = z.chunk(4, dim=1)
        cc = th.sigmoid(f) * cc + th.sigmoid(i) * th.tanh(g)
        hh = th.sigmoid(o) * th.tanh(cc)
        h, c = h.index_copy(0, act, hh), c.index_copy(0, act, cc)
        rows_all.append(rows), outs.append(hh)
    out = x.new_zeros(x.shape[0], w_hh.shape[1]).index_copy(0, th.cat(rows_all), th.cat(outs))
    return out, h, c


class RecurrentActorCriticPolicy(ActorCriticPolicy):
    def __init__(self, observation_space, action_space, lr_schedule, lstm_hidden_size: int = 256, n_lstm_layers: int = 1,
                 shared_lstm: bool = False, enable_critic_lstm: bool = True, lstm_kwargs=None, **kwargs):
        if n_lstm_layers != 1:
            raise ValueError(f"MlpLstmPolicy is built for n_lstm_layers=1, got {n_lstm_layers}")
        if lstm_kwargs:
            raise ValueError("MlpLstmPolicy takes no lstm_kwargs: a single-layer, unidirectional nn.LSTM without dropout")
        assert not (shared_lstm and enable_critic_lstm), "You must choose between shared LSTM, seperate or no LSTM for the critic."
        self.lstm_hidden_size = int(lstm_hidden_size)
        super().__init__(observation_space, action_space, lr_schedule, **kwargs)
        self.n_lstm_layers, self.shared_lstm, self.enable_critic_lstm = 1, bool(shared_lstm), bool(enable_critic_lstm)
        self.lstm_actor = nn.LSTM(self.features_dim, self.lstm_hidden_size, num_layers=1)
        self.lstm_critic = self.critic = None
        if self.enable_critic_lstm:
            self.lstm_critic = nn.LSTM(self.features_dim, self.lstm_hidden_size, num_layers=1)
        elif not self.shared_lstm:
            self.critic = nn.Linear(self.features_dim, self.lstm_hidden_size)

    def _mlp_input_dim(self) -> int:
        return self.lstm_hidden_size

    # ---- torch statements (the fallback path and the tests' reference) -------------------------------------------------------------------
    def latents_torch(self, obs, episode_start, states: dict, table: np.ndarray):
        """-> (actor features [R, H], critic features [R, H], new states {pi_h, pi_c, vf_h, vf_c} [n_seg, H])"""
        x = obs.to(self.log_std.dtype)
        pi, pi_h, pi_c = lstm_torch(self.lstm_actor, x, episode_start, states["pi_h"], states["pi_c"], table)
        if self.lstm_critic is not None:
            vf, vf_h, vf_c = lstm_torch(self.lstm_critic, x, episode_start, states["vf_h"], states["vf_c"], table)
        else:
            vf = pi.detach() if self.shared_lstm else self.critic(x)
            vf_h, vf_c = pi_h.detach(), pi_c.detach()
        return pi, vf, dict(pi_h=pi_h, pi_c=pi_c, vf_h=vf_h, vf_c=vf_c)

    def heads_torch(self, latent_pi, latent_vf):
        """-> (action mean [R, A], values [R, 1])"""
        return self.action_net(self.mlp_extractor.forward_actor(latent_pi)), self.value_net(self.mlp_extractor.forward_critic(latent_vf))

    def evaluate_actions_torch(self, obs, actions, episode_start, states: dict, table: np.ndarray):
        """sb3_contrib's evaluate_actions on one chunk -> (values [R, 1], log_prob [R], entropy [R])"""
        pi, vf, _ = self.latents_torch(obs, episode_start, states, table)
        mean, values = self.heads_torch(pi, vf)
        dist = self.action_dist.proba_distribution(mean, self.log_std)
        return values, dist.log_prob(actions), dist.entropy()

    def forward(self, *args, **kwargs):
        raise NotImplementedError("MlpLstmPolicy is stepped by RecurrentPPO (collect_rollouts / predict), which carries the LSTM states")

    evaluate_actions = get_distribution = predict_values = _predict = forward


MlpLstmPolicy = RecurrentActorCriticPolicy
