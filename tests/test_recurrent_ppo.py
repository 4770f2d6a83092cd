"""RecurrentPPO on the MI355X: one train() of the kernel path against the torch-statement path on the same model and the same filled buffer
(the 4 x rule: both against the same statements in float64), the segment tables against a plain Python restatement, the timeout bootstrap,
predict's state, a save / load round trip, a short learn(), the refusals that need a device env."""
import numpy as np
import pytest
import torch as th

from core import _native as nv
from core.common.vec_env import CSTRVecEnv
from core.ppo_recurrent import RecurrentPPO, segment_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, B, H = 20, 6, 32, 16
SPLIT = 37  # chunks cut sequences mid-env and wrap past the end


def make(max_steps=7, **kw):
    env = CSTRVecEnv(N, device=DEV)
    env.coef = nv.default_coef(0.20, 0.05, 0.45, max_steps)  # short episodes: resets inside the segments, timeouts in the rollout
    return RecurrentPPO("MlpLstmPolicy", env, n_steps=T, batch_size=B, n_epochs=1, seed=0, device=DEV, policy_kwargs=dict(lstm_hidden_size=H), **kw)


@pytest.fixture(scope="module")
def filled():
    """a model behind two rollouts (carried LSTM states, episode ends) and no optimiser step"""
    model = make()
    model.debug_capture = True
    _, cb = model._setup_learn(2 * T * N, None)
    for _ in range(2):
        assert model.collect_rollouts(model.env, cb, model.rollout_buffer, T)
    th.cuda.synchronize()
    return model


def _clone(model):
    """a fresh model with the given one's parameters and buffer contents (fields, LSTM states)"""
    m = make()
    m.policy.load_state_dict(model.policy.state_dict())
    src, dst = model.rollout_buffer, m.rollout_buffer
    for name in src._FIELDS:
        getattr(dst, name).copy_(getattr(src, name))
    for k, v in src.hidden.items():
        dst.hidden[k].copy_(v)
    dst.rb.ctl.copy_(src.rb.ctl)
    dst._adds = src._adds
    m.debug_capture = True
    return m


def _train(model, fused):
    m = _clone(model)
    m.fused_learner = fused
    m.rollout_buffer.forced_splits = [SPLIT]
    m.train()
    th.cuda.synchronize()
    return m, th.stack([c["scalars"] for c in m.last_train_minibatches]).cpu().double()


def _train64(model):
    """train()'s statements in float64 with torch's own Adam and clip -> (policy, scalars per chunk)"""
    src = model.policy
    pol = type(src)(src.observation_space, src.action_space, lambda _: 3e-4, lstm_hidden_size=H)
    pol.load_state_dict({k: v.cpu() for k, v in src.state_dict().items()})
    pol = pol.double().to(DEV)
    opt = th.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5)
    rb = _clone(model).rollout_buffer
    rb.forced_splits = [SPLIT]
    states = {k: rb.state_rows(k).double() for k in rb.hidden}
    scalars = []
    for rd, es, segs in rb.get(B):
        obs, act, old_v, old_lp, adv, ret = (t.double() for t in rd)
        values, log_prob, entropy = pol.evaluate_actions_torch(obs, act, es.double(), states, segs.host)
        values = values.flatten()
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = th.exp(log_prob - old_lp)
        policy_loss = -th.min(adv * ratio, adv * th.clamp(ratio, 0.8, 1.2)).mean()
        value_loss = ((ret - values) ** 2).mean()
        entropy_loss = -entropy.mean()
        loss = policy_loss + 0.0 * entropy_loss + 0.5 * value_loss
        log_ratio = (log_prob - old_lp).detach()
        scalars.append(th.stack([policy_loss, value_loss, entropy_loss, loss, ((th.exp(log_ratio) - 1) - log_ratio).mean(),
                                 ((ratio - 1).abs() > 0.2).double().mean()]).detach())
        opt.zero_grad()
        loss.backward()
        th.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
        opt.step()
    return pol, th.stack(scalars).cpu()


def test_train_kernel_path_against_torch_statements(filled):
    assert filled.fused_learner
    (ker, s_ker), (tor, s_tor) = _train(filled, True), _train(filled, False)
    p64, s64 = _train64(filled)
    assert s_ker.shape == (4, 6) and ker.rollout_buffer.last_split == SPLIT
    figures = [("scalars", s_ker, s_tor, s64)]
    ref = dict(p64.named_parameters())
    for (name, a), (_, b) in zip(ker.policy.named_parameters(), tor.policy.named_parameters()):
        figures.append((name, a.detach().cpu().double(), b.detach().cpu().double(), ref[name].detach().cpu()))
    for name, a, b, r in figures:
        ek, ea = float((a - r).abs().max()), float((b - r).abs().max())
        print(f"{name}: kernel path {ek:.3e} torch path {ea:.3e} ratio {ek / ea if ea else 0.0:.2f}")
        assert ek <= 4.0 * ea, f"{name}: kernel path error {ek:.3e} above 4 x the torch path's {ea:.3e}"


@pytest.mark.parametrize("split", [0, 1, SPLIT, T * N - 1])
def test_segment_tables_against_plain_python(split):
    idx, table, bounds = segment_tables(split, T, N, B)
    order = list(range(split, T * N)) + list(range(split))
    assert idx.tolist() == order
    want, chunk_bounds = [], [0]
    for start in range(0, T * N, B):
        chunk = order[start:start + B]
        for j, row in enumerate(chunk):
            if j == 0 or row // T != chunk[j - 1] // T or row % T == 0:
                want.append([j, 0, (row % T) * N + row // T])
            want[-1][1] += 1
        chunk_bounds.append(len(want))
    assert table.tolist() == want and bounds.tolist() == chunk_bounds


def test_timeout_bootstrap_uses_the_post_step_critic_state(filled):
    rb, pol = filled.rollout_buffer, filled.policy
    seen = 0
    for t, d in enumerate(filled.last_rollout_debug):
        rows = th.nonzero(d["timeouts"] > 0).flatten()
        if len(rows) == 0:
            continue
        seen += len(rows)
        table = np.array([(i, 1, i) for i in range(N)], dtype=np.int32)
        value = {}
        for slot in (t, t + 1):  # the pre-step and the post-step state of the critic
            st = {k: rb.hidden[k][slot] for k in rb.hidden}
            with th.no_grad():
                _, vf, _ = pol.latents_torch(d["terminal_obs"], th.zeros(N, device=DEV), st, table)
                value[slot] = pol.heads_torch(vf, vf)[1].reshape(-1)
        assert th.allclose(d["terminal_values"][rows], value[t + 1][rows], atol=1e-5)
        assert not th.allclose(value[t][rows], value[t + 1][rows], atol=1e-5)
    assert seen > 0


def test_predict_state_save_load_and_learn(filled, tmp_path):
    obs = np.linspace(-0.5, 0.5, 3 * 4, dtype=np.float32).reshape(3, 4)
    a0, s0 = filled.predict(obs, deterministic=True)
    a1, s1 = filled.predict(obs, state=s0, deterministic=True)
    a2, s2 = filled.predict(obs, state=s0, episode_start=np.array([1, 0, 0]), deterministic=True)
    assert a0.shape == (3, 2) and s0[0].shape == (1, 3, H) and s0[1].shape == (1, 3, H)
    assert not np.allclose(a0, a1) and np.array_equal(a2[0], a0[0]) and np.array_equal(a2[1:], a1[1:])  # the state is carried; a start drops it
    filled.save(tmp_path / "rppo")
    again = RecurrentPPO.load(tmp_path / "rppo", env=filled.env, device=DEV)
    assert set(again.policy.state_dict()) == set(filled.policy.state_dict()) and "lstm_critic.weight_hh_l0" in again.policy.state_dict()
    b1, t1 = again.predict(obs, state=s0, deterministic=True)
    assert np.array_equal(b1, a1) and np.array_equal(t1[0], s1[0]) and np.array_equal(t1[1], s1[1])
    model = make()
    model.learn(2 * T * N)
    th.cuda.synchronize()
    assert model.fused_learner and model._n_updates == 2 and model.policy.optimizer.step_count == 8
    assert all(bool(th.isfinite(p).all()) for p in model.policy.parameters()) and bool(th.isfinite(model._sums).all())


def test_refusals_on_a_device_env():
    from core.common.vec_env import VecNormalize

    for face in (dict(discrete_actions=3), dict(multi_discrete_actions=(3, 5))):
        with pytest.raises(ValueError, match="Box valve face"):
            RecurrentPPO("MlpLstmPolicy", CSTRVecEnv(2, device=DEV, **face), device=DEV)
    with pytest.raises(ValueError, match="Dict observation space"):
        RecurrentPPO("MlpLstmPolicy", CSTRVecEnv(2, device=DEV, goal_conditioned=True, goal_range=(0.1, 0.4)), device=DEV)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        RecurrentPPO("MlpLstmPolicy", VecNormalize(CSTRVecEnv(2, device=DEV)), device=DEV)
    with pytest.raises(NotImplementedError, match="hipGraph"):
        make().enable_graph_capture(True)
    for kw in (dict(enable_critic_lstm=False), dict(enable_critic_lstm=False, shared_lstm=True)):  # the torch-statement path
        env = CSTRVecEnv(N, device=DEV)
        m = RecurrentPPO("MlpLstmPolicy", env, n_steps=8, batch_size=B, n_epochs=1, seed=0, device=DEV, policy_kwargs=dict(lstm_hidden_size=H, **kw))
        m.learn(8 * N)
        assert not m.fused_learner and all(bool(th.isfinite(p).all()) for p in m.policy.parameters())
