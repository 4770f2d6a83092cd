"""NumPy restatement of HerReplayBuffer on the goal face of the CSTR env (reference: core/her/her_replay_buffer.py:135-184 `add` and
`_compute_episode_length`, :186-384 `sample`, `_get_real_samples`, `_get_virtual_samples`, `_sample_goals`), on flat rows
[achieved_goal | desired_goal | observation] and an explicit `np.random.RandomState`. tests/test_her_abi.py holds it to the fixture
recorded from the unmodified reference, bit for bit; tests/test_her.py compares the kernels of csrc/cstr_her.hip with it at other shapes.
"""
import numpy as np

S_LO2, S_SPAN2, CONC_SPAN = np.float32(0.0), np.float32(0.7) - np.float32(0.0), np.float32(0.45 - 0.05)
GOAL_TAG = 0x90A17A67


def goal_reward(ag, dg):
    """the goal face's reward statement, float32, in this order"""
    ag, dg = np.asarray(ag, np.float32), np.asarray(dg, np.float32)
    c2 = S_LO2 + (ag + np.float32(1)) * S_SPAN2 / np.float32(2)
    t = S_LO2 + (dg + np.float32(1)) * S_SPAN2 / np.float32(2)
    ne = np.abs(c2 - t) / CONC_SPAN
    return (np.float32(-5) * (ne * ne) - np.float32(2) * ne).astype(np.float32)


def goal_of_target(target):
    return np.float32(2) * (np.asarray(target, np.float32) - S_LO2) / S_SPAN2 - np.float32(1)


class HerNp:
    def __init__(self, rows, n_envs, n_sampled_goal=4, strategy="future"):
        self.rows, self.n_envs, self.strategy = rows, n_envs, strategy
        self.her_ratio = 1 - (1.0 / (n_sampled_goal + 1))
        z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
        self.observation, self.next_observation, self.desired_goal = z(rows, n_envs, 4), z(rows, n_envs, 4), z(rows, n_envs)
        self.actions, self.rewards, self.dones, self.timeouts = z(rows, n_envs, 2), z(rows, n_envs), z(rows, n_envs), z(rows, n_envs)
        self.ep_start, self.ep_length = np.zeros((rows, n_envs), np.int64), np.zeros((rows, n_envs), np.int64)
        self.cur = np.zeros(n_envs, np.int64)
        self.pos, self.full, self.adds = 0, False, 0

    def _compute_episode_length(self, env_idx):  # :169-184
        episode_start, episode_end = self.cur[env_idx], self.pos
        if episode_end < episode_start:
            episode_end += self.rows
        episode_indices = np.arange(episode_start, episode_end) % self.rows
        self.ep_length[episode_indices, env_idx] = episode_end - episode_start
        self.cur[env_idx] = self.pos

    def add(self, obs_rows, next_rows, act, rew, done, timeout):  # :135-167
        for env_idx in range(self.n_envs):
            episode_start, episode_length = self.ep_start[self.pos, env_idx], self.ep_length[self.pos, env_idx]
            if episode_length > 0:
                episode_end = episode_start + episode_length
                episode_indices = np.arange(self.pos, episode_end) % self.rows
                self.ep_length[episode_indices, env_idx] = 0
        self.ep_start[self.pos] = self.cur.copy()
        p = self.pos
        self.observation[p], self.next_observation[p], self.desired_goal[p] = obs_rows[:, 2:6], next_rows[:, 2:6], obs_rows[:, 1]
        self.actions[p], self.rewards[p], self.dones[p], self.timeouts[p] = act, rew, done, timeout
        self.pos += 1  # DictReplayBuffer.add's epilogue
        self.adds += 1
        if self.pos == self.rows:
            self.full, self.pos = True, 0
        for env_idx in range(self.n_envs):
            if done[env_idx]:
                self._compute_episode_length(env_idx)

    def sample(self, rs, batch_size, forced=None):
        """-> dict: row / env / goal_row int64 [B] and the five outputs, all in OUTPUT order (real transitions first); goal_idx = the
        drawn indices in the episode (draw order). forced = (rows, envs) or (rows, envs, goal_rows) in draw order."""
        is_valid = self.ep_length > 0
        nb_virtual = int(self.her_ratio * batch_size)  # :218
        if forced is None:
            if not np.any(is_valid):
                raise RuntimeError("Unable to sample before the end of the first episode.")
            valid_indices = np.flatnonzero(is_valid)
            sampled_indices = rs.choice(valid_indices, size=batch_size, replace=True)  # :212
            batch_indices, env_indices = np.unravel_index(sampled_indices, is_valid.shape)
        else:
            batch_indices, env_indices = np.asarray(forced[0], np.int64), np.asarray(forced[1], np.int64)
        vb, rb = np.split(batch_indices, [nb_virtual])
        ve, re = np.split(env_indices, [nb_virtual])
        goal_idx = np.zeros(0, np.int64)
        if forced is not None and len(forced) > 2:
            goal_rows = np.asarray(forced[2], np.int64)[:nb_virtual]
        else:  # _sample_goals (:355-384)
            start, length = self.ep_start[vb, ve], self.ep_length[vb, ve]
            if self.strategy == "final":
                goal_idx = length - 1
            elif self.strategy == "future":
                current = (vb - start) % self.rows
                goal_idx = rs.randint(current, length) if nb_virtual else np.zeros(0, np.int64)
            elif self.strategy == "episode":
                goal_idx = rs.randint(0, length) if nb_virtual else np.zeros(0, np.int64)
            else:
                raise ValueError(self.strategy)
            goal_rows = (goal_idx + start) % self.rows
        new_goals = self.next_observation[goal_rows, ve][:, 2]
        rows, envs = np.concatenate([rb, vb]), np.concatenate([re, ve])
        dg = np.concatenate([self.desired_goal[rb, re], new_goals]).astype(np.float32)
        o, n = self.observation[rows, envs], self.next_observation[rows, envs]
        rew = np.concatenate([self.rewards[rb, re], goal_reward(self.next_observation[vb, ve][:, 2], new_goals)]).astype(np.float32)
        return dict(row=rows, env=envs, goal_row=np.concatenate([np.full(len(rb), -1, np.int64), goal_rows]), goal_idx=np.asarray(goal_idx, np.int64),
                    obs=np.concatenate([o[:, 2:3], dg[:, None], o], axis=1), next=np.concatenate([n[:, 2:3], dg[:, None], n], axis=1),
                    act=self.actions[rows, envs], done=(self.dones[rows, envs] * (1 - self.timeouts[rows, envs]))[:, None], rew=rew[:, None],
                    flat_idx=None if forced is not None else sampled_indices)


def mt_image(rs):
    """uint32 [628] device image of a RandomState: key, pos, has_gauss, gauss (f64, low word first)"""
    st = rs.get_state()
    g = np.array([st[4]], np.float64).view(np.uint32)
    return np.concatenate([st[1].astype(np.uint32), np.array([st[2], st[3]], np.uint32), g])


def scripted_adds(rng, n_envs, steps, lengths):
    """`steps` add inputs for envs whose episodes last lengths[i] steps: flat rows with a fixed goal per env, done = timeout at episode ends"""
    t_in = np.zeros(n_envs, np.int64)
    goal = rng.uniform(-1, 1, n_envs).astype(np.float32)
    obs = rng.uniform(-1, 1, (n_envs, 4)).astype(np.float32)
    for _ in range(steps):
        nxt = rng.uniform(-1, 1, (n_envs, 4)).astype(np.float32)
        t_in += 1
        done = (t_in >= np.asarray(lengths)).astype(np.float32)
        row = lambda x: np.concatenate([x[:, 2:3], goal[:, None], x], axis=1).astype(np.float32)  # noqa: E731
        act, rew = rng.uniform(-1, 1, (n_envs, 2)).astype(np.float32), rng.uniform(-3, 0, n_envs).astype(np.float32)
        timeout = done * (rng.uniform(size=n_envs) < 0.7)
        yield row(obs), row(nxt), act, rew, done, timeout.astype(np.float32)
        obs = np.where(done[:, None] > 0, rng.uniform(-1, 1, (n_envs, 4)).astype(np.float32), nxt)
        t_in[done > 0] = 0
