#!/usr/bin/env python3
"""The learning run of tests/test_rmsprop_tf.py::test_it_learns_with_the_tf_like_optimiser on the UNMODIFIED reference, CPU, one seed:
A2C on 32 envs, 300 iterations of 16 steps, lr 1e-3, gae_lambda 0.95, log_std_init -1 (the settings of tests/test_a2c.py::test_it_learns)
with optimizer_class=RMSpropTFLike, optimizer_kwargs eps=1e-5. Prints evaluate_policy (8 envs seeded 1000, 8 episodes, deterministic)
before and after. Dev container only (tools/refharness/refload.py).

    python tools/refharness/a2c_tflike_learning.py SEED"""
import os
import sys

import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refload  # noqa: E402

refload.load()
th.set_num_threads(1)


def main(seed: int) -> None:
    from core.a2c.a2c import A2C
    from core.common.evaluation import evaluate_policy
    from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike
    from core.common.vec_env.dummy_vec_env import DummyVecEnv
    from twoseriescstr import TwoSeriesCSTREnv

    def venv(n):
        return DummyVecEnv([lambda: TwoSeriesCSTREnv() for _ in range(n)])

    def score(model):
        env = venv(8)
        env.seed(1000)
        return evaluate_policy(model, env, n_eval_episodes=8, deterministic=True)[0]

    model = A2C("MlpPolicy", venv(32), learning_rate=1e-3, n_steps=16, gae_lambda=0.95, seed=seed, device="cpu",
                policy_kwargs=dict(log_std_init=-1.0, optimizer_class=RMSpropTFLike, optimizer_kwargs=dict(eps=1e-5)))
    before = score(model)
    model.learn(32 * 16 * 300)
    print(f"reference A2C + RMSpropTFLike seed {seed}: evaluate_policy before {before:.1f}, after {score(model):.1f}", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]))
