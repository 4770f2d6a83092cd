#!/usr/bin/env python3
"""Byte-identity probe of every launch that uses the shared actor-head functions (csrc/cstr_gaussian_device.h, the head stages of
csrc/cstr_policy_device.h, the action scaling chain of csrc/cstr_env_device.h). Not a test: it runs each entry point on fixed seeded
inputs, at the smallest shapes that reach every path, and writes every output as OUT/<name>.npy.

    CSTR_LIB_PATH=<library A> python tools/actor_head_ab.py out_a      # a fresh process per library (core/_native.py honours
    CSTR_LIB_PATH=<library B> python tools/actor_head_ab.py out_b      # CSTR_LIB_PATH)
    python tools/actor_head_ab.py --compare out_a out_b                # byte-by-byte, exit status 1 on any difference

CSTR_POLICY_V1=1 in the environment runs the first policy kernel where the pipelined one would run (both sides of an A/B alike).
"""
import argparse
import filecmp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-rl-enhancedstablebaselines_amd"), ROOT):
    if p not in sys.path:
        sys.path.append(p)

import numpy as np  # noqa: E402

DEV = "cuda:0"


def compare(a: str, b: str) -> int:
    names_a, names_b = sorted(os.listdir(a)), sorted(os.listdir(b))
    bad = sorted(set(names_a) ^ set(names_b))
    for n in sorted(set(names_a) & set(names_b)):
        if not filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False):
            bad.append(n)
    print(f"{len(names_a)} files in {a}, {len(names_b)} in {b}: " + ("all identical" if not bad else f"{len(bad)} DIFFER: {bad}"))
    return 1 if bad else 0


class Dump:
    def __init__(self, out):
        self.out, self.n = out, 0
        os.makedirs(out, exist_ok=True)

    def __call__(self, name, **tensors):
        for k, t in tensors.items():
            np.save(os.path.join(self.out, f"{name}.{k}.npy"), t.detach().cpu().numpy())
            self.n += 1


def run(out: str) -> None:
    import torch as th

    from core import _native as nv
    from core.common import hip_ops as ops

    nv.lib()
    dump = Dump(out)
    gen = th.Generator(device=DEV).manual_seed(20261020)
    r = lambda *sh: th.randn(*sh, device=DEV, generator=gen)  # noqa: E731
    new = lambda *sh: th.full(sh, -7.0, device=DEV)  # noqa: E731
    coef = nv.default_coef()

    def mlp(k0, h1, h2, n_out):
        return [r(h1, k0) / k0 ** 0.5, r(h1) * 0.1, r(h2, h1) / h1 ** 0.5, r(h2) * 0.1, r(n_out, h2) / h2 ** 0.5, r(n_out) * 0.1]

    # ---- cstr_policy_rows_fwd_f32: M = 17 (a partial second workgroup), both kernels, both heads, both noise sources ----
    M = 17
    for k0 in (4, 6):
        for h1, h2 in ((20, 36), (256, 256)):
            for A in (1, 2, 4):
                for head in (0, 1):
                    w = mlp(k0, h1, h2, 2 * A if head == 0 else A)
                    x, eps = r(M, k0), r(M, A)
                    for swz in (None, ops.policy_swizzle(w[2])):
                        tag = f"policy.k{k0}.h{h1}x{h2}.a{A}.head{head}.{'v2' if swz is not None else 'v1'}"
                        if head == 1:
                            for out_act in (0, 1, 2):
                                act = new(M, A)
                                ops.policy_rows_fwd(x, *w, 1, 1, out_act, act, w2_swz=swz)
                                dump(f"{tag}.out{out_act}", action=act)
                            continue
                        for with_logp in (False, True):
                            act, lp = new(M, A), new(M) if with_logp else None
                            ops.policy_rows_fwd(x, *w, 1, 0, 0, act, eps=eps, logp=lp, w2_swz=swz)
                            dump(f"{tag}.eps.lp{int(with_logp)}", action=act, **({"logp": lp} if with_logp else {}))
                            ctl, act, lp = ops.new_rng_ctl(77, DEV), new(M, A), new(M) if with_logp else None
                            ops.policy_rows_fwd(x, *w, 2, 0, 0, act, rng_ctl=ctl, logp=lp, w2_swz=swz)
                            dump(f"{tag}.philox.lp{int(with_logp)}", action=act, ctl=ctl, **({"logp": lp} if with_logp else {}))

    # ---- cstr_rollout_step_f32 and cstr_collect_step_f32: 17 envs, both integrators, both heads, with and without action noise ----
    N = 17
    for integ in ("euler", "rk4"):
        for head, (h1, h2) in ((0, (256, 256)), (1, (400, 300)), (0, (20, 36))):
            w = mlp(4, h1, h2, 4 if head == 0 else 2)
            for noisy in (False, True):
                obs = (th.rand(N, 4, device=DEV, generator=gen) * 2 - 1).contiguous()
                steps = th.full((N,), 398, dtype=th.int32, device=DEV)
                steps[::3] = 0
                ring, act = ops.DeviceRing(3, N, 4, 2, DEV), new(N, 2)
                pcg = th.arange(1, 4 * N + 1, dtype=th.int64, device=DEV).view(N, 4).contiguous()
                noise = r(N, 2) * 0.3 if noisy else None
                ctl = ops.new_rng_ctl(5, DEV) if head == 0 else None
                ops.rollout_step(obs, *w, 1, head, 2 if head else 0, ops.policy_swizzle(w[2]), ctl, coef, integ, ring, obs, steps,
                                 1, [-1, -1], [1, 1], noise=noise, pcg_state=pcg, action_out=act)
                dump(f"rollout.{integ}.head{head}.h{h1}.noise{int(noisy)}", obs=obs, steps=steps, action=act, ring_obs=ring.observations,
                     ring_next=ring.next_observations, ring_act=ring.actions, ring_rew=ring.rewards, ring_done=ring.dones, pcg=pcg)
        for squashed in (0, 1):
            obs = (th.rand(N, 4, device=DEV, generator=gen) * 2 - 1).contiguous()
            steps = th.full((N,), 398, dtype=th.int32, device=DEV)
            ring, pol = ops.DeviceRing(3, N, 4, 2, DEV), th.tanh(r(N, 2))
            ops.collect_step(coef, integ, ring, obs, steps, pol, squashed, [-1, -0.5], [1, 2], noise=r(N, 2) * 0.3, reset_obs=obs.clone())
            dump(f"collect.{integ}.sq{squashed}", obs=obs, steps=steps, ring_act=ring.actions, ring_next=ring.next_observations, ring_rew=ring.rewards)

    # ---- cstr_eval_episodes_f32 / cstr_eval_goal_episodes_f32: 17 envs, 2 episodes each, both head forms (and both policy heads) ----
    for goal in (False, True):
        for head, out_act in ((0, 0), (1, 2)):
            for h1, h2 in ((20, 36), (256, 256)):
                w = mlp(6 if goal else 4, h1, h2, 4 if head == 0 else 2)
                for swz in (None, ops.policy_swizzle(w[2])):
                    for squashed in (True, False):
                        obs = (th.rand(N, 4, device=DEV, generator=gen) * 2 - 1).contiguous()
                        steps = th.full((N,), 380, dtype=th.int32, device=DEV)
                        pcg = th.arange(1, 4 * N + 1, dtype=th.int64, device=DEV).view(N, 4).contiguous()
                        tag = f"{'goal_eval' if goal else 'eval'}.head{head}.h{h1}.{'splitk' if swz is not None else 'tree'}.sq{int(squashed)}"
                        if goal:
                            target = th.rand(N, device=DEV, generator=gen) * 0.3 + 0.1
                            res = ops.goal_eval_episodes(*w, 1, head, out_act, swz, coef, "euler", obs, steps, pcg, target, squashed, [-1, -1], [1, 1],
                                                         [2] * N, 1000)
                            dump(tag, target=target)
                        else:
                            res = ops.eval_episodes(*w, 1, head, out_act, swz, coef, "rk4", obs, steps, pcg, squashed, [-1, -1], [1, 1], [2] * N, 1000)
                        dump(tag, ep_return=res[0], ep_len=res[1], ep_done=res[2], obs=obs, steps=steps, pcg=pcg)

    # ---- the three head forwards and the three head backwards, B = 65 ----
    B, K = 65, 40
    for A in (1, 2, 3, 4):
        hid, w3, b3, eps = r(B, K), r(2 * A, K) / K ** 0.5, r(2 * A) * 0.1, r(B, A)
        params = hid @ w3.t()
        params[:, A:] *= 8  # both sides of the log-std clamp
        for draw in (False, True):
            tag = f"head.a{A}.{'philox' if draw else 'eps'}"
            ctl = lambda: ops.new_rng_ctl(9, DEV) if draw else None  # noqa: E731
            if not draw:
                a, lp = new(B, A), new(B)
                ops.squashed_gaussian_fwd(params[:, :A], params[:, A:], eps, a, lp)
                dump(f"{tag}.squashed_fwd", action=a, logp=lp)
            p, e, a, lp = params.clone(), eps.clone(), new(B, A), new(B)
            ops.gaussian_head_fwd_(p, b3, e, ctl(), a, lp)
            dump(f"{tag}.head_fwd", params=p, eps=e, action=a, logp=lp)
            p2, e2, a2, lp2 = new(B, 2 * A), eps.clone(), new(B, A), new(B)
            ops.gaussian_head_gemm_fwd(hid, w3, b3, p2, e2, ctl(), a2, lp2)
            dump(f"{tag}.gemm_fwd", params=p2, eps=e2, action=a2, logp=lp2)
        ga, gl = r(B, A), r(B)
        gp0, gp1, gb, gp2, dz = new(B, 2 * A), new(B, 2 * A), new(2 * A), new(B, 2 * A), new(B, K)
        ops.squashed_gaussian_bwd(ga, gl, a, p[:, A:], e, gp0[:, :A], gp0[:, A:])
        ops.gaussian_head_bwd(ga, gl, a, p, e, gp1, gb)
        ops.gaussian_head_bwd_input(ga, gl, a, p, e, w3, hid, 1, gp2, dz)
        dump(f"head.a{A}.bwd", squashed=gp0, head=gp1, g_bias=gb, input=gp2, dz=dz)

    # ---- cstr_target_smooth_f32 / cstr_linear_smooth_fwd_f32, M = 33 ----
    M = 33
    for A in (1, 2, 3):
        action, noise = th.tanh(r(M, A)), r(M, A) * 0.2
        for draw in (False, True):
            sm = new(M, A)
            ops.target_smooth(action, None if draw else noise, ops.new_rng_ctl(3, DEV) if draw else None, 0.2, 0.5, sm)
            dump(f"target_smooth.a{A}.{int(draw)}", out=sm)
            x, w, b, sm = r(M, 48), r(A, 48) / 7, r(A) * 0.1, new(M, A)
            ops.linear_smooth_fwd(x, w, b, 2, None if draw else noise, ops.new_rng_ctl(3, DEV) if draw else None, 0.2, 0.5, sm)
            dump(f"linear_smooth.a{A}.{int(draw)}", out=sm)

    # ---- the SAC chain's actor forward (noise stage) and backward (head gradient), B = 16 and 32 ----
    D, A, tiles = 4, 2, 2
    for B in (16, 32):
        for h1, h2 in ((256, 256), (20, 36)):
            w = mlp(D, h1, h2, 2 * A)
            actor = ops.sac_actor_desc(D, A, *w)
            G = ops.chain_colgroups(h2, tiles)
            x_pi, x_next = th.zeros(B, D + A, device=DEV), th.zeros(B, D + A, device=DEV)
            x_pi[:, :D], x_next[:, :D] = r(B, D), r(B, D)
            a_h1, a_h2, head_part, eps_all = new(B, h1), new(B, h2), new(G, 2 * B, 2 * A), new(2 * B, A)
            ops.sac_actor_chain_fwd(actor, B, None, x_pi, x_next, None, None, a_h1, a_h2, head_part, tiles, head_rng_ctl=ops.new_rng_ctl(77, DEV),
                                    head_rng_offset=5, eps_all=eps_all, rows_mode=nv.CHAIN_ROWS_PAIR, head_n=2 * A)
            dump(f"chain_fwd.b{B}.h{h1}", a_h1=a_h1, a_h2=a_h2, head_part=head_part, eps_all=eps_all)
            n_nets, n_parts = 2, 3
            x_pi[:, D:] = th.tanh(r(B, A))
            params = r(B, 2 * A)
            params[:, A:] *= 8
            g_params, dz2, dz1 = new(B, 2 * A), new(B, h2), new(B, h1)
            ops.sac_actor_chain_bwd(actor, r(n_nets, n_parts, B, A), n_nets, n_parts, th.full((1,), 0.2, device=DEV), x_pi, params, r(B, A),
                                    th.relu(r(B, h1)), th.relu(r(B, h2)), g_params, dz2, dz1, B, tiles, kind=nv.CHAIN_HEAD_GAUSSIAN)
            dump(f"chain_bwd.b{B}.h{h1}", g_params=g_params, dz2=dz2, dz1=dz1)
    th.cuda.synchronize()
    print(f"{dump.n} arrays written to {out} (library {nv.LIB_PATH})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("give an output directory, or --compare A B")
    run(args.out)
