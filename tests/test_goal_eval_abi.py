"""CPU-side checks of cstr_eval_goal_episodes_f32 (whole evaluation episodes on the goal face in one launch): the symbol, every
CSTR_E_BADARG / CSTR_E_UNSUPPORTED case of the header on pointers that are never dereferenced (the pattern of
tests/test_callbacks_host.py for the Box entry), the wrapper's shape predicate, and the Python names the feature adds."""
import ctypes as C

from core import _native as nv

BAD, UNS = -1, -2


def test_goal_eval_symbol_is_exported():
    lib = nv.lib()
    assert "cstr_eval_goal_episodes_f32" in nv.SYMBOLS and hasattr(lib, "cstr_eval_goal_episodes_f32")


def test_goal_eval_entry_point_rejects_bad_arguments_on_the_host():
    lib = nv.lib()
    coef = nv.default_coef()
    null = C.c_void_p(None)
    A = lambda i: C.c_void_p(0x100000 * (i + 1))  # noqa: E731  distinct, 16-byte aligned, 1 MiB apart: nothing overlaps
    off = lambda p, d: C.c_void_p(p.value + d)  # noqa: E731
    lo, hi = (C.c_float * 2)(-1, -1), (C.c_float * 2)(1, 1)
    good_net = dict(k0=6, h1=64, h2=64, act_dim=2, act=1, head=0, out_act=0, reserved=0, w1=A(0).value, b1=A(1).value, w2=A(2).value, b2=A(3).value,
                    w3=A(4).value, b3=A(5).value, w2_swizzled=A(6).value)

    def call(net=None, coef_=C.byref(coef), integrator=0, env_obs=A(7), steps=A(8), pcg=A(9), static=null, target=A(13), episode=A(14), seed=(1 << 40) + 3,
             index_offset=5, g_lo=0.1, g_hi=0.4, squashed=1, lo_=lo, hi_=hi, targets=(1, 0, 2), n=3, max_steps=10, ret=A(10), ln=A(11), dn=A(12),
             goal=A(15), gap=A(16), abs_gap=A(17)):
        f = dict(good_net, **(net or {}))
        pm = nv.PolicyMlp(*[f[k] for k in ("k0", "h1", "h2", "act_dim", "act", "head", "out_act", "reserved", "w1", "b1", "w2", "b2", "w3", "b3",
                                           "w2_swizzled")])
        tg = null if targets is None else (C.c_int32 * len(targets))(*targets)
        return lib.cstr_eval_goal_episodes_f32(C.byref(pm), coef_, integrator, env_obs, steps, pcg, static, target, episode, C.c_uint64(seed),
                                               C.c_int64(index_offset), C.c_float(g_lo), C.c_float(g_hi), squashed, lo_, hi_, tg, C.c_int64(n),
                                               C.c_int64(max_steps), ret, ln, dn, goal, gap, abs_gap, null)

    # NULL required pointers (episode, static_init and the three tracking outputs are optional: not among them)
    assert lib.cstr_eval_goal_episodes_f32(null, C.byref(coef), 0, A(7), A(8), A(9), null, A(13), null, C.c_uint64(0), C.c_int64(0), C.c_float(0),
                                           C.c_float(0), 1, lo, hi, (C.c_int32 * 1)(1), C.c_int64(1), C.c_int64(5), A(10), A(11), A(12), null, null,
                                           null, null) == BAD
    for kw in (dict(coef_=null), dict(env_obs=null), dict(steps=null), dict(pcg=null), dict(target=null), dict(lo_=null), dict(hi_=null),
               dict(targets=None), dict(ret=null), dict(ln=null), dict(dn=null), dict(net=dict(w1=None)), dict(net=dict(b2=None)),
               dict(net=dict(w3=None))):
        assert call(**kw) == BAD, kw
    # sizes, targets, the row width, the goal interval
    assert call(n=0) == BAD and call(n=-3) == BAD
    assert call(targets=(1, -1, 2)) == BAD
    assert call(max_steps=0) == BAD and call(max_steps=-1) == BAD
    assert call(squashed=2) == BAD and call(net=dict(reserved=1)) == BAD
    assert call(net=dict(k0=4)) == BAD and call(net=dict(k0=8)) == BAD      # the policy reads the goal face's six-float rows
    assert call(g_lo=0.4, g_hi=0.1) == BAD and call(g_lo=float("nan")) == BAD
    assert call(hi_=(C.c_float * 2)(1, -1)) == BAD                          # empty action interval
    # misaligned rows
    for kw in (dict(env_obs=off(A(7), 4)), dict(pcg=off(A(9), 8)), dict(ret=off(A(10), 4)), dict(ln=off(A(11), 2)), dict(dn=off(A(12), 2)),
               dict(steps=off(A(8), 2)), dict(target=off(A(13), 2)), dict(episode=off(A(14), 2)), dict(goal=off(A(15), 2)), dict(gap=off(A(16), 1)),
               dict(abs_gap=off(A(17), 4)), dict(net=dict(w1=A(0).value + 2)), dict(net=dict(w2=A(2).value + 4)),
               dict(net=dict(w2_swizzled=A(6).value + 8))):
        assert call(**kw) == BAD, kw
    # outputs overlapping inputs, or each other
    assert call(ret=A(7)) == BAD and call(ln=A(9)) == BAD and call(dn=A(8)) == BAD and call(ret=A(2)) == BAD
    assert call(goal=A(13)) == BAD and call(gap=A(14)) == BAD and call(abs_gap=A(0)) == BAD and call(goal=A(9)) == BAD
    assert call(ln=off(A(10), 16)) == BAD and call(dn=off(A(7), 32)) == BAD
    assert call(gap=off(A(15), 4)) == BAD and call(abs_gap=off(A(10), 8)) == BAD and call(goal=off(A(11), 4)) == BAD
    # unsupported action widths, integrators and network shapes
    assert call(net=dict(act_dim=4)) == UNS and call(net=dict(act_dim=3)) == UNS and call(net=dict(act_dim=1)) == UNS
    assert call(integrator=7) == UNS
    assert call(net=dict(h1=66)) == UNS and call(net=dict(act=3)) == UNS and call(net=dict(head=2)) == UNS and call(net=dict(out_act=5)) == UNS
    assert call(net=dict(h1=1024, h2=512)) == UNS                           # more than 64 KB of LDS


def test_goal_eval_episodes_supported_shapes():
    from core.common import hip_ops as ops

    for h1, h2 in ((16, 16), (36, 20), (256, 256), (400, 300), (528, 32)):
        assert ops.goal_eval_episodes_supported(h1, h2, 4, 0) and ops.goal_eval_episodes_supported(h1, h2, 2, 1)
    assert not ops.goal_eval_episodes_supported(64, 64, 2, 0) and not ops.goal_eval_episodes_supported(64, 64, 4, 1)  # two valves
    assert not ops.goal_eval_episodes_supported(64, 64, 8, 0) and not ops.goal_eval_episodes_supported(64, 64, 2, 2)
    assert not ops.goal_eval_episodes_supported(66, 64, 4, 0) and not ops.goal_eval_episodes_supported(64, 30, 2, 1)  # widths % 4
    assert not ops.goal_eval_episodes_supported(1024, 512, 4, 0)                                                       # LDS


def test_goal_tracking_names_are_importable():
    import inspect

    from core.common import evaluation

    assert callable(evaluation.evaluate_goal_tracking) and callable(evaluation.supported)
    assert list(inspect.signature(evaluation.evaluate_goal_tracking).parameters) == ["model", "env", "n_eval_episodes", "warn"]
    # `evaluate_policy_fused` keeps its signature
    assert list(inspect.signature(evaluation.evaluate_policy_fused).parameters) == [
        "model", "env", "n_eval_episodes", "deterministic", "reward_threshold", "return_episode_rewards", "warn"]
