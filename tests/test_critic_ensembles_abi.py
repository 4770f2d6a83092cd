"""CPU-side checks of the critic-ensemble loss heads' C ABI (cstr_td_ens_q_loss_f32, cstr_sac_actor_ens_loss_f32): exported,
declared, and every bad argument is rejected on the host before anything is dereferenced or launched."""
import ctypes as C

from core import _native as nv


def _td(lib, q_t, q, gq, n, batch, stride=256, next_logp=None, ent_coef=None, alpha=None, rew=0x1000, done=0x1000):
    p = C.c_void_p
    return lib.cstr_td_ens_q_loss_f32(p(q_t), C.c_int64(stride), p(next_logp), p(rew), p(done), p(ent_coef), C.c_float(0.99), p(q),
                                      C.c_int64(stride), C.c_float(1.0), p(None), p(gq), p(None), p(None),
                                      None if alpha is None else C.byref(alpha), C.c_int(n), C.c_int64(batch), p(None))


def _actor(lib, logp, q, ent_coef, g_logp, gq, n, batch, stride=256):
    p = C.c_void_p
    return lib.cstr_sac_actor_ens_loss_f32(p(logp), p(q), C.c_int64(stride), p(ent_coef), p(g_logp), p(gq), p(None), p(None), C.c_int(n),
                                           C.c_int64(batch), p(None))


def test_ensemble_loss_heads_are_exported():
    lib = nv.lib()
    for name in ("cstr_td_ens_q_loss_f32", "cstr_sac_actor_ens_loss_f32"):
        assert hasattr(lib, name) and name in nv.SYMBOLS
    assert nv.MAX_ENS_CRITICS == 16


def test_ensemble_loss_heads_reject_bad_arguments_on_the_host():
    lib = nv.lib()
    f = 0x1000  # never dereferenced: the argument checks fail first
    # critic count: 0 and negative are bad arguments, above CSTR_MAX_ENS_CRITICS unsupported
    assert _td(lib, f, f, f, 0, 256) == -1 and _td(lib, f, f, f, -3, 256) == -1
    assert _td(lib, f, f, f, 17, 256) == -2
    assert _actor(lib, f, f, f, f, f, 0, 256) == -1 and _actor(lib, f, f, f, f, f, 17, 256) == -2
    # batch: 0 bad, above the single-workgroup limit unsupported
    assert _td(lib, f, f, f, 3, 0) == -1 and _actor(lib, f, f, f, f, f, 3, 0) == -1
    assert _td(lib, f, f, f, 3, 16385, stride=16385) == -2 and _actor(lib, f, f, f, f, f, 3, 16385, stride=16385) == -2
    # NULL operands
    assert _td(lib, None, f, f, 3, 256) == -1 and _td(lib, f, None, f, 3, 256) == -1 and _td(lib, f, f, None, 3, 256) == -1
    assert _td(lib, f, f, f, 3, 256, rew=None) == -1 and _td(lib, f, f, f, 3, 256, done=None) == -1
    for i in range(5):
        args = [f] * 5
        args[i] = None
        assert _actor(lib, *args, 3, 256) == -1
    # overlapping rows (stride below the batch) with more than one critic; a single critic has no stride
    assert _td(lib, f, f, f, 3, 256, stride=255) == -1 and _actor(lib, f, f, f, f, f, 3, 256, stride=255) == -1
    # an entropy term without its coefficient; an alpha part with missing pointers
    assert _td(lib, f, f, f, 3, 256, next_logp=f) == -1
    part = nv.AlphaPart(0x1000, None, -2.0, 0x1000, 0x1000, None, None, None)
    assert _td(lib, f, f, f, 3, 256, alpha=part) == -1
