"""The two training-step sequencers of libkf_host.so (kfh_gpt2_*, kfh_qwen3t_*) without a GPU: what a trainer with nothing registered answers, and the argument
refusals of the entries both families have -- one body for both, because the code behind them is one (koifish::TrainerCore, host/kf_train_common.hpp).  The context is
a zeroed buffer that no call here dereferences: every entry used returns before it would."""
import ctypes as C

import pytest

from koifish_amd import lib as L

INVALID_ARGS = -20
HYPER = (3e-4, 0.9, 0.95, 1e-8, 0.1, 1234)   # lr, beta1, beta2, eps, wd, seed


def _fake_ctx():
    buf = C.create_string_buffer(4096)
    return buf, C.cast(buf, C.c_void_p)


TRAINERS = {
    "gpt2": ("gpt2", lambda host, ctx: host.kfh_gpt2_create(ctx, 128, 2, 2, 250, 256, 2, 64), 12 * 2 + 4),
    "qwen3t-tied": ("qwen3t", lambda host, ctx: host.kfh_qwen3t_create(ctx, 128, 2, 4, 2, 64, 256, 250, 256, 2, 64, 1e-6, 1), 11 * 2 + 2),
    "qwen3t-untied": ("qwen3t", lambda host, ctx: host.kfh_qwen3t_create(ctx, 128, 2, 4, 2, 64, 256, 250, 256, 2, 64, 1e-6, 0), 11 * 2 + 3),
}


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_unregistered_trainer_refuses_the_step_and_checks_its_arguments(which):
    _, host = L.load()
    family, create, n_params = TRAINERS[which]
    f = lambda name: getattr(host, "kfh_%s_%s" % (family, name))
    keep, ctx = _fake_ctx()
    h = create(host, ctx)
    assert h
    try:
        assert f("n_params")(h) == n_params
        # nothing registered: every part of the step is refused, and a refused update does not count as a step
        assert f("forward")(h, None, None) == INVALID_ARGS
        assert f("backward")(h) == INVALID_ARGS
        assert f("update")(h, *HYPER) == INVALID_ARGS
        assert f("step")(h, None, None, *HYPER) == INVALID_ARGS
        assert f("steps_taken")(h) == 0
        # set_param: the index, and a length that is no multiple of 8
        mem = C.create_string_buffer(256)
        p = C.cast(mem, C.c_void_p)
        assert f("set_param")(h, 10 ** 6, p, p, p, p, 16, 0, None, 0) == INVALID_ARGS
        assert f("set_param")(h, 0, p, p, p, p, 12, 0, None, 0) == INVALID_ARGS
        assert f("set_param")(h, 0, p, p, p, p, 16, 0, None, 0) == 0
        # set_optimizer: an unknown method; Muon without a scratch; Muon with one while no tensor is a Muon tensor (no blob registered)
        assert f("set_optimizer")(h, 2, 50.0, 0.95, 1e-7, 1, p, 256) == INVALID_ARGS
        assert f("set_optimizer")(h, 1, 50.0, 0.95, 1e-7, 1, None, 0) == INVALID_ARGS
        assert f("set_optimizer")(h, 1, 50.0, 0.95, 1e-7, 1, p, 256) == 0
        assert f("steps_taken")(h) == 0
    finally:
        f("destroy")(h)
    del keep


def test_create_refuses_a_shape_it_cannot_serve():
    _, host = L.load()
    keep, ctx = _fake_ctx()
    assert not host.kfh_qwen3t_create(ctx, 128, 2, 4, 3, 64, 256, 250, 256, 2, 64, 1e-6, 1)   # 4 heads over 3 kv heads
    assert host.kfh_qwen3t_last_error().decode().startswith("kfh_qwen3t_create:")
    assert not host.kfh_gpt2_create(ctx, 130, 4, 2, 250, 256, 2, 64)   # C no multiple of H
    del keep
