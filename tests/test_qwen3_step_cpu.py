"""The Qwen3 training step without a GPU: the new ABI entry's scratch rule and its refusals before any launch, and Qwen3Step's argument check."""
import ctypes as C

import pytest

from koifish_amd import lib as L


def test_scratch_bytes_positive_for_served_shapes_zero_for_refused():
    hip, _ = L.load()
    f = hip.kf_qknorm_rope_backward_scratch_bytes
    for n_tok, n_head, n_kv, hd in ((1, 1, 1, 64), (128, 4, 2, 64), (51, 2, 2, 128), (8192, 16, 8, 128), (8192, 32, 8, 128)):
        assert f(n_tok, n_head, n_kv, hd) > 0, (n_tok, n_head, n_kv, hd)
    assert f(128, 4, 2, 64) % 8 == 0
    assert f(8192, 16, 8, 128) >= f(128, 16, 8, 128)
    for n_tok, n_head, n_kv, hd in ((0, 4, 2, 64), (-3, 4, 2, 64), (128, 4, 3, 64), (128, 0, 0, 64), (128, 4, 0, 64), (128, 4, 2, 96), (128, 4, 2, 256), (128, 4, 2, 32)):
        assert f(n_tok, n_head, n_kv, hd) == 0, (n_tok, n_head, n_kv, hd)


def test_entry_refuses_null_context_and_null_pointers_before_any_launch():
    hip, _ = L.load()
    args = [None] * 3 + [256] + [None, 256, None, 128] + [None] * 5 + [128, 64, 4, 2, 64] + [None] * 6
    assert hip.kf_qknorm_rope_backward(None, *args) == -20
    assert b"null kf_ctx" in hip.kf_last_error()
    # a context that is never dereferenced: the pointer checks come before anything touches it
    fake = C.create_string_buffer(4096)
    assert hip.kf_qknorm_rope_backward(C.cast(fake, C.c_void_p), *args) == -20
    assert b"null pointer" in hip.kf_last_error()
    assert hip.kf_d2d_rows(None, None, 0, None, 0, 0, 0) == -20


def test_qwen3_step_rejects_an_unknown_train_target():
    from koifish_amd.train_step import Qwen3Step
    cfg = dict(dim=128, n_layer=2, n_head=4, n_kv=2, head_dim=64, ffn=256, vocab=250, theta=10000.0, rms_eps=1e-6)
    with pytest.raises(ValueError, match="train_target"):
        Qwen3Step(None, cfg, 2, 64, train_target="zero_step")
