"""Adapters at inference without a GPU: the numpy restatement of kf_lora_apply's vector form (tests/lora_apply_restate.py) is exact on the integer operands of
tests/lora_restate.py::lora_exact_case and within a rounding of fp64 on random ones; kf_lora_apply_status is a pure host function with the served / refused table of
include/kf_abi.h; the symbols are exported and mirrored; Qwen3.set_adapters' argument errors are raised by a classmethod before anything touches a device."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from koifish_amd.runtime import Qwen3
from oracle import oracle as O
from tests import exact_inputs as E
from tests import lora_apply_restate as A
from tests import lora_restate as R

CFG = dict(dim=128, n_layer=2, n_head=4, n_kv=2, head_dim=64, ffn=256, vocab=250)


@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("OC,IC", [(128, 128), (192, 576)])
def test_vector_restatement_is_exact_on_integer_operands(r, OC, IC):
    """every partial sum of lora_exact_case is an fp32 value in every order: the stated order must give the exact ax and y of every row"""
    c = R.lora_exact_case(OC, IC, 64, r, 2 if r == 64 else 1, seed=OC + IC + r)
    for row in (0, 17, 63):
        assert np.array_equal(A.vec_ax_bits(c["a"], c["x"][row], c["s"]), c["ax"][row]), (r, OC, IC, row)
        assert np.array_equal(A.vec_apply_bits(c["a"], c["b"], c["x"][row], c["y0"][row], c["s"]), c["y"][row]), (r, OC, IC, row)


@pytest.mark.parametrize("r", R.RANKS)
@pytest.mark.parametrize("IC", [128, 576])
def test_exact_groups_of_the_gpu_test_hold_their_preconditions(r, IC):
    """the three-adapter integer groups tests/test_gpu_lora_apply.py launches: representable results (asserted inside), reproduced by the restatement"""
    for OCs in ((128,), (192,), (256, 128, 128)):
        x, group = A.exact_group(r, IC, OCs, seed=r + IC)
        for a, b, y0, y in group:
            assert np.array_equal(A.vec_apply_bits(a, b, x, y0, 1.0), y)


def test_vector_restatement_follows_fp64_on_random_operands():
    """random operands: inside the bound tests/lora_restate.py derives for an fp32 device against its fp64 restatement"""
    r, OC, IC, s = 32, 192, 576, 0.5
    rng = np.random.default_rng(5)
    bf = lambda v: O.f32_to_bf16(v.astype(np.float32))
    a, b, x, y0 = bf(rng.normal(0, 0.1, (r, IC))), bf(rng.normal(0, 0.1, (OC, r))), bf(rng.normal(0, 1.0, (1, IC))), bf(rng.normal(0, 1.0, (1, OC)))
    f = [E.f64(v) for v in (a, b, x, y0)]
    ax_r, _ = R.lora_forward(*f, s)
    _, y = R.lora_forward(*f, s, store=False)
    Amag = np.abs(f[3]) + s * (np.abs(ax_r) @ np.abs(f[1]).T)
    got = E.f64(A.vec_apply_bits(a, b, x[0], y0[0], s))
    assert (np.abs(got - y[0]) <= R.bound(y, Amag, r, f[3], True)[0]).all()


def test_symbols_exported_and_mirrored():
    hip, host = L.load()
    for f in ("kf_lora_apply", "kf_lora_apply_status"):
        assert f in L.ABI_SYMBOLS and hasattr(hip, f), f
    assert len(hip.kf_lora_apply.argtypes) == 12 and len(hip.kf_lora_apply_status.argtypes) == 5
    for f in ("kfh_set_adapter", "kfh_clear_adapters", "kfh_n_adapters"):
        assert hasattr(host, f), f
    assert hip.kf_lora_apply(None, 1, None, None, 16, None, 128, None, None, None, 1, 1.0) == -20   # no context: refused, nothing dereferenced


def test_apply_status_table():
    st = L.load()[0].kf_lora_apply_status
    for r in R.RANKS:
        for n in (1, 2, 31, 70):
            assert st(r, 128, 128, n, 1) == 0 and st(r, 192, 576, n, 1) == 0, (r, n)
        assert st(r, 256, 128, 1, 3) == 0 and st(r, 3072, 1024, 1, 2) == 0
    INV = -20   # KF_INVALID_ARGS
    for args in ((8, 128, 128, 1, 1), (16, 96, 128, 1, 1), (16, 128, 160, 1, 1), (16, 128, 128, 0, 1), (16, 128, 128, 2, 2), (16, 128, 128, 1, 4),
                 (24, 128, 128, 2, 1), (128, 256, 256, 2, 1), (16, 64, 128, 2, 1), (16, 128, 64, 1, 1), (16, 128, 128, -1, 1), (16, 128, 128, 1, 0), (16, 128, 128, 70, 3)):
        assert st(*args) == INV, args


def _pair(r=16, OC=128, IC=128, dtype=torch.bfloat16):
    return torch.zeros(r, IC, dtype=dtype), torch.zeros(OC, r, dtype=dtype)


def test_set_adapters_argument_errors_need_no_device():
    chk = Qwen3.check_adapters
    items, rank = chk(CFG, {"l0.q.w": _pair(16, 256, 128), "l1.down.w": _pair(16, 128, 256)}, 0.5)
    assert rank == 16 and [(l, s) for l, s, _, _ in items] == [(0, 0), (1, 6)]
    for bad in ({"l0.qq.w": _pair()}, {"l2.q.w": _pair(16, 256, 128)}, {"q": _pair()}, {"l0.q": _pair(16, 256, 128)}, {}):   # unknown names
        with pytest.raises(ValueError):
            chk(CFG, bad, 0.5)
    with pytest.raises(ValueError, match="a \\[r, 128\\]"):   # wrong shape: k is [128, 128] on this card
        chk(CFG, {"l0.k.w": _pair(16, 256, 128)}, 0.5)
    with pytest.raises(ValueError, match="r 16, 32 or 64"):
        chk(CFG, {"l0.k.w": _pair(8, 128, 128)}, 0.5)
    with pytest.raises(ValueError, match="bf16"):
        chk(CFG, {"l0.k.w": _pair(dtype=torch.float32)}, 0.5)
    with pytest.raises(ValueError, match="one rank"):
        chk(CFG, {"l0.k.w": _pair(16), "l0.v.w": _pair(32)}, 0.5)
    for s in (float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="lora_s"):
            chk(CFG, {"l0.k.w": _pair()}, s)
