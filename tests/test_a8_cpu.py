"""The int8-activation arithmetic (include/kf_abi.h "int8 activations") without a GPU: the properties its exactness claims rest on, checked on the numpy restatement
that tests/test_gpu_a8.py holds the kernels to (tests/a8_restate.py, stated once).  They test the definition, not the kernels; what the library can answer without a GPU --
its entries and the served-storage rule kf_linear_a8_status -- is checked here too."""
import ctypes as C

import numpy as np
import pytest

from a8_restate import bf as bf16_to_f32
from a8_restate import quant_rows_f32 as quant_rows
from a8_restate import to_bf as f32_to_bf16
from koifish_amd import lib as L


@pytest.fixture(autouse=True, scope="module")
def the_library_has_the_feature():
    """these tests check the DEFINITION (tests/a8_restate.py, the expectation of every GPU test of the feature), not the kernels; they stand only beside a library that
    has the entries the definition belongs to"""
    hip, host = L.load()
    for f in ("kf_act_quant_i8", "kf_linear_a8", "kf_linear_a8_status", "kfdbg_a8_plan"):
        assert hasattr(hip, f), f
    assert hasattr(host, "kfh_set_act_int8")


def test_served_storage_rule():
    """kf_linear_a8_status, the rule the host routes layer matrices by: no launch, so it answers without a GPU"""
    hip, _ = L.load()
    buf = (C.c_uint8 * 64)()
    data = (C.addressof(buf) + 15) & ~15

    def st(type_, ne1=256, lGroup=128, gama=True, quant=0, off=0, qz=None):
        w = L.Weight(data + off, data if gama else None, type_, 16, ne1, 16 * ne1 // max(lGroup, 1), lGroup, 0, 1, 0, qz, None, quant, 0)
        return hip.kf_linear_a8_status(C.byref(w), 1)
    assert [st(t) for t in (L.T_SIGN, L.BOOL1, L.T_BINARY)] == [0, 0, 0]
    assert [st(t, gama=(t == L.Q4)) for t in (L.Q4, L.BF16, L.F8E5M2)] == [-1000] * 3
    assert st(L.T_SIGN, quant=L.QUANT_ROW_LUT) == -1000 and st(L.T_SIGN, qz=data) == -1000
    assert st(L.T_SIGN, lGroup=64) == -701 and st(L.BOOL1, gama=False) == -701
    assert st(L.T_SIGN, ne1=192) == -20 and st(L.T_SIGN, off=8) == -2000
    assert hip.kf_linear_a8_status(None, 1) == -20


def test_group_products_are_exact_in_fp32():
    """fp32(step) * fp32(I): a bf16 step (8 significant bits) times |I| <= 16 256 (14 bits) has at most 22 -- no rounding"""
    rng = np.random.default_rng(1)
    step = bf16_to_f32(f32_to_bf16(np.exp(rng.normal(-4.0, 3.0, 200000)).astype(np.float32)))
    I = rng.integers(-16256, 16257, size=step.size)
    I[:4] = (16256, -16256, 16255, 1)
    p32 = step * I.astype(np.float32)
    assert p32.dtype == np.float32
    assert np.array_equal(p32.astype(np.float64), step.astype(np.float64) * I.astype(np.float64))


def test_requantising_is_idempotent():
    """step * q of a row whose largest |q| is 127 quantises back to the same q and the same step"""
    rng = np.random.default_rng(2)
    x = bf16_to_f32(f32_to_bf16(rng.normal(0, 1, (64, 384)).astype(np.float32)))
    q, step = quant_rows(x)
    assert (np.abs(q).max(axis=1) == 127).all()
    back = (step[:, None] * q.astype(np.float32)).astype(np.float32)
    q2, step2 = quant_rows(back)
    assert np.array_equal(q2, q) and np.array_equal(step2.view(np.uint32), step.view(np.uint32))


def test_halves_round_away_from_zero():
    x = np.zeros(128, dtype=np.float32)
    x[:8] = (127.0, 0.5, -0.5, 2.5, -2.5, 126.5, 1.5, -126.5)   # amax = 127: step = 1, every quotient is the element itself
    q, step = quant_rows(x)
    assert step[0] == np.float32(1.0)
    assert q[0, :8].tolist() == [127, 1, -1, 3, -3, 127, 2, -127]
    assert not q[0, 8:].any()


def test_the_all_zero_row():
    q, step = quant_rows(np.zeros((2, 128), dtype=np.float32))
    assert step.view(np.uint32).tolist() == [0, 0] and not q.any()


def test_a_row_whose_largest_magnitude_is_negative():
    """the absolute maximum, not CU_X2A8_'s signed one (T.cu:41-43): step > 0, the negative extreme is -127 and nothing clips"""
    x = np.full(128, -0.25, dtype=np.float32)
    x[3], x[5] = -8.0, 2.0
    q, step = quant_rows(x)
    assert step[0] == np.float32(8.0) / np.float32(127.0) and step[0] > 0
    assert q[0, 3] == -127 and q[0, 5] == 32 and q[0, 0] == -4   # 2 / step = 31.75 -> 32; 0.25 / step = 3.97 -> 4
    allneg = -np.abs(np.random.default_rng(3).normal(0, 1, 256)).astype(np.float32)
    q, step = quant_rows(allneg)
    assert step[0] > 0 and q.min() == -127 and q.max() <= 0
