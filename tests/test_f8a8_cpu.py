"""fp8 activations for f8e5m2 layers without a GPU: kf::f8a8_plan (through kfdbg_f8a8_plan) is the one rule behind kf_linear_f8a8 -- refusals in order, the single chain, the
tile form -- and the restated quantiser (tests/f8a8_restate.py) has the properties the definition states (include/kf_abi.h "fp8 activations for f8e5m2 layers")."""
import ctypes as C

import numpy as np
import pytest

import f8a8_restate as R
from a8_plan_mirror import BF16, F8, INVALID_ARGS, OK, Q4, ROW_LUT, T_SIGN, UNALIGN, UNSUPPORTED, mat
from koifish_amd import lib as L
from plan_structs import GemmMat

ORDER_CHAIN, TILE_MIN, FORM_TOK = 1, 128, (16, 32, 64, 128)   # kf_f8a8.h; KF_F8A8_TILE_MIN


class Problem(C.Structure):   # kf::F8A8Problem
    _fields_ = [("w", GemmMat), ("nTok", C.c_int), ("q_al", C.c_int)]


class Plan(C.Structure):   # kf::F8A8Plan
    _fields_ = [(f, C.c_int) for f in ("status", "order", "n_steps", "half_tail", "form", "row_tile", "tok_tile", "stages", "grid_x", "grid_y", "block", "lds", "min_tok")]


def plan(m, nTok=1, q_al=1):
    hip = L.load()[0]
    hip.kfdbg_f8a8_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]
    out = Plan()
    assert hip.kfdbg_f8a8_plan(C.byref(Problem(m, nTok, q_al)), C.byref(out)) == 0 and out.min_tok == TILE_MIN
    assert out.status == OK or not any(getattr(out, f) for f, _ in Plan._fields_ if f not in ("status", "min_tok"))   # a refusal carries no figure
    return out


def f8(M, K, **kw):
    return mat(M, K, type=F8, gama=0, **kw)


@pytest.mark.parametrize("m,nTok,q_al,want", [
    (mat(64, 1024, type=BF16, gama=0), 1, 1, UNSUPPORTED), (mat(64, 1024, type=Q4), 1, 1, UNSUPPORTED), (mat(64, 1024, type=T_SIGN), 1, 1, UNSUPPORTED),
    (mat(64, 1024, type=5, gama=0), 1, 1, UNSUPPORTED),                               # KF_F8E4M3 weights are out of scope
    (f8(64, 1024, awq=1), 1, 1, UNSUPPORTED), (f8(64, 1024, quant=ROW_LUT), 1, 1, UNSUPPORTED),
    (mat(0, 100, type=BF16, al=0), 0, 0, UNSUPPORTED),                                # the storage before anything else
    (f8(64, 64), 1, 1, INVALID_ARGS), (f8(64, 127), 1, 1, INVALID_ARGS), (f8(64, 128), 1, 1, OK), (f8(64, 192), 1, 1, OK), (f8(64, 160), 1, 1, INVALID_ARGS),
    (f8(0, 1024), 1, 1, INVALID_ARGS), (f8(1, 1024), 1, 1, OK), (f8(64, 1024), 0, 1, INVALID_ARGS), (f8(64, 1600), 2047, 1, OK),
    (f8(64, 127, al=0), 1, 0, INVALID_ARGS),                                          # the shape before the alignment
    (f8(64, 1024, al=2), 1, 1, UNALIGN), (f8(64, 1024, al=1), 1, 1, OK), (f8(64, 1024), 1, 0, UNALIGN),
])
def test_refusals(m, nTok, q_al, want):
    assert plan(m, nTok, q_al).status == want


@pytest.mark.parametrize("K,n_steps,half", [(128, 1, 0), (192, 2, 1), (1024, 8, 0), (1600, 13, 1), (25600, 200, 0)])
def test_chain_depends_on_K_only_and_the_tiles_cover(K, n_steps, half):
    seen = set()
    for M in (1, 130, 4096, 151936):
        for nTok in (1, 17, 129, 2047):
            p = plan(f8(M, K), nTok)
            seen.add((p.order, p.n_steps, p.half_tail))
            assert p.row_tile == 128 and p.block == 256 and p.stages == 2 and p.tok_tile == FORM_TOK[p.form]
            assert (p.grid_x - 1) * p.row_tile < M <= p.grid_x * p.row_tile and (p.grid_y - 1) * p.tok_tile < nTok <= p.grid_y * p.tok_tile
            assert p.lds == p.stages * (p.row_tile + p.tok_tile) * 128 <= 64 * 1024
            assert p.form == 0 or (FORM_TOK[p.form - 1] < nTok and p.grid_x * p.grid_y >= 256)   # a wider tile only where it is needed and 256 workgroups remain
    assert seen == {(ORDER_CHAIN, n_steps, half)}


@pytest.mark.parametrize("M,nTok,form", [(16, 1, 0), (256, 129, 0), (4096, 256, 1), (4096, 512, 2), (4096, 1024, 3), (1024, 2047, 2), (3072, 2047, 3)])
def test_token_tile_widens(M, nTok, form):
    assert plan(f8(M, 1024), nTok).form == form


def test_status_entry_for_every_storage():
    hip = L.load()[0]
    buf = (C.c_uint8 * 64)()
    data = (C.addressof(buf) + 15) & ~15
    st = lambda type_, nTok=40, ne1=256, off=0, quant=0, awq=False: hip.kf_linear_f8a8_status(
        C.byref(L.Weight(data + off, None, type_, 16, ne1, 0, 0, 0, 0, 0, data if awq else None, None, quant, 0)), nTok)
    others = (L.F32, L.F16, L.BF16, L.F8E4M3, L.I8, L.Q4, L.Q3, L.Q2, L.T_SIGN, L.T_SEQ, L.BOOL1, L.T_BINARY, L.T_BINARY_3, L.T_BINARY_TILE)
    assert [st(t) for t in others] == [UNSUPPORTED] * len(others) and st(L.F8E5M2, awq=True) == UNSUPPORTED and st(L.F8E5M2, quant=L.QUANT_ROW_LUT) == UNSUPPORTED
    assert [st(L.F8E5M2, n) for n in (1, 40, 2047)] == [OK] * 3 and st(L.F8E5M2, ne1=64) == INVALID_ARGS and st(L.F8E5M2, 0) == INVALID_ARGS and st(L.F8E5M2, off=8) == UNALIGN
    assert hip.kf_linear_f8a8_status(None, 1) == INVALID_ARGS
    from koifish_amd.runtime import Context, Qwen3
    assert all(hasattr(Context, f) for f in ("act_quant_f8", "linear_f8a8")) and all(hasattr(Qwen3, f) for f in ("set_act_fp8", "set_f8a8_tile_min", "f8a8_route_counts"))


def test_restated_quantiser():
    rng = np.random.default_rng(5)
    v = (rng.normal(0, 1, (64, 256)) * np.exp2(rng.integers(-20, 20, (64, 1)))).astype(np.float32)
    v[:4] = 0.0                                       # row 0 stays a zero row: step 0, every code 0
    v[1, 0], v[2, 0], v[3, 0] = 448.0 * 2.0 ** 5, 448.0 * 2.0 ** -7 * (1 + 2.0 ** -20), 1e30   # exactly 448 * 2^e keeps e; a hair above moves to e + 1
    q, step = R.quant_rows_f32(v)
    amax = np.abs(v).max(axis=1)
    assert step[0] == 0 and not q[0].any() and step[1] == 2.0 ** 5 and q[1, 0] == 0x7e and step[2] == 2.0 ** -6
    r = amax[1:].astype(np.float64) / step[1:]
    assert (r > 224).all() and (r <= 448).all() and (np.log2(step[1:]) % 1 == 0).all()
    assert not np.isin(q, (0x7f, 0xff)).any()         # never NaN: nothing exceeds 448
    # ties round to even: between the neighbours 16 (0x58) and 18 (0x59) lies 17 -> 16; between 18 and 20 (0x5a) lies 19 -> 20; and the e4m3 subnormals (multiples of 2^-9)
    t = np.array([[448.0, 17.0, 19.0, -17.0, 2.0 ** -9, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -10 * 1.01, 7 * 2.0 ** -9]], dtype=np.float32)
    q, step = R.quant_rows_f32(t)
    assert step[0] == 1.0 and list(q[0]) == [0x7e, 0x58, 0x5a, 0xd8, 0x01, 0x02, 0x02, 0x00, 0x01, 0x07]
    assert R.E4M3[0x7e] == 448 and R.E4M3[0x01] == 2.0 ** -9 and R.E5M2[0x7b] == 57344 and R.E5M2[0x01] == 2.0 ** -16 and R.E5M2[0xbc] == -1.0
