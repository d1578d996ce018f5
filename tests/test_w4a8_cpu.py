"""W4.A8 without a GPU: the two routes of kf::a8_plan (through kfdbg_a8_route_plan, tests/a8_plan_mirror.py) are the one rule behind kf_linear_w4a8 and
kf_linear_w4a8_tiles -- refusals, lanes per row, tiles, grid, LDS -- and the numpy restatement (tests/w4a8_restate.py) of the definition (include/kf_abi.h "int8
activations for 4-bit layers") is held against exact rational arithmetic with one rounding per operation."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import w4a8_restate as R
from a8_plan_mirror import (BF16, BOOL1, F8, GROUP_LDS, INVALID_ARGS, LDS_MAX, MATVEC, OK, ORDER_CHAIN, Q2, Q3, Q4, Q4_FAMILY, QUANT_ERR, ROW_LUT, ROW_RTN, T_BINARY, T_SIGN,
                            TILE_MIN, TILES, TOK_TILE, UNALIGN, UNSUPPORTED, plan)
from a8_plan_mirror import mat as any_mat
from koifish_amd import lib as L
from oracle import oracle as O


def mat(M, K, type=Q4, **kw):
    return any_mat(M, K, type=type, **kw)


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def plans():
    return lambda m, nTok=1, qbias=0: (plan(Q4_FAMILY, MATVEC, m, nTok, qbias), plan(Q4_FAMILY, TILES, m, nTok, qbias))


def test_symbols():
    hip, host = L.load()
    for f in ("kf_linear_w4a8", "kf_linear_w4a8_status", "kf_linear_w4a8_tiles", "kf_linear_w4a8_tiles_status", "kfdbg_w4a8_plan", "kfdbg_w4a8_tile_plan", "kfdbg_a8_route_plan"):
        assert hasattr(hip, f), f
        assert not f.startswith("kf_") or f in L.ABI_SYMBOLS
    assert hasattr(host, "kfh_set_act_int8_q4")
    from koifish_amd.runtime import Context, Qwen3
    assert hasattr(Context, "linear_w4a8") and hasattr(Context, "linear_w4a8_tiles") and hasattr(Qwen3, "set_act_int8_q4")


# ---------------------------------------------------------------- 1. the refusals: the low-bit family's order and codes
@pytest.mark.parametrize("m,nTok,qbias,want", [
    (mat(64, 1024, type=BF16, gama=0), 1, 0, UNSUPPORTED),
    (mat(64, 1024, type=F8, gama=0), 1, 0, UNSUPPORTED),
    (mat(64, 1024, type=T_SIGN), 1, 1, UNSUPPORTED),
    (mat(64, 1024, type=BOOL1), 1, 0, UNSUPPORTED),
    (mat(64, 1024, type=T_BINARY), 1, 0, UNSUPPORTED),
    (mat(64, 1024, type=Q2), 1, 0, UNSUPPORTED),
    (mat(64, 1024, type=Q3), 1, 0, UNSUPPORTED),
    (mat(64, 1024, awq=1), 1, 0, UNSUPPORTED),
    (mat(64, 1024, quant=ROW_LUT), 1, 0, UNSUPPORTED),
    (mat(64, 1024, quant=ROW_RTN), 1, 0, UNSUPPORTED),
    (mat(64, 1024, type=T_SIGN, lgroup=64, al=0), 1, 0, UNSUPPORTED),   # the storage before anything else
    (mat(64, 1024, lgroup=64), 1, 0, QUANT_ERR),
    (mat(64, 1024, lgroup=256), 1, 0, QUANT_ERR),
    (mat(64, 1024, gama=0), 1, 0, QUANT_ERR),
    (mat(64, 1024), 1, 7, QUANT_ERR),
    (mat(64, 1024), 1, 1, QUANT_ERR),
    (mat(64, 1024), 1, -8, QUANT_ERR),
    (mat(64, 1088, gama=0, al=0), 1, 0, QUANT_ERR),                     # the groups before the shape and the alignment
    (mat(64, 1088), 1, 0, INVALID_ARGS),                                # 1088 % 128 = 64
    (mat(64, 64), 1, 0, INVALID_ARGS),
    (mat(0, 1024), 1, 8, INVALID_ARGS),
    (mat(64, 1024), 0, 0, INVALID_ARGS),
    (mat(64, 1088, al=0), 1, 0, INVALID_ARGS),                          # the shape before the alignment
    (mat(64, 1024, al=2), 1, 0, UNALIGN),
    (mat(64, 1024, al=0), 1, 8, UNALIGN),
    (mat(64, 1024), 1, 0, OK),
    (mat(64, 1024), 1, 8, OK),
    (mat(64, 128), 70, 8, OK),
    (mat(1, 1024, al=1), 1, 0, OK),                                     # only the data's alignment counts
])
def test_refusals(plans, m, nTok, qbias, want):
    a, b = plans(m, nTok, qbias)
    assert a.status == want and b.status == want   # the tile plan takes the mat-vec plan's status
    if want == OK:
        assert a.qbias == b.qbias == qbias


def test_lds_bound_refuses(plans):
    """four token rows of K bytes (x 144 / 128) must fit in the mat-vec's LDS; the tile plan takes that status"""
    assert [p.status for p in plans(mat(8, 36352), 2)] == [OK, OK]
    assert [p.status for p in plans(mat(8, 36480), 2)] == [INVALID_ARGS, INVALID_ARGS]
    assert plans(mat(8, 36480), 1)[0].status == OK


# ---------------------------------------------------------------- 2. geometry; the order is a function of K alone
@pytest.mark.parametrize("K,lpr_log2,iters", [(128, 0, 1), (384, 1, 2), (1280, 3, 2), (1024, 3, 1), (8192, 6, 1)])
@pytest.mark.parametrize("M", [1, 80, 151936])
@pytest.mark.parametrize("nTok", [1, TOK_TILE, TOK_TILE + 1])
def test_matvec_geometry(plans, K, lpr_log2, iters, M, nTok):
    p = plans(mat(M, K), nTok)[0]
    G = K // 128
    assert p.status == OK
    assert (p.order, p.n_groups, p.lpr_log2, p.iters) == (ORDER_CHAIN, G, lpr_log2, iters)
    assert (iters << lpr_log2) >= G > ((iters - 1) << lpr_log2)                 # every group has a lane, no step is empty
    assert p.rows_per_wave == 64 >> lpr_log2 and p.rows_per_wg == 4 * p.rows_per_wave and p.block == 256
    assert p.tok_tile == (1 if nTok == 1 else TOK_TILE)
    assert p.tok_tiles == -(-nTok // p.tok_tile) == p.grid_y
    assert (p.grid_x - 1) * p.rows_per_wg < M <= p.grid_x * p.rows_per_wg       # every row has a lane group, no workgroup is empty
    assert p.lds == p.tok_tile * G * GROUP_LDS and 0 < p.lds <= LDS_MAX


@pytest.mark.parametrize("K", [128, 384, 1280, 1024, 8192])
@pytest.mark.parametrize("M", [1, 80, 130, 151936])
@pytest.mark.parametrize("nTok", [1, 16, 17, 70, 2047])
def test_tile_geometry(plans, K, M, nTok):
    p = plans(mat(M, K), nTok, 8)[1]
    assert p.status == OK and p.qbias == 8
    assert (p.order, p.n_groups) == (ORDER_CHAIN, K // 128)
    assert p.waves == 4 and p.row_tile == 64 and p.block == 256
    assert p.mfma_tok in (1, 2, 4) and p.tok_tile == 16 * p.mfma_tok
    assert (p.grid_x - 1) * p.row_tile < M <= p.grid_x * p.row_tile             # the tiles cover every row, no workgroup is empty
    assert (p.grid_y - 1) * p.tok_tile < nTok <= p.grid_y * p.tok_tile          # ... and every token
    assert p.chunk == min(8, K // 128)
    assert p.lds == p.tok_tile * p.chunk * GROUP_LDS + 2 * p.row_tile * p.chunk * 4   # staged activations + the chunk's STEP and ZERO as fp32
    assert 0 < p.lds <= LDS_MAX
    assert p.min_tok == TILE_MIN


@pytest.mark.parametrize("K", [128, 384, 1280, 1024, 8192])
def test_order_depends_on_K_only(plans, K):
    seen = set()
    for M in (1, 7, 80, 151936):
        for nTok in (1, 2, 5, 17, 2047):
            for qb in (0, 8):
                a, b = plans(mat(M, K), nTok, qb)
                seen |= {(a.order, a.n_groups), (b.order, b.n_groups)}
    assert seen == {(ORDER_CHAIN, K // 128)}


# ---------------------------------------------------------------- 3. the status entries, for every storage type
def test_status_entries(hip):
    assert hip.kf_linear_w4a8_status(None, 1) == INVALID_ARGS and hip.kf_linear_w4a8_tiles_status(None, 1) == INVALID_ARGS
    buf = (C.c_uint8 * 64)()
    data = (C.addressof(buf) + 15) & ~15

    def both(type_, nTok=1, ne1=256, lGroup=128, gama=True, quant=0, off=0, qBias=0, awq=False):
        w = L.Weight(data + off, data if gama else None, type_, 16, ne1, 16 * ne1 // max(lGroup, 1), lGroup, 0, 15, qBias, data if awq else None, None, quant, 0)
        a, b = hip.kf_linear_w4a8_status(C.byref(w), nTok), hip.kf_linear_w4a8_tiles_status(C.byref(w), nTok)
        assert a == b
        return a
    assert [both(L.Q4, n, qBias=qb) for n in (1, 70) for qb in (0, 8)] == [OK] * 4
    others = (L.F32, L.F16, L.BF16, L.F8E5M2, L.F8E4M3, L.I8, L.Q3, L.Q2, L.T_SIGN, L.T_SEQ, L.BOOL1, L.T_BINARY, L.T_BINARY_3, L.T_BINARY_TILE)
    assert [both(t, 70) for t in others] == [UNSUPPORTED] * len(others)
    assert both(L.Q4, quant=L.QUANT_ROW_LUT) == UNSUPPORTED and both(L.Q4, quant=L.QUANT_ROW_RTN) == UNSUPPORTED and both(L.Q4, awq=True) == UNSUPPORTED
    assert both(L.T_SIGN, lGroup=64, gama=False, off=8) == UNSUPPORTED   # the other family's storage is refused as storage, whatever else is wrong with it
    assert both(L.Q4, lGroup=64) == QUANT_ERR and both(L.Q4, gama=False) == QUANT_ERR and both(L.Q4, qBias=4) == QUANT_ERR
    assert both(L.Q4, ne1=192) == INVALID_ARGS and both(L.Q4, 0) == INVALID_ARGS and both(L.Q4, off=8) == UNALIGN
    # the existing entries keep refusing 4-bit storage
    w = L.Weight(data, data, L.Q4, 16, 256, 32, 128, 0, 15, 0, None, None, 0, 0)
    assert hip.kf_linear_a8_status(C.byref(w), 1) == UNSUPPORTED and hip.kf_linear_a8_tiles_status(C.byref(w), 70) == UNSUPPORTED


# ---------------------------------------------------------------- 4. the restatement against exact rational arithmetic
def rn32(x):
    """a Fraction rounded to the nearest fp32, ties to even: numpy's float64 -> float32 is exact here only when x is a float64, so round by hand"""
    if x == 0:
        return Fraction(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and e >= -126   # normal range: the tests' magnitudes
    ulp = Fraction(2) ** (e - 23)
    n = a / ulp
    k = n.numerator // n.denominator
    r = n - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and k % 2 == 1):
        k += 1
    return s * k * ulp


def exact_chain(w, q, r, t):
    """the definition for output (row r, token t) in Fractions: one rounding per multiply, subtract and add"""
    G = w.K // 128
    acc = Fraction(0)
    for g in range(G):
        qs = [int(v) for v in q[t, 128 * g:128 * g + 128]]
        I = sum(int(c) * v for c, v in zip(w.t[r, 128 * g:128 * g + 128], qs))
        S = sum(qs)
        p = rn32(Fraction(float(w.step[r, g])) * I)
        z = Fraction(float(w.zero[r, g])) * S
        assert rn32(z) == z, "ZERO * S_g is exact"
        acc = rn32(acc + rn32(p - z))
    return acc


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("K", [128, 384, 1280])
def test_restatement_against_fractions(symmetric, K):
    M, n = 6, 3
    rng = np.random.default_rng(K + symmetric)
    wf = rng.normal(0, 0.05, (M, K)).astype(np.float32) + np.repeat(rng.normal(0, 0.04, (M, K // 128)).astype(np.float32), 128, axis=1)   # a per-group offset: ZERO != 0
    ow = O.quantize(R.to_bf(wf), M, K, L.Q4, symmetric=symmetric)
    assert ow.qBias == (8 if symmetric else 0)
    w = R.IntW4(ow)
    assert symmetric or (w.zero != 0).all()
    q, _ = R.quant_rows(R.to_bf(rng.normal(0, 1, (n, K)).astype(np.float32)))
    acc = R.chain(w, q)
    for r in range(M):
        for t in range(n):
            want = exact_chain(w, q, r, t)
            assert Fraction(float(acc[t, r])) == want, (r, t)


@pytest.mark.parametrize("qBias", [0, 8])
def test_restatement_where_the_multiply_rounds(qBias):
    """sums of 17 and 18 significant bits: STEP * I_g is NOT exact there, and the restatement rounds it once, then the subtract, then the add"""
    M, K, n = 24, 384, 4
    ow, q, _ = R.large_sum_case(M, K, n, 11, qBias)
    w = R.IntW4(ow)
    acc = R.chain(w, q)
    I, _ = R.group_sums(w, q)
    inexact = fused = 0
    for r in range(M):
        for t in range(n):
            assert Fraction(float(acc[t, r])) == exact_chain(w, q, r, t), (r, t)
            a1 = Fraction(0)   # the chain a fused multiply-subtract would give
            for g in range(K // 128):
                pe = Fraction(float(w.step[r, g])) * int(I[t, r, g])
                inexact += pe != rn32(pe)
                S = int(q[t, 128 * g:128 * g + 128].astype(np.int64).sum())
                a1 = rn32(a1 + rn32(pe - Fraction(float(w.zero[r, g])) * S))
            fused += a1 != Fraction(float(acc[t, r]))
    assert inexact > 0 and fused > 0, "the case must tell the three roundings from an fma"


def test_group_sums_are_the_integer_sums():
    """the restatement forms I_g through float64 matrix products: equal to the plain int64 sums"""
    ow, q, _ = R.large_sum_case(5, 384, 3, 2, 8)
    w = R.IntW4(ow)
    I, S = R.group_sums(w, q)
    want = np.einsum("mgc,tgc->tmg", w.t.reshape(5, 3, 128), q.astype(np.int64).reshape(3, 3, 128))
    assert I.dtype == np.int64 and np.array_equal(I, want) and np.array_equal(S, q.astype(np.int64).reshape(3, 3, 128).sum(axis=2))


@pytest.mark.parametrize("M,nTok,mfma_tok", [(1000, 500, 2), (1000, 1030, 4), (1000, 70, 1), (3072, 2047, 4), (1024, 128, 1)])
def test_token_tile_widens(plans, M, nTok, mfma_tok):
    """the 32- and 64-token forms are chosen once 256 workgroups remain: the shapes tests/test_gpu_w4a8_tiles.py runs them at, and Qwen3-0.6B's gate at a long prompt"""
    assert plans(mat(M, 1280), nTok)[1].mfma_tok == mfma_tok


def test_bounds_of_the_definition():
    """|I_g| <= 243 840 < 2^24 and |S_g| <= 16 256: fp32(I_g), fp32(S_g) and ZERO * S_g (8 + 14 bits) are exact"""
    assert 128 * 15 * 127 == 243840 < 2 ** 24 and 128 * 127 == 16256 < 2 ** 14
    for v in (243840, -243840, 243839, 16256):
        assert int(np.float32(v)) == v
    z = R.bf(np.array([0x3f7f], dtype=np.uint16))[0]   # 8 significant bits
    assert Fraction(float(np.float32(z) * np.float32(16255))) == Fraction(float(z)) * 16255
