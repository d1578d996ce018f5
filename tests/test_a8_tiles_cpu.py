"""The int8 MFMA tile plan without a GPU: the tile route of kf::a8_plan (through kfdbg_a8_route_plan) is the one rule behind kf_linear_a8_tiles.  Its refusals are the mat-vec
route's -- one rule, asked twice: the refusal table of tests/test_a8_plan_cpu.py gives the same status through either -- and its tiles cover M x nTok with no empty workgroup inside
160 KB of LDS.  The per-row summation order (one ascending chain over the K / 128 groups) is a function of K alone: the fields that carry it may not move with M or nTok."""
import ctypes as C

import pytest

import test_a8_plan_cpu as P1
from a8_plan_mirror import LOWBIT, MATVEC, TILE_MIN, TILES, plan
from koifish_amd import lib as L


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def tile_plan():
    return lambda m, nTok=1: plan(LOWBIT, TILES, m, nTok)


def test_symbols():
    hip, host = L.load()
    for f in ("kf_linear_a8_tiles", "kf_linear_a8_tiles_status", "kfdbg_a8_tile_plan", "kf_linear_a8", "kfdbg_a8_plan", "kfdbg_a8_route_plan"):
        assert hasattr(hip, f), f
    for f in ("kfh_set_a8_tile_min", "kfh_a8_route_counts"):
        assert hasattr(host, f), f
    assert "kf_linear_a8_tiles" in L.ABI_SYMBOLS and "kf_linear_a8_tiles_status" in L.ABI_SYMBOLS
    from koifish_amd.runtime import Context, Qwen3
    assert hasattr(Context, "linear_a8_tiles") and hasattr(Qwen3, "set_a8_tile_min") and hasattr(Qwen3, "a8_route_counts")


REFUSALS = list(P1.test_refusals.pytestmark[0].args[1])   # the table of tests/test_a8_plan_cpu.py itself


def test_the_refusal_table_is_the_other_file_s():
    assert len(REFUSALS) == 22 and {w for _, _, w in REFUSALS} == {P1.OK, P1.INVALID_ARGS, P1.QUANT_ERR, P1.UNSUPPORTED, P1.UNALIGN}


@pytest.mark.parametrize("m,nTok,want", REFUSALS)
def test_one_rule_asked_twice(tile_plan, m, nTok, want):
    assert tile_plan(m, nTok).status == plan(LOWBIT, MATVEC, m, nTok).status == want


def test_lds_refusal_is_a8_plan_s(tile_plan):
    """a row the mat-vec route refuses for its own LDS (tests/test_a8_plan_cpu.py test_lds_bound_refuses) is refused here with the same status"""
    assert tile_plan(P1.mat(8, 36352), 2).status == P1.OK
    assert tile_plan(P1.mat(8, 36480), 2).status == P1.INVALID_ARGS


@pytest.mark.parametrize("K", [128, 384, 1024, 3072, 25600])
@pytest.mark.parametrize("M", [1, 257, 151936])
@pytest.mark.parametrize("nTok", [1, 16, 17, 2047])
@pytest.mark.parametrize("type_,bits", [(P1.T_SIGN, 2), (P1.BOOL1, 1)])
def test_geometry(tile_plan, K, M, nTok, type_, bits):
    p = tile_plan(P1.mat(M, K, type=type_), nTok)
    assert p.status == P1.OK and p.bits == bits
    assert (p.order, p.n_groups) == (P1.ORDER_CHAIN, K // 128)                      # whatever M and nTok
    assert p.waves == 4 and p.row_tile == 16 * p.waves and p.block == 64 * p.waves
    assert p.mfma_tok in (1, 2, 4) and p.tok_tile == 16 * p.mfma_tok
    assert p.grid_x > 0 and p.grid_y > 0
    assert (p.grid_x - 1) * p.row_tile < M <= p.grid_x * p.row_tile                 # the tiles cover every row, no workgroup is empty
    assert (p.grid_y - 1) * p.tok_tile < nTok <= p.grid_y * p.tok_tile              # ... and every token
    assert 1 <= p.chunk <= min(8, K // 128)
    assert p.lds == p.tok_tile * p.chunk * P1.GROUP_LDS + p.row_tile * p.chunk * 4  # staged activations + the chunk's weight steps
    assert 0 < p.lds <= P1.LDS_MAX
    assert p.min_tok == TILE_MIN


@pytest.mark.parametrize("K", [128, 384, 1024, 3072, 25600])
def test_order_depends_on_K_only(tile_plan, K):
    seen = {(p.order, p.n_groups) for p in (tile_plan(P1.mat(M, K, type=t), n) for M in (1, 7, 257, 151936) for n in (1, 16, 17, 33, 2047) for t in (P1.T_SIGN, P1.BOOL1))}
    assert seen == {(P1.ORDER_CHAIN, K // 128)}


def test_status_entry(hip):
    """kf_linear_a8_tiles_status: the plan's answer without a launch -- the same answers as kf_linear_a8_status"""
    assert hip.kf_linear_a8_tiles_status(None, 1) == -20
    buf = (C.c_uint8 * 64)()
    data = (C.addressof(buf) + 15) & ~15

    def both(type_, nTok=1, ne1=256, lGroup=128, gama=True, quant=0, off=0):
        w = L.Weight(data + off, data if gama else None, type_, 16, ne1, 16 * ne1 // max(lGroup, 1), lGroup, 0, 1, 0, None, None, quant, 0)
        a, b = hip.kf_linear_a8_tiles_status(C.byref(w), nTok), hip.kf_linear_a8_status(C.byref(w), nTok)
        assert a == b
        return a
    assert [both(t, n) for t in (L.T_SIGN, L.BOOL1, L.T_BINARY) for n in (1, 70)] == [0] * 6
    assert [both(t, 70, gama=(t == L.Q4)) for t in (L.Q4, L.BF16, L.F8E5M2)] == [-1000] * 3
    assert both(L.T_SIGN, quant=L.QUANT_ROW_LUT) == -1000
    assert both(L.Q4, lGroup=64, gama=False, off=8) == -1000   # the other family's storage is refused as storage, whatever else is wrong with it
    assert both(L.T_SIGN, lGroup=64) == -701 and both(L.BOOL1, gama=False) == -701
    assert both(L.T_SIGN, ne1=192) == -20 and both(L.T_SIGN, 0) == -20 and both(L.T_SIGN, off=8) == -2000
