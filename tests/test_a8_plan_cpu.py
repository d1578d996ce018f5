"""The int8-activation mat-vec plan without a GPU: the mat-vec route of kf::a8_plan (through kfdbg_a8_route_plan, tests/a8_plan_mirror.py) is the one rule behind kf_linear_a8
-- the refusals, the lanes per row, the token rows per weight pass, grid and LDS -- pinned on each side of every boundary.  The per-row summation order (one ascending chain over the K / 128 groups) is a function of K
alone: the fields that carry it may not move with nTok or M."""
import pytest

from a8_plan_mirror import (BF16, BOOL1, F8, GROUP_LDS, INVALID_ARGS, LDS_MAX, LOWBIT, MATVEC, OK, ORDER_CHAIN, Q2, Q4, QUANT_ERR, ROW_LUT, ROW_RTN, T_BINARY, T_SIGN, TOK_TILE,  # noqa: F401
                            UNALIGN, UNSUPPORTED, mat)
from a8_plan_mirror import check_views
from a8_plan_mirror import plan as a8_plan


@pytest.fixture(scope="module")
def plan():
    return lambda m, nTok=1: a8_plan(LOWBIT, MATVEC, m, nTok)


@pytest.mark.parametrize("m,nTok,want", [
    (mat(64, 1024, type=BF16, gama=0), 1, UNSUPPORTED),
    (mat(64, 1024, type=F8, gama=0), 1, UNSUPPORTED),
    (mat(64, 1024, type=Q4), 1, UNSUPPORTED),
    (mat(64, 1024, type=Q4, awq=1), 1, UNSUPPORTED),
    (mat(64, 1024, type=T_SIGN, awq=1), 1, UNSUPPORTED),
    (mat(64, 1024, type=Q4, quant=ROW_LUT), 1, UNSUPPORTED),
    (mat(64, 1024, type=Q2, quant=ROW_RTN), 1, UNSUPPORTED),
    (mat(64, 1024, type=T_SIGN, quant=ROW_LUT), 1, UNSUPPORTED),
    (mat(64, 1024, type=Q4, lgroup=64, al=0), 1, UNSUPPORTED),        # the storage before anything else
    (mat(64, 1024, lgroup=64), 1, QUANT_ERR),
    (mat(64, 1024, lgroup=256), 1, QUANT_ERR),
    (mat(64, 1024, gama=0), 1, QUANT_ERR),
    (mat(64, 1024, type=BOOL1, gama=0, al=0), 1, QUANT_ERR),          # the groups before the alignment
    (mat(64, 1088), 1, INVALID_ARGS),                                 # 1088 % 128 = 64
    (mat(64, 64), 1, INVALID_ARGS),
    (mat(0, 1024), 1, INVALID_ARGS),
    (mat(64, 1024), 0, INVALID_ARGS),
    (mat(64, 1024, al=2), 1, UNALIGN),
    (mat(64, 1024, type=BOOL1, al=0), 1, UNALIGN),
    (mat(64, 1024), 1, OK),
    (mat(64, 128), 1, OK),
    (mat(1, 1024, al=1), 1, OK),                                      # only the data's alignment counts
])
def test_refusals(plan, m, nTok, want):
    assert plan(m, nTok).status == want


@pytest.mark.parametrize("type_,bits", [(T_SIGN, 2), (BOOL1, 1), (T_BINARY, 1)])
def test_served_types(plan, type_, bits):
    p = plan(mat(1024, 1024, type=type_))
    assert (p.status, p.bits, p.order, p.n_groups) == (OK, bits, ORDER_CHAIN, 8)


@pytest.mark.parametrize("K,lpr_log2,iters", [
    (128, 0, 1),      # one group: one lane per row
    (256, 1, 1),
    (384, 1, 2),      # three groups: two lanes, the second step half masked
    (1024, 3, 1),
    (2048, 4, 1),
    (3072, 3, 3),     # 24 groups: 8 divides them
    (8192, 6, 1),
    (25600, 3, 25),   # 200 groups
])
@pytest.mark.parametrize("M", [1, 151936])
@pytest.mark.parametrize("nTok", [1, TOK_TILE, TOK_TILE + 1])
def test_geometry(plan, K, lpr_log2, iters, M, nTok):
    p = plan(mat(M, K), nTok)
    G = K // 128
    assert p.status == OK
    assert (p.n_groups, p.lpr_log2, p.iters) == (G, lpr_log2, iters)
    assert (iters << lpr_log2) >= G > ((iters - 1) << lpr_log2)                 # every group has a lane, no step is empty
    assert p.rows_per_wave == 64 >> lpr_log2 and p.rows_per_wg == 4 * p.rows_per_wave and p.block == 256
    assert p.tok_tile == (1 if nTok == 1 else TOK_TILE)
    assert p.tok_tiles == -(-nTok // p.tok_tile) == p.grid_y
    assert p.grid_x > 0 and p.grid_y > 0
    assert (p.grid_x - 1) * p.rows_per_wg < M <= p.grid_x * p.rows_per_wg       # every row has a lane group, no workgroup is empty
    assert p.lds == p.tok_tile * G * GROUP_LDS and 0 < p.lds <= LDS_MAX


def test_lds_bound_refuses(plan):
    """four token rows of K bytes (x 144 / 128) must fit: the longest row of a token batch is 36 352, of a single token 145 536"""
    assert plan(mat(8, 36352), 2).status == OK and plan(mat(8, 36352), 2).lds <= LDS_MAX
    assert plan(mat(8, 36480), 2).status == INVALID_ARGS
    assert plan(mat(8, 36480), 1).status == OK
    assert plan(mat(8, 145536), 1).status == OK
    assert plan(mat(8, 145664), 1).status == INVALID_ARGS


@pytest.mark.parametrize("K", [128, 384, 1024, 3072, 25600])
@pytest.mark.parametrize("type_", [T_SIGN, BOOL1])
def test_order_depends_on_K_only(plan, K, type_):
    """the plans for nTok = 1 and nTok = 9, for one row and for 151 936, name the same per-row order"""
    ref = plan(mat(64, K, type=type_), 1)
    for M in (1, 7, 151936):
        for nTok in (1, 2, 5, 9):
            p = plan(mat(M, K, type=type_), nTok)
            assert (p.order, p.n_groups) == (ref.order, ref.n_groups) == (ORDER_CHAIN, K // 128)


def test_the_earlier_exports_are_views_of_this_plan():
    check_views()
