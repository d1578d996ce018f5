"""The row mat-vec plan without a GPU: kf::gemv_rows_plan (through kfdbg_gemv_rows_plan) lays out the launch of R = 1 .. 8 activation rows over one pass of the
packed weights (kf_linear_rows and its siblings).  What fixes the bits -- the storage form, the lanes per row, the steps per row, the group shift -- must be the
one-token plan's (kfdbg_gemv_plan) for the same matrices, so that row r carries the one-token launch's bits by construction; what the row plan adds -- the rows per
pass, the activation form in LDS, the panel cut, the route -- is pinned on each side of its boundaries."""
import ctypes as C

import pytest

from koifish_amd import lib as L
from plan_structs import GemmMat as Mat, GemvPlan as Plan, GemvProblem as Problem, GemvRowsPlan as RowsPlan, GemvRowsProblem as RowsProblem

BF16, F8, Q4, Q3, T_SIGN, BOOL1 = 3, 4, 14, 15, 17, 19                          # kf_dtype
GROUP, ROW_LUT = 0, 1
FMT_BF16, FMT_F8, FMT_Q4, FMT_Q2, FMT_Q1, FMT_Q4P, FMT_Q4R, FMT_Q1T, FMT_Q2T = range(9)
PLAIN, PAIRED, ARGMAX = range(3)
OK, INVALID_ARGS, QUANT_ERR, UNSUPPORTED, UNALIGN = 0, -20, -701, -1000, -2000
LDS_MAX, XF_LDS_MAX, RED = 80 * 1024, 53 * 1024, 256                             # GEMV_ROWS_LDS_MAX, GEMV_ROWS_XF_LDS_MAX, GEMV_RED_BYTES


def mat(M, K, type=Q4, quant=GROUP, lgroup=128, gama=1, al=3, awq=0):
    return Mat(type, quant, awq, M, K, lgroup, gama, al)


@pytest.fixture(scope="module")
def plans():
    hip = L.load()[0]
    hip.kfdbg_gemv_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]
    hip.kfdbg_gemv_rows_plan.argtypes = [C.POINTER(RowsProblem), C.POINTER(RowsPlan)]

    def f(mats, R, mode=PLAIN, norm=0, canon=1, sparse=0, q4_perm=1):
        P = Problem(mode=mode, n_w=len(mats), sparse=sparse, n_hot=0, norm=norm, canon=canon, q4_perm=q4_perm, q2_tab=1, q1_tab=1, xf2=1)
        for i, m in enumerate(mats):
            P.w[i] = m
        one, rows = Plan(), RowsPlan()
        assert hip.kfdbg_gemv_plan(C.byref(P), C.byref(one)) == 0
        assert hip.kfdbg_gemv_rows_plan(C.byref(RowsProblem(P, R)), C.byref(rows)) == 0
        return one, rows
    return f


# ---- the bits: every branch of gemv_lpr_log2 -- fewer than 16 blocks (masked tail), a power of two dividing the blocks, the lanes bump of a short launch with a
# masked last step, a long row, three matrices of unequal heights whose rows count together, bf16 blocks, the arithmetic 4-bit form
CASES = [
    ([mat(64, 128)], {}),                                            # 4 blocks: 4 lanes per row
    ([mat(70, 1024)], {}),
    ([mat(1024, 1024)], {"norm": 1}),
    ([mat(1024, 3072)], {}),                                         # 96 blocks: 32 lanes x 3 steps -> 64 lanes x 2 steps, the last one masked
    ([mat(2560, 9728)], {}),
    ([mat(256, 256), mat(128, 256), mat(128, 256)], {"norm": 1}),    # q | k | v
    ([mat(2048, 1024), mat(1024, 1024), mat(1024, 1024)], {"norm": 1}),
    ([mat(3072, 1024), mat(3072, 1024)], {"mode": PAIRED, "norm": 1}),
    ([mat(512, 256, type=BF16)], {"mode": ARGMAX, "norm": 1}),
    ([mat(151936, 1024, type=BF16)], {"mode": ARGMAX, "norm": 1}),   # the 0.6B head: the one-token plan streams it four slots at a time
    ([mat(64, 1024, lgroup=256)], {}),                               # not the register-table form
    ([mat(64, 1024)], {"q4_perm": 0}),
]


@pytest.mark.parametrize("R", [2, 3, 5, 8])
@pytest.mark.parametrize("mats,kw", CASES)
def test_what_fixes_the_bits_is_the_one_token_plans(plans, mats, kw, R):
    one, rows = plans(mats, R, **kw)
    assert one.status == OK and rows.status == OK and rows.shared == 1
    assert (rows.fmt, rows.mode, rows.K, rows.nBlk, rows.lpr_log2, rows.iters, rows.lgroup, rows.gshift) == \
           (one.fmt, one.mode, one.K, one.nBlk, one.lpr_log2, one.iters, one.lgroup, one.gshift)
    assert rows.njobs == one.njobs and list(rows.M) == list(one.M)
    assert rows.norm_regs == int(one.G == 1 and one.K // 8 <= 512)
    # the geometry of its own: whole waves per job, every slot of every job inside the grid's waves
    rps = 64 >> rows.lpr_log2
    for j in range(rows.njobs):
        end = rows.slot0[j + 1] if j + 1 < rows.njobs else rows.total_slots
        assert rows.slot0[j] % rows.spw == 0 and (end - rows.slot0[j]) * rps >= rows.M[j]
    assert all(s == 0x7fffffff for s in list(rows.slot0)[rows.njobs:])
    assert rows.grid * 4 * rows.spw >= rows.total_slots and rows.grid <= 4096
    assert rows.n_panels * rows.panel_rows >= R and (rows.n_panels - 1) * rows.panel_rows < R
    assert rows.NR == (4 if rows.panel_rows <= 4 else 8) and rows.panel_rows <= rows.NR
    assert rows.lds == rows.panel_rows * rows.K * (4 if rows.xf else 2) + RED <= (XF_LDS_MAX if rows.xf else LDS_MAX)
    assert rows.xf == int(rows.fmt != FMT_BF16 and rows.panel_rows * rows.K * 4 + RED <= XF_LDS_MAX)


def test_pinned_examples(plans):
    _, p = plans([mat(1024, 3072)], 8)
    assert (p.fmt, p.lpr_log2, p.iters, p.xf, p.NR, p.n_panels, p.panel_rows, p.lds, p.spw, p.grid) == (FMT_Q4P, 6, 2, 0, 8, 1, 8, 8 * 6144 + RED, 1, 256)
    _, p = plans([mat(1024, 3072)], 3)
    assert (p.xf, p.NR, p.n_panels, p.panel_rows, p.lds) == (1, 4, 1, 3, 3 * 12288 + RED)
    _, p = plans([mat(64, 128)], 2)
    assert (p.fmt, p.lpr_log2, p.iters, p.gshift, p.xf, p.lds, p.grid) == (FMT_Q4P, 2, 1, 2, 1, 2 * 512 + RED, 1)
    _, p = plans([mat(512, 256, type=BF16)], 8, mode=ARGMAX)
    assert (p.fmt, p.xf, p.lpr_log2, p.iters) == (FMT_BF16, 0, 5, 1)


def test_activation_form_on_each_side_of_the_lds_boundary(plans):
    """fp32 activations while the panel fits 53 KiB that way (three workgroups per CU), else bf16"""
    _, p = plans([mat(64, 2560)], 5)       # 5 x 10240 + 256 = 51456 <= 54272
    assert (p.xf, p.lds) == (1, 51456)
    _, p = plans([mat(64, 2560)], 6)       # 6 x 10240 + 256 = 61696 > 54272: bf16, 6 x 5120 + 256
    assert (p.xf, p.lds) == (0, 30976)
    _, p = plans([mat(64, 1024)], 8)       # the 0.6B hidden size: all eight rows as fp32 (33024)
    assert (p.xf, p.lds) == (1, 33024)
    _, p = plans([mat(64, 1696)], 8)       # 8 x 6784 + 256 = 54528 > 54272 ...
    assert p.xf == 0
    _, p = plans([mat(64, 1664)], 8)       # ... and 8 x 6656 + 256 = 53504
    assert p.xf == 1


def test_panel_cut_on_each_side_of_the_lds_boundary(plans):
    _, p = plans([mat(64, 4992)], 8)       # 8 x 9984 + 256 = 80128: one panel
    assert (p.shared, p.n_panels, p.panel_rows, p.NR, p.xf, p.lds) == (1, 1, 8, 8, 0, 80128)
    _, p = plans([mat(64, 5120)], 8)       # 8 x 10240 + 256 = 82176: two panels of four (as fp32 they would be 82176 bytes again: bf16)
    assert (p.shared, p.n_panels, p.panel_rows, p.NR, p.xf, p.lds) == (1, 2, 4, 4, 0, 4 * 10240 + RED)
    _, p = plans([mat(2560, 9728)], 8)     # the 4B down_proj: four bf16 rows of 19456 bytes per panel
    assert (p.n_panels, p.panel_rows, p.NR, p.xf, p.lds) == (2, 4, 4, 0, 4 * 19456 + RED)
    _, p = plans([mat(2560, 9728)], 5)     # cap 4 -> two panels of 3 and 2
    assert (p.n_panels, p.panel_rows) == (2, 3)
    _, p = plans([mat(64, 13696)], 8)      # cap 2 -> four panels of two
    assert (p.n_panels, p.panel_rows, p.NR) == (4, 2, 4)
    _, p = plans([mat(64, 40832, type=BF16)], 4)   # 81664 + 256 = 81920: one row per panel still shares nothing but fits
    assert (p.shared, p.n_panels, p.panel_rows) == (1, 4, 1)
    _, p = plans([mat(64, 40840, type=BF16)], 4)   # a row too long for LDS next to the scratch: row by row
    assert (p.status, p.shared, p.n_panels, p.panel_rows) == (OK, 0, 4, 1)


@pytest.mark.parametrize("mats,kw,R", [
    ([mat(64, 1024)], {"canon": 0}, 4),                           # the v_dot2c order
    ([mat(64, 1024)], {}, 1),                                     # one row
    ([mat(64, 1024, type=F8)], {}, 4),
    ([mat(64, 1024, type=T_SIGN)], {}, 4),
    ([mat(64, 1024, type=BOOL1)], {}, 8),
    ([mat(64, 1024, type=Q4, quant=ROW_LUT, lgroup=0)], {}, 4),
])
def test_row_by_row_routes(plans, mats, kw, R):
    one, p = plans(mats, R, **kw)
    assert (p.status, p.shared, p.n_panels, p.panel_rows) == (OK, 0, R, 1)
    assert (p.fmt, p.lpr_log2, p.iters) == (one.fmt, one.lpr_log2, one.iters)


@pytest.mark.parametrize("mats,kw,R,want", [
    ([mat(64, 1024)], {}, 0, INVALID_ARGS),
    ([mat(64, 1024)], {}, 9, INVALID_ARGS),                       # from 8 rows up the MFMA tiles' order differs: not this entry's
    ([mat(64, 1024)], {"sparse": 1}, 4, INVALID_ARGS),
    ([mat(64, 1024, type=Q3)], {}, 4, UNSUPPORTED),               # the one-token plan's refusals, in its order
    ([mat(64, 1040)], {}, 4, INVALID_ARGS),
    ([mat(64, 1024), mat(64, 2048)], {}, 4, INVALID_ARGS),
    ([mat(64, 1024, awq=1, al=0)], {}, 4, UNSUPPORTED),
    ([mat(64, 1024, al=0)], {}, 4, UNALIGN),
    ([mat(64, 1024, gama=0)], {}, 4, QUANT_ERR),
    ([mat(64, 1024, lgroup=96)], {}, 4, QUANT_ERR),
    ([mat(64, 1024), mat(32, 1024)], {"mode": PAIRED}, 4, INVALID_ARGS),
    ([mat(64, 81800, type=BF16)], {}, 4, INVALID_ARGS),
])
def test_refusals(plans, mats, kw, R, want):
    assert plans(mats, R, **kw)[1].status == want
