"""The AutoAWQ layout's token-batch plan without a GPU (kf::gemm_plan through kfdbg_gemm_plan): the route stays GR_AWQ, and from AWQ_TILE_MIN rows the plan carries the
kf_gemm_awq.hip tiles -- family, form, grid, block and LDS as kf_gemm_plan.h awq_kern states them; below, unaligned, or with a shape the layout refuses: the mat-vec loop."""
import ctypes as C

import pytest

from koifish_amd import lib as L
from plan_structs import GemmMat as Mat, GemmPlan as Plan, GemmProblem as Problem

Q4, LINEAR, AWQ, NONE = 14, 0, 1, 0   # kf_dtype, GemmEntry, GemmRoute, GemmFamily
GK_AWQ = 6                      # appended to GemmFamily
AWQ_TILE_MIN, AWQ_WIDE_MIN = 16, 128
# AwqCfg: narrow 16 outputs x 32 tokens, stage = 128 rows x (2 + 2) words + 32 rows x (128 + 8) bf16; wide 256 x 128, stage = 64 x (32 + 2) words + 128 x (64 + 8) bf16
NARROW = dict(bo=16, bt=32, block=256, lds=2 * (128 * 4 * 4 + 32 * 136 * 2))
WIDE = dict(bo=256, bt=128, block=256, lds=2 * (64 * 34 * 4 + 128 * 72 * 2))


def cdiv(a, b):
    return -(-a // b)


def mat(M, K, type=Q4, lgroup=128, al=3, awq=1):
    return Mat(type, 0, awq, M, K, lgroup, 0, al)


def kern(p):
    return (p.k.fam, p.k.form, p.k.gx, p.k.gy, p.k.block, p.k.lds)


@pytest.fixture(scope="module")
def plan():
    hip = L.load()[0]
    hip.kfdbg_gemm_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]

    def f(entry, mats, n, x_al=1):
        P = Problem(entry=entry, n_w=len(mats), n=n, x_al=x_al, y_al=1)
        for i, m in enumerate(mats):
            P.w[i] = m
        out = Plan()
        assert hip.kfdbg_gemm_plan(C.byref(P), C.byref(out)) == 0
        return out
    return f


@pytest.mark.parametrize("M,K,n,f", [(1024, 1024, AWQ_TILE_MIN, NARROW), (1024, 1024, 64, NARROW), (1024, 1024, AWQ_WIDE_MIN - 1, NARROW), (1024, 1024, AWQ_WIDE_MIN, WIDE),
                                     (1024, 1024, 2047, WIDE), (200, 384, 33, NARROW), (3072, 1024, 129, WIDE)])
def test_batches_plan_the_tiles(plan, M, K, n, f):
    p = plan(LINEAR, [mat(M, K, awq=1)], n)
    assert p.route == AWQ and p.status == 0 and p.deq == 0 and p.deq_bytes == 0 and p.ws_bytes == 0
    assert kern(p) == (GK_AWQ, f["bt"], cdiv(M, f["bo"]), cdiv(n, f["bt"]), f["block"], f["lds"])
    assert f["lds"] <= 160 * 1024


@pytest.mark.parametrize("n,kw,mkw", [(1, {}, {}), (8, {}, {}), (AWQ_TILE_MIN - 1, {}, {}), (64, dict(x_al=0), {}), (64, {}, dict(al=0)), (64, {}, dict(lgroup=64)),
                                      (64, {}, dict(type=17)), (64, {}, dict(M=1020)), (64, {}, dict(K=1088)), (64, {}, dict(K=64))])
def test_the_mat_vec_loop_keeps_the_rest(plan, n, kw, mkw):
    p = plan(LINEAR, [mat(**dict(dict(M=1024, K=1024), **mkw))], n, **kw)   # n, alignment, and the shapes the layout refuses
    assert p.route == AWQ and p.k.fam == NONE
