"""kf_linear_backward's plan without a GPU: kf::linear_bwd_plan (through kfdbg_linear_backward_plan) decides which shapes are served, where the regions of the scratch lie,
the plan of each wanted product and where the W operand comes from (csrc/kf_linear_bwd_plan.h).  Pinned here: the scratch query's values (they size every trainer's
scratch), the regions, the products against kf::gemm_plan, each refusal on both sides of its rule, and that no served shape of a grid lacks a tile kernel."""
import ctypes as C
import itertools

import pytest

from koifish_amd import lib as L
from plan_structs import GemmMat as Mat, GemmPlan, GemmProblem, LinearBwdPlan as Plan, LinearBwdProblem as Problem

BF16, Q4 = 3, 14                                          # kf_dtype
BWD_DX, BWD_DW = 4, 5                                     # GemmEntry
KMAJOR, TRANSPOSE = 11, 12                                # GemmRoute
GK_NONE = 0
OK, INVALID_ARGS, UNSUPPORTED_DATATYPE = 0, -20, -1000    # kf_abi.h
NONE, AWQ, NOTHING, SHAPE, DX_UNCOVERED, DW_UNCOVERED = range(6)   # LinearBwdRefusal
STORED, DEQUANT, COPY = range(3)                          # LBW_*
SK_BYTES = 256 * 256 * 256 * 4 + 8192                     # gemm3_sk_ws_bytes(): a multiple of 256


def up256(v):
    return (v + 255) & ~255


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def plan(hip):
    hip.kfdbg_linear_backward_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]

    def f(OC, IC, n, delta=1, gw=1, bias=1, type=BF16, awq=0):
        out = Plan()
        assert hip.kfdbg_linear_backward_plan(C.byref(Problem(Mat(type, 0, awq, OC, IC, 128, int(type != BF16), 3), n, delta, gw, bias)), C.byref(out)) == 0
        return out
    return f


@pytest.fixture(scope="module")
def product(hip):
    hip.kfdbg_gemm_plan.argtypes = [C.POINTER(GemmProblem), C.POINTER(GemmPlan)]

    def f(entry, OC, IC, n, scratch):
        P = GemmProblem(entry=entry, n_w=1, n=n, x_al=1, scratch=scratch)
        P.w[0] = Mat(BF16, 0, 0, OC, IC, 128, 0, 3)
        out = GemmPlan()
        assert hip.kfdbg_gemm_plan(C.byref(P), C.byref(out)) == 0
        return out
    return f


def fields(s):
    """every field of a ctypes struct, nested structs included, as a flat tuple"""
    return tuple(x for f, _ in s._fields_ for x in (fields(getattr(s, f)) if isinstance(getattr(s, f), C.Structure) else (getattr(s, f),)))


# ---- the scratch query: the values of the commit before the plan existed (its library, asked on the CPU).  The middle region is the three transposed copies for
# (50304, 1600, 8192) and (4096, 4096, 8192), the split-K workspace for the others
SCRATCH = {
    (256, 128, 128): 67184640, (1024, 3072, 128): 73416704, (4800, 1600, 192): 82515456, (1600, 6400, 320): 87622656, (1024, 1024, 1024): 69246976,
    (1600, 1600, 2048): 72339456, (2048, 2056, 2048): 75669504, (1600, 1600, 8192): 72646656, (50304, 1600, 8192): 1185218560, (512, 1024, 96): 68169728,
    (128, 128, 96): 67150848, (4096, 4096, 8192): 202375168,
}


@pytest.mark.parametrize("shape", SCRATCH)
def test_scratch_query_unchanged(hip, plan, shape):
    assert hip.kf_linear_backward_scratch_bytes(*shape) == SCRATCH[shape]
    for wants in ((1, 1, 1), (1, 0, 0), (0, 0, 1)):      # the scratch does not depend on the outputs wanted, nor on a refusal for the shape
        assert plan(*shape, *wants).bytes == SCRATCH[shape]


def test_scratch_query_empty(hip):
    for shape in ((0, 128, 128), (128, 0, 128), (128, 128, 0), (-64, 128, 128)):
        assert hip.kf_linear_backward_scratch_bytes(*shape) == 0


@pytest.mark.parametrize("shape", SCRATCH)
def test_regions(plan, shape):
    """[W bf16] [middle] [bias slabs], the middle holding [W^T] [deltaIn^T] [inp^T] or the split-K slots: ascending, 256-byte aligned, disjoint, ending at `bytes`"""
    OC, IC, n = shape
    p = plan(OC, IC, n)
    regions = [(0, OC * IC * 2), (p.off_mid, OC * IC * 2), (p.off_dInT, OC * n * 2), (p.off_inpT, IC * n * 2), (p.off_slabs, (n + 255) // 256 * OC * 8)]
    for (a, a_len), (b, _) in zip(regions, regions[1:]):
        assert a % 256 == 0 and b % 256 == 0 and a + a_len <= b
    assert p.off_inpT + IC * n * 2 <= p.off_mid + p.mid_bytes == p.off_slabs                  # the copies lie inside the middle, the slabs right behind it
    assert p.mid_bytes % 256 == 0 and p.mid_bytes >= up256(SK_BYTES)                          # and so do the split-K slots
    assert p.mid_bytes == max(up256(SK_BYTES), up256(OC * IC * 2) + up256(OC * n * 2) + up256(IC * n * 2))
    assert p.bytes == p.off_slabs + up256(regions[-1][1])


def test_middle_is_the_larger_use(plan):
    assert plan(1600, 1600, 8192).mid_bytes == up256(SK_BYTES)                                 # 57.5 MB of transposed copies < the 64 MiB of split-K slots
    assert plan(4096, 4096, 8192).mid_bytes == 4096 * 4096 * 2 + 2 * 4096 * 8192 * 2 > up256(SK_BYTES)


# ---- the products: kf::gemm_plan's, with the middle region lent.  The shapes of test_gemm_plan_cpu.py's test_backward_kmajor / test_backward_transpose
PRODUCT_SHAPES = [(1024, 1024, 2048), (4096, 4096, 8192), (1024, 3072, 4096), (1024, 2048, 3584), (1024, 2048, 3328), (1024, 1024, 128), (128, 1024, 2048), (1024, 200, 2048)]


@pytest.mark.parametrize("shape", PRODUCT_SHAPES)
def test_products(plan, product, shape):
    p = plan(*shape)
    assert (p.status, p.refusal) == (OK, NONE)
    assert fields(p.dx) == fields(product(BWD_DX, *shape, p.mid_bytes))
    assert fields(p.dw) == fields(product(BWD_DW, *shape, p.mid_bytes))
    q = plan(*shape, gw=0)                                # a product that is not wanted is not planned
    assert fields(q.dx) == fields(p.dx) and fields(q.dw) == fields(GemmPlan())
    assert fields(plan(*shape, delta=0).dx) == fields(GemmPlan())


def test_w_operand(plan):
    """the stored bf16 as it lies on the k-major route; a quantised weight's dequantised copy on either route; the transpose route's copy of a bf16 weight"""
    assert (plan(1024, 1024, 2048).dx.route, plan(1024, 1024, 2048).w_from) == (KMAJOR, STORED)
    assert (plan(1024, 1024, 128).dx.route, plan(1024, 1024, 128).w_from) == (TRANSPOSE, COPY)
    assert plan(1024, 1024, 2048, type=Q4).w_from == DEQUANT and plan(1024, 1024, 128, type=Q4).w_from == DEQUANT
    assert plan(1024, 1024, 128, delta=0).w_from == STORED and plan(1024, 1024, 128, delta=0, type=Q4).w_from == STORED   # no input gradient: W is not read


# ---- the refusals, on each side of each rule
@pytest.mark.parametrize("OC,IC,n,wants,want", [
    (96, 128, 128, (1, 1, 1), (INVALID_ARGS, SHAPE)),      # OC: a multiple of 64 from 128
    (64, 128, 128, (1, 1, 1), (INVALID_ARGS, SHAPE)),
    (128, 128, 128, (1, 1, 1), (OK, NONE)),
    (160, 128, 128, (1, 1, 1), (INVALID_ARGS, SHAPE)),
    (192, 128, 128, (1, 1, 1), (OK, NONE)),
    (128, 12, 128, (1, 1, 1), (INVALID_ARGS, SHAPE)),      # IC: a multiple of 8
    (128, 16, 128, (1, 1, 1), (OK, NONE)),
    (128, 128, 96, (1, 1, 1), (INVALID_ARGS, SHAPE)),      # n: a multiple of 64 from 128, for the weight gradient only
    (128, 128, 96, (0, 1, 0), (INVALID_ARGS, SHAPE)),
    (128, 128, 64, (1, 1, 1), (INVALID_ARGS, SHAPE)),
    (128, 128, 96, (1, 0, 1), (OK, NONE)),
    (512, 1024, 96, (1, 0, 0), (OK, NONE)),
    (128, 128, 1, (1, 0, 0), (OK, NONE)),
    (128, 128, 128, (1, 1, 1), (OK, NONE)),
    (128, 128, 0, (1, 0, 0), (INVALID_ARGS, SHAPE)),
    (128, 128, 128, (0, 0, 0), (INVALID_ARGS, NOTHING)),   # nothing to compute
    (128, 128, 128, (0, 0, 1), (OK, NONE)),                # the bias gradient alone
])
def test_refusals(plan, OC, IC, n, wants, want):
    p = plan(OC, IC, n, *wants)
    assert (p.status, p.refusal) == want


def test_awq_refused(plan):
    for shape in ((1024, 1024, 128), (96, 128, 128), (128, 128, 0)):   # whatever else is wrong: the entry said so first
        p = plan(*shape, type=Q4, awq=1)
        assert (p.status, p.refusal) == (UNSUPPORTED_DATATYPE, AWQ)


def test_every_served_shape_is_covered(plan):
    """the refusal "no tile kernel covers the product" is a status before any launch now; on this grid no shape that passes the shape rules meets it"""
    served = 0
    for OC, IC, n, gw in itertools.product(range(128, 1025, 64), (8, 16, 24, 64, 200, 1024), (1, 8, 96, 128, 192, 2048), (0, 1)):
        p = plan(OC, IC, n, gw=gw)
        if gw and n in (1, 8, 96):
            assert (p.status, p.refusal) == (INVALID_ARGS, SHAPE)
            continue
        assert (p.status, p.refusal) == (OK, NONE), (OC, IC, n, gw)
        assert p.dx.k.fam != GK_NONE and (not gw or p.dw.k.fam != GK_NONE), (OC, IC, n, gw)
        served += 1
    assert served == 15 * 6 * (6 + 3)
