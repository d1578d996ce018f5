"""The ctypes mirror of kf::A8Problem / kf::A8Plan (csrc/kf_a8.h; kf::GemmMat: plan_structs.py) and the call of kfdbg_a8_route_plan, once, for every test of the int8-activation products."""
import ctypes as C

from koifish_amd import lib as L
from plan_structs import GemmMat as Mat

BF16, F8, Q4, Q3, Q2, T_SIGN, BOOL1, T_BINARY = 3, 4, 14, 15, 16, 17, 19, 20   # kf_dtype
GROUP, ROW_LUT, ROW_RTN = 0, 1, 2                                              # quant forms
OK, INVALID_ARGS, QUANT_ERR, UNSUPPORTED, UNALIGN = 0, -20, -701, -1000, -2000
ORDER_CHAIN, TOK_TILE, GROUP_LDS, LDS_MAX, TILE_MIN = 1, 4, 144, 160 * 1024, 32   # kf_a8.h; TILE_MIN = KF_A8_TILE_MIN (include/kf_abi.h)
LOWBIT, Q4_FAMILY = 1, 2                                                       # A8Plan::family
MATVEC, TILES = 0, 1                                                           # A8Problem::route


class Problem(C.Structure):   # kf::A8Problem
    _fields_ = [("w", Mat), ("nTok", C.c_int), ("qbias", C.c_int), ("route", C.c_int)]


class Plan(C.Structure):   # kf::A8Plan
    _fields_ = [(f, C.c_int) for f in ("status", "family", "route", "bits", "qbias", "order", "n_groups", "lpr_log2", "iters", "rows_per_wave", "rows_per_wg", "tok_tiles",
                                       "row_tile", "waves", "mfma_tok", "chunk", "min_tok", "tok_tile", "grid_x", "grid_y", "block", "lds")]


MATVEC_FIELDS = ("lpr_log2", "iters", "rows_per_wave", "rows_per_wg", "tok_tiles")   # A8Plan: the figures only the mat-vec route fills
TILE_FIELDS = ("row_tile", "waves", "mfma_tok", "chunk")                              # ... and only the tile route


def mat(M, K, type=T_SIGN, quant=GROUP, lgroup=128, gama=1, al=3, awq=0):
    return Mat(type, quant, awq, M, K, lgroup, gama, al)


def plan(family, route, m, nTok=1, qbias=0):
    """kf::a8_plan's answer for one route, as an entry of `family` takes it: the other family's storage has no form there, whatever else is wrong with it (kf_abi.hip
    a8_entry_plan; the status entries pin that: test_status_entry, test_status_entries)"""
    hip = L.load()[0]
    hip.kfdbg_a8_route_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]
    out = Plan()
    assert hip.kfdbg_a8_route_plan(C.byref(Problem(m, nTok, qbias, route)), C.byref(out)) == 0 and out.route == route
    assert out.status == OK or not any(getattr(out, f) for f, _ in Plan._fields_ if f not in ("status", "family", "route", "min_tok"))   # a refusal carries no figure
    assert not any(getattr(out, f) for f in (TILE_FIELDS if route == MATVEC else MATVEC_FIELDS)) and out.min_tok == (TILE_MIN if route == TILES else 0)   # nor the other route's
    assert out.status != OK or (out.family, out.bits) in ((LOWBIT, 2 if m.type == T_SIGN else 1), (Q4_FAMILY, 4))
    return out if out.family == family else Plan(status=UNSUPPORTED)


def weight_tile_plan(dw, n):
    """the tile plan of a device weight (runtime.Weight) at n token rows"""
    family = Q4_FAMILY if dw.type == L.Q4 else LOWBIT
    out = plan(family, TILES, Mat(dw.type, 0, 0, dw.ne0, dw.ne1, 128, 1, 3), n, dw.qBias)
    assert out.status == OK
    return out


def check_views():
    """the four per-entry exports of earlier versions (kfdbg_a8_plan, kfdbg_a8_tile_plan, kfdbg_w4a8_plan, kfdbg_w4a8_tile_plan) are views of the one plan: a route's figures,
    in their old layouts -- second word `bits` (low-bit) or `qbias` (q4); the low-bit problem ends at nTok"""
    hip = L.load()[0]
    head = ("order", "n_groups")
    mv = head + ("lpr_log2", "iters", "rows_per_wave", "rows_per_wg", "tok_tile", "tok_tiles", "grid_x", "grid_y", "block", "lds")
    tl = head + ("row_tile", "tok_tile", "waves", "mfma_tok", "chunk", "grid_x", "grid_y", "block", "lds", "min_tok")
    for name, family, route, fields in (("kfdbg_a8_plan", LOWBIT, MATVEC, mv), ("kfdbg_a8_tile_plan", LOWBIT, TILES, tl), ("kfdbg_w4a8_plan", Q4_FAMILY, MATVEC, mv),
                                        ("kfdbg_w4a8_tile_plan", Q4_FAMILY, TILES, tl)):
        for m, n, qb in ((mat(1000, 1280, T_SIGN), 70, 0), (mat(64, 384, BOOL1), 1, 0), (mat(1000, 1280, Q4), 500, 8), (mat(64, 1024, Q4), 1, 3), (mat(8, 36480), 2, 0), (mat(8, 64, Q4), 1, 0)):
            want, got = plan(family, route, m, n, qb), (C.c_int * 14)(*([-1] * 14))
            getattr(hip, name).argtypes, getattr(hip, name).restype = None, C.c_int
            assert getattr(hip, name)(C.byref(Problem(m, n, qb, -1)), got) == 0   # the views read no route, and the low-bit ones no qbias
            second = (want.qbias if family == Q4_FAMILY else want.bits) if want.status == OK else 0
            assert list(got) == [want.status, second] + [TILE_MIN if f == "min_tok" else getattr(want, f) if want.status == OK else 0 for f in fields], (name, list(got))
