"""The e4m3 block-scaled storage (include/kf_abi.h "FP8 block-scaled layers") without a GPU: its layout and card through kfh_weight_layout / kfh_quant_card against
literal sizes, and the refusals of the entries that serve it, each by its code, before anything is launched (no context exists here: a served weight would reach the
context check, a refused one never does)."""
import ctypes as C

import pytest

from koifish_amd import lib as L
from koifish_amd import runtime as R

KF_INVALID_ARGS, KF_QUANT_ERR, KF_UNSUPPORTED_DATATYPE, KF_BLAS_UNALIGN = -20, -701, -1000, -2000


@pytest.mark.parametrize("ne0,ne1,sizes", [(16, 128, (2048, 4, 1)), (144, 256, (36864, 16, 4)), (1024, 1024, (1048576, 256, 64))])
def test_layout_and_card(ne0, ne1, sizes):
    """a byte per weight, then one fp32 scale per 128 x 128 block; a last scale row may cover fewer than 128 rows (144 = 128 + 16)"""
    assert R.weight_layout(L.F8E4M3, ne0, ne1, 128) == sizes
    assert R.F8BlockDevWeight.blob_bytes(ne0, ne1) == sizes[0] + sizes[1]
    v = (C.c_int * 4)()
    assert L.load()[1].kfh_quant_card(L.F8E4M3, 0, 0, v) == 0 and tuple(v) == (8, 0, 0, 0)


def weight(ne0=16, ne1=128, qzeros=False, qscales=True, lGroup=128, quant=0):
    buf = (C.c_uint8 * 64)()
    p = (C.addressof(buf) + 15) & ~15
    return buf, L.Weight(p, None, L.F8E4M3, ne0, ne1, 1, lGroup, 0, 0, 0, p if qzeros else None, p + 16 if qscales else None, quant, 0)


REFUSED = [
    ("ne1 = 192", dict(ne1=192), KF_BLAS_UNALIGN, "in % 128 == 0"),
    ("ne0 = 24", dict(ne0=24), KF_BLAS_UNALIGN, "out % 16 == 0"),
    ("no qscales", dict(qscales=False), KF_QUANT_ERR, "without qscales"),
    ("qzeros and qscales", dict(qzeros=True), KF_QUANT_ERR, "AutoAWQ"),
    ("group 64", dict(lGroup=64), KF_QUANT_ERR, "lGroup = 128"),
]


@pytest.mark.parametrize("name,kw,code,why", REFUSED, ids=[r[0] for r in REFUSED])
def test_entries_refuse_by_code_before_any_launch(name, kw, code, why):
    hip = L.load()[0]
    keep, w = weight(**kw)
    fake = C.c_void_p(64)   # never dereferenced: the storage is judged first; only a SERVED weight goes on to the context check
    wp, yp = (C.c_void_p * 1)(C.addressof(w)), (C.c_void_p * 1)(64)
    calls = [lambda: hip.kf_linear(None, C.byref(w), fake, fake, None, 1, 1.0, 0.0, 0, None), lambda: hip.kf_dequant(None, C.byref(w), fake),
             lambda: hip.kf_quantize(None, C.byref(w), fake, 0), lambda: hip.kf_norm_linear(None, fake, None, 1e-6, 1, wp, yp, None, 0, None),
             lambda: hip.kf_norm_gateup_swiglu(None, fake, None, 1e-6, C.byref(w), C.byref(w), fake)]
    for call in calls:
        assert call() == code and why in hip.kf_last_error().decode()
    del keep


def test_a_served_weight_reaches_the_context_check_and_needs_no_scratch():
    hip = L.load()[0]
    keep, w = weight()
    fake = C.c_void_p(64)
    assert hip.kf_linear(None, C.byref(w), fake, fake, None, 1, 1.0, 0.0, 0, None) == KF_INVALID_ARGS and "null kf_ctx" in hip.kf_last_error().decode()
    assert hip.kf_linear_scratch_bytes(C.byref(w), 64) == 0
    del keep
