"""The 3- / 2-bit row forms unpacked in registers (kf_set_row_unpack), without a GPU: the 4-bit twin the kernels are tested against holds the same weights bit for bit
in the oracle; kf::rowq_standin (through kfdbg_rowq_standin) plans a weight as the 4-bit row codebook of its shape and carries the shape rule in the stand-in's
alignment bits; the plans the existing rule gives the stand-in; the constants the Python side adds."""
import ctypes as C

import numpy as np
import pytest

import exact_inputs as E
import rowq_twin as T
from koifish_amd import lib as L
from oracle import oracle as O

OK, UNSUPPORTED, UNALIGN = 0, -1000, -2000
FMT_Q4R = 6
GM_DATA_AL, GM_TAB_AL = 1, 2


@pytest.mark.parametrize("kind", ["nf3", "lut2", "rtn2"])
@pytest.mark.parametrize("shape", [(8, 128), (40, 384), (256, 512), (64, 3072)])
def test_twin_holds_the_same_weights(kind, shape):
    m, k = shape
    ow = T.random_weight(np.random.default_rng(41), kind, m, k)
    tw = T.twin(ow)
    assert tw.bits == 4 and tw.data.size == m * k // 2 and tw.lut.shape == (m, 16)
    assert np.array_equal(O.dequant(tw), O.dequant(ow))
    n = 1 << ow.bits
    assert np.array_equal(tw.lut[:, :n], T.table_of(ow)) and (tw.lut[:, n:] == T.FILL).all()
    assert T.ids_of(ow).max() < n


def test_twin_canonical_outputs_are_those_of_the_original_values():
    """the canonical order of a 4-bit row codebook depends on the values and the shape alone: the twin's outputs are a function of the dequantised matrix"""
    rng = np.random.default_rng(42)
    m, k = 40, 384
    ow = T.random_weight(rng, "nf3", m, k)
    x = O.f32_to_bf16(rng.normal(0, 1.0, size=k).astype(np.float32))
    with O.canonical():
        y = O.linear(T.twin(ow), x)
    exact = O.bf16_to_f32(O.dequant(ow)).astype(np.float64).reshape(m, k) @ O.bf16_to_f32(x).astype(np.float64)
    assert np.abs(O.bf16_to_f32(y) - exact).max() <= 2.0 ** -8 * np.abs(exact).max() + 1e-6


def _standin(hip, type_, quant, m, k, data=0x10000, gama=0x20000, awq=False):
    hip.kfdbg_rowq_standin.argtypes = [C.POINTER(L.Weight), C.POINTER(C.c_int)]
    w = L.Weight(data, gama, type_, m, k, 0, 0, 0, 7, 0, 0x30000 if awq else None, 0x40000 if awq else None, quant, 0)
    out = (C.c_int * 8)()
    assert hip.kfdbg_rowq_standin(C.byref(w), out) == 0
    return dict(status=out[0], fmt=out[1], type=out[2], quant=out[3], M=out[4], K=out[5], gama=out[6], al=out[7])


def test_standin_is_the_four_bit_row_codebook_of_the_shape():
    hip = L.load()[0]
    for type_, quant, fmt in ((L.Q3, L.QUANT_ROW_LUT, L.FMT_Q3R), (L.Q2, L.QUANT_ROW_LUT, L.FMT_Q2R), (L.Q2, L.QUANT_ROW_RTN, L.FMT_Q2N)):
        s = _standin(hip, type_, quant, 64, 384)   # gama + (64 + 384) * 2 bytes: 16-byte aligned
        assert s == dict(status=OK, fmt=fmt, type=L.Q4, quant=L.QUANT_ROW_LUT, M=64, K=384, gama=1, al=GM_DATA_AL | GM_TAB_AL)
    assert (L.FMT_Q3R, L.FMT_Q2R, L.FMT_Q2N) == (9, 10, 11) and L.NF3 == 1001 and L.NF3 != L.NF4


def test_standin_refusals():
    hip = L.load()[0]
    # the shape rule rides in the data bit: K = 64, K = 192
    for k in (64, 192):
        s = _standin(hip, L.Q3, L.QUANT_ROW_LUT, 64, k)
        assert s["status"] == UNALIGN and not (s["al"] & GM_DATA_AL) and (s["al"] & GM_TAB_AL)
    # a table is aligned to its own size: 16 / 8 / 4 bytes.  ne0 + ne1 = 449 elements puts the tables at gama + 898 bytes
    for type_, quant, gama, want in ((L.Q3, L.QUANT_ROW_LUT, 0x20000, UNALIGN), (L.Q3, L.QUANT_ROW_LUT, 0x20000 + 14, OK), (L.Q3, L.QUANT_ROW_LUT, 0x20000 + 6, UNALIGN),
                                     (L.Q2, L.QUANT_ROW_LUT, 0x20000 + 6, OK), (L.Q2, L.QUANT_ROW_LUT, 0x20000 + 2, UNALIGN), (L.Q2, L.QUANT_ROW_RTN, 0x20000 + 2, OK),
                                     (L.Q2, L.QUANT_ROW_RTN, 0x20000, UNALIGN)):
        s = _standin(hip, type_, quant, 65, 384, gama=gama)
        assert s["status"] == want and bool(s["al"] & GM_TAB_AL) == (want == OK) and (s["al"] & GM_DATA_AL), (type_, quant, gama, s)
    assert _standin(hip, L.Q3, L.QUANT_ROW_LUT, 64, 384, data=0x10008)["status"] == UNALIGN
    assert _standin(hip, L.Q3, L.QUANT_ROW_LUT, 64, 384, gama=0)["status"] == UNALIGN
    # not a 3- / 2-bit row form, or the AutoAWQ layout
    assert _standin(hip, L.Q3, L.QUANT_ROW_LUT, 64, 384, awq=True)["status"] == UNSUPPORTED
    assert _standin(hip, L.Q4, L.QUANT_ROW_LUT, 64, 384) == dict(status=UNSUPPORTED, fmt=-1, type=0, quant=0, M=0, K=0, gama=0, al=0)
    assert _standin(hip, L.Q3, L.QUANT_ROW_RTN, 64, 384)["status"] == UNSUPPORTED
    assert _standin(hip, L.Q2, L.QUANT_GROUP, 64, 384)["status"] == UNSUPPORTED


def test_the_existing_rules_plan_the_standin():
    """no new planning rule: a runnable stand-in is storage "lut" of tests/exact_inputs.py to kf::gemm_plan, and a stand-in with a missing bit is refused by kf::gemv_plan
    with the code it has for a misaligned row codebook"""
    import test_gemv_plan_cpu as G
    hip = L.load()[0]
    hip.kfdbg_gemv_plan.argtypes = [C.POINTER(G.Problem), C.POINTER(G.Plan)]

    def gemv(al, K=384):
        P = G.Problem(mode=G.PLAIN, n_w=1, canon=1, q4_perm=1, q2_tab=1, q1_tab=1, xf2=1)
        P.w[0] = G.mat(64, K, type=G.Q4, quant=G.ROW_LUT, lgroup=0, al=al)
        out = G.Plan()
        assert hip.kfdbg_gemv_plan(C.byref(P), C.byref(out)) == 0
        return out
    p = gemv(3)
    assert (p.status, p.fmt, p.nBlk, p.lds) == (OK, FMT_Q4R, 12, 384 * 2 + 256)
    assert gemv(GM_TAB_AL).status == UNALIGN and gemv(GM_DATA_AL).status == UNALIGN
    assert E.forward_name(E.forward_plan(hip, "linear", "lut", [384], 512, 5)) == "MATVEC"
    assert E.forward_name(E.forward_plan(hip, "linear", "lut", [384], 512, 33)) == "TILE/DIRECT/32/q4r"
    assert E.forward_name(E.forward_plan(hip, "linear", "lut", [1312], 128, 1024)) == "TILE/STAGED/KS2/q4r"
    assert E.forward_name(E.forward_plan(hip, "linear", "lut", [8192], 128, 1024)) == "TILE/STAGED/KS1/q4r"


def test_kun_writer_round_trips_a_three_bit_normal_float_entry(tmp_path):
    """dtype "Q<3>": szData = ne0 ne1 3 / 8, gama = [R ne0][C ne1][LUT ne0 x 8] -- written and read back byte for byte by the host container code"""
    import json
    host = L.load()[1]
    host.kfh_st_open.restype = C.c_void_p
    rng = np.random.default_rng(43)
    ne0, ne1 = 64, 256
    ow = T.random_weight(rng, "nf3", ne0, ne1)
    blob = np.ascontiguousarray(T.blob(ow))
    szd, szg = ne0 * ne1 * 3 // 8, (ne0 + ne1 + 8 * ne0) * 2
    assert blob.size == szd + szg
    name = "model.layers.0.self_attn.q_proj.weight"
    config = {"vendor": "gruai", "CLI_params": {"config": {"quantizer": {"self_attn": {"quant_method": "NF", "bits": 3}}}}, "tokenizer": {"tokens": ""}}
    shape4 = np.array([[ne0, ne1, 0, 0]], np.int64)
    d, g = np.array([szd], np.uint64), np.array([szg], np.uint64)
    path = tmp_path / "q3.kun"
    rc = host.kfh_kun_write(str(path).encode(), 1, (C.c_char_p * 1)(name.encode()), (C.c_char_p * 1)(b"Q<3>"), C.c_void_p(shape4.ctypes.data), C.c_void_p(d.ctypes.data),
                            C.c_void_p(g.ctypes.data), (C.c_void_p * 1)(blob.ctypes.data), json.dumps(config).encode())
    assert rc == 0, host.kfh_last_error()
    h = C.c_void_p(host.kfh_st_open(str(path).encode(), 0))
    assert h
    nm, dt = C.create_string_buffer(256), C.create_string_buffer(16)
    sh = (C.c_int64 * 4)()
    nd, b, e = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    assert host.kfh_st_info(h, 0, nm, 256, dt, 16, sh, C.byref(nd), C.byref(b), C.byref(e)) == 0
    assert (nm.value.decode(), dt.value.decode(), tuple(sh[:nd.value]), e.value - b.value) == (name, "Q<3>", (ne0, ne1), szd + szg)
    dd, gg = C.c_uint64(0), C.c_uint64(0)
    assert host.kfh_st_blob_sizes(h, 0, C.byref(dd), C.byref(gg)) == 0 and (dd.value, gg.value) == (szd, szg)
    buf = (C.c_ubyte * (szd + szg))()
    assert host.kfh_st_read(h, name.encode(), buf, szd + szg) == 0 and bytes(buf) == blob.tobytes()
    host.kfh_st_close(h)
