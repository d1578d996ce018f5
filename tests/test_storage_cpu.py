"""The storage rule (koifish_amd/host/kf_storage.hpp) and the parameter table (kf_params.hpp) without a GPU.

kfh_weight_layout / kfh_quant_card -- what every loader and runtime.py's weight classes size a blob by -- against sizes and cards written out here as literals, every
refusal included; kfhdbg_param_table against lists written out here; and tests/storage_main.cpp, the two headers alone as a program under AddressSanitizer + UBSan
(the sanitizer runtimes linked in, nothing preloaded)."""
import ctypes as C
import os
import subprocess

import pytest

from koifish_amd import lib as L
from koifish_amd import runtime as R

HERE = os.path.dirname(os.path.abspath(__file__))
KF_INVALID_ARGS, KF_QUANT_ERR, KF_UNSUPPORTED_DATATYPE, KF_BLAS_UNALIGN = -20, -701, -1000, -2000


def layout(type_, ne0, ne1, group=128, nf=0, sym=0, rtn=0):
    host = L.load()[1]
    d, g, n = C.c_uint64(7), C.c_uint64(7), C.c_int64(7)
    rc = host.kfh_weight_layout(type_, ne0, ne1, group, nf, sym, rtn, C.byref(d), C.byref(g), C.byref(n))
    return rc, d.value, g.value, n.value, host.kfh_host_error().decode()


def card(type_, sym=0, nf=0):
    v = (C.c_int * 4)()
    assert L.load()[1].kfh_quant_card(type_, sym, nf, v) == 0
    return tuple(v)


# (type, ne0, ne1, group, normal-float, symmetric, row-RTN) -> (szData, szGama, nGroup), (bits, qMin, qMax, qBias)
SERVED = [
    ("bf16", (L.BF16, 8, 32, 128, 0, 0, 0), (512, 0, 0), (16, 0, 0, 0)),
    ("f8", (L.F8E5M2, 8, 32, 128, 0, 0, 0), (256, 0, 0), (8, 0, 0, 0)),
    ("q4 8x128", (L.Q4, 8, 128, 128, 0, 0, 0), (512, 304, 8), (4, 0, 15, 0)),
    ("q4 16x256", (L.Q4, 16, 256, 128, 0, 0, 0), (2048, 672, 32), (4, 0, 15, 0)),
    ("q4 symmetric", (L.Q4, 8, 128, 128, 0, 1, 0), (512, 304, 8), (4, -8, 7, 8)),
    ("ternary", (L.T_SIGN, 8, 128, 128, 0, 0, 0), (256, 304, 8), (2, -1, 1, 1)),
    ("binary", (L.T_BINARY, 8, 128, 128, 0, 0, 0), (128, 304, 8), (1, 0, 1, 0)),
    ("bool1", (L.BOOL1, 8, 128, 128, 0, 0, 0), (128, 304, 8), (1, 0, 1, 0)),
    ("nf4", (L.Q4, 8, 32, 0, 1, 0, 0), (128, 336, 0), (4, 0, 15, 0)),
    ("nf3", (L.Q3, 8, 128, 0, 1, 0, 0), (384, 400, 0), (3, 0, 7, 0)),
    ("2-bit row lut", (L.Q2, 8, 128, 0, 1, 0, 0), (256, 336, 0), (2, 0, 3, 0)),
    ("2-bit row rtn", (L.Q2, 8, 128, 0, 1, 0, 1), (256, 304, 0), (2, 0, 3, 0)),
]


@pytest.mark.parametrize("name,args,sizes,want_card", SERVED, ids=[s[0] for s in SERVED])
def test_layout_and_card_of_every_served_form(name, args, sizes, want_card):
    rc, d, g, n, _ = layout(*args)
    assert (rc, d, g, n) == (0,) + sizes
    assert card(args[0], args[5], args[4]) == want_card


# 8 x 96 in groups of 128 divides (768 = 6 x 128): the refusal is n % lGroup != 0, shown by 8 x 40 in groups of 128 and by 8 x 96 in groups of 512
REFUSED = [
    ("group 0", (L.Q4, 8, 128, 0), KF_QUANT_ERR),
    ("group 0, ternary", (L.T_SIGN, 8, 128, 0), KF_QUANT_ERR),
    ("8x40 group 128", (L.Q4, 8, 40, 128), KF_QUANT_ERR),
    ("8x96 group 512", (L.Q4, 8, 96, 512), KF_QUANT_ERR),
    ("q3 in groups", (L.Q3, 8, 128, 128), KF_UNSUPPORTED_DATATYPE),
    ("f32", (L.F32, 8, 32, 128), KF_UNSUPPORTED_DATATYPE),
    ("no such type", (77, 8, 32, 128), KF_UNSUPPORTED_DATATYPE),
    ("row rtn at 4 bits", (L.Q4, 8, 32, 0, 1, 0, 1), KF_UNSUPPORTED_DATATYPE),
    ("ne0 = 0", (L.BF16, 0, 32, 128), KF_INVALID_ARGS),
    ("bf16 overflow", (L.BF16, 1 << 40, 1 << 40, 128), KF_INVALID_ARGS),
    ("q4 n * bits overflow", (L.Q4, 1 << 31, 1 << 31, 128), KF_INVALID_ARGS),
    ("nf4 overflow", (L.Q4, (1 << 63) - 8, 32, 0, 1), KF_INVALID_ARGS),
]


@pytest.mark.parametrize("name,args,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_layout_refusals(name, args, code):
    rc, d, g, n, why = layout(*args)
    assert rc == code and (d, g, n) == (0, 0, 0) and why.startswith("kfh_weight_layout: ")


@pytest.mark.parametrize("type_,ne0,ne1,sizes", [(L.Q4, 8, 48, (192, 368)), (L.Q4, 12, 32, (192, 472)), (L.Q3, 8, 64, (192, 272))], ids=["nf4 ne1=48", "nf4 ne0=12", "nf3 ne1=64"])
def test_row_shape_refusals_keep_their_sizes(type_, ne0, ne1, sizes):
    """the decode path does not multiply such a stream (each loader answers with its own code); the operators do, so the sizes stand"""
    rc, d, g, n, why = layout(type_, ne0, ne1, 0, 1)
    assert rc == KF_BLAS_UNALIGN and (d, g, n) == sizes + (0,) and "row form needs" in why
    assert R.weight_layout(type_, ne0, ne1, normal_float=True)[:2] == sizes


def test_python_weight_classes_ask_the_library():
    assert R.DevWeight.blob_bytes(L.Q4, 16, 256) == 2048 + 672 and R.DevWeight.blob_bytes(L.BF16, 8, 32) == 512 and R.DevWeight.blob_bytes(L.T_SIGN, 8, 128, 64) == 256 + 336
    assert R.LutDevWeight.blob_bytes(8, 32) == 128 + 336 and R.LutDevWeight.blob_bytes(8, 128, 3) == 384 + 400 and R.LutDevWeight.blob_bytes(8, 128, 2) == 256 + 336
    assert R.quant_range(L.Q4) == (0, 15, 0) and R.quant_range(L.Q4, True) == (-8, 7, 8) and R.quant_range(L.T_SIGN) == (-1, 1, 1) and R.quant_range(L.BF16) == (0, 0, 0)
    with pytest.raises(L.KFError, match="group size 0"):
        R.DevWeight.blob_bytes(L.Q4, 8, 128, 0)


def table(qk_norm, tied, n_layer=2):
    host = L.load()[1]
    buf = C.create_string_buffer(1 << 14)
    need = host.kfhdbg_param_table(256, n_layer, 4, 2, 64, 512, 512, int(qk_norm), int(tied), buf, len(buf))
    assert 0 < need <= len(buf)
    return [tuple(ln.split()[:1] + ln.split()[1:2] + [int(x) for x in ln.split()[2:]]) for ln in buf.value.decode().splitlines()]


def layer_rows(l, qk_norm):
    p = "model.layers.%d." % l
    rows = [(p + "input_layernorm.weight", "norm", l, 0, 256, 1, 1),
            (p + "self_attn.q_proj.weight", "matrix", l, 0, 256, 256, 1),
            (p + "self_attn.k_proj.weight", "matrix", l, 1, 128, 256, 1),
            (p + "self_attn.v_proj.weight", "matrix", l, 2, 128, 256, 1),
            (p + "self_attn.q_norm.weight", "norm", l, 2, 64, 1, 0),
            (p + "self_attn.k_norm.weight", "norm", l, 3, 64, 1, 0),
            (p + "self_attn.o_proj.weight", "matrix", l, 3, 256, 256, 1),
            (p + "post_attention_layernorm.weight", "norm", l, 1, 256, 1, 1),
            (p + "mlp.gate_proj.weight", "matrix", l, 4, 512, 256, 1),
            (p + "mlp.up_proj.weight", "matrix", l, 5, 512, 256, 1),
            (p + "mlp.down_proj.weight", "matrix", l, 6, 256, 512, 1)]
    return rows if qk_norm else rows[:4] + rows[6:]


@pytest.mark.parametrize("qk_norm", [True, False])
@pytest.mark.parametrize("tied", [True, False])
def test_parameter_table_names_order_slots_and_shapes(qk_norm, tied):
    """the order is a .kun file's tensor order: embedding, the layers, the final norm, the head (when it is a tensor of its own)"""
    want = [("model.embed_tokens.weight", "embed", -1, 0, 512, 256, 1)] + layer_rows(0, qk_norm) + layer_rows(1, qk_norm) + [("model.norm.weight", "norm", -1, 0, 256, 1, 1)]
    if not tied:
        want.append(("lm_head.weight", "head", -1, 1, 512, 256, 0))
    assert table(qk_norm, tied) == want


def test_storage_headers_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "storage_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(HERE, "storage_main.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert " 0 failed" in run.stdout and "ERROR" not in run.stdout and "runtime error" not in run.stdout, run.stdout
