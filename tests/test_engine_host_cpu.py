"""The host rules both decode-engine families state once (csrc/kf_engine_host.h), without a GPU: which heads and embedding tables the in-launch phases take
(kfdbg_engine_operand_rule) and what a build answers for a descriptor, with its reason (kfdbg_engine_desc_refusal: every check of create except the device's CU count, in
create's order).  No device pointer is dereferenced: the addresses below are made up, aligned as the rules ask."""
import ctypes as C

import pytest

from koifish_amd import lib as L
from plan_structs import EngineDesc, EngineLayer

OK, INVALID_ARGS, UNSUPPORTED = 0, -20, -1000   # kf_abi.h
PERSISTENT, XCD = 0, 1
HEAD, EMBEDDING = 0, 1
ADDR = 0x7f0000001000   # "device" addresses: never read


@pytest.fixture(scope="module")
def hip():
    h = L.load()[0]
    h.kfdbg_engine_operand_rule.argtypes = [C.c_int, C.POINTER(L.Weight), C.c_int, C.c_int]
    h.kfdbg_engine_desc_refusal.argtypes = [C.c_int, C.POINTER(EngineDesc), C.c_int, C.c_char_p, C.c_size_t]
    return h


def weight(ne0, ne1, type_=L.BF16, lGroup=128, data=ADDR, **kw):
    w = L.Weight(data=data, gama=None if type_ == L.BF16 else ADDR + 0x100000, type=type_, ne0=ne0, ne1=ne1, nGroup=ne0 * ne1 // lGroup, lGroup=lGroup, qBias=0 if type_ == L.BF16 else 8,
                 quant=L.QUANT_GROUP)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


# ---- operands
def operand(hip, kind, w, dim, given=True):
    return hip.kfdbg_engine_operand_rule(kind, C.byref(w), dim, int(given))


def test_head_rule_at_dim_1024(hip):
    assert operand(hip, HEAD, weight(151936, 1024), 1024) == OK
    assert operand(hip, HEAD, weight(64, 1024), 1024) == OK
    refused = [weight(151936, 1024, type_=L.Q4), weight(151936, 1024, quant=L.QUANT_ROW_LUT), weight(151936, 1024, qzeros=ADDR), weight(151936, 2048),
               weight(151936, 1024, data=None), weight(151936, 1024, data=ADDR + 8), weight(63, 1024)]
    for w in refused:
        assert operand(hip, HEAD, w, 1024) == UNSUPPORTED, (w.type, w.quant, w.qzeros, w.ne0, w.ne1, w.data)
    assert operand(hip, HEAD, weight(151936, 1024), 1024, given=False) == UNSUPPORTED


def test_head_rule_lanes_per_row_clause(hip):
    """gemv_lpr_log2(8, 192, rows) is 5 up to 4095 rows and 4 from 4096 on (the head phases are compiled for the long-matrix figure); at the widths of the served models
    it does not depend on the rows, so 192 is the smallest width at which the clause decides"""
    assert operand(hip, HEAD, weight(4095, 192), 192) == UNSUPPORTED
    assert operand(hip, HEAD, weight(4096, 192), 192) == OK
    for dim in (256, 1024, 2048, 2560, 4096, 5120):
        assert operand(hip, HEAD, weight(64, dim), dim) == OK


def test_embedding_rule(hip):
    assert operand(hip, EMBEDDING, weight(151936, 1024), 1024) == OK
    assert operand(hip, EMBEDDING, weight(151936, 2048), 1024) == UNSUPPORTED
    assert operand(hip, EMBEDDING, weight(151936, 1024, type_=L.Q4), 1024) == UNSUPPORTED
    assert operand(hip, EMBEDDING, weight(151936, 1024, data=None), 1024) == UNSUPPORTED


# ---- descriptors
SMALL = dict(dim=256, n_head=4, n_kv=2, head_dim=64, ffn=512)       # the 256-wide test shape
QWEN3_4B = dict(dim=2560, n_head=32, n_kv=8, head_dim=128, ffn=9728)


def desc(shape=SMALL, n_layer=2, type_=L.Q4, lGroup=128, **kw):
    """a descriptor of 4-bit layers in groups of 128 (every matrix the same made-up addresses)"""
    hd, dim, ffn = shape["head_dim"], shape["dim"], shape["ffn"]
    qd, kvd = shape["n_head"] * hd, shape["n_kv"] * hd
    layers = (EngineLayer * n_layer)()
    for ly in layers:
        for j, (m, k) in enumerate(((qd, dim), (kvd, dim), (kvd, dim), (dim, qd), (ffn, dim), (ffn, dim), (dim, ffn))):
            ly.w[j] = weight(m, k, type_, lGroup)
        ly.norm_in = ly.norm_post = ly.q_norm = ly.k_norm = ADDR
        ly.kcache, ly.vcache = ADDR + 0x200000, ADDR + 0x300000
    d = EngineDesc(n_layer=n_layer, kv_stride=kvd, max_seq=64, rms_eps=1e-6, qk_eps=1e-6, rope_table=ADDR, layers=layers, **shape)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def refusal(hip, family, d, n_seq=1):
    why = C.create_string_buffer(512)
    rc = hip.kfdbg_engine_desc_refusal(family, C.byref(d), n_seq, why, len(why))
    return rc, why.value.decode()


FAMILIES = [PERSISTENT, XCD]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_test_shape_is_served_dense_or_with_a_hot_row_mask(hip, family):
    assert refusal(hip, family, desc()) == (OK, "")
    d = desc()
    d.layers[1].hot_ffn = ADDR
    assert refusal(hip, family, d) == (OK, "")


@pytest.mark.parametrize("family", FAMILIES)
def test_descriptor_refusals_of_both_families(hip, family):
    rc, why = refusal(hip, family, desc(dict(SMALL, head_dim=96)))
    assert rc == UNSUPPORTED and "head_dim must be 64 or 128" in why, why
    rc, why = refusal(hip, family, desc(dict(SMALL, dim=128)))
    assert rc == UNSUPPORTED and "not instantiated" in why, why
    rc, why = refusal(hip, family, desc(kv_stride=12))
    assert rc == INVALID_ARGS and "kv_stride not a multiple of 8" in why, why


@pytest.mark.parametrize("family", FAMILIES)
def test_layer_storage_not_served(hip, family):
    other = desc()
    other.layers[1].w[3] = weight(256, 256, L.T_SIGN)      # one matrix of another storage
    cache = desc()
    cache.layers[0].kcache = ADDR + 0x200008
    for d in (desc(type_=L.F8E5M2), desc(lGroup=64), other, cache):
        rc, why = refusal(hip, family, d)
        assert rc == UNSUPPORTED and "storage not served" in why, why


def test_persistent_engine_depth_bound(hip):
    """the deepest model of the 256-wide shape in 160 KB of LDS: the depth tests/test_engine_form_cpu.py pins for the form"""
    assert refusal(hip, PERSISTENT, desc(n_layer=579)) == (OK, "")
    rc, why = refusal(hip, PERSISTENT, desc(n_layer=580))
    assert rc == UNSUPPORTED and "exceed 160 KB of LDS" in why, why


def test_xcd_engines_sequence_bounds(hip):
    rc, why = refusal(hip, XCD, desc(QWEN3_4B), n_seq=9)
    assert rc == UNSUPPORTED and "at most 8 sequences" in why, why
    assert refusal(hip, XCD, desc(), n_seq=33)[0] == INVALID_ARGS
