"""The weight setters' all-or-nothing rule ("a refused call changes nothing") and the .kun header against the recorded one.

kfh_set_weight* / kfh_set_norm resolve their target and run every check -- slot, adapter, layout, the NF3 conditions -- before the first change: a refused call
answers its documented status with a reason, and leaves the tensors, the captured graphs and the tokens of the model exactly as they were."""
import ctypes as C
import json
import os
import struct

import pytest
import torch

from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import DevWeight

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KF_INVALID_ARGS, KF_BLAS_UNALIGN = -20, -2000


@pytest.fixture(scope="module")
def model():
    cfg = dict(synth.CONFIGS["tiny"], tied=False)
    raw = synth.raw_weights_numpy(cfg, 77, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    yield cfg, m
    m.close()


def set_weight(m, layer, slot, w, blob_bytes=None, szData=None):
    return m.host.kfh_set_weight(m.h, layer, slot, w.type, w.ne0, w.ne1, C.c_void_p(w.blob.data_ptr()), w.blob.numel() if blob_bytes is None else blob_bytes,
                                 w.szData if szData is None else szData, 1, w.lGroup, w.qMin, w.qMax, w.qBias)


def test_a_refused_setter_changes_nothing(model):
    cfg, m = model
    m.set_engine(False)   # the step graphs are captured, so a dropped engine table shows as a dropped graph
    prompt = prompt_ids(cfg, 6)
    q = m.weights[(0, 0)]                                # layer 0's q_proj: Q4 [256, 256] in groups of 128
    one_group = 128 * 4 // 8
    assert q.szData == 256 * 256 // 2 and q.blob.numel() == DevWeight.blob_bytes(L.Q4, 256, 256)
    norm = torch.ones(cfg["dim"], dtype=torch.bfloat16, device=m.device)
    lut = torch.zeros(256 * 64 * 3 // 8 + (256 + 64 + 8 * 256) * 2, dtype=torch.uint8, device=m.device)   # the bytes of a 3-bit row codebook [256, 64]
    calls = [
        ("blob one group short", lambda: set_weight(m, 0, 0, q, blob_bytes=q.blob.numel() - one_group), KF_INVALID_ARGS),
        ("szData > blob_bytes", lambda: set_weight(m, 0, 0, q, szData=q.blob.numel() + 16), KF_INVALID_ARGS),
        ("slot 7", lambda: set_weight(m, 0, 7, q), KF_INVALID_ARGS),
        ("layer -1, slot 2", lambda: set_weight(m, -1, 2, q), KF_INVALID_ARGS),
        ("norm slot 4", lambda: m.host.kfh_set_norm(m.h, 0, 4, C.c_void_p(norm.data_ptr()), norm.numel(), 1), KF_INVALID_ARGS),
        ("3 bits, ne1 = 64", lambda: m.host.kfh_set_weight_lut_bits(m.h, 0, 0, 3, 256, 64, C.c_void_p(lut.data_ptr()), lut.numel(), 256 * 64 * 3 // 8, 1), KF_BLAS_UNALIGN),
    ]

    def refusals(calls):
        want = m.generate(prompt, 4, use_graph=True)
        for name, call, code in calls:
            graphs = m.num_graphs()
            rc = call()
            why = m.host.kfh_host_error().decode()
            print(name, rc, why)
            assert rc == code and why, name
            assert m.num_graphs() == graphs, name
            assert m.generate(prompt, 4, use_graph=True) == want, name
        return graphs

    assert refusals(calls) > 0, "the graphs were not active: the test would not see a dropped engine table"
    # a matrix that carries an adapter (an eager-only mode: no graphs to count, the tokens are the adapted model's)
    r = 16
    g = torch.Generator(device=m.device).manual_seed(3)
    a = (torch.randn(r, cfg["dim"], generator=g, device=m.device) * 0.05).to(torch.bfloat16)
    b = (torch.randn(cfg["n_head"] * cfg["head_dim"], r, generator=g, device=m.device) * 0.05).to(torch.bfloat16)
    m.set_adapters({"l0.q.w": (a, b)})
    try:
        refusals([("a matrix with an adapter", lambda: set_weight(m, 0, 0, q), KF_INVALID_ARGS)])
        assert m.host.kfh_n_adapters(m.h) == 1
    finally:
        m.clear_adapters()
    # and an accepted call still installs: the same blob again gives the same tokens, through graphs captured afresh
    want = m.generate(prompt, 4, use_graph=True)
    assert set_weight(m, 0, 0, q) == 0 and m.num_graphs() == 0
    assert m.generate(prompt, 4, use_graph=True) == want


def test_kun_header_is_the_recorded_one(model, tmp_path):
    """tests/golden/kun_header_tiny_q4_bf16.bin: the length prefix, the JSON header and the config tensor's bytes of this model's file as the commit before the
    parameter table wrote them (the tensor order and every offset follow the table); the data region is test_gpu_kun's save -> load -> same tokens"""
    _, m = model
    path = tmp_path / "tiny.kun"
    m.save_kun(path)
    raw = path.read_bytes()
    hlen = struct.unpack("<Q", raw[:8])[0]
    o0, o1 = json.loads(raw[8:8 + hlen])["__koifish__config__"]["data_offsets"]
    assert 8 + hlen + o1 == len(raw)
    with open(os.path.join(HERE, "golden", "kun_header_tiny_q4_bf16.bin"), "rb") as f:
        assert raw[:8 + hlen] + raw[8 + hlen + o0:] == f.read()
