"""NF3 layers through the checkpoint paths: Qwen3.from_hf(layer_type=L.NF3) quantises a Hugging Face directory to the blobs Context.quantize(., L.NF3) makes, and a
`.kun` file written from such a model (dtype "Q<3>", quant_method "NF", bits 3, gama = [R][C][LUT ne0 x 8]) loads back as the same model."""
import json
import struct

import msgpack
import numpy as np
import pytest

from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import Qwen3
from test_gpu_hf_load import write_hf

pytestmark = pytest.mark.gpu
HF = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _parse(path):
    raw = path.read_bytes()
    hlen = struct.unpack("<Q", raw[:8])[0]
    return json.loads(raw[8:8 + hlen]), raw[8 + hlen:]


def same_steps(a, b, cfg, n=12):
    prompt = prompt_ids(cfg, 10)
    tok = int(prompt[0])
    for pos in range(n):
        na, la = a.forward(tok, pos)
        nb, lb = b.forward(tok, pos)
        assert na == nb and np.array_equal(la, lb), "step %d" % pos
        tok = int(prompt[pos + 1]) if pos + 1 < len(prompt) else na
    assert a.generate(prompt, 16) == b.generate(prompt, 16)


def test_from_hf_and_kun_round_trip(tmp_path):
    cfg = synth.CONFIGS["tiny"]
    raw = synth.raw_weights_numpy(cfg, 4321, w_std=0.1)
    write_hf(tmp_path, cfg, raw)
    a = Qwen3.from_hf(tmp_path, L.NF3, L.BF16, max_seq=cfg["max_seq"])
    b = synth.build_from_raw(cfg, raw, L.NF3, L.BF16)          # Context.quantize(., L.NF3) per layer matrix
    # the loaded model's blobs, read back through the file it writes, are Context.quantize's
    path = tmp_path / "nf3.kun"
    a.save_kun(path)
    hdr, data = _parse(path)
    for (layer, slot), w in b.weights.items():
        if layer < 0:
            continue
        d = hdr["model.layers.%d.%s.weight" % (layer, HF[slot])]
        assert w.bits == 3 and d["dtype"] == "Q<3>" and d["shape"] == [w.ne0, w.ne1]
        assert d["szData"] == w.ne0 * w.ne1 * 3 // 8 and d["szGama"] == (w.ne0 + w.ne1 + 8 * w.ne0) * 2
        assert data[d["data_offsets"][0]:d["data_offsets"][1]] == w.blob.cpu().numpy().tobytes(), (layer, slot)
    js = msgpack.unpackb(data[hdr["__koifish__config__"]["data_offsets"][0]:])
    q = js["CLI_params"]["config"]["quantizer"]
    assert q["self_attn"] == {"quant_method": "NF", "bits": 3} and q["mlp"] == {"quant_method": "NF", "bits": 3} and "group_size" not in q
    same_steps(a, b, cfg)
    # save -> load keeps blobs and ids; a second generation of the file is the same file
    c = Qwen3.from_kun(path)
    same_steps(a, c, cfg)
    path2 = tmp_path / "again.kun"
    c.save_kun(path2)
    assert path2.read_bytes() == path.read_bytes()
    for m in (a, b, c):
        m.close()


def test_nf3_is_a_layer_storage(tmp_path):
    cfg = synth.CONFIGS["tiny"]
    write_hf(tmp_path, cfg, synth.raw_weights_numpy(cfg, 4321, w_std=0.1))
    with pytest.raises(L.KFError, match="NF3"):
        Qwen3.from_hf(tmp_path, L.NF3, L.NF3, max_seq=cfg["max_seq"])
