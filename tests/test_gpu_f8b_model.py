"""A host model of e4m3 block-scaled layers (include/kf_abi.h "FP8 block-scaled layers"): the tiny model against its bf16 twin -- the project's quantiser uses
power-of-two scales, so every dequantised weight is a bf16 value and a model of bf16 layers built from them is the same function -- and an FP8 checkpoint directory
against the same blobs set directly."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

from f8a8_restate import bf
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import SLOTS, Qwen3
from test_gpu_hf_load import HF, write_hf

pytestmark = pytest.mark.gpu
CFG = synth.CONFIGS["tiny"]
BAR = 2.0 ** -6   # the token-batch bar on logits, times max |logit|


@pytest.fixture(scope="module")
def pair(ctx):
    raw = synth.raw_weights_numpy(CFG, 4321, w_std=0.1)
    a, b = synth.build_from_raw(CFG, raw, L.F8E4M3, L.BF16), synth.build_from_raw(CFG, raw, L.BF16, L.BF16)
    for li in range(CFG["n_layer"]):
        for si in range(len(SLOTS)):
            b.set_weight(li, si, ctx.quantize(ctx.dequant(a.weights[(li, si)]), L.BF16))
    yield a, b
    a.close(), b.close()


def test_tiny_model_against_its_bf16_twin(pair):
    a, b = pair
    toks = prompt_ids(CFG, 32)
    serial, top = [], 0.0
    for pos in range(25):   # token-serial logits of both; the twin's largest |logit| is the scale of every bar below
        la, lb = bf(a.forward(int(toks[pos]), pos)[1]), bf(b.forward(int(toks[pos]), pos)[1])
        top = max(top, float(np.abs(lb).max()))
        serial.append(la)
        assert pos >= 6 or np.abs(la - lb).max() <= BAR * np.abs(lb).max(), "position %d" % pos
    a.prefill(toks[:24])   # MFMA tiles from the stored bytes, then one step on the rows they left in the cache
    assert np.abs(bf(a.forward(int(toks[24]), 24)[1]) - serial[24]).max() <= BAR * np.abs(serial[24]).max()
    # a log-prob is logit[target] - logsumexp(logits): logits that move by at most d move it by at most 2 d, and so the mean; ppl = exp(-mean)
    pa, pb = a.perplexity(toks)[0], b.perplexity(toks)[0]
    for pos in range(25, 32):
        top = max(top, float(np.abs(bf(b.forward(int(toks[pos]), pos)[1])).max()))
    assert abs(np.log(pa / pb)) <= 2 * BAR * top


def test_what_the_storage_is_not_served_by_says_so(pair):
    a, _ = pair
    a.generate(prompt_ids(CFG, 4), 4)   # the decode path asks for the engine and takes the per-layer launches
    assert "e4m3 block-scaled" in a.engine_why()
    for call in (lambda: a.generate_batch([[1, 2], [3, 4]], 2), lambda: a.verify([1, 2], 0), lambda: a.set_kv_int8(True)):
        with pytest.raises(L.KFError, match="e4m3 block-scaled"):
            call()


def test_checkpoint_directory(pair, tmp_path):
    a, _ = pair
    write_hf(tmp_path, CFG, synth.raw_weights_numpy(CFG, 4321, w_std=0.1))
    t = load_file(str(tmp_path / "model.safetensors"))
    for li in range(CFG["n_layer"]):
        for si, s in enumerate(SLOTS):
            w, name = a.weights[(li, si)], "model.layers.%d.%s" % (li, HF[s])
            t[name + ".weight"] = w.codes().cpu().view(torch.float8_e4m3fn)
            t[name + ".weight_scale_inv"] = w.scales().cpu().to(torch.bfloat16 if si == 0 else torch.float32)   # power-of-two scales: exact in either
    save_file(t, str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    card = json.loads((tmp_path / "config.json").read_text())
    card["quantization_config"] = {"quant_method": "fp8", "weight_block_size": [128, 128]}
    (tmp_path / "config.json").write_text(json.dumps(card))
    c = Qwen3.from_hf(tmp_path, max_seq=CFG["max_seq"])
    toks = prompt_ids(CFG, 6)
    for pos in range(6):
        (na, la), (nc, lc) = a.forward(int(toks[pos]), pos), c.forward(int(toks[pos]), pos)
        assert na == nc and np.array_equal(la, lc), "position %d" % pos
    c.close()
    card["quantization_config"]["weight_block_size"] = [64, 64]
    (tmp_path / "config.json").write_text(json.dumps(card))
    with pytest.raises(L.KFError, match=r"weight_block_size \[128, 128\]"):
        Qwen3.from_hf(tmp_path, max_seq=CFG["max_seq"])
