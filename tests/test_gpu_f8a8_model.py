"""Qwen3.set_act_fp8 -- fp8 activations for the f8e5m2 layer matrices of token batches -- on the synthetic "tiny" model (2 layers, every layer matrix KF_F8E5M2).  Layer
0's V rows of a batch have no attention in front of them: embedding rows, the norm folded into kf_act_quant_f8, kf_linear_f8a8 -- held to Context.act_quant_f8 (itself
held to the restatement, tests/f8a8_restate.py) and Context.linear_f8a8 on the same inputs, bit for bit."""
import numpy as np
import pytest
import torch

import f8a8_restate as R
from conftest import bf16_t, u16
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth

pytestmark = pytest.mark.gpu
CFG = dict(synth.CONFIGS["tiny"], max_seq=96)
N_MAT = 7 * CFG["n_layer"]


@pytest.fixture(scope="module")
def gm():
    raw = synth.raw_weights_numpy(CFG, 1234, w_std=0.1)
    m = synth.build_from_raw(CFG, raw, L.F8E5M2, L.BF16)
    m.raw, m.toks = raw, prompt_ids(CFG, 41)
    yield m
    m.close()


@pytest.mark.parametrize("entry", ["prefill", "score"])
def test_token_batch_takes_the_fp8_route(gm, entry):
    c, lw, n = gm._ctx, gm.raw["layers"][0], 40
    gm.set_act_fp8(True)
    try:
        gm.prefill(gm.toks[:n])
        assert gm.f8a8_route_counts() == (0, N_MAT)   # the default threshold (128) keeps 40 rows on kf_linear
        gm.set_f8a8_tile_min(32)
        gm.set_act_fp8(True)
        gm.prefill(gm.toks[:n]) if entry == "prefill" else gm.score(gm.toks[:n + 1])
        rows = n if entry == "prefill" else n + 1
        assert gm.f8a8_route_counts() == (N_MAT, 0)
        v = gm.kv_to_host()[1][0, :rows]
        x = gm.raw["embed"][gm.toks[:rows]]
        q, step = c.act_quant_f8(bf16_t(x, c.device), bf16_t(lw["norm_in"], c.device))
        wq, ws = R.quant_rows(x, lw["norm_in"])
        assert np.array_equal(q.cpu().numpy(), wq) and np.array_equal(step.cpu().numpy(), ws)
        want = u16(c.linear_f8a8(c.quantize(bf16_t(lw["v"], c.device), L.F8E5M2), q, step))
        assert np.array_equal(v, want), "%d V elements differ" % int((v != want).sum())
        gm.set_act_fp8(True)   # the counts restart; 8 tokens stay on kf_linear, and so does a single token
        gm.prefill(gm.toks[:8])
        gm.forward(int(gm.toks[8]), 8)
        assert gm.f8a8_route_counts() == (0, 2 * N_MAT)
        gm.set_f8a8_tile_min(8)
        gm.prefill(gm.toks[:8])
        assert gm.f8a8_route_counts() == (N_MAT, 2 * N_MAT) and np.isfinite(gm.perplexity(gm.toks)[0])
    finally:
        gm.set_f8a8_tile_min(0)
        gm.set_act_fp8(False)


def test_switch_off_is_the_parent_path_and_refusals(gm):
    nb, lb = gm.prefill(gm.toks[:40])
    lp = gm.score(gm.toks).copy()
    gm.set_f8a8_tile_min(32)
    gm.set_act_fp8(True)
    assert "int8 activations run on the per-layer launches" in gm.engine_why()
    assert not np.array_equal(gm.prefill(gm.toks[:40])[1], lb)   # another arithmetic
    hot = np.zeros(CFG["ffn"], dtype=np.int32)
    hot[::2] = 1
    with pytest.raises(L.KFError, match="int8 activations are on"):
        gm.set_hot(0, hot)
    a, b = (torch.zeros(s, dtype=torch.bfloat16, device=gm._ctx.device) for s in ((16, CFG["dim"]), (CFG["n_head"] * CFG["head_dim"], 16)))
    with pytest.raises(L.KFError, match="int8 activations are on"):
        gm.set_adapters({"l0.q.w": (a, b)}, 1.0)
    gm.set_act_fp8(False)
    gm.set_f8a8_tile_min(0)
    na, la = gm.prefill(gm.toks[:40])
    assert na == nb and np.array_equal(la, lb) and np.array_equal(gm.score(gm.toks), lp)
    gm.set_hot(0, hot)
    with pytest.raises(L.KFError, match="hot-row mask"):
        gm.set_act_fp8(True)
    gm.set_hot(0, None)
    q4 = synth.build_from_raw(synth.CONFIGS["tiny"], gm.raw, L.Q4, L.BF16)
    with pytest.raises(L.KFError, match="no layer matrix is plain f8e5m2"):
        q4.set_act_fp8(True)
    q4.close()
