"""A whole Qwen3 (tiny) with NF3 layer matrices -- 3-bit row codebooks multiplied from the packed stream (kf_set_row_unpack, switched on by the host model for its own
context) -- against the CPU oracle, and against the TWIN MODEL on the device: the same blobs re-packed as 4-bit row codebooks (tests/rowq_twin.py), which must give the
same bits everywhere, in both summation orders.

The embedding is redrawn at std 0.1: with it the oracle's top-2 margin is above 0.6 max|logit| at all 36 positions for both heads (with the stock 0.02 it falls to
0.004 and to exact ties), so greedy ids are compared at every position."""
import numpy as np
import pytest

import rowq_twin as T
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import Context, Qwen3
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2.0 ** -6
HEADS = [L.BF16, L.NF4]


def raw_weights(cfg):
    raw = synth.raw_weights_numpy(cfg, 4321, 0.02)
    raw["embed"] = synth.f32_to_bf16_np(np.random.default_rng(5321).normal(0.0, 0.1, size=raw["embed"].shape).astype(np.float32))
    return raw


def oracle_nf3(cfg, raw, head_type):
    emb = O.quantize_nf4(raw["embed"], *raw["embed"].shape) if head_type == L.NF4 else O.quantize(raw["embed"], *raw["embed"].shape, L.BF16, 128)
    w = {"embed": emb, "head": emb, "final_norm": raw["final_norm"], "layers": []}
    for lw in raw["layers"]:
        d = {s: O.quantize_nf3(lw[s], *lw[s].shape) for s in synth.SLOTS}
        d.update({s: lw[s] for s in synth.NORMS})
        w["layers"].append(d)
    return O.Qwen3Oracle(cfg, w)


def twin_of(cfg, raw, gm, head_type):
    """the model whose layer matrices are the 4-bit twins of gm's device blobs"""
    ctx = Context(0)
    m = Qwen3(cfg, 0)
    m._ctx = ctx
    m.set_weight(-1, 0, ctx.quantize(synth._bf16_t(raw["embed"], ctx.device), head_type, 128))
    m.tie_head()
    m.set_norm(-1, 0, synth._bf16_t(raw["final_norm"], ctx.device))
    for li, lw in enumerate(raw["layers"]):
        for si in range(len(synth.SLOTS)):
            w = gm.weights[(li, si)]
            assert w.bits == 3
            b = w.blob.cpu().numpy()
            ow = O.LutWeight(w.ne0, w.ne1, b[:w.szData], b[w.szData:].view(np.uint16)[w.ne0 + w.ne1:], bits=3)
            tw = T.twin(ow)
            assert np.array_equal(O.dequant(tw), O.dequant(ow))
            m.set_weight(li, si, ctx.upload_lut_blob(w.ne0, w.ne1, T.blob(tw), bits=4))
        for si, s in enumerate(synth.NORMS):
            m.set_norm(li, si, synth._bf16_t(lw[s], ctx.device))
    ctx.sync()
    return m


@pytest.fixture(scope="module", params=HEADS, ids=["bf16-head", "nf4-head"])
def models(request):
    cfg = synth.CONFIGS["tiny"]
    raw = raw_weights(cfg)
    gm = synth.build_from_raw(cfg, raw, L.NF3, request.param)
    tm = twin_of(cfg, raw, gm, request.param)
    yield cfg, raw, request.param, gm, tm
    gm.close()
    tm.close()


def test_against_the_oracle(models):
    cfg, raw, head_type, gm, _ = models
    om = oracle_nf3(cfg, raw, head_type)
    prompt = prompt_ids(cfg, 24)
    tok = int(prompt[0])
    o_logits = o_next = None
    for pos in range(36):   # 24 teacher-forced, 12 free
        g_next, g_logits = gm.forward(tok, pos)
        o_next, o_logits, _ = om.decode(tok, pos)
        gl, ol = O.bf16_to_f32(g_logits), O.bf16_to_f32(o_logits)
        assert np.abs(gl - ol).max() <= LOGIT_TOL * np.abs(ol).max(), "step %d" % pos
        assert g_next == O.argmax_bf16(g_logits) and g_next == o_next, "step %d: greedy id %d vs oracle %d" % (pos, g_next, o_next)
        if pos == 23:
            p_logits, p_next = o_logits, o_next
        tok = int(prompt[pos + 1]) if pos + 1 < len(prompt) else o_next
    assert gm.generate(prompt, 12, use_graph=True) == gm.generate(prompt, 12, use_graph=False)
    g_next, g_logits = gm.prefill(prompt)
    assert np.abs(O.bf16_to_f32(g_logits) - O.bf16_to_f32(p_logits)).max() <= LOGIT_TOL * np.abs(O.bf16_to_f32(p_logits)).max()
    assert g_next == p_next
    om.close()


@pytest.mark.parametrize("canon", [True, False], ids=["canonical", "dot2"])
def test_bit_equal_to_the_twin_model(models, canon):
    cfg, _, _, gm, tm = models
    try:
        gm.set_canonical(canon), tm.set_canonical(canon)
        seq = prompt_ids(cfg, 40, seed=11)
        tok = int(seq[0])
        for pos in range(36):   # decode steps: 24 forced, 12 free
            a, la = gm.forward(tok, pos)
            b, lb = tm.forward(tok, pos)
            assert a == b and np.array_equal(la, lb), "decode step %d" % pos
            tok = int(seq[pos + 1]) if pos + 1 < 24 else a
        for x, y in zip(gm.kv_to_host(), tm.kv_to_host()):
            assert np.array_equal(x[:, :36], y[:, :36]), "K / V rows of the decode steps"
        assert gm.generate(seq[:24], 12, use_graph=True) == tm.generate(seq[:24], 12, use_graph=True)
        for n in (24, 40):      # token batches: Q | K | V, gate | up and the single matrices on the tile kernels
            a, la = gm.prefill(seq[:n])
            b, lb = tm.prefill(seq[:n])
            assert a == b and np.array_equal(la, lb), "prefill of %d tokens" % n
            for x, y in zip(gm.kv_to_host(), tm.kv_to_host()):
                assert np.array_equal(x[:, :n], y[:, :n]), "K / V rows of the prefill of %d tokens" % n
        sa, ta = gm.score(seq, want_top1=True)
        sb, tb = tm.score(seq, want_top1=True)
        assert np.array_equal(sa, sb) and np.array_equal(ta, tb)
        assert gm.perplexity(seq) == tm.perplexity(seq)
    finally:
        gm.set_canonical(True), tm.set_canonical(True)


def test_what_the_storage_refuses(models):
    cfg, raw, head_type, gm, _ = models
    gm.forward(1, 0)
    assert gm.engine_steps() <= 0 and "3-bit row codebook" in gm.engine_why()
    with pytest.raises(L.KFError, match="3-bit row codebook"):
        gm.verify([1, 2, 3], 0)
    if head_type == L.BF16:   # once: the embedding and the head stay bf16 or 4-bit
        with pytest.raises(L.KFError, match="NF3"):
            synth.build_from_raw(cfg, raw, L.NF3, L.NF3)
