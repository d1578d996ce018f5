"""Qwen3.set_kv_int8_prefill -- the int8 prompt attention, a sub-setting of the int8 KV cache -- on the synthetic "tiny" model (4-bit layers, canonical order) against a
batch-form decoder built from the oracle's own ops with the restated quantiser and the restated prompt attention (tests/kv8_prefill_restate.py) in place of the
dequantise route.  The restated attention of a row depends on its position alone, so ONE run of the decoder over 34 tokens is the reference of prefill, score, a chunked
prefill and a chunk behind a prefix alike.  Logits are held to the project's token-batch bar (LOGIT_TOL of tests/test_gpu_prefill.py, as tests/test_gpu_kv8_model.py);
what the definition states as exact is held bit for bit: layer 0's int8 rows (the quantiser is the dequantise route's), the attention bits of a chunked prefill
against an unchunked one on the model's own cache, and the dequantise route's logits once the sub-setting is off again.

Observed on an MI355X, max |logit error| against the bar 2^-6 max|logit| (printed by held_to_the_bar): prefill of 33: 0 (bar 0.0845); score of 34: 0 (bar 0.0796);
20 tokens behind a prefix of 13: 0 (bar 0.0845); prefill of 33 in chunks of 17 + 16: 0 (bar 0.0845) -- on this model the kernel's fp32 sums round to the same bf16
values as the restatement's exact ones everywhere, so the logits come out bit-equal; the bar, not equality, is what the definition promises."""
import numpy as np
import pytest
import torch

import kv8_prefill_restate as P
import kv8_restate as R
from conftest import bf16_t, u16
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import runtime, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2.0 ** -6  # tests/test_gpu_prefill.py
CFG = dict(synth.CONFIGS["tiny"], max_seq=96)
WHY = "int8 KV cache runs on the per-layer launches"
NOTE = "kfh_set_kv_int8_prefill"
N_BATCH, N_PROMPT, N_NEW = 34, 12, 8


class BatchDecoder:
    """A Qwen3 decoder from the oracle's own ops on the int8 cache: token batches attend with the restated prompt form (every row of the batch is quantised into the
    cache first), single tokens with the restated decode form"""

    def __init__(self, cfg, raw):
        self.c = cfg
        qz = lambda a, t: O.quantize(a, a.shape[0], a.shape[1], t)
        self.embed = qz(raw["embed"], L.BF16)
        self.final_norm = raw["final_norm"]
        self.layers = [dict({s: qz(lw[s], L.Q4) for s in synth.SLOTS}, **{s: lw[s] for s in synth.NORMS}) for lw in raw["layers"]]
        self.kv = [R.Cache8(cfg["max_seq"], cfg["n_kv"], cfg["head_dim"]) for _ in self.layers]
        self.attn = P.BatchAttention(cfg["n_head"], cfg["n_kv"], cfg["head_dim"])

    def _qkv(self, w, x, pos):
        c = self.c
        nh, nkv, hd = c["n_head"], c["n_kv"], c["head_dim"]
        xn = O.rmsnorm(x, w["norm_in"])
        qv, kr, vr = (O.linear(w[s], xn) for s in ("q", "k", "v"))
        return (O.rope(O.headnorm(qv, w["qn"], nh, hd), nh, hd, pos, c["theta"]), O.rope(O.headnorm(kr, w["kn"], nkv, hd), nkv, hd, pos, c["theta"]), vr)

    def _rest(self, w, x, a):
        x = O.add(x, O.linear(w["o"], a))
        xn = O.rmsnorm(x, w["norm_post"])
        return O.add(x, O.linear(w["down"], O.swiglu(O.linear(w["gate"], xn), O.linear(w["up"], xn))))

    def batch(self, tokens, pos0=0):
        """-> the logits of every row"""
        with O.canonical():
            xs = [O.embed(self.embed, int(t)) for t in tokens]
            for w, kv in zip(self.layers, self.kv):
                qs = []
                for i, x in enumerate(xs):
                    qv, kr, vr = self._qkv(w, x, pos0 + i)
                    kv.put(pos0 + i, kr, vr)
                    qs.append(qv)
                a = self.attn(kv, np.stack(qs), pos0)
                xs = [self._rest(w, x, a[i]) for i, x in enumerate(xs)]
            return [O.linear(self.embed, O.rmsnorm(x, self.final_norm)) for x in xs]

    def decode(self, token, pos):
        with O.canonical():
            x = O.embed(self.embed, token)
            for w, kv in zip(self.layers, self.kv):
                qv, kr, vr = self._qkv(w, x, pos)
                kv.put(pos, kr, vr)
                x = self._rest(w, x, kv.attend(qv, pos, self.c["n_head"]))
            logits = O.linear(self.embed, O.rmsnorm(x, self.final_norm))
            return O.argmax_bf16(logits), logits


_M = {}


def model():
    """the 4-bit tiny model; the batch-form decoder's logits of 34 tokens; the restatement's greedy ids behind an int8 prefill of 12: built once, never changed"""
    if not _M:
        raw = synth.raw_weights_numpy(CFG, 1234, w_std=0.1)
        gm = synth.build_from_raw(CFG, raw, L.Q4, L.BF16)
        gm.set_canonical(1)
        toks = prompt_ids(CFG, N_BATCH)
        blogits = BatchDecoder(CFG, raw).batch(toks)
        g = BatchDecoder(CFG, raw)
        tok = O.argmax_bf16(g.batch(toks[:N_PROMPT])[-1])
        ids = [tok]
        for p in range(N_PROMPT, N_PROMPT + N_NEW - 1):
            tok, _ = g.decode(tok, p)
            ids.append(tok)
        _M["m"] = (gm, raw, toks, blogits, ids)
    return _M["m"]


def held_to_the_bar(got_u16, ref_u16, what):
    ref = R.bf(ref_u16)
    err, bar = float(np.abs(R.bf(got_u16) - ref).max()), LOGIT_TOL * float(np.abs(ref).max())
    print("%s: max |logit error| %g, bar %g" % (what, err, bar))
    assert err <= bar, what


def same_rows(a, b, n, layer=0):
    """(k8, ks, v8, vs) of two models: rows 0 .. n - 1 of a layer, bit for bit"""
    for x, y in zip(a, b):
        assert np.array_equal(x[layer, :n].view(np.uint8), y[layer, :n].view(np.uint8))


def test_token_batches_against_the_restatement():
    gm, raw, toks, blogits, ids = model()
    n, layers = 33, CFG["n_layer"]
    gm.set_kv_int8(True)
    try:
        assert not gm.kv_int8_prefill()                      # off by default
        gm.kv8_route_counts(reset=True)
        _, l_deq = gm.prefill(toks[:n])
        rows_deq = gm.kv8_to_host()
        assert gm.kv8_route_counts(reset=True) == {"prefill_int8": 0, "prefill_dequant": layers}
        gm.set_kv_int8_prefill(True)
        assert gm.kv_int8_prefill() and gm.kv_int8()
        assert WHY in gm.engine_why() and NOTE in gm.engine_why()
        _, lg = gm.prefill(toks[:n])
        assert gm.kv8_route_counts() == {"prefill_int8": layers, "prefill_dequant": 0}
        held_to_the_bar(lg, blogits[n - 1], "prefill of %d" % n)
        same_rows(gm.kv8_to_host(), rows_deq, n)             # layer 0: no attention precedes its rows, and the quantiser is the dequantise route's
        # score of n + 1 tokens: every log-prob against the batch-form decoder's logits
        lp = gm.score(toks[:n + 1])
        for i in range(n):
            f = R.bf(blogits[i]).astype(np.float64)
            want = f[toks[i + 1]] - (f.max() + np.log(np.exp(f - f.max()).sum()))
            bar = 2 * LOGIT_TOL * float(np.abs(f).max())
            assert abs(float(lp[i]) - want) <= bar, "position %d: log-prob %g against %g, bar %g" % (i, lp[i], want, bar)
        held_to_the_bar(gm.logits(), blogits[n], "score of %d" % (n + 1))
        # 20 tokens at pos0 = 13 behind a prefix
        gm.prefill(toks[:13])
        _, l2 = gm.prefill(toks[13:33], pos0=13)
        held_to_the_bar(l2, blogits[n - 1], "20 tokens behind a prefix of 13")
        ppl = gm.perplexity(toks[:n + 1])
        assert np.isfinite(ppl[0]) and ppl[2] == n
        c = gm.kv8_route_counts(reset=True)
        assert c["prefill_dequant"] == 0 and c["prefill_int8"] == layers * 5   # prefill, score, prefix, chunk, perplexity: one launch per layer and batch
        # off again: the dequantise route's logits, bit for bit
        gm.set_kv_int8_prefill(False)
        _, l_off = gm.prefill(toks[:n])
        assert np.array_equal(l_off, l_deq) and gm.kv8_route_counts() == {"prefill_int8": 0, "prefill_dequant": layers}
        assert not np.array_equal(lg, l_deq)                 # and the int8 prompt attention is another arithmetic
        # the sub-setting goes with the cache
        gm.set_kv_int8_prefill(True)
        gm.set_kv_int8(False)
        assert not gm.kv_int8_prefill()
    finally:
        gm.set_kv_int8(False)


def test_chunked_prefill_and_generate():
    """17 + 16 against one batch of 33: the later chunk attends to the earlier one's int8 rows exactly as an unchunked row attends to them"""
    gm, raw, toks, blogits, ids = model()
    n, layers, c = 33, CFG["n_layer"], CFG
    g2 = synth.build_from_raw(CFG, raw, L.Q4, L.BF16)
    gm.set_kv_int8(True)
    try:
        gm.set_kv_int8_prefill(True)
        gm.prefill(toks[:n])
        whole = gm.kv8_to_host()
        g2.set_canonical(1)
        g2.set_prefill_mode(0, 17)       # the chunk is fixed before a model's first token batch: a model of its own
        g2.set_kv_int8(True)
        g2.set_kv_int8_prefill(True)
        g2.kv8_route_counts(reset=True)
        _, lc = g2.prefill(toks[:n])
        held_to_the_bar(lc, blogits[n - 1], "prefill of %d in chunks of 17 + 16" % n)
        assert g2.kv8_route_counts() == {"prefill_int8": layers * 2, "prefill_dequant": 0}
        chunked = g2.kv8_to_host()
        same_rows(chunked, whole, n)
        # the attention itself on the model's own layer-0 rows: the same q rows in one launch of 33 and in launches of 17 + 16
        ctx, dev = g2._ctx, g2._ctx.device
        k8, ks, v8, vs = (torch.from_numpy(np.ascontiguousarray(a[0])).to(dev) for a in chunked)
        q = bf16_t(R.to_bf((0.5 * np.random.default_rng(5).standard_normal((n, c["n_head"] * c["head_dim"]))).astype(np.float32)), dev)
        run = lambda pos0, m: u16(ctx.attn_prefill_kv8(q[pos0:pos0 + m], k8, v8, ks, vs, pos0, c["n_head"], c["n_kv"], c["head_dim"]))
        assert np.array_equal(run(0, n), np.concatenate([run(0, 17), run(17, 16)]))
        # generate with the prompt as an int8 token batch, then the decode kernel on the rows it left: the restatement's ids
        g2.set_prefill_mode(1)
        assert list(g2.generate(toks[:N_PROMPT], N_NEW, use_graph=True)) == ids
        assert g2.kv8_route_counts()["prefill_dequant"] == 0
    finally:
        gm.set_kv_int8(False)
        g2.close()


def test_refused_while_the_cache_is_off():
    gm, raw, toks, blogits, ids = model()
    assert not gm.kv_int8() and not gm.kv_int8_prefill()
    with pytest.raises(L.KFError, match="sub-setting of the int8 KV cache"):
        gm.set_kv_int8_prefill(True)
    assert not gm.kv_int8_prefill()
    gm.set_kv_int8_prefill(False)                            # switching off is never refused
    gm.kv8_route_counts(reset=True)
    gm.prefill(toks[:8])
    assert gm.kv8_route_counts(reset=True) == {"prefill_int8": 0, "prefill_dequant": 0}   # the bf16 cache: neither route


def test_an_existing_xcd_replicas_object_refuses_at_its_next_use():
    """as for set_kv_int8: an XcdReplicas built before the switches moved re-checks at its next use, refuses with the reason (which names the sub-setting) and launches
    nothing; moving the sub-setting alone makes it re-check too; with everything off again it decodes on"""
    cfg = dict(synth.CONFIGS["small"], max_seq=64)
    gm = synth.build_from_raw(cfg, synth.raw_weights_numpy(cfg, 1234, w_std=0.1), L.Q4, L.BF16)
    try:
        gm.set_canonical(1)
        xr = runtime.XcdReplicas(gm, 2)
        for s_ in range(2):
            xr.set_state(s_, 5 + s_, 0)
        xr.run_steps(3)
        xr.check()
        before = [xr.tokens_out(s_, 3).copy() for s_ in range(2)]
        gm.set_kv_int8(True)
        gm.set_kv_int8_prefill(True)
        with pytest.raises(L.KFError):
            xr.run_steps(1)
        why = gm.host.kfh_host_error().decode()
        assert WHY in why and NOTE in why
        with pytest.raises(L.KFError, match=WHY):
            runtime.XcdReplicas(gm, 2)
        gm.set_kv_int8_prefill(False)
        with pytest.raises(L.KFError):
            xr.run_steps(1)
        assert WHY in gm.host.kfh_host_error().decode() and NOTE not in gm.host.kfh_host_error().decode()
        assert all(np.array_equal(xr.tokens_out(s_, 3), before[s_]) for s_ in range(2)) and xr.state(0)[1] == 3   # nothing was launched
        gm.set_kv_int8(False)
        xr.run_steps(1)
        xr.check()
        assert xr.state(0)[1] == 4
    finally:
        gm.close()
