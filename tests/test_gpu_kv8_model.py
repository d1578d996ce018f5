"""Qwen3.set_kv_int8 -- the int8 KV cache -- on the synthetic "tiny" model (4-bit layers, canonical order) against a numpy decoder built from the oracle's own ops with the
restated quantiser and the restated integer-score attention (tests/kv8_restate.py) in place of O.attn_decode.  Token-serial steps are held bit for bit: logits, ids and the
int8 rows with their steps; generate() on captured graphs gives the restatement's ids.  A token batch attends with bf16 q to the DEQUANTISED rows on the MFMA prompt kernel
-- another approximation than the decode kernel's integer score, stated in DESIGN 4.2d: layer 0's int8 rows, which no attention precedes, are held bit for bit to the
restated quantiser on the bf16 rows the same prefill leaves with the switch off; logits and log-probs against a batch-form decoder (dequantised rows + O.attn_decode) to
the project's token-batch bar (LOGIT_TOL of tests/test_gpu_prefill.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import kv8_restate as R
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import runtime, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2.0 ** -6  # tests/test_gpu_prefill.py
CFG = dict(synth.CONFIGS["tiny"], max_seq=96)
WHY = "int8 KV cache runs on the per-layer launches"


class Decoder:
    """A Qwen3 decoder from the oracle's own ops on the int8 cache.  batch=False: the decode step's arithmetic (the restated integer-score attention); batch=True: a token
    batch's -- every key, the token's own included, dequantised, then the oracle's canonical attention with the bf16 q"""

    def __init__(self, cfg, raw, batch=False):
        self.c, self.batch = cfg, batch
        qz = lambda a, t: O.quantize(a, a.shape[0], a.shape[1], t)
        self.embed = qz(raw["embed"], L.BF16)
        self.final_norm = raw["final_norm"]
        self.layers = [dict({s: qz(lw[s], L.Q4) for s in synth.SLOTS}, **{s: lw[s] for s in synth.NORMS}) for lw in raw["layers"]]
        self.kv = [R.Cache8(cfg["max_seq"], cfg["n_kv"], cfg["head_dim"]) for _ in self.layers]

    def decode(self, token, pos):
        c = self.c
        nh, nkv, hd = c["n_head"], c["n_kv"], c["head_dim"]
        with O.canonical():
            x = O.embed(self.embed, token)
            for w, kv in zip(self.layers, self.kv):
                xn = O.rmsnorm(x, w["norm_in"])
                qv, kr, vr = (O.linear(w[s], xn) for s in ("q", "k", "v"))
                qv = O.rope(O.headnorm(qv, w["qn"], nh, hd), nh, hd, pos, c["theta"])
                kr = O.rope(O.headnorm(kr, w["kn"], nkv, hd), nkv, hd, pos, c["theta"])
                kv.put(pos, kr, vr)                             # the new row is quantised first and attended in its quantised form
                if self.batch:
                    kd, vd = kv.rows(pos + 1)
                    a = O.attn_decode(qv, kd, vd, pos, nh, nkv, hd, mode=O.ATTN_CANON)
                else:
                    a = kv.attend(qv, pos, nh)
                x = O.add(x, O.linear(w["o"], a))
                xn = O.rmsnorm(x, w["norm_post"])
                x = O.add(x, O.linear(w["down"], O.swiglu(O.linear(w["gate"], xn), O.linear(w["up"], xn))))
            logits = O.linear(self.embed, O.rmsnorm(x, self.final_norm))
            return O.argmax_bf16(logits), logits


_M = {}
N_SERIAL, N_BATCH, N_PROMPT, N_NEW = 20, 34, 12, 8


def model():
    """the 4-bit tiny model; beside it the restatement's forced steps (decode form) with their logits, its greedy steps behind a 12-token prompt, and the batch-form
    decoder's logits of 34 forced steps: built once, never changed"""
    if not _M:
        raw = synth.raw_weights_numpy(CFG, 1234, w_std=0.1)
        gm = synth.build_from_raw(CFG, raw, L.Q4, L.BF16)
        gm.set_canonical(1)
        toks = prompt_ids(CFG, N_BATCH)
        dec = Decoder(CFG, raw)
        logits = [dec.decode(int(toks[p]), p)[1] for p in range(N_SERIAL)]
        g = Decoder(CFG, raw)
        ids, tok = [], None
        for p in range(N_PROMPT + N_NEW):
            tok, _ = g.decode(int(toks[p]) if p < N_PROMPT else tok, p)
            ids.append(tok)
        bd = Decoder(CFG, raw, batch=True)
        blogits = [bd.decode(int(toks[p]), p)[1] for p in range(N_BATCH)]
        _M["m"] = (gm, raw, dec, toks, logits, ids, blogits)
    return _M["m"]


def rows_equal(gm, dec, n):
    k8, ks, v8, vs = gm.kv8_to_host()
    for l, kv in enumerate(dec.kv):
        for got, want, name in ((k8[l], kv.k8, "k8"), (v8[l], kv.v8, "v8")):
            assert np.array_equal(got[:n], want[:n]), "layer %d %s: %d codes differ" % (l, name, int((got[:n] != want[:n]).sum()))
        for got, want, name in ((ks[l], kv.ks, "ks"), (vs[l], kv.vs, "vs")):
            assert np.array_equal(got[:n].view(np.uint32), want[:n].view(np.uint32)), "layer %d %s" % (l, name)


def test_token_serial_bit_for_bit():
    gm, raw, dec, toks, logits, ids, _ = model()
    gm.set_kv_int8(True)
    try:
        assert gm.kv_int8()
        for p in range(N_SERIAL):
            tok, lg = gm.forward(int(toks[p]), p)
            assert np.array_equal(lg, logits[p]), "step %d: %d logits differ" % (p, int((lg != logits[p]).sum()))
            assert tok == O.argmax_bf16(logits[p])
        rows_equal(gm, dec, N_SERIAL)
        # generate on captured graphs (d_pos, position buckets): the restatement's ids; the engine refuses with the reason
        assert list(gm.generate(toks[:N_PROMPT], N_NEW, use_graph=True)) == ids[N_PROMPT - 1:N_PROMPT + N_NEW - 1]
        assert gm.num_graphs() >= 1
        assert WHY in gm.engine_why() and gm.engine_steps() <= 0
        gm.set_engine(True)
        assert list(gm.generate(toks[:N_PROMPT], N_NEW, use_graph=False)) == ids[N_PROMPT - 1:N_PROMPT + N_NEW - 1] and gm.engine_steps() <= 0
    finally:
        gm.set_kv_int8(False)
    assert not gm.kv_int8()


def held_to_the_bar(got_u16, ref_u16, what):
    ref = R.bf(ref_u16)
    err, bar = float(np.abs(R.bf(got_u16) - ref).max()), LOGIT_TOL * float(np.abs(ref).max())
    print("%s: max |logit error| %g, bar %g" % (what, err, bar))
    assert err <= bar, what


def test_prefill_of_33_tokens():
    gm, raw, dec, toks, logits, ids, blogits = model()
    n, hd = 33, CFG["head_dim"]
    gm.prefill(toks[:n])                                   # switch off: the bf16 rows
    k16, v16 = gm.kv_to_host()
    gm.set_kv_int8(True)
    try:
        nxt, lg = gm.prefill(toks[:n])
        k8, ks, v8, vs = gm.kv8_to_host()
        # layer 0: embed, rmsnorm, the projections, head-norm, rope -- no attention precedes them: the restated quantiser on the bf16 rows, bit for bit
        for got8, gots, rows in ((k8, ks, k16), (v8, vs, v16)):
            want8, wants = R.quant_heads(rows[0, :n], hd)
            assert np.array_equal(got8[0, :n], want8), "%d codes differ" % int((got8[0, :n] != want8).sum())
            assert np.array_equal(gots[0, :n].view(np.uint32), wants.view(np.uint32))
        held_to_the_bar(lg, blogits[n - 1], "prefill of %d" % n)
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
    finally:
        gm.set_kv_int8(False)
    # the same prompt cut into chunks of 16 (the chunk is fixed before a model's first token batch: a model of its own): the later chunks attend to the earlier ones'
    # dequantised rows; layer 0's int8 rows are the unchunked prefill's
    g2 = synth.build_from_raw(CFG, raw, L.Q4, L.BF16)
    try:
        g2.set_canonical(1)
        g2.set_prefill_mode(0, 16)
        g2.set_kv_int8(True)
        _, lc = g2.prefill(toks[:n])
        held_to_the_bar(lc, blogits[n - 1], "prefill of %d in chunks of 16" % n)
        c8 = g2.kv8_to_host()
        assert np.array_equal(c8[0][0, :n], k8[0, :n]) and np.array_equal(c8[2][0, :n], v8[0, :n])
        assert np.array_equal(c8[1][0, :n].view(np.uint32), ks[0, :n].view(np.uint32)) and np.array_equal(c8[3][0, :n].view(np.uint32), vs[0, :n].view(np.uint32))
    finally:
        g2.close()


def test_switch_on_and_off_restores_the_bits():
    gm, raw, dec, toks, logits, ids, _ = model()
    before = [gm.forward(int(toks[p]), p)[1] for p in range(4)]
    nb, lb = gm.prefill(toks[:33])
    gm.set_kv_int8(True)
    assert not np.array_equal(gm.forward(int(toks[0]), 0)[1], before[0])   # another arithmetic
    gm.set_kv_int8(False)
    for p in range(4):
        assert np.array_equal(gm.forward(int(toks[p]), p)[1], before[p]), "step %d: switching off did not restore the bits" % p
    na, la = gm.prefill(toks[:33])
    assert na == nb and np.array_equal(la, lb)


def test_refusals():
    """every refusal, in both directions, with its code and its reason"""
    cfg = synth.CONFIGS["tiny"]
    raw = synth.raw_weights_numpy(cfg, 7, w_std=0.1)
    gm = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    hot = np.zeros(cfg["ffn"], dtype=np.int32)
    hot[::2] = 1
    dev = gm._ctx.device
    a = torch.zeros((16, cfg["dim"]), dtype=torch.bfloat16, device=dev)
    b = torch.zeros((cfg["n_head"] * cfg["head_dim"], 16), dtype=torch.bfloat16, device=dev)
    adapter = lambda: gm.host.kfh_set_adapter(gm.h, 0, 0, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), 16, 1.0)
    why = lambda: gm.host.kfh_host_error().decode()
    INVALID = -20   # KF_INVALID_ARGS
    try:
        # while the switch is on
        gm.set_kv_int8(True)
        with pytest.raises(L.KFError, match="int8 KV cache is on"):
            gm.set_act_int8_q4(True)
        with pytest.raises(L.KFError, match="int8 KV cache is on"):
            gm.set_act_int8(True)
        assert adapter() == INVALID and "the int8 KV cache is on" in why() and gm.host.kfh_n_adapters(gm.h) == 0
        with pytest.raises(L.KFError, match="int8 KV cache is on"):
            gm.set_hot(0, hot)
        with pytest.raises(L.KFError, match="fuse_level 0 has no int8 KV cache form"):
            gm.set_fuse_level(0)
        rc = gm.host.kfh_tp_init(gm.h, 0, 2, 0)
        assert rc != 0 and rc != INVALID and "int8 KV cache is on" in why()
        with pytest.raises(L.KFError, match=WHY):
            runtime.XcdReplicas(gm, 2)
        gm.set_kv_int8(False)
        # the other direction: each of them refuses the switch
        gm.set_act_int8_q4(True)
        with pytest.raises(L.KFError, match="int8 activations are on"):
            gm.set_kv_int8(True)
        gm.set_act_int8_q4(False)
        assert adapter() == 0
        with pytest.raises(L.KFError, match="adapters are attached"):
            gm.set_kv_int8(True)
        gm.clear_adapters()
        gm.set_hot(0, hot)
        with pytest.raises(L.KFError, match="hot-row mask"):
            gm.set_kv_int8(True)
        gm.set_hot(0, None)
        gm.set_fuse_level(0)
        with pytest.raises(L.KFError, match="fuse_level 0"):
            gm.set_kv_int8(True)
        gm.set_fuse_level(1)
        assert not gm.kv_int8()
        gm.set_kv_int8(True)                                  # and with all of them gone it switches on again
        gm.set_kv_int8(False)
        assert gm.host.kfh_tp_init(gm.h, 0, 2, 0) == 0         # last: this model is a TP rank from here on
        with pytest.raises(L.KFError, match="tensor-parallel rank"):
            gm.set_kv_int8(True)
    finally:
        gm.close()


def test_an_existing_xcd_replicas_object_refuses_at_its_next_use():
    """the XCD objects in the other direction: an XcdReplicas built while the switch is off decodes; the switch moved on its Fish, its next use re-checks, refuses with
    the reason and launches nothing; with the switch off again it decodes on.  (XcdTP is built over tensor-parallel ranks, and a rank refuses the switch itself --
    test_refusals -- so XcdTP::Build's own check is a second line that no public path reaches.)"""
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
        with pytest.raises(L.KFError):
            xr.run_steps(1)
        assert WHY in gm.host.kfh_host_error().decode()
        assert all(np.array_equal(xr.tokens_out(s_, 3), before[s_]) for s_ in range(2)) and xr.state(0)[1] == 3   # nothing was launched
        gm.set_kv_int8(False)
        xr.run_steps(1)
        xr.check()
        assert xr.state(0)[1] == 4
    finally:
        gm.close()
