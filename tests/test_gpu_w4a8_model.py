"""Qwen3.set_act_int8_q4 -- int8 activations for the 4-bit layer matrices -- on the synthetic "tiny" model against a numpy decoder built from the oracle's own ops with
the restated quantiser and the restated W4.A8 product (tests/w4a8_restate.py) in place of the seven linears.  Token-serial steps are held bit for bit (logits, ids, K / V
rows); so are layer 0's K / V rows of a token batch, which no attention precedes, and the two routes of a batch (MFMA tiles, mat-vec) against each other.  Logits and
log-probs behind a token batch's prompt attention, which sums in MFMA order, are held to the project's token-batch bar (tests/test_gpu_prefill.py), as
tests/test_gpu_a8.py holds the ternary family's."""
import numpy as np
import pytest

from a8_restate import BITS, IntW, linear_a8
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O
from w4a8_restate import IntW4, bf, linear_w4a8, quant_rows

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2.0 ** -6  # tests/test_gpu_prefill.py
CFG = dict(synth.CONFIGS["tiny"], max_seq=96)
N_MAT = 7 * CFG["n_layer"]
WHY = "int8 activations run on the per-layer launches"


class Decoder:
    """A Qwen3 decoder from the oracle's own ops; `q4` / `tern`: which switch is on.  A 4-bit matrix takes the restated W4.A8 product under q4, a ternary / 1-bit one the
    restated W1.58.A8 product under tern, every other one the oracle's bf16-activation linear"""

    def __init__(self, cfg, raw, types, q4=True, tern=False):
        self.c = cfg
        qz = lambda a, t: O.quantize(a, a.shape[0], a.shape[1], t)
        self.embed = qz(raw["embed"], L.BF16)
        self.final_norm = raw["final_norm"]
        self.layers = []
        for lw in raw["layers"]:
            d = {}
            for s in synth.SLOTS:
                w = qz(lw[s], types[s])
                d[s] = IntW4(w) if (q4 and types[s] == L.Q4) else IntW(w) if (tern and types[s] in BITS) else w
            d.update({s: lw[s] for s in synth.NORMS})
            self.layers.append(d)
        kvd = cfg["n_kv"] * cfg["head_dim"]
        self.k = np.zeros((cfg["n_layer"], cfg["max_seq"], kvd), dtype=np.uint16)
        self.v = np.zeros_like(self.k)

    def mv(self, w, x, qx, sx):
        return linear_w4a8(w, qx, sx)[0] if isinstance(w, IntW4) else linear_a8(w, qx, sx)[0] if isinstance(w, IntW) else O.linear(w, x)

    def lin(self, w, x):
        return self.mv(w, x, *quant_rows(x))

    def decode(self, token, pos):
        c = self.c
        with O.canonical():
            x = O.embed(self.embed, token)
            for l, w in enumerate(self.layers):
                xn = O.rmsnorm(x, w["norm_in"])
                qx, sx = quant_rows(xn)                       # one quantisation of the normed row for q | k | v
                qv, kv, vv = (self.mv(w[s], xn, qx, sx) for s in ("q", "k", "v"))
                qv = O.rope(O.headnorm(qv, w["qn"], c["n_head"], c["head_dim"]), c["n_head"], c["head_dim"], pos, c["theta"])
                kv = O.rope(O.headnorm(kv, w["kn"], c["n_kv"], c["head_dim"]), c["n_kv"], c["head_dim"], pos, c["theta"])
                self.k[l, pos], self.v[l, pos] = kv, vv
                a = O.attn_decode(qv, self.k[l], self.v[l], pos, c["n_head"], c["n_kv"], c["head_dim"], mode=O.ATTN_CANON)
                x = O.add(x, self.lin(w["o"], a))             # y = bf16(residual + bf16(W.x))
                xn = O.rmsnorm(x, w["norm_post"])
                qx, sx = quant_rows(xn)                       # ... and one for gate | up
                act = O.swiglu(self.mv(w["gate"], xn, qx, sx), self.mv(w["up"], xn, qx, sx))
                x = O.add(x, self.lin(w["down"], act))
            logits = O.linear(self.embed, O.rmsnorm(x, self.final_norm))
            return O.argmax_bf16(logits), logits


ALL_Q4 = {s: L.Q4 for s in synth.SLOTS}
_M = {}


def model():
    """the 4-bit tiny model; beside it the restatement's 71 forced steps (logits of each, K / V rows) and its 8 greedy steps behind a 12-token prompt: built once"""
    if not _M:
        raw = synth.raw_weights_numpy(CFG, 1234, w_std=0.1)
        gm = synth.build_from_raw(CFG, raw, L.Q4, L.BF16)
        gm.set_canonical(1)
        toks = prompt_ids(CFG, 71)
        dec = Decoder(CFG, raw, ALL_Q4)
        logits = [dec.decode(int(toks[p]), p)[1] for p in range(71)]
        g = Decoder(CFG, raw, ALL_Q4)
        ids, tok = [], None
        for p in range(20):
            tok, _ = g.decode(int(toks[p]) if p < 12 else tok, p)
            ids.append(tok)
        _M["m"] = (gm, raw, dec, toks, logits, ids)
    return _M["m"]


def test_token_serial_bit_for_bit():
    gm, raw, dec, toks, logits, ids = model()
    gm.set_act_int8_q4(True)
    try:
        for p in range(20):
            tok, lg = gm.forward(int(toks[p]), p)
            assert np.array_equal(lg, logits[p]), "step %d: %d logits differ" % (p, int((lg != logits[p]).sum()))
            assert tok == O.argmax_bf16(logits[p])
        assert gm.a8_route_counts() == (0, 20 * N_MAT)     # a single token always takes the mat-vec
        gk, gv = gm.kv_to_host()
        assert np.array_equal(gk[:, :20], dec.k[:, :20]) and np.array_equal(gv[:, :20], dec.v[:, :20])
        # run_steps / generate take the same launches
        assert list(gm.generate(toks[:12], 8, use_graph=True)) == ids[11:19]
        assert WHY in gm.engine_why()                      # the engine refuses with the reason while the switch is on
        gm.set_engine(True)
        assert list(gm.generate(toks[:12], 8, use_graph=True)) == ids[11:19] and gm.engine_steps() <= 0
    finally:
        gm.set_act_int8_q4(False)


def batch_passes(gm, toks, n, tile_min, want_counts):
    """prefill of n tokens, then score of n + 1, on the route tile_min selects: what either leaves behind, and the route counts of each pass"""
    gm.set_a8_tile_min(tile_min)
    gm.set_act_int8_q4(True)   # the counts restart at a switch-on
    nxt, lg = gm.prefill(toks[:n])
    assert gm.a8_route_counts() == want_counts
    k, v = gm.kv_to_host()
    out = [np.array([nxt]), lg, k[:, :n].copy(), v[:, :n].copy()]
    gm.set_act_int8_q4(True)
    lp = gm.score(toks[:n + 1])
    assert gm.a8_route_counts() == want_counts
    k, v = gm.kv_to_host()
    return out + [lp.view(np.uint32), gm.logits(), k[:, :n + 1].copy(), v[:, :n + 1].copy()]


@pytest.mark.parametrize("n", [33, 70])
def test_token_batches(n):
    gm, raw, dec, toks, logits, ids = model()
    try:
        tiles = batch_passes(gm, toks, n, 2, (N_MAT, 0))
        matvec = batch_passes(gm, toks, n, -1, (0, N_MAT))
        names = ("next id", "prefill logits", "prefill K rows", "prefill V rows", "log-probs", "score logits", "score K rows", "score V rows")
        for name, a, b in zip(names, tiles, matvec):
            assert np.array_equal(a, b), "%s: %d elements differ between the tile route and the mat-vec route" % (name, int((np.asarray(a) != np.asarray(b)).sum()))
        # layer 0's K / V rows: embed, rmsnorm, quantise, the W4.A8 product, head-norm, rope -- no attention precedes them: the restatement's bits
        assert np.array_equal(tiles[2][0], dec.k[0, :n]), "%d K elements differ" % int((tiles[2][0] != dec.k[0, :n]).sum())
        assert np.array_equal(tiles[3][0], dec.v[0, :n]), "%d V elements differ" % int((tiles[3][0] != dec.v[0, :n]).sum())
        # behind the prompt attention: the token-batch bar
        ref = bf(logits[n - 1])
        err, bar = float(np.abs(bf(tiles[1]) - ref).max()), LOGIT_TOL * float(np.abs(ref).max())
        print("prefill of %d: max |logit error| %g, bar %g" % (n, err, bar))
        assert err <= bar
        lp = tiles[4].view(np.float32)
        for i in range(n):
            f = bf(logits[i]).astype(np.float64)
            want = f[toks[i + 1]] - (f.max() + np.log(np.exp(f - f.max()).sum()))
            bar = 2 * LOGIT_TOL * float(np.abs(f).max())
            assert abs(float(lp[i]) - want) <= bar, "position %d: log-prob %g against %g, bar %g" % (i, lp[i], want, bar)
        # the default threshold (32) serves this family too
        gm.set_a8_tile_min(0)
        gm.set_act_int8_q4(True)
        gm.prefill(toks[:12])
        assert gm.a8_route_counts() == (0, N_MAT)
        gm.prefill(toks[:n])
        assert gm.a8_route_counts() == (N_MAT, N_MAT)
        ppl = gm.perplexity(toks[:n + 1])
        assert np.isfinite(ppl[0]) and gm.a8_route_counts()[0] == 2 * N_MAT
    finally:
        gm.set_a8_tile_min(0)
        gm.set_act_int8_q4(False)


def test_switch_off_restores_and_refusals():
    gm, raw, dec, toks, logits, ids = model()
    before = [gm.forward(int(toks[p]), p)[1] for p in range(4)]
    nb, lb = gm.prefill(toks[:33])
    gm.set_act_int8_q4(True)
    assert not np.array_equal(gm.forward(int(toks[0]), 0)[1], before[0])   # another arithmetic (the header's deviation 1)
    gm.set_act_int8_q4(False)
    for p in range(4):
        assert np.array_equal(gm.forward(int(toks[p]), p)[1], before[p]), "step %d: switching off did not restore the bits" % p
    na, la = gm.prefill(toks[:33])
    assert na == nb and np.array_equal(la, lb)
    # the old switch keeps refusing an all-4-bit model; the new one a model without a 4-bit matrix; a hot-row mask stops both
    with pytest.raises(L.KFError, match="ternary"):
        gm.set_act_int8(True)
    cfg = synth.CONFIGS["tiny"]
    raw_t = synth.raw_weights_numpy(cfg, 7)
    tern = synth.build_from_raw(cfg, raw_t, L.T_SIGN, L.BF16)
    with pytest.raises(L.KFError, match="no layer matrix is 4-bit"):
        tern.set_act_int8_q4(True)
    tern.close()
    q4 = synth.build_from_raw(cfg, raw_t, L.Q4, L.BF16)
    hot = np.zeros(cfg["ffn"], dtype=np.int32)
    hot[::2] = 1
    q4.set_act_int8_q4(True)
    with pytest.raises(L.KFError, match="int8 activations are on"):
        q4.set_hot(0, hot)
    q4.set_act_int8_q4(False)
    q4.set_hot(0, hot)
    with pytest.raises(L.KFError, match="hot-row mask"):
        q4.set_act_int8_q4(True)
    q4.close()


def test_mixed_storage_model():
    """q | k | v | gate | up ternary, o_proj and down_proj 4-bit.  Both switches on: every matrix on its integer route, the restatement's bits.  Only the old switch on:
    what it gives today -- the 4-bit matrices on kf_rmsnorm / kf_linear.  Only the new one: the ternary matrices on the bf16-activation route."""
    cfg = dict(synth.CONFIGS["tiny"], max_seq=32)
    types = {s: (L.Q4 if s in ("o", "down") else L.T_SIGN) for s in synth.SLOTS}
    raw = synth.raw_weights_numpy(cfg, 77, w_std=0.1)
    gm = synth.build_from_raw(cfg, raw, L.T_SIGN, L.BF16)
    for li, lw in enumerate(raw["layers"]):
        for si, slot in enumerate(synth.SLOTS):
            if types[slot] == L.Q4:
                gm.set_weight(li, si, gm._ctx.quantize(synth._bf16_t(lw[slot], gm._ctx.device), L.Q4))
    gm.set_canonical(1)
    prompt = prompt_ids(cfg, 6)
    nl = cfg["n_layer"]
    try:
        for tern, q4, per_layer in ((True, True, 7), (True, False, 5), (False, True, 2)):
            gm.set_act_int8(tern)
            gm.set_act_int8_q4(q4)
            assert WHY in gm.engine_why()
            dec = Decoder(cfg, raw, types, q4=q4, tern=tern)
            for p in range(6):
                tok, lg = gm.forward(int(prompt[p]), p)
                rt, rl = dec.decode(int(prompt[p]), p)
                assert np.array_equal(lg, rl), "switches (%d, %d), step %d: %d logits differ" % (tern, q4, p, int((lg != rl).sum()))
                assert tok == rt
            assert gm.a8_route_counts() == (0, 6 * per_layer * nl)
            gk, gv = gm.kv_to_host()
            assert np.array_equal(gk[:, :6], dec.k[:, :6]) and np.array_equal(gv[:, :6], dec.v[:, :6])
            gm.set_act_int8(False)
            gm.set_act_int8_q4(False)
        # a token batch with both on: all seven matrices of a layer on the tiles, the same bits as on the mat-vecs
        outs = []
        for tile_min, want in ((2, (7 * nl, 0)), (-1, (0, 7 * nl))):
            gm.set_a8_tile_min(tile_min)
            gm.set_act_int8(True)
            gm.set_act_int8_q4(True)
            nxt, lg = gm.prefill(np.resize(prompt, 20))
            assert gm.a8_route_counts() == want
            outs.append((nxt, lg) + gm.kv_to_host())
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
    finally:
        gm.close()
