"""Int8 activations for 1-bit and ternary layers on the GPU: kf_act_quant_i8, kf_linear_a8 and the model switch against a numpy restatement of the definition in
include/kf_abi.h ("int8 activations"), written in tests/a8_restate.py (shared with tests/test_a8_cpu.py) -- never the library.  The arithmetic is exact up to one ascending fp32 chain over the K / 128 groups of a row, so
every comparison of the kernels is bit for bit; only the token-batch model path, whose prompt attention sums in MFMA order, is held to the project's token-batch bar."""
import numpy as np
import pytest
import torch

from a8_restate import BITS, IntW, bf, linear_a8, quant_rows, to_bf
from helpers import oracle_model, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FILL = 0x7fc1          # a bf16 NaN pattern no kernel stores
LOGIT_TOL = 2.0 ** -6  # tests/test_gpu_prefill.py


def t_bf16(u16, dev):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).to(dev).view(torch.bfloat16)


def u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def special_rows(dim):
    """the tie, zero and negative-maximum rows of tests/test_a8_cpu.py"""
    tie = np.zeros(dim, dtype=np.float32)
    tie[:8] = (127.0, 0.5, -0.5, 2.5, -2.5, 126.5, 1.5, -126.5)
    neg = np.full(dim, -0.25, dtype=np.float32)
    neg[3], neg[5] = -8.0, 2.0
    return [to_bf(tie), np.zeros(dim, dtype=np.uint16), to_bf(neg)]


# ---------------------------------------------------------------- 1. the quantiser
@pytest.mark.parametrize("dim", [128, 1024, 3072])
@pytest.mark.parametrize("rows", [1, 3])
def test_quantiser(ctx, dim, rows):
    rng = np.random.default_rng(dim + rows)
    cases = [to_bf(rng.normal(0, 1.5, (rows, dim)).astype(np.float32))]
    sp = special_rows(dim)
    cases += [np.stack([sp[(i + r) % 3] for r in range(rows)]) for i in range(3)]
    for x in cases:
        wide = torch.zeros((rows, dim + 40), dtype=torch.bfloat16, device=ctx.device)   # a row stride larger than the dim
        wide[:, :dim] = t_bf16(x, ctx.device)
        q, step = ctx.act_quant_i8(wide[:, :dim])
        ctx.sync()
        rq, rs = quant_rows(x)
        assert np.array_equal(step.cpu().numpy().view(np.uint32), rs.view(np.uint32))
        assert np.array_equal(q.cpu().numpy(), rq)
    # the norm prologue = kf_rmsnorm followed by the plain call = the restatement on O.rmsnorm
    x = cases[0]
    nw = to_bf((1.0 + rng.normal(0, 0.1, dim)).astype(np.float32))
    dx, dw = t_bf16(x, ctx.device), t_bf16(nw, ctx.device)
    q1, s1 = ctx.act_quant_i8(dx, norm_w=dw, eps=1e-6)
    q2, s2 = ctx.act_quant_i8(ctx.rmsnorm(dx, dw, 1e-6))
    ctx.sync()
    rq, rs = quant_rows(O.rmsnorm(x, nw, 1e-6))
    assert torch.equal(q1, q2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert np.array_equal(q1.cpu().numpy(), rq) and np.array_equal(s1.cpu().numpy().view(np.uint32), rs.view(np.uint32))


# ---------------------------------------------------------------- 2. the product
_W = {}


def weight(ctx, type_, M, K, seed=5):
    """one quantised weight per (type, shape): the oracle's quantiser, uploaded; the integer restatement beside it"""
    key = (type_, M, K, seed)
    if key not in _W:
        w = to_bf(np.random.default_rng(seed + M + K).normal(0, 0.05, (M, K)).astype(np.float32))
        ow = O.quantize(w, M, K, type_)
        _W[key] = (ow, ctx.upload_blob(type_, M, K, ow.blob()), IntW(ow))
    return _W[key]


def run_a8(ctx, dw, q, step, bias=None, residual=None):
    n, M = q.shape[0], dw.ne0
    y = t_bf16(np.full((n, M), FILL, dtype=np.uint16), ctx.device)
    dq, ds = torch.from_numpy(q).to(ctx.device), torch.from_numpy(step).to(ctx.device)
    ctx.linear_a8(dw, dq, ds, bias=None if bias is None else t_bf16(bias, ctx.device), residual=None if residual is None else t_bf16(residual, ctx.device), y=y)
    ctx.sync()
    return u16(y)


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1, L.T_BINARY])
@pytest.mark.parametrize("M,K", [(1, 128), (7, 384), (64, 1024), (257, 3072)])
def test_product(ctx, type_, M, K):
    ow, dw, iw = weight(ctx, type_, M, K)
    rng = np.random.default_rng(M * K)
    x9 = to_bf(rng.normal(0, 1, (9, K)).astype(np.float32))
    q9, s9 = quant_rows(x9)
    ref9 = linear_a8(iw, q9, s9)
    for n in (1, 2, 5, 9):
        got = run_a8(ctx, dw, q9[:n], s9[:n])
        assert not (got == FILL).any(), "an output element kept the fill value"
        assert np.array_equal(got, ref9[:n]), "nTok = %d: %d of %d outputs differ" % (n, int((got != ref9[:n]).sum()), got.size)
    # the rows of nTok = 9 are the same rows computed one at a time
    one = np.concatenate([run_a8(ctx, dw, q9[t:t + 1], s9[t:t + 1]) for t in range(9)])
    assert np.array_equal(one, run_a8(ctx, dw, q9, s9))
    # bias, and the residual epilogue
    bias = to_bf(rng.normal(0, 0.5, M).astype(np.float32))
    res = to_bf(rng.normal(0, 1, (5, M)).astype(np.float32))
    assert np.array_equal(run_a8(ctx, dw, q9[:5], s9[:5], bias=bias), linear_a8(iw, q9[:5], s9[:5], bias=bias))
    assert np.array_equal(run_a8(ctx, dw, q9[:5], s9[:5], residual=res), linear_a8(iw, q9[:5], s9[:5], residual=res))
    assert np.array_equal(run_a8(ctx, dw, q9[:1], s9[:1], bias=bias, residual=res[:1]), linear_a8(iw, q9[:1], s9[:1], bias=bias, residual=res[:1]))


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1])
def test_product_saturating(ctx, type_):
    """every q = +-127 against all-ones 1-bit weights, all-+1 / all--1 ternary groups: |I_g| = 16 256, where overflow of a narrower intermediate shows"""
    M, K = 8, 384
    G = K // 128
    codes = np.ones((M, G, 128), dtype=np.int32)
    if type_ == L.T_SIGN:
        codes[:] = 2                      # t_w = +1
        codes[1::2, :, :] = 0             # t_w = -1 in every other row
        codes[2, 1, :] = 1                # one all-zero group
    step_w = to_bf(np.random.default_rng(9).uniform(0.01, 0.2, M * G).astype(np.float32))
    ow = O.QWeight(type_, M, K, O.pack(codes, BITS[type_]), np.zeros(M * G, dtype=np.uint16), step_w, 128, 1 if type_ == L.T_SIGN else 0)
    dw, iw = ctx.upload_blob(type_, M, K, ow.blob()), IntW(ow)
    q = np.full((5, K), 127, dtype=np.int8)
    q[1] = -127
    q[2, ::2] = -127
    q[3, 128:256] = -127
    step = np.array([1.0, 0.37, 2.5e-3, 11.0, 1.0], dtype=np.float32)
    I = np.einsum("mgc,tgc->tmg", iw.t.reshape(M, G, 128), q.astype(np.int64).reshape(5, G, 128))
    assert np.abs(I).max() == 16256
    got = run_a8(ctx, dw, q, step)
    assert not (got == FILL).any() and np.array_equal(got, linear_a8(iw, q, step))
    assert np.array_equal(run_a8(ctx, dw, q[:1], step[:1]), linear_a8(iw, q[:1], step[:1]))


# ---------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("type_", [L.Q4, L.BF16])
def test_refusals(ctx, type_):
    M, K = 16, 256
    w = to_bf(np.random.default_rng(3).normal(0, 0.05, (M, K)).astype(np.float32))
    dw = ctx.upload_blob(type_, M, K, O.quantize(w, M, K, type_).blob())
    q = torch.zeros((1, K), dtype=torch.int8, device=ctx.device)
    step = torch.ones(1, dtype=torch.float32, device=ctx.device)
    with pytest.raises(L.KFError) as e:
        ctx.linear_a8(dw, q, step)
    assert "code -1000" in str(e.value) and ("type %d" % type_) in str(e.value)


# ---------------------------------------------------------------- 4 - 6. the model
class A8Decoder:
    """A Qwen3 decoder from the oracle's own ops in SURVEY section 9's op order, the restated quantiser and product in place of the seven linears"""

    def __init__(self, cfg, raw, layer_type):
        self.c = cfg
        q = lambda a, t: O.quantize(a, a.shape[0], a.shape[1], t)
        self.embed = q(raw["embed"], L.BF16)
        self.final_norm = raw["final_norm"]
        self.layers = []
        types = layer_type if isinstance(layer_type, dict) else {s: layer_type for s in synth.SLOTS}
        for lw in raw["layers"]:
            d = {s: (IntW(q(lw[s], types[s])) if types[s] in BITS else q(lw[s], types[s])) for s in synth.SLOTS}   # other storages keep the oracle's bf16-activation linear
            d.update({s: lw[s] for s in synth.NORMS})
            self.layers.append(d)
        kvd = cfg["n_kv"] * cfg["head_dim"]
        self.k = np.zeros((cfg["n_layer"], cfg["max_seq"], kvd), dtype=np.uint16)
        self.v = np.zeros_like(self.k)

    def mv(self, w, x, qx, sx):
        return linear_a8(w, qx, sx)[0] if isinstance(w, IntW) else O.linear(w, x)

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


CFG = dict(synth.CONFIGS["small"], max_seq=32)
_M = {}


def model(layer_type):
    """the 3-layer test shape with `layer_type` layers and a bf16 head, the restatement's 12 forced + 8 greedy steps beside it: built once per type"""
    if layer_type not in _M:
        raw = synth.raw_weights_numpy(CFG, 1234, w_std=0.1)
        gm = synth.build_from_raw(CFG, raw, layer_type, L.BF16)
        gm.set_canonical(1)
        dec = A8Decoder(CFG, raw, layer_type)
        prompt = prompt_ids(CFG, 12)
        ids, logits, tok = [], [], None
        for p in range(20):
            tok, lg = dec.decode(int(prompt[p]) if p < 12 else tok, p)
            ids.append(tok), logits.append(lg)
        _M[layer_type] = (gm, raw, dec, prompt, ids, logits)
    return _M[layer_type]


@pytest.mark.parametrize("layer_type", [L.T_SIGN, L.BOOL1])
def test_model_token_serial_bit_for_bit(layer_type):
    gm, raw, dec, prompt, ids, logits = model(layer_type)
    gm.set_act_int8(True)
    tok = None
    for p in range(20):
        tok, lg = gm.forward(int(prompt[p]) if p < 12 else tok, p)
        assert np.array_equal(lg, logits[p]), "step %d: %d logits differ" % (p, int((lg != logits[p]).sum()))
        assert tok == ids[p]
    gk, gv = gm.kv_to_host()
    assert np.array_equal(gk[:, :20], dec.k[:, :20]) and np.array_equal(gv[:, :20], dec.v[:, :20])
    # run_steps / generate take the same launches
    assert gm.generate(prompt, 8, use_graph=True) == ids[11:19]
    gm.set_act_int8(False)


def test_model_batch_route():
    gm, raw, dec, prompt, ids, logits = model(L.T_SIGN)
    gm.set_act_int8(True)
    nxt, lg = gm.prefill(prompt)
    gk, gv = gm.kv_to_host()
    assert np.array_equal(gk[0, :12], dec.k[0, :12]) and np.array_equal(gv[0, :12], dec.v[0, :12])   # no attention precedes layer 0's K / V rows
    ref = bf(logits[11])
    err, bar = float(np.abs(bf(lg) - ref).max()), LOGIT_TOL * float(np.abs(ref).max())
    print("prefill: max |logit error| %g, bar %g" % (err, bar))
    assert err <= bar
    toks = np.concatenate([prompt, np.asarray(ids[11:19], dtype=np.int32)])   # the 20 tokens the restatement decoded
    lp = gm.score(toks)
    for i in range(19):
        f = bf(logits[i]).astype(np.float64)
        want = f[toks[i + 1]] - (f.max() + np.log(np.exp(f - f.max()).sum()))
        bar = 2 * LOGIT_TOL * float(np.abs(f).max())
        assert abs(float(lp[i]) - want) <= bar, "position %d: log-prob %g against %g, bar %g" % (i, lp[i], want, bar)
    gm.set_act_int8(False)


def test_switch():
    gm, raw, dec, prompt, ids, logits = model(L.T_SIGN)
    # off: today's logits
    O.set_order(O.ORDER_CANON)
    try:
        om = oracle_model(CFG, raw, L.T_SIGN, L.BF16, attn_mode=O.ATTN_CANON)
        for p in range(4):
            t, lg = gm.forward(int(prompt[p]), p)
            ot, olg, _ = om.decode(int(prompt[p]), p)
            assert t == ot and np.array_equal(lg, olg)
        om.close()
    finally:
        O.set_order(O.ORDER_DOT16)
    # on: the engine is not served and says why; set_engine(True) still decodes, on the per-layer launches
    gm.set_act_int8(True)
    assert "int8 activations run on the per-layer launches" in gm.engine_why()
    gm.set_engine(True)
    assert gm.generate(prompt, 8, use_graph=True) == ids[11:19]
    assert gm.engine_steps() <= 0
    gm.set_act_int8(False)
    # refusals with the reason
    raw_t = synth.raw_weights_numpy(synth.CONFIGS["tiny"], 7)
    q4 = synth.build_from_raw(synth.CONFIGS["tiny"], raw_t, L.Q4, L.BF16)
    with pytest.raises(L.KFError, match="ternary"):
        q4.set_act_int8(True)
    q4.close()
    tern = synth.build_from_raw(synth.CONFIGS["tiny"], raw_t, L.T_SIGN, L.BF16)
    hot = np.zeros(synth.CONFIGS["tiny"]["ffn"], dtype=np.int32)
    hot[::2] = 1
    tern.set_act_int8(True)
    with pytest.raises(L.KFError, match="int8 activations are on"):   # a mask while the switch is on: refused with the reason, nothing changes
        tern.set_hot(0, hot)
    tern.set_act_int8(False)
    tern.set_hot(0, hot)
    with pytest.raises(L.KFError, match="hot-row mask"):
        tern.set_act_int8(True)
    tern.close()


def test_mixed_storage_model():
    """q | k | v | gate | up ternary, o_proj and down_proj 4-bit: the ternary matrices take int8 activations, the 4-bit ones keep kf_rmsnorm / kf_linear with the residual
    epilogue (Fish::A8Group's other branch) -- token-serial bit for bit, the token batch within the token-batch bar"""
    cfg = dict(synth.CONFIGS["tiny"], max_seq=32)
    types = {s: (L.Q4 if s in ("o", "down") else L.T_SIGN) for s in synth.SLOTS}
    raw = synth.raw_weights_numpy(cfg, 77, w_std=0.1)
    gm = synth.build_from_raw(cfg, raw, L.T_SIGN, L.BF16)
    for li, lw in enumerate(raw["layers"]):
        for si, slot in enumerate(synth.SLOTS):
            if types[slot] == L.Q4:
                gm.set_weight(li, si, gm._ctx.quantize(synth._bf16_t(lw[slot], gm._ctx.device), L.Q4))
    gm.set_canonical(1)
    gm.set_act_int8(True)
    dec = A8Decoder(cfg, raw, types)
    prompt = prompt_ids(cfg, 10)
    want = []
    for p in range(10):
        tok, lg = gm.forward(int(prompt[p]), p)
        rt, rl = dec.decode(int(prompt[p]), p)
        want.append(rl)
        assert np.array_equal(lg, rl), "step %d: %d logits differ" % (p, int((lg != rl).sum()))
        assert tok == rt
    gk, gv = gm.kv_to_host()
    assert np.array_equal(gk[:, :10], dec.k[:, :10]) and np.array_equal(gv[:, :10], dec.v[:, :10])
    nxt, lg = gm.prefill(prompt)
    ref = bf(want[9])
    assert float(np.abs(bf(lg) - ref).max()) <= LOGIT_TOL * float(np.abs(ref).max())
    gm.close()


def test_norm_prologue_refuses_what_rmsnorm_refuses(ctx):
    x = torch.zeros(129, dtype=torch.bfloat16, device=ctx.device)
    with pytest.raises(L.KFError, match="code -2100"):
        ctx.act_quant_i8(x, norm_w=x)
    with pytest.raises(L.KFError, match="code -2100"):
        ctx.rmsnorm(x, x)
    q, step = ctx.act_quant_i8(x)   # without the prologue an odd dim is served
    assert not q.any().item()
