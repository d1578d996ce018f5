"""Token batches on the AutoAWQ layout (kf_gemm_awq.hip: MFMA tiles fed from the packed words) through kf_linear / Context.linear, against the CPU oracle's `linear`
row by row.

Exact operands: q, z in 0 .. 15, scales in {2^-6, 2^-7, 2^-8}, x integers with |x| <= 8.  Every weight (q - z) s is exact in bf16, every partial sum a multiple of 2^-8
below 15 * 8 * 2048 * 2^-6 < 2^12 for in <= 2048 -- far inside fp32's 24 bits, so ANY summation order gives the exact sum and the device must equal the oracle in every
bit (checked for the oracle itself against an fp64 product below).  Random operands (the distribution of test_gpu_ops.py's AWQ case): the bar of test_gemm_vs_oracle."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from conftest import bf16_t, close_bf16, u16
from exact_inputs import small_ints
from helpers import ids_agree_up_to_a_token_batch_near_tie, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import AWQDevWeight, Context, Qwen3
from oracle import oracle as O

pytestmark = pytest.mark.gpu
# (in, out, n): one group, one tile | three groups (an odd number of k-steps), out and n end inside a tile | the wide form plus one row | 3072 outputs, two narrow tiles
SHAPES = [(128, 64, 16), (384, 200, 33), (2048, 1024, 129), (1024, 3072, 64)]
LOGIT_TOL = 2.0 ** -6


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """(oracle weight, x [n, in] bf16 bits, oracle rows [n, out]) -- made once per (kind, shape) and shared, never written to"""
    n_in, n_out, n = shape
    rng = np.random.default_rng(n_in + n_out + n)
    q, z = rng.integers(0, 16, size=(n_in, n_out)), rng.integers(0, 16, size=(n_in // 128, n_out))
    if kind == "exact":
        s = (2.0 ** -rng.integers(6, 9, size=(n_in // 128, n_out))).astype(np.float16)
        xf = small_ints(rng, (n, n_in))
    else:
        s = rng.uniform(0.003, 0.012, size=(n_in // 128, n_out)).astype(np.float16)
        xf = rng.normal(0, 1.0, size=(n, n_in))
    ow = O.AWQWeight(n_out, n_in, O.awq_pack(q), O.awq_pack(z), s)
    x = O.f32_to_bf16(xf.astype(np.float32))
    ref = np.stack([O.linear(ow, x[t]) for t in range(n)])
    if kind == "exact":   # the oracle's own sums are the exact ones
        w = (q - np.repeat(z, 128, axis=0)).astype(np.float64) * np.repeat(s.astype(np.float64), 128, axis=0)
        assert np.array_equal(O.bf16_to_f32(ref).astype(np.float64), O.bf16_to_f32(O.f32_to_bf16((xf @ w).astype(np.float32))).astype(np.float64))
    return ow, x, ref


def dev_weight(ctx, ow):
    return AWQDevWeight(ow.ne0, ow.ne1, torch.from_numpy(ow.data.view(np.int32)).to(ctx.device), torch.from_numpy(ow.qzeros.view(np.int32)).to(ctx.device),
                        torch.from_numpy(ow.scales.view(np.int16)).to(ctx.device))


def set_knob(ctx, name, value):
    ctx.hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    assert ctx.hip.kfdbg_set_knob(name, value) == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_rows_vs_oracle(ctx, kind, shape):
    """exact operands: every bit; random operands: every row close_bf16, the bar of test_gemm_vs_oracle"""
    ow, x, ref = case(kind, shape)
    got = u16(ctx.linear(dev_weight(ctx, ow), bf16_t(x, ctx.device)))
    assert np.array_equal(got, ref) if kind == "exact" else all(close_bf16(got[t], ref[t]).all() for t in range(x.shape[0]))


def test_exact_operands_through_the_whole_epilogue(ctx):
    """alpha, beta on a prior y, bias -- then the same under a residual: the oracle's fp32 steps on the exact sums, so still every bit"""
    ow, x, _ = case("exact", SHAPES[1])
    n, n_out = x.shape[0], ow.ne0
    rng = np.random.default_rng(5)
    b, y0, res = (O.f32_to_bf16(rng.normal(0, sd, size=sz).astype(np.float32)) for sd, sz in ((0.1, n_out), (0.5, (n, n_out)), (0.5, (n, n_out))))
    want = np.stack([O.linear(ow, x[t], bias=b, alpha=0.5, beta=2.0, y=y0[t]) for t in range(n)])
    dw, dev = dev_weight(ctx, ow), ctx.device
    for r_np, w_ in ((None, want), (res, np.stack([O.add(res[t], want[t]) for t in range(n)]))):
        got = u16(ctx.linear(dw, bf16_t(x, dev), bias=bf16_t(b, dev), alpha=0.5, beta=2.0, y=bf16_t(y0, dev), residual=None if r_np is None else bf16_t(r_np, dev)))
        assert np.array_equal(got, w_), "residual" if r_np is not None else "alpha, beta, bias"


def test_the_route_is_the_tiles_and_the_knob_gives_the_loop():
    """no scratch is set: a 64-row batch runs (the per-row mat-vec refuses without one); with the knob forcing the loop and the scratch set, the loop's result -- on exact
    operands the same bits"""
    c = Context(0)
    try:
        for kind in ("random", "exact"):
            ow, x, ref = case(kind, SHAPES[3])
            dw = dev_weight(c, ow)
            d, xd = dw.desc(), bf16_t(x, c.device)
            y = torch.zeros(x.shape[0], ow.ne0, dtype=torch.bfloat16, device=c.device)
            assert c.hip.kf_set_scratch(c.h, None, C.c_size_t(0)) == 0
            c._lin_ws = None
            assert c.hip.kf_linear(c.h, C.byref(d), C.c_void_p(xd.data_ptr()), C.c_void_p(y.data_ptr()), None, x.shape[0], 1.0, 0.0, 0, None) == 0
            tiles = u16(y)
            assert np.array_equal(tiles, ref) if kind == "exact" else all(close_bf16(tiles[t], ref[t]).all() for t in range(x.shape[0]))
            set_knob(c, b"awq_route", 1)
            try:
                assert c.hip.kf_linear(c.h, C.byref(d), C.c_void_p(xd.data_ptr()), C.c_void_p(y.data_ptr()), None, x.shape[0], 1.0, 0.0, 0, None) != 0   # the loop, no scratch
                loop = u16(c.linear(dw, xd))
            finally:
                set_knob(c, b"awq_route", 0)
            assert np.array_equal(loop, tiles) if kind == "exact" else all(close_bf16(loop[t], ref[t]).all() for t in range(x.shape[0]))
    finally:
        c.close()


@pytest.mark.parametrize("front", [8, 4])   # elements before y: 16-byte aligned rows (one store per eight outputs), or not (element stores)
def test_rows_past_n_and_columns_past_out_are_left_alone(ctx, front):
    ow, x, ref = case("exact", SHAPES[1])
    n, n_out = ref.shape
    buf = torch.full((front + (n + 3) * n_out,), -7.0, dtype=torch.bfloat16, device=ctx.device)
    y = buf[front:front + n * n_out].view(n, n_out)
    ctx.linear(dev_weight(ctx, ow), bf16_t(x, ctx.device), y=y)
    got, sentinel = u16(buf), u16(torch.tensor([-7.0], dtype=torch.bfloat16))[0]
    assert np.array_equal(got[front:front + n * n_out].reshape(n, n_out), ref)
    assert (got[:front] == sentinel).all() and (got[front + n * n_out:] == sentinel).all()


HF = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj", "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
HFN = {"norm_in": "input_layernorm", "norm_post": "post_attention_layernorm", "qn": "self_attn.q_norm", "kn": "self_attn.k_norm"}


def test_a_two_layer_awq_checkpoint_prefills_scores_and_generates_on_the_tiles(tmp_path):
    """a 40-token prompt, batched prefill: every AWQ layer is a tile launch.  K/V rows and the last logits within 2^-6 max|logit| of the oracle's token-serial forward, ids
    equal up to a token-batch near tie, perplexity within the mean of the per-token bounds (tests/test_gpu_score.py)"""
    cfg = dict(synth.CONFIGS["small"], n_layer=2, vocab=1024, max_seq=64)
    raw = synth.raw_weights_numpy(cfg, 7, w_std=0.05)
    rng = np.random.default_rng(3)
    as_bf16 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)   # noqa: E731
    t = {"model.embed_tokens.weight": as_bf16(raw["embed"]), "model.norm.weight": as_bf16(raw["final_norm"])}
    ow = {"embed": O.quantize(raw["embed"], cfg["vocab"], cfg["dim"], L.BF16), "final_norm": raw["final_norm"], "layers": []}
    ow["head"] = ow["embed"]
    for i, lw in enumerate(raw["layers"]):
        d = {}
        for s, name in HF.items():
            n_out, n_in = synth.SHAPES[s](cfg)
            aw = O.AWQWeight(n_out, n_in, O.awq_pack(rng.integers(0, 16, size=(n_in, n_out))), O.awq_pack(rng.integers(0, 16, size=(n_in // 128, n_out))),
                             rng.uniform(0.002, 0.01, size=(n_in // 128, n_out)).astype(np.float16))
            d[s] = aw
            p = "model.layers.%d.%s" % (i, name)
            t[p + ".qweight"] = torch.from_numpy(aw.data.view(np.int32).reshape(n_in, n_out // 8).copy())
            t[p + ".qzeros"] = torch.from_numpy(aw.qzeros.view(np.int32).reshape(n_in // 128, n_out // 8).copy())
            t[p + ".scales"] = torch.from_numpy(aw.scales.reshape(n_in // 128, n_out).copy())
        for s, name in HFN.items():
            t["model.layers.%d.%s.weight" % (i, name)] = as_bf16(lw[s])
            d[s] = lw[s]
        ow["layers"].append(d)
    card = {"hidden_size": cfg["dim"], "num_hidden_layers": cfg["n_layer"], "num_attention_heads": cfg["n_head"], "num_key_value_heads": cfg["n_kv"],
            "head_dim": cfg["head_dim"], "intermediate_size": cfg["ffn"], "vocab_size": cfg["vocab"], "rms_norm_eps": 1e-6, "rope_theta": cfg["theta"],
            "tie_word_embeddings": True, "quantization_config": {"quant_method": "awq", "bits": 4, "group_size": 128, "version": "gemm"}}
    (tmp_path / "config.json").write_text(json.dumps(card))
    save_file(t, str(tmp_path / "model.safetensors"))
    m = Qwen3.from_hf(tmp_path, L.Q4, L.BF16, max_seq=cfg["max_seq"])
    om = O.Qwen3Oracle(cfg, ow)
    prompt, n = prompt_ids(cfg, 40), 40
    lp, bar, o_logits = [], [], None
    for pos, tok in enumerate(prompt):   # the oracle, token by token: last logits, K/V rows, log-probs of the next tokens
        _, o_logits, _ = om.decode(int(tok), pos)
        f = O.bf16_to_f32(o_logits).astype(np.float64)
        if pos + 1 < n:
            lp.append(f[int(prompt[pos + 1])] - (f.max() + np.log(np.exp(f - f.max()).sum())))
            bar.append(2 * LOGIT_TOL * np.abs(f).max())
    ok, ov = (a.copy() for a in om.kv())
    m.set_prefill_mode(1)
    _, g_logits = m.prefill(prompt)
    gl, ol = O.bf16_to_f32(g_logits), O.bf16_to_f32(o_logits)
    assert np.abs(gl - ol).max() <= LOGIT_TOL * np.abs(ol).max()
    gk, gv = m.kv_to_host()
    for g, o in ((gk, ok), (gv, ov)):
        for l in range(cfg["n_layer"]):
            a, b = O.bf16_to_f32(g[l, :n]), O.bf16_to_f32(o[l, :n])
            assert np.abs(a - b).max() <= LOGIT_TOL * np.abs(b).max(), "layer %d KV rows differ" % l
    ppl, err, nz = m.perplexity(prompt)
    assert nz == n - 1 and abs(np.log(ppl) + np.mean(lp)) <= np.mean(bar), "ppl %g vs %g" % (ppl, np.exp(-np.mean(lp)))
    ref = om.generate(prompt.tolist(), 8)
    good, why = ids_agree_up_to_a_token_batch_near_tie(om, prompt.tolist(), m.generate(prompt, 8), ref)
    assert good, why
    m.close()
