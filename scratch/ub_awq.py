"""kf_linear on AutoAWQ layers, three routes inside one process: the MFMA tiles of kf_gemm_awq.hip, the per-row mat-vec loop they replace (kfdbg_set_knob "awq_route" 1: the
parent's own route), and kf_dequant -> transpose -> the bf16 tile kernels (the copy kf_dequant leaves is [in, out]; the bf16 kernels want [out, in], so this route pays a
transpose the other two do not; the bf16 product alone on a copy that already exists is listed beside it).  Then Qwen3.perplexity of 2047 tokens on a model with the
Qwen3-0.6B layer shapes in AWQ storage (vocabulary cut to 32768: the head is bf16 either way), tiles against the loop.  Device events on the stream, every cell warmed up,
routes alternated, medians and minima of repeated windows.  Usage: python scratch/ub_awq.py [out.json]"""
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L          # noqa: E402
from koifish_amd import synth             # noqa: E402
from koifish_amd.runtime import AWQDevWeight, Context, Qwen3, _ptr   # noqa: E402

SHAPES = [(1024, 1024), (2048, 1024), (3072, 1024), (1024, 3072), (9728, 2560)]   # [out, in]: the Qwen3-0.6B layers, and gate / up of Qwen3-4B
ROWS = [16, 64, 512, 2047]
HF = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj", "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
HFN = {"norm_in": "input_layernorm", "norm_post": "post_attention_layernorm", "qn": "self_attn.q_norm", "kn": "self_attn.k_norm"}


def awq_tensors(rng, n_out, n_in):
    qw = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(n_in, n_out // 8), dtype=np.int64).astype(np.int32))
    qz = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(n_in // 128, n_out // 8), dtype=np.int64).astype(np.int32))
    sc = torch.from_numpy(rng.uniform(0.003, 0.012, size=(n_in // 128, n_out)).astype(np.float16))
    return qw, qz, sc


def window(ctx, f, reps):
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        f()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / reps   # us per call


def operators(ctx, out):
    dev, rng = ctx.device, np.random.default_rng(1)
    ctx.hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    for n_out, n_in in SHAPES:
        qw, qz, sc = awq_tensors(rng, n_out, n_in)
        dw = AWQDevWeight(n_out, n_in, qw.to(dev), qz.to(dev), sc.view(torch.int16).to(dev))
        d = dw.desc()
        ctx.linear_scratch(dw, 1)
        copy = torch.empty(n_in, n_out, dtype=torch.bfloat16, device=dev)
        for n in ROWS:
            x = torch.randn(n, n_in, device=dev).to(torch.bfloat16)
            y = torch.empty(n, n_out, dtype=torch.bfloat16, device=dev)

            def tiles():
                L.check(ctx.hip.kf_linear(ctx.h, C.byref(d), _ptr(x), _ptr(y), None, n, 1.0, 0.0, 0, None), "kf_linear")

            def loop():
                ctx.hip.kfdbg_set_knob(b"awq_route", 1)
                tiles()
                ctx.hip.kfdbg_set_knob(b"awq_route", 0)

            def deq_bf16():
                L.check(ctx.hip.kf_dequant(ctx.h, C.byref(d), _ptr(copy)), "kf_dequant")
                wb = ctx.quantize(copy.t().contiguous(), L.BF16)
                db = wb.desc()
                L.check(ctx.hip.kf_linear(ctx.h, C.byref(db), _ptr(x), _ptr(y), None, n, 1.0, 0.0, 0, None), "kf_linear bf16")

            deq_bf16()
            wres = ctx.quantize(copy.t().contiguous(), L.BF16)
            dres = wres.desc()

            def bf16_only():
                L.check(ctx.hip.kf_linear(ctx.h, C.byref(dres), _ptr(x), _ptr(y), None, n, 1.0, 0.0, 0, None), "kf_linear bf16")

            variants = {"tiles": (tiles, 50), "loop": (loop, 50 if n <= 64 else 3), "dequant_transpose_bf16": (deq_bf16, 20), "bf16_on_a_resident_copy": (bf16_only, 50)}
            tiles()
            t_y = y.clone()
            loop()
            ctx.sync()
            diff = float((t_y.float() - y.float()).abs().max() / y.float().abs().max())
            for f, _ in variants.values():
                window(ctx, f, 2)
            t = {k: [] for k in variants}
            for _ in range(5):
                for k, (f, reps) in variants.items():
                    t[k].append(window(ctx, f, reps))
            res = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)} for k, v in t.items()}
            res["tiles_vs_loop_max_rel_diff"] = diff
            out["%dx%d_n%d" % (n_out, n_in, n)] = res
            print(n_out, n_in, n, json.dumps(res), flush=True)


def model(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"], vocab=32768, max_seq=2048)
    rng = np.random.default_rng(2)
    bf = lambda *s: (torch.randn(*s) * 0.02).to(torch.bfloat16)   # noqa: E731
    t = {"model.embed_tokens.weight": bf(cfg["vocab"], cfg["dim"]), "model.norm.weight": torch.ones(cfg["dim"], dtype=torch.bfloat16)}
    for i in range(cfg["n_layer"]):
        for s, name in HF.items():
            n_out, n_in = synth.SHAPES[s](cfg)
            p = "model.layers.%d.%s" % (i, name)
            t[p + ".qweight"], t[p + ".qzeros"], t[p + ".scales"] = awq_tensors(rng, n_out, n_in)
        for s, name in HFN.items():
            t["model.layers.%d.%s.weight" % (i, name)] = torch.ones(cfg["head_dim"] if s in ("qn", "kn") else cfg["dim"], dtype=torch.bfloat16)
    card = {"hidden_size": cfg["dim"], "num_hidden_layers": cfg["n_layer"], "num_attention_heads": cfg["n_head"], "num_key_value_heads": cfg["n_kv"],
            "head_dim": cfg["head_dim"], "intermediate_size": cfg["ffn"], "vocab_size": cfg["vocab"], "rms_norm_eps": 1e-6, "rope_theta": cfg["theta"],
            "tie_word_embeddings": True, "quantization_config": {"quant_method": "awq", "bits": 4, "group_size": 128, "version": "gemm"}}
    from safetensors.torch import save_file
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / "config.json").write_text(json.dumps(card))
        save_file(t, str(Path(tmp) / "model.safetensors"))
        m = Qwen3.from_hf(Path(tmp), L.Q4, L.BF16, max_seq=cfg["max_seq"])
    m.hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    prompt = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)

    def timed(knob, reps):
        m.hip.kfdbg_set_knob(b"awq_route", knob)
        ts, ppl = [], None
        for _ in range(reps):
            m.sync()
            t0 = time.perf_counter()
            ppl = m.perplexity(prompt)[0]
            m.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        m.hip.kfdbg_set_knob(b"awq_route", 0)
        return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "ppl": float(ppl)}

    timed(0, 1)
    res = {"tiles": timed(0, 5), "loop": timed(1, 2), "tiles_again": timed(0, 5)}
    out["perplexity_2047"] = res
    print(json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    out = {}
    ctx = Context(0)
    operators(ctx, out)
    ctx.close()
    model(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
