"""kf_head_logprob on the Qwen3-0.6B head (151 936 x 1024 bf16) against the route a user has without it: kf_linear into a materialised [rows x V] bf16 matrix, then
torch.logsumexp and a gather on it.  Then Qwen3.score of a 2047-token prompt against Qwen3.prefill of the same prompt and against 2047 forward() calls with a host
log-softmax.  Device events on the stream, warm-up of every shape, variants alternated inside one process, medians (and minima) of repeated windows; the clock is read
before and after.  Usage: python scratch/ub_score.py [out.json]"""
import ctypes as C
import json
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L          # noqa: E402
from koifish_amd import synth             # noqa: E402
from koifish_amd.runtime import Context, _ptr   # noqa: E402

V, D = 151936, 1024
PEAK_BF16 = 2.5e15   # dense bf16, MI355X


def clock():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()[-12:]
    except Exception as e:   # the figure is a note, never a condition
        return [repr(e)]


def window(ctx, f, reps):
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(reps):
        f()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / reps   # us per call


def head(ctx, out):
    dev = ctx.device
    ctx.hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    w = ctx.quantize((torch.randn(V, D, device=dev) * 0.02).to(torch.bfloat16), L.BF16)
    d = w.desc()
    for rows in (128, 512, 2047):
        x = torch.randn(rows, D, device=dev).to(torch.bfloat16)
        tg = torch.randint(0, V, (rows,), device=dev, dtype=torch.int32)
        tg64 = tg.to(torch.int64)
        lp = torch.empty(rows, dtype=torch.float32, device=dev)
        lse = torch.empty(rows, dtype=torch.float32, device=dev)
        top1 = torch.empty(rows, dtype=torch.int32, device=dev)
        ws = torch.empty(rows * 1187 * 16 + 256, dtype=torch.uint8, device=dev)
        logits = torch.empty(rows, V, dtype=torch.bfloat16, device=dev)

        def fused():
            L.check(ctx.hip.kf_head_logprob(ctx.h, C.byref(d), _ptr(x), D, rows, _ptr(tg), _ptr(lp), _ptr(lse), _ptr(top1), _ptr(ws)), "kf_head_logprob")

        def fused_form(form):
            def f():
                ctx.hip.kfdbg_set_knob(b"score_form", form)
                fused()
                ctx.hip.kfdbg_set_knob(b"score_form", -1)
            return f

        def materialised():
            L.check(ctx.hip.kf_linear(ctx.h, C.byref(d), _ptr(x), _ptr(logits), None, rows, 1.0, 0.0, 0, None), "kf_linear")
            f = logits.float()
            return f.gather(1, tg64[:, None])[:, 0] - torch.logsumexp(f, dim=1)

        def gemm_only():
            L.check(ctx.hip.kf_linear(ctx.h, C.byref(d), _ptr(x), _ptr(logits), None, rows, 1.0, 0.0, 0, None), "kf_linear")

        variants = {"fused": fused, "fused_128": fused_form(1), "fused_256": fused_form(0), "materialised": materialised, "kf_linear_only": gemm_only}
        ref = materialised()
        fused()
        ctx.sync()
        err = float((lp - ref).abs().max())
        reps = 20 if rows >= 2047 else 50
        for f in variants.values():
            window(ctx, f, 3)
        t = {k: [] for k in variants}
        for _ in range(9):   # alternate the variants: nine windows each
            for k, f in variants.items():
                t[k].append(window(ctx, f, reps))
        res = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in t.items()}
        flop = 2.0 * rows * V * D
        for k in ("fused", "fused_128", "fused_256"):
            res[k]["mfma_fraction"] = flop / (res[k]["median_us"] * 1e-6) / PEAK_BF16
        res["max_abs_diff_vs_materialised"] = err
        out["head_rows_%d" % rows] = res
        print(rows, json.dumps(res), flush=True)
        del logits


def model(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.Q4, head_type=L.BF16)
    prompt = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)

    def timed(f, n):
        ts = []
        for _ in range(n):
            m.sync()
            t0 = time.perf_counter()
            f()
            m.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts)}

    m.prefill(prompt, want_logits=False)
    m.score(prompt)
    res = {}
    for _ in range(2):   # alternated; host clock around calls that end in a device synchronise (both copy their results back)
        res["prefill_2047"] = timed(lambda: m.prefill(prompt, want_logits=False), 7)
        res["score_2047"] = timed(lambda: m.score(prompt), 7)

    def serial():
        lp = []
        for pos in range(2046):
            _, logits = m.forward(int(prompt[pos]), pos)
            f = (logits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
            mx = f.max()
            lp.append(f[int(prompt[pos + 1])] - (mx + np.log(np.exp(f - mx).sum())))
        return lp

    res["forward_x2046_host_logsoftmax"] = timed(serial, 1)
    out["model"] = res
    print(json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    out = {"clock_before": clock()}
    ctx = Context(0)
    head(ctx, out)
    ctx.close()
    model(out)
    out["clock_after"] = clock()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
