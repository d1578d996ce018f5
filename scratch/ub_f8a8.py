"""fp8 activations against the bf16-activation routes on token batches: kf_act_quant_f8 + kf_linear_f8a8 (both launches inside the timed span) against kf_linear on the
same f8e5m2 weight WITHOUT a dequant arena (bytes converted to bf16 in registers) and WITH the resident bf16 copy (kf_set_dequant_arena), at the layer shapes of
Qwen3-0.6B and Qwen3-32B, at nTok = 32, 128, 512, 2047; then perplexity() of 2047 tokens on the 0.6B-shaped f8e5m2 model, set_act_fp8 on against off with and without
resident copies.  The protocol of scratch/ub_w4a8.py: every kernel sample is ONE call sequence between two device events behind a cache flush (a 512 MiB fill), variants
alternated, medians of 30 samples after a warm-up; the model figures are medians of 5, alternated.
Usage: python scratch/ub_f8a8.py [out.json] [--no-model]"""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L                  # noqa: E402
from koifish_amd import synth                     # noqa: E402
from koifish_amd.runtime import Context, _ptr     # noqa: E402

SHAPES = {"0.6B q": (2048, 1024), "0.6B k": (1024, 1024), "0.6B o": (1024, 2048), "0.6B gate": (3072, 1024), "0.6B down": (1024, 3072),   # v has k's shape, up has gate's
          "32B q": (8192, 5120), "32B k": (1024, 5120), "32B o": (5120, 8192), "32B gate": (25600, 5120), "32B down": (5120, 25600)}
NTOKS = (32, 128, 512, 2047)
NAMES = ("f8a8", "kf_linear", "kf_linear arena")


def kernels(ctx, out):
    dev = ctx.device
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    arena = torch.empty(320 << 20, dtype=torch.uint8, device=dev)   # the largest matrix is 250 MiB as bf16
    ws_bytes = int(ctx.hip.kf_resident_scratch_bytes())

    def sample(f):
        flush.fill_(1)
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for slot, (M, K) in SHAPES.items():
        w = ctx.quantize((torch.randn(M, K, device=dev) * 0.02).to(torch.bfloat16), L.F8E5M2)
        d = w.desc()
        for n in NTOKS:
            x = torch.randn(n, K, device=dev).to(torch.bfloat16)
            q, step = ctx.act_quant_f8(x)
            y = torch.empty((n, M), dtype=torch.bfloat16, device=dev)
            need = max(int(ctx.hip.kf_linear_scratch_bytes(C.byref(d), n)), ws_bytes)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            ctx.sync()
            L.check(ctx.hip.kf_set_scratch(ctx.h, C.c_void_p(ws.data_ptr()), C.c_size_t(need)), "kf_set_scratch")

            def fp8_route():
                L.check(ctx.hip.kf_act_quant_f8(ctx.h, _ptr(x), K, None, 0.0, n, K, _ptr(q), _ptr(step)), "kf_act_quant_f8")
                L.check(ctx.hip.kf_linear_f8a8(ctx.h, C.byref(d), _ptr(q), _ptr(step), _ptr(y), None, None, n), "kf_linear_f8a8")

            def bf16_route():
                L.check(ctx.hip.kf_linear(ctx.h, C.byref(d), _ptr(x), _ptr(y), None, n, 1.0, 0.0, 0, None), "kf_linear")

            def set_arena(on):
                ctx.sync()
                L.check(ctx.hip.kf_set_dequant_arena(ctx.h, C.c_void_p(arena.data_ptr()) if on else None, C.c_size_t(arena.numel() if on else 0)), "kf_set_dequant_arena")
                if on:
                    bf16_route()   # the first meeting fills the copy: not timed
                    ctx.sync()

            def timed(name):
                if name == "kf_linear arena":
                    set_arena(True)
                    t = sample(bf16_route)
                    used = int(ctx.hip.kf_dequant_arena_used(ctx.h))
                    set_arena(False)
                    return t, used
                return sample(fp8_route if name == "f8a8" else bf16_route), 0

            ts, used = {k: [] for k in NAMES}, 0
            for k in NAMES:
                for _ in range(3):
                    timed(k)
            for _ in range(30):
                for k in NAMES:
                    t, u = timed(k)
                    ts[k].append(t)
                    used = max(used, u)
            res = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in ts.items()}
            res["arena_bytes_used"] = used   # 0: the arena route was not taken at this nTok -- the column repeats "kf_linear"
            out["%s %dx%d nTok=%d" % (slot, M, K, n)] = res
            print(slot, M, K, n, json.dumps(res), flush=True)


def ppl(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.F8E5M2, head_type=L.BF16)
    toks = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)

    def run(name):
        m.set_act_fp8(name == "f8a8")
        m.set_prefill_resident(name == "bf16 arena")
        m.perplexity(toks)     # warm-up: buffers, first launches, the resident copies
        m.sync()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            p = m.perplexity(toks)
            m.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        r = {"median_ms": statistics.median(ts), "min_ms": min(ts), "ppl": p[0], "resident_bytes": m.resident_bytes()}
        if name == "f8a8":
            r["route_counts"] = m.f8a8_route_counts()
        return r

    res = {}
    for _ in range(2):   # alternated
        for name in ("f8a8", "bf16", "bf16 arena"):
            res[name] = run(name)
    m.set_act_fp8(False)
    m.set_prefill_resident(False)
    out["perplexity_2047"] = res
    print(json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = {}
    ctx = Context(0)
    kernels(ctx, out)
    ctx.close()
    if "--no-model" not in sys.argv:
        ppl(out)
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
