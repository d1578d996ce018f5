"""kf_linear on e4m3 block-scaled layers (kf_f8b.hip) against the same shape stored e5m2 (FMT_F8: a byte per weight, no scales -- the nearest route the storage had
before) and stored bf16, in one process: the Qwen3-0.6B and Qwen3-32B layer shapes at 1 / 16 / 128 / 512 / 2047 token rows.  Device events on the stream, every cell
warmed up, the three storages alternated window by window, the median and the minimum of the windows.  The weights of a storage are walked through up to eight copies: more than the
256 MiB cache for the 32B shapes (times from HBM); the 0.6B shapes still sit in it.
Then two models with the Qwen3-0.6B layer shapes (vocabulary cut to 32768, bf16 head), layers in this storage and in the 4-bit group storage: a decode step
(64 steps from position 1024 in one captured-graph run, wall clock around a sync) and Qwen3.perplexity of 2047 tokens.  Usage: python scratch/ub_f8b.py [out.json]"""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L          # noqa: E402
from koifish_amd import synth             # noqa: E402
from koifish_amd.runtime import Context, _ptr   # noqa: E402

SHAPES = [("0.6B q", 2048, 1024), ("0.6B o", 1024, 2048), ("0.6B gate", 3072, 1024), ("0.6B down", 1024, 3072),
          ("32B q", 8192, 5120), ("32B o", 5120, 8192), ("32B gate", 25600, 5120), ("32B down", 5120, 25600)]   # [out, in]
ROWS = [1, 16, 128, 512, 2047]
CACHE = 256 << 20


def window(ctx, f, reps):
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for i in range(reps):
        f(i)
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1) * 1e3 / reps   # us per call


def models(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"], vocab=32768, max_seq=2048)
    prompt = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)
    for name, lt in (("f8b", L.F8E4M3), ("q4", L.Q4)):
        m = synth.build_on_gpu(cfg, layer_type=lt)

        def wall(f, reps):
            ts = []
            for _ in range(reps):
                m.sync()
                t0 = time.perf_counter()
                f()
                m.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(ts), 3), round(min(ts), 3)

        def steps():
            m.set_state(1, 1024)
            m.run_steps(1024, 64)
        m.prefill(prompt[:1024])
        wall(steps, 2)
        wall(lambda: m.perplexity(prompt), 1)
        st, pp = wall(steps, 7), wall(lambda: m.perplexity(prompt), 5)
        res = {"layers": name, "decode_step_ms_median": round(st[0] / 64, 4), "decode_step_ms_min": round(st[1] / 64, 4), "ppl2047_ms_median": pp[0], "ppl2047_ms_min": pp[1],
               "engine_why": m.engine_why()}
        out.setdefault("models", []).append(res)
        print(json.dumps(res), flush=True)
        m.close()


def main():
    ctx = Context()
    dev, out = ctx.device, {"cells": []}
    if "--models" in sys.argv:
        sys.argv.remove("--models")
        models(out)
        ctx = None
    for name, M, K in SHAPES if ctx else []:
        src = (torch.randn(M, K, device=dev) * 0.05).to(torch.bfloat16)
        copies = max(1, min(8, -(-2 * CACHE // (M * K))))   # of each storage: walking them keeps the one-token stream out of the cache
        ws = {s: [ctx.quantize(src, t) for _ in range(copies)] for s, t in (("f8b", L.F8E4M3), ("e5m2", L.F8E5M2), ("bf16", L.BF16))}
        for n in ROWS:
            x = torch.randn(n, K, device=dev).to(torch.bfloat16)
            y = torch.empty(n, M, dtype=torch.bfloat16, device=dev)
            descs = {s: [w.desc() for w in v] for s, v in ws.items()}
            for w in ws["bf16"] + ws["e5m2"]:
                ctx.linear_scratch(w, n)

            def call(s):
                return lambda i: L.check(ctx.hip.kf_linear(ctx.h, C.byref(descs[s][i % copies]), _ptr(x), _ptr(y), None, n, 1.0, 0.0, 0, None), "kf_linear " + s)
            reps = 40 if n <= 128 else 10
            times = {s: [] for s in ws}
            for s in ws:
                window(ctx, call(s), reps)   # warm-up
            for _ in range(7):
                for s in ws:
                    times[s].append(window(ctx, call(s), reps))
            cell = {"shape": name, "out": M, "in": K, "rows": n}
            for s in ws:
                cell[s + "_us_median"], cell[s + "_us_min"] = round(statistics.median(times[s]), 2), round(min(times[s]), 2)
            cell["f8b_GBps"] = round(M * K / cell["f8b_us_median"] / 1e3, 1)   # weight bytes per second
            out["cells"].append(cell)
            print(json.dumps(cell), flush=True)
        del ws
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
