"""NF3 layers multiplied from the packed stream (kf_set_row_unpack) against what they replace and against their neighbours, all in one run:
  one token, per matrix   kf_linear on an NF3 weight with the switch on and off (off = dequantise into the scratch + the bf16 mat-vec, the same binary), and the NF4 and
                          4-bit group mat-vecs on the same shape, at the layer shapes of Qwen3-0.6B and the 32B down_proj (5120 x 25600); GB/s over the algorithmic
                          bytes of the NF3 form (stream + tables + x + y) resp. each storage's own
  decode step             a 0.6B-shaped model at 2 k context on the per-layer launches (captured graph, no engine) with NF3, NF4 and 4-bit group layers
  perplexity              2047 tokens, NF3 against NF4
Every kernel sample is ONE call between two device events behind a cache flush (a 512 MiB fill), variants alternated, medians of 40 samples after a warm-up; an event
pair around one short kernel carries a few microseconds of its own, the same for every variant.  Usage: python scratch/ub_rowq.py [out.json]"""
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L          # noqa: E402
from koifish_amd import synth             # noqa: E402
from koifish_amd.runtime import Context   # noqa: E402

SHAPES = {"q": (2048, 1024), "k|v": (1024, 1024), "o": (1024, 2048), "gate|up": (3072, 1024), "down": (1024, 3072), "32B down": (5120, 25600)}


def kernels(ctx, out):
    dev = ctx.device
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def sample(f):
        flush.fill_(1)
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for slot, (M, K) in SHAPES.items():
        src = (torch.randn(M, K, device=dev) * 0.02).to(torch.bfloat16)
        w3, w4, wg = ctx.quantize(src, L.NF3), ctx.quantize(src, L.NF4), ctx.quantize(src, L.Q4)
        x = torch.randn(K, device=dev).to(torch.bfloat16)
        y = torch.empty(M, dtype=torch.bfloat16, device=dev)
        ctx.linear_scratch(w3, 1)

        def nf3(on):
            ctx.set_row_unpack(on)
            ctx.linear(w3, x, y=y)
        variants = {"nf3_on": lambda: nf3(1), "nf3_off": lambda: nf3(0), "nf4": lambda: ctx.linear(w4, x, y=y), "q4_group": lambda: ctx.linear(wg, x, y=y)}
        bytes_ = {"nf3_on": M * K * 3 // 8 + 16 * M + 2 * K + 2 * M, "nf4": M * K // 2 + 32 * M + 2 * K + 2 * M, "q4_group": M * K // 2 + 4 * (M * K // 128) + 2 * K + 2 * M}
        bytes_["nf3_off"] = bytes_["nf3_on"]   # the same algorithm's bytes: what the route moves on top of them is the point
        ts = {k: [] for k in variants}
        for k, f in variants.items():
            for _ in range(5):
                sample(f)
        for _ in range(40):
            for k, f in variants.items():
                ts[k].append(sample(f))
        ctx.set_row_unpack(0)
        res = {k: {"median_us": statistics.median(v), "min_us": min(v), "p90_us": sorted(v)[35], "GBps": bytes_[k] / statistics.median(v) * 1e-3} for k, v in ts.items()}
        out["%s %dx%d" % (slot, M, K)] = res
        print(slot, M, K, json.dumps(res), flush=True)


def models(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    forced = np.random.default_rng(17).integers(0, cfg["vocab"], size=cfg["max_seq"]).astype(np.int32)
    pos, n = 1984, 48
    for name, t in (("nf3", L.NF3), ("nf4", L.NF4), ("q4_group", L.Q4)):
        m = synth.build_on_gpu(cfg, seed=1234, layer_type=t, head_type=L.BF16)
        m.set_engine(False)
        m.set_forced(forced)
        m.set_state(int(forced[0]), 0)
        m.run_steps(0, pos, use_graph=True)   # fills the cache rows, warms up
        m.sync()
        ts = []
        for _ in range(7):
            m.set_state(int(forced[pos]), pos)
            m.sync()
            t0 = time.perf_counter()
            m.run_steps(pos, n, use_graph=True)
            m.sync()
            ts.append((time.perf_counter() - t0) * 1e3 / n)
        res = {"median_ms_per_step": statistics.median(ts), "min_ms_per_step": min(ts), "max_ms_per_step": max(ts)}
        if t != L.Q4:
            tp = []
            m.perplexity(forced[:2047])
            for _ in range(5):
                m.sync()
                t0 = time.perf_counter()
                m.perplexity(forced[:2047])
                m.sync()
                tp.append((time.perf_counter() - t0) * 1e3)
            res["perplexity_2047_ms"] = {"median": statistics.median(tp), "min": min(tp), "max": max(tp)}
        out["model %s" % name] = res
        print(name, json.dumps(res), flush=True)
        m.close()


if __name__ == "__main__":
    out = {}
    ctx = Context(0)
    kernels(ctx, out)
    ctx.close()
    models(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
