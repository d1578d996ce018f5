"""Int8 MFMA tiles against the integer mat-vec on token batches: kf_linear_a8_tiles, kf_linear_a8 (the route it replaces) and kf_linear on the bf16-activation tiles (the
yardstick: the same weights, measured in the same run) at the layer shapes of Qwen3-0.6B, for T_SIGN and BOOL1, at nTok = 32, 128, 512, 2047; then perplexity() of 2047
tokens on the config-5-shaped model (ternary layers, bf16 head) with int8 activations on, the tile route on and off.  The protocol of scratch/ub_a8.py: every kernel sample
is ONE call between two device events behind a cache flush (a 512 MiB fill), variants alternated, medians of 40 samples after a warm-up.
Usage: python scratch/ub_a8_tiles.py [out.json] [--no-model]"""
import ctypes as C
import json
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L                  # noqa: E402
from koifish_amd import synth                     # noqa: E402
from koifish_amd.runtime import Context, _ptr     # noqa: E402

SHAPES = {"q": (2048, 1024), "k": (1024, 1024), "o": (1024, 2048), "gate": (3072, 1024), "down": (1024, 3072)}   # v has k's shape, up has gate's
NTOKS = (32, 128, 512, 2047)


def clock():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()[-12:]
    except Exception as e:   # the figure is a note, never a condition
        return [repr(e)]


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

    for tname, t in (("T_SIGN", L.T_SIGN), ("BOOL1", L.BOOL1)):
        for slot, (M, K) in SHAPES.items():
            w = ctx.quantize((torch.randn(M, K, device=dev) * 0.02).to(torch.bfloat16), t)
            d = w.desc()
            for n in NTOKS:
                x = torch.randn(n, K, device=dev).to(torch.bfloat16)
                q, step = ctx.act_quant_i8(x)
                y = torch.empty((n, M), dtype=torch.bfloat16, device=dev)
                ctx.linear_scratch(w, n)

                def bf16_tiles():
                    L.check(ctx.hip.kf_linear(ctx.h, C.byref(d), _ptr(x), _ptr(y), None, n, 1.0, 0.0, 0, None), "kf_linear")
                variants = {"kf_linear_a8_tiles": lambda: ctx.linear_a8_tiles(w, q, step, y=y), "kf_linear_a8": lambda: ctx.linear_a8(w, q, step, y=y), "kf_linear": bf16_tiles}
                ts = {k: [] for k in variants}
                for k, f in variants.items():
                    for _ in range(5):
                        sample(f)
                for _ in range(40):
                    for k, f in variants.items():
                        ts[k].append(sample(f))
                res = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in ts.items()}
                out["%s %s %dx%d nTok=%d" % (tname, slot, M, K, n)] = res
                print(tname, slot, M, K, n, json.dumps(res), flush=True)


def ppl(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.T_SIGN, head_type=L.BF16)
    toks = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)
    m.set_act_int8(True)

    def run(tile_min):
        m.set_a8_tile_min(tile_min)
        m.set_act_int8(True)   # restarts the route counts
        m.perplexity(toks)     # warm-up: buffers, first launches
        m.sync()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            p = m.perplexity(toks)
            m.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "ppl": p[0], "route_counts": m.a8_route_counts()}

    res = {}
    for _ in range(2):   # alternated
        res["tiles"] = run(0)
        res["matvec"] = run(-1)
    m.set_act_int8(False)
    out["perplexity_2047"] = res
    print(json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = {"clock_before": clock()}
    ctx = Context(0)
    kernels(ctx, out)
    ctx.close()
    if "--no-model" not in sys.argv:
        ppl(out)
    out["clock_after"] = clock()
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
