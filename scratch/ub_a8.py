"""Int8 activations against bf16 activations on 1-bit / ternary weights: kf_linear_a8, kf_act_quant_i8 and kf_linear (the yardstick: the same weights on the bf16
mat-vec, canonical order, measured in the same run) at the seven layer shapes of Qwen3-0.6B, for T_SIGN and BOOL1; then one decode step of the config-5 model (ternary
layers, bf16 head, no masks) with the switch on and off, both on the per-layer launches (set_engine(False), eager).  Every kernel sample is ONE call between two device
events behind a cache flush (a 512 MiB fill: the weights of a real step arrive cold), variants alternated, medians of 40 samples after a warm-up; an event pair around one
short kernel carries a few microseconds of its own, the same for every variant.  Usage: python scratch/ub_a8.py [out.json]"""
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
from koifish_amd.runtime import Context   # noqa: E402

SHAPES = {"q": (2048, 1024), "k": (1024, 1024), "v": (1024, 1024), "o": (1024, 2048), "gate": (3072, 1024), "up": (3072, 1024), "down": (1024, 3072)}


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
            if slot in ("v", "up"):
                continue   # the shapes of k and gate
            w = ctx.quantize((torch.randn(M, K, device=dev) * 0.02).to(torch.bfloat16), t)
            x = torch.randn(K, device=dev).to(torch.bfloat16)
            q, step = ctx.act_quant_i8(x)
            y = torch.empty(M, dtype=torch.bfloat16, device=dev)
            variants = {"kf_linear_a8": lambda: ctx.linear_a8(w, q, step, y=y), "kf_act_quant_i8": lambda: ctx.act_quant_i8(x), "kf_linear": lambda: ctx.linear(w, x, y=y)}
            ts = {k: [] for k in variants}
            for k, f in variants.items():
                for _ in range(5):
                    sample(f)
            for _ in range(40):
                for k, f in variants.items():
                    ts[k].append(sample(f))
            res = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in ts.items()}
            out["%s %s %dx%d" % (tname, slot, M, K)] = res
            print(tname, slot, M, K, json.dumps(res), flush=True)


def step(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.T_SIGN, head_type=L.BF16)
    m.set_engine(False)
    forced = np.random.default_rng(17).integers(0, cfg["vocab"], size=cfg["max_seq"]).astype(np.int32)
    m.set_forced(forced)

    def run(on, n=64, pos=256):
        m.set_act_int8(on)
        m.set_state(int(forced[0]), 0)
        m.run_steps(0, pos, use_graph=False)   # fills the cache rows, warms up
        m.sync()
        ts = []
        for _ in range(7):
            m.set_state(int(forced[pos]), pos)
            m.sync()
            t0 = time.perf_counter()
            m.run_steps(pos, n, use_graph=False)
            m.sync()
            ts.append((time.perf_counter() - t0) * 1e3 / n)
        return {"median_ms_per_step": statistics.median(ts), "min_ms_per_step": min(ts)}

    res = {}
    for _ in range(2):   # alternated
        res["a16_per_layer_eager"] = run(False)
        res["a8_per_layer_eager"] = run(True)
    m.set_act_int8(False)
    out["decode_step_pos_256"] = res
    print(json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    out = {"clock_before": clock()}
    ctx = Context(0)
    kernels(ctx, out)
    ctx.close()
    step(out)
    out["clock_after"] = clock()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
