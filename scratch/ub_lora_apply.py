"""Adapters at inference, timed in one run on a synthetic Qwen3-0.6B (4-bit layers), rank 16 and 64:
  vec     kf_lora_apply's vector form alone, one launch per group that shares an input row: q | k | v (2048 / 1024 / 1024 x 1024), gate | up (3072 x 1024 twice),
          down (1024 x 3072); beside it the kf_linear mat-vecs of the same matrices, which the adapters stand behind
  decode  one decode step around position 1000: the engine, the per-layer launches without adapters (set_engine(False)), and adapters on all seven matrices
  ppl     perplexity of 2047 tokens without and with the adapters (the tile form, one launch per adapted matrix)
Each figure is the mean of REPS calls, measured ROUNDS times: printed are the median and the spread (max - min) over the rounds.  The decode and perplexity figures are
host clocks around work that ends in a synchronise (the per-layer decode is bound by its launches, not by the kernels)."""
import os, sys, ctypes as C, statistics, time, torch
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koifish_amd.runtime import Context
from koifish_amd import lib as L, synth
from koifish_amd.train_step import Q3_MATS, Qwen3Step
ctx = Context(0); dev = ctx.device; hip = ctx.hip
bf = torch.bfloat16
cfg = synth.CONFIGS["qwen3-0.6b"]
shapes = Qwen3Step._mat_shapes(cfg)
rnd = lambda *s: (torch.randn(*s, device=dev) * 0.02).to(bf)


def timed(fn, reps=20, rounds=5):
    for _ in range(3): fn()
    out = []
    for _ in range(rounds):
        ctx.sync(); e0, e1 = ctx.event(), ctx.event(); ctx.record(e0)
        for _ in range(reps): fn()
        ctx.record(e1); ctx.sync(); out.append(ctx.elapsed_ms(e0, e1) / reps * 1e3)
    return statistics.median(out), max(out) - min(out)


def wall(fn, sync, reps, rounds=5):
    fn(); sync()
    out = []
    for _ in range(rounds):
        sync(); t0 = time.perf_counter()
        for _ in range(reps): fn()
        sync(); out.append((time.perf_counter() - t0) / reps * 1e6)
    return statistics.median(out), max(out) - min(out)


print("%-10s %-22s  r | %9s %8s | %9s" % ("group", "OC x IC", "vec us", "spread", "base us"))
for group in (("q", "k", "v"), ("gate", "up"), ("down",)):
    IC = shapes[group[0]][1]
    OCs = [shapes[k][0] for k in group]
    x = torch.randn(IC, device=dev).to(bf)
    ys = [torch.zeros(OC, device=dev, dtype=bf) for OC in OCs]
    ws = [ctx.quantize(rnd(OC, IC), L.Q4) for OC in OCs]
    def run_base():
        for w, y in zip(ws, ys): ctx.linear(w, x.view(1, IC), y=y.view(1, -1))
    t_b, _ = timed(run_base)
    for r in (16, 64):
        a, b = [rnd(r, IC) for _ in OCs], [rnd(OC, r) for OC in OCs]
        t_v, s_v = timed(lambda: ctx.lora_apply(a, b, x, ys, 0.5))
        print("%-10s %-22s %2d | %9.1f %8.1f | %9.1f   (%d kf_linear launches)" % (" | ".join(group), " / ".join(map(str, OCs)) + " x %d" % IC, r, t_v, s_v, t_b, len(OCs)))
    del ws

m = synth.build_on_gpu(cfg)
rng = np.random.default_rng(0)
toks = rng.integers(0, cfg["vocab"], cfg["max_seq"]).astype(np.int32)
P0, NS = 1000, 64
m.set_forced(toks)
m.prefill(toks[:P0])


def steps():
    m.set_state(int(toks[P0]), P0)
    m.run_steps(P0, NS)


def adapters(r):
    return {"l%d.%s.w" % (l, k): (rnd(r, shapes[k][1]), rnd(shapes[k][0], r)) for l in range(cfg["n_layer"]) for k in Q3_MATS}


t, s = wall(steps, m.sync, 4)
print("decode step, engine:                          %8.1f us (spread %.1f)" % (t / NS, s / NS))
m.set_engine(False)
t, s = wall(steps, m.sync, 4)
print("decode step, per-layer launches, no adapters: %8.1f us (spread %.1f)" % (t / NS, s / NS))
m.set_engine(True)
ppl0 = wall(lambda: m.perplexity(toks[:2047]), m.sync, 3)
print("perplexity of 2047 tokens, no adapters:       %8.1f us (spread %.1f)" % ppl0)
for r in (16, 64):
    m.set_adapters(adapters(r), 0.5)
    t, s = wall(steps, m.sync, 4)
    print("decode step, adapters r%-2d on all seven:       %8.1f us (spread %.1f)" % (r, t / NS, s / NS))
    print("perplexity of 2047 tokens, adapters r%-2d:       %8.1f us (spread %.1f)" % ((r,) + wall(lambda: m.perplexity(toks[:2047]), m.sync, 3)))
    m.clear_adapters()
t, s = wall(steps, m.sync, 4)
print("decode step, engine (again, after detaching): %8.1f us (spread %.1f)" % (t / NS, s / NS))
