"""kf_evolve (kf_evo.hip), algorithm pso_ga, on the fc (6400 x 1600) and proj (1600 x 1600) shapes of a GPT2-1558M block, beside a bandwidth yardstick that moves the
same 6 bytes per element in the same process: torch.add(x, head, out=x) on bf16 (read x, read head, write x).  A sample is ONE call between two device events, the two
variants alternated, medians of 30 samples after a warm-up.  Each variant works on its own pair of tensors (a few times the 256 MB the last-level cache keeps would be
needed to take it out of the picture: both variants see the same residency, which is what the ratio compares).  Then a full GPT2Step.evolve() over ONE follower section
of the 1558M shape: a two-layer trainer with layers_in_branch = 1 (head = layer 0, follower = layer 1: its four matrices evolved and re-quantised).
Usage: python scratch/ub_evo.py [out.json]"""
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from koifish_amd.runtime import Context   # noqa: E402

SHAPES = {"fc": (6400, 1600), "proj": (1600, 1600)}


def main(out):
    ctx = Context(0)
    dev, bf = ctx.device, torch.bfloat16

    def sample(f):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for name, (ne0, ne1) in SHAPES.items():
        mk = lambda: (torch.randn(ne0, ne1, device=dev) * 0.02).to(bf)
        xa, ha, xb, hb = mk(), mk(), mk(), mk()
        variants = {"kf_evolve pso_ga": lambda: ctx.evolve(xa, ha, "pso_ga", seed=7), "torch.add": lambda: torch.add(xb, hb, out=xb)}
        ts = {k: [] for k in variants}
        for f in variants.values():
            for _ in range(5):
                sample(f)
        for _ in range(30):
            for k, f in variants.items():
                ts[k].append(sample(f))
        n = ne0 * ne1
        res = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "GBps": 6.0 * n / statistics.median(v) * 1e-3} for k, v in ts.items()}
        res["ratio"] = res["kf_evolve pso_ga"]["median_us"] / res["torch.add"]["median_us"]
        out["%s %dx%d" % (name, ne0, ne1)] = res
        print(name, ne0, ne1, json.dumps(res), flush=True)

    from koifish_amd.train_step import GPT2Step
    st = GPT2Step(ctx, 1600, 25, 2, 50257, 50304, 1, 128, layers_in_branch=1)
    ts = []
    for i in range(13):
        t = sample(lambda: st.evolve(0, "pso_ga", seed=i))
        if i >= 3:
            ts.append(t)
    out["evolve() one follower section, 1558M block"] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}
    print("evolve() section", json.dumps(out["evolve() one follower section, 1558M block"]), flush=True)
    st.close()
    ctx.close()


if __name__ == "__main__":
    out = {}
    main(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
