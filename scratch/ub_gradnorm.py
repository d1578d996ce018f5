"""kf_grad_norms (kf_gradnorm.hip: every gradient tensor's sum of squares in one launch, the per-tensor and the total follow-ups behind it) over the tensor lists
of GPT2-1558M and Qwen3-0.6B: time of the three launches and the achieved GB/s at 2 bytes per parameter, with kf_adamw over the same tensors (one launch per tensor,
16 bytes per parameter with bf16 moments) as the yardstick; then one whole Qwen3Step.step at the Qwen3-0.6B shape, 8 x 1024 tokens, with clipping off, "report" and
"tensor".  Each figure is the mean of REPS launches, measured ROUNDS times: printed are the median and the spread (max - min) over the rounds.
Usage: python scratch/ub_gradnorm.py [out.json]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koifish_amd import lib as L          # noqa: E402
from koifish_amd import synth             # noqa: E402
from koifish_amd.runtime import Context   # noqa: E402
from koifish_amd.train_step import Qwen3Step   # noqa: E402

REPS, ROUNDS = 10, 5


def gpt2_1558m():
    """the registered order of GPT2Step: per block qkv.w qkv.b proj.w proj.b fc.w fc.b proj2.w proj2.b ln1.w ln1.b ln2.w ln2.b, then wte wpe lnf.w lnf.b"""
    C_, NL, Vp, T = 1600, 48, 50304, 1024
    blk = [3 * C_ * C_, 3 * C_, C_ * C_, C_, 4 * C_ * C_, 4 * C_, 4 * C_ * C_, C_, C_, C_, C_, C_]
    return blk * NL + [Vp * C_, T * C_, C_, C_]


def main(out):
    ctx = Context(0)
    hip, dev, bf = ctx.hip, ctx.device, torch.bfloat16

    def timed(fn, reps=REPS, rounds=ROUNDS):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(rounds):
            ctx.sync()
            e0, e1 = ctx.event(), ctx.event()
            ctx.record(e0)
            for _ in range(reps):
                fn()
            ctx.record(e1)
            ctx.sync()
            ts.append(ctx.elapsed_ms(e0, e1) / reps * 1e3)
        return statistics.median(ts), max(ts) - min(ts)

    cfg = synth.CONFIGS["qwen3-0.6b"]
    st = Qwen3Step(ctx, cfg, 8, 1024)
    lists = {"GPT2-1558M": gpt2_1558m(), "Qwen3-0.6B": [e["g"].numel() for e in st.params]}
    for name, sizes in lists.items():
        n = sum(sizes)
        g = [(torch.randn(s, device=dev) * 0.01).to(bf) for s in sizes]
        plan = ctx.grad_norms_plan(g)
        t_n, s_n = timed(lambda: ctx.grad_norms(plan, "tensor", 1.0))
        p, m, v = ([torch.zeros(s, device=dev, dtype=bf) for s in sizes] for _ in range(3))

        def adamw():   # gradients are zeroed by the first pass: the time does not depend on the values
            for i in range(len(sizes)):
                L.check(hip.kf_adamw(ctx.h, p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), sizes[i], L.BF16, 1e-4, 0.9, 0.95, 0.1, 0.05, 1e-8, 0.0, 1.0, i, None), "kf_adamw")
        t_a, s_a = timed(adamw, reps=3, rounds=3)
        res = dict(tensors=len(sizes), params=n, chunks=sum((s + 4095) // 4096 for s in sizes), grad_norms_us=t_n, grad_norms_spread_us=s_n, grad_norms_GBps=2 * n / t_n * 1e-3,
                   adamw_us=t_a, adamw_spread_us=s_a, adamw_GBps=16 * n / t_a * 1e-3)
        out[name] = res
        print(name, json.dumps(res), flush=True)
        del g, p, m, v, plan
        torch.cuda.empty_cache()

    ids = torch.randint(0, cfg["vocab"], (8 * 1024,), device=dev, dtype=torch.int32)
    tgt = torch.randint(0, cfg["vocab"], (8 * 1024,), device=dev, dtype=torch.int32)
    for mode in (None, "report", "tensor"):
        st.set_grad_clip(1.0, mode)
        t_s, s_s = timed(lambda: st.step(ids, tgt), reps=3, rounds=3)
        out["step clip=%s" % mode] = dict(step_us=t_s, spread_us=s_s)
        print("Qwen3-0.6B, 8 x 1024 tokens, 4-bit layers: Qwen3Step.step with clipping %-6s %9.1f us (spread %.1f)%s"
              % (mode, t_s, s_s, "" if mode is None else "   |g| = %.4g" % st.grad_norm()), flush=True)
    ctx.close()


if __name__ == "__main__":
    out = {}
    main(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
