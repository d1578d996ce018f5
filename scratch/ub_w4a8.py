"""W4.A8 against the bf16-activation routes on token batches: kf_linear_w4a8_tiles, kf_linear_w4a8, kf_linear on the same 4-bit weights WITHOUT a dequant arena (codes
unpacked to bf16 in registers; from 1024 rows dequantise-then-multiply through the scratch) and kf_linear WITH resident bf16 copies (kf_set_dequant_arena; consulted from
320 rows) at the layer shapes of Qwen3-0.6B, at nTok = 32, 128, 512, 2047; then perplexity() of 2047 tokens on the 0.6B-shaped 4-bit model, set_act_int8_q4 on against
off with and without resident copies.  The protocol of scratch/ub_a8_tiles.py: every kernel sample is ONE call between two device events behind a cache flush (a 512 MiB
fill), variants alternated, medians of 40 samples after a warm-up; the model figures are medians of 5, alternated.
Usage: python scratch/ub_w4a8.py [out.json] [--no-model]"""
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

SHAPES = {"q": (2048, 1024), "k": (1024, 1024), "o": (1024, 2048), "gate": (3072, 1024), "down": (1024, 3072)}   # v has k's shape, up has gate's
NTOKS = (32, 128, 512, 2047)


def kernels(ctx, out):
    dev = ctx.device
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    arena = torch.empty(64 << 20, dtype=torch.uint8, device=dev)   # the largest matrix is 6 MiB as bf16
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
        w = ctx.quantize((torch.randn(M, K, device=dev) * 0.02).to(torch.bfloat16), L.Q4)
        d = w.desc()
        for n in NTOKS:
            x = torch.randn(n, K, device=dev).to(torch.bfloat16)
            q, step = ctx.act_quant_i8(x)
            y = torch.empty((n, M), dtype=torch.bfloat16, device=dev)
            need = max(int(ctx.hip.kf_linear_scratch_bytes(C.byref(d), n)), ws_bytes)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            ctx.sync()
            L.check(ctx.hip.kf_set_scratch(ctx.h, C.c_void_p(ws.data_ptr()), C.c_size_t(need)), "kf_set_scratch")

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
                f = {"kf_linear_w4a8_tiles": lambda: ctx.linear_w4a8_tiles(w, q, step, y=y), "kf_linear_w4a8": lambda: ctx.linear_w4a8(w, q, step, y=y), "kf_linear": bf16_route}[name]
                return sample(f), 0

            names = ("kf_linear_w4a8_tiles", "kf_linear_w4a8", "kf_linear", "kf_linear arena")
            ts, used = {k: [] for k in names}, 0
            for k in names:
                for _ in range(5):
                    timed(k)
            for _ in range(40):
                for k in names:
                    t, u = timed(k)
                    ts[k].append(t)
                    used = max(used, u)
            res = {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in ts.items()}
            res["arena_bytes_used"] = used   # 0: the arena route was not taken at this nTok -- the column repeats "kf_linear"
            out["%s %dx%d nTok=%d" % (slot, M, K, n)] = res
            print(slot, M, K, n, json.dumps(res), flush=True)


def ppl(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.Q4, head_type=L.BF16)
    toks = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)

    def run(name):
        m.set_act_int8_q4(name == "w4a8")
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
        if name == "w4a8":
            r["route_counts"] = m.a8_route_counts()
        return r

    res = {}
    for _ in range(2):   # alternated
        for name in ("w4a8", "bf16", "bf16 arena"):
            res[name] = run(name)
    m.set_act_int8_q4(False)
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
