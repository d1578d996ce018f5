"""The int8 prompt attention (kf_attn_prefill_kv8) against the route it replaces and against the bf16 prompt attention, measured in one run with the method of
scratch/ub_kv8.py (nothing here is asserted anywhere):
  call     16 / 8 heads x 128, cells (pos0, n) = (0, 128) (0, 512) (0, 2047) (8192, 512) (32768 - 512, 512).  Three ways of attending one batch:
             int8      kf_attn_prefill_kv8 on the int8 rows
             dequant   kf_kv8_dequant_rows over rows 0 .. pos0 + n - 1 of the staging pair, then kf_attn_prefill on it -- the route the switch replaces
             bf16      kf_attn_prefill on a bf16 cache -- the int8 cache off
           The CALL TIME: the calls of a way between two device events behind a cache flush (a 512 MiB fill), the three ways alternated inside one run, medians of 30
           samples after a warm-up, minimum and maximum stated.  Not a profiler's kernel time: an event pair carries a few microseconds of its own, the same for all.
  model    perplexity() of 2047 tokens on a Qwen3-0.6B-shaped 4-bit model under the same three ways: per way and round ONE switch, one untimed pass, three timed
           passes with nothing switched inside them; two rounds, alternated.
Usage: python scratch/ub_kv8_prefill.py [out.json]"""
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

NH, NKV, HD = 16, 8, 128
CELLS = [(0, 128), (0, 512), (0, 2047), (8192, 512), (32768 - 512, 512)]
SAMPLES = 30


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def calls(ctx, out):
    dev = ctx.device
    kvd, qd, T = NKV * HD, NH * HD, 32768
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    kc = torch.randn(T, kvd, device=dev).to(torch.bfloat16)
    vc = torch.randn(T, kvd, device=dev).to(torch.bfloat16)
    sk, sv = torch.zeros_like(kc), torch.zeros_like(vc)   # the staging pair
    k8 = torch.zeros(T, kvd, dtype=torch.int8, device=dev)
    v8 = torch.zeros_like(k8)
    ks = torch.zeros(T, NKV, dtype=torch.float32, device=dev)
    vs = torch.zeros_like(ks)
    for r0 in range(0, T, 4096):
        ctx.kv8_quant_rows(kc[r0:r0 + 4096], vc[r0:r0 + 4096], k8, v8, ks, vs, r0, NKV, HD)
    q_all = torch.randn(2048, qd, device=dev).to(torch.bfloat16)
    o_all = torch.empty_like(q_all)

    def bf16_attn(k, v, q, o, pos0, n):
        L.check(ctx.hip.kf_attn_prefill(ctx.h, _ptr(q), _ptr(k), _ptr(v), _ptr(o), pos0, n, qd, NH, NKV, HD, kvd), "kf_attn_prefill")

    def sample(f):
        flush.fill_(1)
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for pos0, n in CELLS:
        q, o = q_all[:n], o_all[:n]

        def dequant_route():
            ctx.kv8_dequant_rows(k8, v8, ks, vs, pos0 + n, NKV, HD, sk, sv)
            bf16_attn(sk, sv, q, o, pos0, n)

        ways = {"int8": lambda: ctx.attn_prefill_kv8(q, k8, v8, ks, vs, pos0, NH, NKV, HD, out=o), "dequant": dequant_route, "bf16": lambda: bf16_attn(kc, vc, q, o, pos0, n)}
        ts = {w: [] for w in ways}
        for f in ways.values():
            for _ in range(4):
                sample(f)
        for _ in range(SAMPLES):
            for w, f in ways.items():
                ts[w].append(sample(f))
        res = {w: spread(v) for w, v in ts.items()}
        out["call pos0 %d n %d" % (pos0, n)] = res
        print("call", pos0, n, json.dumps(res), flush=True)


def model(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"], max_seq=2048)
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.Q4, head_type=L.BF16)
    toks = np.random.default_rng(17).integers(0, cfg["vocab"], size=2047).astype(np.int32)
    ways = {"int8": (True, True), "dequant": (True, False), "bf16": (False, False)}
    ts, ppl = {w: [] for w in ways}, {}
    for _ in range(2):
        for w, (kv, pre) in ways.items():
            m.set_kv_int8(kv)
            m.set_kv_int8_prefill(pre)
            m.perplexity(toks)   # untimed
            for _ in range(3):
                m.sync()
                t0 = time.perf_counter()
                ppl[w] = m.perplexity(toks)[0]
                ts[w].append((time.perf_counter() - t0) * 1e3)
    m.set_kv_int8(False)
    res = {w: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "ppl": ppl[w]} for w, v in ts.items()}
    out["perplexity of 2047 tokens"] = res
    print("perplexity", json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("scratch/ub_kv8_prefill.py measures on the GPU: no device here")
    out = {}
    c = Context(0)
    calls(c, out)
    c.close()
    model(out)
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)
