"""The int8 KV cache against the bf16 cache, measured in one run (nothing here is asserted anywhere):
  call     kf_attn_block_kv8 against kf_attn_block (canonical order), 16 / 8 heads x 128, at 2 k, 8 k and 32 k keys: the CALL TIME -- ONE call between two device events
           behind a cache flush (a 512 MiB fill: the rows of a real step arrive cold), the two alternated, medians of 40 samples after a warm-up.  This is not the kernel
           time of a profiler's trace: an event pair around one short launch carries a few microseconds of its own, the same for both, a large share of both cells at
           2 k keys.  Bytes per second of a call from the bytes the algorithm needs -- bf16: 2 tensors x keys x kv_dim x 2 B; int8: keys x (2 x kv_dim + 2 x n_kv x 4) B --
           over that call time: a lower bound of the kernel's own rate.
  model    a Qwen3-0.6B-shaped 4-bit model with a 32 k context: windows of 16 decode steps ending at 2 k, 8 k and 32 k keys, host clock around a synchronise.  Three ways:
           switch on (captured per-layer graphs), off through the persistent engine, off on captured per-layer graphs.  A switch drops the engine and the captured graphs,
           so a way is switched to ONCE per round, two untimed windows follow (the graphs are captured, the engine and its head screen built), then WINDOWS timed windows
           run with nothing switched between them; ROUNDS rounds alternate the ways.  Median and minimum over all timed windows of a way.
  prefill  perplexity() of 2047 tokens, on and off: per switch one untimed pass, then three timed ones; two rounds, alternated.
Usage: python scratch/ub_kv8.py [out.json]"""
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

NH, NKV, HD = 16, 8, 128
CONTEXTS = [2048, 8192, 32768]
ROUNDS, WINDOWS = 3, 8   # model steps: rounds of (switch, two untimed windows, WINDOWS timed windows) per way


def calls(ctx, out):
    dev = ctx.device
    kvd = NKV * HD
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    T = max(CONTEXTS)
    kc = (torch.randn(T, kvd, device=dev)).to(torch.bfloat16)
    vc = (torch.randn(T, kvd, device=dev)).to(torch.bfloat16)
    k8 = torch.zeros(T, kvd, dtype=torch.int8, device=dev)
    v8 = torch.zeros_like(k8)
    ks = torch.zeros(T, NKV, dtype=torch.float32, device=dev)
    vs = torch.zeros_like(ks)
    for r0 in range(0, T, 4096):
        ctx.kv8_quant_rows(kc[r0:r0 + 4096], vc[r0:r0 + 4096], k8, v8, ks, vs, r0, NKV, HD)
    q, kr, vr = (torch.randn(n, device=dev).to(torch.bfloat16) for n in (NH * HD, kvd, kvd))
    wn = torch.ones(HD, dtype=torch.bfloat16, device=dev)
    tab = ctx.rope_table(T, HD, 1e6)
    ctx.set_canonical(True)

    def sample(f):
        flush.fill_(1)
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for keys in CONTEXTS:
        pos = keys - 1
        variants = {"kf_attn_block": (lambda: ctx.attn_block(q, kr, kc, vc, wn, wn, tab, pos, NH, NKV, HD), 2 * keys * kvd * 2),
                    "kf_attn_block_kv8": (lambda: ctx.attn_block_kv8(q, kr, vr, k8, v8, ks, vs, wn, wn, tab, pos, NH, NKV, HD), keys * (2 * kvd + 8 * NKV))}
        ts = {k: [] for k in variants}
        for k, (f, _) in variants.items():
            for _ in range(5):
                sample(f)
        for _ in range(40):
            for k, (f, _) in variants.items():
                ts[k].append(sample(f))
        res = {k: {"median_us": statistics.median(v), "min_us": min(v), "bytes": variants[k][1], "GBps_at_median": variants[k][1] / statistics.median(v) / 1e3} for k, v in ts.items()}
        out["call %d keys" % keys] = res
        print("call", keys, "keys", json.dumps(res), flush=True)


def model(out):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"], max_seq=max(CONTEXTS))
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.Q4, head_type=L.BF16)
    forced = np.random.default_rng(17).integers(0, cfg["vocab"], size=cfg["max_seq"]).astype(np.int32)
    m.set_forced(forced)
    N = 16

    def setup(way):
        m.set_kv_int8(way == "int8 cache, per-layer graphs")
        m.set_engine(way != "bf16 cache, per-layer graphs")

    def window(pos0):
        m.set_state(int(forced[pos0]), pos0)
        m.sync()
        t0 = time.perf_counter()
        m.run_steps(pos0, N, use_graph=True)
        m.sync()
        return (time.perf_counter() - t0) / N * 1e3

    ways = ["int8 cache, per-layer graphs", "bf16 cache, engine", "bf16 cache, per-layer graphs"]
    for keys in CONTEXTS:
        pos0 = keys - N
        ts = {w: [] for w in ways}
        first = {w: [] for w in ways}
        why = ""
        for _ in range(ROUNDS):
            for w in ways:
                setup(w)   # the ONLY switch of this way in this round: everything below runs on what the untimed windows build
                first[w].append(window(pos0))
                window(pos0)
                ts[w] += [window(pos0) for _ in range(WINDOWS)]
                if w == "bf16 cache, engine":
                    why = m.engine_why()
        res = {w: {"median_ms_per_step": statistics.median(v), "min_ms_per_step": min(v), "max_ms_per_step": max(v), "windows": len(v),
                   "first_window_after_a_switch_ms_per_step": statistics.median(first[w])} for w, v in ts.items()}
        res["engine_why (bf16 cache, engine)"] = why
        out["model step ending at %d keys" % keys] = res
        print("model", keys, "keys", json.dumps(res), flush=True)
    # prefill: perplexity of 2047 tokens
    toks = forced[:2047]
    ts = {True: [], False: []}
    ppl = {}
    for _ in range(2):
        for on in (True, False):
            m.set_kv_int8(on)
            m.perplexity(toks)   # untimed: buffers and (first time) the int8 pair allocated
            for _ in range(3):
                m.sync()
                t0 = time.perf_counter()
                ppl[on] = m.perplexity(toks)[0]
                ts[on].append((time.perf_counter() - t0) * 1e3)
    m.set_kv_int8(False)
    res = {("int8 cache" if on else "bf16 cache"): {"median_ms": statistics.median(v), "min_ms": min(v), "ppl": ppl[on]} for on, v in ts.items()}
    out["perplexity of 2047 tokens"] = res
    print("perplexity", json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("scratch/ub_kv8.py measures on the GPU: no device here")
    out = {}
    c = Context(0)
    calls(c, out)
    c.close()
    model(out)
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)
