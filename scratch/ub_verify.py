"""The verify pass of speculative decoding against the one-token launches it replaces, everything timed in ONE run with the variants alternated.
  1. per matrix group (q|k|v, o, gate|up, down, head) of the 0.6B / 1.7B / 4B shapes, 4-bit layers and a bf16 head: the row entry at R = 1 .. 8 against R one-token
     launches of the same group.  A sample is ONE call (or the R calls) between two device events behind a cache flush (a 512 MiB fill: the weights of a real step
     arrive cold); medians after a warm-up; an event pair carries a few microseconds of its own, the same for every variant.
  2. kf_attn_decode_rows alone at 2 k and 8 k keys (the 0.6B head shape), R = 1 .. 8, against R kf_attn_decode launches, sampled the same way.
  3. whole models (synthetic weights): verify(R) at position 2040 against (a) one decode step on the per-layer launches and (b) R of them -- eager and on captured
     graphs -- and the engine's step where it serves the model; host clock around work that ends in a synchronise, windows alternated.
Usage: python scratch/ub_verify.py [out.json] [models: 0.6b,1.7b,4b]"""
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
from koifish_amd.runtime import Context   # noqa: E402

RS = list(range(1, 9))
N_WARM, N_SAMPLE = 3, 15


def sampler(ctx):
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=ctx.device)

    def sample(f):
        flush.fill_(1)
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3
    return sample


def ab(sample, variants):
    """variants: name -> callable; alternated; {name: median us}"""
    ts = {k: [] for k in variants}
    for k, f in variants.items():
        for _ in range(N_WARM):
            sample(f)
    for _ in range(N_SAMPLE):
        for k, f in variants.items():
            ts[k].append(sample(f))
    return {k: round(statistics.median(v), 2) for k, v in ts.items()}


def groups(ctx, name, cfg, out):
    """the ABI entries themselves (ctypes, every buffer allocated beforehand: nothing but the entry's own launches lies between the two events)"""
    dev, sample, hip, h = ctx.device, sampler(ctx), ctx.hip, ctx.h
    D, qd, kvd, F, V = cfg["dim"], cfg["n_head"] * cfg["head_dim"], cfg["n_kv"] * cfg["head_dim"], cfg["ffn"], cfg["vocab"]
    q4 = lambda m, k: ctx.quantize((torch.randn(m, k, device=dev) * 0.02).to(torch.bfloat16), L.Q4)
    ws_ = [q4(qd, D), q4(kvd, D), q4(kvd, D), q4(D, qd), q4(F, D), q4(F, D), q4(D, F), ctx.quantize((torch.randn(V, D, device=dev) * 0.02).to(torch.bfloat16), L.BF16)]
    dq, dk, dv, do, dg, du, dd, dh = [w.desc() for w in ws_]
    nw = torch.ones(D, dtype=torch.bfloat16, device=dev)
    rows = lambda k: torch.randn(8, k, device=dev).to(torch.bfloat16)
    buf = lambda k: torch.empty(8, k, dtype=torch.bfloat16, device=dev)
    xD, xQ, xF, res = rows(D), rows(qd), rows(F), rows(D)
    yq, yk, yv, yD, act, logits = buf(qd), buf(kvd), buf(kvd), buf(D), buf(F), buf(V)
    top1 = torch.zeros(8, dtype=torch.int32, device=dev)
    head_ws = torch.empty(hip.kf_head_rows_scratch_bytes(C.byref(dh)), dtype=torch.uint8, device=dev)
    P = lambda t, r=0: C.c_void_p(t.data_ptr() + r * t.stride(0) * t.element_size())
    wp = (C.c_void_p * 3)(C.addressof(dq), C.addressof(dk), C.addressof(dv))
    yp = [(C.c_void_p * 3)(P(yq, r).value, P(yk, r).value, P(yv, r).value) for r in range(8)]
    rs, ps = (C.c_int64 * 3)(qd, kvd, kvd), (C.c_int64 * 3)(0, 0, 0)
    eps = 1e-6
    for R in RS:
        cases = {
            "qkv": (lambda: hip.kf_norm_linear_rows(h, P(xD), D, P(nw), eps, 3, wp, yp[0], rs, ps, 0, R),
                    lambda: [hip.kf_norm_linear(h, P(xD, r), P(nw), eps, 3, wp, yp[r], None, 0, None) for r in range(R)]),
            "o": (lambda: hip.kf_linear_rows(h, C.byref(do), P(xQ), qd, P(yD), D, R, 1, P(res), D),
                  lambda: [hip.kf_linear(h, C.byref(do), P(xQ, r), P(yD, r), None, 1, 1.0, 0.0, 1, P(res, r)) for r in range(R)]),
            "gate_up": (lambda: hip.kf_norm_gateup_swiglu_rows(h, P(xD), D, P(nw), eps, C.byref(dg), C.byref(du), P(act), F, R),
                        lambda: [hip.kf_norm_gateup_swiglu(h, P(xD, r), P(nw), eps, C.byref(dg), C.byref(du), P(act, r)) for r in range(R)]),
            "down": (lambda: hip.kf_linear_rows(h, C.byref(dd), P(xF), F, P(yD), D, R, 1, P(res), D),
                     lambda: [hip.kf_linear(h, C.byref(dd), P(xF, r), P(yD, r), None, 1, 1.0, 0.0, 1, P(res, r)) for r in range(R)]),
            "head": (lambda: hip.kf_norm_lm_head_rows(h, P(xD), D, None, eps, C.byref(dh), P(logits), V, P(top1), R, P(head_ws)),
                     lambda: [hip.kf_lm_head(h, C.byref(dh), P(xD, r), P(logits, r), P(top1, r), P(head_ws)) for r in range(R)]),
        }
        for g, (rows_f, one_f) in cases.items():
            assert rows_f() == 0 and all(rc == 0 for rc in one_f()), (name, g, R)
            r = ab(sample, {"rows": rows_f, "one_token_x_R": one_f})
            out["%s %s R=%d" % (name, g, R)] = r
            print(name, g, "R=%d" % R, json.dumps(r), flush=True)


def attention(ctx, out):
    dev, sample = ctx.device, sampler(ctx)
    n_head, n_kv, hd = 16, 8, 128
    for keys in (2048, 8192):
        kc = torch.randn(keys, n_kv * hd, device=dev).to(torch.bfloat16)
        vc = torch.randn(keys, n_kv * hd, device=dev).to(torch.bfloat16)
        q = torch.randn(8, n_head * hd, device=dev).to(torch.bfloat16)
        ws = torch.zeros(ctx.hip.kf_attn_rows_scratch_bytes(n_head, hd, 8), dtype=torch.uint8, device=dev)
        for R in RS:
            pos0 = keys - R
            r = ab(sample, {"rows": lambda: ctx.attn_decode_rows(q[:R], kc, vc, pos0, n_head, n_kv, hd, scratch=ws),
                            "one_token_x_R": lambda: [ctx.attn_decode(q[i], kc, vc, pos0 + i, n_head, n_kv, hd) for i in range(R)]})
            out["attn %d keys R=%d" % (keys, R)] = r
            print("attn", keys, "R=%d" % R, json.dumps(r), flush=True)


def model(name, out, pos0=2040, n_rep=9):
    cfg = dict(synth.CONFIGS["qwen3-" + name])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.Q4, head_type=L.BF16)
    forced = np.random.default_rng(17).integers(0, cfg["vocab"], size=cfg["max_seq"]).astype(np.int32)
    m.set_forced(forced)
    m.set_state(int(forced[0]), 0)
    m.run_steps(0, pos0 + 7)   # every cache row the windows read
    m.sync()

    def steps(n, graph):
        m.set_state(int(forced[pos0]), pos0)
        m.sync()
        t0 = time.perf_counter()
        m.run_steps(pos0, n, use_graph=graph)
        m.sync()
        return (time.perf_counter() - t0) * 1e3

    def verify(R):
        t0 = time.perf_counter()
        m.verify(forced[pos0:pos0 + R], pos0)   # ends in the read of the R ids
        return (time.perf_counter() - t0) * 1e3

    res = {}
    m.set_engine(True)
    steps(8, True)
    eng = [steps(8, True) / 8 for _ in range(n_rep)]
    res["engine_step_ms"] = round(statistics.median(eng), 4) if m.engine_steps() > 0 else None
    m.set_engine(False)
    for R in RS:
        variants = {"verify": lambda: verify(R), "steps_eager": lambda: steps(R, False), "steps_graph": lambda: steps(R, True)}
        ts = {k: [] for k in variants}
        for f in variants.values():
            f(), f()
        for _ in range(n_rep):
            for k, f in variants.items():
                ts[k].append(f())
        res["R=%d" % R] = {k: round(statistics.median(v), 4) for k, v in ts.items()}
        print(name, "R=%d" % R, json.dumps(res["R=%d" % R]), flush=True)
    out["model " + name] = res
    print(name, "engine_step_ms", res["engine_step_ms"], flush=True)
    m.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else None
    names = (sys.argv[2] if len(sys.argv) > 2 else "0.6b,1.7b,4b").split(",")
    out = {}
    ctx = Context(0)
    for n in names:
        groups(ctx, n, synth.CONFIGS["qwen3-" + n], out)
    attention(ctx, out)
    for n in names:
        model(n, out)
        if path:
            json.dump(out, open(path, "w"), indent=1)
    if path:
        json.dump(out, open(path, "w"), indent=1)
