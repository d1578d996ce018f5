"""Batched decode against sequence-serial decode, measured in one run (nothing here is asserted anywhere; the method is scratch/ub_kv8.py's):
  call     ONE kf_attn_block_seqs launch against n_seq kf_attn_block launches (canonical order) on the same rows: n_seq 4 / 8 / 32 sequences of 2 k and 8 k keys each,
           16 / 8 heads x 128 and 64 / 8 x 128.  The CALL TIME: the launches between two device events behind a cache flush (a 512 MiB fill), the two ways alternated,
           medians of 20 samples after a warm-up.  Not a profiler's kernel time: an event pair carries a few microseconds of its own.  Bytes per second from the bytes
           the algorithm needs (n_seq x 2 tensors x keys x kv_dim x 2 B) over that time.
  model    tokens/s of generate_batch (n_seq prompts of 8 tokens, 48 new ids each) against n_seq generate() calls one after the other on the per-layer path (engine
           off, captured graphs: code this commit does not touch) and, for the shapes it serves, through the persistent engine (the default); n_seq 1 / 4 / 8 / 16 / 32;
           the 0.6B shape and a 4-layer slice of the 32B shape (bench.py's config-4 slice), 4-bit and NF4 layers.  Host clock around calls that end in a device read;
           per n_seq one untimed pass of every way, then ROUNDS rounds alternating them; median, minimum and maximum.
Usage: python scratch/ub_decode_seqs.py [out.json]"""
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

HEADS = [(16, 8, 128), (64, 8, 128)]
KEYS = [2048, 8192]
N_SEQ = [4, 8, 32]
MODEL_N_SEQ = [1, 4, 8, 16, 32]
N_PROMPT, N_NEW, ROUNDS = 8, 48, 3


def calls(ctx, out):
    dev = ctx.device
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    ctx.set_canonical(True)

    def sample(f):
        flush.fill_(1)
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for nh, nkv, hd in HEADS:
        kvd, S = nkv * hd, max(N_SEQ)
        wn = torch.ones(hd, dtype=torch.bfloat16, device=dev)
        tab = ctx.rope_table(max(KEYS), hd, 1e6)
        q, kr, vr = (torch.randn(S, n, device=dev).to(torch.bfloat16) for n in (nh * hd, kvd, kvd))
        for keys in KEYS:
            kc = torch.randn(S * keys, kvd, device=dev).to(torch.bfloat16)
            vc = torch.randn(S * keys, kvd, device=dev).to(torch.bfloat16)
            for n_seq in N_SEQ:
                pos, row0 = [keys - 1] * n_seq, [s * keys for s in range(n_seq)]
                d_pos = torch.tensor(pos, dtype=torch.int32, device=dev)
                d_row0 = torch.tensor(row0, dtype=torch.int32, device=dev)
                o = torch.zeros(n_seq, nh * hd, dtype=torch.bfloat16, device=dev)
                ws = torch.zeros(ctx.hip.kf_attn_seqs_scratch_bytes(nh, hd, n_seq), dtype=torch.uint8, device=dev)

                def one():
                    ctx.attn_block_seqs(q[:n_seq], kr[:n_seq], vr[:n_seq], kc, vc, wn, wn, tab, pos, row0, nh, nkv, hd, out=o, scratch=ws, d_pos=d_pos, d_row0=d_row0)

                def serial():
                    for s in range(n_seq):   # (the V rows are in place already: kf_attn_block reads them from the cache)
                        ctx.attn_block(q[s], kr[s], kc[row0[s]:], vc[row0[s]:], wn, wn, tab, pos[s], nh, nkv, hd)

                variants = {"kf_attn_block_seqs": one, "n_seq x kf_attn_block": serial}
                ts = {k: [] for k in variants}
                for f in variants.values():
                    for _ in range(3):
                        sample(f)
                for _ in range(20):
                    for k, f in variants.items():
                        ts[k].append(sample(f))
                nbytes = n_seq * 2 * keys * kvd * 2
                res = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "GBps_at_median": nbytes / statistics.median(v) / 1e3} for k, v in ts.items()}
                name = "call %d/%d x %d, %d keys, n_seq %d" % (nh, nkv, hd, keys, n_seq)
                out[name] = res
                print(name, json.dumps(res), flush=True)
            del kc, vc


def model(out, shape, layer_type, tag):
    cfg = dict(synth.CONFIGS[shape], max_seq=2048)
    if shape == "qwen3-32b":
        cfg["n_layer"] = 4
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=layer_type, head_type=L.BF16)
    m.set_canonical(True)
    m.set_prefill_mode(1)
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, cfg["vocab"], size=N_PROMPT).astype(np.int32).tolist() for _ in range(max(MODEL_N_SEQ))]

    def timed(f, n_seq):
        m.sync()
        t0 = time.perf_counter()
        f()
        return n_seq * N_NEW / (time.perf_counter() - t0)

    for n_seq in MODEL_N_SEQ:
        ps = prompts[:n_seq]

        def batch():
            return m.generate_batch(ps, N_NEW)

        def serial():
            return [m.generate(p, N_NEW) for p in ps]

        ways = {"generate_batch": (batch, None), "generate x n_seq, per-layer path": (serial, False), "generate x n_seq, engine (default)": (serial, True)}
        ts = {w: [] for w in ways}
        ids = {}
        for rnd in range(ROUNDS + 1):   # round 0 untimed: buffers, graphs, the engine
            for w, (f, engine) in ways.items():
                if engine is not None:
                    m.set_engine(engine)
                tps = timed(f, n_seq)
                if rnd:
                    ts[w].append(tps)
                else:
                    ids[w] = f()
        m.set_engine(True)
        res = {w: {"median_tok_s": statistics.median(v), "min_tok_s": min(v), "max_tok_s": max(v)} for w, v in ts.items()}
        res["ids equal (batch == per-layer path)"] = ids["generate_batch"] == ids["generate x n_seq, per-layer path"]
        res["engine_why"] = m.engine_why()
        res["route"] = m.seqs_route_counts()
        name = "model %s %s, n_seq %d" % (shape if shape != "qwen3-32b" else "qwen3-32b 4-layer slice", tag, n_seq)
        out[name] = res
        print(name, json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("scratch/ub_decode_seqs.py measures on the GPU: no device here")
    out = {}
    c = Context(0)
    calls(c, out)
    c.close()
    for shape in ("qwen3-0.6b", "qwen3-32b"):
        for layer_type, tag in ((L.Q4, "4-bit"), (L.NF4, "NF4")):
            model(out, shape, layer_type, tag)
            if len(sys.argv) > 1:
                json.dump(out, open(sys.argv[1], "w"), indent=1)
