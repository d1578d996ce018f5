"""kf_newton_schulz (kf_muon.hip: the symmetric-tile products) on the three Muon shapes of a GPT2-1558M block, against the same five iterations composed from entries
that existed before it: kf_linear on bf16 "weights" for X B and A A, kf_linear on a transposed copy of X for X^T X, the axpys and the transpose in torch.  Both are
five iterations from a pre-scaled X; a sample is ONE whole call (or composition) between two device events, variants alternated, medians of 20 samples after a
warm-up.  The flop rate counts the FULL products (2 ne1^2 ne0 + 2 ne1^3 + 2 ne0 ne1^2 per iteration), whichever tiles a kernel skips.
Usage: python scratch/ub_muon.py [out.json]"""
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from koifish_amd import lib as L          # noqa: E402
from koifish_amd.runtime import Context   # noqa: E402

SHAPES = {"qkv": (4800, 1600), "proj": (1600, 1600), "fc": (6400, 1600)}
A_, B_, C_ = 3.4445, -4.7750, 2.0315


def main(out):
    ctx = Context(0)
    hip, dev, bf = ctx.hip, ctx.device, torch.bfloat16

    def lin(w, x, y, n, alpha=1.0):
        d = ctx.quantize(w, L.BF16).desc()
        L.check(hip.kf_linear(ctx.h, C.byref(d), x.data_ptr(), y.data_ptr(), None, n, alpha, 0.0, 0, None), "kf_linear")

    def sample(f):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) * 1e3

    for name, (ne0, ne1) in SHAPES.items():
        X0 = (torch.randn(ne0, ne1, device=dev) * 0.02).to(bf)
        X0 = (X0.float() / X0.float().norm()).to(bf)
        nb = hip.kf_muon_scratch_bytes(ne0, ne1)
        sc = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        sp = (sc.data_ptr() + 255) & ~255
        Xa = X0.clone()
        A, AA, XB = torch.empty(ne1, ne1, dtype=bf, device=dev), torch.empty(ne1, ne1, dtype=bf, device=dev), torch.empty(ne0, ne1, dtype=bf, device=dev)
        ctx.linear_scratch(ctx.quantize(X0, L.BF16), ne0)

        def symmetric():
            Xa.copy_(X0)
            L.check(hip.kf_newton_schulz(ctx.h, Xa.data_ptr(), ne0, ne1, None, 1e-7, 5, A_, B_, C_, sp, nb), "kf_newton_schulz")

        def composed():
            X = X0
            for _ in range(5):
                Xt = X.t().contiguous()
                lin(Xt, Xt, A, ne1)
                lin(A, A, AA, ne1, C_)
                Bm = (B_ * A.float() + AA.float()).to(bf)
                lin(Bm, X, XB, ne0)
                X = (A_ * X.float() + XB.float()).to(bf)
            return X

        torch.cuda.synchronize()
        variants = {"kf_newton_schulz": symmetric, "composed": composed}
        ts = {k: [] for k in variants}
        for f in variants.values():
            for _ in range(3):
                sample(f)
        for _ in range(20):
            for k, f in variants.items():
                ts[k].append(sample(f))
        flop = 5 * (2.0 * ne1 * ne1 * ne0 + 2.0 * ne1 ** 3 + 2.0 * ne0 * ne1 * ne1)
        res = {k: {"median_us": statistics.median(v), "min_us": min(v), "tflops_full": flop / statistics.median(v) * 1e-6} for k, v in ts.items()}
        ref = composed().float()
        torch.cuda.synchronize()
        res["rel_diff"] = float((Xa.float() - ref).norm() / ref.norm())
        out["%s %dx%d" % (name, ne0, ne1)] = res
        print(name, ne0, ne1, json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    out = {}
    main(out)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
