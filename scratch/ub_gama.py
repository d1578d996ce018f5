"""kf_gama_backward against what it stands beside and what it makes unnecessary, timed in the same run:
  gama    kf_gama_backward                                   (the (zero, step) gradients, 2 values per 128 weights)
  gW      kf_linear_backward with only gW wanted             (the same contraction, the whole [OC, IC] gradient stored)
  upd     kf_adamw on the [OC, IC] master + kf_quantize      (the shadow-weight update a gama-trained matrix never runs)
at config 3's 4-bit shapes (6400 x 1600 and 1600 x 6400, n = 8192) and Qwen3-0.6B's (3072 x 1024, 1024 x 3072, n = 2048).  Each figure is the mean of REPS launches,
measured ROUNDS times: printed are the median and the spread (max - min) over the rounds.  A shape kf_gama_backward refuses is reported as such (6400 x 1600: 1600 input
features are no whole number of 128-weight groups per row)."""
import os, sys, ctypes as C, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koifish_amd.runtime import Context
from koifish_amd import lib as L
ctx = Context(0); dev = ctx.device; hip = ctx.hip
REPS, ROUNDS = 10, 5


def timed(fn):
    for _ in range(3): fn()
    out = []
    for _ in range(ROUNDS):
        ctx.sync(); e0, e1 = ctx.event(), ctx.event(); ctx.record(e0)
        for _ in range(REPS): fn()
        ctx.record(e1); out.append(ctx.elapsed_ms(e0, e1) / REPS * 1e3)
    return statistics.median(out), max(out) - min(out)


for name, OC, IC, n in (("gpt2 fc", 6400, 1600, 8192), ("gpt2 proj2", 1600, 6400, 8192), ("qwen3 up", 3072, 1024, 2048), ("qwen3 down", 1024, 3072, 2048)):
    W = (torch.randn(OC, IC, device=dev) * 0.02).to(torch.bfloat16)
    dw = ctx.quantize(W, L.Q4); d = dw.desc()
    dIn = (torch.randn(n, OC, device=dev) / 64).to(torch.bfloat16); inp = torch.randn(n, IC, device=dev).to(torch.bfloat16)
    gW = torch.zeros(OC, IC, device=dev, dtype=torch.bfloat16); m = torch.zeros_like(gW); v = torch.zeros_like(gW)
    sc = torch.empty(hip.kf_linear_backward_scratch_bytes(OC, IC, n) + 256, dtype=torch.uint8, device=dev); sp = (sc.data_ptr() + 255) & ~255
    def run_gw(): L.check(hip.kf_linear_backward(ctx.h, C.byref(d), dIn.data_ptr(), inp.data_ptr(), None, gW.data_ptr(), None, n, 0, sp), "gW")
    def run_upd():
        L.check(hip.kf_adamw(ctx.h, W.data_ptr(), gW.data_ptr(), m.data_ptr(), v.data_ptr(), OC * IC, L.BF16, 1e-4, 0.9, 0.95, 0.1, 0.05, 1e-8, 0.1, 1.0, 7, None), "adamw")
        L.check(hip.kf_quantize(ctx.h, C.byref(d), W.data_ptr(), 0), "quantize")
    t_gw, s_gw = timed(run_gw)
    t_up, s_up = timed(run_upd)
    nb = hip.kf_gama_backward_scratch_bytes(OC, IC, n)
    if nb == 0:
        print("%-10s %5d x %5d n %5d: gama REFUSED (IC %% 128 = %d)   gW %7.1f us (spread %.1f)   adamw + quantize %7.1f us (spread %.1f)" % (name, OC, IC, n, IC % 128, t_gw, s_gw, t_up, s_up))
        continue
    g = torch.zeros(2 * dw.nGroup, device=dev, dtype=torch.bfloat16)
    sg = torch.empty(nb + 256, dtype=torch.uint8, device=dev); spg = (sg.data_ptr() + 255) & ~255
    def run_gama(): L.check(hip.kf_gama_backward(ctx.h, C.byref(d), dIn.data_ptr(), inp.data_ptr(), g.data_ptr(), n, 1.0, spg), "gama")
    t_ga, s_ga = timed(run_gama)
    print("%-10s %5d x %5d n %5d: gama %7.1f us (spread %.1f, %d slab(s), %.0f TFLOP/s)   gW %7.1f us (spread %.1f)   adamw + quantize %7.1f us (spread %.1f)"
          % (name, OC, IC, n, t_ga, s_ga, nb // (2 * dw.nGroup * 4), 2.0 * n * OC * IC / t_ga / 1e6, t_gw, s_gw, t_up, s_up))
