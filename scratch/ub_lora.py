"""The adapter launches against what they stand beside and what they make unnecessary, timed in one run at the Qwen3-0.6B shapes and 8 x 1024 tokens, rank 16 and 64:
  fwd     kf_lora_forward                                     (one launch: ax, then y += in place)
  bwd     kf_lora_backward                                    (four launches: the transposes, the row side, both gradients' slabs, the finish)
  base    kf_linear_backward with delta only (gW = NULL)      (what an adapted matrix still runs)
  full    kf_linear_backward with delta and gW                (what a shadow-weight matrix runs): full - base is the weight-gradient product the adapter drops
then the whole step, Qwen3Step.step under "weights" (twice: the run-to-run spread of the unchanged path) and under "lora" at both ranks.  Each figure is the mean of
REPS launches, measured ROUNDS times: printed are the median and the spread (max - min) over the rounds."""
import os, sys, ctypes as C, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koifish_amd.runtime import Context
from koifish_amd import lib as L, synth
from koifish_amd.train_step import Qwen3Step
ctx = Context(0); dev = ctx.device; hip = ctx.hip
bf = torch.bfloat16
B, T = 8, 1024
n = B * T


def timed(fn, reps=10, rounds=5):
    for _ in range(2): fn()
    out = []
    for _ in range(rounds):
        ctx.sync(); e0, e1 = ctx.event(), ctx.event(); ctx.record(e0)
        for _ in range(reps): fn()
        ctx.record(e1); ctx.sync(); out.append(ctx.elapsed_ms(e0, e1) / reps * 1e3)
    return statistics.median(out), max(out) - min(out)


cfg = synth.CONFIGS["qwen3-0.6b"]
shapes = Qwen3Step._mat_shapes(cfg)
print("%-5s %5s x %5s  r  | %9s %9s | %9s %9s  (gW) %8s | adapter - gW" % ("", "OC", "IC", "fwd us", "bwd us", "base us", "full us", "us"))
for name in ("q", "k", "o", "gate", "down"):   # v is k's shape, up is gate's
    OC, IC = shapes[name]
    W = (torch.randn(OC, IC, device=dev) * 0.02).to(bf)
    dw = ctx.quantize(W, L.Q4); d = dw.desc()
    x = torch.randn(n, IC, device=dev).to(bf); dIn = (torch.randn(n, OC, device=dev) / 64).to(bf)
    y = torch.zeros(n, OC, device=dev, dtype=bf); delta = torch.zeros(n, IC, device=dev, dtype=bf); gW = torch.zeros(OC, IC, device=dev, dtype=bf)
    sc = torch.empty(hip.kf_linear_backward_scratch_bytes(OC, IC, n) + 256, dtype=torch.uint8, device=dev); sp = (sc.data_ptr() + 255) & ~255
    def run_base(): L.check(hip.kf_linear_backward(ctx.h, C.byref(d), dIn.data_ptr(), x.data_ptr(), delta.data_ptr(), None, None, n, 0, sp), "base")
    def run_full(): L.check(hip.kf_linear_backward(ctx.h, C.byref(d), dIn.data_ptr(), x.data_ptr(), delta.data_ptr(), gW.data_ptr(), None, n, 0, sp), "full")
    t_b, s_b = timed(run_base); t_f, s_f = timed(run_full)
    for r in (16, 64):
        a = (torch.randn(r, IC, device=dev) * 0.02).to(bf); b = (torch.randn(OC, r, device=dev) * 0.02).to(bf)
        ax = torch.zeros(n, r, device=dev, dtype=bf); g = torch.zeros(r * (IC + OC), device=dev, dtype=bf)
        sl = torch.empty(hip.kf_lora_backward_scratch_bytes(r, OC, IC, n) + 256, dtype=torch.uint8, device=dev); spl = (sl.data_ptr() + 255) & ~255
        def run_fwd(): L.check(hip.kf_lora_forward(ctx.h, a.data_ptr(), b.data_ptr(), r, OC, IC, x.data_ptr(), y.data_ptr(), ax.data_ptr(), n, 0.5), "fwd")
        def run_bwd(): L.check(hip.kf_lora_backward(ctx.h, a.data_ptr(), b.data_ptr(), r, OC, IC, dIn.data_ptr(), x.data_ptr(), ax.data_ptr(), delta.data_ptr(), g.data_ptr(), n, 0.5, spl), "bwd")
        t_fw, s_fw = timed(run_fwd); t_bw, s_bw = timed(run_bwd)
        print("%-5s %5d x %5d %2d  | %9.1f %9.1f | %9.1f %9.1f  %13.1f | %+9.1f   (spreads %.1f %.1f %.1f %.1f)"
              % (name, OC, IC, r, t_fw, t_bw, t_b, t_f, t_f - t_b, t_fw + t_bw - (t_f - t_b), s_fw, s_bw, s_b, s_f))
    del W, dw, x, dIn, y, delta, gW, sc

ids = torch.randint(0, cfg["vocab"], (n,), device=dev, dtype=torch.int32)
tgt = torch.randint(0, cfg["vocab"], (n,), device=dev, dtype=torch.int32)
for label, kw in (("weights", {}), ("weights (again)", {}), ("lora r16", dict(train_target="lora", lora_rank=16)), ("lora r64", dict(train_target="lora", lora_rank=64))):
    st = Qwen3Step(ctx, cfg, B, T, **kw)
    t_s, s_s = timed(lambda: st.step(ids, tgt), reps=2, rounds=3)
    print("Qwen3-0.6B, 8 x 1024 tokens, 4-bit layers, %-16s %11d trained parameters: Qwen3Step.step %9.1f us (spread %.1f) = %.0f tokens/s" % (label + ":", st.n_params(), t_s, s_s, n / t_s * 1e6))
    st.close(); del st
    torch.cuda.empty_cache()
