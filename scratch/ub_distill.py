"""kf_distill_classifier beside kf_fused_classifier at 8192 rows of the GPT-2 and the Qwen3 vocabulary (time, bytes/s over the compulsory traffic: read z, read u, write
dlogits = 3 V 2 bytes per row for the distilling kernel, 2 V 2 for the plain one), then a Qwen3-0.6B-shaped training step of 8 x 1024 tokens: the plain step, a teacher's
forward_logits alone, the distilling step.  `--plain-only` times the plain step alone and touches nothing this script's own commit added: run on a checkout of the
parent commit (KF_TREE=<that checkout>) it gives the baseline of the same session.  `--kernels-only` stops after the two kernels (what a counter run wraps:
rocprofv3 --pmc VALUBusy -d <dir> -- python scratch/ub_distill.py --kernels-only; counters in a run of their own, never beside a trace).  NL=<layers> shortens the model."""
import os, sys, torch
sys.path.insert(0, os.environ.get("KF_TREE", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from koifish_amd.runtime import Context
from koifish_amd.train_step import Qwen3Step
ctx = Context(0); dev = ctx.device
plain_only = "--plain-only" in sys.argv
def timed(fn, reps=50, warm=3):
    for _ in range(warm): fn()
    ctx.sync(); e0, e1 = ctx.event(), ctx.event(); ctx.record(e0)
    for _ in range(reps): fn()
    ctx.record(e1); return ctx.elapsed_ms(e0, e1) / reps
if not plain_only:
    B, T = 8, 1024
    for V, P in ((50257, 50264), (151936, 151936)):
        lg = torch.empty(B * T, P, dtype=torch.bfloat16, device=dev); te = torch.empty(B * T, P, dtype=torch.bfloat16, device=dev)
        for r in range(0, B * T, 1024): lg[r:r + 1024] = (torch.randn(1024, P, device=dev) * 2.0).to(torch.bfloat16); te[r:r + 1024] = (torch.randn(1024, P, device=dev) * 3.0).to(torch.bfloat16)
        keep = lg.clone()
        tg = torch.randint(0, V, (B * T,), device=dev, dtype=torch.int32)
        losses = torch.zeros(B * T, dtype=torch.float32, device=dev); kd = torch.zeros(B * T, dtype=torch.float32, device=dev)
        # every timed call starts from logits, not from the gradient the call before left there: the copy is timed alone and subtracted
        t_copy = timed(lambda: lg.copy_(keep))
        def ce(): lg.copy_(keep); ctx.hip.kf_fused_classifier(ctx.h, lg.data_ptr(), losses.data_ptr(), None, 1.0 / (B * T), tg.data_ptr(), B, T, V, P, None, 1)
        def kdc(a=0.5, b=0.5, tau=2.0): lg.copy_(keep); ctx.hip.kf_distill_classifier(ctx.h, lg.data_ptr(), te.data_ptr(), P, losses.data_ptr(), kd.data_ptr(), 1.0 / (B * T), tg.data_ptr(), B, T, V, P, None, a, b, tau, 1)
        t_ce, t_kd, t_kd0 = timed(ce) - t_copy, timed(kdc) - t_copy, timed(lambda: kdc(1.0, 0.0, 1.0)) - t_copy
        b_ce, b_kd = B * T * V * 2 * 2, B * T * V * 2 * 3
        print(f"8192 x {V}: fused_classifier {t_ce:.3f} ms {b_ce / t_ce / 1e6:.0f} GB/s ({t_ce / b_ce * 1e9:.3f} ps/B) | distill_classifier {t_kd:.3f} ms {b_kd / t_kd / 1e6:.0f} GB/s "
              f"({t_kd / b_kd * 1e9:.3f} ps/B, {t_kd / b_kd / (t_ce / b_ce):.2f} x per byte) | distill_classifier kd_weight 0: {t_kd0:.3f} ms | logits copy {t_copy:.3f} ms", flush=True)
        del lg, te, keep
if "--kernels-only" in sys.argv: sys.exit(0)
cfg = dict(dim=1024, n_layer=int(os.environ.get("NL", "28")), n_head=16, n_kv=8, head_dim=128, ffn=3072, vocab=151936, theta=1e6, rms_eps=1e-6)
B, T = 8, 1024
ids = torch.randint(0, cfg["vocab"], (B * T,), device=dev, dtype=torch.int32); tgt = torch.randint(0, cfg["vocab"], (B * T,), device=dev, dtype=torch.int32)
st = Qwen3Step(ctx, cfg, B, T, seed=1)
t_plain = timed(lambda: st.step(ids, tgt), reps=5, warm=1)
print(f"Qwen3-0.6B shape ({cfg['n_layer']} layers), 8 x 1024 tokens: plain step {t_plain:.1f} ms", flush=True)
if not plain_only:
    te = Qwen3Step(ctx, cfg, B, T, seed=2)
    t_teach = timed(lambda: te.forward_logits(ids), reps=5, warm=1)
    st.set_distill(te, kd_weight=0.5, ce_weight=0.5, temperature=2.0)
    t_dist = timed(lambda: st.step(ids, tgt), reps=5, warm=1)
    kl = st.kd_loss()
    st.set_distill(None)
    t_again = timed(lambda: st.step(ids, tgt), reps=5, warm=1)
    print(f"teacher forward_logits {t_teach:.1f} ms | distilling step (teacher forward included) {t_dist:.1f} ms = plain + {t_dist - t_plain:.1f} ms | plain step again {t_again:.1f} ms | "
          f"mean KL of the last step {kl:.4f}", flush=True)
