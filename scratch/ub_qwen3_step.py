"""The Qwen3 training step, timed in one run:
  entry   kf_qknorm_rope_backward                                                       (one pass: RoPE^T, q/k-norm backward, the dense copies, dwq / dwk)
  route   the unchanged route it replaces: 2 x kf_rope_backward in place, 3 strided-to-dense copies (copy_ into preallocated buffers), 2 zero fills, 2 x kf_norm_backward
at n_tok 8192, 16 / 8 heads of 128, and
  step    one Qwen3Step.step at the Qwen3-0.6B shape (28 layers, dim 1024, ffn 3072, V 151936), 8 x 1024 tokens, 4-bit layers.
Each figure is the mean of REPS launches, measured ROUNDS times: printed are the median and the spread (max - min) over the rounds.  The entry's bytes are the
algorithmic ones: read dq | dk | dv and raw q | k, write dq_raw | dk_raw | dv_out (2 bytes each; rstd, the table and the weights are noise beside them)."""
import os, sys, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koifish_amd.runtime import Context
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.train_step import Qwen3Step
ctx = Context(0); dev = ctx.device; hip = ctx.hip
REPS, ROUNDS = 10, 5
PEAK = 8.0e12


def timed(fn, reps=REPS, rounds=ROUNDS):
    for _ in range(2): fn()
    out = []
    for _ in range(rounds):
        ctx.sync(); e0, e1 = ctx.event(), ctx.event(); ctx.record(e0)
        for _ in range(reps): fn()
        ctx.record(e1); out.append(ctx.elapsed_ms(e0, e1) / reps * 1e3)
    return statistics.median(out), max(out) - min(out)


n_tok, T, H, KV, hd = 8192, 1024, 16, 8, 128
Cq, Ck = H * hd, KV * hd
W_ = Cq + 2 * Ck
bf = torch.bfloat16
d = (torch.randn(n_tok, W_, device=dev) * 0.05).to(bf)
qraw, kraw = torch.randn(n_tok, Cq, device=dev).to(bf), torch.randn(n_tok, Ck, device=dev).to(bf)
wq, wk = torch.ones(hd, device=dev, dtype=bf), torch.ones(hd, device=dev, dtype=bf)
rq, rk = torch.rand(n_tok * H, device=dev) + 0.5, torch.rand(n_tok * KV, device=dev) + 0.5
table = ctx.rope_table(T, hd, 1e6)
dq, dk, dv = torch.empty(n_tok, Cq, device=dev, dtype=bf), torch.empty(n_tok, Ck, device=dev, dtype=bf), torch.empty(n_tok, Ck, device=dev, dtype=bf)
dwq, dwk = torch.zeros(hd, device=dev, dtype=bf), torch.zeros(hd, device=dev, dtype=bf)
sc = torch.empty(hip.kf_qknorm_rope_backward_scratch_bytes(n_tok, H, KV, hd) // 8 + 1, dtype=torch.float64, device=dev)


def entry():
    L.check(hip.kf_qknorm_rope_backward(ctx.h, d.data_ptr(), d[:, Cq:].data_ptr(), d[:, Cq + Ck:].data_ptr(), W_, qraw.data_ptr(), Cq, kraw.data_ptr(), Ck, wq.data_ptr(), wk.data_ptr(),
                                        rq.data_ptr(), rk.data_ptr(), table.data_ptr(), n_tok, T, H, KV, hd, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dwq.data_ptr(), dwk.data_ptr(),
                                        sc.data_ptr()), "kf_qknorm_rope_backward")


# the route's dense operands are allocated once and filled with copy_: the timed region holds kernels and device copies only, no allocator call.  The rotation works in
# place, so every repetition rotates d2 once more: a rotation keeps magnitudes, and none of these kernels' time depends on the values.
d2 = d.clone()
a_, b_, c_ = torch.empty(n_tok, Cq, device=dev, dtype=bf), torch.empty(n_tok, Ck, device=dev, dtype=bf), torch.empty(n_tok, Ck, device=dev, dtype=bf)
dq2, dk2 = torch.empty(n_tok, Cq, device=dev, dtype=bf), torch.empty(n_tok, Ck, device=dev, dtype=bf)
dwq2, dwk2 = torch.zeros(hd, device=dev, dtype=bf), torch.zeros(hd, device=dev, dtype=bf)
scq = torch.empty(hip.kf_norm_backward_scratch_bytes(n_tok * H, hd, 0) // 8 + 1, dtype=torch.float64, device=dev)


def route():
    L.check(hip.kf_rope_backward(ctx.h, d2.data_ptr(), table.data_ptr(), 0, n_tok, T, W_, H, hd), "rope_bwd")
    L.check(hip.kf_rope_backward(ctx.h, d2[:, Cq:].data_ptr(), table.data_ptr(), 0, n_tok, T, W_, KV, hd), "rope_bwd")
    a_.copy_(d2[:, :Cq]); b_.copy_(d2[:, Cq:Cq + Ck]); c_.copy_(d2[:, Cq + Ck:])
    L.check(hip.kf_memset32(ctx.h, dq2.data_ptr(), 0, dq2.numel() // 2), "memset")
    L.check(hip.kf_memset32(ctx.h, dk2.data_ptr(), 0, dk2.numel() // 2), "memset")
    L.check(hip.kf_norm_backward(ctx.h, dq2.data_ptr(), dwq2.data_ptr(), None, a_.data_ptr(), qraw.data_ptr(), wq.data_ptr(), None, rq.data_ptr(), n_tok * H, hd, scq.data_ptr()), "norm_bwd")
    L.check(hip.kf_norm_backward(ctx.h, dk2.data_ptr(), dwk2.data_ptr(), None, b_.data_ptr(), kraw.data_ptr(), wk.data_ptr(), None, rk.data_ptr(), n_tok * KV, hd, scq.data_ptr()), "norm_bwd")


t_e, s_e = timed(entry)
t_r, s_r = timed(route)
nbytes = 2 * n_tok * (W_ + Cq + Ck + W_)
print("n_tok %d, %d / %d heads of %d: kf_qknorm_rope_backward %7.1f us (spread %.1f) = %.2f TB/s = %.0f %% of %.0f TB/s   two-launch route %7.1f us (spread %.1f)"
      % (n_tok, H, KV, hd, t_e, s_e, nbytes / t_e / 1e6, 100 * nbytes / t_e * 1e6 / PEAK, PEAK / 1e12, t_r, s_r))

cfg = synth.CONFIGS["qwen3-0.6b"]
st = Qwen3Step(ctx, cfg, 8, 1024)
ids = torch.randint(0, cfg["vocab"], (8 * 1024,), device=dev, dtype=torch.int32)
tgt = torch.randint(0, cfg["vocab"], (8 * 1024,), device=dev, dtype=torch.int32)
t_s, s_s = timed(lambda: st.step(ids, tgt), reps=2, rounds=3)
print("Qwen3-0.6B, 8 x 1024 tokens, 4-bit layers, %d parameters: Qwen3Step.step %9.1f us (spread %.1f) = %.0f tokens/s" % (st.n_params(), t_s, s_s, 8192 / t_s * 1e6))
