"""Packed documents at Qwen3-0.6B shapes (16 / 8 heads of 128, 8 x 1024 rows).  Events go around steady-state windows, and the two sides alternate in one run.
(a) kf_attn_prefill_docs / kf_attn_backward_docs with 8 documents of 1024 rows against kf_attn_prefill_batch_strided / kf_attn_backward on the same tensors: the
    arithmetic is identical, only the table read is added.  Printed: the median of each side over the repeats, the spread (max - min) between the repeats of the plain
    form, and whether docs <= plain + spread.
(b) a seeded mix of document lengths, log-uniform in 32 .. 1024, back to back over the 8192 rows: the whole Qwen3Step.step with the documents set against the plain
    step (recorded, not gated), the attention launches' share of each, and -- computed, not timed -- the rows the same samples would occupy padded one per row.
NL=<layers> shortens the model of (b); `--kernels-only` stops after (a)."""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.environ.get("KF_TREE", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from koifish_amd.runtime import Context
from koifish_amd.train_step import Qwen3Step
ctx = Context(0); dev, hip = ctx.device, ctx.hip
H, KV, hd, B, T = 16, 8, 128, 8, 1024
N, Cq, Ck = B * T, H * hd, KV * hd
W = Cq + 2 * Ck
def window(fn, reps):
    ctx.sync(); e0, e1 = ctx.event(), ctx.event(); ctx.record(e0)
    for _ in range(reps): fn()
    ctx.record(e1); return ctx.elapsed_ms(e0, e1) / reps * 1e3   # us per call
def alternate(sides, reps, rounds, warm=2):
    """sides: {name: fn}; every round times one window of every side in turn; returns {name: [us per call, one per round]}"""
    for fn in sides.values():
        for _ in range(warm): fn()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items(): out[k].append(window(fn, reps))
    return out
def table(rows, lens):
    r, l = np.asarray(rows, dtype=np.int32), np.asarray(lens, dtype=np.int32)
    g = (r.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), len(l), N, T, H, KV, hd)
    t = np.zeros(hip.kf_attn_docs_table_bytes(*g), dtype=np.uint8)
    assert t.size and hip.kf_attn_docs_plan(*g, t.ctypes.data_as(C.c_void_p), t.size) == 0
    return t, torch.from_numpy(t).to(dev)
qkv = torch.randn(N, W, device=dev).to(torch.bfloat16); dO = torch.randn(N, Cq, device=dev).to(torch.bfloat16)
out = torch.zeros(N, Cq, dtype=torch.bfloat16, device=dev); dqkv = torch.zeros(N, W, dtype=torch.bfloat16, device=dev)
sc = torch.zeros(hip.kf_attn_backward_scratch_bytes(T, H, B) // 4 + 1, dtype=torch.float32, device=dev)
q, k, v, dq, dk, dv = (t_.data_ptr() for t_ in (qkv, qkv[:, Cq:], qkv[:, Cq + Ck:], dqkv, dqkv[:, Cq:], dqkv[:, Cq + Ck:]))
def attn_sides(tab, d_tab):
    hp = tab.ctypes.data_as(C.c_void_p)
    return (dict(plain=lambda: hip.kf_attn_prefill_batch_strided(ctx.h, q, k, v, out.data_ptr(), T, W, Cq, H, KV, hd, W, B),
                 docs=lambda: hip.kf_attn_prefill_docs(ctx.h, q, k, v, out.data_ptr(), hp, d_tab.data_ptr(), W, Cq, H, KV, hd, W)),
            dict(plain=lambda: hip.kf_attn_backward(ctx.h, q, k, v, W, out.data_ptr(), dO.data_ptr(), Cq, dq, dk, dv, W, T, H, KV, hd, B, sc.data_ptr()),
                 docs=lambda: hip.kf_attn_backward_docs(ctx.h, q, k, v, W, out.data_ptr(), dO.data_ptr(), Cq, dq, dk, dv, W, hp, d_tab.data_ptr(), H, KV, hd, sc.data_ptr())))
tab, d_tab = table([i * T for i in range(B)], [T] * B)
for name, sides in zip(("forward", "backward"), attn_sides(tab, d_tab)):
    assert all(fn() == 0 for fn in sides.values()), hip.kf_last_error()
    r = alternate(sides, reps=20, rounds=7)
    p, d = np.array(r["plain"]), np.array(r["docs"])
    spread = p.max() - p.min()
    print(f"(a) {name}, 8 documents of 1024: plain median {np.median(p):.1f} us (min {p.min():.1f}, max {p.max():.1f}, spread {spread:.1f}) | docs median {np.median(d):.1f} us "
          f"(min {d.min():.1f}, max {d.max():.1f}) | docs - plain {np.median(d) - np.median(p):+.1f} us | docs <= plain + spread: {bool(np.median(d) <= np.median(p) + spread)}", flush=True)
# (b) the seeded mix
rng = np.random.default_rng(20240)
lens, left = [], N
while left:
    n = min(int(round(float(np.exp(rng.uniform(np.log(32), np.log(1024)))))), left)
    lens.append(n); left -= n
rows = [int(x) for x in np.cumsum([0] + lens[:-1])]
print(f"(b) {len(lens)} documents, log-uniform 32 .. 1024, mean {np.mean(lens):.0f} rows, back to back in {N} rows; padded one per row of {T}: {len(lens) * T} rows "
      f"({len(lens) * T / N:.2f} x the packed rows)", flush=True)
mtab, d_mtab = table(rows, lens)
for name, sides in zip(("forward", "backward"), attn_sides(mtab, d_mtab)):
    r = alternate(sides, reps=20, rounds=5)
    print(f"(b) attention {name}: plain geometry {np.median(r['plain']):.1f} us | the mix {np.median(r['docs']):.1f} us", flush=True)
    if name == "forward": a_f = {k_: float(np.median(v_)) for k_, v_ in r.items()}
    else: a_b = {k_: float(np.median(v_)) for k_, v_ in r.items()}
if "--kernels-only" in sys.argv: sys.exit(0)
cfg = dict(dim=1024, n_layer=int(os.environ.get("NL", "28")), n_head=H, n_kv=KV, head_dim=hd, ffn=3072, vocab=151936, theta=1e6, rms_eps=1e-6)
ids = torch.randint(0, cfg["vocab"], (N,), device=dev, dtype=torch.int32); tgt = torch.randint(0, cfg["vocab"], (N,), device=dev, dtype=torch.int32)
st = Qwen3Step(ctx, cfg, B, T, seed=1)
res = {"plain": [], "docs": []}
for rnd in range(3):
    for side in ("plain", "docs"):
        st.set_documents(lens if side == "docs" else None)
        st.step(ids, tgt)
        res[side].append(window(lambda: st.step(ids, tgt), 3) / 1e3)
NL = cfg["n_layer"]
for side in ("plain", "docs"):
    att = NL * (a_f[side] + a_b[side]) / 1e3
    print(f"(b) Qwen3-0.6B shape ({NL} layers) step, {side}: median {np.median(res[side]):.1f} ms (min {min(res[side]):.1f}, max {max(res[side]):.1f}); attention launches "
          f"{att:.1f} ms = {100 * att / np.median(res[side]):.1f} %", flush=True)
