"""kf_qknorm_rope_backward alone: the backward of the per-head q/k RMSNorm + rotate-half RoPE in one entry, against torch fp64 autograd of rope(rmsnorm(q_raw) * w) on the
same bf16 inputs, side by side with the UNCHANGED two-launch route (kf_rope_backward in place + kf_norm_backward over n_tok * heads rows of head_dim).

Acceptance (set by the issue): per output tensor, the max and the rms deviation from fp64 as fractions of the tensor's largest magnitude; the new entry's figures may
exceed the old route's by at most 2^-9 (half a bf16 ulp of the scale: its summation order over the rows differs), and neither route may exceed max 2^-5 / rms 2^-7 for
dq_raw, dk_raw and max 2^-5 / rms 2^-6 for the weight gradients -- the bounds of tests/test_gpu_train_step.py::test_qwen3_toy_training_step_vs_autograd.  As there, the
expectation does not include the forward's rounding of rstd: the device's rstd is the fp32 one kf_qknorm_rope_train writes."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu
EPS, THETA, PAD = 1e-6, 10000.0, 24
CASES = [(4, 2, 64, 2, 40), (2, 2, 128, 3, 17), (16, 8, 128, 1, 64)]


def _case(ctx, n_head, n_kv, hd, n_seq, seq_len):
    """inputs on the device (rows wider than their dense width), the forward's rstd, and the fp64 expectation"""
    rng = np.random.default_rng(1000 * n_head + hd + seq_len)
    n_tok, Cq, Ck = n_seq * seq_len, n_head * hd, n_kv * hd
    dev = ctx.device
    mk = lambda *s, std=1.0: O.f32_to_bf16(rng.normal(0, std, size=s).astype(np.float32))
    ld_d, ld_q, ld_k = Cq + 2 * Ck + PAD, Cq + 8, Ck + 16
    d = bf16_t(mk(n_tok, ld_d, std=0.05), dev)                       # dq | dk | dv column blocks + padding columns
    qraw, kraw = bf16_t(mk(n_tok, ld_q), dev), bf16_t(mk(n_tok, ld_k), dev)
    wq = bf16_t(O.f32_to_bf16((1 + rng.normal(0, 0.1, hd)).astype(np.float32)), dev)
    wk = bf16_t(O.f32_to_bf16((1 + rng.normal(0, 0.1, hd)).astype(np.float32)), dev)
    table = ctx.rope_table(seq_len, hd, THETA)
    # the forward, for its rstd (on copies: it works in place)
    q2, k2 = qraw.clone(), kraw.clone()
    rq, rk = torch.zeros(n_tok * n_head, dtype=torch.float32, device=dev), torch.zeros(n_tok * n_kv, dtype=torch.float32, device=dev)
    L.check(ctx.hip.kf_qknorm_rope_train(ctx.h, q2.data_ptr(), k2.data_ptr(), wq.data_ptr(), wk.data_ptr(), table.data_ptr(), n_tok, seq_len, ld_q, ld_k, n_head, n_kv, hd, EPS,
                                         rq.data_ptr(), rk.data_ptr()), "kf_qknorm_rope_train")
    # fp64 autograd of rope(rmsnorm(raw) * w) against the given output gradients
    f64 = lambda t_: torch.tensor(O.bf16_to_f32(u16(t_)).astype(np.float64))
    ang = torch.arange(seq_len, dtype=torch.float64)[:, None] * (1.0 / (THETA ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd)))[None, :]
    cs, sn = torch.cos(ang)[None, :, None, :], torch.sin(ang)[None, :, None, :]
    want = {}
    for nm, raw, w, nh, c0, ld in (("q", qraw, wq, n_head, 0, ld_q), ("k", kraw, wk, n_kv, Cq, ld_k)):
        x = f64(raw)[:, :nh * hd].reshape(n_seq, seq_len, nh, hd).clone().requires_grad_(True)
        wt = f64(w).clone().requires_grad_(True)
        y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS) * wt
        a, b = y[..., :hd // 2], y[..., hd // 2:]
        out = torch.cat([a * cs - b * sn, a * sn + b * cs], dim=-1)
        out.backward(f64(d)[:, c0:c0 + nh * hd].reshape(n_seq, seq_len, nh, hd))
        want["d%s_raw" % nm], want["dw%s" % nm] = x.grad.reshape(n_tok, nh * hd).numpy(), wt.grad.numpy()
    return dict(d=d, qraw=qraw, kraw=kraw, wq=wq, wk=wk, table=table, rq=rq, rk=rk, ld=(ld_d, ld_q, ld_k), want=want, n_tok=n_tok, Cq=Cq, Ck=Ck)


def _dev(got_bf16, ref, minus=None):
    got = O.bf16_to_f32(u16(got_bf16)).astype(np.float64).reshape(ref.shape)
    if minus is not None:
        got = got - minus
    sc_ = np.abs(ref).max()
    return float(np.abs(got - ref).max() / sc_), float(np.sqrt(((got - ref) ** 2).mean()) / sc_)


def _new(ctx, c, n_head, n_kv, hd, seq_len, with_dv, dw0, garbage):
    """one call of the new entry; outputs sit inside larger allocations planted with a fill value"""
    dev, n_tok, Cq, Ck = ctx.device, c["n_tok"], c["Cq"], c["Ck"]
    FILL, TAIL = 0x4D4D, 64
    fill = lambda n: torch.full((n + TAIL,), FILL, dtype=torch.int16, device=dev).view(torch.bfloat16)
    dq, dk, dv = fill(n_tok * Cq), fill(n_tok * Ck), fill(n_tok * Ck)
    dwq, dwk = torch.cat([dw0[0].clone(), fill(0)]), torch.cat([dw0[1].clone(), fill(0)])
    nb = ctx.hip.kf_qknorm_rope_backward_scratch_bytes(n_tok, n_head, n_kv, hd)
    assert nb > 0
    sc = torch.full((nb // 8 + 1,), garbage, dtype=torch.float64, device=dev)
    d = c["d"]
    rc = ctx.hip.kf_qknorm_rope_backward(ctx.h, d.data_ptr(), d[:, Cq:].data_ptr(), d[:, Cq + Ck:].data_ptr() if with_dv else None, c["ld"][0], c["qraw"].data_ptr(), c["ld"][1],
                                         c["kraw"].data_ptr(), c["ld"][2], c["wq"].data_ptr(), c["wk"].data_ptr(), c["rq"].data_ptr(), c["rk"].data_ptr(), c["table"].data_ptr(),
                                         n_tok, seq_len, n_head, n_kv, hd, dq.data_ptr(), dk.data_ptr(), dv.data_ptr() if with_dv else None, dwq.data_ptr(), dwk.data_ptr(),
                                         sc.data_ptr())
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    for t_, n in ((dq, n_tok * Cq), (dk, n_tok * Ck), (dv, n_tok * Ck if with_dv else 0), (dwq, hd), (dwk, hd)):
        assert (u16(t_)[n:] == FILL).all(), "an element beyond the written extent changed"
    return dict(dq_raw=dq[:n_tok * Cq], dk_raw=dk[:n_tok * Ck], dv=dv[:n_tok * Ck], dwq=dwq[:hd], dwk=dwk[:hd])


def _old(ctx, c, n_head, n_kv, hd, seq_len, dw0):
    """the unchanged two-launch route of tests/test_gpu_train_step.py: kf_rope_backward in place, dense copies, kf_norm_backward on zero-filled input gradients; its
    weight gradients accumulate onto the same start values as the new entry's (kf_norm_backward: bf16(sum + old)), so both routes round the same kind of sum"""
    dev, n_tok, Cq, Ck = ctx.device, c["n_tok"], c["Cq"], c["Ck"]
    d = c["d"].clone()
    out = {}
    for nm, c0, nh, raw, w, rstd, g0 in (("q", 0, n_head, c["qraw"], c["wq"], c["rq"], dw0[0]), ("k", Cq, n_kv, c["kraw"], c["wk"], c["rk"], dw0[1])):
        L.check(ctx.hip.kf_rope_backward(ctx.h, d[:, c0:].data_ptr(), c["table"].data_ptr(), 0, n_tok, seq_len, c["ld"][0], nh, hd), "kf_rope_backward")
        rows = n_tok * nh
        post, x = d[:, c0:c0 + nh * hd].contiguous().view(rows, hd), raw[:, :nh * hd].contiguous().view(rows, hd)
        dx, gw = torch.zeros(rows, hd, dtype=torch.bfloat16, device=dev), g0.clone()
        sc = torch.empty(ctx.hip.kf_norm_backward_scratch_bytes(rows, hd, 0) // 8 + 1, dtype=torch.float64, device=dev)
        L.check(ctx.hip.kf_norm_backward(ctx.h, dx.data_ptr(), gw.data_ptr(), None, post.data_ptr(), x.data_ptr(), w.data_ptr(), None, rstd.data_ptr(), rows, hd, sc.data_ptr()),
                "kf_norm_backward")
        out["d%s_raw" % nm], out["dw%s" % nm] = dx, gw
    ctx.sync()
    return out


@pytest.mark.parametrize("n_head,n_kv,hd,n_seq,seq_len", CASES)
def test_qknorm_rope_backward_vs_fp64_and_the_two_launch_route(ctx, n_head, n_kv, hd, n_seq, seq_len):
    c = _case(ctx, n_head, n_kv, hd, n_seq, seq_len)
    dev = ctx.device
    rng = np.random.default_rng(5)
    dw0 = [bf16_t(O.f32_to_bf16(rng.normal(0, 0.5, hd).astype(np.float32)), dev) for _ in range(2)]   # dwq / dwk hold something: the entry ACCUMULATES
    old0 = [O.bf16_to_f32(u16(t_)).astype(np.float64) for t_ in dw0]
    new = _new(ctx, c, n_head, n_kv, hd, seq_len, True, dw0, 1e300)
    old = _old(ctx, c, n_head, n_kv, hd, seq_len, dw0)
    for name, (mx_tol, rms_tol) in (("dq_raw", (2.0 ** -5, 2.0 ** -7)), ("dk_raw", (2.0 ** -5, 2.0 ** -7)), ("dwq", (2.0 ** -5, 2.0 ** -6)), ("dwk", (2.0 ** -5, 2.0 ** -6))):
        ref = c["want"][name]
        # a weight gradient: what was accumulated minus the start value (the rounding of bf16(sum + old) is part of both routes' figures)
        start = old0[0 if name == "dwq" else 1] if name.startswith("dw") else None
        n_mx, n_rms = _dev(new[name], ref, minus=start)
        o_mx, o_rms = _dev(old[name], ref, minus=start)
        print("%s heads %d/%d hd %d rows %d x %d: two-launch max %.3e rms %.3e | one entry max %.3e rms %.3e" % (name, n_head, n_kv, hd, n_seq, seq_len, o_mx, o_rms, n_mx, n_rms))
        assert o_mx <= mx_tol and o_rms <= rms_tol, "two-launch route, %s: max %.4f rms %.5f of scale" % (name, o_mx, o_rms)
        assert n_mx <= mx_tol and n_rms <= rms_tol, "kf_qknorm_rope_backward, %s: max %.4f rms %.5f of scale" % (name, n_mx, n_rms)
        assert n_mx <= o_mx + 2.0 ** -9 and n_rms <= o_rms + 2.0 ** -9, "%s: one entry (%.3e, %.3e) against two launches (%.3e, %.3e)" % (name, n_mx, n_rms, o_mx, o_rms)
    # dv_out is dv, bit for bit
    Cq, Ck = c["Cq"], c["Ck"]
    assert np.array_equal(u16(new["dv"]).reshape(c["n_tok"], Ck), u16(c["d"][:, Cq + Ck:Cq + 2 * Ck]))
    # dv NULL: the same q / k results, nothing else written; scratch pre-filled with other garbage: identical bits
    again = _new(ctx, c, n_head, n_kv, hd, seq_len, False, dw0, -7.25)
    for name in ("dq_raw", "dk_raw", "dwq", "dwk"):
        assert np.array_equal(u16(new[name]), u16(again[name])), name
    third = _new(ctx, c, n_head, n_kv, hd, seq_len, True, dw0, float("nan"))
    for name in ("dq_raw", "dk_raw", "dv", "dwq", "dwk"):
        assert np.array_equal(u16(new[name]), u16(third[name])), name


def test_qknorm_rope_backward_refusals(ctx):
    hip, dev = ctx.hip, ctx.device
    n_head, n_kv, hd, seq_len = 4, 2, 64, 8
    c = _case(ctx, n_head, n_kv, hd, 1, seq_len)
    Cq, Ck, n_tok = c["Cq"], c["Ck"], c["n_tok"]
    z = lambda n: torch.zeros(n + 8, dtype=torch.bfloat16, device=dev)
    dq, dk, dv, dwq, dwk = z(n_tok * Cq), z(n_tok * Ck), z(n_tok * Ck), z(hd), z(hd)
    sc = torch.zeros(hip.kf_qknorm_rope_backward_scratch_bytes(n_tok, n_head, n_kv, hd) // 8 + 1, dtype=torch.float64, device=dev)
    d = c["d"]

    def call(**kw):
        a = dict(dq=d.data_ptr(), dk=d[:, Cq:].data_ptr(), dv=d[:, Cq + Ck:].data_ptr(), ld_d=c["ld"][0], qraw=c["qraw"].data_ptr(), ld_q=c["ld"][1], kraw=c["kraw"].data_ptr(),
                 ld_k=c["ld"][2], n_tok=n_tok, seq_len=seq_len, n_head=n_head, n_kv=n_kv, hd=hd, dq_raw=dq.data_ptr(), dv_out=dv.data_ptr(), sc=sc.data_ptr())
        a.update(kw)
        return hip.kf_qknorm_rope_backward(ctx.h, a["dq"], a["dk"], a["dv"], a["ld_d"], a["qraw"], a["ld_q"], a["kraw"], a["ld_k"], c["wq"].data_ptr(), c["wk"].data_ptr(),
                                           c["rq"].data_ptr(), c["rk"].data_ptr(), c["table"].data_ptr(), a["n_tok"], a["seq_len"], a["n_head"], a["n_kv"], a["hd"], a["dq_raw"],
                                           dk.data_ptr(), a["dv_out"], dwq.data_ptr(), dwk.data_ptr(), a["sc"])
    assert call() == 0, hip.kf_last_error()
    assert call(dq=None) == -20 and call(sc=None) == -20 and call(dv_out=None) == -20          # null pointers; dv without dv_out
    assert call(seq_len=3) == -20 and call(n_head=3) == -20 and call(ld_d=Cq - 8) == -20     # n_tok % seq_len, n_head % n_kv, a stride below its row
    assert call(hd=96) == -1000                                                               # KF_UNSUPPORTED_DATATYPE
    assert hip.kf_qknorm_rope_backward_scratch_bytes(n_tok, n_head, n_kv, 96) == 0
    assert call(dq_raw=dq.data_ptr() + 2) == -2000 and call(qraw=c["qraw"].data_ptr() + 2) == -2000   # KF_BLAS_UNALIGN
    ctx.sync()
    assert not u16(dq)[n_tok * Cq:].any()
