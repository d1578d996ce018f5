"""Packed documents on the device: kf_attn_prefill_docs, kf_attn_backward_docs and the _pos forms of the q/k-norm + RoPE entries against the existing single-sequence
entries on each document's slice alone, bit for bit.  The layout is tests/test_sft_docs_cpu.py's: documents of 1, 63, 65, 129 and 96 rows with 0, 0, 3, 0 and 5 gap rows
in front of them in 384 rows (a 22-row gap behind the last); q | k | v are the column blocks of one fused buffer; every output is pre-filled with NaN bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu
LENS, GAPS, N, T = [1, 63, 65, 129, 96], [0, 0, 3, 0, 5], 384, 256
ROWS = [int(sum(LENS[:d]) + sum(GAPS[:d + 1])) for d in range(len(LENS))]
GEOMS = [(64, 4, 2), (128, 4, 2), (128, 4, 1), (64, 2, 2)]   # (head_dim, n_head, n_kv)
NAN16 = -1                                                    # int16 0xFFFF: a bf16 NaN
THETA, EPS = 10000.0, 1e-6


def _gaps(rows=ROWS, lens=LENS, n=N):
    at, out = 0, []
    for r, ln in list(zip(rows, lens)) + [(n, 0)]:
        if r > at:
            out.append((at, r - at))
        at = r + ln
    return out


def _table(ctx, rows, lens, n_rows, max_len, H, KV, hd):
    """(the host table: its head is the header the launches read, its device copy)"""
    r, l = np.asarray(rows, dtype=np.int32), np.asarray(lens, dtype=np.int32)
    geom = (r.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), len(l), n_rows, max_len, H, KV, hd)
    tab = np.zeros(ctx.hip.kf_attn_docs_table_bytes(*geom), dtype=np.uint8)
    assert tab.size and ctx.hip.kf_attn_docs_plan(*geom, tab.ctypes.data_as(C.c_void_p), tab.size) == 0, ctx.hip.kf_last_error()
    return tab, torch.from_numpy(tab).to(ctx.device)


def _nan(ctx, *shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=ctx.device).view(torch.bfloat16)


def _qkv(ctx, n, H, KV, hd, seed):
    rng = np.random.default_rng(seed)
    Cq, Ck = H * hd, KV * hd
    return bf16_t(O.f32_to_bf16(rng.normal(0, 1.0, (n, Cq + 2 * Ck)).astype(np.float32)), ctx.device), Cq, Ck, rng


def _forward_docs(ctx, qkv, tab, d_tab, H, KV, hd, n):
    Cq, Ck = H * hd, KV * hd
    W = Cq + 2 * Ck
    out = _nan(ctx, n, Cq)
    rc = ctx.hip.kf_attn_prefill_docs(ctx.h, qkv.data_ptr(), qkv[:, Cq:].data_ptr(), qkv[:, Cq + Ck:].data_ptr(), out.data_ptr(), tab.ctypes.data_as(C.c_void_p), d_tab.data_ptr(), W, Cq,
                                      H, KV, hd, W)
    assert rc == 0, ctx.hip.kf_last_error()
    return out


@pytest.mark.parametrize("hd,H,KV", GEOMS)
def test_forward_and_backward_equal_the_plain_entries_per_document(ctx, hd, H, KV):
    hip, dev = ctx.hip, ctx.device
    qkv, Cq, Ck, rng = _qkv(ctx, N, H, KV, hd, 7 * hd + H + KV)
    W = Cq + 2 * Ck
    tab, d_tab = _table(ctx, ROWS, LENS, N, T, H, KV, hd)
    out = _forward_docs(ctx, qkv, tab, d_tab, H, KV, hd, N)
    ctx.sync()
    lone = torch.zeros(N, Cq, dtype=torch.bfloat16, device=dev)
    for r, n in zip(ROWS, LENS):   # every length is below ATTN_PAIR_MIN_TOK = 256: the lone call takes the ATTN_TILE route
        s = qkv[r:r + n]
        assert hip.kf_attn_prefill_batch_strided(ctx.h, s.data_ptr(), s[:, Cq:].data_ptr(), s[:, Cq + Ck:].data_ptr(), lone[r:r + n].data_ptr(), n, W, Cq, H, KV, hd, W, 1) == 0, hip.kf_last_error()
    ctx.sync()
    got, want = u16(out), u16(lone)
    for r, n in zip(ROWS, LENS):
        assert np.array_equal(got[r:r + n], want[r:r + n]), "forward, document at row %d" % r
        assert want[r:r + n].any()
    for r, n in _gaps():
        assert not got[r:r + n].any(), "forward: gap rows %d .. %d are not zero" % (r, r + n)

    # the backward: o is the forward's output with the gap rows as the forward left them, dO seeded everywhere (a gap row's dO is never read)
    dO = bf16_t(O.f32_to_bf16(rng.normal(0, 1.0, (N, Cq)).astype(np.float32)), dev)
    dqkv = _nan(ctx, N, W)
    sc = torch.full((hip.kf_attn_backward_docs_scratch_bytes(N, H) // 4,), float("nan"), dtype=torch.float32, device=dev)
    rc = hip.kf_attn_backward_docs(ctx.h, qkv.data_ptr(), qkv[:, Cq:].data_ptr(), qkv[:, Cq + Ck:].data_ptr(), W, out.data_ptr(), dO.data_ptr(), Cq, dqkv.data_ptr(),
                                   dqkv[:, Cq:].data_ptr(), dqkv[:, Cq + Ck:].data_ptr(), W, tab.ctypes.data_as(C.c_void_p), d_tab.data_ptr(), H, KV, hd, sc.data_ptr())
    assert rc == 0, hip.kf_last_error()
    ctx.sync()
    ref = torch.zeros(N, W, dtype=torch.bfloat16, device=dev)
    for r, n in zip(ROWS, LENS):
        s, g = qkv[r:r + n], ref[r:r + n]
        sc1 = torch.zeros(hip.kf_attn_backward_scratch_bytes(n, H, 1) // 4 + 1, dtype=torch.float32, device=dev)
        assert hip.kf_attn_backward(ctx.h, s.data_ptr(), s[:, Cq:].data_ptr(), s[:, Cq + Ck:].data_ptr(), W, out[r:r + n].data_ptr(), dO[r:r + n].data_ptr(), Cq, g.data_ptr(),
                                    g[:, Cq:].data_ptr(), g[:, Cq + Ck:].data_ptr(), W, n, H, KV, hd, 1, sc1.data_ptr()) == 0, hip.kf_last_error()
    ctx.sync()
    got, want = u16(dqkv), u16(ref)
    for name, c0, c1 in (("dq", 0, Cq), ("dk", Cq, Cq + Ck), ("dv", Cq + Ck, W)):
        for r, n in zip(ROWS, LENS):
            assert np.array_equal(got[r:r + n, c0:c1], want[r:r + n, c0:c1]), "%s, document at row %d" % (name, r)
        assert want[:, c0:c1].any()
    for r, n in _gaps():
        assert not got[r:r + n].any(), "backward: gap rows %d .. %d of dq | dk | dv are not zero" % (r, r + n)


@pytest.mark.parametrize("hd,H,KV", GEOMS)
def test_a_long_document_against_fp64_softmax(ctx, hd, H, KV):
    """One document of 300 rows behind a 7-row gap, 13 gap rows behind it.  The lone plain call may take the paired route at this length, so bit equality is not
    claimed; the bar is derived, not measured.  The kernel rounds a scaled score s to bf16 before the softmax (half an ulp: |s| 2^-9), which changes a probability
    by the factor exp(+-|s| 2^-9); with smax the largest scaled score of the case, numerator and denominator of out = sum p v / sum p each move by at most
    smax 2^-9 relative (first order), so |out - ref| <= 2 smax 2^-9 max|v|; the bf16 store of out adds 2^-9 max|v|, and the fp32 sums and the 16-bit probabilities
    of the P.V product stay below another 2^-9 max|v|.  Bar: (2 smax + 2) 2^-9 max|v|, with smax from the fp64 scores of the inputs."""
    n, r0, ln = 320, 7, 300
    qkv, Cq, Ck, _ = _qkv(ctx, n, H, KV, hd, 31 * hd + H)
    tab, d_tab = _table(ctx, [r0], [ln], n, 512, H, KV, hd)
    out = _forward_docs(ctx, qkv, tab, d_tab, H, KV, hd, n)
    ctx.sync()
    got = O.bf16_to_f32(u16(out)).astype(np.float64)
    x = O.bf16_to_f32(u16(qkv)).astype(np.float64)[r0:r0 + ln]
    q, k, v = x[:, :Cq].reshape(ln, H, hd), x[:, Cq:Cq + Ck].reshape(ln, KV, hd), x[:, Cq + Ck:].reshape(ln, KV, hd)
    causal = np.tril(np.ones((ln, ln), dtype=bool))
    worst = 0.0
    for h in range(H):
        g = h // (H // KV)
        s = q[:, h] @ k[:, g].T / np.sqrt(hd)
        smax = np.abs(s[causal]).max()
        s = np.where(causal, s, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        ref = (p / p.sum(axis=1, keepdims=True)) @ v[:, g]
        bar = (2 * smax + 2) * 2.0 ** -9 * np.abs(v[:, g]).max()
        err = np.abs(got[r0:r0 + ln, h * hd:(h + 1) * hd] - ref).max()
        worst = max(worst, err / bar)
        assert err <= bar, "head %d: |out - fp64| %.4g above the bar %.4g" % (h, err, bar)
    print("hd %d heads %d/%d: largest |out - fp64| / bar = %.3f" % (hd, H, KV, worst))
    assert not u16(out)[:r0].any() and not u16(out)[r0 + ln:].any(), "gap rows are zero"


@pytest.mark.parametrize("hd,H,KV", GEOMS)
def test_rope_pos_entries_equal_the_plain_entries_per_document(ctx, hd, H, KV):
    """Forward outputs, rstd, dq_raw, dk_raw and the dense dv: bit for bit the plain entries on each document's slice (seq_len = its length) and on each gap run at
    position 0 (seq_len = 1).  dwq / dwk are ONE sum over all 384 rows in the entry's fixed order, where the per-slice calls give one sum per slice: a different
    order, so they are compared -- against the fp64 sum of the per-slice results, each accumulated from zero -- at the q/k-norm bar of
    tests/test_gpu_qknorm_rope_bwd.py: max 2^-5 and rms 2^-6 of the largest reference magnitude."""
    hip, dev = ctx.hip, ctx.device
    qkv, Cq, Ck, rng = _qkv(ctx, N, H, KV, hd, 3 * hd + 5 * H + KV)
    W = Cq + 2 * Ck
    wq = bf16_t(O.f32_to_bf16((1 + rng.normal(0, 0.1, hd)).astype(np.float32)), dev)
    wk = bf16_t(O.f32_to_bf16((1 + rng.normal(0, 0.1, hd)).astype(np.float32)), dev)
    table = ctx.rope_table(T, hd, THETA)
    pos = np.zeros(N, dtype=np.int32)
    for r, n in zip(ROWS, LENS):
        pos[r:r + n] = np.arange(n)
    d_pos = torch.from_numpy(pos).to(dev)
    runs = [(r, n, n) for r, n in zip(ROWS, LENS)] + [(r, n, 1) for r, n in _gaps()]   # (first row, rows, seq_len of the plain call)
    stat = lambda n, v=float("nan"): torch.full((n,), v, dtype=torch.float32, device=dev)
    a, b = qkv.clone(), qkv.clone()
    rq, rk, rq1, rk1 = stat(N * H), stat(N * KV), stat(N * H), stat(N * KV)
    assert hip.kf_qknorm_rope_train_pos(ctx.h, a.data_ptr(), a[:, Cq:].data_ptr(), wq.data_ptr(), wk.data_ptr(), table.data_ptr(), N, d_pos.data_ptr(), W, W, H, KV, hd, EPS, rq.data_ptr(),
                                        rk.data_ptr()) == 0, hip.kf_last_error()
    for r, n, sl in runs:
        assert hip.kf_qknorm_rope_train(ctx.h, b[r:].data_ptr(), b[r:, Cq:].data_ptr(), wq.data_ptr(), wk.data_ptr(), table.data_ptr(), n, sl, W, W, H, KV, hd, EPS, rq1[r * H:].data_ptr(),
                                        rk1[r * KV:].data_ptr()) == 0, hip.kf_last_error()
    ctx.sync()
    assert np.array_equal(u16(a), u16(b)) and not np.array_equal(u16(a), u16(qkv))
    assert torch.equal(rq, rq1) and torch.equal(rk, rk1) and bool(torch.isfinite(rq).all())

    # the backward, on gradients that are zero in the gap rows (what kf_attn_backward_docs leaves there)
    d = rng.normal(0, 0.05, (N, W)).astype(np.float32)
    for r, n in _gaps():
        d[r:r + n] = 0
    d = bf16_t(O.f32_to_bf16(d), dev)
    qraw, kraw = qkv[:, :Cq].contiguous(), qkv[:, Cq:Cq + Ck].contiguous()
    sc = torch.full((hip.kf_qknorm_rope_backward_scratch_bytes(N, H, KV, hd) // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
    dq, dk, dv = _nan(ctx, N, Cq), _nan(ctx, N, Ck), _nan(ctx, N, Ck)
    dwq, dwk = (torch.zeros(hd, dtype=torch.bfloat16, device=dev) for _ in range(2))
    assert hip.kf_qknorm_rope_backward_pos(ctx.h, d.data_ptr(), d[:, Cq:].data_ptr(), d[:, Cq + Ck:].data_ptr(), W, qraw.data_ptr(), Cq, kraw.data_ptr(), Ck, wq.data_ptr(), wk.data_ptr(),
                                           rq.data_ptr(), rk.data_ptr(), table.data_ptr(), N, d_pos.data_ptr(), H, KV, hd, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dwq.data_ptr(),
                                           dwk.data_ptr(), sc.data_ptr()) == 0, hip.kf_last_error()
    dq1, dk1, dv1 = _nan(ctx, N, Cq), _nan(ctx, N, Ck), _nan(ctx, N, Ck)
    f64 = lambda t_: O.bf16_to_f32(u16(t_)).astype(np.float64)
    sum_q, sum_k = np.zeros(hd), np.zeros(hd)
    for r, n, sl in runs:
        gq, gk = (torch.zeros(hd, dtype=torch.bfloat16, device=dev) for _ in range(2))
        assert hip.kf_qknorm_rope_backward(ctx.h, d[r:].data_ptr(), d[r:, Cq:].data_ptr(), d[r:, Cq + Ck:].data_ptr(), W, qraw[r:].data_ptr(), Cq, kraw[r:].data_ptr(), Ck, wq.data_ptr(),
                                           wk.data_ptr(), rq[r * H:].data_ptr(), rk[r * KV:].data_ptr(), table.data_ptr(), n, sl, H, KV, hd, dq1[r:].data_ptr(), dk1[r:].data_ptr(),
                                           dv1[r:].data_ptr(), gq.data_ptr(), gk.data_ptr(), sc.data_ptr()) == 0, hip.kf_last_error()
        ctx.sync()
        sum_q, sum_k = sum_q + f64(gq), sum_k + f64(gk)
    ctx.sync()
    assert np.array_equal(u16(dq), u16(dq1)) and np.array_equal(u16(dk), u16(dk1)) and np.array_equal(u16(dv), u16(dv1))
    assert np.array_equal(u16(dv), u16(d[:, Cq + Ck:]))
    for name, got, ref in (("dwq", f64(dwq), sum_q), ("dwk", f64(dwk), sum_k)):
        scale = np.abs(ref).max()
        mx, rms = np.abs(got - ref).max() / scale, np.sqrt(((got - ref) ** 2).mean()) / scale
        print("%s hd %d heads %d/%d: max %.3e rms %.3e of scale" % (name, hd, H, KV, mx, rms))
        assert scale > 0 and mx <= 2.0 ** -5 and rms <= 2.0 ** -6, "%s: max %.4f rms %.5f of scale" % (name, mx, rms)
    assert hip.kf_qknorm_rope_backward_pos(ctx.h, d.data_ptr(), d[:, Cq:].data_ptr(), d[:, Cq + Ck:].data_ptr(), W, qraw.data_ptr(), Cq, kraw.data_ptr(), Ck, wq.data_ptr(), wk.data_ptr(),
                                           rq.data_ptr(), rk.data_ptr(), table.data_ptr(), N, None, H, KV, hd, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dwq.data_ptr(), dwk.data_ptr(),
                                           sc.data_ptr()) == -20
    assert hip.kf_qknorm_rope_train_pos(ctx.h, a.data_ptr(), a[:, Cq:].data_ptr(), wq.data_ptr(), wk.data_ptr(), table.data_ptr(), N, None, W, W, H, KV, hd, EPS, None, None) == -20


def test_refusals_launch_nothing(ctx):
    hip, dev = ctx.hip, ctx.device
    hd, H, KV = 64, 4, 2
    qkv, Cq, Ck, rng = _qkv(ctx, N, H, KV, hd, 1)
    W = Cq + 2 * Ck
    tab, d_tab = _table(ctx, ROWS, LENS, N, T, H, KV, hd)
    other, _ = _table(ctx, ROWS, LENS, N, T, 8, 2, hd)   # planned for 8 / 2 heads
    big = torch.zeros(d_tab.numel() + 16, dtype=torch.uint8, device=dev)
    out, dqkv = _nan(ctx, N, Cq), _nan(ctx, N, W)
    dO = torch.zeros(N, Cq, dtype=torch.bfloat16, device=dev)
    sc = torch.zeros(hip.kf_attn_backward_docs_scratch_bytes(N, H) // 4, dtype=torch.float32, device=dev)
    hp = lambda t_: t_.ctypes.data_as(C.c_void_p)

    def fwd(q=qkv.data_ptr(), k=qkv[:, Cq:].data_ptr(), h=hp(tab), t=d_tab.data_ptr(), out_stride=Cq):
        return hip.kf_attn_prefill_docs(ctx.h, q, k, qkv[:, Cq + Ck:].data_ptr(), out.data_ptr(), h, t, W, out_stride, H, KV, hd, W)

    def bwd(q=qkv.data_ptr(), h=hp(tab), t=d_tab.data_ptr(), dq=dqkv.data_ptr(), s=sc.data_ptr()):
        return hip.kf_attn_backward_docs(ctx.h, q, qkv[:, Cq:].data_ptr(), qkv[:, Cq + Ck:].data_ptr(), W, out.data_ptr(), dO.data_ptr(), Cq, dq, dqkv[:, Cq:].data_ptr(),
                                         dqkv[:, Cq + Ck:].data_ptr(), W, h, t, H, KV, hd, s)
    for f in (fwd, bwd):
        assert f(t=None) == -20 and f(h=None) == -20, "a NULL table"
        assert f(h=hp(other)) == -20, "a table planned for another geometry"
        assert f(t=big.data_ptr() + 8) == -2000, "a misaligned table"          # KF_BLAS_UNALIGN
        assert f(q=qkv.data_ptr() + 2) == -2000, "misaligned rows"
    assert fwd(k=qkv[:, Cq:].data_ptr() + 2) == -2000 and fwd(out_stride=Cq - 8) == -20
    assert bwd(dq=dqkv.data_ptr() + 2) == -2000 and bwd(s=None) == -20
    ctx.sync()
    assert (u16(out) == 0xFFFF).all() and (u16(dqkv) == 0xFFFF).all(), "a refusal wrote something"
    assert fwd() == 0 and bwd() == 0, hip.kf_last_error()
    ctx.sync()
