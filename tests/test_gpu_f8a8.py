"""kf_act_quant_f8 and kf_linear_f8a8 (include/kf_abi.h "fp8 activations for f8e5m2 layers") against the restatement (tests/f8a8_restate.py): the quantiser bit for bit;
the product bit for bit wherever the sum is exact whatever the instruction's adder does (one-hot rows, small integers), invariant under the batch, and inside the derived
bar of any-order fp32 summation on general inputs."""
import numpy as np
import pytest
import torch

import f8a8_restate as R
from conftest import bf16_t, u16
from koifish_amd import lib as L
from koifish_amd.runtime import DevWeight
from test_f8a8_cpu import f8, plan

pytestmark = pytest.mark.gpu
FINITE_W = np.array([b for b in range(256) if (b & 0x7c) != 0x7c], dtype=np.uint8)       # every finite e5m2 byte, subnormals and both zeros included
CODES = np.array([c for c in range(256) if c & 0x7f not in (0, 0x7f)], dtype=np.uint8)   # every finite non-zero e4m3 code
INT_CODE = {v: int(np.flatnonzero(R.E4M3 == v)[0]) for v in (-2, -1, 1, 2)}
INT_BYTE = {v: int(np.flatnonzero(R.E5M2 == v)[0]) for v in (-2, -1, 1, 2)}


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def weight(ctx, wb):
    return DevWeight(L.F8E5M2, wb.shape[0], wb.shape[1], dev(ctx, wb.reshape(-1)))


def run(ctx, w, q, step, **kw):
    return u16(ctx.linear_f8a8(w, dev(ctx, q), dev(ctx, np.asarray(step, dtype=np.float32)), **kw))


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("dim", [128, 1600])
def test_quantiser_bit_for_bit(ctx, dim, fold):
    """rows whose targets are every e4m3 value and every midpoint between neighbours (ties), under row scales from 2^-9 up; Gaussian rows; a zero row; ldx > dim"""
    rng = np.random.default_rng(dim)
    pos = R.E4M3[:0x7f]
    vals = np.concatenate([pos, -pos, (pos[:-1] + pos[1:]) / 2, -(pos[:-1] + pos[1:]) / 2])
    rows = 3 * -(-vals.size // (dim - 1)) + 6
    x = rng.normal(0, 1, (rows, dim)) * np.exp2(rng.integers(-9, 9, (rows, 1)))
    n_t = rows - 6
    x[:n_t, 1:] = np.resize(vals, (n_t, dim - 1))
    x[:n_t, 0] = 448.0
    x[:n_t] *= np.exp2(np.arange(n_t) % 18 - 9)[:, None]
    x[n_t] = 0.0
    xu = R.to_bf(x.astype(np.float32))
    assert fold or np.array_equal(R.bf(xu[:n_t]), x[:n_t].astype(np.float32))   # the targets are bf16 values
    norm_w = R.to_bf(rng.uniform(0.5, 1.5, dim).astype(np.float32)) if fold else None
    xd = torch.zeros((rows, dim + 24), dtype=torch.bfloat16, device=ctx.device)
    xd[:, :dim] = bf16_t(xu, ctx.device)
    q, step = ctx.act_quant_f8(xd[:, :dim], None if norm_w is None else bf16_t(norm_w, ctx.device))
    wq, ws = R.quant_rows(xu, norm_w)
    assert np.array_equal(step.cpu().numpy(), ws)
    assert np.array_equal(q.cpu().numpy(), wq), "%d codes differ" % int((q.cpu().numpy() != wq).sum())
    assert fold or set(np.unique(wq[:n_t])) >= set(range(0x7f)) | set(range(0x80, 0xff))


@pytest.mark.parametrize("M,K,n,form", [(16, 128, 1, 0), (48, 192, 17, 0), (130, 1600, 33, 0), (256, 512, 129, 0), (4096, 128, 256, 1), (4096, 192, 512, 2), (4096, 192, 1024, 3)])
def test_one_hot_exact(ctx, M, K, n, form):
    """token t holds one non-zero code at k_t, k_t sweeps every position of K: y = bf16(step * a * w) exactly -- any wrong k slot, row map or swizzle shows"""
    assert plan(f8(M, K), n).form == form
    wb = FINITE_W[(17 * np.arange(M)[:, None] + np.arange(K)[None, :]) % FINITE_W.size]
    w = weight(ctx, wb)
    for j in range(-(-K // n)):
        t = np.arange(n)
        kt = (j * n + t) % K
        q = np.zeros((n, K), dtype=np.uint8)
        q[t, kt] = CODES[(7 * t + j) % CODES.size]
        step = np.exp2(t % 5 - 2).astype(np.float32)
        want = R.epilogue(0.0 + R.E4M3[q[t, kt]][:, None] * R.E5M2[wb[:, kt]].T, step)   # the accumulator starts from +0: a product of -0 leaves +0
        got = run(ctx, w, q, step)
        assert np.array_equal(got, want), "launch %d: %d of %d differ, first at (token, row) %s" % (j, (got != want).sum(), got.size, np.argwhere(got != want)[0])


@pytest.mark.parametrize("M,K,n", [(48, 192, 17), (130, 1600, 33)])
def test_small_integers_exact(ctx, M, K, n):
    """codes and weights in {-2 .. 2}: every partial sum is an integer below 2^24, exact in any order; dense +-1 blocks on the seams of the 128-byte steps and on the half step"""
    rng = np.random.default_rng(K)
    a, wv = rng.integers(-2, 3, (n, K)), rng.integers(-2, 3, (M, K))
    for s in list(range(128, K, 128)) + [K]:
        a[:, s - 12:min(s + 12, K)], wv[:, s - 12:min(s + 12, K)] = 1, 1 - 2 * (np.arange(M)[:, None] % 2)
    a[:, K - 64:], wv[::3, K - 64:] = -1, 1
    q = np.vectorize(lambda v: INT_CODE.get(v, 0))(a).astype(np.uint8)
    wb = np.vectorize(lambda v: INT_BYTE.get(v, 0))(wv).astype(np.uint8)
    acc = (a @ wv.T).astype(np.float32)
    assert (np.abs(a) @ np.abs(wv.T)).max() < 2 ** 24 and np.abs(acc).max() > 64
    step = np.exp2(np.arange(n) % 7 - 3).astype(np.float32)
    bias, res = R.to_bf(rng.normal(0, 8, M).astype(np.float32)), R.to_bf(rng.normal(0, 30, (n, M)).astype(np.float32))
    w = weight(ctx, wb)
    assert np.array_equal(run(ctx, w, q, step), R.epilogue(acc, step))
    want = R.epilogue(acc, step, bias, res)
    assert np.array_equal(run(ctx, w, q, step, bias=bf16_t(bias, ctx.device), residual=bf16_t(res, ctx.device)), want)
    y = bf16_t(res, ctx.device).clone()   # the residual aliasing y
    assert np.array_equal(run(ctx, w, q, step, bias=bf16_t(bias, ctx.device), residual=y, y=y), want)


@pytest.fixture(scope="module")
def gauss(ctx):
    """Gaussian x and W -> device weight, restated codes and steps, the fp64 product and sum of magnitudes, what the device gives: once per shape"""
    def make(M, K, n):
        rng = np.random.default_rng(M + K)
        wb = (rng.normal(0, 0.05, (M, K)).astype(np.float16).view(np.uint16) >> 8).astype(np.uint8)   # the high byte of the half
        q, step = R.quant_rows(R.to_bf(rng.normal(0, 1, (n, K)).astype(np.float32)))
        w = weight(ctx, wb)
        return w, wb, q, step, run(ctx, w, q, step)
    cache = {}
    return lambda *s: cache.setdefault(s, make(*s))


def test_invariance(ctx, gauss):
    """the bits of y[t] are a function of weight row and activation row alone: row t of a 129-token batch, alone, and at another place of a 33-token batch"""
    w, wb, q, step, y = gauss(256, 512, 129)
    for t in (0, 77, 128):
        assert np.array_equal(run(ctx, w, q[t:t + 1], step[t:t + 1])[0], y[t]), t
    assert np.array_equal(run(ctx, w, q[60:93], step[60:93]), y[60:93])


@pytest.mark.parametrize("M,K,n", [(256, 1024, 64), (96, 1600, 40)])
def test_general_inputs(ctx, gauss, M, K, n):
    """|y - step * acc64| <= one bf16 ulp of the reference + K * 2^-24 * step * sum_k |a_k w_k|: the output rounding, and the worst case of any-order fp32 summation of
    exact terms (each of the K - 1 additions errs by at most 2^-24 of a partial sum that is at most the sum of magnitudes).  Derived, not tuned."""
    w, wb, q, step, y = gauss(M, K, n)
    ref = step[:, None].astype(np.float64) * R.product(wb, q)
    mag = step[:, None].astype(np.float64) * (np.abs(R.E4M3[q]) @ np.abs(R.E5M2[wb]).T)
    ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)
    err, bar = np.abs(R.bf(y).astype(np.float64) - ref), ulp + K * 2.0 ** -24 * mag
    print("max err / bar %.3f; max err in ulps %.3f; max summation term / ulp %.4f" % ((err / bar).max(), (err / ulp).max(), (K * 2.0 ** -24 * mag / ulp).max()))
    assert (err <= bar).all(), "%d elements over the bar, worst ratio %g" % ((err > bar).sum(), (err / bar).max())


def test_refusals_launch_nothing(ctx):
    n, K, M = 4, 256, 16
    y = torch.full((n, M), 7.0, dtype=torch.bfloat16, device=ctx.device)
    q, step = torch.ones(n * K + 16, dtype=torch.uint8, device=ctx.device), torch.ones(n, dtype=torch.float32, device=ctx.device)
    ok = weight(ctx, np.full((M, K), 0x3c, dtype=np.uint8))
    bad = [(DevWeight(L.BF16, M, K, torch.zeros(2 * M * K, dtype=torch.uint8, device=ctx.device)), q[:n * K].view(n, K), "no fp8 form"),
           (weight(ctx, np.full((M, 64), 0x3c, dtype=np.uint8)), q[:n * 64].view(n, 64), "at least 128 bytes"), (ok, q[8:8 + n * K].view(n, K), "not 16-byte aligned")]
    for w, qq, why in bad:
        with pytest.raises(L.KFError, match=why):
            ctx.linear_f8a8(w, qq, step, y=y)
    ctx.sync()
    assert (y == 7.0).all()
    assert (ctx.linear_f8a8(ok, q[:n * K].view(n, K), step, y=y) == 0.5).all()   # ... and the served call writes: 256 x (code 0x01 = 2^-9) x (byte 0x3c = 1.0)
