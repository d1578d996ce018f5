"""The e4m3 block-scaled storage on the GPU (include/kf_abi.h "FP8 block-scaled layers"; koifish_amd/csrc/kf_f8b.hip) against plain float64 numpy: the mat-vec
(nTok < 8) and the MFMA tiles (nTok >= 8) of kf_linear bit for bit where every partial sum is exact, inside the derived fp32 summation bar on general inputs; the fused
decode entries against norm + kf_linear bit for bit; the quantiser and kf_dequant against the rule restated here."""
import ctypes as C

import numpy as np
import pytest
import torch

import f8a8_restate as R
from conftest import bf16_t, u16
from koifish_amd import lib as L
from koifish_amd.runtime import F8BlockDevWeight

pytestmark = pytest.mark.gpu
SHAPES = [(M, K) for M in (16, 144, 256) for K in (128, 384, 1024)]
NTOK = (1, 7, 8, 17, 64)
INT_CODE = np.array([int(np.flatnonzero(R.E4M3 == v)[0]) for v in range(-8, 9)], dtype=np.uint8)   # integer v -> its e4m3 code, at index v + 8


def weight(ctx, codes, scales):
    blob = np.concatenate([codes.reshape(-1), np.ascontiguousarray(scales, dtype=np.float32).reshape(-1).view(np.uint8)])
    return F8BlockDevWeight(codes.shape[0], codes.shape[1], torch.from_numpy(blob).to(ctx.device))


def dense(codes, scales):
    """float64 [M, K]: scale[r // 128][k // 128] * e4m3(byte)"""
    M, K = codes.shape
    return R.E4M3[codes] * np.repeat(np.repeat(scales.astype(np.float64), 128, axis=0)[:M], 128, axis=1)


@pytest.fixture(scope="module")
def exact():
    """per shape: integer codes in [-8, 8], power-of-two scales in [2^-2, 2^2] that differ per block, integer x for 64 tokens, and the float64 product"""
    out = {}
    for M, K in SHAPES:
        rng = np.random.default_rng(M * 7 + K)
        codes = INT_CODE[rng.integers(-8, 9, (M, K)) + 8]
        scales = np.exp2((np.arange(-(-M // 128) * (K // 128)) % 5 - 2).reshape(-1, K // 128)).astype(np.float32)
        x = rng.integers(-8, 9, (64, K)).astype(np.float64)
        W = dense(codes, scales)
        assert (np.abs(x) @ np.abs(W).T).max() * 4 < 2.0 ** 24   # every partial sum, in any order, is an integer below 2^24 times 2^-2: exact in fp32
        out[M, K] = codes, scales, x, x @ W.T
    return out


@pytest.mark.parametrize("n", NTOK)
@pytest.mark.parametrize("M,K", SHAPES)
def test_linear_exact(ctx, exact, M, K, n):
    """a wrong scale index, block boundary or tile bound shows as a wrong integer: y == bf16_rne(ref64) bit for bit, whatever the summation order"""
    codes, scales, x, ref = exact[M, K]
    y = u16(ctx.linear(weight(ctx, codes, scales), bf16_t(R.to_bf(x[:n].astype(np.float32)), ctx.device)))
    assert np.array_equal(y, R.to_bf(ref[:n].astype(np.float32)))


@pytest.fixture(scope="module")
def general(ctx):
    """per shape: Gaussian weights quantised by Context.quantize, the scales then multiplied by a per-block factor in [0.5, 2) (any finite fp32 scale is served),
    Gaussian x, the float64 product and the magnitude sum of its terms"""
    out = {}
    for M, K in SHAPES:
        rng = np.random.default_rng(M * 11 + K)
        w = ctx.quantize(bf16_t(R.to_bf(rng.normal(0, 0.05, (M, K)).astype(np.float32)), ctx.device), L.F8E4M3)
        codes = w.codes().cpu().numpy()
        scales = (w.scales().cpu().numpy() * rng.uniform(0.5, 2.0, (-(-M // 128), K // 128))).astype(np.float32)
        xu = R.to_bf(rng.normal(0, 1, (64, K)).astype(np.float32))
        W, x = dense(codes, scales), R.bf(xu).astype(np.float64)
        out[M, K] = codes, scales, xu, x @ W.T, np.abs(x) @ np.abs(W).T
    return out


@pytest.mark.parametrize("n", NTOK)
@pytest.mark.parametrize("M,K", SHAPES)
def test_linear_general(ctx, general, M, K, n):
    """|y - ref64| <= ulp_bf16(ref64) + (K + 2 K / 128) 2^-24 sum |s w x|: K adds and K / 128 scale multiplies and adds in fp32 in any order, then one bf16 rounding"""
    codes, scales, xu, ref, mag = general[M, K]
    y = R.bf(u16(ctx.linear(weight(ctx, codes, scales), bf16_t(xu[:n], ctx.device)))).astype(np.float64)
    ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(ref[:n]), 2.0 ** -126))) - 7)
    err, bar = np.abs(y - ref[:n]), ulp + (K + 2 * (K // 128)) * 2.0 ** -24 * mag[:n]
    print("max err / bar = %.3f" % (err / bar).max())
    assert (err <= bar).all()


@pytest.mark.parametrize("n", [1, 17])
def test_residual_may_alias_y(ctx, exact, n):
    codes, scales, x, ref = exact[144, 384]
    rng = np.random.default_rng(n)
    res = rng.integers(-64, 65, (n, 144)).astype(np.float32)
    y = bf16_t(R.to_bf(res), ctx.device)
    ctx.linear(weight(ctx, codes, scales), bf16_t(R.to_bf(x[:n].astype(np.float32)), ctx.device), residual=y, y=y)
    want = R.to_bf((res + R.bf(R.to_bf(ref[:n].astype(np.float32)))).astype(np.float32))   # bf16(residual + bf16(W.x))
    assert np.array_equal(u16(y), want)


def test_fused_entries_equal_norm_then_linear(ctx, general):
    """kf_norm_linear and kf_norm_gateup_swiglu sum as kf_linear does: bit for bit against kf_rmsnorm + kf_linear (+ kf_swiglu, the same rule on the bf16 projections)"""
    ws = [weight(ctx, *general[M, 1024][:2]) for M in (256, 144, 16)]
    rng = np.random.default_rng(5)
    x = bf16_t(R.to_bf(rng.normal(0, 2, 1024).astype(np.float32)), ctx.device)
    nw = bf16_t(R.to_bf(rng.uniform(0.5, 1.5, 1024).astype(np.float32)), ctx.device)
    xn = ctx.rmsnorm(x, nw)
    want = [ctx.linear(w, xn) for w in ws]
    for got, w in zip(ctx.norm_linear(x, nw, ws), want):
        assert torch.equal(got, w)
    up = weight(ctx, general[256, 1024][0][::-1].copy(), general[256, 1024][1][::-1].copy())
    assert torch.equal(ctx.norm_gateup_swiglu(x, nw, ws[0], up), ctx.swiglu(want[0], ctx.linear(up, xn)))


@pytest.mark.parametrize("dev_pos", [False, True])
def test_norm_linear_lands_in_the_row_of_its_position(ctx, general, dev_pos):
    """y_pos_stride: projection i goes to y[i] + pos * stride[i] (K / V into their cache row); pos by value, or read from *d_pos with `pos` only a bound"""
    ws = [weight(ctx, *general[M, 1024][:2]) for M in (256, 144)]
    rng = np.random.default_rng(6)
    x = bf16_t(R.to_bf(rng.normal(0, 2, 1024).astype(np.float32)), ctx.device)
    nw = bf16_t(R.to_bf(rng.uniform(0.5, 1.5, 1024).astype(np.float32)), ctx.device)
    want = ctx.norm_linear(x, nw, ws)
    pos, ys = 3, [torch.zeros(256, dtype=torch.bfloat16, device=ctx.device), torch.zeros(5, 160, dtype=torch.bfloat16, device=ctx.device)]
    descs = [w.desc() for w in ws]
    wp, yp = (C.c_void_p * 2)(*[C.addressof(d) for d in descs]), (C.c_void_p * 2)(*[y.data_ptr() for y in ys])
    d_pos = torch.tensor([pos], dtype=torch.int32, device=ctx.device)
    L.check(ctx.hip.kf_norm_linear(ctx.h, C.c_void_p(x.data_ptr()), C.c_void_p(nw.data_ptr()), 1e-6, 2, wp, yp, (C.c_int64 * 2)(0, 160), 4 if dev_pos else pos,
                                   C.c_void_p(d_pos.data_ptr()) if dev_pos else None), "kf_norm_linear")
    assert torch.equal(ys[0], want[0]) and torch.equal(ys[1][pos, :144], want[1])
    ys[1][pos, :144] = 0
    assert not ys[1].any()   # nothing else was written


def test_entries_that_do_not_serve_the_storage_refuse_it(ctx, exact):
    d = weight(ctx, *exact[16, 128][:2]).desc()
    x = torch.zeros(128, dtype=torch.bfloat16, device=ctx.device)
    y = torch.zeros(16, dtype=torch.float32, device=ctx.device)
    assert ctx.hip.kf_linear_f32(ctx.h, C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())) == -1000   # KF_UNSUPPORTED_DATATYPE
    assert "e4m3 block-scaled" in ctx.hip.kf_last_error().decode()


def quant_restated(v):
    """codes and scales of bf16 values v [M, K] (float32): per 128 x 128 block e = the smallest integer with amax 2^-e <= 448, scale = 2^e, code = e4m3_rne(v 2^-e);
    an all-zero block: scale 0, codes 0"""
    M, K = v.shape
    codes, scales = np.zeros((M, K), dtype=np.uint8), np.zeros((-(-M // 128), K // 128), dtype=np.float32)
    for rb in range(scales.shape[0]):
        for kb in range(scales.shape[1]):
            blk = v[128 * rb:128 * rb + 128, 128 * kb:128 * kb + 128]
            q, step = R.quant_rows_f32(blk.reshape(1, -1))   # the same power-of-two rule, over the block
            codes[128 * rb:128 * rb + 128, 128 * kb:128 * kb + 128], scales[rb, kb] = q.reshape(blk.shape), step[0]
    return codes, scales


def test_quantiser_and_dequant(ctx):
    """144 x 384: a partial scale row; block (0, 1) all zero; block (0, 2) with amax exactly 448 * 2^-3; block (1, 0) with amax just above 448 * 2^-3"""
    rng = np.random.default_rng(9)
    v = R.bf(R.to_bf(rng.normal(0, 0.3, (144, 384)).astype(np.float32)))
    v[:128, 128:256] = 0.0
    v[:128, 256:] = np.clip(v[:128, 256:], -50, 50)
    v[5, 300] = -56.0
    v[128:, :128] = np.clip(v[128:, :128], -50, 50)
    v[130, 7] = 56.25
    w = ctx.quantize(bf16_t(R.to_bf(v), ctx.device), L.F8E4M3)
    codes, scales = quant_restated(v)
    assert scales[0, 1] == 0 and scales[0, 2] == 0.125 and scales[1, 0] == 0.25
    assert np.array_equal(w.scales().cpu().numpy(), scales) and np.array_equal(w.codes().cpu().numpy(), codes)
    scales2 = (scales * rng.uniform(0.5, 2.0, scales.shape)).astype(np.float32)   # kf_dequant: bf16(scale * value), one rounding, any scale
    want = R.to_bf((np.repeat(np.repeat(scales2, 128, axis=0)[:144], 128, axis=1) * R.E4M3[codes].astype(np.float32)).astype(np.float32))
    assert np.array_equal(u16(ctx.dequant(weight(ctx, codes, scales2))), want)
