"""kf_linear_w4a8_tiles -- the W4.A8 product of a token batch on int8 MFMA tiles.  The tile kernel keeps the definition's one ascending fp32 chain per output element
(include/kf_abi.h "int8 activations for 4-bit layers"), so every comparison here is an equality of bits: with the numpy restatement (tests/w4a8_restate.py) and with
kf_linear_w4a8 on the device."""
import numpy as np
import pytest
import torch

from a8_plan_mirror import weight_tile_plan as tile_plan
from koifish_amd import lib as L
from oracle import oracle as O
from w4a8_cases import FILL, SHAPES, IntW4, case, large_sum_case, linear_w4a8, run, saturating, t_bf16, u16, upload
from w4a8_restate import group_sums, quant_rows, to_bf

pytestmark = pytest.mark.gpu
NTOKS = (1, 15, 16, 17, 33, 70)   # below, at and above one MFMA token tile; three and five workgroups along the tokens, the last a tail.  SHAPES are too narrow to fill
                                  # 256 workgroups, so all of these run the 16-token form (mfma_tok = 1); the 32- and 64-token forms: test_wide_token_tiles


@pytest.mark.parametrize("qBias", [0, 8])
@pytest.mark.parametrize("M,K", SHAPES)
def test_product_bit_for_bit(ctx, M, K, qBias):
    dw, iw, q, s, ref = case(ctx, M, K, qBias)
    for n in NTOKS:
        got = run(ctx, "linear_w4a8_tiles", dw, q[:n], s[:n])
        assert not (got == FILL).any(), "nTok = %d: an output element kept the fill value" % n
        assert np.array_equal(got, ref[:n]), "nTok = %d: %d of %d outputs differ from the restatement" % (n, int((got != ref[:n]).sum()), got.size)
        assert np.array_equal(got, run(ctx, "linear_w4a8", dw, q[:n], s[:n])), "nTok = %d: differs from kf_linear_w4a8" % n


WIDE = (1000, 1280)   # 16 row tiles, the last 40 rows; 10 groups: a chunk of 8, where a thread of the 64-token form stages two (group, token) units, and one of 2


@pytest.mark.parametrize("qBias", [0, 8])
def test_wide_token_tiles(ctx, qBias):
    """the 32- and the 64-token form (w4a8_tiles_kernel<2>, <4>), which the plan picks once 256 workgroups remain: 500 tokens = 16 tiles of 32 with a tail of 20, 1030
    tokens = 17 tiles of 64 with a tail of 6 -- against the restatement and against kf_linear_w4a8; the plan's choice is asserted so the coverage cannot lapse"""
    M, K = WIDE
    rng = np.random.default_rng(31 + qBias)
    w = rng.normal(0, 0.05, (M, K)).astype(np.float32) + np.repeat(rng.choice([-1.0, 1.0], (M, K // 128)) * rng.uniform(0.03, 0.08, (M, K // 128)), 128, axis=1).astype(np.float32)
    ow = O.quantize(to_bf(w), M, K, L.Q4)
    assert (ow.zero & 0x7fff).all()
    if qBias:
        ow = O.QWeight(L.Q4, M, K, ow.data, ow.zero, ow.step, 128, qBias)
    iw, dw = IntW4(ow), upload(ctx, ow)
    q, s = quant_rows(to_bf(rng.normal(0, 1, (1030, K)).astype(np.float32)))
    ref = linear_w4a8(iw, q, s)
    for n, mfma_tok in ((500, 2), (1030, 4)):
        p = tile_plan(dw, n)
        assert (p.mfma_tok, p.tok_tile, p.chunk, p.grid_x) == (mfma_tok, 16 * mfma_tok, 8, 16) and p.grid_y == -(-n // p.tok_tile)
        got = run(ctx, "linear_w4a8_tiles", dw, q[:n], s[:n])
        assert not (got == FILL).any(), "nTok = %d: an output element kept the fill value" % n
        assert np.array_equal(got, ref[:n]), "nTok = %d: %d of %d outputs differ from the restatement" % (n, int((got != ref[:n]).sum()), got.size)
        assert np.array_equal(got, run(ctx, "linear_w4a8", dw, q[:n], s[:n])), "nTok = %d: differs from kf_linear_w4a8" % n
    # the 64-token form on the other staging path and with the epilogue: activation rows that are not 16-byte aligned; bias, residual aliasing y
    n = 1030
    raw = torch.zeros(n * K + 16, dtype=torch.int8, device=ctx.device)
    dq = raw[1:1 + n * K].view(n, K)
    dq.copy_(torch.from_numpy(np.ascontiguousarray(q)))
    assert dq.data_ptr() % 16 == 1
    y = t_bf16(np.full((n, M), FILL, dtype=np.uint16), ctx.device)
    ctx.linear_w4a8_tiles(dw, dq, torch.from_numpy(np.ascontiguousarray(s)).to(ctx.device), y=y)
    ctx.sync()
    assert np.array_equal(u16(y), ref)
    bias = to_bf(rng.normal(0, 0.5, M).astype(np.float32))
    res = to_bf(rng.normal(0, 1, (n, M)).astype(np.float32))
    assert np.array_equal(run(ctx, "linear_w4a8_tiles", dw, q, s, bias=bias, residual=res, alias=True), linear_w4a8(iw, q, s, bias=bias, residual=res))


@pytest.mark.parametrize("qBias", [0, 8])
def test_product_saturating(ctx, qBias):
    ow, q, step, top = saturating(qBias)
    iw = IntW4(ow)
    assert (np.abs(group_sums(iw, q)[0]) == top).all()
    dw = upload(ctx, ow)
    got = run(ctx, "linear_w4a8_tiles", dw, q, step)
    assert not (got == FILL).any() and np.array_equal(got, linear_w4a8(iw, q, step))
    assert np.array_equal(got, run(ctx, "linear_w4a8", dw, q, step))


@pytest.mark.parametrize("qBias", [0, 8])
def test_product_where_the_multiply_rounds(ctx, qBias):
    """sums of 17 and 18 significant bits: an fma in place of the multiply and the subtract gives other bits on this draw (tests/test_w4a8_cpu.py)"""
    ow, q, step = large_sum_case(24, 384, 17, 11, qBias)
    iw = IntW4(ow)
    assert np.array_equal(run(ctx, "linear_w4a8_tiles", upload(ctx, ow), q, step), linear_w4a8(iw, q, step))


@pytest.mark.parametrize("M,K", [(130, 384), (64, 1280)])
@pytest.mark.parametrize("n", [1, 17, 70])
def test_epilogue(ctx, M, K, n):
    dw, iw, q, s, _ = case(ctx, M, K, 0)
    rng = np.random.default_rng(M + n)
    bias = to_bf(rng.normal(0, 0.5, M).astype(np.float32))
    res = to_bf(rng.normal(0, 1, (n, M)).astype(np.float32))
    q, s = q[:n], s[:n]
    assert np.array_equal(run(ctx, "linear_w4a8_tiles", dw, q, s, bias=bias), linear_w4a8(iw, q, s, bias=bias))
    want = linear_w4a8(iw, q, s, residual=res)
    assert np.array_equal(run(ctx, "linear_w4a8_tiles", dw, q, s, residual=res), want)
    assert np.array_equal(run(ctx, "linear_w4a8_tiles", dw, q, s, residual=res, alias=True), want), "residual aliasing y"
    want = linear_w4a8(iw, q, s, bias=bias, residual=res)
    assert np.array_equal(run(ctx, "linear_w4a8_tiles", dw, q, s, bias=bias, residual=res, alias=True), want)


@pytest.mark.parametrize("qBias", [0, 8])
def test_unaligned_activations(ctx, qBias):
    """q one byte into a buffer: the kernel's 16-byte staging loads are not allowed there; the contract (any q the mat-vec takes) and the bits stay"""
    M, K, n = 130, 384, 17
    dw, iw, q, s, ref = case(ctx, M, K, qBias)
    raw = torch.zeros(n * K + 16, dtype=torch.int8, device=ctx.device)
    dq = raw[1:1 + n * K].view(n, K)
    dq.copy_(torch.from_numpy(np.ascontiguousarray(q[:n])))
    assert dq.data_ptr() % 16 == 1
    y = t_bf16(np.full((n, M), FILL, dtype=np.uint16), ctx.device)
    ctx.linear_w4a8_tiles(dw, dq, torch.from_numpy(np.ascontiguousarray(s[:n])).to(ctx.device), y=y)
    ctx.sync()
    assert np.array_equal(u16(y), ref[:n])
