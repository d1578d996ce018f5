"""kf_linear_w4a8 -- 4-bit group weights times int8 activations on v_dot4c_i32_i8.  The definition (include/kf_abi.h "int8 activations for 4-bit layers") fixes every
rounding: per group one fp32 multiply, one exact multiply, one subtract, one add into ONE ascending chain.  So every comparison here is an equality of bits with the numpy
restatement (tests/w4a8_restate.py)."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from w4a8_cases import FILL, SHAPES, IntW4, case, large_sum_case, linear_w4a8, run, saturating, t_bf16, u16, upload
from w4a8_restate import group_sums, to_bf

pytestmark = pytest.mark.gpu
NTOKS = (1, 3, 4, 5)   # the token tile is 4: one row (its own instantiation), below, at and above a tile


@pytest.mark.parametrize("qBias", [0, 8])
@pytest.mark.parametrize("M,K", SHAPES)
def test_product_bit_for_bit(ctx, M, K, qBias):
    dw, iw, q, s, ref = case(ctx, M, K, qBias)
    for n in NTOKS:
        got = run(ctx, "linear_w4a8", dw, q[:n], s[:n])
        assert not (got == FILL).any(), "nTok = %d: an output element kept the fill value" % n
        assert np.array_equal(got, ref[:n]), "nTok = %d: %d of %d outputs differ from the restatement" % (n, int((got != ref[:n]).sum()), got.size)


def test_single_row_vector_form(ctx):
    """q [K] and y [M] without a token dimension: the call decode makes"""
    dw, iw, q, s, ref = case(ctx, 72, 1024, 0)
    y = ctx.linear_w4a8(dw, torch.from_numpy(q[0].copy()).to(ctx.device), torch.from_numpy(s[:1].copy()).to(ctx.device))
    ctx.sync()
    assert np.array_equal(u16(y), ref[0])


@pytest.mark.parametrize("qBias", [0, 8])
def test_product_saturating(ctx, qBias):
    ow, q, step, top = saturating(qBias)
    iw = IntW4(ow)
    I, S = group_sums(iw, q)
    assert (np.abs(I) == top).all() and (np.abs(S) == 16256).all()
    got = run(ctx, "linear_w4a8", upload(ctx, ow), q, step)
    assert not (got == FILL).any() and np.array_equal(got, linear_w4a8(iw, q, step))


@pytest.mark.parametrize("qBias", [0, 8])
def test_product_where_the_multiply_rounds(ctx, qBias):
    """sums of 17 and 18 significant bits (tests/test_w4a8_cpu.py test_restatement_where_the_multiply_rounds: an fma in place of the multiply and the subtract gives other
    bits on this draw)"""
    ow, q, step = large_sum_case(24, 384, 5, 11, qBias)
    iw = IntW4(ow)
    assert np.abs(group_sums(iw, q)[0]).max() >= 1 << 16
    assert np.array_equal(run(ctx, "linear_w4a8", upload(ctx, ow), q, step), linear_w4a8(iw, q, step))


@pytest.mark.parametrize("M,K", [(130, 384), (64, 1280)])
@pytest.mark.parametrize("n", [1, 5])
def test_epilogue(ctx, M, K, n):
    dw, iw, q, s, _ = case(ctx, M, K, 8)
    rng = np.random.default_rng(M + n)
    bias = to_bf(rng.normal(0, 0.5, M).astype(np.float32))
    res = to_bf(rng.normal(0, 1, (n, M)).astype(np.float32))
    q, s = q[:n], s[:n]
    assert np.array_equal(run(ctx, "linear_w4a8", dw, q, s, bias=bias), linear_w4a8(iw, q, s, bias=bias))
    want = linear_w4a8(iw, q, s, residual=res)
    assert np.array_equal(run(ctx, "linear_w4a8", dw, q, s, residual=res), want)
    assert np.array_equal(run(ctx, "linear_w4a8", dw, q, s, residual=res, alias=True), want), "residual aliasing y"
    assert np.array_equal(run(ctx, "linear_w4a8", dw, q, s, bias=bias, residual=res, alias=True), linear_w4a8(iw, q, s, bias=bias, residual=res))


def test_quantiser_feeds_it(ctx):
    """kf_act_quant_i8 -> kf_linear_w4a8 on the device against quant_rows -> linear_w4a8 in numpy: the pair the model runs"""
    from w4a8_restate import quant_rows
    dw, iw, _, _, _ = case(ctx, 72, 1024, 0)
    x = to_bf(np.random.default_rng(4).normal(0, 1.5, (5, 1024)).astype(np.float32))
    dq, ds = ctx.act_quant_i8(t_bf16(x, ctx.device))
    y = ctx.linear_w4a8(dw, dq, ds)
    ctx.sync()
    q, s = quant_rows(x)
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(ds.cpu().numpy(), s)
    assert np.array_equal(u16(y), linear_w4a8(iw, q, s))


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1, L.BF16])
def test_refusals(ctx, type_):
    M, K = 16, 256
    w = to_bf(np.random.default_rng(3).normal(0, 0.05, (M, K)).astype(np.float32))
    dw = ctx.upload_blob(type_, M, K, O.quantize(w, M, K, type_).blob())
    q = torch.zeros((5, K), dtype=torch.int8, device=ctx.device)
    step = torch.ones(5, dtype=torch.float32, device=ctx.device)
    for entry in ("linear_w4a8", "linear_w4a8_tiles"):
        with pytest.raises(L.KFError) as e:
            getattr(ctx, entry)(dw, q, step)
        assert "code -1000" in str(e.value) and ("type %d" % type_) in str(e.value)
