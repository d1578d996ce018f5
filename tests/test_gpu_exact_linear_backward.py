"""kf_linear_backward on inputs whose arithmetic is exact in fp32 under every summation order (tests/exact_inputs.py): delta, gW and gBias equal bf16(exact) BIT FOR
BIT, every element, in every form kf_gemm_plan.h gemm_plan_backward sends the two products down -- the transposed copies on the direct and the 64 x 64 tiles, the
K-major 128 x 128 and 256 x 256 tiles plain, in S >= 2 k pieces, and in the owner / helper cut (tests/test_exact_inputs_cpu.py pins which case runs which form and
checks every precondition on the CPU).  Two input families per shape: random {-1, 0, 1} entries, and dense +-1 blocks of 128 contraction indices laid on the first and
last k tile and astride every seam between two workgroups' k pieces of the plan of that very shape.  One dropped, doubled or misplaced product changes an integer:
no tolerance anywhere.  The scratch arrives filled with a byte pattern, and every call runs twice (another pattern) to the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests import exact_inputs as E
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu


def _call(ctx, c, dw, accumulate, pattern, want_delta=True, want_gw=True, want_bias=True):
    """one kf_linear_backward on fresh copies of the prior values -> the bits of (delta, gW, gBias) afterwards"""
    OC, IC, n, dev = c["OC"], c["IC"], c["n"], ctx.device
    d_delta, d_gW, d_gb = bf16_t(c["delta0"], dev), bf16_t(c["gW0"], dev), bf16_t(c["gb0"], dev)
    d_dIn, d_inp = bf16_t(c["dIn"], dev), bf16_t(c["inp"], dev)
    nb = ctx.hip.kf_linear_backward_scratch_bytes(OC, IC, n)
    scratch = torch.full((nb + 256,), pattern, dtype=torch.uint8, device=dev)   # the header: contents need not be initialised, results do not depend on them
    sp = (scratch.data_ptr() + 255) & ~255
    desc = dw.desc()
    rc = ctx.hip.kf_linear_backward(ctx.h, C.byref(desc), d_dIn.data_ptr(), d_inp.data_ptr(), d_delta.data_ptr() if want_delta else None,
                                    d_gW.data_ptr() if want_gw else None, d_gb.data_ptr() if want_bias else None, n, int(accumulate), sp)
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    return u16(d_delta), u16(d_gW), u16(d_gb)


def _check(ctx, c, dw, want_delta=True, want_gw=True):
    for accumulate in (False, True):
        runs = [_call(ctx, c, dw, accumulate, pattern, want_delta, want_gw) for pattern in (0xA5, 0x3C)]
        for delta, gW, gb in runs:
            assert np.array_equal(delta, (c["delta_acc"] if accumulate else c["delta"]) if want_delta else c["delta0"])
            assert np.array_equal(gW, c["gW"] if want_gw else c["gW0"])
            assert np.array_equal(gb, c["gb"])
        assert all(np.array_equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("family", ["sparse", "block"])
@pytest.mark.parametrize("shape", list(E.LINEAR_CASES), ids=lambda s: "%dx%dx%d" % s)
def test_linear_backward_exact(ctx, shape, family):
    """bf16 storage: the integer entries are the weight.  Forms of (input gradient, weight gradient) per shape: E.LINEAR_CASES"""
    c = E.linear_case(ctx.hip, shape, family)
    OC, IC, _ = shape
    dw = ctx.upload_blob(L.BF16, OC, IC, O.quantize(c["W"], OC, IC, L.BF16).blob())
    _check(ctx, c, dw)


def test_linear_backward_exact_with_twos(ctx):
    """+-2 among the weight's entries: products that are not all of one magnitude"""
    shape = (1024, 256, 1024)
    c = E.linear_case(ctx.hip, shape, "sparse", twos=True)
    dw = ctx.upload_blob(L.BF16, shape[0], shape[1], O.quantize(c["W"], shape[0], shape[1], L.BF16).blob())
    _check(ctx, c, dw)


def test_linear_backward_exact_q4_grid(ctx):
    """4-bit storage holding a weight on its own grid (every group spans -7 .. 8 in steps of 1): the dequantised operand is the integer weight, the rest as above.
    The other storages' dequantise kernels are held bit for bit by their own tests; a grid like this one needs 16 levels."""
    OC, IC, _ = E.Q4_CASE
    w, ow = E.q4_grid_weight(OC, IC, seed=3)
    c = E.linear_case(ctx.hip, E.Q4_CASE, "sparse", w=w)
    _check(ctx, c, ctx.upload_blob(L.Q4, OC, IC, ow.blob()))


@pytest.mark.parametrize("want_delta,want_gw", [(True, False), (False, True)])
def test_linear_backward_exact_null_outputs(ctx, want_delta, want_gw):
    """gW = NULL (a fixed weight: input gradient only) and delta = NULL (the first layer: weight gradient only), once each; the tensor not asked for is not touched"""
    shape = (1024, 256, 1024)
    c = E.linear_case(ctx.hip, shape, "block")
    dw = ctx.upload_blob(L.BF16, shape[0], shape[1], O.quantize(c["W"], shape[0], shape[1], L.BF16).blob())
    _check(ctx, c, dw, want_delta, want_gw)
