"""The row siblings of the fused mat-vec entries (kf_linear_rows, kf_norm_linear_rows, kf_norm_gateup_swiglu_rows, kf_norm_lm_head_rows): R = 1 .. 8 activation
rows against one pass over the weights.  Everything is compared bit for bit (== on the uint16 / int32 arrays) with the one-token entry called row by row AND with
the oracle's canonical mat-vec: the row kernel shares the unpack, never the bits.  Shapes are the smallest that reach every path: fewer than 16 blocks per row (masked
tail), M no multiple of the rows per wave slot, the lanes bump with a masked last step (1024 x 3072), three jobs of unequal heights writing cache rows, the paired
form, the residual in place, the arg-max with a tie, both 4-bit biases, a storage that falls back, and a row long enough to cut R = 8 into two panels."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import bf16_t, u16
from koifish_amd import lib as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu
RS = [1, 2, 3, 5, 8]
RMAX = 8


@pytest.fixture(autouse=True)
def canonical_ctx(ctx):
    """the session's context in the canonical order for every test here, whatever order an earlier test file left it in; put back afterwards"""
    was = ctx.hip.kf_get_canonical(ctx.h)
    ctx.set_canonical(True)
    yield
    ctx.set_canonical(bool(was))


@pytest.fixture()
def canon():
    O.set_order(O.ORDER_CANON)
    yield
    O.set_order(O.ORDER_DOT16)


def weights(rng, m, k, type_=None, symmetric=False, std=0.05):
    w = O.f32_to_bf16(rng.normal(0, std, size=(m, k)).astype(np.float32))
    return O.quantize(w, m, k, L.Q4 if type_ is None else type_, symmetric=symmetric)


def rows_x(ctx, rng, k, pad=8):
    """eight activation rows, on the host and as a strided device view (row stride k + pad elements)"""
    x = O.f32_to_bf16(rng.normal(0, 1.0, size=(RMAX, k)).astype(np.float32))
    buf = torch.zeros(RMAX, k + pad, dtype=torch.bfloat16, device=ctx.device)
    buf[:, :k] = bf16_t(x, ctx.device)
    return x, buf[:, :k]


_PLAIN = {}


def plain_case(ctx, m, k, symmetric):
    """weights, eight rows of x, and per row the one-token kf_linear result and the oracle's: computed once per shape, shared by every R"""
    key = (m, k, symmetric)
    if key not in _PLAIN:
        rng = np.random.default_rng(m * 31 + k + symmetric)
        ow = weights(rng, m, k, symmetric=symmetric)
        dw = ctx.upload_blob(L.Q4, m, k, ow.blob(), symmetric=symmetric)
        x, xd = rows_x(ctx, rng, k)
        one = np.stack([u16(ctx.linear(dw, xd[r])) for r in range(RMAX)])
        with O.canonical():
            ref = np.stack([O.linear(ow, x[r]) for r in range(RMAX)])
        _PLAIN[key] = (ow, dw, x, xd, one, ref)
    return _PLAIN[key]


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("m,k", [(64, 128), (70, 1024), (1024, 3072)])
def test_linear_rows(ctx, m, k, symmetric, R):
    ow, dw, x, xd, one, ref = plain_case(ctx, m, k, symmetric)
    assert ow.qBias == (8 if symmetric else 0)
    assert np.array_equal(one, ref)   # the premise: the one-token entry is the oracle's
    before = ctx.rows_route_counts()
    y = u16(ctx.linear_rows(dw, xd[:R]))
    assert np.array_equal(y, one[:R]), "%d of %d outputs differ from the one-token entry" % (int((y != one[:R]).sum()), y.size)
    assert np.array_equal(y, ref[:R])
    after = ctx.rows_route_counts()
    assert (after[0] - before[0], after[1] - before[1]) == ((R, 0) if R > 1 else (0, 1))


@pytest.mark.parametrize("R", [2, 8])
def test_residual_in_place(ctx, R):
    """the residual epilogue with residual == y: every element is read before it is stored"""
    ow, dw, x, xd, one, ref = plain_case(ctx, 70, 1024, False)
    rng = np.random.default_rng(R)
    res = O.f32_to_bf16(rng.normal(0, 1.0, size=(R, 70)).astype(np.float32))
    want = np.stack([O.add(res[r], ref[r]) for r in range(R)])
    one_tok = np.stack([u16(ctx.linear(dw, xd[r], residual=bf16_t(res[r], ctx.device))) for r in range(R)])
    assert np.array_equal(one_tok, want)
    y = bf16_t(res, ctx.device).clone()
    ctx.linear_rows(dw, xd[:R], residual=y, y=y)
    assert np.array_equal(u16(y), want)
    y2 = ctx.linear_rows(dw, xd[:R], residual=bf16_t(res, ctx.device))
    assert np.array_equal(u16(y2), want)


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("norm", [True, False])
def test_three_jobs_into_cache_rows(ctx, canon, norm, R):
    """q | k | v of unequal heights sharing the (normed) input: q to its own rows, k and v to cache rows pos0 + r"""
    rng = np.random.default_rng(77)
    k, ms, pos0, n_pos = 256, [256, 128, 128], 5, 16
    ows = [weights(rng, m, k) for m in ms]
    dws = [ctx.upload_blob(L.Q4, m, k, ow.blob()) for m, ow in zip(ms, ows)]
    x, xd = rows_x(ctx, rng, k)
    nw = O.f32_to_bf16((1 + rng.normal(0, 0.1, size=k)).astype(np.float32)) if norm else None
    nwd = bf16_t(nw, ctx.device) if norm else None
    q = torch.zeros(R, ms[0], dtype=torch.bfloat16, device=ctx.device)
    kc = torch.zeros(n_pos, ms[1], dtype=torch.bfloat16, device=ctx.device)
    vc = torch.zeros(n_pos, ms[2], dtype=torch.bfloat16, device=ctx.device)
    ctx.norm_linear_rows(xd[:R], nwd, dws, ys=[q, kc, vc], y_row_stride=[ms[0], 0, 0], y_pos_stride=[0, ms[1], ms[2]], pos0=pos0)
    got = [u16(q), u16(kc), u16(vc)]
    for r in range(R):
        one = [u16(y) for y in ctx.norm_linear(xd[r], nwd, dws)]
        xn = O.rmsnorm(x[r], nw, 1e-6) if norm else x[r]
        with O.canonical(rows=sum(ms)):
            ref = [O.linear(ow, xn) for ow in ows]
        for j in range(3):
            mine = got[j][r] if j == 0 else got[j][pos0 + r]
            assert np.array_equal(mine, one[j]) and np.array_equal(mine, ref[j]), (r, j)
    for c in got[1:]:   # no other cache row is touched
        assert not c[:pos0].any() and not c[pos0 + R:].any()


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("norm", [True, False])
def test_gate_up_swiglu_rows(ctx, canon, norm, R):
    rng = np.random.default_rng(78)
    f, k = 330, 1024   # 330: no multiple of the two rows per wave slot's workgroup share
    og, ou = weights(rng, f, k), weights(rng, f, k, symmetric=True)
    dg, du = ctx.upload_blob(L.Q4, f, k, og.blob()), ctx.upload_blob(L.Q4, f, k, ou.blob(), symmetric=True)
    x, xd = rows_x(ctx, rng, k)
    nw = O.f32_to_bf16((1 + rng.normal(0, 0.1, size=k)).astype(np.float32)) if norm else None
    nwd = bf16_t(nw, ctx.device) if norm else None
    act = u16(ctx.norm_gateup_swiglu_rows(xd[:R], nwd, dg, du))
    for r in range(R):
        one = u16(ctx.norm_gateup_swiglu(xd[r], nwd, dg, du))
        xn = O.rmsnorm(x[r], nw, 1e-6) if norm else x[r]
        with O.canonical(rows=f):
            ref = O.swiglu(O.linear(og, xn), O.linear(ou, xn))
        assert np.array_equal(act[r], one) and np.array_equal(act[r], ref), r


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("norm", [True, False])
def test_head_rows_pick_the_first_maximum(ctx, canon, norm, R):
    """a 512 x 256 bf16 head whose rows 100 and 300 are equal and win for the even activation rows: the tie must go to id 100"""
    rng = np.random.default_rng(79)
    v, k = 512, 256
    x = O.f32_to_bf16(rng.normal(0, 1.0, size=(RMAX, k)).astype(np.float32))
    for r in range(2, RMAX, 2):
        x[r] = O.f32_to_bf16(O.bf16_to_f32(x[0]) * 2.0 ** (r // 2))   # exact scalings of row 0
    w = O.f32_to_bf16(rng.normal(0, 0.05, size=(v, k)).astype(np.float32))
    w[100] = w[300] = O.f32_to_bf16(O.bf16_to_f32(x[0]) * 0.5)
    oh = O.quantize(w, v, k, L.BF16)
    dh = ctx.upload_blob(L.BF16, v, k, oh.blob())
    buf = torch.zeros(RMAX, k + 8, dtype=torch.bfloat16, device=ctx.device)
    buf[:, :k] = bf16_t(x, ctx.device)
    xd = buf[:, :k]
    nw = O.f32_to_bf16((1 + rng.normal(0, 0.1, size=k)).astype(np.float32)) if norm else None
    nwd = bf16_t(nw, ctx.device) if norm else None
    logits, top1 = ctx.norm_lm_head_rows(dh, xd[:R], nwd)
    _, top1_only = ctx.norm_lm_head_rows(dh, xd[:R], nwd, want_logits=False)
    logits = u16(logits)
    d = dh.desc()
    for r in range(R):
        one = torch.zeros(v, dtype=torch.bfloat16, device=ctx.device)
        L.check(ctx.hip.kf_norm_lm_head(ctx.h, C.c_void_p(xd[r].data_ptr()), C.c_void_p(nwd.data_ptr()) if norm else None, 1e-6, C.byref(d),
                                        C.c_void_p(one.data_ptr()), None, None, C.c_void_p(ctx._head_ws.data_ptr())), "kf_norm_lm_head")
        xn = O.rmsnorm(x[r], nw, 1e-6) if norm else x[r]
        ref = O.linear(oh, xn)
        assert np.array_equal(logits[r], u16(one)) and np.array_equal(logits[r], ref), r
        assert top1[r] == O.argmax_bf16(ref) == top1_only[r], r
        if r % 2 == 0:
            assert ref[100] == ref[300] and top1[r] == 100, r


def test_a_storage_that_falls_back(ctx, canon):
    """1-bit weights through the same entry: the one-token launch row by row, the same bits, and the route says so"""
    rng = np.random.default_rng(80)
    m, k, R = 96, 1024, 3
    ow = weights(rng, m, k, type_=L.BOOL1)
    dw = ctx.upload_blob(L.BOOL1, m, k, ow.blob())
    x, xd = rows_x(ctx, rng, k)
    before = ctx.rows_route_counts()
    y = u16(ctx.linear_rows(dw, xd[:R]))
    after = ctx.rows_route_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (0, R)
    for r in range(R):
        assert np.array_equal(y[r], u16(ctx.linear(dw, xd[r]))) and np.array_equal(y[r], O.linear(ow, x[r])), r


def test_the_dot2_order_falls_back(ctx):
    ow, dw, x, xd, one, ref = plain_case(ctx, 70, 1024, False)
    ctx.set_canonical(False)
    try:
        before = ctx.rows_route_counts()
        y = u16(ctx.linear_rows(dw, xd[:4]))
        after = ctx.rows_route_counts()
        one2 = np.stack([u16(ctx.linear(dw, xd[r])) for r in range(4)])
    finally:
        ctx.set_canonical(True)
    assert (after[0] - before[0], after[1] - before[1]) == (0, 4)
    assert np.array_equal(y, one2)


@pytest.mark.parametrize("R", [5, 8])
def test_two_row_panels(ctx, canon, R):
    """9728-wide rows (the 4B down_proj's width): four bf16 rows of activations per 80 KiB panel, so R = 8 runs as 4 + 4 and R = 5 as 3 + 2"""
    rng = np.random.default_rng(81)
    m, k = 66, 9728
    ow = weights(rng, m, k)
    dw = ctx.upload_blob(L.Q4, m, k, ow.blob())
    x, xd = rows_x(ctx, rng, k)
    res = O.f32_to_bf16(rng.normal(0, 1.0, size=(R, m)).astype(np.float32))
    y = bf16_t(res, ctx.device).clone()
    ctx.linear_rows(dw, xd[:R], residual=y, y=y)
    y = u16(y)
    for r in range(R):
        one = u16(ctx.linear(dw, xd[r], residual=bf16_t(res[r], ctx.device)))
        ref = O.add(res[r], O.linear(ow, x[r]))
        assert np.array_equal(y[r], one) and np.array_equal(y[r], ref), r


def test_refusals(ctx):
    ow, dw, x, xd, one, ref = plain_case(ctx, 70, 1024, False)
    d = dw.desc()
    y = torch.zeros(9, 70, dtype=torch.bfloat16, device=ctx.device)
    x9 = torch.zeros(9, 1024, dtype=torch.bfloat16, device=ctx.device)
    call = lambda n, xs, epi, res: ctx.hip.kf_linear_rows(ctx.h, C.byref(d), C.c_void_p(x9.data_ptr()), xs, C.c_void_p(y.data_ptr()), 70, n, epi, res, 0)
    assert call(0, 1024, 0, None) == -20 and call(9, 1024, 0, None) == -20      # KF_INVALID_ARGS: rows outside 1 .. 8
    assert call(4, 1028, 0, None) == -2000                                         # KF_BLAS_UNALIGN: rows of x not 16-byte aligned
    assert call(4, 1024, L.KF_EPI_RESIDUAL, None) == -20                           # the residual epilogue without a residual
    assert call(4, 1024, 0, None) == 0
