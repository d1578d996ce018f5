"""kf_attn_decode_rows: R consecutive queries of one sequence in one launch, query r at position pos0 + r against keys 0 .. pos0 + r.  Every output row equals
kf_attn_decode at its position AND the oracle's CANON attention, bit for bit -- across the one-slice / sliced boundary at 192 keys, across the 4-wave / 8-wave
boundary at 128 keys per slice, from position 0, and on a scratch that two calls share without re-zeroing."""
import numpy as np
import pytest
import torch

from conftest import bf16_t, u16
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def canonical_ctx(ctx):
    """the session's context in the canonical order for every test here, whatever order an earlier test file left it in; put back afterwards"""
    was = ctx.hip.kf_get_canonical(ctx.h)
    ctx.set_canonical(True)
    yield
    ctx.set_canonical(bool(was))


def case(ctx, n_head, n_kv, hd, pos0, R, seed=0):
    rng = np.random.default_rng(seed + pos0 + hd + n_head)
    kvd, n = n_kv * hd, pos0 + R
    q = O.f32_to_bf16(rng.normal(0, 1.0, size=(R, n_head * hd)).astype(np.float32))
    kc = O.f32_to_bf16(rng.normal(0, 1.0, size=(n, kvd)).astype(np.float32))
    vc = O.f32_to_bf16(rng.normal(0, 1.0, size=(n, kvd)).astype(np.float32))
    return q, kc, vc, bf16_t(q, ctx.device), bf16_t(kc, ctx.device), bf16_t(vc, ctx.device)


def check(ctx, got, q, kc, vc, qd, kd, vd, n_head, n_kv, hd, pos0):
    for r in range(got.shape[0]):
        one = u16(ctx.attn_decode(qd[r], kd, vd, pos0 + r, n_head, n_kv, hd))
        ref = O.attn_decode(q[r], kc[:pos0 + r + 1], vc[:pos0 + r + 1], pos0 + r, n_head, n_kv, hd, mode=O.ATTN_CANON)
        assert np.array_equal(got[r], one), "row %d: %d outputs differ from kf_attn_decode" % (r, int((got[r] != one).sum()))
        assert np.array_equal(got[r], ref), "row %d: %d outputs differ from the oracle" % (r, int((got[r] != ref).sum()))


@pytest.mark.parametrize("n_head,n_kv,hd,pos0,R", [
    (4, 2, 64, 188, 8),      # GQA-2, hd 64: rows 0 - 3 in one slice, rows 4 - 7 in four
    (8, 2, 128, 188, 8),     # GQA-4, hd 128
    (64, 32, 64, 2044, 8),   # GQA-2, 16 slices: 128 keys per slice up to row 3, 129 from row 4 on -- the launch's eight waves serve both
    (4, 2, 64, 0, 8),        # row 0 sees one key
    (8, 2, 128, 0, 3),
    (8, 8, 64, 300, 1),      # GQA-1, one row
    (16, 2, 128, 250, 5),    # GQA-8
])
def test_rows_equal_decode_at_each_position(ctx, n_head, n_kv, hd, pos0, R):
    q, kc, vc, qd, kd, vd = case(ctx, n_head, n_kv, hd, pos0, R)
    got = u16(ctx.attn_decode_rows(qd, kd, vd, pos0, n_head, n_kv, hd))
    check(ctx, got, q, kc, vc, qd, kd, vd, n_head, n_kv, hd, pos0)


def test_scratch_reused_without_rezeroing(ctx):
    """the arrival counters return to zero: two calls of different shapes on one scratch, zero-filled once"""
    n_head, n_kv, hd = 4, 2, 64
    scratch = torch.zeros(ctx.hip.kf_attn_rows_scratch_bytes(n_head, hd, 8), dtype=torch.uint8, device=ctx.device)
    for pos0, R in ((500, 8), (260, 6), (500, 8)):
        q, kc, vc, qd, kd, vd = case(ctx, n_head, n_kv, hd, pos0, R, seed=3)
        got = u16(ctx.attn_decode_rows(qd, kd, vd, pos0, n_head, n_kv, hd, scratch=scratch))
        check(ctx, got, q, kc, vc, qd, kd, vd, n_head, n_kv, hd, pos0)
    ctx.sync()
    assert not scratch[:16384].any()   # KF_ATTN_CNT_BYTES of row 0; the other rows' counters lie at the head of their own scratch
    per = scratch.numel() // 8
    assert all(not scratch[r * per:r * per + 16384].any() for r in range(8))


def test_the_dot2_order_runs_row_by_row(ctx):
    n_head, n_kv, hd, pos0, R = 4, 2, 64, 200, 4
    q, kc, vc, qd, kd, vd = case(ctx, n_head, n_kv, hd, pos0, R)
    ctx.set_canonical(False)
    try:
        got = u16(ctx.attn_decode_rows(qd, kd, vd, pos0, n_head, n_kv, hd))
        one = np.stack([u16(ctx.attn_decode(qd[r], kd, vd, pos0 + r, n_head, n_kv, hd)) for r in range(R)])
    finally:
        ctx.set_canonical(True)
    assert np.array_equal(got, one)


def test_refusals(ctx):
    q, kc, vc, qd, kd, vd = case(ctx, 4, 2, 64, 10, 2)
    out = torch.zeros(9, 256, dtype=torch.bfloat16, device=ctx.device)
    ws = torch.zeros(ctx.hip.kf_attn_rows_scratch_bytes(4, 64, 8), dtype=torch.uint8, device=ctx.device)
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda n, stride=256, pos0=10, hd=64: ctx.hip.kf_attn_decode_rows(ctx.h, p(qd), stride, p(kd), p(vd), p(out), pos0, n, 4, 2, hd, 128, p(ws))
    assert call(0) == -20 and call(9) == -20 and call(2, pos0=-1) == -20 and call(2, stride=128) == -20
    assert call(2) == 0
