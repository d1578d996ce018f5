"""kf_linear_a8_tiles -- the int8-activation product of a token batch on int8 MFMA tiles -- and the host route that sends token batches to it.  The definition
(include/kf_abi.h "int8 activations") is exact up to ONE ascending fp32 chain over the K / 128 groups of a row, and the tile kernel keeps that chain, so every comparison
here is an equality of bits: with the numpy restatement (tests/a8_restate.py), with kf_linear_a8 on the device, and of the model's two routes with each other."""
import numpy as np
import pytest
import torch

from a8_restate import BITS, IntW, linear_a8, quant_rows, to_bf
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FILL = 0x7fc1      # a bf16 NaN pattern no kernel stores
ROW_TILE = 64      # kf::a8_tile_plan: four waves of 16 rows (tests/test_a8_tiles_cpu.py pins it)
NTOKS = (1, 15, 16, 17, 33, 70)


def t_bf16(u16_, dev):
    return torch.from_numpy(np.ascontiguousarray(u16_).view(np.int16)).to(dev).view(torch.bfloat16)


def u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def run(ctx, entry, dw, q, step, bias=None, residual=None, alias=False):
    """one launch into a buffer pre-filled with FILL that has two guard rows behind the outputs; alias: the residual is y itself"""
    n, M = q.shape[0], dw.ne0
    buf = t_bf16(np.full((n + 2, M), FILL, dtype=np.uint16), ctx.device)
    y = buf[:n]
    if alias:
        y.copy_(t_bf16(residual, ctx.device))
    dq, ds = torch.from_numpy(np.ascontiguousarray(q)).to(ctx.device), torch.from_numpy(np.ascontiguousarray(step)).to(ctx.device)
    res = y if alias else None if residual is None else t_bf16(residual, ctx.device)
    getattr(ctx, entry)(dw, dq, ds, bias=None if bias is None else t_bf16(bias, ctx.device), residual=res, y=y)
    ctx.sync()
    out = u16(buf)
    assert (out[n:] == FILL).all(), "%s wrote behind its %d token rows" % (entry, n)
    return out[:n]


# ---------------------------------------------------------------- 1. the product
_CASE = {}


def case(ctx, type_, M, K):
    """per (type, shape): the oracle-quantised weight on the device, its integer restatement, ONE draw of 70 activation rows and the restatement's product of all 70"""
    key = (type_, M, K)
    if key not in _CASE:
        w = to_bf(np.random.default_rng(5 + M + K).normal(0, 0.05, (M, K)).astype(np.float32))
        ow = O.quantize(w, M, K, type_)
        iw = IntW(ow)
        q, s = quant_rows(to_bf(np.random.default_rng(M * K).normal(0, 1, (70, K)).astype(np.float32)))
        _CASE[key] = (ctx.upload_blob(type_, M, K, ow.blob()), iw, q, s, linear_a8(iw, q, s))
    return _CASE[key]


SHAPES = [(1, 128), (7, 384), (64, 1024), (257, 3072), (2 * ROW_TILE + 22, 512)]   # the last: above the row tile and no multiple of it, two full workgroups and a tail


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1, L.T_BINARY])
@pytest.mark.parametrize("M,K", SHAPES)
def test_product_bit_for_bit(ctx, type_, M, K):
    dw, iw, q, s, ref = case(ctx, type_, M, K)
    for n in NTOKS:
        got = run(ctx, "linear_a8_tiles", dw, q[:n], s[:n])
        assert not (got == FILL).any(), "nTok = %d: an output element kept the fill value" % n
        assert np.array_equal(got, ref[:n]), "nTok = %d: %d of %d outputs differ from the restatement" % (n, int((got != ref[:n]).sum()), got.size)
        assert np.array_equal(got, run(ctx, "linear_a8", dw, q[:n], s[:n])), "nTok = %d: differs from kf_linear_a8" % n


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1])
@pytest.mark.parametrize("M,K", [(7, 384), (257, 3072)])
@pytest.mark.parametrize("n", [1, 17, 70])
def test_epilogue(ctx, type_, M, K, n):
    dw, iw, q, s, _ = case(ctx, type_, M, K)
    rng = np.random.default_rng(M + n)
    bias = to_bf(rng.normal(0, 0.5, M).astype(np.float32))
    res = to_bf(rng.normal(0, 1, (n, M)).astype(np.float32))
    q, s = q[:n], s[:n]
    assert np.array_equal(run(ctx, "linear_a8_tiles", dw, q, s, bias=bias), linear_a8(iw, q, s, bias=bias))
    want = linear_a8(iw, q, s, residual=res)
    assert np.array_equal(run(ctx, "linear_a8_tiles", dw, q, s, residual=res), want)
    assert np.array_equal(run(ctx, "linear_a8_tiles", dw, q, s, residual=res, alias=True), want), "residual aliasing y"
    want = linear_a8(iw, q, s, bias=bias, residual=res)
    assert np.array_equal(run(ctx, "linear_a8_tiles", dw, q, s, bias=bias, residual=res, alias=True), want)
    assert np.array_equal(run(ctx, "linear_a8", dw, q, s, bias=bias, residual=res), want)


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1])
def test_product_saturating(ctx, type_):
    """the setup of tests/test_gpu_a8.py test_product_saturating at nTok = 17: every |I_g| = 16 256, where a narrower intermediate would overflow"""
    M, K, n = 8, 384, 17
    G = K // 128
    codes = np.ones((M, G, 128), dtype=np.int32)
    if type_ == L.T_SIGN:
        codes[:] = 2                      # t_w = +1
        codes[1::2, :, :] = 0             # t_w = -1 in every other row
        codes[2, 1, :] = 1                # one all-zero group
    step_w = to_bf(np.random.default_rng(9).uniform(0.01, 0.2, M * G).astype(np.float32))
    ow = O.QWeight(type_, M, K, O.pack(codes, BITS[type_]), np.zeros(M * G, dtype=np.uint16), step_w, 128, 1 if type_ == L.T_SIGN else 0)
    dw, iw = ctx.upload_blob(type_, M, K, ow.blob()), IntW(ow)
    q = np.full((n, K), 127, dtype=np.int8)
    q[1::4] = -127
    q[2::4, ::2] = -127
    q[3::4, 128:256] = -127
    step = np.resize(np.array([1.0, 0.37, 2.5e-3, 11.0, 1.0], dtype=np.float32), n)
    I = np.einsum("mgc,tgc->tmg", iw.t.reshape(M, G, 128), q.astype(np.int64).reshape(n, G, 128))
    assert np.abs(I).max() == 16256
    got = run(ctx, "linear_a8_tiles", dw, q, step)
    assert not (got == FILL).any() and np.array_equal(got, linear_a8(iw, q, step))
    assert np.array_equal(got, run(ctx, "linear_a8", dw, q, step))


@pytest.mark.parametrize("type_", [L.T_SIGN, L.BOOL1])
def test_unaligned_activations(ctx, type_):
    """q one byte into a buffer: the kernel's 16-byte staging loads are not allowed there; the contract (any q the mat-vec takes) and the bits stay"""
    M, K, n = 7, 384, 17
    dw, iw, q, s, ref = case(ctx, type_, M, K)
    raw = torch.zeros(n * K + 16, dtype=torch.int8, device=ctx.device)
    dq = raw[1:1 + n * K].view(n, K)
    dq.copy_(torch.from_numpy(np.ascontiguousarray(q[:n])))
    assert dq.data_ptr() % 16 == 1
    y = t_bf16(np.full((n, M), FILL, dtype=np.uint16), ctx.device)
    ctx.linear_a8_tiles(dw, dq, torch.from_numpy(np.ascontiguousarray(s[:n])).to(ctx.device), y=y)
    ctx.sync()
    assert np.array_equal(u16(y), ref[:n])


# ---------------------------------------------------------------- 2. refusals
@pytest.mark.parametrize("type_", [L.Q4, L.BF16])
def test_refusals(ctx, type_):
    M, K = 16, 256
    w = to_bf(np.random.default_rng(3).normal(0, 0.05, (M, K)).astype(np.float32))
    dw = ctx.upload_blob(type_, M, K, O.quantize(w, M, K, type_).blob())
    q = torch.zeros((33, K), dtype=torch.int8, device=ctx.device)
    step = torch.ones(33, dtype=torch.float32, device=ctx.device)
    for entry in ("linear_a8_tiles", "linear_a8"):
        with pytest.raises(L.KFError) as e:
            getattr(ctx, entry)(dw, q, step)
        assert "code -1000" in str(e.value) and ("type %d" % type_) in str(e.value)


# ---------------------------------------------------------------- 3. the model's routes
CFG = dict(synth.CONFIGS["small"], max_seq=96)
N_MAT = 7 * CFG["n_layer"]   # layer matrices = launches of one pass
_M = {}


def model(layer_type):
    if layer_type not in _M:
        raw = synth.raw_weights_numpy(CFG, 1234, w_std=0.1)
        gm = synth.build_from_raw(CFG, raw, layer_type, L.BF16)
        gm.set_canonical(1)
        _M[layer_type] = (gm, raw, prompt_ids(CFG, 71))
    return _M[layer_type]


def both_passes(gm, toks, tile_min, want_counts):
    """prefill of the first 70 tokens, then score of all 71, on the route tile_min selects: everything either leaves behind, and the route counts of each pass"""
    gm.set_a8_tile_min(tile_min)
    gm.set_act_int8(True)   # the counts restart at a switch-on
    nxt, lg = gm.prefill(toks[:70])
    assert gm.a8_route_counts() == want_counts
    k, v = gm.kv_to_host()
    out = [np.array([nxt]), lg, k[:, :70].copy(), v[:, :70].copy()]
    gm.set_act_int8(True)
    lp = gm.score(toks)
    assert gm.a8_route_counts() == want_counts
    k, v = gm.kv_to_host()
    return out + [lp.view(np.uint32), gm.logits(), k[:, :71].copy(), v[:, :71].copy()]


@pytest.mark.parametrize("layer_type", [L.T_SIGN, L.BOOL1])
def test_model_route_equivalence(layer_type):
    gm, raw, toks = model(layer_type)
    try:
        tiles = both_passes(gm, toks, 2, (N_MAT, 0))
        matvec = both_passes(gm, toks, -1, (0, N_MAT))
        names = ("next id", "prefill logits", "prefill K rows", "prefill V rows", "log-probs", "score logits", "score K rows", "score V rows")
        for name, a, b in zip(names, tiles, matvec):
            assert np.array_equal(a, b), "%s: %d elements differ between the tile route and the mat-vec route" % (name, int((np.asarray(a) != np.asarray(b)).sum()))
        assert np.isfinite(tiles[4].view(np.float32)).all()
        # the default threshold (32): 12 tokens keep the mat-vec, 70 take the tiles
        gm.set_a8_tile_min(0)
        gm.set_act_int8(True)
        gm.prefill(toks[:12])
        assert gm.a8_route_counts() == (0, N_MAT)
        gm.set_act_int8(True)
        gm.prefill(toks[:70])
        assert gm.a8_route_counts() == (N_MAT, 0)
        # a single token always takes the mat-vec, whatever the threshold (1 is treated as 2)
        gm.set_a8_tile_min(1)
        gm.set_act_int8(True)
        gm.forward(int(toks[0]), 0)
        assert gm.a8_route_counts() == (0, N_MAT)
    finally:
        gm.set_a8_tile_min(0)
        gm.set_act_int8(False)


def test_layer0_against_the_restatement():
    """layer 0's K and V rows of the 70-token prefill on the tile route, computed directly (no attention precedes them): embed, rmsnorm, quant_rows, linear_a8,
    head-norm, rope -- as tests/test_gpu_a8.py test_model_batch_route holds the 12-token batch of the mat-vec route"""
    gm, raw, toks = model(L.T_SIGN)
    c, lw = CFG, raw["layers"][0]
    try:
        gm.set_a8_tile_min(2)
        gm.set_act_int8(True)
        gm.prefill(toks[:70])
        assert gm.a8_route_counts() == (N_MAT, 0)
        gk, gv = gm.kv_to_host()
    finally:
        gm.set_a8_tile_min(0)
        gm.set_act_int8(False)
    embed = O.quantize(raw["embed"], raw["embed"].shape[0], raw["embed"].shape[1], L.BF16)
    wk, wv = (IntW(O.quantize(lw[s], lw[s].shape[0], lw[s].shape[1], L.T_SIGN)) for s in ("k", "v"))
    with O.canonical():
        xn = np.stack([O.rmsnorm(O.embed(embed, int(t)), lw["norm_in"]) for t in toks[:70]])
        qx, sx = quant_rows(xn)
        kraw, vraw = linear_a8(wk, qx, sx), linear_a8(wv, qx, sx)
        k = np.stack([O.rope(O.headnorm(kraw[p], lw["kn"], c["n_kv"], c["head_dim"]), c["n_kv"], c["head_dim"], p, c["theta"]) for p in range(70)])
    assert np.array_equal(gv[0, :70], vraw), "%d V elements differ" % int((gv[0, :70] != vraw).sum())
    assert np.array_equal(gk[0, :70], k), "%d K elements differ" % int((gk[0, :70] != k).sum())


def test_mixed_storage_routes():
    """o_proj stored 4-bit: it keeps kf_rmsnorm / kf_linear, the other six matrices of a layer take the tiles -- the same equivalence, 6 launches per layer"""
    cfg = dict(synth.CONFIGS["tiny"], max_seq=96)
    raw = synth.raw_weights_numpy(cfg, 77, w_std=0.1)
    gm = synth.build_from_raw(cfg, raw, L.T_SIGN, L.BF16)
    si = synth.SLOTS.index("o")
    for li, lw in enumerate(raw["layers"]):
        gm.set_weight(li, si, gm._ctx.quantize(synth._bf16_t(lw["o"], gm._ctx.device), L.Q4))
    gm.set_canonical(1)
    toks, n6 = prompt_ids(cfg, 71), 6 * cfg["n_layer"]
    try:
        tiles = both_passes(gm, toks, 2, (n6, 0))
        matvec = both_passes(gm, toks, -1, (0, n6))
        for i, (a, b) in enumerate(zip(tiles, matvec)):
            assert np.array_equal(a, b), "output %d: %d elements differ between the routes" % (i, int((np.asarray(a) != np.asarray(b)).sum()))
    finally:
        gm.close()
