"""The forward token-batch GEMMs (kf_linear from 8 rows, kf_linear_multi, kf_gateup_swiglu_batch, kf_qkv_rope_batch / _seqs) on inputs whose arithmetic is exact in fp32
under every summation order (tests/exact_inputs.py): every element of y equals bf16(exact) BIT FOR BIT, in every family and form kf_gemm_plan.h sends a forward
product down -- the direct kernel (32- and 64-token tiles), the paired one, the staged kernel (KS 1 and 2), the producer / consumer kernel, the five kf_gemm3.hip tile
forms plain, in S k pieces and in the owner / helper cut -- on every storage the kernels unpack in registers (bf16, f8e5m2, 4-bit groups of 64 / 128 / 256 with either
qBias, 4-bit row codebooks, ternary, both 1-bit types), and on the routes that dequantise first (scratch, resident, stacked, interleaved + SwiGLU, stacked + RoPE).
The weights are built from chosen codes and chosen (zero, step) tables that differ from group to group; tests/test_exact_inputs_cpu.py pins which case runs which
form and checks every precondition on the CPU.  Before each call the plan of that very call is asserted to be the one the case table names.  Guard rows lie before and
behind every output, outputs and scratch arrive filled with a pattern, and every call runs twice (other patterns) to the same bits.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests import exact_inputs as E
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu
GUARD, GUARD_BITS = 4, 0x7B7B            # rows before and behind every output, and what they hold
PATTERNS = ((0xA5, 0x4B4B), (0x3C, 0x3A3A))   # (scratch byte, output prefill) of the two runs


@pytest.fixture(autouse=True)
def nothing_lent(ctx):
    """every case starts and ends with no scratch lent and no arena set"""
    def reset():
        ctx.sync()
        L.check(ctx.hip.kf_set_dequant_arena(ctx.h, None, 0), "kf_set_dequant_arena")
        L.check(ctx.hip.kf_set_scratch(ctx.h, None, 0), "kf_set_scratch")
        ctx._lin_ws = None
    reset()
    yield
    reset()


def _upload(ctx, storage, ow, W):
    """the constructed weight on the device; its kf_dequant equals the integer weight (the operand the GEMM is given), its pointers are aligned as the plan assumes"""
    type_, row_lut, symmetric, lgroup = E.STORAGES[storage]
    dw = ctx.upload_lut_blob(ow.ne0, ow.ne1, ow.blob()) if row_lut else ctx.upload_blob(type_, ow.ne0, ow.ne1, ow.blob(), lgroup, symmetric)
    d = dw.desc()
    assert d.data % 16 == 0 and (not row_lut or (d.gama + 2 * (ow.ne0 + ow.ne1)) % 16 == 0)
    assert d.qBias == ow.qBias
    assert np.array_equal(u16(ctx.dequant(dw)), E.exact_bits(W))
    return dw


def _guarded(ctx, n, M, fill):
    """(buffer, its [n, M] middle): GUARD rows of GUARD_BITS on either side, the middle prefilled with `fill` (bit pattern, or an [n, M] array of them)"""
    buf = torch.full(((n + 2 * GUARD) * M,), GUARD_BITS, dtype=torch.int16, device=ctx.device).view(torch.bfloat16)
    y = buf[GUARD * M:(GUARD + n) * M].view(n, M)
    if np.isscalar(fill):
        y.view(torch.int16).fill_(fill)
    else:
        y.copy_(bf16_t(fill, ctx.device))
    return buf, y


def _guards_intact(buf, n, M):
    b = u16(buf)
    return (b[:GUARD * M] == GUARD_BITS).all() and (b[(GUARD + n) * M:] == GUARD_BITS).all()


def _lend(ctx, nbytes, byte):
    """a scratch of nbytes filled with `byte`, lent through kf_set_scratch (kept alive on the context)"""
    ctx.sync()
    ctx._lin_ws = torch.full((nbytes + 256,), byte, dtype=torch.uint8, device=ctx.device)
    sp = (ctx._lin_ws.data_ptr() + 255) & ~255
    L.check(ctx.hip.kf_set_scratch(ctx.h, C.c_void_p(sp), C.c_size_t(nbytes)), "kf_set_scratch")


def _assert_plan(ctx, key, arena_hit=0):
    p = E.case_plan(ctx.hip, key, arena_hit)
    assert E.forward_name(p) == E.FORWARD_CASES[key], "the plan moved: %s is now %s" % (key, E.forward_name(p))
    return p


def _ids(keys):
    return ["%s-%s-%s-K%d-n%d-%s%s" % (k[0], k[1], "x".join(map(str, k[2])), k[3], k[4], k[5], "-" + k[6] if k[6] else "") for k in keys]


def _keys(entry, *settings):
    return [k for k in E.FORWARD_CASES if k[0] in entry and (not settings or k[6] in settings)]


# ---------------------------------------------------------------------------------------------------------------- kf_linear
def _linear(ctx, dw, c, key, pattern):
    """one kf_linear of the case (its epilogue form when the case has one) -> the bits of y; the guards are checked here"""
    n, M, epi = c["n"], c["M"], key[6] == "epi"
    x = bf16_t(c["x"], ctx.device)
    assert x.data_ptr() % 16 == 0
    buf, y = _guarded(ctx, n, M, c["y0"] if epi else pattern[1])
    bias = bf16_t(c["bias"], ctx.device) if epi else None
    res = bf16_t(c["residual"], ctx.device) if epi else None
    d = dw.desc()
    rc = ctx.hip.kf_linear(ctx.h, C.byref(d), x.data_ptr(), y.data_ptr(), bias.data_ptr() if epi else None, n, E.ALPHA if epi else 1.0, E.BETA if epi else 0.0,
                           L.KF_EPI_RESIDUAL if epi else 0, res.data_ptr() if epi else None)
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    assert _guards_intact(buf, n, M)
    return u16(y).copy()


@pytest.mark.parametrize("key", _keys(("linear",), "", "epi", "scratch"), ids=_ids(_keys(("linear",), "", "epi", "scratch")))
def test_linear_forward_exact(ctx, key):
    """kf_linear on the weight as stored (the mat-vec loop below 8 rows included) and on the copy dequantised into the caller's scratch"""
    c = E.forward_case(ctx.hip, key)
    dw = _upload(ctx, key[1], c["ow"], c["W"])
    want = c["y_epi"] if key[6] == "epi" else c["y"]
    scratch, _ = E.case_setting(key)
    if scratch:
        d = dw.desc()
        assert ctx.hip.kf_linear_scratch_bytes(C.byref(d), c["n"]) == scratch
    runs = []
    for pattern in PATTERNS:
        if scratch:
            _lend(ctx, scratch, pattern[0])
        _assert_plan(ctx, key)
        runs.append(_linear(ctx, dw, c, key, pattern))
        print("%s: %d of %d values differ from the exact bits" % (key, int((runs[-1] != want).sum()), want.size))
        assert np.array_equal(runs[-1], want)
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("key", _keys(("linear",), "arena"), ids=_ids(_keys(("linear",), "arena")))
def test_linear_forward_exact_resident(ctx, key):
    """kf_linear on the resident bf16 copy with the 64-row tiles in k pieces: once filling the arena, once finding the copy in it.  The block family lays a dense 128-term
    sum on the first and last k tile and astride every seam between two workgroups' pieces of this very plan."""
    c = E.forward_case(ctx.hip, key)
    dw = _upload(ctx, key[1], c["ow"], c["W"])
    scratch, _ = E.case_setting(key)
    assert scratch == ctx.hip.kf_resident_scratch_bytes()
    nbytes = (c["M"] * c["K"] * 2 + 255) & ~255
    arena = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=ctx.device)
    runs = []
    try:
        L.check(ctx.hip.kf_set_dequant_arena(ctx.h, C.c_void_p(arena.data_ptr()), C.c_size_t(nbytes)), "kf_set_dequant_arena")
        for i, pattern in enumerate(PATTERNS):
            _lend(ctx, scratch, pattern[0])
            assert ctx.hip.kf_dequant_arena_used(ctx.h) == (nbytes if i else 0)
            p = _assert_plan(ctx, key, arena_hit=i)   # the copy in the stacked form (bit 0) is resident from the second call on
            assert p.deq == (E.DQ_RESIDENT if i else E.DQ_ARENA) and p.ws_bytes == scratch
            runs.append(_linear(ctx, dw, c, key, pattern))
            print("%s (%s): %d of %d values differ from the exact bits" % (key, "finding" if i else "filling", int((runs[-1] != c["y"]).sum()), c["y"].size))
            assert np.array_equal(runs[-1], c["y"])
            assert ctx.hip.kf_dequant_arena_used(ctx.h) == nbytes
        assert np.array_equal(u16(arena.view(torch.bfloat16)).reshape(-1)[:c["M"] * c["K"]], E.exact_bits(c["W"]).reshape(-1))   # the resident copy is the integer weight
    finally:
        ctx.sync()
        L.check(ctx.hip.kf_set_dequant_arena(ctx.h, None, 0), "kf_set_dequant_arena")
    assert np.array_equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------------------- several matrices sharing x
def _shared(ctx, key):
    """the case, its uploaded weights and their descriptors; the scratch query answers what the case lends"""
    c = E.forward_case(ctx.hip, key)
    parts = [c] + c["more"]
    dws = [_upload(ctx, key[1], p["ow"], p["W"]) for p in parts]
    descs = [d.desc() for d in dws]
    scratch, _ = E.case_setting(key)
    if scratch:
        wp = (C.c_void_p * len(descs))(*[C.addressof(d) for d in descs])
        assert ctx.hip.kf_linear_multi_scratch_bytes(len(descs), wp, c["n"]) == scratch
    return c, parts, dws, descs, scratch


@pytest.mark.parametrize("key", _keys(("multi",)), ids=_ids(_keys(("multi",))))
def test_linear_multi_exact(ctx, key):
    """kf_linear_multi: the fused direct launch (32- and 64-token tiles) and the stacked kf_gemm3.hip launch; a distinct weight per matrix, so a row landing in the wrong
    output shows"""
    c, parts, dws, descs, scratch = _shared(ctx, key)
    n, x = c["n"], bf16_t(c["x"], ctx.device)
    wp = (C.c_void_p * len(descs))(*[C.addressof(d) for d in descs])
    runs = []
    for pattern in PATTERNS:
        if scratch:
            _lend(ctx, scratch, pattern[0])
        _assert_plan(ctx, key)
        outs = [_guarded(ctx, n, p["M"], pattern[1]) for p in parts]
        yp = (C.c_void_p * len(outs))(*[y.data_ptr() for _, y in outs])
        assert ctx.hip.kf_linear_multi(ctx.h, len(descs), wp, x.data_ptr(), yp, n) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        got = [u16(y).copy() for _, y in outs]
        for j, (p, (buf, _), g) in enumerate(zip(parts, outs, got)):
            print("%s matrix %d: %d of %d values differ from the exact bits" % (key, j, int((g != p["y"]).sum()), g.size))
            assert _guards_intact(buf, n, p["M"])
            assert np.array_equal(g, p["y"]), "matrix %d" % j
        runs.append(got)
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("key", _keys(("gateup",)), ids=_ids(_keys(("gateup",))))
def test_gateup_swiglu_exact(ctx, key):
    """kf_gateup_swiglu_batch: the paired direct kernel and the interleaved copy with the SwiGLU epilogue (128 x 128, 192 x 256 and 256 x 256 tiles).  Both apply kf_swiglu's
    expression to the bf16-rounded projections; with integer accumulators that rounding is the identity, so act = swiglu(bits(gate), bits(up)) bit for bit"""
    c, parts, dws, descs, scratch = _shared(ctx, key)
    n, ffn, x = c["n"], c["M"], bf16_t(c["x"], ctx.device)
    want = O.swiglu(parts[0]["y"].reshape(-1), parts[1]["y"].reshape(-1)).reshape(n, ffn)
    runs = []
    for pattern in PATTERNS:
        if scratch:
            _lend(ctx, scratch, pattern[0])
        p = _assert_plan(ctx, key)
        (abuf, act), (ubuf, up) = _guarded(ctx, n, ffn, pattern[1]), _guarded(ctx, n, ffn, pattern[1])
        assert act.data_ptr() % 8 == 0
        rc = ctx.hip.kf_gateup_swiglu_batch(ctx.h, C.byref(descs[0]), C.byref(descs[1]), x.data_ptr(), act.data_ptr(), up.data_ptr(), n)
        assert rc == 0, ctx.hip.kf_last_error()
        ctx.sync()
        runs.append(u16(act).copy())
        print("%s: %d of %d values differ from the exact bits" % (key, int((runs[-1] != want).sum()), want.size))
        assert _guards_intact(abuf, n, ffn) and _guards_intact(ubuf, n, ffn)
        assert np.array_equal(runs[-1], want)
        if E.FWD_ROUTES[p.route] == "SWIGLU":   # the up projection is never written
            assert (u16(up) == pattern[1]).all()
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("key", _keys(("rope", "rope_seqs")), ids=_ids(_keys(("rope", "rope_seqs"))))
def test_qkv_rope_exact(ctx, key):
    """kf_qkv_rope_batch / kf_qkv_rope_seqs: the stacked launch with q/k-norm + RoPE in its epilogue.  v equals the exact bits; q and k equal kf_qknorm_rope_batch /
    kf_qknorm_rope_train run on the uploaded EXACT q and k bits -- the GEMM held exactly, the epilogue against the separate launch (which has its own oracle tests)"""
    c, parts, dws, descs, scratch = _shared(ctx, key)
    n, x, hd, eps = c["n"], bf16_t(c["x"], ctx.device), 128, 1e-6
    ms = [p["M"] for p in parts]
    n_head, n_kv = ms[0] // hd, ms[1] // hd
    seq = E.ROPE_SEQ_LEN[c["n"]] if key[0] == "rope_seqs" else 0
    pos0 = 0 if seq else 3
    rng = np.random.default_rng(n)
    wq, wk = (bf16_t(O.f32_to_bf16((1 + rng.normal(0, 0.1, size=hd)).astype(np.float32)), ctx.device) for _ in range(2))
    table = ctx.rope_table(pos0 + n + 1, hd, 1e6)
    q_ref, k_ref = bf16_t(parts[0]["y"], ctx.device).clone(), bf16_t(parts[1]["y"], ctx.device).clone()
    if seq:
        L.check(ctx.hip.kf_qknorm_rope_train(ctx.h, q_ref.data_ptr(), k_ref.data_ptr(), wq.data_ptr(), wk.data_ptr(), table.data_ptr(), n, seq, ms[0], ms[1], n_head, n_kv, hd, eps,
                                             None, None), "kf_qknorm_rope_train")
    else:
        L.check(ctx.hip.kf_qknorm_rope_batch(ctx.h, q_ref.data_ptr(), k_ref.data_ptr(), wq.data_ptr(), wk.data_ptr(), table.data_ptr(), pos0, n, ms[0], ms[1], n_head, n_kv, hd, eps),
                "kf_qknorm_rope_batch")
    ctx.sync()
    want = [u16(q_ref).copy(), u16(k_ref).copy(), parts[2]["y"]]
    assert not np.array_equal(want[0], parts[0]["y"])   # q really went through the norm and the rotation
    runs = []
    for pattern in PATTERNS:
        _lend(ctx, scratch, pattern[0])
        _assert_plan(ctx, key)
        outs = [_guarded(ctx, n, m, pattern[1]) for m in ms]
        ys = [y for _, y in outs]
        assert (ys[0].data_ptr() | ys[1].data_ptr()) % 8 == 0
        if seq:
            L.check(ctx.hip.kf_qkv_rope_seqs(ctx.h, C.byref(descs[0]), C.byref(descs[1]), C.byref(descs[2]), x.data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(), ys[2].data_ptr(), n, seq,
                                             wq.data_ptr(), wk.data_ptr(), table.data_ptr(), 0, n_head, n_kv, hd, eps), "kf_qkv_rope_seqs")
        else:
            L.check(ctx.hip.kf_qkv_rope_batch(ctx.h, C.byref(descs[0]), C.byref(descs[1]), C.byref(descs[2]), x.data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(), ys[2].data_ptr(), n,
                                              wq.data_ptr(), wk.data_ptr(), table.data_ptr(), pos0, n_head, n_kv, hd, eps), "kf_qkv_rope_batch")
        ctx.sync()
        got = [u16(y).copy() for y in ys]
        for name, (buf, _), g, w, m in zip("qkv", outs, got, want, ms):
            print("%s %s: %d of %d values differ" % (key, name, int((g != w).sum()), g.size))
            assert _guards_intact(buf, n, m)
            assert np.array_equal(g, w), name
        runs.append(got)
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
