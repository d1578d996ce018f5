"""The int8 KV cache kernels on the GPU, bit for bit against the numpy restatement of the definition (tests/kv8_restate.py; include/kf_abi.h "int8 KV cache"):
kf_kv8_quant_rows and kf_kv8_dequant_rows on strided rows inside pre-filled buffers, and kf_attn_block_kv8 -- the output, the new row's codes and both steps, every other
cache row and the row padding untouched, the arrival counters back at zero -- at the plan's seams (one slice up to 192 keys, four at 193, five for the bound 300, 32 at
2047), in both settings of kf_set_canonical (there is ONE arithmetic), and with the position below the launch bound."""
import numpy as np
import pytest
import torch

import exact_inputs as E
import kv8_restate as R
from conftest import bf16_t, u16
from oracle import oracle as O

pytestmark = pytest.mark.gpu
THETA, EPS = 1e6, 1e-6
PAD = 16            # bytes of padding behind every K8 / V8 row (kv_stride = kv_dim + PAD)
FILL8, FILLS = 0x5B, np.float32(777.0)
POSITIONS = [0, 1, 63, 64, 191, 192, 193, 300, 2047]   # the plan's slices are attn_slices': one slice | four (192 | 193 keys at 191 | 192), five of 61, 32 of 64
T_MAX = 2048


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("n_kv,hd", [(1, 64), (2, 128), (8, 128)])
@pytest.mark.parametrize("n", [1, 5, 33])
def test_quant_and_dequant_rows(ctx, n, n_kv, hd):
    kvd, pos0 = n_kv * hd, 3
    rng = np.random.default_rng(1000 * n + kvd)
    k = R.to_bf((rng.standard_normal((n, kvd + 8)) * rng.uniform(0.01, 30.0, (n, 1))).astype(np.float32))
    v = R.to_bf(rng.standard_normal((n, kvd + 8)).astype(np.float32))
    k[0, :hd] = 0                                         # a zero head
    v[n - 1, :hd] = R.to_bf(-np.abs(R.bf(v[n - 1, :hd])))  # a head whose largest element is negative
    rows = pos0 + n + 2
    k8 = torch.full((rows, kvd + PAD), FILL8, dtype=torch.int8, device=ctx.device)
    v8 = torch.full_like(k8, FILL8)
    ks = torch.full((rows, n_kv), float(FILLS), dtype=torch.float32, device=ctx.device)
    vs = torch.full_like(ks, float(FILLS))
    kd, vd = bf16_t(k, ctx.device), bf16_t(v, ctx.device)
    ctx.kv8_quant_rows(kd[:, :kvd], vd[:, :kvd], k8, v8, ks, vs, pos0, n_kv, hd)
    for got8, gots, src in ((k8, ks, k), (v8, vs, v)):
        want8, wants = R.quant_heads(src[:, :kvd], hd)
        full8 = np.full((rows, kvd + PAD), FILL8, dtype=np.int8)
        fulls = np.full((rows, n_kv), FILLS, dtype=np.float32)
        full8[pos0:pos0 + n, :kvd], fulls[pos0:pos0 + n] = want8, wants
        assert np.array_equal(got8.cpu().numpy(), full8), "%d codes differ" % int((got8.cpu().numpy() != full8).sum())
        assert np.array_equal(gots.cpu().numpy().view(np.uint32), fulls.view(np.uint32))
    # rows 0 .. n - 1 of a pair back to bf16, rows kv_dim + 8 apart, the 8 elements between them untouched
    c8 = [dev(R.quant_heads(s[:, :kvd], hd)[0], ctx.device) for s in (k, v)]
    cs = [dev(R.quant_heads(s[:, :kvd], hd)[1], ctx.device) for s in (k, v)]
    pad8 = [torch.full((n + 1, kvd + PAD), FILL8, dtype=torch.int8, device=ctx.device) for _ in range(2)]
    for p, c in zip(pad8, c8):
        p[:n, :kvd] = c
    ko = torch.full((n + 1, kvd + 8), 1.5, dtype=torch.bfloat16, device=ctx.device)
    vo = torch.full_like(ko, 1.5)
    ctx.kv8_dequant_rows(pad8[0], pad8[1], cs[0], cs[1], n, n_kv, hd, ko[:, :kvd], vo[:, :kvd])
    for got, c, s in ((ko, c8[0], cs[0]), (vo, c8[1], cs[1])):
        want = np.full((n + 1, kvd + 8), 0x3FC0, dtype=np.uint16)
        want[:n, :kvd] = R.dequant_heads(c.cpu().numpy(), s.cpu().numpy(), hd)
        assert np.array_equal(u16(got), want), "%d elements differ" % int((u16(got) != want).sum())


_BASE, _REF, _WS = {}, {}, {}


def base(nh, nkv, hd):
    """T_MAX random K / V rows of a shape already in the cache's form, raw q / k / v of the new token, the norm weights: drawn once per shape"""
    key = (nh, nkv, hd)
    if key not in _BASE:
        rng = np.random.default_rng(nh * 1000 + nkv * 10 + hd)
        kvd = nkv * hd
        draw = lambda *s: R.to_bf(rng.standard_normal(s).astype(np.float32))
        k = R.to_bf((rng.standard_normal((T_MAX, kvd)) * rng.uniform(0.25, 4.0, (T_MAX, 1))).astype(np.float32))
        c = R.Cache8(T_MAX, nkv, hd)
        c.put(0, k, draw(T_MAX, kvd))
        wq, wk = R.to_bf(rng.uniform(0.5, 1.5, hd).astype(np.float32)), R.to_bf(rng.uniform(0.5, 1.5, hd).astype(np.float32))
        _BASE[key] = (c, R.to_bf((3 * rng.standard_normal(nh * hd)).astype(np.float32)), draw(kvd), draw(kvd), wq, wk)
    return _BASE[key]


def reference(nh, nkv, hd, pos):
    """the restatement at `pos`: (out, the new row's K codes, K steps, V codes, V steps): computed once, shared by every test and order"""
    key = (nh, nkv, hd, pos)
    if key not in _REF:
        c, q, kr, vr, wq, wk = base(nh, nkv, hd)
        qp = O.rope(O.headnorm(q, wq, nh, hd, EPS), nh, hd, pos, THETA)
        kp = O.rope(O.headnorm(kr, wk, nkv, hd, EPS), nkv, hd, pos, THETA)
        old = [a[pos].copy() for a in (c.k8, c.ks, c.v8, c.vs)]
        c.put(pos, kp, vr)
        new = [a[pos].copy() for a in (c.k8, c.ks, c.v8, c.vs)]
        out = c.attend(qp, pos, nh)
        c.k8[pos], c.ks[pos], c.v8[pos], c.vs[pos] = old
        _REF[key] = [out] + new
    return _REF[key]


def scratch(ctx):
    """ONE scratch for the module, zeroed when it is made and never again: the kernel leaves its arrival counters at zero"""
    if "ws" not in _WS:
        _WS["ws"] = torch.zeros(ctx.hip.kf_attn_scratch_bytes(8, 128), dtype=torch.uint8, device=ctx.device)
        _WS["tab"] = {hd: ctx.rope_table(T_MAX, hd, THETA) for hd in E.HEAD_DIMS}
    return _WS["ws"], _WS["tab"]


def run_case(ctx, nh, nkv, hd, bound, pos, spoil_behind=False):
    c, q, kr, vr, wq, wk = base(nh, nkv, hd)
    kvd, rows = nkv * hd, bound + 2
    ws, tabs = scratch(ctx)
    host8 = [np.full((rows, kvd + PAD), FILL8, dtype=np.int8) for _ in range(2)]
    hosts = [np.full((rows, nkv), FILLS, dtype=np.float32) for _ in range(2)]
    for h8, hs, s8, ss in ((host8[0], hosts[0], c.k8, c.ks), (host8[1], hosts[1], c.v8, c.vs)):
        h8[:bound + 1, :kvd], hs[:bound + 1] = s8[:bound + 1], ss[:bound + 1]
        if spoil_behind:   # rows behind the position that would dominate if admitted: the largest codes, huge steps
            h8[pos + 1:bound + 1, :kvd], hs[pos + 1:bound + 1] = 127, np.float32(1e4)
        h8[pos, :kvd], hs[pos] = FILL8, FILLS   # the row the kernel must write
    k8, v8, ks, vs = dev(host8[0], ctx.device), dev(host8[1], ctx.device), dev(hosts[0], ctx.device), dev(hosts[1], ctx.device)
    dp = None if bound == pos else torch.tensor([pos], dtype=torch.int32, device=ctx.device)
    want_out, wk8, wks, wv8, wvs = reference(nh, nkv, hd, pos)
    host8[0][pos, :kvd], hosts[0][pos], host8[1][pos, :kvd], hosts[1][pos] = wk8, wks, wv8, wvs
    args = [bf16_t(a, ctx.device) for a in (q, kr, vr)]
    for call in range(2):   # twice on the scratch zeroed once: the second call attends the row the first one wrote
        out = ctx.attn_block_kv8(args[0], args[1], args[2], k8, v8, ks, vs, bf16_t(wq, ctx.device), bf16_t(wk, ctx.device), tabs[hd], bound, nh, nkv, hd, eps=EPS, d_pos=dp, ws=ws)
        got = u16(out)
        what = "%d / %d heads x %d, bound %d, pos %d, call %d" % (nh, nkv, hd, bound, pos, call)
        assert np.array_equal(got, want_out), "%s: %d outputs differ" % (what, int((got != want_out).sum()))
        for g, w, name in ((k8, host8[0], "K8"), (v8, host8[1], "V8")):
            g = g.cpu().numpy()
            assert np.array_equal(g[pos], w[pos]), "%s: the new %s row: %d codes differ" % (what, name, int((g[pos] != w[pos]).sum()))
            assert np.array_equal(g, w), "%s: %s outside the new row changed" % (what, name)
        for g, w, name in ((ks, hosts[0], "KS"), (vs, hosts[1], "VS")):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32)), "%s: %s" % (what, name)
        assert not ws[:16384].any(), "%s: arrival counters not back at zero" % what


@pytest.fixture
def both_orders(ctx):
    was = ctx.hip.kf_get_canonical(ctx.h)
    yield ctx.set_canonical
    ctx.set_canonical(was)


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_attn_block_kv8(ctx, both_orders, nh, nkv, hd):
    for canon in (1, 0):   # ONE arithmetic: the switch changes nothing
        both_orders(canon)
        for pos in POSITIONS:
            run_case(ctx, nh, nkv, hd, pos, pos)


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_position_below_the_bound(ctx, nh, nkv, hd):
    """launched for 300 with d_pos = 130: rows 131 .. 300 hold the largest codes and huge steps; they take no part, and only row 130 is written"""
    run_case(ctx, nh, nkv, hd, 300, 130, spoil_behind=True)


def test_refusals(ctx):
    d = ctx.device
    z8 = torch.zeros((4, 144), dtype=torch.int8, device=d)
    zs = torch.zeros((4, 2), dtype=torch.float32, device=d)
    x = torch.zeros(1024, dtype=torch.bfloat16, device=d)
    ws, tabs = scratch(ctx)
    from koifish_amd import lib as L
    for nh, nkv, hd in ((10, 2, 64), (4, 2, 96)):
        with pytest.raises(L.KFError, match="kf_attn_block_kv8"):
            ctx.attn_block_kv8(x, x, x, z8, z8, zs, zs, None, None, tabs[64], 0, nh, nkv, hd, ws=ws)
    odd = z8[:, :136].contiguous()   # rows 136 bytes apart
    with pytest.raises(L.KFError, match="multiple of 16"):
        ctx.attn_block_kv8(x, x, x, odd, odd, zs, zs, None, None, tabs[64], 0, 4, 2, 64, ws=ws)
