"""kf_attn_prefill_kv8 -- the prompt attention on the int8 KV cache -- on the GPU against the numpy restatement (tests/kv8_prefill_restate.py; include/kf_abi.h "int8 KV
cache, the prompt form").  Every output element is held to the DERIVED bound of tests/test_kv8_prefill_cpu.py (its docstring has the derivation; no element is exempt);
the row with one key, where nothing is summed, bit for bit.  What the definition states as exact is checked as exact: a row's bits do not depend on how the batch was
cut (split invariance), the two settings of kf_set_canonical give the same bits, the cache, the steps, the rows past n_tok and the padding between strided rows are not
written, and rows past a position take no part whatever they hold.  Every position has ONE q row and ONE reference per shape and kind of input, computed once."""
import numpy as np
import pytest
import torch

import exact_inputs as E
import kv8_prefill_restate as P
import kv8_restate as R
from conftest import bf16_t, u16
from koifish_amd import lib as L

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD, QPAD = 16, 8       # bytes behind every K8 / V8 row, elements behind every q / out row
FILL8, FILLS, FILLQ = 0x5B, np.float32(777.0), 0x3FC0
T_MAX = 336             # positions 0 .. 335: the last case ends at 330
CASES = [(0, 1), (0, 8), (0, 33), (0, 64), (0, 65), (0, 129), (1, 63), (63, 2), (64, 64), (100, 57), (300, 31)]
INVALID, UNALIGN = -20, -2000
_BASE = {}


def base(nh, nkv, hd, kind="normal"):
    """the cache, one prepared q row per position, and the restatement of every position (ref, tol, row 0's exact bits): once per shape and kind"""
    key = (nh, nkv, hd, kind)
    if key not in _BASE:
        rng = np.random.default_rng(nh * 1000 + nkv * 10 + hd)
        kvd, T = nkv * hd, T_MAX if kind == "normal" else 130
        k = (rng.standard_normal((T, kvd)) * rng.uniform(0.25, 4.0, (T, 1))).astype(F32)
        if kind == "flat":       # all keys equal: every score of a row is the same, the softmax is flat
            k[:] = k[0]
        if kind == "dominant":   # one key far ahead of the rest for every query: the q rows below point along it
            k[77] *= 6.0
        c = R.Cache8(T, nkv, hd)
        c.put(0, R.to_bf(k), R.to_bf(rng.standard_normal((T, kvd)).astype(F32)))
        q = (0.5 * rng.standard_normal((T, nh * hd))).astype(F32)
        if kind == "dominant":
            q = q + 0.5 * np.repeat(k[77].reshape(nkv, hd), nh // nkv, axis=0).reshape(-1)[None, :] / np.abs(k[77]).max()
        q = R.to_bf(q)
        ref, tol, exact = P.attn_prefill_kv8(q, c.k8, c.ks, c.v8, c.vs, 0, nh, nkv, hd)
        _BASE[key] = (c, q, ref, tol, exact)
    return _BASE[key]


def device_cache(ctx, c, rows, spoil_from=None):
    """the int8 pair as the library keeps it, rows kv_dim + PAD bytes apart; spoil_from: rows from there on hold the largest codes and huge steps"""
    kvd = c.k8.shape[1]
    h8 = [np.full((rows, kvd + PAD), FILL8, dtype=np.int8) for _ in range(2)]
    hs = [np.zeros((rows, c.n_kv), dtype=F32) for _ in range(2)]
    for a8, as_, s8, ss in ((h8[0], hs[0], c.k8, c.ks), (h8[1], hs[1], c.v8, c.vs)):
        a8[:, :kvd], as_[:] = s8[:rows], ss[:rows]
        if spoil_from is not None:
            a8[spoil_from:, :kvd], as_[spoil_from:] = 127, np.float32(1e4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    return h8, hs, [dev(a) for a in h8], [dev(a) for a in hs]


def launch(ctx, nh, nkv, hd, q, d8, ds, pos0, n):
    """rows pos0 .. pos0 + n - 1 of q as strided rows inside a pre-filled buffer -> the out buffer's bits [n + 2, nh * hd + QPAD]"""
    qd = nh * hd
    qbuf = np.full((n + 2, qd + QPAD), FILLQ, dtype=np.uint16)
    qbuf[:n, :qd] = q[pos0:pos0 + n]
    qt = bf16_t(qbuf, ctx.device)
    out = bf16_t(np.full((n + 2, qd + QPAD), FILLQ, dtype=np.uint16), ctx.device)
    ctx.attn_prefill_kv8(qt[:n, :qd], d8[0], d8[1], ds[0], ds[1], pos0, nh, nkv, hd, out=out[:n, :qd])
    return u16(out)


def held(got_u16, ref, tol, what):
    err = np.abs(R.bf(got_u16).astype(np.float64) - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print("%s: worst |error| / tol = %.3f" % (what, worst))
    assert (err <= tol).all(), "%s: %d elements outside the bound, worst %.3f x tol" % (what, int((err > tol).sum()), worst)


@pytest.fixture
def both_orders(ctx):
    was = ctx.hip.kf_get_canonical(ctx.h)
    yield ctx.set_canonical
    ctx.set_canonical(was)


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_against_the_restatement(ctx, both_orders, nh, nkv, hd):
    c, q, ref, tol, exact = base(nh, nkv, hd)
    qd = nh * hd
    h8, hs, d8, ds = device_cache(ctx, c, T_MAX)
    both_orders(1)
    for pos0, n in CASES:
        what = "%d / %d heads x %d, pos0 %d, n %d" % (nh, nkv, hd, pos0, n)
        got = launch(ctx, nh, nkv, hd, q, d8, ds, pos0, n)
        held(got[:n, :qd], ref[pos0:pos0 + n], tol[pos0:pos0 + n], what)
        assert (got[n:] == FILLQ).all() and (got[:, qd:] == FILLQ).all(), what + ": rows past n_tok or the row padding were written"
        if pos0 == 0:
            assert np.array_equal(got[0, :qd], exact), what + ": the one-key row: %d elements differ" % int((got[0, :qd] != exact).sum())
        # rows past the batch's last position hold the largest codes and huge steps: not one output bit moves
        _, _, s8, ss = device_cache(ctx, c, T_MAX, spoil_from=pos0 + n)
        assert np.array_equal(launch(ctx, nh, nkv, hd, q, s8, ss, pos0, n), got), what + ": rows past the position took part"
        if (pos0, n) in ((0, 33), (100, 57)):   # ONE arithmetic: the other setting of kf_set_canonical gives the same bits
            both_orders(0)
            assert np.array_equal(launch(ctx, nh, nkv, hd, q, d8, ds, pos0, n), got), what + ": kf_set_canonical changed the bits"
            both_orders(1)
    for g, w in zip(d8 + ds, h8 + hs):
        assert np.array_equal(g.cpu().numpy().view(np.uint8), w.view(np.uint8)), "the cache or its steps were written"


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_split_invariance(ctx, nh, nkv, hd):
    """a row's bits depend on its position, its q row and the cache -- not on pos0, n_tok or the rows beside it"""
    c, q, ref, tol, exact = base(nh, nkv, hd)
    qd = nh * hd
    _, _, d8, ds = device_cache(ctx, c, T_MAX)
    run = lambda pos0, n: launch(ctx, nh, nkv, hd, q, d8, ds, pos0, n)[:n, :qd]
    whole, part = run(0, 97), run(40, 57)
    assert np.array_equal(whole[40:97], part), "(0, 97) against (40, 57): %d elements differ" % int((whole[40:97] != part).sum())
    whole, last = run(0, 129), run(128, 1)
    assert np.array_equal(whole[128:129], last), "(0, 129) against (128, 1): %d elements differ" % int((whole[128:129] != last).sum())


@pytest.mark.parametrize("kind", ["flat", "dominant"])
@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_flat_and_peaked_softmax(ctx, nh, nkv, hd, kind):
    c, q, ref, tol, exact = base(nh, nkv, hd, kind)
    _, _, d8, ds = device_cache(ctx, c, 130)
    got = launch(ctx, nh, nkv, hd, q, d8, ds, 0, 129)
    held(got[:129, :nh * hd], ref[:129], tol[:129], "%s keys, %d / %d heads x %d" % (kind, nh, nkv, hd))
    assert np.array_equal(got[0, :nh * hd], exact)


def test_refusals(ctx):
    """every refusal returns its code, and kf_attn_prefill_kv8_status says the same without a launch"""
    d = ctx.device
    z8 = torch.zeros((8, 144), dtype=torch.int8, device=d)
    zs = torch.zeros((8, 2), dtype=torch.float32, device=d)
    x = torch.zeros((4, 1024 + 8), dtype=torch.bfloat16, device=d)
    y = torch.zeros_like(x)
    p = lambda t: None if t is None else t.data_ptr()

    def rc(nh, nkv, hd, pos0=0, n=4, q=x, k8=z8, v8=z8, ks=zs, vs=zs, out=y, q_stride=None, kv_stride=144):
        return ctx.hip.kf_attn_prefill_kv8(ctx.h, p(q), p(k8), p(v8), p(ks), p(vs), p(out), pos0, n, x.stride(0) if q_stride is None else q_stride, nh, nkv, hd, kv_stride)

    assert rc(4, 2, 64) == 0
    for name in ("q", "k8", "v8", "ks", "vs", "out"):
        assert rc(4, 2, 64, **{name: None}) == INVALID, name
    for nh, nkv, hd, n in ((10, 2, 64, 4), (4, 2, 96, 4), (4, 3, 64, 4), (4, 2, 64, 0)):
        assert rc(nh, nkv, hd, n=n) == INVALID and ctx.hip.kf_attn_prefill_kv8_status(nh, nkv, hd, n) == INVALID
    assert rc(4, 2, 64, pos0=-1) == INVALID
    assert rc(4, 2, 64, q_stride=128) == INVALID          # a row stride shorter than the row
    assert ctx.hip.kf_attn_prefill_kv8_status(4, 2, 64, 4) == 0
    assert rc(4, 2, 64, kv_stride=136) == UNALIGN         # rows 136 bytes apart
    assert rc(4, 2, 64, k8=z8.view(-1)[8:]) == UNALIGN    # the cache 8 bytes off
    assert rc(4, 2, 64, q=x.view(-1)[4:]) == UNALIGN      # q 8 bytes off
    assert rc(4, 2, 64, out=y.view(-1)[1:]) == UNALIGN    # out 2 bytes off
    assert rc(4, 2, 64, q_stride=1028) == UNALIGN
    with pytest.raises(L.KFError, match="kf_attn_prefill_kv8"):
        ctx.attn_prefill_kv8(x[:, :640], z8, z8, zs, zs, 0, 10, 2, 64)
