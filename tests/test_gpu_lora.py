"""kf_lora_forward / kf_lora_backward on the device (kf_lora.hip; the launches: kf_lora_plan.h).

Exact: on the integer operands of tests/lora_restate.py::lora_exact_case every partial sum of every kernel is an fp32 value in every order, so ax, y, adelta (read
from offset 0 of the scratch), delta and g equal the exact results BIT FOR BIT -- one tile of everything, three row tiles, column tails with an uneven slab cut at
rank 64 and s = 2, the k-loop depth of a 0.6B matrix, and a dense +-1 block of 128 token rows astride a slab seam taken from the plan.  No tolerance anywhere.
Random: normal operands against the numpy restatement, inside the bound derived in tests/lora_restate.py (never fitted to what the device returns).
Then: two calls give the same bits whatever the scratch held, and every refusal returns its code and touches nothing."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests import exact_inputs as E
from tests import lora_restate as R
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu


def _run(ctx, c, pattern=0xA5):
    """forward on y0, then backward on delta0 / g0, the scratch filled with a byte pattern first -> the bits of (ax, y, adelta, delta, g)"""
    dev, hip = ctx.device, ctx.hip
    OC, IC, n, r, s = c["OC"], c["IC"], c["n"], c["r"], c["s"]
    a, b, x, dIn = (bf16_t(c[k], dev) for k in ("a", "b", "x", "dIn"))
    y, delta, g = bf16_t(c["y0"], dev), bf16_t(c["delta0"], dev), bf16_t(c["g0"], dev)
    ax = torch.full((n, r), float("nan"), dtype=torch.bfloat16, device=dev)
    nb = hip.kf_lora_backward_scratch_bytes(r, OC, IC, n)
    scratch = torch.full((nb + 256,), pattern, dtype=torch.uint8, device=dev)
    off = ((scratch.data_ptr() + 255) & ~255) - scratch.data_ptr()
    assert hip.kf_lora_forward(ctx.h, a.data_ptr(), b.data_ptr(), r, OC, IC, x.data_ptr(), y.data_ptr(), ax.data_ptr(), n, s) == 0, hip.kf_last_error()
    assert hip.kf_lora_backward(ctx.h, a.data_ptr(), b.data_ptr(), r, OC, IC, dIn.data_ptr(), x.data_ptr(), ax.data_ptr(), delta.data_ptr(), g.data_ptr(), n, s,
                                scratch.data_ptr() + off) == 0, hip.kf_last_error()
    ctx.sync()
    adelta = scratch[off:off + n * r * 2].view(torch.bfloat16)   # the documented place: offset 0
    return u16(ax).reshape(-1), u16(y).reshape(-1), u16(adelta).reshape(-1), u16(delta).reshape(-1), u16(g).reshape(-1)


def _check_exact(ctx, c):
    runs = [_run(ctx, c, pattern) for pattern in (0xA5, 0xFF)]
    for got in runs:
        for name, bits in zip(("ax", "y", "adelta", "delta", "g"), got):
            want = c[name].reshape(-1)
            bad = np.flatnonzero(bits != want)
            assert not len(bad), "%s: %d of %d elements differ, first at %d: got %g, exact %g" % (name, len(bad), len(want), bad[0], E.f64(bits[bad[:1]])[0], E.f64(want[bad[:1]])[0])
    assert all(np.array_equal(p, q) for p, q in zip(*runs))


@pytest.mark.parametrize("shape", R.EXACT_SHAPES, ids=lambda s: "%dx%dx%d_r%d_s%d" % s)
def test_lora_exact(ctx, shape):
    _check_exact(ctx, R.exact_case(shape))


def test_lora_exact_block_astride_a_slab_seam(ctx):
    OC, IC, n, r, _ = R.BLOCK_SHAPE
    p = R.lora_plan(ctx.hip, r, OC, IC, n)
    assert p.SA >= 2 and p.SB >= 2 and R.slab_seams(p, n, "A")[0] == R.slab_seams(p, n, "B")[0]
    _check_exact(ctx, R.exact_case(R.BLOCK_SHAPE, block=True, hip=ctx.hip))


@pytest.mark.parametrize("shape", R.RANDOM_SHAPES, ids=lambda s: "%dx%dx%d_r%d" % s)
def test_lora_random_operands_within_the_derived_bound(ctx, shape):
    OC, IC, n, r = shape
    s = 0.5
    rng = np.random.default_rng(OC + r)
    bf = lambda v: O.f32_to_bf16(v.astype(np.float32))
    c = dict(OC=OC, IC=IC, n=n, r=r, s=s, a=bf(rng.normal(0, 0.1, (r, IC))), b=bf(rng.normal(0, 0.1, (OC, r))), x=bf(rng.normal(0, 1.0, (n, IC))),
             dIn=bf(rng.normal(0, 2.0 ** -6, (n, OC))), y0=bf(rng.normal(0, 1.0, (n, OC))), delta0=bf(rng.normal(0, 2.0 ** -4, (n, IC))), g0=bf(rng.normal(0, 0.1, r * (IC + OC))))
    f = {k: E.f64(c[k]) for k in ("a", "b", "x", "dIn", "y0", "delta0", "g0")}
    ax_r, _ = R.lora_forward(f["a"], f["b"], f["x"], f["y0"], s)                       # as stored: what the backward reads
    adelta_r, _, _ = R.lora_backward(f["a"], f["b"], f["dIn"], f["x"], ax_r, f["delta0"], f["g0"], s)
    ax, y = R.lora_forward(f["a"], f["b"], f["x"], f["y0"], s, store=False)           # every output before its own final store
    adelta, delta, g = R.lora_backward(f["a"], f["b"], f["dIn"], f["x"], ax_r, f["delta0"], f["g0"], s, store=False)
    mags = R.magnitudes(f["a"], f["b"], f["x"], f["y0"], f["dIn"], f["x"], ax_r, adelta_r, f["delta0"], f["g0"], s)
    gA0, gB0 = f["g0"][:r * IC].reshape(r, IC), f["g0"][r * IC:].reshape(OC, r)
    got = [E.f64(v) for v in _run(ctx, c)]
    refs = dict(ax=(ax, None, False), y=(y, f["y0"], True), adelta=(adelta, None, False), delta=(delta, f["delta0"], True))
    for (name, (ref, prior, second)), dev_v in zip(refs.items(), (got[0], got[1], got[2], got[3])):
        A, T = mags[name]
        err, bd = np.abs(dev_v.reshape(ref.shape) - ref), R.bound(ref, A, T, prior, second)
        print("%s: largest error / bound %.3f" % (name, float((err / bd).max())))
        assert (err <= bd).all(), (name, float((err / bd).max()))
    for name, ref, prior, dev_v in (("gA", g[:r * IC].reshape(r, IC), gA0, got[4][:r * IC]), ("gB", g[r * IC:].reshape(OC, r), gB0, got[4][r * IC:])):
        A, T = mags[name]
        err, bd = np.abs(dev_v.reshape(ref.shape) - ref), R.bound(ref, A, T, prior, True)
        print("%s: largest error / bound %.3f" % (name, float((err / bd).max())))
        assert (err <= bd).all(), (name, float((err / bd).max()))


def test_lora_wrappers(ctx):
    """Context.lora_forward / lora_backward: the same bits through the wrappers that own ax and the scratch"""
    c = R.exact_case(R.EXACT_SHAPES[1])
    dev = ctx.device
    a, b, x, dIn = (bf16_t(c[k], dev).view(sh) for k, sh in (("a", (c["r"], c["IC"])), ("b", (c["OC"], c["r"])), ("x", (c["n"], c["IC"])), ("dIn", (c["n"], c["OC"]))))
    y, delta, g = bf16_t(c["y0"], dev).view(c["n"], c["OC"]), bf16_t(c["delta0"], dev).view(c["n"], c["IC"]), bf16_t(c["g0"], dev)
    ax = ctx.lora_forward(a, b, x, y, c["s"])
    adelta = ctx.lora_backward(a, b, dIn, x, ax, delta, g, c["s"])
    ctx.sync()
    for name, t_ in (("ax", ax), ("y", y), ("adelta", adelta), ("delta", delta), ("g", g)):
        assert np.array_equal(u16(t_).reshape(-1), c[name].reshape(-1)), name
    with pytest.raises(L.KFError):
        ctx.lora_forward(a, b, x[:, :64], y, 1.0)


def test_lora_refusals_touch_nothing(ctx):
    hip, dev = ctx.hip, ctx.device
    c = R.exact_case(R.EXACT_SHAPES[0])
    OC, IC, n, r = c["OC"], c["IC"], c["n"], c["r"]
    big = lambda k, extra=0: torch.cat([bf16_t(c[k], dev).reshape(-1), torch.zeros(extra, dtype=torch.bfloat16, device=dev)])
    a, b, x, dIn = big("a", 8), big("b", 8), big("x", 8), big("dIn", 8)
    y, delta, g, ax = big("y0", 8), big("delta0", 8), big("g0", 8), torch.full((n * r + 8,), 3.0, dtype=torch.bfloat16, device=dev)
    nb = hip.kf_lora_backward_scratch_bytes(r, OC, IC, n)
    scratch = torch.full((nb + 512,), 0x5A, dtype=torch.uint8, device=dev)
    sp = (scratch.data_ptr() + 255) & ~255
    outs = (y, delta, g, ax, scratch)
    before = [t_.clone() for t_ in outs]
    P = lambda t_, off=0: t_.data_ptr() + off
    fwd = lambda a_=P(a), b_=P(b), r_=r, OC_=OC, IC_=IC, x_=P(x), y_=P(y), ax_=P(ax), n_=n, h=ctx.h: hip.kf_lora_forward(h, a_, b_, r_, OC_, IC_, x_, y_, ax_, n_, 1.0)
    bwd = lambda a_=P(a), b_=P(b), r_=r, OC_=OC, IC_=IC, d_=P(dIn), i_=P(x), ax_=P(ax), dl_=P(delta), g_=P(g), n_=n, sc_=sp, h=ctx.h: \
        hip.kf_lora_backward(h, a_, b_, r_, OC_, IC_, d_, i_, ax_, dl_, g_, n_, 1.0, sc_)
    INV, UNAL = -20, -2000   # KF_INVALID_ARGS, KF_BLAS_UNALIGN
    # other shapes, null pointers, no context: KF_INVALID_ARGS
    for kw in (dict(r_=8), dict(r_=24), dict(r_=128), dict(OC_=64), dict(IC_=192 + 32), dict(n_=96), dict(n_=0), dict(OC_=0), dict(h=None)):
        assert fwd(**kw) == INV and bwd(**kw) == INV, kw
    for k in ("a_", "b_", "x_", "y_", "ax_"):
        assert fwd(**{k: None}) == INV, k
    for k in ("a_", "b_", "d_", "i_", "ax_", "dl_", "g_", "sc_"):
        assert bwd(**{k: None}) == INV, k
    # misaligned operands (16 bytes) and scratch (256 bytes): KF_BLAS_UNALIGN
    codes = set()
    for k, t_ in (("a_", a), ("b_", b), ("x_", x), ("y_", y), ("ax_", ax)):
        codes.add(fwd(**{k: P(t_, 2)}))
    for k, t_ in (("a_", a), ("b_", b), ("d_", dIn), ("i_", x), ("ax_", ax), ("dl_", delta), ("g_", g)):
        codes.add(bwd(**{k: P(t_, 2)}))
    codes.add(bwd(sc_=sp + 16))
    assert codes == {UNAL}, codes
    assert b"aligned" in hip.kf_last_error()
    ctx.sync()
    for t_, t0 in zip(outs, before):
        assert torch.equal(t_.view(torch.uint8), t0.view(torch.uint8))
