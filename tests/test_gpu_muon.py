"""The Muon entries (kf_muon_momentum, kf_newton_schulz, kf_muon_apply, kf_muon: PIPE_Muon::CU_core, Optimizer.cu:498-583) against the restatement of
tests/muon_restate.py: the two elementwise kernels bit for bit, the Newton-Schulz iteration against torch on the CPU within a bound taken from the restatement's own
two summation orders, the symmetric products symmetric bit for bit."""
import functools

import numpy as np
import pytest
import torch

import muon_restate as R

pytestmark = pytest.mark.gpu

INVALID = -20
SHAPES = [(64, 64), (320, 192), (640, 256), (384, 384)]
RECT = [(320, 192), (640, 256)]
EPS = 1e-7


def _dev(a_u16, ctx):
    return torch.from_numpy(np.ascontiguousarray(a_u16).view(np.int16).copy()).to(ctx.device)


def _back(t):
    return t.cpu().numpy().view(np.uint16)


def _bf(rng, n, std):
    return R.rne_bf16(rng.normal(0, std, n).astype(np.float32))


class Scratch:
    """kf_muon_scratch_bytes(ne0, ne1) of device memory, 256-byte aligned, and views of the regions include/kf_abi.h documents"""

    def __init__(self, ctx, ne0, ne1, short=0):
        self.ne0, self.ne1 = ne0, ne1
        self.bytes = ctx.hip.kf_muon_scratch_bytes(ne0, ne1)
        assert self.bytes > 0 and self.bytes % 256 == 0
        self.t = torch.zeros(self.bytes + 256, dtype=torch.uint8, device=ctx.device)
        self.off = (-self.t.data_ptr()) % 256
        self.ptr = self.t.data_ptr() + self.off
        self.bytes -= short

    def _u16(self, byte_off, count):
        return self.t[self.off + byte_off: self.off + byte_off + 2 * count].cpu().numpy().view(np.uint16)

    def A(self):
        return self._u16(0, self.ne1 * self.ne1).reshape(self.ne1, self.ne1)

    def B(self):
        up = (2 * self.ne1 * self.ne1 + 255) & ~255
        return self._u16(up, self.ne1 * self.ne1).reshape(self.ne1, self.ne1)

    def doubles(self):
        b = self.off + self.bytes - 256
        return self.t[b: b + 16].cpu().numpy().view(np.float64)


@pytest.mark.parametrize("n", [8 * 512 * 3, 8 * (512 * 2 + 5)])
def test_momentum_and_apply_bit_for_bit(ctx, n):
    """two consecutive calls with different seeds (the second starts from stochastically rounded state): mG, X, p and the zeroed gradient equal the numpy restatement
    bit for bit; the two device sums equal the fp64 sum of the device's own values to the round-off of a differently ordered fp64 sum (every term is an exact product
    of bf16 values: relative 1e-12)."""
    rng = np.random.default_rng(n)
    mG, p = _bf(rng, n, 0.01), _bf(rng, n, 0.05)
    d_mG, d_p = _dev(mG, ctx), _dev(p, ctx)
    d_X = torch.zeros(n, dtype=torch.int16, device=ctx.device)
    d_ss = torch.zeros(2, dtype=torch.float64, device=ctx.device)
    mui, lr, wd = 0.95, 0.015, 0.002
    for step, seed in enumerate((4242, 977)):
        g = _bf(rng, n, 0.02)
        d_g = _dev(g, ctx)
        assert ctx.hip.kf_muon_momentum(ctx.h, d_mG.data_ptr(), d_g.data_ptr(), d_X.data_ptr(), n, mui, seed, d_ss.data_ptr()) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        mG, x = R.momentum(mG, g, mui, seed)
        assert np.array_equal(_back(d_mG), mG), "mG differs at step %d" % step
        assert np.array_equal(_back(d_X), x), "X differs at step %d" % step
        assert np.array_equal(_back(d_g), g)
        ss = float(d_ss[0].item())
        assert ss > 0 and abs(ss - R.sumsq(_back(d_X))) <= 1e-12 * ss
        # apply, with the device's X
        assert ctx.hip.kf_muon_apply(ctx.h, d_p.data_ptr(), d_g.data_ptr(), d_X.data_ptr(), n, lr, wd, seed, d_ss.data_ptr() + 8) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        p = R.apply(p, _back(d_X), lr, wd, seed)
        assert np.array_equal(_back(d_p), p), "params differ at step %d" % step
        assert not _back(d_g).any()
        wn = float(d_ss[1].item())
        assert wn > 0 and abs(wn - R.sumsq(_back(d_p))) <= 1e-12 * wn
    # no destination for wnorm^2: the update is the same, nothing else is written
    g = _bf(rng, n, 0.02)
    d_g = _dev(g, ctx)
    assert ctx.hip.kf_muon_apply(ctx.h, d_p.data_ptr(), d_g.data_ptr(), d_X.data_ptr(), n, lr, wd, 5, None) == 0
    ctx.sync()
    assert np.array_equal(_back(d_p), R.apply(p, _back(d_X), lr, wd, 5)) and float(d_ss[1].item()) == wn


def _input(shape):
    g = torch.Generator()
    g.manual_seed(1000 * shape[0] + shape[1])
    return (0.02 * torch.randn(shape[0], shape[1], generator=g)).to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)


@functools.lru_cache(maxsize=None)
def _restated(shape):
    """(R64, d0): the fp64-product restatement and its distance from the fp32-product one -- two legitimate summation orders of the same arithmetic"""
    x = _input(shape)
    r32 = R.newton_schulz(x, shape[0], shape[1], EPS, 5, torch.float32)[0]
    r64 = R.newton_schulz(x, shape[0], shape[1], EPS, 5, torch.float64)[0]
    return r64, float(torch.linalg.norm(r32 - r64) / torch.linalg.norm(r64))


def _ns(ctx, x_u16, shape, n_iter, sc, d_sumsq=None):
    d_x = _dev(x_u16, ctx)
    rc = ctx.hip.kf_newton_schulz(ctx.h, d_x.data_ptr(), shape[0], shape[1], d_sumsq, EPS, n_iter, R.A_, R.B_, R.C_, sc.ptr, sc.bytes)
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    return _back(d_x)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_newton_schulz_against_the_restatement(ctx, shape):
    """Five iterations against torch on the CPU with bf16 stores at the device's rounding points.  The bound is not a constant: d0 = |R32 - R64| / |R64| (Frobenius) is
    the distance between the restatement summed in fp32 and in fp64, one sample of how far bf16 store flips compounded over five iterations carry two legitimate
    summation orders apart; the device must lie within 4 x max(d0, d0 of 320 x 192) of R64 (a wrong tile, a missed k-step or a wrong coefficient is an O(1) error).
    Without a tolerance: A and B after one iteration are symmetric bit for bit; every singular value of the rectangular results lies in [0.6, 1.25]; n_iter = 0
    returns bf16(X + (alpha - 1) X) bit for bit; the entry is deterministic."""
    ne0, ne1 = shape
    x = _input(shape)
    sc = Scratch(ctx, ne0, ne1)
    r64, d0 = _restated(shape)
    bound = 4.0 * max(d0, _restated((320, 192))[1])
    dev = _ns(ctx, x, shape, 5, sc)
    devf = torch.from_numpy(R.f32(dev).astype(np.float64).reshape(ne0, ne1))
    ratio = float(torch.linalg.norm(devf - r64) / torch.linalg.norm(r64))
    print("newton_schulz %dx%d: |dev - R64| / |R64| = %.5f, d0 = %.5f, bound = %.5f" % (ne0, ne1, ratio, d0, bound))
    assert ratio <= bound
    assert np.array_equal(_ns(ctx, x, shape, 5, sc), dev), "two runs on the same input differ"
    if shape in RECT:
        for name, m in (("R64", r64), ("device", devf)):
            sv = torch.linalg.svdvals(m)
            print("  singular values of %s: [%.3f, %.3f]" % (name, float(sv.min()), float(sv.max())))
            assert 0.6 <= float(sv.min()) and float(sv.max()) <= 1.25, name
    # one iteration: the symmetric products as the scratch layout of include/kf_abi.h holds them
    _ns(ctx, x, shape, 1, sc)
    A, B = sc.A(), sc.B()
    assert A.any() and B.any()
    assert np.array_equal(A, A.T), "A = bf16(X^T X) is not symmetric bit for bit"
    assert np.array_equal(B, B.T), "B = bf16(b A + bf16(c A A)) is not symmetric bit for bit"
    x0 = R.prescale(x, R.sumsq(x), EPS)
    a_ref = R.newton_schulz(x, ne0, ne1, EPS, 1, torch.float64)[1].numpy()
    assert np.abs(R.f32(A).astype(np.float64) - a_ref).max() <= 2.0 ** -7 * np.abs(a_ref).max(), "A is not X^T X"   # one bf16 store of an fp32 sum: half an ulp of the largest entry, twice over
    # no iteration: the pre-scale alone, from the device's own sum (left in the scratch) and from a sum the caller hands in
    got = _ns(ctx, x, shape, 0, sc)
    ss = float(sc.doubles()[0])
    assert abs(ss - R.sumsq(x)) <= 1e-12 * ss
    assert np.array_equal(got, R.prescale(x, ss, EPS))
    d_ss = torch.tensor([R.sumsq(x)], dtype=torch.float64, device=ctx.device)
    assert np.array_equal(_ns(ctx, x, shape, 0, sc, d_ss.data_ptr()), x0)


def test_muon_is_the_three_entries_in_sequence(ctx):
    ne0, ne1 = 320, 192
    n = ne0 * ne1
    rng = np.random.default_rng(5)
    p, g, mG = _bf(rng, n, 0.05), _bf(rng, n, 0.02), _bf(rng, n, 0.01)
    mui, lr, wd, seed = 0.95, 0.015, 0.002, 31337
    sc1, sc2 = Scratch(ctx, ne0, ne1), Scratch(ctx, ne0, ne1)
    p1, g1, m1 = _dev(p, ctx), _dev(g, ctx), _dev(mG, ctx)
    w1 = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    assert ctx.hip.kf_muon(ctx.h, p1.data_ptr(), g1.data_ptr(), m1.data_ptr(), ne0, ne1, lr, wd, mui, EPS, 5, seed, sc1.ptr, sc1.bytes, w1.data_ptr()) == 0, ctx.hip.kf_last_error()
    p2, g2, m2 = _dev(p, ctx), _dev(g, ctx), _dev(mG, ctx)
    X = torch.zeros(n, dtype=torch.int16, device=ctx.device)
    d = torch.zeros(2, dtype=torch.float64, device=ctx.device)
    assert ctx.hip.kf_muon_momentum(ctx.h, m2.data_ptr(), g2.data_ptr(), X.data_ptr(), n, mui, seed, d.data_ptr()) == 0
    assert ctx.hip.kf_newton_schulz(ctx.h, X.data_ptr(), ne0, ne1, d.data_ptr(), EPS, 5, R.A_, R.B_, R.C_, sc2.ptr, sc2.bytes) == 0
    assert ctx.hip.kf_muon_apply(ctx.h, p2.data_ptr(), g2.data_ptr(), X.data_ptr(), n, lr, wd, seed, d.data_ptr() + 8) == 0
    ctx.sync()
    assert not np.array_equal(_back(p1), p), "the parameters did not move"
    assert np.array_equal(_back(p1), _back(p2)) and np.array_equal(_back(m1), _back(m2))
    assert not _back(g1).any() and not _back(g2).any()
    assert float(w1.item()) == float(d[1].item()) > 0
    assert np.array_equal(sc1.A(), sc2.A()) and np.array_equal(sc1.B(), sc2.B())


def test_refusals(ctx):
    """each returns KF_INVALID_ARGS, launches nothing and changes no buffer"""
    hip = ctx.hip
    ne0, ne1 = 128, 64
    n = ne0 * ne1
    rng = np.random.default_rng(9)
    x = _bf(rng, n + 8, 0.02)
    d_x, d_g, d_m = _dev(x, ctx), _dev(x, ctx), _dev(x, ctx)
    sc = Scratch(ctx, ne0, ne1)
    sc.t.fill_(7)
    ns = lambda xp, a, b, it, sp, sb: hip.kf_newton_schulz(ctx.h, xp, a, b, None, EPS, it, R.A_, R.B_, R.C_, sp, sb)
    mu = lambda pp, a, b, it, sp, sb: hip.kf_muon(ctx.h, pp, d_g.data_ptr(), d_m.data_ptr(), a, b, 0.01, 0.0, 0.95, EPS, it, 1, sp, sb, None)
    for f in (ns, mu):
        assert f(d_x.data_ptr(), ne1, ne0, 5, sc.ptr, sc.bytes) == INVALID          # ne0 < ne1
        assert f(d_x.data_ptr(), 96, 64, 5, sc.ptr, sc.bytes) == INVALID            # a dimension of 96
        assert f(d_x.data_ptr(), 128, 96, 5, sc.ptr, sc.bytes) == INVALID
        assert f(d_x.data_ptr(), ne0, ne1, 5, sc.ptr, sc.bytes - 1) == INVALID      # a scratch one byte short
        assert f(d_x.data_ptr(), ne0, ne1, 5, None, sc.bytes) == INVALID            # no scratch
        assert f(d_x.data_ptr() + 2, ne0, ne1, 5, sc.ptr, sc.bytes) == INVALID      # a misaligned tensor
        assert f(d_x.data_ptr(), ne0, ne1, 5, sc.ptr + 16, sc.bytes) == INVALID     # a misaligned scratch
        assert f(d_x.data_ptr(), ne0, ne1, 17, sc.ptr, sc.bytes) == INVALID and f(d_x.data_ptr(), ne0, ne1, -1, sc.ptr, sc.bytes) == INVALID
        assert b"kf_" in hip.kf_last_error()
    assert hip.kf_muon_scratch_bytes(ne1, ne0) == 0 and hip.kf_muon_scratch_bytes(96, 64) == 0
    d = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    assert hip.kf_muon_momentum(ctx.h, d_m.data_ptr() + 2, d_g.data_ptr(), d_x.data_ptr(), n, 0.95, 1, d.data_ptr()) == INVALID
    assert hip.kf_muon_momentum(ctx.h, d_m.data_ptr(), d_g.data_ptr(), d_x.data_ptr(), n + 4, 0.95, 1, d.data_ptr()) == INVALID
    assert hip.kf_muon_apply(ctx.h, d_x.data_ptr(), d_g.data_ptr() + 2, d_m.data_ptr(), n, 0.01, 0.0, 1, None) == INVALID
    ctx.sync()
    for t in (d_x, d_g, d_m):
        assert np.array_equal(_back(t), x)
    assert bool((sc.t == 7).all()) and float(d.item()) == 0.0
