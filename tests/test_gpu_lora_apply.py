"""kf_lora_apply on the device (kf_lora_apply.hip; the form and the launch: kf::lora_apply_plan).

Tile form (n >= 2): rows < n are BIT FOR BIT kf_lora_forward's on the same input zero-padded to 128 rows, for row counts below, at and above the 32-row tile and
the 64-row granule of the training entry; rows >= n of y and of ax keep a canary; ax = NULL gives the same y.
Vector form (n == 1): one adapter, one whose rows are no multiple of 128, and three adapters of different sizes in one launch with the third y inside a larger buffer;
BIT FOR BIT the numpy restatement (tests/lora_apply_restate.py) of the order include/kf_abi.h states on random operands, and exact on integer operands.
Across the forms: equal on integer operands; on random operands within the bound tests/lora_restate.py derives for its random-operand test (bound()).
Refusals return their code and touch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests import exact_inputs as E
from tests import lora_apply_restate as A
from tests import lora_restate as R
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128), (192, 576)]   # (OC, IC): two chunks of the contraction against eight waves / nine, so that wave 0 takes two; 192 = six 32-column blocks
ROWS = (2, 31, 33, 64, 70, 96)
VEC_GROUPS = [(128,), (192,), (256, 128, 128)]   # the adapters' rows per launch
CANARY = 0x7FC1                     # a NaN pattern no computation here produces
S = 0.5
bf = lambda v: O.f32_to_bf16(np.asarray(v, dtype=np.float32))


def _random(r, OC, IC, n, seed):
    rng = np.random.default_rng(seed)
    return dict(a=bf(rng.normal(0, 0.1, (r, IC))), b=bf(rng.normal(0, 0.1, (OC, r))), x=bf(rng.normal(0, 1.0, (n, IC))), y0=bf(rng.normal(0, 1.0, (n, OC))))


def _apply(ctx, a, b, x, y, ax, n, s, r, IC):
    """kf_lora_apply on lists of device tensors (one adapter per entry): the raw entry, so that sub-buffers and NULL can be passed"""
    n_w = len(a)
    ptrs = lambda ts: (C.c_void_p * n_w)(*[t if isinstance(t, int) else t.data_ptr() for t in ts])
    OC = (C.c_int * n_w)(*[t.shape[0] for t in b])
    return ctx.hip.kf_lora_apply(ctx.h, n_w, ptrs(a), ptrs(b), r, OC, IC, x.data_ptr(), ptrs(y), None if ax is None else ax.data_ptr(), n, s)


@pytest.mark.parametrize("OC,IC", SHAPES)
@pytest.mark.parametrize("r", R.RANKS)
def test_tile_form_rows_are_kf_lora_forwards(ctx, r, OC, IC):
    dev, hip = ctx.device, ctx.hip
    c = _random(r, OC, IC, 128, seed=r + OC)
    a, b = bf16_t(c["a"], dev), bf16_t(c["b"], dev)
    for n in ROWS:
        xp, yp = c["x"].copy(), c["y0"].copy()
        xp[n:] = 0   # the training entry on the input zero-padded to 128 rows
        x_ref, y_ref, ax_ref = bf16_t(xp, dev), bf16_t(yp, dev), torch.zeros(128, r, dtype=torch.bfloat16, device=dev)
        assert hip.kf_lora_forward(ctx.h, a.data_ptr(), b.data_ptr(), r, OC, IC, x_ref.data_ptr(), y_ref.data_ptr(), ax_ref.data_ptr(), 128, S) == 0, hip.kf_last_error()
        x = bf16_t(c["x"], dev)   # ALL 128 rows hold data: a row >= n that is read would show
        got = []
        for keep in (True, False):
            yb, axb = c["y0"].copy(), np.full((128, r), CANARY, dtype=np.uint16)
            yb[n:] = CANARY
            y, ax = bf16_t(yb, dev), bf16_t(axb, dev)
            assert _apply(ctx, [a], [b], x, [y], ax if keep else None, n, S, r, IC) == 0, hip.kf_last_error()
            ctx.sync()
            yg, axg = u16(y), u16(ax)
            assert np.array_equal(yg[:n], u16(y_ref)[:n]), "n %d: y rows differ from kf_lora_forward's" % n
            assert (yg[n:] == CANARY).all(), "n %d: a y row >= n was written" % n
            assert (axg[n:] == CANARY).all(), "n %d: an ax row >= n was written" % n
            if keep:
                assert np.array_equal(axg[:n], u16(ax_ref)[:n]), "n %d: ax rows differ" % n
            else:
                assert (axg == CANARY).all()
            got.append(yg)
        assert np.array_equal(got[0], got[1]), "n %d: ax = NULL changes y" % n


def _launch_group(ctx, r, IC, x_bits, group, s):
    """one vector-form launch for the adapters [(a, b, y0)] (bf16 bits); the LAST y lies at element offset 64 of a buffer with 64 canary elements on either side"""
    dev = ctx.device
    a, b = [bf16_t(g[0], dev) for g in group], [bf16_t(g[1], dev) for g in group]
    ys = [bf16_t(g[2], dev) for g in group[:-1]]
    OCl = len(group[-1][2])
    big = np.full(OCl + 128, CANARY, dtype=np.uint16)
    big[64:64 + OCl] = group[-1][2]
    bigt = bf16_t(big, dev)
    x = bf16_t(x_bits, dev)
    assert _apply(ctx, a, b, x, ys + [bigt.data_ptr() + 128], None, 1, s, r, IC) == 0, ctx.hip.kf_last_error()
    ctx.sync()
    out = u16(bigt)
    assert (out[:64] == CANARY).all() and (out[64 + OCl:] == CANARY).all(), "bytes around the last y changed"
    return [u16(y) for y in ys] + [out[64:64 + OCl]]


@pytest.mark.parametrize("IC", [128, 576])
@pytest.mark.parametrize("r", R.RANKS)
def test_vector_form_bits_of_the_stated_order(ctx, r, IC):
    for OCs in VEC_GROUPS:
        rng = np.random.default_rng(r + IC + len(OCs))
        x = bf(rng.normal(0, 1.0, IC))
        group = [(bf(rng.normal(0, 0.1, (r, IC))), bf(rng.normal(0, 0.1, (OC, r))), bf(rng.normal(0, 1.0, OC))) for OC in OCs]
        for (a, b, y0), got in zip(group, _launch_group(ctx, r, IC, x, group, S)):
            want = A.vec_apply_bits(a, b, x, y0, S)
            bad = np.flatnonzero(got != want)
            assert not len(bad), "random, OCs %s: %d of %d outputs differ from the restatement, first at %d" % (OCs, len(bad), len(want), bad[0])
        xe, ge = A.exact_group(r, IC, OCs, seed=r + IC)
        for (_, _, _, want), got in zip(ge, _launch_group(ctx, r, IC, xe, [g[:3] for g in ge], 1.0)):
            assert np.array_equal(got, want), "integer operands, OCs %s" % (OCs,)


@pytest.mark.parametrize("OC,IC", SHAPES)
@pytest.mark.parametrize("r", R.RANKS)
def test_the_two_forms_agree(ctx, r, OC, IC):
    """the same row through both forms (the tile form sees it as row 0 of two): equal on integer operands; on random operands the forms sum in different orders and may
    differ by what tests/lora_restate.py allows a device output against the restated value before its store (bound(), second product included)"""
    dev = ctx.device

    def both(a, b, x_row, y_row, s):
        at, bt = bf16_t(a, dev), bf16_t(b, dev)
        vec = _launch_group(ctx, r, IC, x_row, [(a, b, y_row)], s)[0]
        x2, y2 = bf16_t(np.stack([x_row, x_row]), dev), bf16_t(np.stack([y_row, y_row]), dev)
        assert _apply(ctx, [at], [bt], x2, [y2], None, 2, s, r, IC) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        tile = u16(y2)
        assert np.array_equal(tile[0], tile[1])
        return vec, tile[0]
    xe, ge = A.exact_group(r, IC, (OC,), seed=r + IC + OC)
    vec, tile = both(ge[0][0], ge[0][1], xe, ge[0][2], 1.0)
    assert np.array_equal(vec, ge[0][3]) and np.array_equal(tile, ge[0][3])
    c = _random(r, OC, IC, 1, seed=3 * r + OC)
    vec, tile = both(c["a"], c["b"], c["x"][0], c["y0"][0], S)
    f = {k: E.f64(c[k]) for k in ("a", "b", "x", "y0")}
    ax_r, _ = R.lora_forward(f["a"], f["b"], f["x"], f["y0"], S)
    _, y = R.lora_forward(f["a"], f["b"], f["x"], f["y0"], S, store=False)
    Amag = np.abs(f["y0"]) + S * (np.abs(ax_r) @ np.abs(f["b"]).T)
    bd = R.bound(y, Amag, r, f["y0"], True)[0]
    diff = np.abs(E.f64(vec) - E.f64(tile))
    print("r %d, %d x %d: largest difference between the forms / bound %.3f; %d of %d outputs differ" % (r, OC, IC, float((diff / bd).max()), int((vec != tile).sum()), OC))
    assert (diff <= bd).all(), float((diff / bd).max())
    for name, got in (("vector", vec), ("tile", tile)):   # and each form against the restated value, as tests/test_gpu_lora.py holds kf_lora_forward
        assert (np.abs(E.f64(got) - y[0]) <= bd).all(), name


def test_wrapper(ctx):
    """Context.lora_apply: the same bits through the wrapper, one adapter and three"""
    dev, r, IC = ctx.device, 16, 128
    xe, ge = A.exact_group(r, IC, (256, 128, 128), seed=9)
    a, b, y = ([bf16_t(g[k], dev) for g in ge] for k in range(3))
    assert ctx.lora_apply(a, b, bf16_t(xe, dev), y, 1.0) is None
    ctx.sync()
    assert all(np.array_equal(u16(yt), g[3]) for yt, g in zip(y, ge))
    c = R.exact_case(R.EXACT_SHAPES[0], hip=ctx.hip)
    n = 33
    yt = bf16_t(c["y0"][:n], dev)
    ax = ctx.lora_apply(bf16_t(c["a"], dev), bf16_t(c["b"], dev), bf16_t(c["x"][:n], dev), yt, c["s"], keep_ax=True)
    ctx.sync()
    assert np.array_equal(u16(yt), c["y"][:n]) and np.array_equal(u16(ax), c["ax"][:n])
    with pytest.raises(L.KFError):
        ctx.lora_apply(a[0], b[1], bf16_t(xe, dev), y[0], 1.0)


def test_refusals_touch_nothing(ctx):
    dev, hip, r, OC, IC = ctx.device, ctx.hip, 16, 128, 128
    c = _random(r, OC, IC, 8, seed=1)
    pad = lambda bits: torch.cat([bf16_t(bits, dev).reshape(-1), torch.zeros(8, dtype=torch.bfloat16, device=dev)])
    a, b, x, y, ax = pad(c["a"]), pad(c["b"]), pad(c["x"]), pad(c["y0"]), torch.full((8 * r + 8,), 3.0, dtype=torch.bfloat16, device=dev)
    before = [t.clone() for t in (y, ax)]
    P = lambda t, off=0: t.data_ptr() + off
    arr = lambda *v: (C.c_void_p * len(v))(*v)

    def call(a_=P(a), b_=P(b), r_=r, OC_=(OC,), IC_=IC, x_=P(x), y_=P(y), ax_=P(ax), n_=8, h=ctx.h, n_w=1):
        k = max(n_w, 1)
        return hip.kf_lora_apply(h, n_w, arr(*([a_] * k)), arr(*([b_] * k)), r_, (C.c_int * k)(*(list(OC_) * k)[:k]), IC_, x_, arr(*([y_] * k)), ax_, n_, 1.0)
    INV, UNAL = -20, -2000   # KF_INVALID_ARGS, KF_BLAS_UNALIGN
    for kw in (dict(r_=8), dict(r_=24), dict(r_=128), dict(OC_=(96,)), dict(OC_=(64,)), dict(IC_=160), dict(IC_=64), dict(n_=0), dict(n_=-3), dict(n_w=2), dict(n_w=4, n_=1),
               dict(n_w=0), dict(h=None), dict(a_=None), dict(b_=None), dict(x_=None), dict(y_=None)):
        assert call(**kw) == INV, kw
    assert hip.kf_lora_apply(ctx.h, 1, None, arr(P(b)), r, (C.c_int * 1)(OC), IC, P(x), arr(P(y)), None, 8, 1.0) == INV
    for kw in (dict(a_=P(a, 2)), dict(b_=P(b, 2)), dict(x_=P(x, 2)), dict(y_=P(y, 2)), dict(ax_=P(ax, 2)), dict(y_=P(y, 2), n_=1)):
        assert call(**kw) == UNAL, kw
    assert b"16-byte" in hip.kf_last_error()
    ctx.sync()
    assert all(torch.equal(t, t0) for t, t0 in zip((y, ax), before)), "a refused call wrote something"
    assert call() == 0 and call(n_=1, ax_=None) == 0   # the same arguments, served
    ctx.sync()
    assert not torch.equal(y, before[0])
