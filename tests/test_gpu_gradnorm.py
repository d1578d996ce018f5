"""kf_grad_norms and kf_adamw_scaled on the device against tests/gradnorm_restate.py, bit for bit: one table of eight tensors inside ONE allocation filled with poison
(1e30 behind every buffer: an element read past n would show), sizes on both sides of the 4096-element chunk, two 8-element tensors back to back, pointers that are
16- but not 256-byte aligned; the three modes; the boundary of the comparison; non-finite sums as values; and the device-side scale against the by-value one."""
import ctypes as C

import numpy as np
import pytest
import torch

import gradnorm_restate as G
from koifish_amd import lib as L
from tests import exact_inputs as E
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu

SIZES = [8, 8, 4088, 4096, 4104, 3 * 4096 + 8, 1 << 20, 16]   # tensors 0 and 1 are adjacent; every other one is followed by 8 elements of poison
ZERO, GRID = 3, 4                                             # the all-zero tensor and the one on the exact grid
POISON = 0x7149                                               # 1e30 cut to bf16 (9.98e29)


def _values():
    rng = np.random.default_rng(2024)
    vals = []
    for i, n in enumerate(SIZES):
        if i == ZERO:
            vals.append(np.zeros(n, np.uint16))
        elif i == GRID:
            vals.append(E.exact_bits(E.small_ints(rng, n, 8)))
        else:
            vals.append(E.bits((rng.normal(0, 1, n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)))   # about 40 binades
    return vals


def _place(ctx, vals, gaps):
    """one allocation, poison everywhere, vals[i] at its offset (gaps[i] elements of poison behind it) -> (the allocation, one view per tensor)"""
    off, offs = 0, []
    for v, gp in zip(vals, gaps):
        offs.append(off)
        off += v.size + gp
    host = np.full(off + 8, POISON, np.uint16)
    for v, o in zip(vals, offs):
        host[o:o + v.size] = v
    buf = bf16_t(host, ctx.device)
    return buf, [buf[o:o + v.size] for v, o in zip(vals, offs)]


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32), np.asarray(b).view(np.uint64 if np.asarray(b).dtype == np.float64 else np.uint32))


@pytest.fixture(scope="module")
def table(ctx):
    vals = _values()
    buf, views = _place(ctx, vals, [0] + [8] * (len(vals) - 1))
    assert views[1].data_ptr() == views[0].data_ptr() + 16 and views[2].data_ptr() % 256 == 48 and all(v.data_ptr() % 16 == 0 for v in views)
    ss, gn = G.norms(vals)   # the reference, once
    assert float(E.f64(np.array([POISON], np.uint16))[0]) > 9e29
    return dict(vals=vals, buf=buf, views=views, ss=ss, gn=gn, plan=ctx.grad_norms_plan(views))


def _run(ctx, plan, mode, gclip):
    ss, gn, sc = ctx.grad_norms(plan, mode, gclip)
    ctx.sync()
    return ss.cpu().numpy(), gn.cpu().numpy(), sc.cpu().numpy()


def test_sums_and_norms_bit_for_bit(ctx, table):
    ss, gn, sc = _run(ctx, table["plan"], "report", 1.0)
    assert _same(ss, table["ss"]), (ss, table["ss"])
    assert _same(gn, table["gn"])
    assert ss[ZERO] == 0.0 and gn[ZERO] == 0.0 and ss[GRID] == np.sum(E.f64(table["vals"][GRID]) ** 2)
    assert ss[-1] < 1e29 and np.isfinite(ss).all()   # no poison counted
    assert _same(sc, np.ones(len(SIZES), np.float32))
    # the inputs are only read
    assert np.array_equal(u16(table["views"][6]), table["vals"][6])


def test_clip_modes_bit_for_bit(ctx, table):
    gn_ref = table["gn"]
    nz = np.sort(gn_ref[:-1][gn_ref[:-1] > 0])
    c = float(nz[len(nz) // 2])   # the median of the restated non-zero norms: tensors on both sides, and one AT the bound (not scaled: the comparison is >)
    want = G.scales(gn_ref, G.TENSOR, c)
    assert (want < 1).any() and (want == 1).sum() >= 2
    ss, gn, sc = _run(ctx, table["plan"], "tensor", c)
    assert _same(ss, table["ss"]) and _same(gn, gn_ref) and _same(sc, want), (sc, want)
    for c_g in (0.5 * float(gn_ref[-1]), 2.0 * float(gn_ref[-1])):   # the whole gradient clipped, and not
        want = G.scales(gn_ref, G.GLOBAL, c_g)
        assert (want < 1).all() == (c_g < gn_ref[-1])
        ss, gn, sc = _run(ctx, table["plan"], "global", c_g)
        assert _same(ss, table["ss"]) and _same(gn, gn_ref) and _same(sc, want)
    # a masked tensor keeps 1.0 and still counts in the total
    mask = [0] * len(SIZES)
    mask[6] = 1
    plan = ctx.grad_norms_plan(table["views"], no_clip=mask)
    for mode, m in (("tensor", G.TENSOR), ("global", G.GLOBAL)):
        cc = 0.25 * float(nz[0])   # below every non-zero norm
        want = G.scales(gn_ref, m, cc, no_clip=mask)
        assert want[6] == 1 and (want[[0, 1, 2, 4, 5, 7]] < 1).all()
        ss, gn, sc = _run(ctx, plan, mode, cc)
        assert _same(ss, table["ss"]) and _same(sc, want)


def test_boundary_and_non_finite_sums(ctx):
    """16 elements of 0.25: sumsq exactly 1.0, and with gclip 1.0 the scale is exactly 1.0f (> and not >=).  One +inf element: scale 0.0f; one NaN: 1.0f -- values"""
    quarter = E.exact_bits(np.full(16, 0.25))
    half = E.exact_bits(np.full(16, 0.5))
    inf = E.exact_bits(np.ones(8))
    inf[3] = 0x7F80
    nan = E.exact_bits(np.ones(8))
    nan[5] = 0x7FC0
    vals = [quarter, half, inf, nan]
    buf, views = _place(ctx, vals, [8] * 4)
    plan = ctx.grad_norms_plan(views)
    ss, gn, sc = _run(ctx, plan, "tensor", 1.0)
    assert ss[0] == 1.0 and gn[0] == 1.0 and sc[0] == 1.0
    assert ss[1] == 4.0 and gn[1] == 2.0 and sc[1] == 0.5
    assert np.isposinf(ss[2]) and np.isposinf(gn[2]) and sc[2] == 0.0 and not np.signbit(sc[2])
    assert np.isnan(ss[3]) and np.isnan(gn[3]) and sc[3] == 1.0
    assert np.isnan(ss[4]) and np.isnan(gn[4])
    want_ss, want_gn = G.norms(vals)
    assert _same(sc, G.scales(want_gn, G.TENSOR, 1.0)) and _same(ss[:3], want_ss[:3]) and _same(gn[:3], want_gn[:3])
    # the whole gradient: finite + inf = inf -> 0.0 for every tensor; with the NaN tensor in the list the total is NaN -> 1.0
    plan3 = ctx.grad_norms_plan(views[:3])
    ss, gn, sc = _run(ctx, plan3, "global", 1.0)
    assert np.isposinf(ss[3]) and (sc == 0.0).all()
    ss, gn, sc = _run(ctx, plan, "global", 1.0)
    assert np.isnan(gn[4]) and (sc == 1.0).all()


def test_unplanned_scratch_is_refused(ctx, table):
    plan = table["plan"]
    out = [plan["sumsq"].data_ptr(), plan["gnorm"].data_ptr(), plan["scale"].data_ptr()]
    # an address no plan was ever written to: 256 bytes into the live scratch (the allocator's blocks start on multiples of 512)
    assert ctx.hip.kf_grad_norms(ctx.h, C.c_void_p(plan["scratch"] + 256), plan["n"], G.REPORT, 1.0, *out) == -20
    assert b"kf_grad_norms_plan first" in ctx.hip.kf_last_error()
    assert ctx.hip.kf_grad_norms(ctx.h, C.c_void_p(plan["scratch"]), plan["n"] - 1, G.REPORT, 1.0, *out) == -20
    assert b"planned for" in ctx.hip.kf_last_error()


@pytest.mark.parametrize("mv", [L.BF16, L.F32], ids=["bf16_moments", "f32_moments"])
def test_adamw_scaled_is_adamw_with_the_same_float(ctx, mv):
    n = 4096 + 8
    rng = np.random.default_rng(77)
    dev = ctx.device
    p0 = E.bits(rng.normal(0, 0.1, n).astype(np.float32))
    g0 = E.bits(rng.normal(0, 0.02, n).astype(np.float32))
    mom = lambda a: bf16_t(E.bits(a.astype(np.float32)), dev) if mv == L.BF16 else torch.from_numpy(a.astype(np.float32)).to(dev)
    m0, v0 = rng.normal(0, 0.01, n), rng.normal(0, 0.01, n) ** 2
    scale = torch.tensor([0.0, 0.37], dtype=torch.float32, device=dev)   # read at d_scale + 1
    hp = (1e-2, 0.9, 0.95, 1.0 - 0.9 ** 3, 1.0 - 0.95 ** 3, 1e-8, 0.1)
    res = []
    for scaled in (False, True):
        p, g, m, v = bf16_t(p0, dev), bf16_t(g0, dev), mom(m0), mom(v0)
        if scaled:
            rc = ctx.hip.kf_adamw_scaled(ctx.h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, mv, *hp, scale.data_ptr() + 4, 4321, None)
        else:
            rc = ctx.hip.kf_adamw(ctx.h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, mv, *hp, 0.37, 4321, None)
        assert rc == 0, ctx.hip.kf_last_error()
        ctx.sync()
        res.append((u16(p), u16(g), m.cpu().view(torch.int16 if mv == L.BF16 else torch.int32).numpy(), v.cpu().view(torch.int16 if mv == L.BF16 else torch.int32).numpy()))
    a, b = res
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], p0) and not a[1].any()   # the parameters moved, the gradients were zeroed
    # and the scale matters: 1.0 gives other bits
    p, g, m, v = bf16_t(p0, dev), bf16_t(g0, dev), mom(m0), mom(v0)
    assert ctx.hip.kf_adamw(ctx.h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, mv, *hp, 1.0, 4321, None) == 0
    ctx.sync()
    assert not np.array_equal(u16(p), a[0])


def test_a_table_that_is_not_the_planned_one_is_not_followed(ctx):
    """the scratch's bytes overwritten since the plan (memory handed out again): the stamp in the sentinel row no longer matches the host's, so no pointer of the
    table is followed -- the partials stay as they were, sums and norms come back NaN, the scales 1.0"""
    vals = [E.exact_bits(np.full(16, 0.5)), E.exact_bits(np.full(4104, 1.0))]
    buf, views = _place(ctx, vals, [8, 8])
    plan = ctx.grad_norms_plan(views)
    ss, gn, sc = _run(ctx, plan, "tensor", 1.0)
    assert ss.tolist() == [4.0, 4104.0, 4108.0]
    off = plan["scratch"] - plan["ws"].data_ptr()
    tab_bytes, off_part = 24 * 3, (24 * 3 + 255) & ~255
    plan["ws"][off:off + tab_bytes] = 0                    # pointers, lengths, wg0 and the stamp: gone
    plan["ws"][off + off_part:off + off_part + 24] = 0x55  # the three partials
    for k in ("sumsq", "gnorm", "scale"):
        plan[k].fill_(7.0)
    ss, gn, sc = _run(ctx, plan, "tensor", 1.0)
    assert np.isnan(ss).all() and np.isnan(gn).all() and (sc == 1.0).all()
    assert (plan["ws"][off + off_part:off + off_part + 24].cpu().numpy() == 0x55).all()
    assert ctx.hip.kf_grad_norms_forget(ctx.h, C.c_void_p(plan["scratch"])) == 0
    out = [plan[k].data_ptr() for k in ("sumsq", "gnorm", "scale")]
    assert ctx.hip.kf_grad_norms(ctx.h, C.c_void_p(plan["scratch"]), 2, G.REPORT, 1.0, *out) == -20 and b"kf_grad_norms_plan first" in ctx.hip.kf_last_error()
