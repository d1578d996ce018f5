"""kf_evolve (kf_evo.hip) against its numpy restatement (tests/evo_restate.py), bit for bit, for the three algorithms; and kf_loss_mean.

Shapes: [1, 8] the smallest n the entry takes; [3, 40] under one wave's 512 elements; [64, 136] a ragged last workgroup (8704 = 4 workgroups of 2048 + 512);
[1600, 648] the issue's large shape -- which the launch geometry (256 threads x 8 bf16, at most 8 workgroups per CU) covers in ONE trip of the grid-stride loop on a
256-CU part (one trip takes 256 x 8 x 2048 = 4 194 304 elements), so the second trip is exercised by [n_cu x 8 x 256 + 1, 8]: the smallest multiple of 8 one trip of
the device at hand does not cover."""
import numpy as np
import pytest
import torch

import evo_restate as R
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu

ALGOS = ("pso", "pso_ga", "mix")
HP = dict(alpha=0.9, social=2.0, t_cross=0.6)
GUARD = 64


def _shapes():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return [(1, 8), (3, 40), (64, 136), (1600, 648), (n_cu * 8 * 256 + 1, 8)]


_PAIRS = {}


def _pair(shape):
    """N(0, 0.02) bf16 bit patterns, one row of x equal to the head's row (where there is more than one row); made once per shape and never modified"""
    if shape not in _PAIRS:
        rng = np.random.default_rng(shape[0] * 1009 + shape[1])
        x = R.rne_bf16(rng.normal(0, 0.02, shape).astype(np.float32))
        g = R.rne_bf16(rng.normal(0, 0.02, shape).astype(np.float32))
        if shape[0] > 1:
            x[shape[0] // 2] = g[shape[0] // 2]
        _PAIRS[shape] = (x, g)
    return _PAIRS[shape]


def _run(ctx, x, g, algo, seed):
    """x with GUARD elements of a pattern behind it -> (new x, guard, head after the call)"""
    n = x.size
    buf = torch.full((n + GUARD,), 1.5, dtype=torch.bfloat16, device=ctx.device)
    buf[:n] = bf16_t(x.reshape(-1), ctx.device)
    d_x, d_g = buf[:n].view(x.shape), bf16_t(g, ctx.device)
    ctx.evolve(d_x, d_g, algo, alpha=HP["alpha"], social=HP["social"], t_crossover=HP["t_cross"], seed=seed)
    ctx.sync()
    return u16(d_x), u16(buf[n:]), u16(d_g)


@pytest.mark.parametrize("shape_i", range(5))
def test_evolve_is_the_restatement(ctx, shape_i):
    shape = _shapes()[shape_i]
    x, g = _pair(shape)
    for algo in ALGOS:
        got, guard, g_after = _run(ctx, x, g, algo, seed=77 + shape_i)
        want = R.evolve(x, g, algo, seed=77 + shape_i, **HP)
        bad = int((got != want).sum())
        assert bad == 0, "%s %s: %d of %d elements differ from the restatement (first at %s)" % (algo, shape, bad, x.size, np.argwhere(got != want)[0])
        assert np.array_equal(g_after, g), "%s %s: head was modified" % (algo, shape)
        assert (guard == 0x3FC0).all(), "%s %s: elements behind x were written" % (algo, shape)
        assert not np.array_equal(got, x), "%s %s: nothing moved" % (algo, shape)
        if algo != "mix" and shape[0] > 1:   # d = 0: the row that equals the head's stays (mix rounds alpha x + beta x, which need not be x)
            assert np.array_equal(got[shape[0] // 2], g[shape[0] // 2])


def test_same_seed_same_bits(ctx):
    x, g = _pair((64, 136))
    a, _, _ = _run(ctx, x, g, "pso_ga", seed=5)
    b, _, _ = _run(ctx, x, g, "pso_ga", seed=5)
    c, _, _ = _run(ctx, x, g, "pso_ga", seed=6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_refusals_launch_nothing(ctx):
    hip = ctx.hip
    x, g = _pair((64, 136))
    d_x, d_g = bf16_t(x, ctx.device), bf16_t(g, ctx.device)
    px, pg = d_x.data_ptr(), d_g.data_ptr()
    ev = lambda x_, g_, ne0, ne1, algo=R.PSO_GA, alpha=0.9, social=2.0, tc=0.6: hip.kf_evolve(ctx.h, x_, g_, ne0, ne1, algo, alpha, social, tc, 3)
    cases = {
        "null x": ev(None, pg, 64, 136), "null head": ev(px, None, 64, 136),
        "x == head": ev(px, px, 64, 136), "overlap": ev(px, px + 16 * 136, 32, 136),
        "n < 8": ev(px, pg, 1, 4), "n % 8": ev(px, pg, 3, 35), "n >= 2^32": ev(px, pg, 65536, 65536), "ne0 < 1": ev(px, pg, 0, 136),
        "x unaligned": ev(px + 2, pg, 8, 8), "head unaligned": ev(px, pg + 2, 8, 8),
        "algorithm 0": ev(px, pg, 64, 136, algo=0), "algorithm 3 (mutation)": ev(px, pg, 64, 136, algo=3),
        "social nan": ev(px, pg, 64, 136, social=float("nan")), "alpha inf": ev(px, pg, 64, 136, alpha=float("inf")),
    }
    msgs = {}
    for k, rc in cases.items():
        assert rc == -20, "%s: returned %d" % (k, rc)
    for k, call in (("null", lambda: ev(None, pg, 64, 136)), ("overlap", lambda: ev(px, px + 16 * 136, 32, 136)), ("multiple of 8", lambda: ev(px, pg, 3, 35)),
                    ("aligned", lambda: ev(px + 2, pg, 8, 8)), ("algorithm", lambda: ev(px, pg, 64, 136, algo=3)), ("finite", lambda: ev(px, pg, 64, 136, social=float("inf")))):
        call()
        msgs[k] = hip.kf_last_error().decode()
        assert k in msgs[k], (k, msgs[k])
    with pytest.raises(ValueError):
        ctx.evolve(d_x, d_g, "mutation")
    ctx.sync()
    assert np.array_equal(u16(d_x), x) and np.array_equal(u16(d_g), g)


@pytest.mark.parametrize("n", [128, 130])
def test_loss_mean(ctx, n):
    rng = np.random.default_rng(n)
    a, b, c = (rng.uniform(0.5, 9.0, n).astype(np.float32) for _ in range(3))
    d = [torch.from_numpy(v).to(ctx.device) for v in (a, b, c)]
    got = ctx.loss_mean(d).cpu().numpy()
    want = ((a + b) + c) / np.float32(3.0)
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    one = ctx.loss_mean(d[:1]).cpu().numpy()
    assert np.array_equal(one.view(np.uint32), a.view(np.uint32))
    hip = ctx.hip
    assert hip.kf_loss_mean(ctx.h, d[0].data_ptr(), d[0].data_ptr(), n, 0, 1) == -20
    assert hip.kf_loss_mean(ctx.h, d[0].data_ptr(), d[1].data_ptr(), n, 2, 2) == -20
    assert hip.kf_loss_mean(ctx.h, d[0].data_ptr(), d[1].data_ptr(), 0, 0, 1) == -20
