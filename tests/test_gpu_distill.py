"""kf_distill_classifier through the C ABI: bit for bit against the numpy restatement of its stated order (tests/distill_restate.py, itself pinned to float64 and to
the oracle's fused classifier by tests/test_distill_cpu.py) on the fused classifier test's own shapes; the pure-CE weighting against the oracle's fused classifier;
the mask, the loss-only mode, unread targets, every refusal; and one full-size case (8 x 1024 rows of the Qwen3 vocabulary: the smallest shape at which a 32-bit row
offset goes wrong) against float64 with the bars derived in tests/test_distill_cpu.py."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import distill_cases as DC
from tests import distill_restate as R
from tests.conftest import bf16_t, u16
from tests.test_distill_cpu import _check_against_fp64

pytestmark = pytest.mark.gpu
INVALID_ARGS, UNALIGN = -20, -2000


def _run(ctx, logits, teacher, ld, losses, kd, dloss, targets, B, T, V, P, mask, a, b, tau, write=1):
    p = lambda t: None if t is None else t.data_ptr()
    return ctx.hip.kf_distill_classifier(ctx.h, p(logits), p(teacher), ld, p(losses), p(kd), dloss, p(targets), B, T, V, P, p(mask), a, b, tau, write)


@pytest.mark.parametrize("weights", DC.WEIGHTS, ids=lambda w: "a%g-b%g-t%g" % w)
@pytest.mark.parametrize("teacher", DC.TEACHERS)
@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distill_classifier_bit_exact(ctx, shape, teacher, weights):
    rows, V, P = shape
    logits, teach, targets = DC.inputs(rows, V, P, teacher)
    want_l, want_kd, want_g = DC.restated(rows, V, P, teacher, weights)
    zd, ud, td = bf16_t(logits.copy(), ctx.device), bf16_t(teach.copy(), ctx.device), torch.from_numpy(targets.copy()).to(ctx.device)
    losses = torch.full((rows,), DC.LOSS_FILL, dtype=torch.float32, device=ctx.device)
    kd = torch.full((rows,), -7.0, dtype=torch.float32, device=ctx.device)   # written, not accumulated
    a, b, tau = weights
    assert _run(ctx, zd, ud, teach.shape[1], losses, kd, DC.dloss_of(rows), td, rows, 1, V, P, None, a, b, tau) == 0
    ctx.sync()
    got_l, got_kd, got_g = losses.cpu().numpy(), kd.cpu().numpy(), u16(zd)
    print("kd rows:", got_kd[:4], "restated:", want_kd[:4])
    assert np.array_equal(got_kd.view(np.uint32), want_kd.view(np.uint32))
    assert np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32))
    assert np.array_equal(got_g[:, :V], want_g[:, :V]), "%d gradient elements differ" % (got_g[:, :V] != want_g[:, :V]).sum()
    assert np.array_equal(got_g[:, V:], logits[:, V:]), "padding columns of the logits"
    assert np.array_equal(u16(ud), teach), "the teacher"


@pytest.mark.parametrize("shape", [(6, 50257, 50264), (2, 9001, 9008), (3, 7, 8)], ids=lambda s: "x".join(map(str, s)))
def test_pure_ce_without_a_teacher_is_the_fused_classifier(ctx, shape):
    rows, V, P = shape
    logits, _, targets = DC.inputs(rows, V, P, "indep")
    want_g, want_l = logits.copy(), np.full(rows, 0.5, np.float32)
    O.fused_classifier(want_g, want_l, targets, V, dloss=DC.dloss_of(rows))
    zd, td = bf16_t(logits.copy(), ctx.device), torch.from_numpy(targets.copy()).to(ctx.device)
    losses = torch.full((rows,), 0.5, dtype=torch.float32, device=ctx.device)
    assert _run(ctx, zd, None, 0, losses, None, DC.dloss_of(rows), td, rows, 1, V, P, None, 1.0, 0.0, 3.0) == 0
    ctx.sync()
    assert np.array_equal(losses.cpu().numpy().view(np.uint32), want_l.view(np.uint32)) and np.array_equal(u16(zd), want_g)


def test_mask_loss_only_and_unread_targets(ctx):
    rows, V, P = 4, 66, 72
    logits, teach, targets = DC.inputs(rows, V, P, "indep")
    ldt = teach.shape[1]
    mask = np.array([0, 0x10000, 5, 0x10003], np.int32)
    logits, teach = logits.copy(), teach.copy()
    zd, ud = bf16_t(logits, ctx.device), bf16_t(teach, ctx.device)
    td, md = torch.from_numpy(targets.copy()).to(ctx.device), torch.from_numpy(mask).to(ctx.device)
    losses = torch.full((rows,), 0.5, dtype=torch.float32, device=ctx.device)
    kd = torch.full((rows,), -7.0, dtype=torch.float32, device=ctx.device)
    assert _run(ctx, zd, ud, ldt, losses, kd, 0.25, td, 2, 2, V, P, md, 0.5, 0.5, 2.0) == 0
    ctx.sync()
    want_l, want_kd, want_g = R.distill_classifier(logits, teach, np.full(rows, 0.5, np.float32), targets, V, 0.25, 0.5, 0.5, 2.0, mask=mask)
    skip = (mask & 0x10000) != 0
    got_l, got_kd, got_g = losses.cpu().numpy(), kd.cpu().numpy(), u16(zd)
    assert np.array_equal(got_g, want_g) and np.array_equal(got_g[skip], logits[skip])
    assert np.array_equal(got_l, want_l) and (got_l[skip] == 0.5).all()
    assert np.array_equal(got_kd[~skip], want_kd[~skip]) and (got_kd[skip] == -7.0).all()
    # write_dlogits = 0: the logits stay as they were, and a second call accumulates
    z2 = bf16_t(logits, ctx.device)
    l2 = torch.zeros(rows, dtype=torch.float32, device=ctx.device)
    for _ in range(2):
        assert _run(ctx, z2, ud, ldt, l2, kd, 0.25, td, 2, 2, V, P, None, 0.5, 0.5, 2.0, write=0) == 0
    ctx.sync()
    once = R.distill_classifier(logits, teach, np.zeros(rows, np.float32), targets, V, 0.25, 0.5, 0.5, 2.0, write_dlogits=False)
    twice = R.distill_classifier(logits, teach, once[0], targets, V, 0.25, 0.5, 0.5, 2.0, write_dlogits=False)
    assert np.array_equal(u16(z2), logits) and np.array_equal(l2.cpu().numpy(), twice[0])
    # ce_weight = 0 reads no targets: ids far out of range, and a NULL pointer
    wild = torch.full((rows,), 2 ** 30, dtype=torch.int32, device=ctx.device)
    want = R.distill_classifier(logits, teach, np.zeros(rows, np.float32), None, V, 0.25, 0.0, 1.0, 2.0)
    for tg in (wild, None):
        z3 = bf16_t(logits, ctx.device)
        l3 = torch.zeros(rows, dtype=torch.float32, device=ctx.device)
        assert _run(ctx, z3, ud, ldt, l3, kd, 0.25, tg, 4, 1, V, P, None, 0.0, 1.0, 2.0) == 0
        ctx.sync()
        assert np.array_equal(l3.cpu().numpy(), want[0]) and np.array_equal(kd.cpu().numpy(), want[1]) and np.array_equal(u16(z3), want[2])


def test_refusals_launch_nothing(ctx):
    z = torch.ones(4, 16, dtype=torch.bfloat16, device=ctx.device)
    u = torch.ones(4, 24, dtype=torch.bfloat16, device=ctx.device)
    big = torch.ones(4 * 16 + 8, dtype=torch.bfloat16, device=ctx.device)
    losses = torch.zeros(4, dtype=torch.float32, device=ctx.device)
    kd = torch.zeros(4, dtype=torch.float32, device=ctx.device)
    td = torch.zeros(4, dtype=torch.int32, device=ctx.device)
    nan, inf = float("nan"), float("inf")

    def call(logits=z, teacher=u, ld=24, ls=losses, tg=td, V=16, P=16, a=0.5, b=0.5, tau=2.0):
        return _run(ctx, logits, teacher, ld, ls, kd, 1.0, tg, 4, 1, V, P, None, a, b, tau)
    refused = [
        (dict(logits=None), INVALID_ARGS, "null"), (dict(ls=None), INVALID_ARGS, "null"),
        (dict(teacher=None), INVALID_ARGS, "teacher"), (dict(tg=None), INVALID_ARGS, "targets"),
        (dict(a=-1.0), INVALID_ARGS, "weight"), (dict(b=nan), INVALID_ARGS, "weight"), (dict(a=inf), INVALID_ARGS, "weight"), (dict(a=0.0, b=0.0), INVALID_ARGS, "weight"),
        (dict(tau=0.0), INVALID_ARGS, "temperature"), (dict(tau=-2.0), INVALID_ARGS, "temperature"), (dict(tau=nan), INVALID_ARGS, "temperature"),
        (dict(tau=inf), INVALID_ARGS, "temperature"),
        (dict(V=16, P=8), INVALID_ARGS, "P >= V"), (dict(V=16, ld=8), INVALID_ARGS, "teacher_ld"),
        (dict(V=10, P=12), UNALIGN, "16-byte"), (dict(V=10, ld=20), UNALIGN, "16-byte"),
        (dict(logits=big[1:65].view(4, 16)), UNALIGN, "16-byte"), (dict(teacher=big[1:65].view(4, 16), ld=16), UNALIGN, "16-byte"),
        (dict(teacher=z, ld=16), INVALID_ARGS, "overlap"), (dict(logits=big[:64].view(4, 16), teacher=big[8:72].view(4, 16), ld=16), INVALID_ARGS, "overlap"),
    ]
    for kw, code, word in refused:
        assert call(**kw) == code, kw
        assert word in ctx.hip.kf_last_error().decode(), (kw, ctx.hip.kf_last_error().decode())
    ctx.sync()
    assert bool((z == 1).all()) and bool((u == 1).all()) and not bool(losses.any()) and not bool(kd.any())
    assert call(tg=None, a=0.0, b=1.0) == 0 and call(teacher=None, ld=0, a=1.0, b=0.0) == 0   # what may be NULL when its weight is zero
    ctx.sync()


def test_full_size_rows_beyond_2_31_bytes(ctx):
    """8 x 1024 rows of V = P = 151 936: row 7067 starts 2^31 bytes in.  The first and the last 32 rows against float64."""
    B, T, V = 8, 1024, 151936
    rows, a, b, tau = B * T, 0.5, 0.5, 2.0
    g = torch.Generator(device=ctx.device).manual_seed(11)
    z = torch.empty(rows, V, dtype=torch.bfloat16, device=ctx.device)
    u = torch.empty(rows, V, dtype=torch.bfloat16, device=ctx.device)
    for r in range(0, rows, 512):   # in slabs: no fp32 copy of a whole matrix
        z[r:r + 512] = (torch.randn(512, V, generator=g, device=ctx.device) * 2.0).to(torch.bfloat16)
        u[r:r + 512] = (torch.randn(512, V, generator=g, device=ctx.device) * 3.0).to(torch.bfloat16)
    tg = torch.randint(0, V, (rows,), generator=g, device=ctx.device, dtype=torch.int32)
    pick = torch.cat([torch.arange(32), torch.arange(rows - 32, rows)]).to(ctx.device)
    z0, u0, t0 = u16(z[pick]), u16(u[pick]), tg[pick].cpu().numpy()
    losses = torch.zeros(rows, dtype=torch.float32, device=ctx.device)
    kd = torch.zeros(rows, dtype=torch.float32, device=ctx.device)
    assert _run(ctx, z, u, V, losses, kd, 1.0 / rows, tg, B, T, V, V, None, a, b, tau) == 0
    ctx.sync()
    got = (losses[pick].cpu().numpy(), kd[pick].cpu().numpy(), u16(z[pick]))
    print("full size: mean loss %.5f mean KL %.5f" % (float(losses.mean()), float(kd.mean())))
    _check_against_fp64(64, V, z0, u0, t0, (a, b, tau), got, 1.0 / rows, 0.0)
    assert bool(torch.isfinite(kd).all()) and bool((kd > 0).all()) and bool(torch.isfinite(losses).all())
    assert np.array_equal(u16(u[pick]), u0), "the teacher"
