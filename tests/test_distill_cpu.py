"""kf_distill_classifier without a GPU: the numpy restatement of its stated order (tests/distill_restate.py) against the oracle's scalar exp / log, against torch
fp64 on the kernel test's own cases, against the oracle's fused classifier where the two must coincide, and the exact-zero property; then the argument checks of
_TrainStep.check_distill and the refusals of an unregistered trainer's new entries.

Bars of the fp64 comparison, from the arithmetic and not from the code under test.  A probability's fp32 chain is at most 150 sequential adds per thread at
V = 151 936 plus two 10-level trees and a 2-ulp exp: relative error under 2^-16.  Gradient: one bf16 rounding (2^-9, doubled for the chain feeding it) plus four times
the chain bound on every term: |g - g64| <= 2^-8 |g64| + 2^-14 dloss (a p + b tau (pt + qt)).  KL: 2^-14 (|A / Ut| + |log Ut| + |log St| + 1).  CE: rtol = atol = 1e-5
as tests/test_gpu_loss.py::test_fused_classifier_full_size_properties; a row's loss a CE + b tau^2 KL gets the two bars weighted the same way."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from koifish_amd.train_step import GPT2Step, Qwen3Step, _TrainStep
from oracle import oracle as O
from tests import distill_cases as DC
from tests import distill_restate as R

INVALID_ARGS = -20


def test_vectorised_exp_and_log_equal_the_oracle_bit_for_bit():
    rng = np.random.default_rng(5)
    x = np.concatenate([np.array([0.0, -0.0, -87.33654, -87.3365, -87.0, -88.0, -100.0, -103.9, -1e30, -np.inf, 88.0, 88.72283, 88.8, 1.0, -1.0, np.nan], dtype=np.float32),
                        -np.abs(rng.standard_normal(1500) * 30).astype(np.float32),          # what z - max and (z - max) / tau produce
                        np.linspace(-87.33654, -80.0, 600, dtype=np.float32),                 # results near and below the smallest normal
                        rng.uniform(-104.0, -87.0, 400).astype(np.float32),                   # the flush region
                        rng.uniform(-3.0, 3.0, 500).astype(np.float32)])
    got, want = R.expf(x), O.expf(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), x[got.view(np.uint32) != want.view(np.uint32)][:8]
    # the recipe cuts off at log(2^-126): its smallest results sit just above the smallest normal and everything below is 0 -- exp itself has no subnormal result;
    # the subnormals of this kernel are products exp * (1 / sum), plain float32 multiplies, and subnormal ARGUMENTS of the log below
    small = want[(x < -87.3) & (x >= np.float32(-87.33654))]
    assert small.size and (small < np.float32(1.3e-38)).all() and (small >= np.float32(1.1754944e-38)).all()
    assert not want[x < np.float32(-87.33654)].any()
    y = np.concatenate([np.array([0.0, 1.0, 2.0, 0.5, np.inf, -1.0, np.nan, 1e-45, 1e-39, 1.1754944e-38, 3.4e38, 1.4142135, 1.4142137, 0.70710677], dtype=np.float32),
                        np.exp(rng.uniform(-100, 88, 2000)).astype(np.float32), rng.uniform(0.5, 2.0, 1000).astype(np.float32)])
    got, want = R.logf(y), O.logf(y)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), y[~same][:8]


def test_fma_rounds_once():
    """the restatement's fma against exact rational arithmetic on products whose low bits decide the rounding"""
    from fractions import Fraction
    rng = np.random.default_rng(6)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.choice([0.0, 2.0 ** -24, -2.0 ** -23, 1e-3], 400))).astype(np.float32)
    got = R.fma(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))   # float(Fraction) rounds the exact value once to double, then once to float32: compare through the neighbours instead
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert np.float32(got[i]) == np.float32(best), (a[i], b[i], c[i])


def _check_against_fp64(rows, V, logits, teach, targets, weights, got, dloss, fill):
    a, b, tau = weights
    losses, kd, glog = got
    ref = R.reference64(logits, teach, targets, V, a, b, tau)
    kl_bar = 2.0 ** -14 * (np.abs(ref["a_over_u"]) + np.abs(ref["log_u"]) + np.abs(ref["log_s"]) + 1.0)
    if b != 0:
        err = np.abs(kd.astype(np.float64) - ref["kl"])
        assert (err <= kl_bar).all(), "KL: worst %.3g against a bar of %.3g" % (err.max(), kl_bar[err.argmax()])
    ce_bar = 1e-5 + 1e-5 * np.abs(ref["ce"])
    err = np.abs((losses.astype(np.float64) - fill) - ref["loss"])
    bar = a * ce_bar + b * tau * tau * kl_bar + 2.0 ** -22 * (fill + np.abs(ref["loss"]))   # the last term: the accumulation into a pre-filled fp32 word
    assert (err <= bar).all(), "loss: worst %.3g against a bar of %.3g" % (err.max(), bar[err.argmax()])
    g = R.bf16_to_f32(glog[:, :V]).astype(np.float64)
    g64 = ref["g"] * dloss
    gbar = 2.0 ** -8 * np.abs(g64) + 2.0 ** -14 * dloss * (a * ref["p"] + b * tau * (ref["pt"] + ref["qt"]))
    err = np.abs(g - g64)
    assert (err <= gbar).all(), "gradient: %d of %d elements over the bar, worst ratio %.3g" % ((err > gbar).sum(), err.size, (err / np.maximum(gbar, 1e-300)).max())


@pytest.mark.parametrize("teacher", DC.TEACHERS)
@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_fp64(shape, teacher):
    rows, V, P = shape
    logits, teach, targets = DC.inputs(rows, V, P, teacher)
    for weights in DC.WEIGHTS:
        got = DC.restated(rows, V, P, teacher, weights)
        _check_against_fp64(rows, V, logits, teach, targets, weights, got, DC.dloss_of(rows), DC.LOSS_FILL)
        assert np.array_equal(got[2][:, V:], logits[:, V:]), "padding columns"
    if teacher == "indep" and V > 100:
        kd = DC.restated(rows, V, P, teacher, DC.WEIGHTS[1])[1]
        assert kd.min() > 1.0, "the independent teacher is meant to be a few nats away"


def test_closed_form_equals_torch_fp64_autograd():
    """reference64's gradient is the derivative of its loss: torch fp64 autograd on a CE + b tau^2 KL(softmax(u / tau) || softmax(z / tau))"""
    F = torch.nn.functional
    logits, teach, targets = DC.inputs(4, 66, 72, "indep")
    z0, u0 = R.bf16_to_f32(logits[:, :66]).astype(np.float64), R.bf16_to_f32(teach[:, :66]).astype(np.float64)
    for a, b, tau in [(0.5, 0.5, 2.0), (0.0, 1.0, 1.0), (1.0, 0.25, 0.5), (0.3, 0.7, 4.0)]:
        z = torch.tensor(z0, requires_grad=True)
        kl = F.kl_div(F.log_softmax(z / tau, -1), F.log_softmax(torch.tensor(u0) / tau, -1), reduction="none", log_target=True).sum(-1)
        loss = a * F.cross_entropy(z, torch.tensor(targets).long(), reduction="none") + b * tau * tau * kl
        loss.sum().backward()
        ref = R.reference64(logits, teach, targets, 66, a, b, tau)
        assert np.allclose(ref["loss"], loss.detach().numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(ref["kl"], kl.detach().numpy(), rtol=1e-11, atol=1e-12)
        assert np.allclose(ref["g"], z.grad.numpy(), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("shape", [(6, 50257, 50264), (4, 66, 72), (2, 9001, 9008), (3, 7, 8), (1, 1, 8)], ids=lambda s: "x".join(map(str, s)))
def test_pure_ce_equals_the_oracles_fused_classifier(shape):
    rows, V, P = shape
    logits, _, targets = DC.inputs(rows, V, P, "indep")
    mask = np.zeros(rows, np.int32)
    if rows > 2:
        mask[1] = 0x10000
    want_logits, want_losses = logits.copy(), np.full(rows, 0.5, np.float32)
    O.fused_classifier(want_logits, want_losses, targets, V, dloss=DC.dloss_of(rows), mask=mask)
    losses, kd, got = R.distill_classifier(logits, None, np.full(rows, 0.5, np.float32), targets, V, DC.dloss_of(rows), 1.0, 0.0, 3.0, mask=mask)
    assert np.array_equal(losses.view(np.uint32), want_losses.view(np.uint32))
    assert np.array_equal(got, want_logits)
    assert not kd.any()


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_teacher_equal_to_student_is_exactly_zero(tau):
    for rows, V, P in [(2, 9001, 9008), (3, 7, 8), (3, 1000, 1000)]:
        logits, _, targets = DC.inputs(rows, V, P, "indep")
        fill = np.full(rows, 0.5, np.float32)
        l_ce, _, g_ce = R.distill_classifier(logits, None, fill, targets, V, DC.dloss_of(rows), 0.75, 0.0, 1.0)
        l_kd, kd, g_kd = R.distill_classifier(logits, logits.copy(), fill, targets, V, DC.dloss_of(rows), 0.75, 0.5, tau)
        assert np.array_equal(kd.view(np.uint32), np.zeros(rows, np.uint32)), kd   # +0.0, bit for bit
        assert np.array_equal(g_kd, g_ce) and np.array_equal(l_kd.view(np.uint32), l_ce.view(np.uint32))


def _student(**kw):
    ctx = types.SimpleNamespace(device=torch.device("cpu"))
    d = dict(ctx=ctx, B=2, T=4, N=8, V=250, Vp=256, _n_sections=1)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _fake_trainer(cls, ctx, **kw):
    t = cls.__new__(cls)   # no __init__: nothing touches a device; close() finds no handle
    t.ctx, t.B, t.T, t.N, t.V, t.Vp = ctx, 2, 4, 8, 250, 256
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_check_distill_refusals():
    chk = _TrainStep.check_distill
    st = _student()
    good = torch.zeros(8, 256, dtype=torch.bfloat16)
    assert chk(st, good) == ("tensor", 256)
    assert chk(st, torch.zeros(8, 512, dtype=torch.bfloat16)[:, :256]) == ("tensor", 512)
    teacher = _fake_trainer(GPT2Step, st.ctx)
    assert chk(st, teacher, 1.0, 0.0, 4.0) == ("trainer", 256)
    assert chk(_fake_trainer(Qwen3Step, st.ctx), teacher) == ("trainer", 256)   # any family teaches any family
    bad = [
        dict(teacher=good, kd_weight=-0.1), dict(teacher=good, ce_weight=float("nan")), dict(teacher=good, kd_weight=0.0, ce_weight=0.0),
        dict(teacher=good, kd_weight=float("inf")), dict(teacher=good, temperature=0.0), dict(teacher=good, temperature=-1.0), dict(teacher=good, temperature=float("inf")),
        dict(teacher=good, temperature="2"),
        dict(teacher=st),                                                    # itself
        dict(teacher="logits"), dict(teacher=np.zeros((8, 256), np.float32)),
        dict(teacher=torch.zeros(8, 256)),                                   # fp32
        dict(teacher=torch.zeros(8 * 256, dtype=torch.bfloat16)),            # 1-D
        dict(teacher=torch.zeros(7, 256, dtype=torch.bfloat16)),             # rows
        dict(teacher=torch.zeros(8, 248, dtype=torch.bfloat16)),             # narrower than V
        dict(teacher=torch.zeros(8, 252, dtype=torch.bfloat16)),             # a row stride that is no multiple of 8
        dict(teacher=torch.zeros(256, 8, dtype=torch.bfloat16).t()),         # column stride
        dict(teacher=torch.zeros(8 * 256 + 8, dtype=torch.bfloat16)[1:8 * 256 + 1].view(8, 256)),   # rows not 16-byte aligned
        dict(teacher=torch.zeros(8, 256, dtype=torch.bfloat16, device="meta")),                       # another device
        dict(teacher=_fake_trainer(GPT2Step, types.SimpleNamespace(device=torch.device("cpu")))),   # another context
        dict(teacher=_fake_trainer(GPT2Step, st.ctx, B=4)), dict(teacher=_fake_trainer(GPT2Step, st.ctx, T=8)),
        dict(teacher=_fake_trainer(Qwen3Step, st.ctx, V=251)), dict(teacher=_fake_trainer(Qwen3Step, st.ctx, Vp=320)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            chk(st, **kw)
    with pytest.raises(ValueError, match="layer sections"):
        chk(_student(_n_sections=2), good)
    me = _fake_trainer(GPT2Step, st.ctx)
    with pytest.raises(ValueError, match="own teacher"):
        chk(me, me)


TRAINERS = {
    "gpt2": ("gpt2", lambda host, ctx: host.kfh_gpt2_create(ctx, 128, 2, 2, 250, 256, 2, 64)),
    "qwen3t": ("qwen3t", lambda host, ctx: host.kfh_qwen3t_create(ctx, 128, 2, 4, 2, 64, 256, 250, 256, 2, 64, 1e-6, 1)),
}


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_unregistered_trainer_refuses_distillation(which):
    """as tests/test_trainers_cpu.py: a zeroed buffer stands in for the context, and no call here dereferences it"""
    _, host = L.load()
    family, create = TRAINERS[which]
    f = lambda name: getattr(host, "kfh_%s_%s" % (family, name))
    keep = C.create_string_buffer(4096)
    h = create(host, C.cast(keep, C.c_void_p))
    assert h
    try:
        mem = C.create_string_buffer(4096)
        p = C.cast(mem, C.c_void_p)
        assert f("forward_logits")(h, p) == INVALID_ARGS
        assert f("last_error")().decode().startswith("forward_logits:")
        assert f("forward_logits")(h, None) == INVALID_ARGS
        assert f("set_distill")(h, p, 256, 0.5, 0.5, 2.0, p) == INVALID_ARGS
        assert "registered" in f("last_error")().decode()
        assert f("set_distill")(h, None, 0, 1.0, 0.0, 1.0, None) == 0   # off is always accepted
        assert f("forward")(h, p, p) == INVALID_ARGS and f("backward")(h) == INVALID_ARGS
    finally:
        f("destroy")(h)
    del keep
