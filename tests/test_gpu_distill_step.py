"""Distillation through the trainers (set_distill / forward_logits / kd_losses of koifish_amd.train_step, TrainerCore::SetDistill / ForwardLogits underneath) at the toy
shape of tests/qwen3_toy.py: the forward against the kernel's contract (tests/distill_restate.py on the two trainers' own logits), the backward against torch fp64
autograd with the bars of tests/test_gpu_qwen3_step.py::_check_grads, the exact zeros of self-distillation, KL falling over steps, the way back to the plain path, a
plain tensor as teacher, one GPT-2 case and the refusals."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from koifish_amd.train_step import MATS, GPT2Step, Qwen3Step
from oracle import oracle as O
from tests import distill_restate as R
from tests.conftest import u16
from tests.qwen3_toy import CFG, HP, Bn, N, T, V, Vp, make, ref_logits, torch_params
from tests.test_gpu_qwen3_step import _check_grads, _dev_ids

pytestmark = pytest.mark.gpu


def _snap_logits(st, d_ids):
    st.forward_logits(d_ids)
    st.ctx.sync()
    return u16(st.logits).copy()


def _check_contract(st, te, d_ids, d_tgt, tgt, ce, kd, tau):
    """after forward under set_distill: logits buffer, losses and kd_losses() equal the restatement applied to the two forward_logits snapshots"""
    zs, ut = _snap_logits(st, d_ids), _snap_logits(te, d_ids)
    assert zs.shape == (N, Vp) and zs[:, :V].any()
    with pytest.raises(L.KFError):
        st.backward()   # forward_logits leaves nothing a backward could start from
    st.set_distill(te, kd, ce, tau)
    st.forward(d_ids, d_tgt)
    st.ctx.sync()
    want_l, want_kd, want_g = R.distill_classifier(zs, ut, np.zeros(N, np.float32), tgt, V, 1.0 / N, ce, kd, tau)
    assert np.array_equal(u16(te.logits), ut), "the teacher's logits are its forward_logits of this batch"
    assert np.array_equal(u16(st.logits), want_g)
    assert np.array_equal(st.losses.cpu().numpy().view(np.uint32), want_l.view(np.uint32))
    assert np.array_equal(st.kd_losses().cpu().numpy().view(np.uint32), want_kd.view(np.uint32))
    assert abs(st.kd_loss() - float(want_kd.astype(np.float64).mean())) <= 1e-5 * float(want_kd.mean())
    return want_kd


def test_forward_matches_the_kernel_contract(ctx):
    st, ids, tgt = make(ctx, seed=91)
    te, _, _ = make(ctx, seed=17)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    kd = _check_contract(st, te, d_ids, d_tgt, tgt, 0.5, 0.5, 2.0)
    print("toy KL rows: mean %.4f max %.4f" % (kd.mean(), kd.max()))
    assert kd.mean() > 1e-3
    st.close(), te.close()


def test_backward_vs_autograd(ctx):
    F = torch.nn.functional
    st, ids, tgt = make(ctx, seed=91)
    te, _, _ = make(ctx, seed=17)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    a, b, tau = 0.5, 0.5, 2.0
    ut = torch.tensor(O.bf16_to_f32(_snap_logits(te, d_ids)[:, :V]).astype(np.float64))   # the device's teacher logits, a constant
    P, leaves = torch_params(ctx, st)
    z = ref_logits(P, ids, Bn, T)
    kl = F.kl_div(F.log_softmax(z / tau, -1), F.log_softmax(ut / tau, -1), reduction="none", log_target=True).sum(-1)
    loss = (a * F.cross_entropy(z, torch.from_numpy(tgt).long(), reduction="none") + b * tau * tau * kl).mean()
    loss.backward()
    st.set_distill(te, b, a, tau)
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    ref, dev = float(loss.detach()), float(st.losses.mean())
    print("distillation loss: device %.6f fp64 %.6f" % (dev, ref))
    assert abs(dev - ref) <= 2.0 ** -7 * ref
    _check_grads(st, leaves)
    st.close(), te.close()


def test_self_distillation_is_exactly_zero(ctx):
    st, ids, tgt = make(ctx, seed=91)
    te, _, _ = make(ctx, seed=91)   # the same masters
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    st.set_grad_clip(mode="report")
    st.set_distill(te, kd_weight=1.0, ce_weight=0.0, temperature=2.0)
    st.forward(d_ids, d_tgt)
    ctx.sync()
    assert not st.kd_losses().cpu().numpy().view(np.uint32).any(), "every KL row is +0.0"
    assert not (u16(st.logits) & 0x7fff).any(), "the logit gradient holds zeros of either sign only"
    assert not st.losses.cpu().numpy().any()
    st.backward()
    st.update(**HP)   # the norms are taken at the head of the update
    ctx.sync()
    assert st.grad_norm() == 0.0
    st.close(), te.close()


def test_steps_reduce_kl(ctx):
    st, ids, tgt = make(ctx, seed=91)
    te, _, _ = make(ctx, seed=17)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    before = [u16(e["p"]).copy() for e in te.params]
    st.set_distill(te, kd_weight=1.0, ce_weight=0.0, temperature=1.0)
    kls = []
    for _ in range(3):
        st.step(d_ids, d_tgt, **HP)
        ctx.sync()
        kls.append(st.kd_loss())
    print("mean KL over three steps on one batch:", ["%.5f" % v for v in kls])
    assert kls[1] < kls[0] and kls[2] < kls[1], kls
    assert all(np.array_equal(u16(e["p"]), b4) for e, b4 in zip(te.params, before)) and te.t == 0, "the teacher is never updated"
    st.close(), te.close()


def test_set_distill_none_restores_the_plain_path(ctx):
    st, ids, tgt = make(ctx, seed=91)
    tw, _, _ = make(ctx, seed=91)   # never distilled
    te, _, _ = make(ctx, seed=17)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    tw.forward(d_ids, d_tgt)
    st.set_distill(te, 0.5, 0.5, 2.0)
    st.forward(d_ids, d_tgt)
    ctx.sync()
    assert not np.array_equal(u16(st.logits), u16(tw.logits))
    st.set_distill(None)
    st.forward(d_ids, d_tgt)
    ctx.sync()
    assert np.array_equal(u16(st.logits), u16(tw.logits)) and np.array_equal(st.losses.cpu().numpy().view(np.uint32), tw.losses.cpu().numpy().view(np.uint32))
    with pytest.raises(L.KFError):
        st.kd_losses()
    st.close(), tw.close(), te.close()


def test_a_plain_tensor_as_teacher(ctx):
    st, ids, tgt = make(ctx, seed=91)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    rng = np.random.default_rng(3)
    wide = np.full((N, Vp + 24), 0x7fc1, np.uint16)   # a row stride of its own, NaN bits beyond V
    wide[:, :V] = O.f32_to_bf16((rng.standard_normal((N, V)) * 1.5).astype(np.float32))
    rows = torch.from_numpy(wide.view(np.int16)).view(torch.bfloat16).to(ctx.device)[:, :Vp]
    zs = _snap_logits(st, d_ids)
    st.set_distill(rows, kd_weight=0.25, ce_weight=1.0, temperature=0.5)
    st.forward(d_ids, d_tgt)
    ctx.sync()
    want_l, want_kd, want_g = R.distill_classifier(zs, wide, np.zeros(N, np.float32), tgt, V, 1.0 / N, 1.0, 0.25, 0.5)
    assert np.array_equal(u16(st.logits), want_g) and np.array_equal(st.losses.cpu().numpy(), want_l) and np.array_equal(st.kd_losses().cpu().numpy(), want_kd)
    st.backward()   # and the step goes on from there
    ctx.sync()
    assert all(u16(e["g"]).any() for e in st.params)
    st.close()


def _gpt2_toy(ctx, seed, **kw):
    """the toy of tests/test_gpu_train_step.py::test_gpt2_two_consecutive_steps_with_update"""
    Cn, H, NL = 128, 2, 2
    rng = np.random.default_rng(seed)
    bf = lambda a: torch.from_numpy(O.f32_to_bf16(a.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    mk = lambda *s, std=0.08: bf(rng.normal(0, std, size=s))
    lnw = lambda: bf(1 + rng.normal(0, 0.1, Cn))
    shapes = dict(qkv=(3 * Cn, Cn), proj=(Cn, Cn), fc=(4 * Cn, Cn), proj2=(Cn, 4 * Cn))
    wte = torch.zeros(Vp, Cn, dtype=torch.bfloat16)
    wte[:V] = mk(V, Cn, std=0.2)
    masters = dict(wte=wte, wpe=mk(T, Cn, std=0.05), lnf=(lnw(), mk(Cn)),
                   blocks=[dict({k: (mk(*shapes[k]), mk(shapes[k][0])) for k in MATS}, ln=(lnw(), mk(Cn), lnw(), mk(Cn))) for _ in range(NL)])
    return GPT2Step(ctx, Cn, H, NL, V, Vp, Bn, T, masters=masters, **kw)


def test_gpt2_forward_matches_the_kernel_contract(ctx):
    st, te = _gpt2_toy(ctx, 303), _gpt2_toy(ctx, 304)
    rng = np.random.default_rng(8)
    ids, tgt = rng.integers(0, V, N).astype(np.int32), rng.integers(0, V, N).astype(np.int32)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    _check_contract(st, te, d_ids, d_tgt, tgt, 0.5, 0.5, 2.0)
    st.backward()
    ctx.sync()
    st.close(), te.close()


def test_refusals(ctx):
    st, ids, tgt = make(ctx, seed=91)
    with pytest.raises(ValueError, match="own teacher"):
        st.set_distill(st)
    for other in (Qwen3Step(ctx, CFG, Bn + 1, T), Qwen3Step(ctx, CFG, Bn, T // 2), Qwen3Step(ctx, dict(CFG, vocab=200), Bn, T), _gpt2_toy(ctx, 1, layers_in_branch=1)):
        if isinstance(other, GPT2Step):
            st.set_distill(other)   # a GPT-2 trainer teaches a Qwen3 one; its own sections do not matter to the student
            st.set_distill(None)
            with pytest.raises(ValueError, match="layer sections"):
                other.set_distill(st)
            with pytest.raises(L.KFError, match="layer sections"):   # and the trainer itself says the same to a caller that skips the Python check
                other._call("set_distill", st.logits.data_ptr(), Vp, 0.5, 0.5, 1.0, None, check=other._check_host)
        else:
            with pytest.raises(ValueError):
                st.set_distill(other)
        other.close()
    with pytest.raises(L.KFError, match="overlap"):
        st._call("set_distill", st.logits.data_ptr(), Vp, 0.5, 0.5, 1.0, None, check=st._check_host)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    tw, _, _ = make(ctx, seed=91)
    st.forward(d_ids, d_tgt)   # every refusal left the plain path in place: a twin that was never asked holds the same bits
    tw.forward(d_ids, d_tgt)
    ctx.sync()
    assert st._distill is None and np.array_equal(st.losses.cpu().numpy().view(np.uint32), tw.losses.cpu().numpy().view(np.uint32)) and np.array_equal(u16(st.logits), u16(tw.logits))
    st.close(), tw.close()
