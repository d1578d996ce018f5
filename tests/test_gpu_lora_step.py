"""Qwen3Step(train_target="lora") on the toy of tests/qwen3_toy.py (dim 128, 2 layers, 4-bit matrices, B 2 x T 64), rank 16: the LORA branch of SLP::Forw / SLP::Back
behind the trainer.  In the torch fp64 model an adapted weight is  W_deq + s^2 b a  with W_deq the dequantisation the device multiplies and a, b the leaves; the device's
gradient vector [gA | gB] is compared with the two leaves' gradients.  Bars are those of tests/test_gpu_qwen3_step.py: loss within 2^-7 relative, every gradient max
<= 2^-5 and rms <= 2^-7 of the reference's largest magnitude (rms 2^-6 for the 64-element q/k-norm weights, as there).  The update is the oracle's CU_adamw on the
device's own gradients, bit for bit, at the trainer's seed rule; the frozen blobs stay byte for byte."""
import numpy as np
import pytest
import torch

import gradnorm_restate as G
from koifish_amd import lib as L
from koifish_amd.train_step import Q3_MATS, Qwen3Step
from oracle import oracle as O
from tests import qwen3_toy as Q
from tests.conftest import u16

pytestmark = pytest.mark.gpu

RANK, S = 16, 0.5
HP = Q.HP


def _adapters(seed=7, targets=Q3_MATS):
    """non-zero a and b for every adapted matrix of the toy, bf16 host tensors"""
    rng = np.random.default_rng(seed)
    bf = lambda v: torch.from_numpy(O.f32_to_bf16(v.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    shapes = Qwen3Step._mat_shapes(Q.CFG)
    return {"l%d.%s.w" % (l, k): (bf(rng.normal(0, 0.05, (RANK, shapes[k][1]))), bf(rng.normal(0, 0.05, (shapes[k][0], RANK))))
            for l in range(Q.CFG["n_layer"]) for k in targets}


def _dev(ctx, ids, tgt):
    return torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device)


def _torch_params(ctx, st):
    """tests/qwen3_toy.py::torch_params with the adapter form: P[k] = W_deq + s^2 b a, leaves (a, b)"""
    P, leaves = {}, {}
    for e in st.params:
        k = Q.key_of(e["name"])
        if e.get("lora"):
            bl, r = e["blob"], e["rank"]
            v = Q.F64(u16(e["p"]))
            a = v[:r * bl.ne1].reshape(r, bl.ne1).clone().requires_grad_(True)
            b = v[r * bl.ne1:].reshape(bl.ne0, r).clone().requires_grad_(True)
            P[k] = Q.F64(u16(ctx.dequant(bl))).reshape(bl.ne0, bl.ne1) + (e["s"] ** 2) * (b @ a)
            leaves[e["name"]] = (a, b)
        elif e["type"] is not None and e["type"] != L.BF16:
            P[k] = Q.F64(u16(ctx.dequant(e["blob"]))).reshape(tuple(e["p"].shape)).requires_grad_(True)
            leaves[e["name"]] = P[k]
        else:
            P[k] = Q.F64(u16(e["p"])).reshape(tuple(e["p"].shape)).requires_grad_(True)
            leaves[e["name"]] = P[k]
    return P, leaves


def _lora_entries(st):
    return [(i, e) for i, e in enumerate(st.params) if e.get("lora")]


def _snapshot(st):
    return [tuple(u16(e[k]).copy() for k in ("p", "g", "m", "v")) for _, e in _lora_entries(st)]


def _oracle_adamw_on_adapters(st, before, t, scale=None):
    """[a | b] of every adapter and both moments == the oracle's CU_adamw on the read-back device gradient, decayed, seed + 7919 t + i; the gradients zeroed"""
    b1c, b2c = 1.0 - HP["beta1"] ** t, 1.0 - HP["beta2"] ** t
    for (i, e), (p0, g0, m0, v0) in zip(_lora_entries(st), before):
        p, g, m, v = (a.copy() for a in (p0, g0, m0, v0))
        assert O.adamw(p, g, m, v, HP["lr"], HP["beta1"], HP["beta2"], b1c, b2c, HP["eps"], HP["wd"], 1.0 if scale is None else float(scale[i]),
                       (HP["seed"] + 7919 * t + i) & 0xFFFFFFFF) == 0
        assert np.array_equal(u16(e["p"]), p), "adapter of %s differs from the oracle's AdamW" % e["name"]
        assert np.array_equal(u16(e["m"]), m) and np.array_equal(u16(e["v"]), v), e["name"]
        assert not u16(e["g"]).any() and not np.array_equal(p, p0), e["name"]


def test_lora_step_gradients_update_and_frozen_base(ctx):
    st, ids, tgt = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters=_adapters())
    d_ids, d_tgt = _dev(ctx, ids, tgt)
    le = _lora_entries(st)
    assert len(le) == 7 * Q.CFG["n_layer"] and [e["name"] for e in st.params][:7] == ["l0.%s.w" % k for k in Q3_MATS]
    for _, e in le:   # the memory claim: one vector [a | b] and its gradient and moments, nothing of the matrix's size
        bl = e["blob"]
        assert all(e[k].numel() == RANK * (bl.ne0 + bl.ne1) for k in ("p", "g", "m", "v")) and e["wd"] and e["lora"] is True and e["ax"].shape == (Q.N, RANK)
    # ---- forward + backward against autograd
    P, leaves = _torch_params(ctx, st)
    loss = Q.ref_loss(P, ids, tgt)
    loss.backward()
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    ref_loss, dev_loss = float(loss.detach()), float(st.losses.mean())
    print("loss: device %.6f, fp64 %.6f" % (dev_loss, ref_loss))
    assert abs(dev_loss - ref_loss) <= 2.0 ** -7 * ref_loss, (dev_loss, ref_loss)
    worst = []
    for e in st.params:
        lf = leaves[e["name"]]
        ref = np.concatenate([lf[0].grad.numpy().reshape(-1), lf[1].grad.numpy().reshape(-1)]) if e.get("lora") else lf.grad.numpy()
        mx, rms = Q.grad_deviation(e["g"], ref)
        worst.append((round(mx, 4), round(rms, 5), e["name"]))
        rms_tol = 2.0 ** -6 if e["name"].endswith(("qn", "kn")) else 2.0 ** -7   # the bars of tests/test_gpu_qwen3_step.py, its 64-element q/k-norm weights included
        assert mx <= 2.0 ** -5 and rms <= rms_tol, "%s: max %.4f rms %.5f of scale" % (e["name"], mx, rms)
    print("largest gradient deviations (max, rms, tensor):", sorted(worst, reverse=True)[:3])
    print("largest adapter deviation:", max(w for w in worst if w[2] in {e["name"] for _, e in le}))
    # ---- update: the adapters move by AdamW's rule, the base blobs stay byte for byte, everything else trains as under "weights"
    frozen = [e["blob"].blob.cpu().numpy().copy() for _, e in le]
    others = [u16(e["p"]).copy() for e in st.params if not e.get("lora")]
    before = _snapshot(st)
    assert all(g.any() for _, g, _, _ in before), "every adapter received a gradient"
    st.update(**HP)
    ctx.sync()
    assert st.t == 1
    _oracle_adamw_on_adapters(st, before, 1)
    for (_, e), f in zip(le, frozen):
        assert np.array_equal(e["blob"].blob.cpu().numpy(), f), "the frozen base of %s changed" % e["name"]
    assert all(not np.array_equal(u16(e["p"]), o) for e, o in zip([e for e in st.params if not e.get("lora")], others))
    # ---- the loss falls over three forwards on one batch
    seen = [dev_loss]
    for _ in range(2):
        st.forward(d_ids, d_tgt)
        ctx.sync()
        seen.append(float(st.losses.mean()))
        st.backward()
        st.update(**HP)
    print("losses on one batch:", seen)
    assert seen[2] < seen[1] < seen[0], seen
    for (_, e), f in zip(le, frozen):
        assert np.array_equal(e["blob"].blob.cpu().numpy(), f), e["name"]
    st.close()


def test_lora_default_init_muon_arena_and_as_model(ctx):
    """b = 0 at the start: gA is exactly zero and gB is not; under set_optimizer("muon") the adapters stay on AdamW while q, k, v, up go to kf_muon; a context that
    holds a dequant arena is accepted (the base never changes); as_model refuses with the reason"""
    targets = ("o", "gate", "down")
    arena = torch.empty(1 << 20, dtype=torch.uint8, device=ctx.device)
    L.check(ctx.hip.kf_set_dequant_arena(ctx.h, arena.data_ptr(), arena.numel()), "kf_set_dequant_arena")
    try:
        st, ids, tgt = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, lora_targets=targets)
        d_ids, d_tgt = _dev(ctx, ids, tgt)
        st.set_optimizer("muon")
        st.forward(d_ids, d_tgt)
        st.backward()
        ctx.sync()
    finally:
        L.check(ctx.hip.kf_set_dequant_arena(ctx.h, None, 0), "kf_set_dequant_arena")
    assert np.isfinite(float(st.losses.mean()))
    le = _lora_entries(st)
    assert sorted({e["name"].split(".")[1] for _, e in le}) == sorted(targets) and len(le) == 3 * Q.CFG["n_layer"]
    for _, e in le:
        r, IC = e["rank"], e["blob"].ne1
        a, b = st.lora_state()[e["name"]]
        assert a.shape == (r, IC) and u16(a).any() and not u16(b).any()
        g = u16(e["g"])
        assert not g[:r * IC].any() and g[r * IC:].any(), e["name"]
    with pytest.raises(L.KFError, match="adapters"):
        st.as_model(128)
    before = _snapshot(st)
    st.update(**HP)
    ctx.sync()
    _oracle_adamw_on_adapters(st, before, 1)
    muon = [e for e in st.params if e["name"].endswith(("q.w", "k.w", "v.w", "up.w"))]
    assert len(muon) == 4 * Q.CFG["n_layer"] and all(not u16(e["v"]).any() and u16(e["m"]).any() for e in muon)   # kf_muon: momentum in m, v never touched
    st.close()


def test_lora_global_clip_norms(ctx):
    st, ids, tgt = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters=_adapters())
    d_ids, d_tgt = _dev(ctx, ids, tgt)
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    grads = [u16(e["g"]).copy() for e in st.params]
    _, gn = G.norms(grads)
    c = float(np.median(gn[:-1])) / 2
    scale = G.scales(gn, G.GLOBAL, c)
    before = _snapshot(st)
    st.set_grad_clip(c, "global")
    st.update(**HP)
    ctx.sync()
    got = st.grad_norms()
    assert np.array_equal(got.view(np.uint32), gn[:-1].view(np.uint32)) and np.float32(st.grad_norm()).view(np.uint32) == gn[-1].view(np.uint32)
    assert scale[0] < 1.0
    _oracle_adamw_on_adapters(st, before, 1, scale)
    st.close()


def test_lora_state_and_merged_masters_round_trip(ctx):
    st, ids, tgt = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters=_adapters())
    d_ids, d_tgt = _dev(ctx, ids, tgt)
    st.forward(d_ids, d_tgt)
    ctx.sync()
    losses = st.losses.clone()
    # lora_state() -> adapters=: the same forward, bit for bit
    again, _, _ = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters={k: (a.cpu().clone(), b.cpu().clone()) for k, (a, b) in st.lora_state().items()})
    again.forward(d_ids, d_tgt)
    ctx.sync()
    assert np.array_equal(losses.cpu().numpy().view(np.uint32), again.losses.cpu().numpy().view(np.uint32))
    # merged_masters() -> a plain bf16 model: the same loss to 2^-7
    plain = Qwen3Step(ctx, Q.CFG, Q.Bn, Q.T, masters=st.merged_masters(), types={k: L.BF16 for k in Q3_MATS})
    assert not any(e.get("lora") for e in plain.params)
    plain.forward(d_ids, d_tgt)
    ctx.sync()
    a_, b_ = float(losses.mean()), float(plain.losses.mean())
    print("loss: adapters %.6f, merged %.6f" % (a_, b_))
    assert abs(a_ - b_) <= 2.0 ** -7 * a_
    for s_ in (st, again, plain):
        s_.close()
