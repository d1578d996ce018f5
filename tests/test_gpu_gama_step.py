"""GPT2Step(train_target="gama"): the reference's "train_target": "gama" (SLP::Back's gama branch, GTensor::InitGamaParam, PIPE_Adamw on the slice) on the toy GPT-2 of
tests/test_gpu_train_step.py (C 128, H 2, NL 2, V 250, Vp 256, B 2, T 64) -- once with all four block matrices 4-bit, once with the default hybrid (f8e5m2 qkv / proj,
4-bit fc / proj2).  A gama-trained matrix keeps its packed integers; its parameter is the [ZERO][STEP] slice of its blob.

In the torch fp64 model such a weight is  W_deq.detach() + (step Q - zero) - (step Q - zero).detach()  with W_deq the stepwise (bf16-rounded) dequantisation the device
multiplies and Q = q - qBias: the forward value is the device's, the gradient flows to the zero / step leaves.  Gradient bars are those of tests/test_gpu_train_step.py:
max <= 2^-5 and rms <= 2^-7 of the tensor's largest reference magnitude, loss within 2^-7 relative.

Decided here and documented in koifish_amd/train_step.py: with set_optimizer("muon") a gama tensor keeps AdamW (the step runs, the slices move by AdamW's rule); a context
that holds a dequant arena is refused with a reason."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from koifish_amd.train_step import GPT2Step, MATS
from oracle import oracle as O
from tests.conftest import u16
from tests.test_gpu_train_step import _ref_loss_fp64

pytestmark = pytest.mark.gpu

Cn, H, NL, V, Vp, Bn, T = 128, 2, 2, 250, 256, 2, 64
N = Bn * T
HP = dict(lr=2e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1, seed=99)
ALL_Q4 = dict(qkv=L.Q4, proj=L.Q4, fc=L.Q4, proj2=L.Q4)
F64 = lambda a_u16: torch.tensor(O.bf16_to_f32(a_u16).astype(np.float64))


def make(ctx, types, seed=303, **kw):
    rng = np.random.default_rng(seed)
    bf = lambda a: torch.from_numpy(O.f32_to_bf16(a.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    mk = lambda *s, std=0.08: bf(rng.normal(0, std, size=s))
    lnw = lambda: bf(1 + rng.normal(0, 0.1, Cn))
    shapes = dict(qkv=(3 * Cn, Cn), proj=(Cn, Cn), fc=(4 * Cn, Cn), proj2=(Cn, 4 * Cn))
    wte = torch.zeros(Vp, Cn, dtype=torch.bfloat16)
    wte[:V] = mk(V, Cn, std=0.2)
    masters = dict(wte=wte, wpe=mk(T, Cn, std=0.05), lnf=(lnw(), mk(Cn)),
                   blocks=[dict({k: (mk(*shapes[k]), mk(shapes[k][0])) for k in MATS}, ln=(lnw(), mk(Cn), lnw(), mk(Cn))) for _ in range(NL)])
    ids, tgt = rng.integers(0, V, N).astype(np.int32), rng.integers(0, V, N).astype(np.int32)
    return GPT2Step(ctx, Cn, H, NL, V, Vp, Bn, T, types=types, masters=masters, **kw), ids, tgt


def key_of(name):
    return name.replace("h", "", 1) if name.startswith("h") and name[1].isdigit() else name


def torch_params(ctx, st):
    """the fp64 model's parameters as the step's forward reads them; for a gama entry the leaves are (zero, step)"""
    P, leaves = {}, {}
    for e in st.params:
        k = key_of(e["name"])
        if e.get("gama"):
            b = e["blob"]
            Q = torch.tensor((O.unpack(b.blob[:b.szData].cpu().numpy(), L.BITS[b.type]).astype(np.float64) - b.qBias).reshape(b.nGroup, 128))
            zs = F64(u16(e["p"]))
            zero, step = zs[:b.nGroup].clone().requires_grad_(True), zs[b.nGroup:].clone().requires_grad_(True)
            lin = (step[:, None] * Q - zero[:, None]).reshape(b.ne0, b.ne1)
            P[k] = F64(u16(ctx.dequant(b))).reshape(b.ne0, b.ne1) + lin - lin.detach()   # kf_dequant is bit-exact against the oracle (tests/test_gpu_ops.py)
            leaves[e["name"]] = (zero, step)
        elif e["type"] in (L.F8E5M2, L.Q4):
            P[k] = F64(u16(ctx.dequant(e["blob"]))).reshape(tuple(e["p"].shape)).requires_grad_(True)
            leaves[e["name"]] = P[k]
        else:
            P[k] = F64(u16(e["p"])).reshape(tuple(e["p"].shape)).requires_grad_(True)
            leaves[e["name"]] = P[k]
    return P, leaves


def gama_entries(st):
    return [(i, e) for i, e in enumerate(st.params) if e.get("gama")]


def oracle_adamw_on_slices(st, before, t):
    """[ZERO][STEP] of every gama entry == the oracle's CU_adamw on the read-back device gradient with the trainer's seed rule, no weight decay; gradients zeroed"""
    b1c, b2c = 1.0 - HP["beta1"] ** t, 1.0 - HP["beta2"] ** t
    for (i, e), (p0, g0, m0, v0) in zip(gama_entries(st), before):
        p, g, m, v = (a.copy() for a in (p0, g0, m0, v0))
        assert O.adamw(p, g, m, v, HP["lr"], HP["beta1"], HP["beta2"], b1c, b2c, HP["eps"], 0.0, 1.0, (HP["seed"] + 7919 * t + i) & 0xFFFFFFFF) == 0
        assert np.array_equal(u16(e["p"]), p), "gama slice of %s differs from the oracle's AdamW" % e["name"]
        assert np.array_equal(u16(e["m"]), m) and np.array_equal(u16(e["v"]), v), e["name"]
        assert not u16(e["g"]).any() and not np.array_equal(p, p0), e["name"]


def snapshot(st):
    return [tuple(u16(e[k]).copy() for k in ("p", "g", "m", "v")) for _, e in gama_entries(st)]


@pytest.mark.parametrize("types,n_gama", [(ALL_Q4, 4 * NL), (None, 2 * NL)], ids=["all_q4", "hybrid"])
def test_gama_step_gradients_update_and_no_stale_weights(ctx, types, n_gama):
    st, ids, tgt = make(ctx, types, train_target="gama")
    d_ids, d_tgt = torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device)
    ge = gama_entries(st)
    assert len(ge) == n_gama
    # the memory claim: no master, no [OC, IC] gradient, no moments of that size
    for _, e in ge:
        b = e["blob"]
        assert all(e[k].numel() == 2 * b.nGroup for k in ("p", "g", "m", "v")) and not e["wd"]
        assert e["p"].data_ptr() == b.blob.data_ptr() + b.szData + 2 * (b.ne0 + b.ne1)
    for e in st.params:   # everything else trains as under "weights"
        if not e.get("gama"):
            assert e["g"].shape == e["p"].shape
    # ---- forward + backward against autograd
    P, leaves = torch_params(ctx, st)
    loss = _ref_loss_fp64(Cn, H, NL, V, Bn, T, P, ids, tgt)
    loss.backward()
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    ref_loss, dev_loss = float(loss.detach()), float(st.losses.mean())
    assert abs(dev_loss - ref_loss) <= 2.0 ** -7 * ref_loss, (dev_loss, ref_loss)
    worst = []
    for e in st.params:
        lf = leaves[e["name"]]
        ref = np.concatenate([lf[0].grad.numpy(), lf[1].grad.numpy()]) if e.get("gama") else lf.grad.numpy()
        got = O.bf16_to_f32(u16(e["g"])).astype(np.float64).reshape(ref.shape)
        sc_ = np.abs(ref).max()
        mx, rms = np.abs(got - ref).max() / sc_, np.sqrt(((got - ref) ** 2).mean()) / sc_
        worst.append((round(float(mx), 4), round(float(rms), 5), e["name"]))
        assert mx <= 2.0 ** -5 and rms <= 2.0 ** -7, "%s: max %.4f rms %.4f of scale" % (e["name"], mx, rms)
    print("largest gradient deviations (max, rms, tensor):", sorted(worst, reverse=True)[:3])
    print("largest gama deviation:", max(w for w in worst if w[2] in {e["name"] for _, e in ge}))
    # ---- update: the integers and the R / C scales stay, the slice moves by AdamW's rule
    frozen = [e["blob"].blob[:e["blob"].szData + 2 * (e["blob"].ne0 + e["blob"].ne1)].cpu().numpy().copy() for _, e in ge]
    others = [u16(e["p"]).copy() for e in st.params if not e.get("gama")]
    before = snapshot(st)
    assert all(g.any() for _, g, _, _ in before), "every gama slice received a gradient"
    st.update(**HP)
    ctx.sync()
    assert st.t == 1
    oracle_adamw_on_slices(st, before, 1)
    for (_, e), f in zip(ge, frozen):
        assert np.array_equal(e["blob"].blob[:len(f)].cpu().numpy(), f), "packed bytes / R, C scales of %s changed" % e["name"]
    assert all(not np.array_equal(u16(e["p"]), o) for e, o in zip([e for e in st.params if not e.get("gama")], others)), "the other tensors train as before"
    # ---- no stale weights: two more steps, then a forward equals a fresh trainer built from the read-back blobs and parameters, bit for bit
    st.step(d_ids, d_tgt, **HP)
    st.step(d_ids, d_tgt, **HP)
    st.forward(d_ids, d_tgt)
    ctx.sync()
    losses = st.losses.clone()
    fresh, _, _ = make(ctx, types, seed=909, train_target="gama")
    for a, b in zip(st.params, fresh.params):
        assert a["name"] == b["name"] and bool(a.get("gama")) == bool(b.get("gama"))
        if a["blob"] is not None:
            b["blob"].blob.copy_(a["blob"].blob)   # a gama entry's p lives inside its blob; a bf16 "blob" is the master itself
        if not a.get("gama") and a["type"] != L.BF16:
            b["p"].copy_(a["p"])
    fresh.forward(d_ids, d_tgt)
    ctx.sync()
    assert np.array_equal(losses.cpu().numpy().view(np.uint32), fresh.losses.cpu().numpy().view(np.uint32))
    assert float(losses.mean()) < dev_loss, "three updates on one batch lower its loss"
    st.close()
    fresh.close()


def test_muon_leaves_gama_tensors_to_adamw(ctx):
    """the hybrid: qkv / proj (f8e5m2, ne0 >= ne1) go to kf_muon, the gama-trained fc / proj2 slices keep kf_adamw"""
    st, ids, tgt = make(ctx, None, train_target="gama")
    st.set_optimizer("muon")
    d_ids, d_tgt = torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device)
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    before = snapshot(st)
    st.update(**HP)
    ctx.sync()
    oracle_adamw_on_slices(st, before, 1)
    assert all(not u16(e["v"]).any() and u16(e["m"]).any() for e in st.params if e["name"].endswith(("qkv.w", "proj.w")))   # kf_muon: momentum in m, v never touched
    # every matrix gama-trained: no Muon tensor is left, the switch is still accepted and the step runs
    st2, _, _ = make(ctx, ALL_Q4, train_target="gama")
    st2.set_optimizer("muon")
    st2.forward(d_ids, d_tgt)
    st2.backward()
    ctx.sync()
    before = snapshot(st2)
    st2.update(**HP)
    ctx.sync()
    oracle_adamw_on_slices(st2, before, 1)
    st.close()
    st2.close()


def test_dequant_arena_is_refused_with_a_reason(ctx):
    """resident dequantised copies of a gama-trained matrix would go stale with every update: the combination is refused, "weights" mode is not affected"""
    st, ids, tgt = make(ctx, ALL_Q4, train_target="gama")
    d_ids, d_tgt = torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device)
    arena = torch.empty(1 << 20, dtype=torch.uint8, device=ctx.device)
    assert ctx.hip.kf_dequant_arena_bytes(ctx.h) == 0
    L.check(ctx.hip.kf_set_dequant_arena(ctx.h, arena.data_ptr(), arena.numel()), "kf_set_dequant_arena")
    try:
        assert ctx.hip.kf_dequant_arena_bytes(ctx.h) == arena.numel()
        with pytest.raises(L.KFError, match="dequant arena"):
            st.forward(d_ids, d_tgt)
        with pytest.raises(L.KFError, match="dequant arena"):
            st.step(d_ids, d_tgt, **HP)
        with pytest.raises(L.KFError, match="dequant arena"):
            make(ctx, ALL_Q4, train_target="gama")
        assert ctx.host.kfh_gpt2_forward(st.h, d_ids.data_ptr(), d_tgt.data_ptr()) == -20   # the sequencer itself refuses too
    finally:
        L.check(ctx.hip.kf_set_dequant_arena(ctx.h, None, 0), "kf_set_dequant_arena")
    st.forward(d_ids, d_tgt)
    ctx.sync()
    assert np.isfinite(float(st.losses.mean()))
    with pytest.raises(ValueError):
        make(ctx, ALL_Q4, train_target="zero")
    st.close()
