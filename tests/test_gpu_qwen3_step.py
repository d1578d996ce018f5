"""koifish_amd.train_step.Qwen3Step (koifish::Qwen3Trainer): the Qwen3 family's training step as ONE loop, at the toy shape of tests/qwen3_toy.py, against torch fp64
autograd on the dequantised blobs and the oracle's AdamW / quantiser restatements.  Gradient bars are those of
tests/test_gpu_train_step.py::test_qwen3_toy_training_step_vs_autograd: loss within 2^-7 relative, max <= 2^-5 and rms <= 2^-7 of the tensor's largest reference
magnitude (rms 2^-6 for the 64-element q/k-norm weights)."""
import ctypes as C
import json
import struct

import numpy as np
import pytest
import torch

import gama_ref
import muon_restate as R
from koifish_amd import lib as L
from koifish_amd.runtime import Qwen3
from koifish_amd.train_step import Q3_MATS
from oracle import oracle as O
from tests.conftest import u16
from tests.qwen3_toy import CFG, HP, N, V, Vp, grad_deviation, make, ref_logits, ref_loss, torch_params

pytestmark = pytest.mark.gpu
MU = dict(lr_scale=50.0, mui=0.95, eps=1e-7, tp_decay=1)
NL = CFG["n_layer"]
ORDER = ["l%d.%s" % (l, k) for l in range(NL) for k in ("q.w", "k.w", "v.w", "o.w", "gate.w", "up.w", "down.w", "n1", "n2", "qn", "kn")] + ["wte", "nf"]


def _dev_ids(ctx, ids, tgt):
    return torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device)


def _check_grads(st, leaves):
    worst = []
    for e in st.params:
        lf = leaves[e["name"]]
        ref = np.concatenate([lf[0].grad.numpy(), lf[1].grad.numpy()]) if e.get("gama") else lf.grad.numpy()
        mx, rms = grad_deviation(e["g"], ref)
        worst.append((round(mx, 4), round(rms, 5), e["name"]))
        rms_tol = 2.0 ** -6 if e["name"].endswith(("qn", "kn")) else 2.0 ** -7
        assert mx <= 2.0 ** -5 and rms <= rms_tol, "%s: max %.4f rms %.5f of scale" % (e["name"], mx, rms)
    print("largest gradient deviations (max, rms, tensor):", sorted(worst, reverse=True)[:3])


def _check_adamw(e, i, before, t):
    p, g, m, v = (a.reshape(-1).copy() for a in before)
    b1c, b2c = 1.0 - HP["beta1"] ** t, 1.0 - HP["beta2"] ** t
    assert O.adamw(p, g, m, v, HP["lr"], HP["beta1"], HP["beta2"], b1c, b2c, HP["eps"], HP["wd"] if e["wd"] else 0.0, 1.0, (HP["seed"] + 7919 * t + i) & 0xFFFFFFFF) == 0
    assert np.array_equal(u16(e["p"]).reshape(-1), p), "step %d: master %s differs from the oracle's AdamW" % (t, e["name"])
    assert np.array_equal(u16(e["m"]).reshape(-1), m) and np.array_equal(u16(e["v"]).reshape(-1), v), e["name"]


def _check_blob(e):
    if e["type"] == L.Q4 and not e.get("gama"):   # the blob the next forward reads = the oracle's quantiser on the updated master
        ne0, ne1 = e["p"].shape
        ow = O.quantize(u16(e["p"]).reshape(ne0, ne1), ne0, ne1, e["type"])
        assert np.array_equal(e["blob"].blob.cpu().numpy(), np.frombuffer(ow.blob(), dtype=np.uint8)), "blob of %s" % e["name"]


def _snapshot(st):
    return [tuple(u16(e[k]).copy() for k in ("p", "g", "m", "v")) for e in st.params]


def test_forward_backward_vs_autograd(ctx):
    st, ids, tgt = make(ctx)
    assert [e["name"] for e in st.params] == ORDER
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    P, leaves = torch_params(ctx, st)
    loss = ref_loss(P, ids, tgt)
    loss.backward()
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    ref, dev_loss = float(loss.detach()), float(st.losses.mean())
    print("loss: device %.6f fp64 %.6f" % (dev_loss, ref))
    assert abs(dev_loss - ref) <= 2.0 ** -7 * ref
    _check_grads(st, leaves)
    st.close()


def test_two_consecutive_steps_with_update(ctx):
    """as tests/test_gpu_train_step.py::test_gpt2_two_consecutive_steps_with_update: per step the loss against fp64 on the blobs the step read; after each update every
    master and both moments equal the oracle's AdamW on the device's own gradients bit for bit, every gradient is zeroed, every blob equals the oracle's quantiser on
    the updated master byte for byte; the loss falls over three forwards on one batch."""
    st, ids, tgt = make(ctx)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    losses = []
    for step in range(3):
        P, _ = torch_params(ctx, st)
        ref = float(ref_loss(P, ids, tgt).detach())
        st.forward(d_ids, d_tgt)
        ctx.sync()
        dev_loss = float(st.losses.mean())
        assert abs(dev_loss - ref) <= 2.0 ** -7 * ref, "step %d: loss %.5f vs fp64 %.5f" % (step, dev_loss, ref)
        losses.append(dev_loss)
        if step == 2:
            break
        st.backward()
        ctx.sync()
        before = _snapshot(st)
        st.update(**HP)
        ctx.sync()
        assert all(g.any() for _, g, _, _ in before), "every tensor received a gradient"
        t = st.t
        assert t == step + 1
        for i, (e, b4) in enumerate(zip(st.params, before)):
            _check_adamw(e, i, b4, t)
            assert not u16(e["g"]).any() and not np.array_equal(u16(e["p"]), b4[0]), e["name"]
            _check_blob(e)
    assert losses[1] < losses[0] and losses[2] < losses[1], losses
    print("toy losses over three forwards on one batch:", ["%.4f" % v for v in losses])
    # step() is forward + backward + update in one call: a twin stepped twice holds the same bits
    tw, _, _ = make(ctx)
    tw.step(d_ids, d_tgt, **HP)
    tw.step(d_ids, d_tgt, **HP)
    ctx.sync()
    for a, b in zip(st.params, tw.params):
        assert np.array_equal(u16(a["p"]), u16(b["p"])) and np.array_equal(u16(a["m"]), u16(b["m"])), a["name"]
        if a["blob"] is not None:
            assert torch.equal(a["blob"].blob, b["blob"].blob), a["name"]
    st.close()
    tw.close()


def test_gama_step(ctx):
    st, ids, tgt = make(ctx, train_target="gama")
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    ge = [(i, e) for i, e in enumerate(st.params) if e.get("gama")]
    assert [e["name"] for _, e in ge] == ["l%d.%s.w" % (l, k) for l in range(NL) for k in Q3_MATS]
    for _, e in ge:
        b = e["blob"]
        assert all(e[k].numel() == 2 * b.nGroup for k in ("p", "g", "m", "v")) and not e["wd"]
        assert e["p"].data_ptr() == b.blob.data_ptr() + b.szData + 2 * (b.ne0 + b.ne1)
    P, leaves = torch_params(ctx, st)
    loss = ref_loss(P, ids, tgt)
    loss.backward()
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    ref, dev_loss = float(loss.detach()), float(st.losses.mean())
    assert abs(dev_loss - ref) <= 2.0 ** -7 * ref, (dev_loss, ref)
    _check_grads(st, leaves)   # every (zero, step) gradient against autograd: the bounds of tests/test_gpu_gama_step.py
    # against tests/gama_ref.py: the expectation needs the two operands the device's LinBack multiplied.  The input activations are kept per layer, but the gradient
    # operands are buffers the whole backward shares, and backward() is one call: after it they hold what the LAST layer run wrote, layer 0.  There dq_raw, dk_raw, dv,
    # d(gate) and d(up) survive (o's and down's operand is dx, which the norm backward behind them adds into), so layer 0's q, k, v, gate, up are checked here; the other
    # nine gama tensors have the autograd check above, which is independent of the device's operands and carries the same bounds.
    f = lambda t_: O.bf16_to_f32(u16(t_)).astype(np.float64)
    for k, dIn, inp in (("q", st.dqr, "h1"), ("k", st.dkr, "h1"), ("v", st.dvd, "h1"), ("gate", st.dgate, "h2"), ("up", st.dact, "h2")):
        e = st.layers[0][k]
        b = e["blob"]
        qmb = O.unpack(b.blob[:b.szData].cpu().numpy(), L.BITS[b.type]).astype(np.float64).reshape(b.ne0, b.ne1) - b.qBias
        want, A = gama_ref.gama_grads(f(dIn), f(st.A[0][inp]), qmb)
        got = f(e["g"])
        assert (np.abs(got - want) <= gama_ref.bound(want, A, N)).all(), "l0.%s" % k
    frozen = [e["blob"].blob[:e["blob"].szData + 2 * (e["blob"].ne0 + e["blob"].ne1)].cpu().numpy().copy() for _, e in ge]
    before = _snapshot(st)
    assert all(g.any() for _, g, _, _ in before)
    st.update(**HP)
    ctx.sync()
    for (i, e), fz in zip(ge, frozen):
        b = e["blob"]
        assert np.array_equal(b.blob[:b.szData + 2 * (b.ne0 + b.ne1)].cpu().numpy(), fz), "packed integers / scales of %s changed" % e["name"]
        p, g, m, v = (a.copy() for a in before[i])
        assert O.adamw(p, g, m, v, HP["lr"], HP["beta1"], HP["beta2"], 1.0 - HP["beta1"], 1.0 - HP["beta2"], HP["eps"], 0.0, 1.0, (HP["seed"] + 7919 + i) & 0xFFFFFFFF) == 0
        assert np.array_equal(u16(e["p"]), p) and not np.array_equal(p, before[i][0]) and not u16(e["g"]).any(), e["name"]
    st.close()
    # a context that holds a dequant arena is refused, with a reason
    arena = torch.empty(1 << 20, dtype=torch.uint8, device=ctx.device)
    L.check(ctx.hip.kf_set_dequant_arena(ctx.h, arena.data_ptr(), arena.numel()), "kf_set_dequant_arena")
    try:
        with pytest.raises(L.KFError, match="dequant arena"):
            make(ctx, train_target="gama")
        st2, _, _ = make(ctx)   # "weights" does not mind
        gq = st2.layers[0]["q"]
        z = torch.zeros(2 * gq["blob"].nGroup, dtype=torch.bfloat16, device=ctx.device)
        d = gq["blob"].desc()
        assert ctx.host.kfh_qwen3t_set_param_gama(st2.h, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), C.byref(d)) == -20
        assert b"dequant arena" in ctx.host.kfh_qwen3t_last_error()
        st2.close()
    finally:
        L.check(ctx.hip.kf_set_dequant_arena(ctx.h, None, 0), "kf_set_dequant_arena")


def test_muon_switch(ctx):
    st, ids, tgt = make(ctx)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    st.set_optimizer("muon", **MU)
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    before = _snapshot(st)
    st.update(**HP)
    ctx.sync()
    # which optimiser a tensor took, read back from its moment buffers: kf_muon leaves v alone
    took_muon = [e["name"] for e in st.params if not u16(e["v"]).any()]
    assert took_muon == ["l%d.%s.w" % (l, k) for l in range(NL) for k in ("q", "k", "v", "gate", "up")]
    for i, (e, b4) in enumerate(zip(st.params, before)):
        assert not u16(e["g"]).any() and u16(e["m"]).any() and not np.array_equal(u16(e["p"]), b4[0]), e["name"]
        if e["name"] not in took_muon:
            _check_adamw(e, i, b4, 1)
        _check_blob(e)
    # one Muon tensor against the numpy restatement, as tests/test_gpu_muon_step.py: mG and the master bit for bit given the device's orthogonalised X
    i = [e["name"] for e in st.params].index("l1.gate.w")
    e, (p0, g0, m0, v0) = st.params[i], before[i]
    ne0, ne1 = e["p"].shape
    seed = (HP["seed"] + 7919 + i) & 0xFFFFFFFF
    m2, x = R.momentum(m0.reshape(-1), g0.reshape(-1), MU["mui"], seed)
    assert np.array_equal(u16(e["m"]).reshape(-1), m2)
    nb = ctx.hip.kf_muon_scratch_bytes(ne0, ne1)
    sc = torch.empty(nb + 256, dtype=torch.uint8, device=ctx.device)
    d_x = torch.from_numpy(x.view(np.int16).copy()).to(ctx.device)
    assert ctx.hip.kf_newton_schulz(ctx.h, d_x.data_ptr(), ne0, ne1, None, MU["eps"], 5, R.A_, R.B_, R.C_, (sc.data_ptr() + 255) & ~255, nb) == 0, ctx.hip.kf_last_error()
    ctx.sync()
    lr_muon, wd_muon = np.float32(HP["lr"]) * np.float32(MU["lr_scale"]), np.float32(HP["wd"]) / np.float32(MU["lr_scale"])
    assert np.array_equal(u16(e["p"]).reshape(-1), R.apply(p0.reshape(-1), d_x.cpu().numpy().view(np.uint16), lr_muon, wd_muon, seed))
    with pytest.raises(ValueError):
        st.set_optimizer("lion")
    st.close()


def test_untied_head(ctx):
    st, ids, tgt = make(ctx, tied=False)
    assert [e["name"] for e in st.params] == ORDER + ["head"]
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    P, leaves = torch_params(ctx, st)
    loss = ref_loss(P, ids, tgt)
    loss.backward()
    st.forward(d_ids, d_tgt)
    st.backward()
    ctx.sync()
    ref, dev_loss = float(loss.detach()), float(st.losses.mean())
    assert abs(dev_loss - ref) <= 2.0 ** -7 * ref
    _check_grads(st, leaves)
    g_wte = u16(st.wte["g"]).reshape(Vp, CFG["dim"])
    unused = np.setdiff1d(np.arange(Vp), ids)
    assert len(unused) and not g_wte[unused].any(), "wte's gradient comes from the embedding rows only"
    assert u16(st.head["g"]).reshape(Vp, CFG["dim"])[unused[unused < V]].any(), "the head has a gradient of its own"
    st.close()


def _scores64(ctx, st, seq):
    """per position t < n - 1: log P(seq[t + 1]) from fp64 logits on the CURRENT dequantised blobs, and the bar of tests/test_gpu_score.py: 2 * 2^-6 * max|logits at t|"""
    P, _ = torch_params(ctx, st)
    with torch.no_grad():
        lg = ref_logits(P, seq, 1, len(seq)).numpy()[:-1]
    m = lg.max(axis=1)
    lse = m + np.log(np.exp(lg - m[:, None]).sum(axis=1))
    return lg[np.arange(len(seq) - 1), seq[1:]] - lse, 2 * 2.0 ** -6 * np.abs(lg).max(axis=1)


def test_as_model_scores_trained_weights_and_round_trips_kun(ctx, tmp_path):
    st, ids, tgt = make(ctx)
    d_ids, d_tgt = _dev_ids(ctx, ids, tgt)
    m = st.as_model(128)
    assert m.weights[(0, 0)].blob.data_ptr() == st.layers[0]["q"]["blob"].blob.data_ptr()   # built ON the trainer's blobs
    seq = ids[:40].copy()
    scores = []
    for rnd in range(2):
        want, bar = _scores64(ctx, st, seq)
        got = m.score(seq).astype(np.float64)
        print("round %d: max |dlp| / bar = %.3f" % (rnd, (np.abs(got - want) / bar).max()))
        assert (np.abs(got - want) <= bar).all(), "round %d: token %d" % (rnd, int(np.argmax(np.abs(got - want) / bar)))
        scores.append(got)
        if rnd == 0:
            st.step(d_ids, d_tgt, **HP)
            ctx.sync()
    assert not np.array_equal(scores[0], scores[1])
    path = tmp_path / "trained.kun"
    m.save_kun(path)
    raw = path.read_bytes()
    hlen = struct.unpack("<Q", raw[:8])[0]
    hdr, data = json.loads(raw[8:8 + hlen]), raw[8 + hlen:]
    hf = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.o_proj", gate="mlp.gate_proj", up="mlp.up_proj", down="mlp.down_proj")
    for l, ly in enumerate(st.layers):
        for k in Q3_MATS:
            d = hdr["model.layers.%d.%s.weight" % (l, hf[k])]
            assert data[d["data_offsets"][0]:d["data_offsets"][1]] == ly[k]["blob"].blob.cpu().numpy().tobytes(), (l, k)
    d = hdr["model.embed_tokens.weight"]
    assert data[d["data_offsets"][0]:d["data_offsets"][1]] == st.wte["blob"].blob[:V * CFG["dim"] * 2].cpu().numpy().tobytes()
    b = Qwen3.from_kun(path)
    assert np.array_equal(b.score(seq), m.score(seq))
    path2 = tmp_path / "again.kun"
    b.save_kun(path2)
    assert path2.read_bytes() == raw
    b.close()
    m.close()
    st.close()
