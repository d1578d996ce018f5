"""GPT2Step with the optimiser switch (kfh_gpt2_set_optimizer): "muon" routes a block's qkv / proj / fc matrices (ne0 >= ne1) through kf_muon and leaves proj2, the
embeddings, biases and norms on kf_adamw; the default stays AdamW on everything, bit for bit.

The toy is C = 128, H = 2, NL = 2, V = Vp = 128, B = 2, T = 64 -- the smallest shape the step's other operators take (the attention tiles need head_dim 64 or 128,
kf_linear_backward needs OC >= 128 and n >= 128 rows), with the hybrid f8 / 4-bit types of tests/test_gpu_train_step.py."""
import numpy as np
import pytest
import torch

import muon_restate as R
from tests.conftest import u16
from koifish_amd import lib as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu

Cn, H, NL, V, Vp, Bn, T = 128, 2, 2, 128, 128, 2, 64
HP = dict(lr=2e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1, seed=99)
MU = dict(lr_scale=50.0, mui=0.95, eps=1e-7, tp_decay=1)
QUANT = (L.F8E5M2, L.Q4)


def _toy(ctx):
    from koifish_amd.train_step import GPT2Step, MATS
    rng = np.random.default_rng(404)
    bf = lambda a: torch.from_numpy(O.f32_to_bf16(a.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    mk = lambda *s, std=0.08: bf(rng.normal(0, std, size=s))
    lnw = lambda: bf(1 + rng.normal(0, 0.1, Cn))
    shapes = dict(qkv=(3 * Cn, Cn), proj=(Cn, Cn), fc=(4 * Cn, Cn), proj2=(Cn, 4 * Cn))
    masters = dict(wte=mk(Vp, Cn, std=0.2), wpe=mk(T, Cn, std=0.05), lnf=(lnw(), mk(Cn)),
                   blocks=[dict({k: (mk(*shapes[k]), mk(shapes[k][0])) for k in MATS}, ln=(lnw(), mk(Cn), lnw(), mk(Cn))) for _ in range(NL)])
    st = GPT2Step(ctx, Cn, H, NL, V, Vp, Bn, T, masters=masters)
    ids = torch.from_numpy(rng.integers(0, V, Bn * T).astype(np.int32)).to(ctx.device)
    tgt = torch.from_numpy(rng.integers(0, V, Bn * T).astype(np.int32)).to(ctx.device)
    return st, ids, tgt


def _is_muon(e):
    return e["name"].startswith("h") and e["name"].endswith(".w") and e["p"].dim() == 2 and e["name"].split(".")[1] in ("qkv", "proj", "fc", "proj2") and e["p"].shape[0] >= e["p"].shape[1]


def _check_adamw(e, i, before, t, step):
    p, g, m, v = (a.reshape(-1).copy() for a in before)
    b1c, b2c = 1.0 - HP["beta1"] ** t, 1.0 - HP["beta2"] ** t
    assert O.adamw(p, g, m, v, HP["lr"], HP["beta1"], HP["beta2"], b1c, b2c, HP["eps"], HP["wd"] if e["wd"] else 0.0, 1.0, (HP["seed"] + 7919 * t + i) & 0xFFFFFFFF) == 0
    assert np.array_equal(u16(e["p"]).reshape(-1), p), "step %d: master %s differs from the oracle's AdamW" % (step, e["name"])
    assert np.array_equal(u16(e["m"]).reshape(-1), m) and np.array_equal(u16(e["v"]).reshape(-1), v), e["name"]


def _check_blob(e, step):
    if e["type"] in QUANT:   # the blob the next forward reads = the oracle's quantiser on the updated master
        ne0, ne1 = e["p"].shape
        ow = O.quantize(u16(e["p"]).reshape(ne0, ne1), ne0, ne1, e["type"])
        assert np.array_equal(e["blob"].blob.cpu().numpy(), np.frombuffer(ow.blob(), dtype=np.uint8)), "step %d: blob of %s" % (step, e["name"])


def test_two_steps_with_muon(ctx):
    """Two consecutive steps on one batch.  After each: every AdamW-routed tensor equals the oracle's AdamW on the device's own gradients, bit for bit; every Muon
    tensor's mG (its m buffer) and master equal the numpy momentum / apply restatement given the device's gradients and the device's orthogonalised X (a second
    kf_newton_schulz run on the restated momentum output: the entry is deterministic, which is asserted); v of a Muon tensor is untouched; every gradient is
    zeroed; every re-quantised blob equals the oracle's quantiser on the updated master."""
    st, ids, tgt = _toy(ctx)
    st.set_optimizer("muon", **MU)
    muon = [e["name"] for e in st.params if _is_muon(e)]
    assert muon == ["h%d.%s.w" % (l, k) for l in range(NL) for k in ("qkv", "proj", "fc")]
    hip = ctx.hip
    for step in range(2):
        st.forward(ids, tgt)
        st.backward()
        ctx.sync()
        before = [(u16(e["p"]).copy(), u16(e["g"]).copy(), u16(e["m"]).copy(), u16(e["v"]).copy()) for e in st.params]
        assert all(g.any() for _, g, _, _ in before), "every tensor received a gradient"
        st.update(**HP)
        ctx.sync()
        t = st.t
        assert t == step + 1
        for i, (e, (p0, g0, m0, v0)) in enumerate(zip(st.params, before)):
            assert not u16(e["g"]).any(), e["name"]
            assert not np.array_equal(u16(e["p"]), p0), "%s did not move" % e["name"]
            if not _is_muon(e):
                _check_adamw(e, i, (p0, g0, m0, v0), t, step)
                _check_blob(e, step)
                continue
            ne0, ne1 = e["p"].shape
            n, seed = ne0 * ne1, (HP["seed"] + 7919 * t + i) & 0xFFFFFFFF
            m2, x = R.momentum(m0.reshape(-1), g0.reshape(-1), MU["mui"], seed)
            assert np.array_equal(u16(e["m"]).reshape(-1), m2), "step %d: mG of %s" % (step, e["name"])
            assert np.array_equal(u16(e["v"]), v0), "v of the Muon tensor %s was touched" % e["name"]
            nb = hip.kf_muon_scratch_bytes(ne0, ne1)
            sc = torch.empty(nb + 256, dtype=torch.uint8, device=ctx.device)
            sp = (sc.data_ptr() + 255) & ~255
            xs = []
            for _ in range(2):
                d_x = torch.from_numpy(x.view(np.int16).copy()).to(ctx.device)
                assert hip.kf_newton_schulz(ctx.h, d_x.data_ptr(), ne0, ne1, None, MU["eps"], 5, R.A_, R.B_, R.C_, sp, nb) == 0, hip.kf_last_error()
                ctx.sync()
                xs.append(d_x.cpu().numpy().view(np.uint16))
            assert np.array_equal(xs[0], xs[1]), "kf_newton_schulz is not deterministic"
            lr_muon, wd_muon = np.float32(HP["lr"]) * np.float32(MU["lr_scale"]), np.float32(HP["wd"]) / np.float32(MU["lr_scale"])
            assert np.array_equal(u16(e["p"]).reshape(-1), R.apply(p0.reshape(-1), xs[0], lr_muon, wd_muon, seed)), "step %d: master of %s" % (step, e["name"])
            _check_blob(e, step)
    st.close()


def test_default_optimizer_is_unchanged(ctx):
    """a GPT2Step nobody switched, and one switched to "muon" and back, give what kf_adamw applied directly gives: masters, both moments, blobs, bit for bit"""
    for switch_back in (False, True):
        st, ids, tgt = _toy(ctx)
        if switch_back:
            st.set_optimizer("muon", **MU)
            st.set_optimizer("adamw")
        st.forward(ids, tgt)
        st.backward()
        ctx.sync()
        direct = [tuple(a.clone() for a in (e["p"], e["g"], e["m"], e["v"])) for e in st.params]
        st.update(**HP)
        b1c, b2c = 1.0 - HP["beta1"], 1.0 - HP["beta2"]
        for i, (e, (p, g, m, v)) in enumerate(zip(st.params, direct)):
            L.check(ctx.hip.kf_adamw(ctx.h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), L.BF16, HP["lr"], HP["beta1"], HP["beta2"], b1c, b2c, HP["eps"],
                                     HP["wd"] if e["wd"] else 0.0, 1.0, (HP["seed"] + 7919 + i) & 0xFFFFFFFF, None), "kf_adamw")
        ctx.sync()
        for e, (p, g, m, v) in zip(st.params, direct):
            assert np.array_equal(u16(e["p"]), u16(p)) and np.array_equal(u16(e["m"]), u16(m)) and np.array_equal(u16(e["v"]), u16(v)), e["name"]
            assert not u16(e["g"]).any() and u16(e["v"]).any()
            _check_blob(e, 0)
        st.close()


def test_set_optimizer_refusals(ctx):
    st, ids, tgt = _toy(ctx)
    host, hip = ctx.host, ctx.hip
    nb = max(hip.kf_muon_scratch_bytes(a, b) for a, b in ((3 * Cn, Cn), (Cn, Cn), (4 * Cn, Cn)))
    sc = torch.empty(nb + 256, dtype=torch.uint8, device=ctx.device)
    sp = (sc.data_ptr() + 255) & ~255
    assert host.kfh_gpt2_set_optimizer(st.h, 1, 50.0, 0.95, 1e-7, 1, sp, nb - 1) == -20    # a scratch one byte short of the largest Muon tensor's
    assert host.kfh_gpt2_set_optimizer(st.h, 1, 50.0, 0.95, 1e-7, 1, None, nb) == -20
    assert host.kfh_gpt2_set_optimizer(st.h, 2, 50.0, 0.95, 1e-7, 1, sp, nb) == -20        # no such method
    assert host.kfh_gpt2_set_optimizer(st.h, 1, 50.0, 0.95, 1e-7, 1, sp, nb) == 0
    with pytest.raises(ValueError):
        st.set_optimizer("lion")
    st.close()
