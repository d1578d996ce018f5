"""GPT2Step with layer-section branches (EOE): set_branch, evolve, eval_loss.

The toy is that of tests/test_gpu_muon_step.py widened to four layers: C = 128, H = 2, V = Vp = 128, B = 2, T = 64, NL = 4, layers_in_branch = 2 -- two branches of
two layers over one embedding, final norm and head; host-provided masters, the default storage types (attention matrices f8e5m2, MLP matrices 4-bit)."""
import numpy as np
import pytest
import torch

import evo_restate as R
from tests.conftest import u16
from koifish_amd import lib as L

pytestmark = pytest.mark.gpu

Cn, H, NL, LIB, V, Vp, Bn, T = 128, 2, 4, 2, 128, 128, 2, 64
PER_BLOCK = 12
HP = dict(lr=2e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1, seed=99)
EV = dict(alpha=0.9, social=2.0, t_crossover=0.6)
MAT_SLOT = dict(qkv=0, proj=2, fc=4, proj2=6)   # a block's weight matrices in the registered order: qkv.w qkv.b proj.w proj.b fc.w fc.b proj2.w proj2.b ln1.w ...


def _masters():
    from koifish_amd.train_step import MATS
    rng = np.random.default_rng(404)
    bf = lambda a: torch.from_numpy(R.rne_bf16(a.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    mk = lambda *s, std=0.08: bf(rng.normal(0, std, size=s))
    lnw = lambda: bf(1 + rng.normal(0, 0.1, Cn))
    shapes = dict(qkv=(3 * Cn, Cn), proj=(Cn, Cn), fc=(4 * Cn, Cn), proj2=(Cn, 4 * Cn))
    masters = dict(wte=mk(Vp, Cn, std=0.2), wpe=mk(T, Cn, std=0.05), lnf=(lnw(), mk(Cn)),
                   blocks=[dict({k: (mk(*shapes[k]), mk(shapes[k][0])) for k in MATS}, ln=(lnw(), mk(Cn), lnw(), mk(Cn))) for _ in range(NL)])
    ids = torch.from_numpy(rng.integers(0, V, Bn * T).astype(np.int32))
    tgt = torch.from_numpy(rng.integers(0, V, Bn * T).astype(np.int32))
    return masters, ids, tgt


def _toy(ctx, layers_in_branch, blocks=None, **kw):
    """blocks: the slice of the four master blocks a shallower model is built from"""
    from koifish_amd.train_step import GPT2Step
    masters, ids, tgt = _masters()
    if blocks is not None:
        masters = dict(masters, blocks=masters["blocks"][blocks])
    st = GPT2Step(ctx, Cn, H, len(masters["blocks"]), V, Vp, Bn, T, masters=masters, layers_in_branch=layers_in_branch, **kw)
    return st, ids.to(ctx.device), tgt.to(ctx.device)


def _snap(ctx, st):
    ctx.sync()
    return [dict({k: u16(e[k]).copy() for k in ("p", "g", "m", "v")}, blob=e["blob"].blob.cpu().numpy().copy() if e["blob"] is not None else None) for e in st.params]


def _same(a, b, keys=("p", "g", "m", "v", "blob")):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in keys)


def _losses(ctx, st):
    ctx.sync()
    return st.losses.cpu().numpy().view(np.uint32).copy()


def test_one_branch_is_todays_behaviour(ctx):
    runs = []
    for lib in (None, NL):
        st, ids, tgt = _toy(ctx, lib)
        assert st.n_branches == 1 and st.branch == 0
        ls = []
        for _ in range(2):
            st.step(ids, tgt, **HP)
            ls.append(_losses(ctx, st))
        runs.append((ls, _snap(ctx, st)))
        st.close()
    (la, sa), (lb, sb) = runs
    assert all(np.array_equal(a, b) for a, b in zip(la, lb))
    assert all(s["m"].any() for s in sa), "every tensor was updated"
    for i, (a, b) in enumerate(zip(sa, sb)):
        assert _same(a, b), "tensor %d" % i


@pytest.mark.parametrize("b", [0, 1])
def test_a_branch_is_the_shallow_model(ctx, b):
    big, ids, tgt = _toy(ctx, LIB)
    small, _, _ = _toy(ctx, None, blocks=slice(b * LIB, (b + 1) * LIB))
    assert big.n_branches == 2 and len(small.params) == LIB * PER_BLOCK + 4
    big.set_branch(b)
    assert big.branch == b
    before = _snap(ctx, big)
    big.forward(ids, tgt)
    small.forward(ids, tgt)
    assert np.array_equal(_losses(ctx, big), _losses(ctx, small)), "per-row losses of branch %d differ from the two-layer model's" % b
    big.backward()
    big.update(**HP)
    small.backward()
    ctx.sync()
    index = lambda j: j + b * LIB * PER_BLOCK if j < LIB * PER_BLOCK else NL * PER_BLOCK + (j - LIB * PER_BLOCK)   # the small model's tensor j in the branch model's order
    b1c, b2c = 1.0 - HP["beta1"], 1.0 - HP["beta2"]
    for j, e in enumerate(small.params):   # the small model's update with the branch model's seed indices: kf_adamw directly, then the quantiser
        assert u16(e["g"]).any(), e["name"]
        L.check(ctx.hip.kf_adamw(ctx.h, e["p"].data_ptr(), e["g"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr(), e["p"].numel(), L.BF16, HP["lr"], HP["beta1"], HP["beta2"],
                                 b1c, b2c, HP["eps"], HP["wd"] if e["wd"] else 0.0, 1.0, (HP["seed"] + 7919 + index(j)) & 0xFFFFFFFF, None), "kf_adamw")
    after = _snap(ctx, big)
    mine = {index(j) for j in range(len(small.params))}
    for j, e in enumerate(small.params):
        a = after[index(j)]
        assert big.params[index(j)]["name"].split(".", 1)[-1] == e["name"].split(".", 1)[-1]
        assert np.array_equal(a["p"], u16(e["p"])) and np.array_equal(a["m"], u16(e["m"])) and np.array_equal(a["v"], u16(e["v"])), e["name"]
        assert not a["g"].any()
        if e["type"] in (L.F8E5M2, L.Q4):
            assert np.array_equal(a["blob"], ctx.quantize(e["p"], e["type"]).blob.cpu().numpy()), "blob of %s" % e["name"]
    others = [i for i in range(len(big.params)) if i not in mine]
    assert len(others) == LIB * PER_BLOCK
    for i in others:
        assert _same(before[i], after[i]), "%s belongs to the other branch and changed" % big.params[i]["name"]
        assert not after[i]["g"].any() and not after[i]["m"].any()
    big.close()
    small.close()


@pytest.mark.parametrize("algo", ["pso_ga", "pso", "mix"])
def test_evolve(ctx, algo):
    from koifish_amd.train_step import MATS
    st, ids, tgt = _toy(ctx, LIB)
    before = _snap(ctx, st)
    st.evolve(0, algo, seed=77, **EV)
    after = _snap(ctx, st)
    followers = {}
    for l in range(LIB, NL):
        for k in MATS:
            followers[l * PER_BLOCK + MAT_SLOT[k]] = (l - LIB) * PER_BLOCK + MAT_SLOT[k]
    assert sorted(st.params[i]["name"] for i in followers) == sorted("h%d.%s.w" % (l, k) for l in (2, 3) for k in MATS)
    for i, e in enumerate(st.params):
        if i not in followers:   # the head's section, every bias and norm, wte / wpe / lnf
            assert _same(before[i], after[i]), "%s was touched" % e["name"]
            continue
        want = R.evolve(before[i]["p"], before[followers[i]]["p"], algo, alpha=EV["alpha"], social=EV["social"], t_cross=EV["t_crossover"], seed=77 + i)
        assert np.array_equal(after[i]["p"], want), "%s: %d elements differ from the restatement" % (e["name"], int((after[i]["p"] != want).sum()))
        assert not np.array_equal(after[i]["p"], before[i]["p"])
        assert _same(before[i], after[i], keys=("g", "m", "v"))
        assert np.array_equal(after[i]["blob"], ctx.quantize(e["p"], e["type"]).blob.cpu().numpy()), "blob of %s" % e["name"]
    st.set_branch(1)
    st.step(ids, tgt, **HP)
    ctx.sync()
    assert torch.isfinite(st.losses).all()
    st.close()


def test_eval_loss(ctx):
    st, ids, tgt = _toy(ctx, LIB)
    st.set_branch(1)
    st.forward(ids, tgt)
    fwd1 = _losses(ctx, st)
    before = _snap(ctx, st)
    l0, l1 = st.eval_loss(ids, tgt, "branch", 0), st.eval_loss(ids, tgt, "branch", 1)
    agg = st.eval_loss(ids, tgt, "aggregation")
    active = st.eval_loss(ids, tgt, "branch")
    ctx.sync()
    assert st.branch == 1
    n0, n1 = l0.cpu().numpy(), l1.cpu().numpy()
    assert n0.dtype == np.float32 and n0.shape == (Bn * T,) and not np.array_equal(n0, n1)
    assert np.array_equal(n1.view(np.uint32), fwd1) and np.array_equal(active.cpu().numpy(), n1)
    want = (n0 + n1) / np.float32(2.0)
    assert np.array_equal(agg.cpu().numpy().view(np.uint32), want.view(np.uint32))
    after = _snap(ctx, st)
    for i, (a, b) in enumerate(zip(before, after)):
        assert _same(a, b), st.params[i]["name"]
    with pytest.raises(L.KFError):
        st.backward()   # the kept activations are the evaluation's: a backward needs a forward of its own
    with pytest.raises(ValueError):
        st.eval_loss(ids, tgt, "best")
    with pytest.raises(L.KFError):
        st.eval_loss(ids, tgt, "branch", 2)
    st.close()


def test_refusals(ctx):
    from koifish_amd.train_step import GPT2Step
    with pytest.raises(L.KFError, match="do not divide"):
        _toy(ctx, 3)
    st, ids, tgt = _toy(ctx, LIB)
    for b in (-1, 2):
        with pytest.raises(L.KFError, match="branch"):
            st.set_branch(b)
    assert st.branch == 0
    with pytest.raises(ValueError):
        st.evolve(0, "mutation")
    with pytest.raises(L.KFError, match="head branch"):
        st.evolve(2, "pso")
    st.close()
    one, _, _ = _toy(ctx, None)
    before = _snap(ctx, one)
    one.evolve(0, "pso_ga", seed=1)   # one branch: ExploreOptimization returns early
    assert all(_same(a, b) for a, b in zip(before, _snap(ctx, one)))
    one.close()
    gm, ids, tgt = _toy(ctx, LIB, train_target="gama")
    assert any(e.get("gama") for e in gm.params)
    before = _snap(ctx, gm)
    with pytest.raises(L.KFError, match="gama-trained") as ei:
        gm.evolve(0, "pso_ga", seed=77)
    assert "-1000" in str(ei.value)
    assert all(_same(a, b) for a, b in zip(before, _snap(ctx, gm)))
    gm.set_branch(1)
    gm.step(ids, tgt, **HP)   # branches themselves serve a gama trainer
    ctx.sync()
    assert torch.isfinite(gm.losses).all()
    gm.close()
