"""set_grad_clip on both trainers (koifish::TrainerCore, one body) at the toy shapes of tests/test_gpu_train_step.py / tests/test_gpu_qwen3_step.py: forward and
backward, every gradient read back, the norms and clip factors from tests/gradnorm_restate.py; after the update every AdamW tensor is bit for bit the oracle's CU_adamw
with THAT tensor's factor as grad_scale and the trainers' seed rule (seed + 7919 t + i), every quantised blob the oracle's quantiser on the updated master.  gclip is
half the median restated per-tensor norm, so clipping bites."""
import numpy as np
import pytest
import torch

import gradnorm_restate as G
from koifish_amd import lib as L
from oracle import oracle as O
from tests import qwen3_toy
from tests.conftest import u16
from tests.test_gpu_evo_step import LIB, PER_BLOCK, _toy
from tests.test_gpu_gama_step import HP, make as gpt2_make

pytestmark = pytest.mark.gpu
assert HP == qwen3_toy.HP
MU = dict(lr_scale=50.0, mui=0.95, eps=1e-7, tp_decay=1)
MODES = {"report": G.REPORT, "tensor": G.TENSOR, "global": G.GLOBAL}


def _make(ctx, family, **kw):
    st, ids, tgt = gpt2_make(ctx, None, **kw) if family == "gpt2" else qwen3_toy.make(ctx, **kw)
    return st, torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device)


def _is_muon(st, e):
    return (st.optimizer == "muon" and e["blob"] is not None and not e.get("gama") and e["name"].startswith(st._layer_prefix) and e["name"][1].isdigit()
            and e["p"].dim() == 2 and e["p"].shape[0] >= e["p"].shape[1])


def _snap(ctx, st):
    ctx.sync()
    return [dict({k: u16(e[k]).reshape(-1).copy() for k in ("p", "g", "m", "v")}, blob=e["blob"].blob.cpu().numpy().copy() if e["blob"] is not None else None) for e in st.params]


def _restate(st, snap):
    """(sumsq, gnorm, the Muon mask) of the gradients just read back"""
    ss, gn = G.norms([s["g"] for s in snap])
    return ss, gn, [_is_muon(st, e) for e in st.params]


def _half_median(gn):
    nz = np.sort(gn[:-1][gn[:-1] > 0])
    return 0.5 * float(nz[len(nz) // 2])


def _check_adamw(st, i, e, s0, scale, t):
    p, g, m, v = (s0[k].copy() for k in ("p", "g", "m", "v"))
    b1c, b2c = 1.0 - HP["beta1"] ** t, 1.0 - HP["beta2"] ** t
    assert O.adamw(p, g, m, v, HP["lr"], HP["beta1"], HP["beta2"], b1c, b2c, HP["eps"], HP["wd"] if e["wd"] else 0.0, float(scale), (HP["seed"] + 7919 * t + i) & 0xFFFFFFFF) == 0
    assert np.array_equal(u16(e["p"]).reshape(-1), p), "%s: master differs from the oracle's AdamW at grad_scale %r" % (e["name"], float(scale))
    assert np.array_equal(u16(e["m"]).reshape(-1), m) and np.array_equal(u16(e["v"]).reshape(-1), v), e["name"]
    assert not u16(e["g"]).any() and not np.array_equal(p, s0["p"]), e["name"]
    if e["type"] in (L.F8E5M2, L.Q4) and not e.get("gama"):   # the blob the next forward reads = the oracle's quantiser on the updated master
        ne0, ne1 = e["p"].shape
        ow = O.quantize(u16(e["p"]).reshape(ne0, ne1), ne0, ne1, e["type"])
        assert np.array_equal(e["blob"].blob.cpu().numpy(), np.frombuffer(ow.blob(), dtype=np.uint8)), "blob of %s" % e["name"]


def _check_norms(st, gn):
    got = st.grad_norms()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), gn[:-1].view(np.uint32))
    assert np.float32(st.grad_norm()).view(np.uint32) == gn[-1].view(np.uint32)


def _clipped_step(ctx, st, ids, tgt, mode):
    """forward, backward, the restated factors at half the median norm, update: returns (the snapshot before the update, scales, gnorm)"""
    st.forward(ids, tgt)
    st.backward()
    s0 = _snap(ctx, st)
    ss, gn, mask = _restate(st, s0)
    c = _half_median(gn)
    scale = G.scales(gn, MODES[mode], c, no_clip=mask)
    st.set_grad_clip(c, mode)
    st.update(**HP)
    ctx.sync()
    return s0, scale, gn, mask


@pytest.mark.parametrize("mode", ["tensor", "global"])
@pytest.mark.parametrize("family", ["gpt2", "qwen3"])
def test_every_adamw_tensor_follows_its_scale(ctx, family, mode):
    st, ids, tgt = _make(ctx, family)
    s0, scale, gn, _ = _clipped_step(ctx, st, ids, tgt, mode)
    assert (scale < 1).all() if mode == "global" else (scale < 1).sum() >= len(scale) // 2   # half the median norm: clipping bites
    for i, e in enumerate(st.params):
        _check_adamw(st, i, e, s0[i], scale[i], st.t)
    _check_norms(st, gn)
    # a second step with the table in place: the norms are those of the new gradients
    st.forward(ids, tgt)
    st.backward()
    s1 = _snap(ctx, st)
    ss, gn1, mask = _restate(st, s1)
    st.update(**HP)
    ctx.sync()
    scale1 = G.scales(gn1, MODES[mode], st._clip[0], no_clip=mask)
    for i, e in enumerate(st.params):
        _check_adamw(st, i, e, s1[i], scale1[i], st.t)
    _check_norms(st, gn1)


@pytest.mark.parametrize("family", ["gpt2", "qwen3"])
def test_report_changes_no_bit_of_the_update(ctx, family):
    st, ids, tgt = _make(ctx, family)
    twin, _, _ = _make(ctx, family)
    st.set_grad_clip(mode="report")
    with pytest.raises(L.KFError):
        st.grad_norms()   # no update yet
    for s in (st, twin):
        s.forward(ids, tgt)
        s.backward()
    s0 = _snap(ctx, st)
    ss, gn, _ = _restate(st, s0)
    assert all(np.array_equal(a["g"], b["g"]) for a, b in zip(s0, _snap(ctx, twin)))
    for s in (st, twin):
        s.update(**HP)
    a, b = _snap(ctx, st), _snap(ctx, twin)
    for x, y, z, e in zip(a, b, s0, st.params):
        assert all(np.array_equal(x[k], y[k]) for k in ("p", "g", "m", "v")) and (x["blob"] is None or np.array_equal(x["blob"], y["blob"])), e["name"]
        assert not np.array_equal(x["p"], z["p"]), e["name"]
    _check_norms(st, gn)
    # off again: nothing to read, and the update goes on as before
    st.set_grad_clip(mode=None)
    with pytest.raises(L.KFError):
        st.grad_norms()
    with pytest.raises(ValueError):
        st.set_grad_clip(1.0, "layer")
    with pytest.raises(L.KFError):
        st.set_grad_clip(0.0, "tensor")


@pytest.mark.parametrize("family", ["gpt2", "qwen3"])
def test_muon_tensors_are_left_alone_and_counted(ctx, family):
    st, ids, tgt = _make(ctx, family)
    twin, _, _ = _make(ctx, family)
    st.set_grad_clip(1.0, "tensor")   # before the switch: set_optimizer writes the table again with the Muon mask
    for s in (st, twin):
        s.set_optimizer("muon", **MU)
    twin.forward(ids, tgt)
    twin.backward()
    twin.update(**HP)
    s0, scale, gn, mask = _clipped_step(ctx, st, ids, tgt, "tensor")
    after_twin = _snap(ctx, twin)
    n_muon = sum(mask)
    assert n_muon == (3 if family == "gpt2" else 5) * 2 and (scale[np.array(mask)] == 1).all() and (scale[~np.array(mask)] < 1).any()
    for i, e in enumerate(st.params):
        if mask[i]:
            assert np.array_equal(u16(e["p"]).reshape(-1), after_twin[i]["p"]) and np.array_equal(u16(e["m"]).reshape(-1), after_twin[i]["m"]), e["name"]
            assert np.array_equal(e["blob"].blob.cpu().numpy(), after_twin[i]["blob"]) and not u16(e["g"]).any(), e["name"]
        else:
            _check_adamw(st, i, e, s0[i], scale[i], st.t)
    _check_norms(st, gn)
    total_wo_muon = np.sqrt(sum(float(g) ** 2 for g, mk in zip(gn[:-1], mask) if not mk))
    assert st.grad_norm() > total_wo_muon   # |g| includes the Muon tensors


@pytest.mark.parametrize("family", ["gpt2", "qwen3"])
def test_gama_tensors_are_clipped_like_any_adamw_tensor(ctx, family):
    st, ids, tgt = _make(ctx, family, train_target="gama")
    s0, scale, gn, _ = _clipped_step(ctx, st, ids, tgt, "tensor")
    ge = [i for i, e in enumerate(st.params) if e.get("gama")]
    assert len(ge) == (4 if family == "gpt2" else 14) and (scale[ge] < 1).any()
    for i, e in enumerate(st.params):
        _check_adamw(st, i, e, s0[i], scale[i], st.t)
    _check_norms(st, gn)


def test_eoe_branch_clips_its_section_only(ctx):
    st, ids, tgt = _toy(ctx, LIB)
    st.set_branch(1)
    before = _snap(ctx, st)
    s0, scale, gn, _ = _clipped_step(ctx, st, ids, tgt, "tensor")
    nl = len(st.blocks)
    inside = lambda i: i >= nl * PER_BLOCK or LIB <= i // PER_BLOCK < 2 * LIB
    assert (scale[[i for i in range(len(st.params)) if inside(i)]] < 1).any()
    after = _snap(ctx, st)
    for i, e in enumerate(st.params):
        if inside(i):
            _check_adamw(st, i, e, s0[i], scale[i], st.t)
        else:   # another branch's tensor: a zero gradient, norm 0, scale 1, and not a bit of it touched
            assert gn[i] == 0 and scale[i] == 1 and not s0[i]["g"].any()
            assert all(np.array_equal(after[i][k], before[i][k]) for k in ("p", "g", "m", "v")) and (before[i]["blob"] is None or np.array_equal(after[i]["blob"], before[i]["blob"])), e["name"]
    _check_norms(st, gn)
    assert st.grad_norms()[:LIB * PER_BLOCK].max() == 0


@pytest.mark.parametrize("family", ["gpt2", "qwen3"])
def test_a_refusal_changes_nothing_and_a_reregistered_tensor_needs_a_new_table(ctx, family):
    st, ids, tgt = _make(ctx, family)
    _clipped_step(ctx, st, ids, tgt, "tensor")
    keep, clip = st._sc_clip, st._clip
    for bad in (0.0, -1.0, float("nan")):   # refused while clipping is ON: the trainer goes on reading the scratch it had, which must still be the one held here
        with pytest.raises(L.KFError):
            st.set_grad_clip(bad, "tensor")
        with pytest.raises(L.KFError):
            st.set_grad_clip(bad, "global")
    with pytest.raises(ValueError):
        st.set_grad_clip(1.0, "layer")
    assert st._sc_clip is keep and st._clip == clip

    def checked_update():
        st.forward(ids, tgt)
        st.backward()
        s = _snap(ctx, st)
        ss, gn, mask = _restate(st, s)
        st.update(**HP)
        ctx.sync()
        scale = G.scales(gn, G.TENSOR, st._clip[0], no_clip=mask)
        assert (scale < 1).any()
        for i, e in enumerate(st.params):
            _check_adamw(st, i, e, s[i], scale[i], st.t)
        _check_norms(st, gn)
    checked_update()
    # the last tensor (a norm weight or bias: no blob) registered again, as _attach registered it: the table is stale until set_grad_clip is called again
    i, e = len(st.params) - 1, st.params[-1]
    assert e["blob"] is None
    st._call("set_param", i, e["p"].data_ptr(), e["g"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr(), e["p"].numel(), int(e["wd"]), None, 0)
    t0 = st.t
    with pytest.raises(L.KFError):
        st.update(**HP)
    with pytest.raises(L.KFError):
        st.forward(ids, tgt)
    assert st.t == t0
    st.set_grad_clip(*clip)
    checked_update()
    assert st.t == t0 + 1
