"""Qwen3Step.set_documents: supervised fine-tuning on packed documents, at the toy shape of tests/qwen3_toy.py (2 x 64 = 128 rows, T = 64), against torch fp64 autograd
per document and against the plain step.

Two layouts.  FULL is documents of 1, 40, 23 and 64 rows back to back: they fill the 128 rows, the last one as long as the rope table.  GAPPED is 1, 40, 23, then
five gap rows, then 59 rows: 1 + 40 + 23 + 64 = 128 leaves no row for a gap, so the layout with one ends in a shorter document; the 64-row document stays covered by
FULL and by set_documents([T] * B).  The loss mask ignores the first half of every document (a one-row document keeps its row)."""
import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from tests.conftest import u16
from tests.qwen3_toy import CFG, HP, N, T, Bn, V, Vp, grad_deviation, make, ref_logits, torch_params

pytestmark = pytest.mark.gpu
FULL = dict(lens=[1, 40, 23, 64], rows=[0, 1, 41, 64])
GAPPED = dict(lens=[1, 40, 23, 59], rows=[0, 1, 41, 69])
NL = CFG["n_layer"]


def _mask(lay):
    m = np.zeros(N, dtype=bool)
    for r, n in zip(lay["rows"], lay["lens"]):
        m[r + n // 2:r + n] = True
    return m


def _in_doc(lay):
    m = np.zeros(N, dtype=bool)
    for r, n in zip(lay["rows"], lay["lens"]):
        m[r:r + n] = True
    return m


def _dev(ctx, a):
    return torch.from_numpy(a).to(ctx.device)


def _grads(st):
    return [u16(e["g"]).copy() for e in st.params]


def _zero_grads(st):
    for e in st.params:
        e["g"].zero_()


def _poison(st):
    """NaN bit patterns in every activation and gradient buffer a gap row could leak from"""
    for t_ in [a[k] for a in st.A for k in ("att", "qkv")] + [st.dqkv, st.datt, st.logits]:
        t_.view(torch.int16).fill_(-1)


def _other_rows(ids, tgt, rows_mask, seed):
    """other valid ids and targets in the rows of rows_mask"""
    rng = np.random.default_rng(seed)
    ids2, tgt2 = ids.copy(), tgt.copy()
    ids2[rows_mask] = (ids[rows_mask] + 1 + rng.integers(0, V - 1, int(rows_mask.sum()))) % V
    tgt2[rows_mask] = (tgt[rows_mask] + 1 + rng.integers(0, V - 1, int(rows_mask.sum()))) % V
    assert (ids2[rows_mask] != ids[rows_mask]).all() and ids2.max() < V and ids2.min() >= 0
    return ids2.astype(np.int32), tgt2.astype(np.int32)


@pytest.mark.parametrize("name", ["FULL", "GAPPED"])
def test_loss_and_gradients_vs_fp64_per_document(ctx, name):
    """fp64: ref_logits on each document alone (positions 0 .. len - 1), cross entropy summed over the rows that count, divided by n_valid.  Bars: the loss within
    2^-7 relative; every gradient within those of tests/test_gpu_qwen3_step.py::_check_grads (max 2^-5, rms 2^-7 of the tensor's largest reference magnitude, rms
    2^-6 for qn / kn)."""
    lay = dict(FULL=FULL, GAPPED=GAPPED)[name]
    st, ids, tgt = make(ctx)
    mask = _mask(lay)
    st.set_documents(lay["lens"], lay["rows"], mask)
    assert st.documents()["n_valid"] == int(mask.sum()) and st.documents()["lens"].tolist() == lay["lens"]
    P, leaves = torch_params(ctx, st)
    total = 0.0
    for r, n in zip(lay["rows"], lay["lens"]):
        lg = ref_logits(P, ids[r:r + n], 1, n)
        ce = torch.nn.functional.cross_entropy(lg, torch.from_numpy(tgt[r:r + n]).long(), reduction="none")
        total = total + (ce * torch.from_numpy(mask[r:r + n].astype(np.float64))).sum()
    loss = total / int(mask.sum())
    loss.backward()
    st.forward(_dev(ctx, ids), _dev(ctx, tgt))
    st.backward()
    ctx.sync()
    ref, got = float(loss.detach()), st.sft_loss()
    print("%s: sft loss device %.6f fp64 %.6f over %d rows" % (name, got, ref, int(mask.sum())))
    assert abs(got - ref) <= 2.0 ** -7 * ref
    losses = st.losses.cpu().numpy()
    assert (losses[~mask] == 0.0).all() and (losses[mask] > 0).all(), "losses of ignored rows stay exactly 0.0"
    assert not u16(st.logits)[~mask].any(), "the ignored rows of the logit gradient are exactly zero"
    worst = []
    for e in st.params:
        mx, rms = grad_deviation(e["g"], leaves[e["name"]].grad.numpy())
        worst.append((round(mx, 4), round(rms, 5), e["name"]))
        assert mx <= 2.0 ** -5 and rms <= (2.0 ** -6 if e["name"].endswith(("qn", "kn")) else 2.0 ** -7), "%s: max %.4f rms %.5f of scale" % (e["name"], mx, rms)
    print("largest gradient deviations (max, rms, tensor):", sorted(worst, reverse=True)[:3])
    st.close()


def test_the_plain_step_is_a_special_case(ctx):
    """B documents of T rows, no mask: the plain step's losses and every gradient bit for bit (at T = 64 the plain forward takes the ATTN_TILE route, the form the
    documents entry always takes); after set_documents(None) the step is the plain one again."""
    st, ids, tgt = make(ctx)
    d_ids, d_tgt = _dev(ctx, ids), _dev(ctx, tgt)
    runs = []
    for docs in (None, [T] * Bn, None):
        if docs is not None or runs:
            st.set_documents(docs)
        assert (st.documents() is None) == (docs is None)
        _zero_grads(st)
        _poison(st)
        st.forward(d_ids, d_tgt)
        st.backward()
        ctx.sync()
        runs.append((st.losses.cpu().numpy().copy(), _grads(st)))
    assert st.documents() is None and runs[0][0].all() and all(g.any() for g in runs[0][1])
    for k in (1, 2):
        assert np.array_equal(runs[0][0], runs[k][0]), "losses, run %d" % k
        for e, a, b in zip(st.params, runs[0][1], runs[k][1]):
            assert np.array_equal(a, b), "run %d: gradient of %s" % (k, e["name"])
    with pytest.raises(L.KFError, match="no documents"):
        st.sft_loss()
    st.close()


def _invariance(ctx, st, ids, tgt, which):
    """two forward + backward from the same weights on GAPPED: the second with other ids and targets in the gap rows, other targets in the ignored rows, and NaN
    patterns in the buffers; returns the two gradient snapshots of the entries `which` selects"""
    mask, in_doc = _mask(GAPPED), _in_doc(GAPPED)
    snaps = []
    for rnd in range(2):
        i2, t2 = ids, tgt
        if rnd:
            i2, t2 = _other_rows(ids, tgt, ~in_doc, 17)
            t2 = _other_rows(ids, t2, in_doc & ~mask, 18)[1]
            _poison(st)
        _zero_grads(st)
        st.forward(_dev(ctx, i2), _dev(ctx, t2))
        st.backward()
        ctx.sync()
        snaps.append([(e["name"], u16(e["g"]).copy(), bool(torch.isfinite(e["g"].float()).all())) for e in st.params if which(e)])
    return snaps


def test_gap_and_ignored_rows_carry_nothing(ctx):
    st, ids, tgt = make(ctx)
    st.set_documents(GAPPED["lens"], GAPPED["rows"], _mask(GAPPED))
    a, b = _invariance(ctx, st, ids, tgt, lambda e: True)
    assert len(a) == len(st.params)
    for (name, g0, fin0), (_, g1, fin1) in zip(a, b):
        assert fin0 and fin1, "%s: a gradient is not finite" % name
        assert g0.any() and np.array_equal(g0, g1), "%s: the gradient depends on what gap rows, ignored targets or stale buffers hold" % name
    st.close()


def test_lora_on_documents(ctx):
    st, ids, tgt = make(ctx, train_target="lora")
    st.set_documents(GAPPED["lens"], GAPPED["rows"], _mask(GAPPED))
    frozen = [(e["name"], e["blob"].blob.clone()) for e in st.params if e.get("lora")]
    assert len(frozen) == 7 * NL
    d_ids, d_tgt = _dev(ctx, ids), _dev(ctx, tgt)
    losses = []
    for _ in range(3):
        st.step(d_ids, d_tgt, **HP)
        ctx.sync()
        losses.append(st.sft_loss())
    print("sft losses over three steps:", ["%.4f" % v for v in losses])
    assert losses[0] > losses[1] > losses[2], losses
    by_name = {e["name"]: e for e in st.params}
    for name, blob in frozen:
        assert torch.equal(by_name[name]["blob"].blob, blob), "the frozen blob of %s changed" % name
    a, b = _invariance(ctx, st, ids, tgt, lambda e: e.get("lora"))
    assert len(a) == 7 * NL
    for (name, g0, fin0), (_, g1, fin1) in zip(a, b):
        assert fin0 and fin1 and g0.any() and np.array_equal(g0, g1), "[a | b] of %s" % name
    st.close()


def test_distillation_and_documents_refuse_each_other(ctx):
    st, ids, tgt = make(ctx)
    teacher = torch.zeros(N, Vp, dtype=torch.bfloat16, device=ctx.device)
    st.set_documents(GAPPED["lens"], GAPPED["rows"])
    with pytest.raises(L.KFError, match="documents are set"):
        st.set_distill(teacher)
    assert st._distill is None and st.documents()["n_valid"] == sum(GAPPED["lens"])
    st.forward(_dev(ctx, ids), _dev(ctx, tgt))   # still the documents step
    ctx.sync()
    assert not st.losses.cpu().numpy()[~_in_doc(GAPPED)].any()
    st.set_documents(None)
    st.set_distill(teacher)
    with pytest.raises(L.KFError, match="a teacher is set"):
        st.set_documents(GAPPED["lens"], GAPPED["rows"])
    assert st.documents() is None and st._distill is not None
    st.set_distill(None)
    st.set_documents(GAPPED["lens"], GAPPED["rows"])
    with pytest.raises(ValueError, match="no row counts"):
        st.set_documents(GAPPED["lens"], GAPPED["rows"], np.zeros(N, dtype=bool))
    assert st.documents()["n_valid"] == sum(GAPPED["lens"]), "a refusal changes nothing"
    st.close()
