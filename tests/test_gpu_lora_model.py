"""Trained low-rank adapters in the decoder: Qwen3Step(train_target="lora").as_model(max_seq, adapters=True) on the toy of tests/qwen3_toy.py (dim 128, 2 layers, 4-bit
matrices, rank 16, lora_s 0.5) scores, decodes, prefills and generates with the adapters applied (kf_lora_apply after every base product, Fish::LoraGroup).

The fp64 reference is tests/qwen3_toy.py::ref_logits on P = W_deq + s^2 b a, built as tests/test_gpu_lora_step.py::_torch_params builds it.  The bar is the project's own
(tests/test_gpu_score.py, tests/test_gpu_qwen3_step.py::_scores64): 2 * 2^-6 * max|reference logits at t| per position.  Adapter entries are drawn with std 0.2: the
0.05 of tests/test_gpu_lora_step.py, doubled until the fp64 reference ALONE tells the adapters from the base -- its own log-probs with and without them differ by more
than 4 bars at half of the positions or more (asserted below on the reference; at 0.05 they move by half a bar and a model that applied no adapter would pass, at 0.1
at a third of the positions only).

With b = 0 (the default initialisation) the adapters add nothing: ids, logits and K / V rows of 24 decoded positions are BIT FOR BIT those of the same model after
clear_adapters() -- the unfused route and the fused ones agree in the canonical order (tests/test_gpu_canonical.py).  The toy's shape (dim 128) is none the persistent
engine is built for, so on it clear_adapters() gives back the fused per-layer launches and engine_why() names the shape again; the same is checked on the 256-wide shape
the engine serves, where clear_adapters() gives back the engine and engine_why() is empty."""
import numpy as np
import pytest
import torch

from helpers import ids_agree_up_to_a_near_tie
from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import XcdReplicas
from koifish_amd.train_step import Q3_MATS, Qwen3Step
from oracle import oracle as O
from test_gpu_lora_step import _torch_params
from tests import qwen3_toy as Q
from tests.conftest import u16

pytestmark = pytest.mark.gpu

RANK, S, STD = 16, 0.5, 0.2
SEQ = np.random.default_rng(5).integers(0, Q.V, 40).astype(np.int32)


def _adapters(targets=Q3_MATS, seed=7, std=STD):
    """non-zero a and b for every adapted matrix of the toy, bf16 host tensors (tests/test_gpu_lora_step.py::_adapters with a chosen std)"""
    rng = np.random.default_rng(seed)
    bf = lambda v: torch.from_numpy(O.f32_to_bf16(v.astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    shapes = Qwen3Step._mat_shapes(Q.CFG)
    return {"l%d.%s.w" % (l, k): (bf(rng.normal(0, std, (RANK, shapes[k][1]))), bf(rng.normal(0, std, (shapes[k][0], RANK)))) for l in range(Q.CFG["n_layer"]) for k in targets}


def _params(ctx, st, with_adapters=True):
    """the fp64 model's parameters on the CURRENT blobs and adapters; with_adapters=False: the frozen base alone"""
    P, _ = _torch_params(ctx, st)
    P = {k: v.detach() for k, v in P.items()}
    if not with_adapters:
        for e in st.params:
            if e.get("lora"):
                P[Q.key_of(e["name"])] = Q.F64(u16(ctx.dequant(e["blob"]))).reshape(e["blob"].ne0, e["blob"].ne1)
    return P


def _ref(P, seq):
    """fp64 logits [n, V], log P(seq[t + 1]) for t < n - 1, and the bar per position"""
    with torch.no_grad():
        lg = Q.ref_logits(P, np.asarray(seq), 1, len(seq)).numpy()
    m = lg[:-1].max(axis=1)
    lse = m + np.log(np.exp(lg[:-1] - m[:, None]).sum(axis=1))
    return lg, lg[np.arange(len(seq) - 1), np.asarray(seq)[1:]] - lse, 2 * 2.0 ** -6 * np.abs(lg).max(axis=1)


class _Ref64:
    """the fp64 reference behind the oracle's decode(token, pos) -> (_, bf16 logits, _), for tests/helpers.py::ids_agree_up_to_a_near_tie"""

    def __init__(self, P):
        self.P, self.toks = P, []

    def decode(self, tok, pos):
        assert pos == len(self.toks)
        self.toks.append(int(tok))
        with torch.no_grad():
            lg = Q.ref_logits(self.P, np.asarray(self.toks), 1, len(self.toks)).numpy()[-1]
        return int(lg.argmax()), O.f32_to_bf16(lg.astype(np.float32)), None


def _decode(m, seq, n):
    """n teacher-forced steps from position 0 -> (ids, logits bits [n, V])"""
    forced = np.full(m.cfg["max_seq"], -1, dtype=np.int32)
    forced[:len(seq)] = seq
    m.set_forced(forced)
    m.set_state(int(seq[0]), 0)
    ids, logits = [], []
    for p in range(n):
        m.run_steps(p, 1)
        m.sync()
        ids.append(int(m.tokens_out(p + 1)[p]))
        logits.append(m.logits())
    return ids, np.stack(logits)


def _check_model(ctx, st, m, what, decode=True):
    """score (token batch: the tile form with a tail) and, token by token, the decode logits (the vector form) against the fp64 reference on the current adapters; the
    reference must itself tell the adapters from the base.  Returns the device's scores"""
    lg, want, bar = _ref(_params(ctx, st), SEQ)
    _, base, _ = _ref(_params(ctx, st, False), SEQ)
    moved = np.abs(want - base) > 4 * bar[:-1]
    print("%s: the reference's log-probs move by more than 4 bars at %d of %d positions (adapter std %g)" % (what, int(moved.sum()), len(moved), STD))
    assert moved.mean() >= 0.5, "the reference does not see the adapters: raise STD"
    got = m.score(SEQ).astype(np.float64)
    print("%s: score, max |dlp| / bar = %.3f" % (what, (np.abs(got - want) / bar[:-1]).max()))
    assert (np.abs(got - want) <= bar[:-1]).all(), "%s: score of token %d" % (what, int(np.argmax(np.abs(got - want) / bar[:-1])))
    if decode:
        _, bits = _decode(m, SEQ, len(SEQ))
        err = np.abs(O.bf16_to_f32(bits).astype(np.float64) - lg).max(axis=1)
        print("%s: decode, max |dlogit| / bar = %.3f" % (what, (err / bar).max()))
        assert (err <= bar).all(), "%s: decode logits at position %d" % (what, int(np.argmax(err / bar)))
    return got


def test_default_init_adapters_change_no_bit(ctx):
    st, _, _ = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S)   # b = 0
    m = st.as_model(128, adapters=True)
    assert "adapters" in m.engine_why()
    state, held = st.lora_state(), m.adapters()
    assert set(held) == set(state) and len(held) == 7 * Q.CFG["n_layer"]
    assert all(held[k][0].data_ptr() == state[k][0].data_ptr() and held[k][1].data_ptr() == state[k][1].data_ptr() for k in state)
    n = 24
    steps0 = m.engine_steps()
    ids_a, lg_a = _decode(m, SEQ, n)
    ka, va = m.kv_to_host()
    assert m.engine_steps() <= max(steps0, 0), "the engine ran with adapters attached"
    m.clear_adapters()
    assert "adapters" not in m.engine_why() and "shape" in m.engine_why() and m.adapters() == {}   # dim 128 is no engine shape: the reason is the shape's again
    ids_b, lg_b = _decode(m, SEQ, n)
    kb, vb = m.kv_to_host()
    assert ids_a == ids_b
    assert np.array_equal(lg_a, lg_b), "positions %s" % np.flatnonzero((lg_a != lg_b).any(axis=1))
    assert np.array_equal(ka[:, :n], kb[:, :n]) and np.array_equal(va[:, :n], vb[:, :n])
    m.close()
    st.close()


def test_detaching_gives_the_engine_back_bit_for_bit():
    """the 256-wide shape the persistent engine serves, b = 0 on all seven matrices: the unfused route with adapters against the ENGINE after clear_adapters()"""
    cfg = synth.CONFIGS["tiny"]
    m = synth.build_from_raw(cfg, synth.raw_weights_numpy(cfg))
    assert m.engine_why() == ""
    dim, H, KV, hd, ffn = (cfg[k] for k in ("dim", "n_head", "n_kv", "head_dim", "ffn"))
    shapes = dict(q=(H * hd, dim), k=(KV * hd, dim), v=(KV * hd, dim), o=(dim, H * hd), gate=(ffn, dim), up=(ffn, dim), down=(dim, ffn))
    g = torch.Generator(device=m.device).manual_seed(3)
    ad = {"l%d.%s.w" % (l, k): ((torch.randn(RANK, shapes[k][1], device=m.device, generator=g) * 0.1).to(torch.bfloat16),
                                 torch.zeros(shapes[k][0], RANK, device=m.device, dtype=torch.bfloat16)) for l in range(cfg["n_layer"]) for k in Q3_MATS}
    seq, n = prompt_ids(cfg, 24), 24
    m.set_adapters(ad, S)
    assert "adapters" in m.engine_why()
    ids_a, lg_a = _decode(m, seq, n)
    ka, va = m.kv_to_host()
    assert m.engine_steps() == -1, "the engine ran with adapters attached"
    m.clear_adapters()
    assert m.engine_why() == "" and m.adapters() == {}
    ids_b, lg_b = _decode(m, seq, n)
    kb, vb = m.kv_to_host()
    assert m.engine_steps() >= n, "without adapters the engine serves this shape"
    assert ids_a == ids_b
    assert np.array_equal(lg_a, lg_b), "positions %s" % np.flatnonzero((lg_a != lg_b).any(axis=1))
    assert np.array_equal(ka[:, :n], kb[:, :n]) and np.array_equal(va[:, :n], vb[:, :n])
    m.close()


def test_adapters_on_all_seven_matrices(ctx):
    st, ids, tgt = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters=_adapters())
    m = st.as_model(128, adapters=True)
    held = m.adapters()
    m.clear_adapters()
    plain = m.generate(SEQ[:17], 8), m.score(SEQ).copy()
    m.set_adapters(held, S)
    assert "adapters" in m.engine_why()
    first = _check_model(ctx, st, m, "all seven")
    assert (np.abs(first - plain[1]) > 0).any()
    # prefill (a 17-row token batch: one tile with a tail) then free-running steps: the reference's greedy ids
    P = _params(ctx, st)
    ref, toks = [], [int(t) for t in SEQ[:17]]
    for _ in range(8):
        with torch.no_grad():
            ref.append(int(Q.ref_logits(P, np.asarray(toks), 1, len(toks)).numpy()[-1].argmax()))
        toks.append(ref[-1])
    m.set_forced(np.full(m.cfg["max_seq"], -1, dtype=np.int32))
    m.prefill(SEQ[:17])
    m.run_steps(17, 7)
    m.sync()
    got = m.tokens_out(24)[16:24].tolist()
    ok, msg = ids_agree_up_to_a_near_tie(_Ref64(P), [int(t) for t in SEQ[:17]], got, ref)
    assert ok, msg
    # one training step: the model reads the trainer's vectors, nothing is attached again
    st.step(torch.from_numpy(ids).to(ctx.device), torch.from_numpy(tgt).to(ctx.device), **Q.HP)
    ctx.sync()
    second = _check_model(ctx, st, m, "after one step", decode=False)
    assert not np.array_equal(first, second)
    # detached: the engine serves the model again (what it then generates: test_clear_adapters_restores_the_plain_model)
    m.clear_adapters()
    assert "adapters" not in m.engine_why() and not np.array_equal(m.score(SEQ), second.astype(np.float32))
    m.close()
    st.close()


def test_clear_adapters_restores_the_plain_model(ctx):
    st, _, _ = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters=_adapters())
    m = st.as_model(128, adapters=True)
    held = m.adapters()
    m.clear_adapters()
    before = m.generate(SEQ[:17], 8)
    lg0 = m.logits()
    m.set_adapters(held, S)
    with_a = m.generate(SEQ[:17], 8)
    lg1 = m.logits()
    assert not np.array_equal(lg0, lg1), "the adapters change nothing"
    m.clear_adapters()
    assert "adapters" not in m.engine_why()
    assert m.generate(SEQ[:17], 8) == before and np.array_equal(m.logits(), lg0)
    print("ids without / with adapters:", before, with_a)
    m.close()
    st.close()


def test_adapters_on_a_subset(ctx):
    targets = ("o", "gate", "down")
    st, _, _ = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, lora_targets=targets, adapters=_adapters(targets))
    m = st.as_model(128, adapters=True)
    assert len(m.adapters()) == 3 * Q.CFG["n_layer"]
    _check_model(ctx, st, m, "o, gate, down")
    m.close()
    st.close()


def test_refusals_name_the_adapters(ctx, tmp_path):
    st, _, _ = Q.make(ctx, train_target="lora", lora_rank=RANK, lora_s=S, adapters=_adapters())
    with pytest.raises(L.KFError, match="adapters"):
        st.as_model(128)
    m = st.as_model(128, adapters=True)
    held = m.adapters()
    with pytest.raises(L.KFError, match="adapters"):
        XcdReplicas(m)
    with pytest.raises(L.KFError, match="adapters"):
        m.set_act_int8(True)
    with pytest.raises(L.KFError, match="adapters"):
        m.set_act_int8_q4(True)
    with pytest.raises(L.KFError, match="adapters"):
        m.set_hot(0, np.ones(Q.CFG["ffn"], dtype=np.int32))
    with pytest.raises(L.KFError, match="adapters"):
        m.save_kun(tmp_path / "no.kun")
    with pytest.raises(L.KFError):   # a matrix set again beside its adapter: the pair was checked against the old one
        m.set_weight(0, 0, st.layers[0]["q"]["blob"])
    assert len(m.adapters()) == len(held) and "adapters" in m.engine_why()   # the refusals changed nothing
    with pytest.raises(ValueError):
        m.set_adapters({"l0.q.w": tuple(t.float() for t in held["l0.q.w"])}, S)
    assert len(m.adapters()) == len(held)
    m.clear_adapters()
    m.set_act_int8_q4(True)
    with pytest.raises(L.KFError, match="adapters"):
        m.set_adapters(held, S)
    assert m.adapters() == {}
    m.set_act_int8_q4(False)
    m.set_hot(0, np.ones(Q.CFG["ffn"], dtype=np.int32))
    with pytest.raises(L.KFError, match="adapters"):
        m.set_adapters(held, S)
    m.set_hot(0, None)
    m.set_adapters(held, S)
    assert len(m.adapters()) == len(held)
    m.close()
    st.close()
    other, _, _ = Q.make(ctx)
    with pytest.raises(L.KFError, match="adapters"):
        other.as_model(128, adapters=True)
    other.close()
