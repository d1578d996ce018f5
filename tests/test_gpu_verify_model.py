"""Speculative decoding on whole models: Qwen3.verify (R tokens at consecutive positions through every layer with one pass over the weights) against R calls of
forward and against the oracle model -- ids, logits rows and K / V rows, bit for bit -- its refusals, and generate_speculative against generate, id for id, with
every kind of drafter, partial acceptance counted exactly, the state it leaves behind, and a 1-bit target that takes the row-by-row route end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import oracle_model, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
N_REF = 198   # positions 0 .. 197 of the teacher-forced reference run: pos0 = 190 with 8 rows ends there


def cfg_of(name):
    return dict(synth.CONFIGS[name], max_seq=256)


@pytest.fixture()
def canon():
    O.set_order(O.ORDER_CANON)
    yield
    O.set_order(O.ORDER_DOT16)


@pytest.fixture(scope="module", params=["tiny", "small"])
def ref_run(request):
    """a model, and N_REF teacher-forced positions through forward() and through the oracle model: ids, logits and K / V rows, computed once for every case below"""
    cfg = cfg_of(request.param)
    raw = synth.raw_weights_numpy(cfg, 4321, w_std=0.1)
    ids = prompt_ids(cfg, N_REF, seed=11)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    O.set_order(O.ORDER_CANON)
    try:
        om = oracle_model(cfg, raw, L.Q4, L.BF16, attn_mode=O.ATTN_CANON)
        top1, logits = np.zeros(N_REF, dtype=np.int32), np.zeros((N_REF, cfg["vocab"]), dtype=np.uint16)
        for p in range(N_REF):
            top1[p], logits[p] = m.forward(int(ids[p]), p)
            o_id, o_logits, _ = om.decode(int(ids[p]), p)
            assert o_id == top1[p] and np.array_equal(o_logits, logits[p]), "the premise (forward == the oracle) fails at position %d" % p
        ok, ov = (a.copy() for a in om.kv())   # views into the oracle's own memory: copied before it is freed
        om.close()
    finally:
        O.set_order(O.ORDER_DOT16)
    gk, gv = m.kv_to_host()
    assert np.array_equal(gk[:, :N_REF], ok[:, :N_REF]) and np.array_equal(gv[:, :N_REF], ov[:, :N_REF])
    yield cfg, m, ids, top1, logits, gk, gv
    m.close()


def zero_kv_rows(m, cfg, pos0, n):
    """the cache rows a verify pass has to write, zeroed first: equal rows afterwards are the pass's own"""
    kvd = cfg["n_kv"] * cfg["head_dim"]
    ctx = C.c_void_p(m.host.kfh_ctx(m.h))
    m.hip.kf_memset.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]
    for base in (m.host.kfh_kcache(m.h), m.host.kfh_vcache(m.h)):
        for l in range(cfg["n_layer"]):
            L.check(m.hip.kf_memset(ctx, C.c_void_p(base + ((l * cfg["max_seq"] + pos0) * kvd) * 2), 0, n * kvd * 2), "kf_memset")


@pytest.mark.parametrize("pos0", [0, 150, 190])
@pytest.mark.parametrize("R", [1, 4, 8])
def test_verify_equals_forward_and_the_oracle(ref_run, R, pos0):
    cfg, m, ids, top1, logits, gk, gv = ref_run
    zero_kv_rows(m, cfg, pos0, R)
    t1, lg = m.verify(ids[pos0:pos0 + R], pos0, want_logits=True)
    assert np.array_equal(t1, top1[pos0:pos0 + R])
    assert np.array_equal(lg, logits[pos0:pos0 + R]), "%d logits differ" % int((lg != logits[pos0:pos0 + R]).sum())
    assert np.array_equal(m.verify(ids[pos0:pos0 + R], pos0), t1)   # without the logits
    k, v = m.kv_to_host()
    assert np.array_equal(k[:, :N_REF], gk[:, :N_REF]) and np.array_equal(v[:, :N_REF], gv[:, :N_REF])


def test_verify_refusals():
    cfg = cfg_of("tiny")
    m = synth.build_from_raw(cfg, synth.raw_weights_numpy(cfg, 7, w_std=0.1), L.Q4, L.BF16)
    dev = m._ctx.device
    a = torch.zeros((16, cfg["dim"]), dtype=torch.bfloat16, device=dev)
    b = torch.zeros((cfg["n_head"] * cfg["head_dim"], 16), dtype=torch.bfloat16, device=dev)
    hot = np.ones(cfg["ffn"], dtype=np.int32)
    hot[::2] = 0
    try:
        assert len(m.verify([1, 2, 3], 0)) == 3
        for bad in ([], list(range(9))):
            with pytest.raises(L.KFError, match="1 .. 8 tokens"):
                m.verify(bad, 0)
        with pytest.raises(L.KFError, match="1 .. 8 tokens"):
            m.verify([1, 2], cfg["max_seq"] - 1)
        with pytest.raises(L.KFError, match="outside the vocabulary"):
            m.verify([1, cfg["vocab"]], 0)
        m.set_kv_int8(True)
        with pytest.raises(L.KFError, match="the int8 KV cache is on and the verify pass has no int8 KV cache form: switch kfh_set_kv_int8 off first"):
            m.verify([1, 2], 0)
        with pytest.raises(L.KFError, match="the int8 KV cache is on"):
            m.generate_speculative([1, 2], 4)
        m.set_kv_int8(False)
        m.set_act_int8_q4(True)
        with pytest.raises(L.KFError, match="int8 activations are on and the verify pass has no int8-activation form"):
            m.verify([1, 2], 0)
        m.set_act_int8_q4(False)
        assert m.host.kfh_set_adapter(m.h, 0, 0, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), 16, 1.0) == 0
        with pytest.raises(L.KFError, match="adapters are attached and the verify pass has no adapter form: clear the adapters first"):
            m.verify([1, 2], 0)
        m.clear_adapters()
        m.set_hot(0, hot)
        with pytest.raises(L.KFError, match="hot-row mask is set and the verify pass has no sparse form"):
            m.verify([1, 2], 0)
        m.set_hot(0, None)
        m.set_fuse_level(0)
        with pytest.raises(L.KFError, match="fuse_level 0 is set and the verify pass has no one-launch-per-kernel form"):
            m.verify([1, 2], 0)
        m.set_fuse_level(1)
        m.set_sampler(temperature=0.7, top_k=20)
        with pytest.raises(L.KFError, match="a sampler is set"):
            m.verify([1, 2], 0)
        with pytest.raises(L.KFError, match="a sampler is set"):
            m.generate_speculative([1, 2], 4)
        m.set_sampler(temperature=0.0)
        assert len(m.verify([1, 2], 0)) == 2                      # with all of them gone it runs again
        with pytest.raises(L.KFError):
            m.generate_speculative([1, 2], 4, k=8)
        assert m.host.kfh_tp_init(m.h, 0, 2, 0) == 0              # last: this model is a TP rank from here on
        with pytest.raises(L.KFError, match="tensor-parallel rank and the verify pass has no tensor-parallel form") as e:
            m.verify([1, 2], 0)
        assert "-1000" in str(e.value)                            # KF_UNSUPPORTED_DATATYPE
    finally:
        m.close()


# ---- generate_speculative == generate
N_NEW = 40


@pytest.fixture(scope="module")
def gen_case():
    cfg = cfg_of("tiny")
    raw = synth.raw_weights_numpy(cfg, 99, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    same = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    other = synth.build_from_raw(cfg, synth.raw_weights_numpy(cfg, 100, w_std=0.1), L.Q4, L.BF16)
    prompt = prompt_ids(cfg, 6, seed=3).tolist()
    ref = m.generate(prompt, N_NEW + 8)
    yield cfg, m, same, other, prompt, ref
    for x in (m, same, other):
        x.close()


def clip_k(k, n_left, pos, n_ctx):
    return max(0, min(k, 7, n_left - 1, n_ctx - 1 - pos))


@pytest.mark.parametrize("k", [1, 4, 7])
def test_a_drafter_with_the_same_weights_is_always_right(gen_case, k):
    cfg, m, same, other, prompt, ref = gen_case
    assert m.generate_speculative(prompt, N_NEW, same, k=k) == ref[:N_NEW]
    s = m.spec_stats()
    assert s["accepted"] == s["proposed"] > 0 and s["rounds"] == -(-N_NEW // (k + 1)), s
    # one-row rounds (a last round with nothing left to draft) are the only rows that do not share the unpack: 6 mat-vec entries per layer pair ... per row
    assert s["rows_shared"] > 0 and s["rows_row_by_row"] <= (4 * cfg["n_layer"] + 1), s


@pytest.mark.parametrize("k", [1, 4, 7])
def test_a_drafter_from_another_seed(gen_case, k):
    cfg, m, same, other, prompt, ref = gen_case
    assert m.generate_speculative(prompt, N_NEW, other, k=k) == ref[:N_NEW]
    s = m.spec_stats()
    assert 0 <= s["accepted"] <= s["proposed"] and s["rounds"] >= -(-N_NEW // (k + 1)), s


@pytest.mark.parametrize("k", [1, 4, 7])
def test_the_lookup_drafter(gen_case, k):
    cfg, m, same, other, prompt, ref = gen_case
    loop = prompt + prompt   # a context that repeats itself: the drafter finds its suffix and proposes
    want = m.generate(loop, N_NEW)
    assert m.generate_speculative(loop, N_NEW, "lookup", k=k, ngram=3) == want
    assert m.spec_stats()["proposed"] > 0
    assert m.generate_speculative(prompt, N_NEW, "lookup", k=k) == ref[:N_NEW]


@pytest.mark.parametrize("k", [1, 4, 7])
def test_partial_acceptance_is_counted_exactly(gen_case, k):
    """a callable that replays the true continuation with every third id replaced: what a round keeps is known in advance"""
    cfg, m, same, other, prompt, ref = gen_case
    wrong = lambda j: j % 3 == 2

    def draft(ids, kk):
        j0 = len(ids) - len(prompt)   # ids emitted so far
        return [(ref[j] + 1) % cfg["vocab"] if wrong(j) else ref[j] for j in range(j0, j0 + kk)]
    assert m.generate_speculative(prompt, N_NEW, draft, k=k) == ref[:N_NEW]
    j = rounds = proposed = accepted = 0
    while j < N_NEW:
        kk = clip_k(k, N_NEW - j, len(prompt) - 1 + j, cfg["max_seq"])
        n_acc = next((i for i in range(kk) if wrong(j + i)), kk)
        rounds, proposed, accepted, j = rounds + 1, proposed + kk, accepted + n_acc, j + n_acc + 1
    s = m.spec_stats()
    assert (s["rounds"], s["proposed"], s["accepted"]) == (rounds, proposed, accepted), s
    assert 0 < accepted < proposed


def test_the_state_it_leaves_behind(gen_case):
    """after a speculative run plain run_steps go on as if generate had run, and the cache rows of the settled ids are the plain run's"""
    cfg, m, same, other, prompt, ref = gen_case
    wrong = lambda j: j % 3 == 2
    draft = lambda ids, kk: [(ref[j] + 1) % cfg["vocab"] if wrong(j) else ref[j] for j in range(len(ids) - len(prompt), len(ids) - len(prompt) + kk)]
    assert m.generate_speculative(prompt, N_NEW, draft, k=4) == ref[:N_NEW]
    pos = len(prompt) + N_NEW - 1   # the row of the last id: rows [0, pos) are in the cache
    m.run_steps(pos, 8)
    m.sync()
    toks = m.tokens_out(pos + 8)
    assert toks[len(prompt) - 1:pos + 8].tolist() == ref
    k1, v1 = m.kv_to_host()
    assert m.generate(prompt, N_NEW + 8) == ref
    k2, v2 = m.kv_to_host()
    assert np.array_equal(k1[:, :pos + 8], k2[:, :pos + 8]) and np.array_equal(v1[:, :pos + 8], v2[:, :pos + 8])


def test_token_batch_prefill_mode(gen_case):
    """generate() with the batched prefill: the speculative run prefills the same way and gives the same ids"""
    cfg, m, same, other, prompt, ref = gen_case
    m.set_prefill_mode(1)
    try:
        want = m.generate(prompt, N_NEW)
        assert m.generate_speculative(prompt, N_NEW, same, k=4) == want
    finally:
        m.set_prefill_mode(0)


def test_small_model(canon):
    cfg = cfg_of("small")
    raw = synth.raw_weights_numpy(cfg, 5, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    try:
        prompt = prompt_ids(cfg, 5, seed=9).tolist()
        ref = m.generate(prompt, 24)
        om = oracle_model(cfg, raw, L.Q4, L.BF16, attn_mode=O.ATTN_CANON)
        assert om.generate(prompt, 24) == ref
        om.close()
        draft = lambda ids, kk: [ref[j] if j % 4 != 3 else 0 for j in range(len(ids) - len(prompt), len(ids) - len(prompt) + kk)]
        assert m.generate_speculative(prompt, 24, draft, k=7) == ref
        assert m.generate_speculative(prompt, 24, "lookup", k=4) == ref
    finally:
        m.close()


def test_one_bit_layers_take_the_row_by_row_route(gen_case):
    """a target whose layers the row kernel does not take: the same entries run the one-token launches row by row -- the ids are still generate's, and spec_stats says so"""
    cfg = cfg_of("tiny")
    raw = synth.raw_weights_numpy(cfg, 21, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.BOOL1, L.BF16)
    try:
        prompt = prompt_ids(cfg, 6, seed=4).tolist()
        ref = m.generate(prompt, 20)
        draft = lambda ids, kk: [ref[j] if j % 3 != 2 else 1 for j in range(len(ids) - len(prompt), len(ids) - len(prompt) + kk)]
        assert m.generate_speculative(prompt, 20, draft, k=4) == ref
        s = m.spec_stats()
        rows = s["proposed"] + s["rounds"]                       # rows of all verify passes
        assert s["rows_row_by_row"] >= 4 * cfg["n_layer"] * rows   # the four mat-vec entries of every layer
        assert s["rows_shared"] <= rows                          # the bf16 head alone shares
    finally:
        m.close()
