"""Batched decode on whole models (Qwen3.generate_batch: regions of the one KV cache, one kf_attn_block_seqs launch per layer for all sequences).  The row route (3 and 8
prompts of unequal lengths, one a single token, 4-bit layers, canonical order) against generate() per prompt, ID FOR ID, and what seqs_route_counts reports.  The
token-batch route (12 prompts on 4-bit layers; 3 on NF4 layers): teacher-forced per-step logits against the token-serial forward() of each sequence within the project's
token-batch bar max|dlogit| <= 2^-6 max|logit|, and -- after the CPU oracle has shown that the seeds keep the reference's top-2 margin above
TWICE that bar at every compared step, so that no admissible error can change the pick -- the greedy ids equal.  A sequence that meets eos parks and the others go on
unchanged; the refusals with their reasons; generate() after the regions are closed."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import oracle_model, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
N_NEW, T_FORCED, BAR = 6, 6, 2.0 ** -6
LENS = [5, 1, 3, 7, 2, 6, 4, 1, 3, 2, 5, 4]   # prompt lengths; with N_NEW ids each fits a region of 256 / 12 = 21 rows
CFG, RAW_SEED = dict(synth.CONFIGS["tiny"], max_seq=256), 4321
# seeds of the teacher-forced sequences, chosen with the CPU oracle ALONE (of 300 .. 419: those whose top-2 margin is above 0.04 max|logit| at all T_FORCED steps)
SEEDS = {L.Q4: [301, 308, 325, 326, 329, 341, 353, 354, 362, 371, 373, 375], L.NF4: [301, 307, 312]}
f32 = lambda u: (np.asarray(u).astype(np.uint32) << 16).view(np.float32)


@pytest.fixture(scope="module")
def cases():
    """per layer storage, built when first asked for: a tiny model in the canonical order with the batched prefill, the prompts, generate()'s ids for each"""
    made = {}

    def get(type_):
        if type_ not in made:
            m = synth.build_from_raw(CFG, synth.raw_weights_numpy(CFG, RAW_SEED, w_std=0.1), type_, L.BF16)
            m.set_canonical(True)
            m.set_prefill_mode(1)
            prompts = [prompt_ids(CFG, n, seed=100 + i).tolist() for i, n in enumerate(LENS)]
            made[type_] = (m, CFG, prompts, [m.generate(p, N_NEW) for p in prompts])
        return made[type_]
    yield get
    for m, _, _, _ in made.values():
        m.close()


@pytest.mark.parametrize("n_seq", [3, 8])
def test_row_route_equals_generate(cases, n_seq):
    m, cfg, prompts, want = cases(L.Q4)
    assert m.generate_batch(prompts[:n_seq], N_NEW) == want[:n_seq]
    r = m.seqs_route_counts()
    assert (r["route"], r["steps"], r["weight_passes"]) == ("rows", N_NEW, N_NEW)   # the one-token prompt needs N_NEW steps; one pass over the weights per step
    assert r["rows_shared"] >= N_NEW * n_seq * 4 * cfg["n_layer"] and r["rows_single"] == 0
    assert m.generate(prompts[0], N_NEW) == want[0]                                 # the regions are closed: generate() gives what it gave


def oracle_margins(type_, ids):
    """min over the sequences and steps of (top-1 - top-2) / max|logit| of the CPU oracle's teacher-forced logits (canonical order: forward()'s own bits)"""
    O.set_order(O.ORDER_CANON)
    try:
        om = oracle_model(CFG, synth.raw_weights_numpy(CFG, RAW_SEED, w_std=0.1), type_, L.BF16, attn_mode=O.ATTN_CANON)
        worst = np.inf
        for seq in ids:
            for p, tok in enumerate(seq):
                lg = np.sort(f32(om.decode(int(tok), p)[1]))
                worst = min(worst, (lg[-1] - lg[-2]) / np.abs(lg).max())
        om.close()
        return worst
    finally:
        O.set_order(O.ORDER_DOT16)


@pytest.mark.parametrize("type_,n_seq", [(L.Q4, 12), (L.NF4, 3)], ids=["q4-12", "nf4-3"])
def test_token_batch_route_within_the_bar(cases, type_, n_seq):
    m, cfg, _, _ = cases(type_)
    ids = [prompt_ids(cfg, T_FORCED, seed=s) for s in SEEDS[type_][:n_seq]]
    ref = np.stack([np.stack([m.forward(int(t), p)[1] for p, t in enumerate(seq)]) for seq in ids])   # [n_seq][T][vocab], token-serial
    got = np.zeros_like(ref)
    host, chk = m.host, m._host_check
    chk(host.kfh_seqs_begin(m.h, n_seq, T_FORCED + 1, -1), "kfh_seqs_begin")
    try:
        for s in range(n_seq):
            chk(host.kfh_seqs_prefill(m.h, s, ids[s][:1].ctypes.data_as(C.c_void_p), 1), "kfh_seqs_prefill")
        chk(host.kfhdbg_seqs_keep_logits(m.h, 1), "kfhdbg_seqs_keep_logits")
        for p in range(T_FORCED):
            chk(host.kfh_seqs_step(m.h, 1), "kfh_seqs_step")
            for s in range(n_seq):
                chk(host.kfhdbg_seqs_logits(m.h, s, got[s, p].ctypes.data_as(C.c_void_p)), "kfhdbg_seqs_logits")
            nxt = np.array([seq[min(p + 1, T_FORCED - 1)] for seq in ids], dtype=np.int32)
            chk(host.kfhdbg_seqs_force(m.h, nxt.ctypes.data_as(C.c_void_p)), "kfhdbg_seqs_force")
        assert m.seqs_route_counts()["route"] == "tiles" and m.seqs_route_counts()["weight_passes"] == T_FORCED
        picked = np.zeros((n_seq, T_FORCED), dtype=np.int32)   # the ids the route itself emitted (kf_head_logprob's top-1 through kf_seqs_advance), one per step
        for s in range(n_seq):
            assert host.kfh_seqs_tokens(m.h, s, picked[s].ctypes.data_as(C.c_void_p), T_FORCED) == T_FORCED
    finally:
        host.kfhdbg_seqs_keep_logits(m.h, 0)
        host.kfh_seqs_end(m.h)
    err = np.abs(f32(got) - f32(ref)).max(axis=2) / np.abs(f32(ref)).max(axis=2)                       # per (sequence, step), in units of max|logit|
    print("token-batch route %s: max |dlogit| / max|logit| = %.3g (bar %.3g)" % (n_seq, err.max(), BAR))
    assert err.max() <= BAR
    assert oracle_margins(type_, ids) > 2 * BAR, "the seeds do not keep the reference's top-2 margin above twice the bar: the ids need not be equal"
    assert np.array_equal(picked, f32(ref).argmax(axis=2)), "the ids the token-batch route picked are not forward()'s"
    assert np.array_equal(f32(got).argmax(axis=2), picked)


def test_eos_parks_one_sequence(cases):
    m, cfg, prompts, want = cases(L.Q4)
    eos = want[1][2]                                    # the third id of sequence 1
    expect = [w[:w.index(eos) + 1] if eos in w else w for w in want[:3]]
    assert len(expect[1]) <= 3
    assert m.generate_batch(prompts[:3], N_NEW, eos=eos) == expect


def test_refusals(cases):
    m, cfg, prompts, want = cases(L.Q4)
    a = torch.zeros((16, cfg["dim"]), dtype=torch.bfloat16, device=m._ctx.device)
    b = torch.zeros((cfg["n_head"] * cfg["head_dim"], 16), dtype=torch.bfloat16, device=m._ctx.device)
    hot = np.ones(cfg["ffn"], dtype=np.int32)
    hot[::2] = 0
    for bad, n_new, why in (([[1]] * 33, 2, "1 .. 32 sequences"), ([[1, cfg["vocab"]]], 2, "outside the vocabulary"),    # 256 / 8 = 32 rows: 5 + 29 - 1 = 33
                            (prompts[:8], 29, r"a prompt of 5 tokens and 29 new ids run past the slot's region of 32 rows \(n_ctx / n_seq\)")):
        with pytest.raises(L.KFError, match=why):
            m.generate_batch(bad, n_new)
    # every mode of the table but TP (below), and a sampler: (switch on, switch off, the reason in the table's words)
    modes = [(lambda: m.set_kv_int8(True), lambda: m.set_kv_int8(False), "the int8 KV cache is on and batched decode has no int8 KV cache form: switch kfh_set_kv_int8 off first"),
             (lambda: m.set_act_int8_q4(True), lambda: m.set_act_int8_q4(False), "int8 activations are on and batched decode has no int8-activation form"),
             (lambda: m.host.kfh_set_adapter(m.h, 0, 0, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), 16, 1.0), m.clear_adapters,
              "adapters are attached and batched decode has no adapter form: clear the adapters first"),
             (lambda: m.set_hot(0, hot), lambda: m.set_hot(0, None), "hot-row mask is set and batched decode has no sparse form"),
             (lambda: m.set_fuse_level(0), lambda: m.set_fuse_level(1), "fuse_level 0 is set and batched decode has no one-launch-per-kernel form"),
             (lambda: m.set_sampler(temperature=0.7, top_k=20), lambda: m.set_sampler(temperature=0.0), "a sampler is set and batched decode accepts greedy ids only")]
    for on, off, why in modes:
        assert on() in (None, 0)
        with pytest.raises(L.KFError, match=why):
            m.generate_batch(prompts[:2], 2)
        off()
    assert m.host.kfh_seqs_begin(m.h, 2, 4, -1) == 0            # while regions are open the entries that share the cache are refused, with the reason
    try:
        with pytest.raises(L.KFError, match="cut into 2 regions of a batched decode .* kfh_seqs_end first"):
            m.generate(prompts[0], 2)
        with pytest.raises(L.KFError, match="regions are open already"):
            m.generate_batch(prompts[:2], 2)
    finally:
        m.host.kfh_seqs_end(m.h)
    assert m.generate_batch(prompts[:3], N_NEW) == want[:3]    # with all of them gone it runs again
    assert m.generate(prompts[0], N_NEW) == want[0]
    m2 = synth.build_from_raw(CFG, synth.raw_weights_numpy(CFG, 7, w_std=0.1), L.Q4, L.BF16)   # a model of its own: a tensor-parallel rank from kfh_tp_init on
    try:
        assert m2.host.kfh_tp_init(m2.h, 0, 2, 0) == 0
        with pytest.raises(L.KFError, match="tensor-parallel rank and batched decode has no tensor-parallel form") as e:
            m2.generate_batch([[1, 2], [3]], 2)
        assert "-1000" in str(e.value)                         # KF_UNSUPPORTED_DATATYPE
    finally:
        m2.close()
