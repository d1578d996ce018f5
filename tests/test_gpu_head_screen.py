"""The int8 screen of the engine's in-launch LM head (kf_engine_set_head_screen): on the steps of a multi-step launch that are not its last the engine streams an int8 copy
of the head and re-computes only the rows that can still be the first maximum.  Everything here is compared by EQUALITY against one launch per step, which never screens:
the ids at every position, the last step's logits, the K / V rows -- both summation orders, several vocabularies, ties, the overflow path, the promise and its withdrawal."""
import numpy as np
import pytest
import torch

from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth

pytestmark = pytest.mark.gpu

N = 90   # positions 0 .. 89: a forced prefix, a free-running stretch across the bucket boundary at 64, a forced island, free running again


def _cfg(name, vocab, tied=True):
    cfg = dict(synth.CONFIGS[name])
    cfg["vocab"], cfg["tied"], cfg["max_seq"] = vocab, tied, 160
    return cfg


def _forced(cfg):
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:12] = prompt_ids(cfg, 12, seed=3)
    forced[50:58] = prompt_ids(cfg, 8, seed=4)
    return forced


def _run(m, forced, multi, n=N):
    m.set_forced(forced)
    m.set_state(int(forced[0]), 0)
    if multi:
        m.run_steps(0, 37, use_graph=True)   # launches of up to 16 steps, cut at the bucket boundaries
        m.run_steps(37, n - 37, use_graph=True)
    else:
        for p in range(n):
            m.run_steps(p, 1, use_graph=True)
    m.sync()
    assert m.engine_steps() >= n
    m.engine_check()
    k, v = m.kv_to_host()
    return m.tokens_out(n).tolist(), m.logits().copy(), k[:, :n].copy(), v[:, :n].copy()


def _both(cfg, raw, canonical, promise=True):
    """(single-step result, multi-step result, the multi-step run's counters)"""
    forced = _forced(cfg)
    res, stats = [], None
    for multi in (False, True):
        m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
        m.set_canonical(canonical)
        m.set_prefill_resident(promise)
        res.append(_run(m, forced, multi))
        st = m.engine_screen_stats()
        if multi:
            stats = st
        else:
            assert st == {"screened_steps": 0, "rows_reranked": 0, "wg_fallbacks": 0}, "a single-step launch screened: %s" % st
        m.close()
    return res[0], res[1], stats


def _assert_equal(a, b):
    assert a[0] == b[0], "ids differ at positions %s" % [i for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y][:8]
    assert np.array_equal(a[1], b[1]), "%d logits of the last step differ" % int((a[1] != b[1]).sum())
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), "K / V rows differ"


# vocabularies: whole workgroups; one that does not divide by 256 (157 rows per workgroup, the last ones short); fewer rows than workgroups; the 256-wide shape
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("cfg_name,vocab", [("small", 4096), ("small", 40001), ("small", 200), ("tiny", 512)])
def test_screened_launches_equal_single_steps(cfg_name, vocab, canonical):
    cfg = _cfg(cfg_name, vocab)
    raw = synth.raw_weights_numpy(cfg, 777, w_std=0.1)
    one, many, st = _both(cfg, raw, canonical)
    _assert_equal(one, many)
    assert len(set(one[0][12:50])) > 8, "degenerate fixture: the free-running ids do not vary"
    assert st["screened_steps"] > N // 2, st   # every step of a multi-step launch but its last
    assert st["rows_reranked"] >= st["screened_steps"] or st["wg_fallbacks"] > 0, st
    print("screen counters %s vocab %d canonical=%s: %s" % (cfg_name, vocab, canonical, st))


@pytest.mark.parametrize("canonical", [True, False])
def test_duplicate_rows_pick_the_lower_copy(canonical):
    """the upper half of the head is a copy of the lower half: every logit occurs twice, the first maximum is always the lower copy"""
    cfg = _cfg("small", 4096, tied=False)
    raw = synth.raw_weights_numpy(cfg, 31, w_std=0.1)
    raw["head"][2048:] = raw["head"][:2048]
    one, many, st = _both(cfg, raw, canonical)
    _assert_equal(one, many)
    assert max(many[0]) < 2048, "an upper copy was picked"
    assert st["screened_steps"] > 0, st


def test_equal_rows_overflow_the_candidate_list():
    """every row of the head equal: every row is a candidate, the list (64 rows per workgroup at this width) overflows, the workgroups fall back to the exact stream; pick 0"""
    cfg = _cfg("small", 20000, tied=False)
    raw = synth.raw_weights_numpy(cfg, 32, w_std=0.1)
    raw["head"][:] = raw["head"][0]
    one, many, st = _both(cfg, raw, True)
    _assert_equal(one, many)
    assert set(many[0]) == {0}, sorted(set(many[0]))
    assert st["screened_steps"] > 0 and st["wg_fallbacks"] > 0, st


def test_promise_and_invalidation():
    cfg = _cfg("small", 4096)
    raw = synth.raw_weights_numpy(cfg, 41, w_std=0.1)
    forced = _forced(cfg)
    # without the promise nothing is screened
    _, _, st = _both(cfg, raw, True, promise=False)
    assert st == {"screened_steps": 0, "rows_reranked": 0, "wg_fallbacks": 0}, st
    # with it: screened; then the head changes in place, the caller says so, and the ids follow the new head
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    m.set_prefill_resident(True)
    first = _run(m, forced, True)
    assert m.engine_screen_stats()["screened_steps"] > 0
    raw2 = dict(raw)
    raw2["embed"] = synth.raw_weights_numpy(cfg, 42, w_std=0.1)["embed"]
    w = m.weights[(-1, 1)]
    n_bytes = cfg["vocab"] * cfg["dim"] * 2
    w.blob[:n_bytes].copy_(torch.from_numpy(np.ascontiguousarray(raw2["embed"]).view(np.uint8).reshape(-1)).to(w.blob.device))
    m.weights_changed()
    second = _run(m, forced, True)
    assert m.engine_screen_stats()["screened_steps"] > 0   # the new engine's screen, built from the new head
    # the promise withdrawn: the screen is dropped, later launches stream the bf16 head
    m.set_prefill_resident(False)
    before = m.engine_screen_stats()
    third = _run(m, forced, True)
    assert m.engine_screen_stats() == before
    m.close()
    ref = synth.build_from_raw(cfg, raw2, L.Q4, L.BF16)
    want = _run(ref, forced, False)
    ref.close()
    _assert_equal(want, second)
    _assert_equal(want, third)
    assert first[0] != second[0], "degenerate fixture: the new head picks the same ids"
