"""The persistent decode engine (kf_engine_*: all layers of a decode step in ONE launch, hand-offs through tagged granules) against the
per-layer launches (kf_norm_linear -> kf_attn_block -> kf_linear -> kf_norm_gateup_swiglu -> kf_linear): the same arithmetic in the same
order, so logits, greedy ids and KV-cache rows must be equal BIT FOR BIT at every position -- single-slice and multi-slice attention,
hipGraph replay and eager launches."""
import numpy as np
import pytest

from helpers import oracle_model, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth

pytestmark = pytest.mark.gpu


def _cfg(name, max_seq=None):
    cfg = dict(synth.CONFIGS[name])
    if max_seq:
        cfg["max_seq"] = max_seq
    return cfg


def _teacher_forced(m, forced, n, use_graph):
    """decode positions 0..n-1 with the ids of `forced`; returns per-step (greedy id, logits)"""
    m.set_forced(forced)
    m.set_state(int(forced[0]), 0)
    out = []
    for p in range(n):
        m.run_steps(p, 1, use_graph=use_graph)
        m.sync()
        out.append((int(m.tokens_out(p + 1)[p]), m.logits()))
    return out


@pytest.mark.parametrize("cfg_name,max_seq,n_steps", [("tiny", 96, 96), ("small", 160, 40), ("tiny", 700, 700), ("small", 320, 300)])
def test_engine_equals_per_layer_launches_bit_for_bit(cfg_name, max_seq, n_steps):
    cfg = _cfg(cfg_name, max_seq)
    raw = synth.raw_weights_numpy(cfg, 4321, w_std=0.1)
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:n_steps] = prompt_ids(cfg, n_steps, seed=11)
    ref_m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    ref_m.set_engine(False)
    ref_m.set_canonical(True)   # bit-identity with the per-layer kernels holds in the canonical order (in the default order the engine's fp32 attention sums are its own)
    ref = _teacher_forced(ref_m, forced, n_steps, use_graph=True)
    assert ref_m.engine_steps() == 0
    rk, rv = ref_m.kv_to_host()
    ref_m.close()
    for use_graph in (True, False):
        m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
        m.set_canonical(True)
        got = _teacher_forced(m, forced, n_steps, use_graph=use_graph)
        assert m.engine_steps() > 0, "the engine was not used (engine_steps = %d)" % m.engine_steps()
        m.engine_check()
        for p in range(n_steps):
            assert got[p][0] == ref[p][0], "graph=%s position %d: greedy id %d vs %d" % (use_graph, p, got[p][0], ref[p][0])
            assert np.array_equal(got[p][1], ref[p][1]), "graph=%s position %d: logits differ in %d places" % (
                use_graph, p, int((got[p][1] != ref[p][1]).sum()))
        k, v = m.kv_to_host()
        assert np.array_equal(k[:, :n_steps], rk[:, :n_steps]) and np.array_equal(v[:, :n_steps], rv[:, :n_steps]), "KV-cache rows differ"
        m.close()


def test_full_size_engine_equals_per_layer_launches_bit_for_bit():
    """The 0.6B instantiation itself (engine_kernel<EngCfg<5, 2, 128, 8, 1024, 2048, 1024, 3072, 256, ...>>, 28 layers, vocab 151 936, in-launch head and pick) against
    the per-layer launches of the SAME model object, teacher-forced over positions 0..63, 250..260, 1020..1030 and 2040..2047 (one slice ... 32 slices, every graph
    bucket): logits, greedy ids and the K / V rows each step writes, bit for bit.  A hand-off race that corrupted one granule in one layer would show here."""
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=4242, layer_type=L.Q4, head_type=L.BF16)
    m.set_canonical(True)   # bit-identity with the per-layer kernels holds in the canonical order
    rng = np.random.default_rng(77)
    toks = rng.integers(0, cfg["vocab"], size=cfg["max_seq"]).astype(np.int32)
    forced = toks.copy()
    m.set_forced(forced)
    total = 0
    for p0, p1 in ((0, 64), (250, 261), (1020, 1031), (2040, 2048)):
        if p0 > 0:
            m.prefill(toks[:p0], want_logits=False)   # rows 0..p0-1 of the cache, shared by both passes
        res = {}
        for engine in (True, False):
            m.set_engine(engine)
            steps0 = m.engine_steps()
            m.set_state(int(toks[p0]), p0)
            out = []
            for p in range(p0, p1):
                m.run_steps(p, 1, use_graph=True)
                m.sync()
                out.append((int(m.tokens_out(p + 1)[p]), m.logits().copy()))
            assert (m.engine_steps() > steps0) == engine
            m.engine_check()
            k, v = m.kv_to_host()
            res[engine] = (out, k[:, p0:p1].copy(), v[:, p0:p1].copy())
        for i, p in enumerate(range(p0, p1)):
            a, b = res[True][0][i], res[False][0][i]
            assert a[0] == b[0], "position %d: greedy id %d vs %d" % (p, a[0], b[0])
            assert np.array_equal(a[1], b[1]), "position %d: %d of %d logits differ" % (p, int((a[1] != b[1]).sum()), a[1].size)
        assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][2], res[False][2]), "K / V rows of positions %d..%d differ" % (p0, p1 - 1)
        total += p1 - p0
    assert total == 94
    m.close()


@pytest.mark.parametrize("canonical", [True, False])
def test_several_steps_per_launch_equal_single_steps(canonical):
    """kf_engine_steps_head: runs of steps inside ONE launch (the picked id handed to the next step's embedding read as a tagged granule) against one launch per step --
    free-running and teacher-forced stretches, across position buckets: ids, the last step's logits and every K / V row, bit for bit, in both summation orders."""
    cfg = _cfg("small", 320)
    raw = synth.raw_weights_numpy(cfg, 777, w_std=0.1)
    n = 150
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:20] = prompt_ids(cfg, 20, seed=3)            # a forced prefix, then free running, then a forced island
    forced[100:110] = prompt_ids(cfg, 10, seed=4)
    res = []
    for multi in (False, True):
        m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
        m.set_canonical(canonical)
        m.set_forced(forced)
        m.set_state(int(forced[0]), 0)
        if multi:
            m.run_steps(0, 37, use_graph=True)           # 37 + 113: launches of up to 16 steps, cut at the bucket boundaries
            m.run_steps(37, n - 37, use_graph=True)
        else:
            for p in range(n):
                m.run_steps(p, 1, use_graph=True)
        m.sync()
        assert m.engine_steps() == n
        m.engine_check()
        k, v = m.kv_to_host()
        res.append((m.tokens_out(n).tolist(), m.logits().copy(), k[:, :n].copy(), v[:, :n].copy()))
        m.close()
    assert res[0][0] == res[1][0], "ids differ"
    assert len(set(res[0][0][20:100])) > 20, "degenerate fixture: the free-running ids do not vary"
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


def test_engine_free_running_ids_match_oracle():
    cfg = _cfg("small", 320)
    raw = synth.raw_weights_numpy(cfg, 1234, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    om = oracle_model(cfg, raw, L.Q4, L.BF16)
    prompt = prompt_ids(cfg, 16)
    ref = om.generate(prompt.tolist(), 24)
    got = m.generate(prompt, 24, use_graph=True)
    assert m.engine_steps() > 0
    m.engine_check()
    assert got == ref, "greedy ids %s differ from the oracle's %s" % (got, ref)
    m.close()


def test_engine_not_served_shapes_fall_back():
    cfg = dict(synth.CONFIGS["tiny"])
    cfg["ffn"] = 768   # not one of the instantiated shapes
    raw = synth.raw_weights_numpy(cfg, 5, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    om = oracle_model(cfg, raw, L.Q4, L.BF16)
    prompt = prompt_ids(cfg, 8)
    assert m.generate(prompt, 8, use_graph=True) == om.generate(prompt.tolist(), 8)
    assert m.engine_steps() == -1
    m.close()


def test_engine_refuses_4bit_groups_other_than_128():
    """The engine kernel has 128-weight groups built in: a 4-bit model of an instantiated shape in groups of 64 is refused at create, with a reason, and decodes through
    the per-layer launches (which read the group size at run time) -- the ids of the same model with the engine switched off, and the oracle's at that group size."""
    cfg = _cfg("small", 64)
    raw = synth.raw_weights_numpy(cfg, 77, w_std=0.1)
    prompt = prompt_ids(cfg, 8)
    ref_m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16, lGroup=64)
    ref_m.set_engine(False)
    ref = ref_m.generate(prompt, 8, use_graph=True)
    ref_m.close()
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16, lGroup=64)
    assert "groups of 128" in m.engine_why(), m.engine_why()
    got = m.generate(prompt, 8, use_graph=True)
    assert m.engine_steps() == -1
    m.close()
    assert got == ref, "greedy ids %s differ from the per-layer launches' %s" % (got, ref)
    om = oracle_model(cfg, raw, L.Q4, L.BF16, lGroup=64)
    assert got == om.generate(prompt.tolist(), 8)


def test_full_size_generations_repeat_bit_for_bit():
    """Soak of the engine inside the suite (round 3 kept it in scratch/): two full greedy decodes of Qwen3-0.6B per summation order (positions 0 .. 2046, runs of up to 16 steps per
    launch, every position bucket and slice count; every fourth id teacher-forced so that the sequence keeps moving) -- the second decode of an order reproduces the first one's
    2047 ids and last logits, and the error word stays clear: no hand-off ever delivered a stale granule, no poll ran out of spins."""
    cfg = synth.CONFIGS["qwen3-0.6b"]
    S = cfg["max_seq"]
    m = synth.build_on_gpu(cfg, seed=1234)
    rng = np.random.default_rng(3)
    forced = np.full(S, -1, dtype=np.int32)
    forced[:128] = rng.integers(0, cfg["vocab"], size=128)
    forced[128::4] = rng.integers(0, cfg["vocab"], size=len(forced[128::4]))
    m.set_forced(forced)
    ref = {}
    for r in range(4):
        canon = (r & 1) == 0
        m.set_canonical(canon)
        m.set_state(int(forced[0]), 0)
        m.run_steps(0, S - 1, use_graph=True)
        m.sync()
        m.engine_check()
        got = (m.tokens_out(S - 1).tolist(), m.logits().copy())
        if canon not in ref:
            ref[canon] = got
        assert got[0] == ref[canon][0], "decode %d differs from the first of its order at index %d" % (r, next(i for i, (a, b) in enumerate(zip(got[0], ref[canon][0])) if a != b))
        assert np.array_equal(got[1], ref[canon][1])
    assert m.engine_steps() >= 4 * (S - 1)
    m.close()


def test_engine_served_says_why_not():
    """kf_engine_served / Fish::EnsureEngine: a model the engine does not serve gets the reason as text, a served one an empty string"""
    cfg = dict(synth.CONFIGS["tiny"])
    cfg["ffn"] = 768
    raw = synth.raw_weights_numpy(cfg, 5, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    why = m.engine_why()
    assert "shape not instantiated" in why, why
    m.close()
    cfg = _cfg("small", 320)
    raw = synth.raw_weights_numpy(cfg, 5, w_std=0.1)
    m = synth.build_from_raw(cfg, raw, L.F8E5M2, L.BF16)   # a storage the engine is not instantiated for
    assert "storage not served" in m.engine_why(), m.engine_why()
    m.close()
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    assert m.engine_why() == ""
    m.close()


def test_engine_tune_changes_timing_not_results():
    """kf_engine_tune (self-calibrated first-sweep delays) and kf_engine_stats: after tuning at several position buckets the decode reproduces the untuned decode's ids, logits
    and K / V rows bit for bit -- the hand-off protocol is correct for any delay -- and the statistics report the delays as measured plus the sweeps per poll."""
    cfg = _cfg("small", 320)
    raw = synth.raw_weights_numpy(cfg, 4242, w_std=0.1)
    n = 260
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:n:3] = prompt_ids(cfg, len(forced[:n:3]), seed=9)
    res = []
    for tune in (0, 3):
        m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
        m.set_canonical(True)
        m.set_engine_autotune(tune)
        m.set_forced(forced)
        m.set_state(int(forced[0]), 0)
        m.run_steps(0, n, use_graph=True)
        m.sync()
        m.engine_check()
        st = m.engine_stats(n - 1)
        assert st["tuned"] == (1 if tune else 0)
        assert st["polls"] > 0 and all(v > 0 for v in st["sweeps_per_poll"][:1])
        if tune:   # an explicit call at the position the state holds: launch time before / after
            before, after = m.engine_tune(1)
            assert before > 0 and after > 0 and after <= before * 1.05
        k, v = m.kv_to_host()
        res.append((m.tokens_out(n).tolist(), m.logits().copy(), k[:, :n].copy(), v[:, :n].copy()))
        m.close()
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


def test_qwen3_1p7b_shape_engine_equals_per_layer_launches_bit_for_bit():
    """The Qwen3-1.7B instantiation (engine_kernel<EngCfg<5, 2, 128, 8, 2048, 2048, 1024, 6144, 256, ...>>: the 0.6B head geometry on a 2048-wide stream; gate | up and
    down_proj hold 8 and 6 blocks per lane, part of them dequantised behind the hand-off -- MvPhase::AH) at full size against the per-layer launches of the same model,
    canonical order, teacher-forced over positions 0..31, 250..258 and 2040..2047: logits, greedy ids and the K / V rows each step writes, bit for bit."""
    cfg = dict(synth.CONFIGS["qwen3-1.7b"])
    m = synth.build_on_gpu(cfg, seed=4243, layer_type=L.Q4, head_type=L.BF16)
    m.set_canonical(True)
    assert m.engine_why() == "", m.engine_why()
    toks = np.random.default_rng(78).integers(0, cfg["vocab"], size=cfg["max_seq"]).astype(np.int32)
    m.set_forced(toks.copy())
    for p0, p1 in ((0, 32), (250, 259), (2040, 2048)):
        if p0 > 0:
            m.prefill(toks[:p0], want_logits=False)
        res = {}
        for engine in (True, False):
            m.set_engine(engine)
            steps0 = m.engine_steps()
            m.set_state(int(toks[p0]), p0)
            out = []
            for p in range(p0, p1):
                m.run_steps(p, 1, use_graph=True)
                m.sync()
                out.append((int(m.tokens_out(p + 1)[p]), m.logits().copy()))
            assert (m.engine_steps() > steps0) == engine
            m.engine_check()
            k, v = m.kv_to_host()
            res[engine] = (out, k[:, p0:p1].copy(), v[:, p0:p1].copy())
        for i, p in enumerate(range(p0, p1)):
            a, b = res[True][0][i], res[False][0][i]
            assert a[0] == b[0], "position %d: greedy id %d vs %d" % (p, a[0], b[0])
            assert np.array_equal(a[1], b[1]), "position %d: %d of %d logits differ" % (p, int((a[1] != b[1]).sum()), a[1].size)
        assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][2], res[False][2]), "K / V rows of positions %d..%d differ" % (p0, p1 - 1)
    # several steps per launch, free running: the same ids as one launch per step
    m.set_engine(True)
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:1990] = toks[:1990]
    m.set_forced(forced)
    ids = {}
    for per_launch in (1, 16):
        m.set_state(int(toks[1984]), 1984)
        for p in range(1984, 2040, per_launch):
            m.run_steps(p, per_launch, use_graph=True)
        m.sync()
        m.engine_check()
        ids[per_launch] = np.asarray(m.tokens_out(cfg["max_seq"])[1985:2040]).copy()
    assert np.array_equal(ids[1], ids[16])
    m.close()


def test_engine_on_a_second_device():
    """The 160 KB ceiling of a kernel's dynamic LDS is an attribute per device, raised before an engine form's first launch on each (kf::eng_raise_lds): the same weights
    built on device 0 and then on device 1 in this process give the same ids through the engine, and the error word stays clear on both."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    cfg = _cfg("small", 64)
    raw = synth.raw_weights_numpy(cfg, 1234, w_std=0.1)
    prompt = prompt_ids(cfg, 8)
    ids = []
    try:
        for device in (0, 1):
            m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16, device=device)
            ids.append(m.generate(prompt, 8, use_graph=True))
            assert m.engine_steps() > 0, "device %d: the engine was not used (%s)" % (device, m.engine_why())
            m.engine_check()
            m.close()
    finally:
        torch.cuda.set_device(0)
    assert ids[0] == ids[1], "greedy ids on device 1 %s differ from device 0's %s" % (ids[1], ids[0])
