"""The persistent engine's canonical attention on ONE fixed reference exponent (koifish_amd/csrc/kf_attn_common.h, KF_CANON_FIX_LIM = 448): no maximum is formed or
exchanged at any level -- wave, slice, merge -- and the engine still equals the per-layer launches (which keep their running maxima) and the CPU oracle bit for bit: ids,
logits, K / V rows.  Here: the seams of the slice geometry inside multi-step launches, a model whose scores reach exponents of 400 and more, the guard beyond the limit,
and the v_dot2c order, which keeps its running maximum."""
import ctypes as C

import numpy as np
import pytest

from fixed_exponent import LIM, build_ref
from helpers import oracle_model, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# the calls of run_steps, (first position, steps): multi-step launches (up to 16 steps each, cut at the position buckets 64 | 128 | 256) that cross
#   63 -> 65     the first bucket boundary; the call ends behind position 65
#   126 .. 132   the boundary between one slice and four slices of 64 keys (a bound of 255): at 128 the new key stands alone in slice 2 and slice 3 is empty
#   190 .. 195   slice 3's first key (192)
CALLS = ((0, 60), (60, 6), (66, 60), (126, 7), (133, 57), (190, 6))
N = 196
SEQ = 256


def _cfg(name):
    return dict(synth.CONFIGS[name], max_seq=SEQ)


def _model(name, c=1.0):
    """(cfg, raw weights with every layer's q-norm and k-norm weight times c, forced ids): a forced prefix of 20 ids, then free running"""
    cfg = _cfg(name)
    raw = synth.raw_weights_numpy(cfg, 4321, w_std=0.1)
    if c != 1.0:
        raw = dict(raw, layers=[dict(lw, qn=O.f32_to_bf16(O.bf16_to_f32(lw["qn"]) * np.float32(c)), kn=O.f32_to_bf16(O.bf16_to_f32(lw["kn"]) * np.float32(c)))
                                for lw in raw["layers"]])
    forced = np.full(SEQ, -1, dtype=np.int32)
    forced[:20] = prompt_ids(cfg, 20, seed=11)
    return cfg, raw, forced


def _oracle_run(cfg, raw, forced, n=N, calls=CALLS):
    """ids of positions 0 .. n - 1, the logits behind the last step of every call, K / V rows 0 .. n - 1"""
    prev = O.get_order()
    O.set_order(O.ORDER_CANON)
    try:
        om = oracle_model(cfg, raw, L.Q4, L.BF16, attn_mode=O.ATTN_CANON)
        ends = {p0 + cnt - 1 for p0, cnt in calls}
        tok, ids, lgs = int(forced[0]), [], {}
        for p in range(n):
            if forced[p] >= 0:
                tok = int(forced[p])
            tok, lg, _ = om.decode(tok, p, want_logits=p in ends)
            ids.append(tok)
            if p in ends:
                lgs[p] = lg
        k, v = om.kv()
        res = (ids, lgs, k[:, :n].copy(), v[:, :n].copy())
        om.close()
    finally:
        O.set_order(prev)
    return res


def _build(cfg, raw, forced, engine, canonical=True):
    m = synth.build_from_raw(cfg, raw, L.Q4, L.BF16)
    m.set_canonical(canonical)
    m.set_engine(engine)
    m.set_forced(forced)
    return m


def _run(m, forced, n=N, calls=CALLS):
    m.set_state(int(forced[0]), 0)
    lgs = {}
    for p0, cnt in calls:
        m.run_steps(p0, cnt, use_graph=True)
        m.sync()
        lgs[p0 + cnt - 1] = m.logits()
    m.engine_check()
    ids = m.tokens_out(n).tolist()
    k, v = m.kv_to_host()
    return ids, lgs, k[:, :n].copy(), v[:, :n].copy()


def _same(got, ref, what):
    assert got[0] == ref[0], "%s: ids differ first at position %d" % (what, next(i for i, (a, b) in enumerate(zip(got[0], ref[0])) if a != b))
    for p in sorted(ref[1]):
        assert np.array_equal(got[1][p], ref[1][p]), "%s: %d logits of position %d differ" % (what, int((got[1][p] != ref[1][p]).sum()), p)
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), "%s: K / V rows differ" % what


def _three_ways(name, c, ref=None):
    cfg, raw, forced = _model(name, c)
    ref = ref or _oracle_run(cfg, raw, forced)
    assert len(set(ref[0][20:])) > 20, "degenerate fixture: the free-running ids do not vary"
    for engine in (True, False):
        m = _build(cfg, raw, forced, engine)
        got = _run(m, forced)
        assert (m.engine_steps() == N) if engine else (m.engine_steps() == 0), m.engine_steps()
        m.close()
        _same(got, ref, "%s, %s against the oracle" % (name, "engine" if engine else "per-layer launches"))


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_seams_engine_equals_per_layer_launches_equals_oracle(name):
    """multi-step launches across 63 -> 65, 126 .. 132 (one slice -> four, the new key alone in its slice, an empty slice behind it) and 190 .. 195 (the empty slice's
    first key): ids of all 196 positions, the logits behind every call, every K / V row"""
    _three_ways(name, 1.0)


@pytest.fixture
def recording_oracle(tmp_path, monkeypatch):
    """the oracle rebuilt with a record of the largest |n| its canonical attention meets (tests/fixed_exponent_ref.c), in place of the oracle library for one test"""
    so = build_ref(tmp_path)
    monkeypatch.setattr(O, "build", lambda force=False: so)
    monkeypatch.setattr(O, "_LIB", None)
    rec = O.lib()
    rec.kfx_max_abs_n.argtypes, rec.kfx_max_abs_n.restype = [C.c_int], C.c_float
    rec.kfx_max_abs_n(1)
    return lambda: float(rec.kfx_max_abs_n(0))


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_wide_range_inside_the_limit(name, recording_oracle):
    """q-norm and k-norm weights times 8 (scores times 64): the largest |n| of the oracle's run is 413 (tiny) / 433 (small) -- recorded on the CPU, asserted to lie in
    [300, 440] -- and the engine, the per-layer launches and the oracle agree bit for bit over the same 196 positions"""
    cfg, raw, forced = _model(name, 8.0)
    ref = _oracle_run(cfg, raw, forced)
    seen = recording_oracle()
    assert 300.0 <= seen <= 440.0, "largest |n| %g: the fixture does not reach the range the test is about" % seen
    _three_ways(name, 8.0, ref)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_guard_beyond_the_limit(name, recording_oracle):
    """the same weights times 10: the largest |n| is 603 (tiny) / 713 (small).  The multi-step run through the engine ends with the error of the fixed-exponent range -- an
    arithmetic flag: every hand-off arrives, nothing waits for a time-out -- and after the reset the per-layer launches reproduce the oracle"""
    cfg, raw, forced = _model(name, 10.0)
    ref = _oracle_run(cfg, raw, forced)
    seen = recording_oracle()
    assert seen > LIM, "largest |n| %g: the fixture does not pass the limit" % seen
    m = _build(cfg, raw, forced, True)
    with pytest.raises(L.KFError, match="fixed-exponent range") as ei:
        _run(m, forced)
    assert "error word 0x80)" in str(ei.value), str(ei.value)   # bit 128 alone: no poll gave up behind the flag
    m.set_engine(False)   # engine_check has reset the engine (Fish::EngineCheck: kf_engine_reset); the per-layer launches serve the model
    m.set_forced(forced)
    got = _run(m, forced)
    m.close()
    _same(got, ref, "%s, per-layer launches behind the guard" % name)


def test_dot2_order_keeps_its_running_maximum():
    """set_canonical(False): the engine's fp32 attention (running integer exponents per wave, rescaled where partials meet) is untouched.  Wide scores (norm weights
    times 10) raise no flag there, and several steps per launch equal one launch per step bit for bit across the same seams."""
    cfg, raw, forced = _model("small", 10.0)
    res = []
    for calls in (CALLS, tuple((p, 1) for p in range(N))):
        m = _build(cfg, raw, forced, True, canonical=False)
        got = _run(m, forced, calls=calls)
        assert m.engine_steps() == N
        m.close()
        res.append(got)
    _same(res[1], res[0], "v_dot2c order, one launch per step against several")


def test_dot2_order_engine_and_per_layer_launches_within_the_default_orders_bar():
    """set_canonical(False), ordinary weights, every id teacher-forced: the engine and the per-layer launches each stay within the default order's bar against the oracle
    (2^-6 of the largest logit, tests/test_gpu_decode.py) behind every call of the seams' schedule, and pick the oracle's ids wherever its two best logits are not that close"""
    cfg, raw, _ = _model("small")
    forced = np.full(SEQ, -1, dtype=np.int32)
    forced[:N] = prompt_ids(cfg, N, seed=12)
    om = oracle_model(cfg, raw, L.Q4, L.BF16)   # the default order's oracle: fp32 softmax, the reference's dot order
    ends = {p0 + cnt - 1 for p0, cnt in CALLS}
    ref = {}
    for p in range(N):
        _, lg, _ = om.decode(int(forced[p]), p, want_logits=p in ends)
        if p in ends:
            ref[p] = O.bf16_to_f32(lg)
    om.close()
    for engine in (True, False):
        m = _build(cfg, raw, forced, engine, canonical=False)
        _, lgs, _, _ = _run(m, forced)
        assert (m.engine_steps() == N) if engine else (m.engine_steps() == 0)
        m.close()
        for p in sorted(ends):
            err = np.abs(O.bf16_to_f32(lgs[p]) - ref[p]).max() / np.abs(ref[p]).max()
            assert err <= 2.0 ** -6, "engine=%s position %d: logits off by %g of the largest" % (engine, p, err)
