"""The persistent engine's hand-offs under a changed issue order between its waves (wave roles and priorities, kf_engine_common.h): whoever wins the issue slots,
every result stays the per-layer launches'.  The 256-wide parity shape (EngCfg EC2: dim 256, 2 kv-heads of 64, ffn 512), 3 layers, vocabulary 4096.  Positions 60..67
cross the bucket boundary 64 (two launches, one attention slice each: kf::attn_slices keeps one slice up to 192 keys, so these steps take the direct ao path only);
positions 124..131 cross the boundary 128, behind which the launch bound is 255 keys in 4 slices: the slice partials and the poller's merge run.  The first-sweep delays are
forced through the non-ABI hook kfdbg_engine_set_delays (kfh_engine_set_delays): 0 makes every first sweep early, so the poller re-sweeps while the compute waves of
its CU still have to publish; 64 makes every first sweep late.  The protocol is correct for any delay: the results must not move and no poll may time out."""
import ctypes as C

import numpy as np
import pytest

from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth

pytestmark = pytest.mark.gpu

N = 8             # steps under test: positions p0 .. p0 + 7
STARTS = [60, 124]
CFG = dict(synth.CONFIGS["tiny"], n_layer=3, vocab=4096, max_seq=256)
_RAW = {}
_REF = {}


def _raw():
    if "w" not in _RAW:
        _RAW["w"] = synth.raw_weights_numpy(CFG, 2024, w_std=0.1)
    return _RAW["w"]


def _forced(P0, teacher):
    """a forced prefix 0 .. p0 - 1; behind it free running (the pick of a step feeds the next one inside the launch) or, teacher = True, forced ids throughout"""
    P1 = P0 + N
    forced = np.full(CFG["max_seq"], -1, dtype=np.int32)
    n = P1 if teacher else P0
    forced[:n] = prompt_ids(CFG, n, seed=17)
    return forced


def _model(P0, layer_type, canonical, teacher):
    """a model that stands at position p0: rows 0 .. p0 - 1 of its cache written by the per-layer launches (the same rows in every case)"""
    m = synth.build_from_raw(CFG, _raw(), layer_type, L.BF16)
    m.set_canonical(canonical)
    m.set_engine_autotune(0)
    m.set_engine(False)
    forced = _forced(P0, teacher)
    m.set_forced(forced)
    m.set_state(int(forced[0]), 0)
    m.run_steps(0, P0, use_graph=True)
    m.sync()
    assert m.engine_steps() <= 0
    return m


def _result(m, P0, p1):
    m.sync()
    m.engine_check()
    k, v = m.kv_to_host()
    return m.tokens_out(p1)[P0:p1].tolist(), m.logits().copy(), k[:, P0:p1].copy(), v[:, P0:p1].copy()


def _reference(P0, layer_type, canonical, teacher, n=N):
    """positions p0 .. p0 + n - 1 through the per-layer launches: computed once per case, shared, never changed"""
    p1 = P0 + n
    key = (P0, layer_type, canonical, teacher, p1)
    if key not in _REF:
        m = _model(P0, layer_type, canonical, teacher)
        m.run_steps(P0, p1 - P0, use_graph=True)
        r = _result(m, P0, p1)
        assert m.engine_steps() <= 0
        m.close()
        for a in r[1:]:
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _engine(P0, layer_type, canonical, teacher, launches, delays=None, screen=True):
    m = _model(P0, layer_type, canonical, teacher)
    if screen:
        m.set_prefill_resident(True)   # the caller's promise: the steps of a launch that are not its last stream the int8 screen of the head
    m.set_engine(True)
    if delays is not None:
        d = (C.c_int * 6)(*delays)
        assert m.host.kfh_engine_set_delays(m.h, d) == 0
    for p, n in launches:
        m.run_steps(p, n, use_graph=True)
    p1 = launches[-1][0] + launches[-1][1]
    r = _result(m, P0, p1)
    assert m.engine_steps() == p1 - P0, m.engine_why()
    st = m.engine_stats(p1 - 1)
    scr = m.engine_screen_stats()
    m.close()
    return r, st, scr


def _assert_bits(got, ref):
    assert got[0] == ref[0], "greedy ids %s vs %s" % (got[0], ref[0])
    assert np.array_equal(got[1], ref[1]), "%d logits of the last step differ" % int((got[1] != ref[1]).sum())
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), "K / V rows differ"


@pytest.mark.parametrize("P0", STARTS)
@pytest.mark.parametrize("delays", [None, [0] * 6, [64] * 6], ids=["built-in delays", "every first sweep early", "every first sweep late"])
def test_bucket_crossing_equals_per_layer_launches(delays, P0):
    """4-bit layers, canonical order, two multi-step launches on the two sides of a bucket boundary (60..63 | 64..67: one attention slice; 124..127 with one slice |
    128..131 with four and the merge), the head screen on: the greedy ids of the 8 steps, the last step's logits and the K / V rows of the 8 positions in every layer
    against the per-layer launches, bit for bit; no timed-out poll (engine_check reads the error word)."""
    ref = _reference(P0, L.Q4, True, False)
    assert len(set(ref[0])) > 2, "degenerate fixture: the free-running ids do not vary"
    got, st, scr = _engine(P0, L.Q4, True, False, [(P0, 4), (P0 + 4, 4)], delays)
    print("delays %s: sweeps per poll (x, q|k|v, partials, ao, xB, act) %s over %d polls; screen %s" % (st["delay"], st["sweeps_per_poll"], st["polls"], scr))
    _assert_bits(got, ref)
    assert scr["screened_steps"] == 6, scr   # all steps of the two launches but their last
    assert (st["sweeps_per_poll"][2] > 0) == (P0 == 124), st   # the slice merge ran behind the boundary 128 and only there
    if delays is not None:
        assert st["delay"] == delays and st["tuned"] == 0, st   # the forced row was the one in use, and it counts as not measured


@pytest.mark.parametrize("P0", STARTS)
def test_dot2_order_against_per_layer_launches(P0):
    """kf_set_canonical(0): the v_dot2c products and the fp32 softmax.  The engine's fp32 attention sums have their own order there (tests/test_gpu_sparse.py compares
    ids only), so against the per-layer launches of that order: teacher-forced positions 60..67 (and 124..131) in one run_steps call; layer 0's K / V rows (they do not depend on any
    attention sum) bit for bit; the picked ids equal wherever the reference's two largest logits are further apart than the bar; the last step's logits within the bar.
    The bar is one bf16 unit in the binade of the largest logit, 2^-7 * max|logit|: both paths store bf16 logits of fp32 sums over the same 256 products, a hidden value
    whose bf16 rounding flipped upstream moves a logit by 2^-8 of ONE of its 256 products -- far below half a unit -- so two stored logits differ by at most one
    rounding flip."""
    ref = _reference(P0, L.Q4, False, True)
    got, st, _ = _engine(P0, L.Q4, False, True, [(P0, N)])
    lr, lg = (ref[1].astype(np.uint32) << 16).view(np.float32), (got[1].astype(np.uint32) << 16).view(np.float32)
    bar = 2.0 ** -7 * float(np.abs(lr).max())
    err = float(np.abs(lg - lr).max())
    print("dot2 order: max |logit difference| %.3g, bar %.3g; ids %s vs %s; sweeps per poll %s" % (err, bar, got[0], ref[0], st["sweeps_per_poll"]))
    assert np.array_equal(got[2][0], ref[2][0]) and np.array_equal(got[3][0], ref[3][0]), "layer 0's K / V rows differ"
    assert err <= bar
    top2 = np.sort(lr)[-2:]
    if top2[1] - top2[0] > bar:
        assert got[0][-1] == ref[0][-1]


@pytest.mark.parametrize("P0", STARTS)
def test_one_bit_storage_equals_per_layer_launches(P0):
    """1-bit layers: BlockPrep's LDS selector-table form, the heaviest work the compute waves do ahead of a hand-off.  One 4-step launch at positions 60..63 (and 124..127): ids, the
    last step's logits and the K / V rows against the per-layer launches, bit for bit."""
    ref = _reference(P0, L.BOOL1, True, False, 4)
    got, st, _ = _engine(P0, L.BOOL1, True, False, [(P0, 4)])
    print("1-bit layers: sweeps per poll %s" % st["sweeps_per_poll"])
    _assert_bits(got, ref)
