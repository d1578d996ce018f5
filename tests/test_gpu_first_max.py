"""Ties on every path that picks a token.  The pick is the FIRST maximum (first_max, kf_device.h): among equal logits the lowest id wins.  Two heads make ties
certain -- A: the upper half of the head is a copy of the lower half (every logit occurs twice, in different lanes, waves and workgroups of each head kernel);
B: every row equals row 0 (every logit ties) -- and three paths pick over them: the per-launch head (gemv_kernel's arg-max form + argmax_finish_kernel), the verify
pass (gemv_rows_kernel + argmax_rows_finish_kernel in the canonical order, the one-token launches row by row in the other) and the XCD engines' in-launch head.
The expectation is np.argmax of the logits the path itself returns: numpy's argmax is the first maximum."""
import ctypes as C

import numpy as np
import pytest

from helpers import prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from koifish_amd.runtime import XcdReplicas
from test_gemv_rows_plan_cpu import ARGMAX, BF16, OK, Plan, Problem, RowsPlan, RowsProblem, mat

pytestmark = pytest.mark.gpu

N_FORCED, N_FREE = 4, 12


def _cfg(name, max_seq):
    cfg = dict(synth.CONFIGS[name])
    cfg["tied"], cfg["max_seq"] = False, max_seq
    return cfg


def _raw(cfg, fixture):
    raw = synth.raw_weights_numpy(cfg, 31, w_std=0.1)
    half = cfg["vocab"] // 2
    if fixture == "A":
        raw["head"][half:] = raw["head"][:half]
    else:
        raw["head"][:] = raw["head"][0]
    return raw


def _f32(bits):
    """bf16 bit patterns (uint16) -> float32, exactly"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def _check(fixture, ids, logits, vocab, what):
    """ids [n], logits [n, vocab] (bf16 bits): the rule on every step or row"""
    for i, (t, lg) in enumerate(zip(ids, logits)):
        assert int(t) == int(np.argmax(_f32(lg))), "%s %d: id %d is not the first maximum %d" % (what, i, int(t), int(np.argmax(_f32(lg))))
        if fixture == "A":
            assert int(t) < vocab // 2, "%s %d: the upper copy %d was picked" % (what, i, int(t))
        else:
            assert int(t) == 0, "%s %d: id %d of equal rows" % (what, i, int(t))


def test_the_head_kernels_span_several_workgroups():
    """the premise of the fixtures: at this vocabulary both head launches have more than one workgroup, so the two copies of a row meet only in the finish kernels"""
    hip = L.load()[0]
    hip.kfdbg_gemv_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]
    hip.kfdbg_gemv_rows_plan.argtypes = [C.POINTER(RowsProblem), C.POINTER(RowsPlan)]
    cfg = synth.CONFIGS["small"]
    for canon in (0, 1):
        P = Problem(mode=ARGMAX, n_w=1, sparse=0, n_hot=0, norm=1, canon=canon, q4_perm=1, q2_tab=1, q1_tab=1, xf2=1)
        P.w[0] = mat(cfg["vocab"], cfg["dim"], type=BF16)
        one, rows = Plan(), RowsPlan()
        assert hip.kfdbg_gemv_plan(C.byref(P), C.byref(one)) == 0 and one.status == OK and one.grid > 1, (one.status, one.grid)
        if canon:
            assert hip.kfdbg_gemv_rows_plan(C.byref(RowsProblem(P, 8)), C.byref(rows)) == 0 and rows.status == OK and rows.shared == 1 and rows.grid > 1, (rows.status, rows.grid)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("fixture", ["A", "B"])
def test_per_launch_head(fixture, canonical):
    """five launches per layer and the LM head's own launch: 4 forced + 12 free steps, one step per call, the logits read back behind each"""
    cfg = _cfg("small", 32)
    m = synth.build_from_raw(cfg, _raw(cfg, fixture), L.Q4, L.BF16)
    m.set_canonical(canonical)
    m.set_engine(False)
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:N_FORCED] = prompt_ids(cfg, N_FORCED, seed=3)
    m.set_forced(forced)
    m.set_state(int(forced[0]), 0)
    n = N_FORCED + N_FREE
    logits = []
    for p in range(n):
        m.run_steps(p, 1, use_graph=True)
        m.sync()
        logits.append(m.logits())
    ids = m.tokens_out(n).tolist()
    free = range(N_FORCED - 1, n)   # position p's output is forced while p + 1 is a forced position
    _check(fixture, [ids[p] for p in free], [logits[p] for p in free], cfg["vocab"], "position")
    if fixture == "A":
        assert len(set(ids[N_FORCED:])) > 4, "degenerate fixture: the free-running ids do not vary"
    m.close()


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("fixture", ["A", "B"])
def test_verify_rows(fixture, canonical):
    """eight rows in one verify pass: the shared row kernel in the canonical order, the one-token launches row by row in the other"""
    cfg = _cfg("small", 32)
    m = synth.build_from_raw(cfg, _raw(cfg, fixture), L.Q4, L.BF16)
    m.set_canonical(canonical)
    ctx = C.c_void_p(m.host.kfh_ctx(m.h))

    def routes():
        out = (C.c_int64 * 2)()
        L.check(m.hip.kf_rows_route_counts(ctx, out), "kf_rows_route_counts")
        return int(out[0]), int(out[1])
    before = routes()
    top1, logits = m.verify(prompt_ids(cfg, 8, seed=5), 0, want_logits=True)
    shared, row_by_row = (a - b for a, b in zip(routes(), before))
    if canonical:
        assert shared > 0 and row_by_row == 0, (shared, row_by_row)
    else:
        assert shared == 0 and row_by_row > 0, (shared, row_by_row)
    _check(fixture, top1, logits, cfg["vocab"], "row")
    m.close()


@pytest.mark.parametrize("fixture", ["A", "B"])
def test_xcd_replicas(fixture):
    """eight sequences, eight steps, one step per launch so that every step's logits can be read: the in-launch head's pick over the decoder's 32 workgroups"""
    cfg = _cfg("tiny", 96)
    m = synth.build_from_raw(cfg, _raw(cfg, fixture), L.Q4, L.BF16)
    m.set_canonical(True)
    n_seq, n_steps = 8, 8
    xr = XcdReplicas(m, n_seq)
    xr.set_steps_per_launch(1)
    for s in range(n_seq):
        f = np.full(cfg["max_seq"], -1, dtype=np.int32)
        f[:2] = prompt_ids(cfg, 2, seed=100 + s)
        xr.set_forced(s, f)
        xr.set_state(s, int(f[0]), 0)
    logits = [[] for _ in range(n_seq)]
    for _ in range(n_steps):
        xr.run_steps(1)
        m.sync()
        for s in range(n_seq):
            logits[s].append(xr.logits(s))
    xr.check()
    free = range(1, n_steps)   # position 0's output is the forced id of position 1
    seen = set()
    for s in range(n_seq):
        ids = xr.tokens_out(s, n_steps).tolist()
        _check(fixture, [ids[p] for p in free], [logits[s][p] for p in free], cfg["vocab"], "sequence %d position" % s)
        seen.update(ids[2:])
    if fixture == "A":
        assert len(seen) > 4, "degenerate fixture: the free-running ids do not vary"
    xr.close()
    m.close()
