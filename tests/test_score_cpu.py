"""Scoring without a GPU: the route plan of kf_head_logprob (kf::score_plan through kfdbg_score_plan, and kf_head_logprob_scratch_bytes called directly), and the
perplexity arithmetic of Fish::Eval_ppl (Evaluate.cpp:64-80) as koifish_amd.runtime.perplexity_from_logprobs restates it."""
import ctypes as C

import numpy as np
import pytest

from koifish_amd import lib as L
from koifish_amd.runtime import perplexity_from_logprobs
from plan_structs import GemmMat as Mat, ScorePlan as Plan, ScoreProblem as Problem

BF16, Q4 = 3, 14                 # kf_dtype
GROUP, ROW_LUT = 0, 1            # quant forms
FUSED, PANEL = 0, 1              # ScoreRoute
BIG, SMALL = 0, 1                # G3 forms
V = 151936
QWEN3_DIMS = (1024, 2048, 2560, 4096, 5120)
ROWS = (1, 7, 128, 2047, 8192)


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def plan(hip):
    hip.kfdbg_score_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]

    def f(M, K, n, type=BF16, quant=GROUP, awq=0, al=3, x_al=1, force=0, form=-1):
        P = Problem(w=Mat(type, quant, awq, M, K, 128, int(type != BF16), al), n=n, x_al=x_al, force=force, form=form)
        out = Plan()
        assert hip.kfdbg_score_plan(C.byref(P), C.byref(out)) == 0
        return out
    return f


@pytest.mark.parametrize("dim", QWEN3_DIMS)
@pytest.mark.parametrize("n", ROWS)
def test_bf16_head_takes_the_fused_route(plan, dim, n):
    p = plan(V, dim, n)
    big = n >= 512                                                     # SCORE_BIG_MIN_ROWS: 256 x 256 tiles from there, 128 x 128 below
    t, nvt = (256, 594) if big else (128, 1187)                        # 151 936 = 1187 x 128 = 593.5 x 256
    assert (p.route, p.status, p.form) == (FUSED, 0, BIG if big else SMALL)
    assert (p.n_vt, p.n_rb) == (nvt, (n + t - 1) // t)
    assert (p.gx, p.block, p.lds) == (nvt * ((n + t - 1) // t), 512 if big else 256, 131072 if big else 65536)
    assert p.scratch >= n * 1187 * 16 and p.scratch % 256 == 0         # one 16-byte partial per row and 128-row vocabulary tile, whatever the form: grows with n
    assert p.scratch * 8 < n * V * 2                                   # far below the logit matrix at every size, not only where the issue asks


@pytest.mark.parametrize("kw", [dict(type=Q4), dict(type=Q4, quant=ROW_LUT), dict(type=Q4, awq=1), dict(K=1000), dict(K=1024 + 32), dict(al=0), dict(x_al=0),
                                dict(force=1)])
@pytest.mark.parametrize("n", ROWS)
def test_everything_else_takes_the_panel_route(plan, kw, n):
    kw = dict(kw)
    p = plan(V, kw.pop("K", 1024), n, **kw)
    assert (p.route, p.status) == (PANEL, 0)                           # never "unsupported"
    assert p.panel_rows == min(n, 128)
    assert p.scratch >= p.panel_rows * V * 2


def test_tile_form_hook_and_bad_shapes(plan):
    p = plan(V, 1024, 2047, form=SMALL)
    assert (p.route, p.form, p.n_vt, p.n_rb, p.block, p.lds) == (FUSED, SMALL, 1187, 16, 256, 65536)
    p = plan(V, 1024, 128, form=BIG)
    assert (p.route, p.form, p.n_vt, p.n_rb, p.block, p.lds) == (FUSED, BIG, 594, 1, 512, 131072)
    assert plan(V, 1024, 511).form == SMALL and plan(V, 1024, 512).form == BIG
    assert plan(V, 1024, 0).status == -20 and plan(0, 1024, 4).status == -20


def test_scratch_query_is_the_plan_and_an_eighth_of_the_logits(hip, plan):
    hip.kf_head_logprob_scratch_bytes.argtypes, hip.kf_head_logprob_scratch_bytes.restype = [C.POINTER(L.Weight), C.c_int], C.c_size_t
    w = L.Weight(None, None, L.BF16, V, 1024, 0, 0, 0, 0, 0, None, None)
    need = hip.kf_head_logprob_scratch_bytes(C.byref(w), 2047)
    assert need == plan(V, 1024, 2047).scratch
    assert 0 < need < 2047 * V * 2 // 8                                # the point of the kernel: 622 MB of logits are never written
    q = L.Weight(None, 16, L.Q4, V, 1024, V * 1024 // 128, 128, 0, 15, 0, None, None)
    assert hip.kf_head_logprob_scratch_bytes(C.byref(q), 2047) == plan(V, 1024, 2047, type=Q4).scratch
    assert hip.kf_head_logprob_scratch_bytes(C.byref(w), 0) == 0


def _reference(lp):
    lp = np.asarray(lp, dtype=np.float64)
    nz = lp.size
    s, ss = lp.sum(), (lp * lp).sum()
    ppl = np.exp(-s / nz)
    return ppl, ppl * np.sqrt((ss - s * s / nz) / nz / nz)


@pytest.mark.parametrize("lp", [np.full(100, -2.5), -np.abs(np.random.default_rng(3).normal(3.0, 2.0, size=4097)), np.array([-0.75])], ids=["constant", "random", "one"])
def test_perplexity_arithmetic(lp):
    ppl, err, nz = perplexity_from_logprobs(lp)
    want_ppl, want_err = _reference(lp)
    assert nz == len(lp)
    assert abs(ppl - np.exp(-np.mean(lp))) <= 1e-12 * np.exp(-np.mean(lp))
    assert abs(ppl - want_ppl) <= 1e-12 * want_ppl
    if len(lp) == 1 or np.ptp(lp) == 0:
        assert err <= 1e-6 * ppl                                       # no spread: the variance term is rounding noise around zero
    else:
        assert abs(err - want_err) <= 1e-12 * want_err


def test_uniform_distribution_has_perplexity_v():
    ppl, err, nz = perplexity_from_logprobs(np.full(2047, -np.log(float(V))))
    assert abs(ppl - V) <= 1e-9 * V and nz == 2047
    with pytest.raises(ValueError):
        perplexity_from_logprobs([])
