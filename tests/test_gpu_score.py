"""Scoring on the device: kf_head_logprob (the LM head with the log-softmax in its epilogue) against numpy fp64, its two routes against each other, and
Qwen3.score / Qwen3.perplexity (Fish::Score / Fish::EvalPPL, the reference's Fish_ppl / Fish::Eval_ppl as a batch) against the CPU oracle's token-serial logits.

The bound used throughout is derived, not measured: log-sum-exp is 1-Lipschitz in the sup norm, so two logit rows within d of each other give log-sum-exps within d
and log-probs within 2 d.  Operator tests: d = 2^-7 max|logit of the row| (the device's bf16 rounding may land one ulp off where the fp32 sum order differs, and a bf16
ulp is at most 2^-7 of the value).  Model tests: d = 2^-6 max|oracle logits at t|, the project's token-batch bar (tests/test_gpu_prefill.py LOGIT_TOL)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from conftest import bf16_t, u16
from helpers import oracle_model, prompt_ids
from koifish_amd import lib as L
from koifish_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2.0 ** -6
ULP = 2.0 ** -7
TIE_CAP = 0.02


# ---------------------------------------------------------------------------------------------------------------- the operator
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _head_logprob(ctx, w, x_t, targets):
    """one kf_head_logprob call: (logprob, lse, top1) as numpy; the outputs start as a fill value that no row may keep"""
    ctx.hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    n = x_t.shape[0]
    d = w.desc()
    need = ctx.hip.kf_head_logprob_scratch_bytes(C.byref(d), n)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=ctx.device)
    tg = torch.from_numpy(np.asarray(targets, dtype=np.int32)).to(ctx.device)
    lp = torch.full((n,), 7.0, dtype=torch.float32, device=ctx.device)
    lse = torch.full((n,), 7.0e9, dtype=torch.float32, device=ctx.device)
    top1 = torch.full((n,), -5, dtype=torch.int32, device=ctx.device)
    ctx.linear_scratch(w, min(n, 128))
    rc = ctx.hip.kf_head_logprob(ctx.h, C.byref(d), _ptr(x_t), x_t.shape[1], n, _ptr(tg), _ptr(lp), _ptr(lse), _ptr(top1), _ptr(ws))
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    return lp.cpu().numpy(), lse.cpu().numpy(), top1.cpu().numpy()


def _expected(W_t, x_t):
    """bf16-rounded logits of fp64 dot products of the same bf16 inputs, [rows, V] fp64 on the host (the product itself in fp64 on the device: torch, not this library)"""
    lg = (x_t.to(torch.float64) @ W_t.to(torch.float64).T).to(torch.float32).to(torch.bfloat16).to(torch.float64)
    return lg.cpu().numpy()


def _logprobs64(logits, targets):
    m = logits.max(axis=1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(axis=1))
    t = np.asarray(targets)
    lp = np.where(t >= 0, logits[np.arange(len(t)), np.maximum(t, 0)] - lse, 0.0)
    return lp, lse


def _planted(rows, V, dim, seed, device):
    """W ~ N(0, 1 / dim) and x[t] = N(0, 1) + 10 W[w_t] with w_t spread over the vocabulary: every row has ONE clear winner (logit ~ 10 against a field of N(0, 1)), so
    the fp64 expectation has no top-2 near-tie (plain Gaussian logits have one within 2^-7 of the maximum on ~ 1 row in 6, whatever their scale) and the winner's
    index is in a different vocabulary tile from row to row -- what the index merge has to get right."""
    rng = np.random.default_rng(seed)
    W = synth.f32_to_bf16_np(rng.normal(0.0, 1.0 / np.sqrt(dim), size=(V, dim)).astype(np.float32))
    win = rng.integers(0, V, size=rows)
    win[0] = V - 1                                                   # the last column of the last (edge) tile
    x = rng.normal(0.0, 1.0, size=(rows, dim)).astype(np.float32) + 10.0 * O.bf16_to_f32(W[win])
    targets = rng.integers(0, V, size=rows).astype(np.int32)
    targets[::5] = win[::5]                                          # likely and unlikely targets
    targets[1::7] = -1
    if rows > 2:
        targets[2] = V - 1
    return bf16_t(W, device), bf16_t(synth.f32_to_bf16_np(x), device), targets, win


def _check_rows(got, logits, targets, what):
    lp, lse, top1 = got
    want_lp, want_lse = _logprobs64(logits, targets)
    d = ULP * np.abs(logits).max(axis=1)
    first = logits.argmax(axis=1)                                    # numpy: the first maximum
    srt = np.sort(logits, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > d
    assert clear.mean() >= 1.0 - TIE_CAP, "%s: the fp64 expectation itself has top-2 near-ties on %.1f %% of rows" % (what, 100 * (1 - clear.mean()))
    print("%s: max |dlp| / 2d = %.3f, max |dlse| / d = %.3f, top1 differs on %d of %d rows" % (
        what, (np.abs(lp - want_lp) / (2 * d)).max(), (np.abs(lse - want_lse) / d).max(), int((top1 != first).sum()), len(first)))
    assert (np.abs(lp - want_lp) <= 2 * d).all(), what
    assert (np.abs(lse - want_lse) <= d).all(), what
    assert (lp[np.asarray(targets) < 0] == 0.0).all(), what
    assert ((top1 >= 0) & (top1 < logits.shape[1])).all(), what
    r = np.arange(len(first))
    excused = (top1 != first) & (np.abs(logits[r, top1] - logits[r, first]) <= d)
    assert ((top1 == first) | excused).all(), what
    assert excused.mean() <= TIE_CAP, what


CASES = [(1, 512, 256), (33, 4096, 1024), (130, 4096 + 128, 1024), (130, 4096 + 72, 1024), (257, 1000, 64), (300, 151936, 1024),
         (600, 4096 + 72, 1024), (513, 1000, 64)]   # the last two: the 256 x 256 tile (from 512 rows), ragged in both directions


@pytest.mark.parametrize("rows,V,dim", CASES)
def test_head_logprob_fused_vs_fp64(ctx, rows, V, dim):
    """the fused route: a bf16 head; edges in every direction (one row, rows past a row block, a vocabulary that ends inside a tile, the real Qwen3 vocabulary)"""
    W_t, x_t, targets, _ = _planted(rows, V, dim, seed=rows + V, device=ctx.device)
    w = ctx.quantize(W_t, L.BF16)
    _check_rows(_head_logprob(ctx, w, x_t, targets), _expected(W_t, x_t), targets, "fused %d x %d x %d" % (rows, V, dim))


@pytest.mark.parametrize("type_", [L.Q4, L.NF4])
def test_head_logprob_panel_route_quantised_head_vs_fp64(ctx, type_):
    rows, V, dim = 33, 4096, 1024
    W_t, x_t, targets, _ = _planted(rows, V, dim, seed=77, device=ctx.device)
    w = ctx.quantize(W_t, type_)
    Wq = ctx.dequant(w)                                              # the head the kernel multiplies: the quantised one
    _check_rows(_head_logprob(ctx, w, x_t, targets), _expected(Wq, x_t), targets, "panel, head type %d" % type_)


def test_head_logprob_odd_dim_takes_the_panel_route(ctx):
    rows, V, dim = 9, 640, 200                                       # 200 is no multiple of the tile's k step
    W_t, x_t, targets, _ = _planted(rows, V, dim, seed=5, device=ctx.device)
    w = ctx.quantize(W_t, L.BF16)
    _check_rows(_head_logprob(ctx, w, x_t, targets), _expected(W_t, x_t), targets, "panel, dim 200")


def test_equal_maxima_in_two_tiles_pick_the_lower_index(ctx):
    """the row maximum planted twice, in two different vocabulary tiles, with exactly equal bf16 values (two identical rows of W give identical sums): top1 is the lower
    index -- on both routes"""
    rows, V, dim = 40, 4096, 256
    W_t, x_t, targets, win = _planted(rows, V, dim, seed=11, device=ctx.device)
    lo = (win % 1500).astype(np.int64)
    hi = lo + 128 * (3 + np.arange(rows) % 11)                       # 3 .. 13 tiles further up
    W = u16(W_t).copy()
    x = np.zeros((rows, dim), dtype=np.float32)
    for t in range(rows):
        W[hi[t]] = W[lo[t]]
    Wf = O.bf16_to_f32(W)
    for t in range(rows):
        x[t] = 10.0 * Wf[lo[t]]
    rng = np.random.default_rng(1)
    x += rng.normal(0.0, 0.3, size=x.shape).astype(np.float32)
    W_t, x_t = bf16_t(W, ctx.device), bf16_t(synth.f32_to_bf16_np(x), ctx.device)
    logits = _expected(W_t, x_t)
    r = np.arange(rows)
    first = logits.argmax(axis=1)                                    # numpy: the first of the equal maxima
    assert (logits[r, hi] == logits.max(axis=1)).all() and (first < hi).all() and (first // 128 != hi // 128).all() and (first == lo).mean() > 0.9
    w = ctx.quantize(W_t, L.BF16)
    for route in (0, 1):
        ctx.hip.kfdbg_set_knob(b"score_route", route)
        try:
            _, _, top1 = _head_logprob(ctx, w, x_t, targets)
        finally:
            ctx.hip.kfdbg_set_knob(b"score_route", 0)
        assert (top1 == first).all(), "route %d: %s vs %s" % (route, top1.tolist(), first.tolist())


@pytest.mark.parametrize("rows,V,dim", [(130, 4096 + 72, 1024), (300, 151936, 1024), (600, 4096 + 72, 1024)])
def test_fused_route_equals_panel_route(ctx, rows, V, dim):
    W_t, x_t, targets, _ = _planted(rows, V, dim, seed=3 + rows, device=ctx.device)
    w = ctx.quantize(W_t, L.BF16)
    fused = _head_logprob(ctx, w, x_t, targets)
    ctx.hip.kfdbg_set_knob(b"score_route", 1)
    try:
        panel = _head_logprob(ctx, w, x_t, targets)
    finally:
        ctx.hip.kfdbg_set_knob(b"score_route", 0)
    logits = _expected(W_t, x_t)
    d = ULP * np.abs(logits).max(axis=1)
    print("fused vs panel: max |dlp| / 2d = %.3f" % (np.abs(fused[0] - panel[0]) / (2 * d)).max())
    assert (np.abs(fused[0] - panel[0]) <= 2 * d).all()
    assert (np.abs(fused[1] - panel[1]) <= d).all()
    r = np.arange(rows)
    diff = fused[2] != panel[2]
    assert (~diff | (np.abs(logits[r, fused[2]] - logits[r, panel[2]]) <= d)).all()
    assert diff.mean() <= TIE_CAP
    _check_rows(panel, logits, targets, "panel (forced) %d x %d" % (rows, V))


def test_head_logprob_bad_args(ctx):
    W_t, x_t, targets, _ = _planted(8, 512, 256, seed=2, device=ctx.device)
    w = ctx.quantize(W_t, L.BF16)
    d = w.desc()
    ws = torch.empty(ctx.hip.kf_head_logprob_scratch_bytes(C.byref(d), 8), dtype=torch.uint8, device=ctx.device)
    tg = torch.zeros(8, dtype=torch.int32, device=ctx.device)
    lp = torch.zeros(8, dtype=torch.float32, device=ctx.device)
    call = ctx.hip.kf_head_logprob
    assert call(ctx.h, C.byref(d), _ptr(x_t), 256, 0, _ptr(tg), _ptr(lp), None, None, _ptr(ws)) == -20
    assert call(ctx.h, C.byref(d), _ptr(x_t), 256, 8, None, _ptr(lp), None, None, _ptr(ws)) == -20
    assert call(ctx.h, C.byref(d), _ptr(x_t), 128, 8, _ptr(tg), _ptr(lp), None, None, _ptr(ws)) == -20       # ldx below dim
    assert call(ctx.h, C.byref(d), C.c_void_p(x_t.data_ptr() + 2), 256, 7, _ptr(tg), _ptr(lp), None, None, _ptr(ws)) == -2000
    assert call(ctx.h, C.byref(d), _ptr(x_t), 256, 8, _ptr(tg), _ptr(lp), None, None, _ptr(ws)) == 0         # lse / top1 are optional
    ctx.sync()


# ---------------------------------------------------------------------------------------------------------------- the model
def _pair(cfg_name, layer_type, head_type, n_prompt, seed=1234, w_std=0.02):
    cfg = synth.CONFIGS[cfg_name]
    raw = synth.raw_weights_numpy(cfg, seed, w_std=w_std)
    gm = synth.build_from_raw(cfg, raw, layer_type, head_type)
    om = oracle_model(cfg, raw, layer_type, head_type)
    return cfg, gm, om, prompt_ids(cfg, n_prompt)


def _oracle_scores(om, prompt):
    """per position t < n - 1: log P(prompt[t + 1]) in fp64 from the oracle's token-serial bf16 logits, and the bar 2 * 2^-6 * max|logits at t|"""
    lp, bar = [], []
    for pos, tok in enumerate(prompt[:-1]):
        _, logits, _ = om.decode(int(tok), pos)
        f = O.bf16_to_f32(logits).astype(np.float64)
        m = f.max()
        lp.append(f[int(prompt[pos + 1])] - (m + np.log(np.exp(f - m).sum())))
        bar.append(2 * LOGIT_TOL * np.abs(f).max())
    return np.array(lp), np.array(bar)


def _assert_scores(got, want, bar, what):
    assert got.shape == want.shape, what
    print("%s: max |dlp| / bar = %.3f over %d tokens" % (what, (np.abs(got - want) / bar).max(), len(want)))
    assert (np.abs(got - want) <= bar).all(), "%s: token %d off by %g, bar %g" % (what, int(np.argmax(np.abs(got - want) / bar)), np.abs(got - want).max(), bar.max())


def _assert_ppl(gm, prompt, want_lp, bar, what):
    ppl, err, nz = gm.perplexity(prompt)
    want = np.exp(-want_lp.mean())
    assert nz == len(prompt) - 1
    assert abs(np.log(ppl) - np.log(want)) <= bar.mean(), "%s: ppl %g vs %g" % (what, ppl, want)   # |d log ppl| <= the mean of the per-token bounds
    assert err >= 0.0 and np.isfinite(err)


@pytest.mark.parametrize("cfg_name,layer_type,head_type,n", [("tiny", L.Q4, L.BF16, 40), ("tiny", L.BOOL1, L.BF16, 40), ("tiny", L.Q4, L.Q4, 9), ("small", L.Q4, L.BF16, 130),
                                                             ("tiny", L.NF4, L.BF16, 40)])
def test_score_and_perplexity_vs_oracle(cfg_name, layer_type, head_type, n):
    cfg, gm, om, prompt = _pair(cfg_name, layer_type, head_type, n)
    want, bar = _oracle_scores(om, prompt)
    got, top1 = gm.score(prompt, want_top1=True)
    assert got.dtype == np.float32 and top1.dtype == np.int32 and top1.shape == (n - 1,)
    what = "%s layers %d head %d" % (cfg_name, layer_type, head_type)
    _assert_scores(got.astype(np.float64), want, bar, what)
    assert (got <= 0).all() and ((top1 >= 0) & (top1 < cfg["vocab"])).all()
    _assert_ppl(gm, prompt, want, bar, what)
    gm.close()


def test_score_chunked_and_in_two_calls():
    """a 50-token prompt in chunks of 16 rows gives 49 values, the pair across every chunk boundary included, equal to one chunk's within the bar.  In two calls --
    score(prompt[:21]) then score(prompt[21:], pos0=21) -- 20 and 28 values come back: values 0 .. 19 and 21 .. 48 of the one-call result; value 20, log P(prompt[21] |
    prompt[:21]), is by definition produced by neither call: the first never saw its target, the second scores only what follows its own first token."""
    cfg, gm, om, prompt = _pair("tiny", L.Q4, L.BF16, 50)
    want, bar = _oracle_scores(om, prompt)
    one = gm.score(prompt).astype(np.float64)
    _assert_scores(one, want, bar, "one chunk")
    cfg, gc, _, _ = _pair("tiny", L.Q4, L.BF16, 50)
    gc.set_prefill_mode(1, chunk=16)
    chunked = gc.score(prompt).astype(np.float64)
    assert chunked.shape == (49,)
    _assert_scores(chunked, want, bar, "chunks of 16 vs oracle")
    assert (np.abs(chunked - one) <= bar).all()
    cfg, g2, _, _ = _pair("tiny", L.Q4, L.BF16, 50)
    a = g2.score(prompt[:21]).astype(np.float64)
    b = g2.score(prompt[21:], pos0=21).astype(np.float64)
    assert a.shape == (20,) and b.shape == (28,)
    assert (np.abs(a - one[:20]) <= bar[:20]).all()
    assert (np.abs(b - one[21:]) <= bar[21:]).all()
    _assert_scores(b, want[21:], bar[21:], "second call vs oracle")
    for m in (gm, gc, g2):
        m.close()


@pytest.mark.parametrize("layer_type", [L.Q4, L.BF16])
def test_score_leaves_the_state_prefill_leaves(layer_type):
    """after score(prompt): logits, next id, K / V rows [0, n) and a following run_steps are what they are after prefill(prompt) on a second model of the same
    weights -- bit for bit (same kernels, same order)"""
    n, n_more = 40, 12
    cfg, ga, _, prompt = _pair("tiny", layer_type, L.BF16, n)
    cfg, gb, _, _ = _pair("tiny", layer_type, L.BF16, n)
    ga.score(prompt)
    nb, lb = gb.prefill(prompt)
    assert int(ga.tokens_out(n)[n - 1]) == nb
    assert (ga.logits() == lb).all()
    (ka, va), (kb, vb) = ga.kv_to_host(), gb.kv_to_host()
    assert (ka[:, :n] == kb[:, :n]).all() and (va[:, :n] == vb[:, :n]).all()
    forced = np.full(cfg["max_seq"], -1, dtype=np.int32)
    forced[:n] = prompt
    for g in (ga, gb):
        g.set_forced(forced)
        g.run_steps(n, n_more)
        g.sync()
    assert (ga.tokens_out(n + n_more) == gb.tokens_out(n + n_more)).all()
    assert (ga.logits() == gb.logits()).all()
    ga.close()
    gb.close()


def test_score_of_a_sparse_model_vs_masked_oracle():
    """hot-row masks set as tests/test_gpu_sparse.py sets them: the scores follow the masked oracle within the bar, and differ from the dense model's by more than the
    bar on at least one token (the mask is really applied)"""
    from test_gpu_sparse import hot_mask
    cfg, gm, om, prompt = _pair("small", L.Q4, L.BF16, 60)
    dense = gm.score(prompt).astype(np.float64)
    for l in range(cfg["n_layer"]):
        hot = hot_mask(cfg["ffn"], 0.2, seed=5 + l)
        gm.set_hot(l, hot)
        om.set_hot(l, hot)
    want, bar = _oracle_scores(om, prompt)
    sparse = gm.score(prompt).astype(np.float64)
    _assert_scores(sparse, want, bar, "sparse vs masked oracle")
    assert (np.abs(sparse - dense) > bar).any(), "masked and dense scores agree within the bar: the mask changes nothing"
    gm.close()


def test_score_agrees_with_the_decode_path():
    """log-probs computed on the host from forward(token, pos) logits (the decode kernels) against score() (the token-batch kernels and the fused head)"""
    cfg, gm, _, prompt = _pair("small", L.Q4, L.BF16, 48)
    got = gm.score(prompt).astype(np.float64)
    lp, bar = [], []
    for pos, tok in enumerate(prompt[:-1]):
        _, logits = gm.forward(int(tok), pos)
        f = O.bf16_to_f32(logits).astype(np.float64)
        m = f.max()
        lp.append(f[int(prompt[pos + 1])] - (m + np.log(np.exp(f - m).sum())))
        bar.append(2 * LOGIT_TOL * np.abs(f).max())
    _assert_scores(got, np.array(lp), np.array(bar), "score vs forward")
    gm.close()


def test_score_bad_args():
    cfg, gm, om, prompt = _pair("tiny", L.Q4, L.BF16, 8)
    t = np.array([1, 2, cfg["vocab"]], dtype=np.int32)
    out = np.zeros(4, dtype=np.float32)
    p, o = t.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert gm.host.kfh_score(gm.h, p, 3, 0, o, None) == -20                      # id outside the table
    assert gm.host.kfh_score(gm.h, p, 2, cfg["max_seq"] - 1, o, None) == -20     # runs past the context
    assert gm.host.kfh_score(gm.h, p, 1, 0, o, None) == -20                      # n < 2: no pair to score
    assert gm.host.kfh_score(gm.h, p, 0, 0, o, None) == -20
    assert gm.host.kfh_score(gm.h, p, 2, 0, o, None) == 0
    gm.close()


# ---------------------------------------------------------------------------------------------------------------- full size
def _full_size(n_tok):
    cfg = dict(synth.CONFIGS["qwen3-0.6b"])
    m = synth.build_on_gpu(cfg, seed=1234, layer_type=L.Q4, head_type=L.BF16)
    om = O.from_device_model(m)
    prompt = np.random.default_rng(17).integers(0, cfg["vocab"], size=n_tok).astype(np.int32)
    t0 = time.time()
    got = m.score(prompt).astype(np.float64)
    t1 = time.time()
    want, bar = _oracle_scores(om, prompt)
    print("full size, %d tokens: score %.2f s (first call, allocations included), oracle %.1f s" % (n_tok, t1 - t0, time.time() - t1))
    _assert_scores(got, want, bar, "qwen3-0.6b, %d tokens" % n_tok)
    _assert_ppl(m, prompt, want, bar, "qwen3-0.6b")
    om.close()
    m.close()


def test_full_size_score_vs_oracle():
    """the Qwen3-0.6B shape with its real 151 936-row head (1187 vocabulary tiles, the last row block ragged), 256 tokens, every token against the oracle"""
    _full_size(256)


@pytest.mark.slow
def test_full_size_score_vs_oracle_whole_context():
    _full_size(2047)
