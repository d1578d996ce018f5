"""The numpy restatement of the int8 KV cache's PROMPT form (include/kf_abi.h "int8 KV cache, the prompt form"; kf_attn_prefill_kv8), stated once for
tests/test_kv8_prefill_cpu.py, tests/test_gpu_kv8_prefill.py and tests/test_gpu_kv8_prefill_model.py.  Up to the weight it is tests/kv8_restate.py's decode definition
(imported, not edited): batch_terms is key_terms on every row of a batch at once.  The tail -- gb = bf16(g), fp32 sums in an order that is the hardware's -- is stated
as its exact value (fp64 sums of exact products) together with the DERIVED bound `tol` that any fp32 summation order stays inside; nothing here calls the library."""
import numpy as np

import kv8_restate as R
from kv8_restate import F32, F64, bf, to_bf

U = 2.0 ** -23          # the unit roundoff the bound assumes: covers an fp32 accumulator that truncates as well as one that rounds to nearest
BF16_STORE = 2.0 ** -8  # the unit roundoff of bf16 (8 significant bits): |bf16_rn(x) - x| <= 2^-8 |x|
DIV = 2.0 ** -24        # the one correctly rounded fp32 division


def batch_terms(q8, sq, k8h, ksh, vsh, hd):
    """rows [n, hd] (codes) / [n] (steps) of ONE query head against keys [T]: (s, f, n, g) fp32 [n, T].  Row by row this is kv8_restate.key_terms: the exact integer
    dot, three separate fp32 multiplies, the bf16 score, kf_exp2_parts, g = f * VS.  Causality is the caller's: every (row, key) pair is evaluated."""
    I = np.asarray(q8).astype(np.int64) @ np.asarray(k8h).astype(np.int64).T
    assert np.abs(I).max(initial=0) < 2 ** 24
    with np.errstate(all="ignore"):   # rows past a position may hold anything (the causal test fills them with huge steps); they are masked by the caller
        c = (np.asarray(sq, dtype=F32)[:, None] * np.asarray(ksh, dtype=F32)[None, :]).astype(F32)
        d = (I.astype(F32) * c).astype(F32)
        s = bf(to_bf((d * R.rden(hd)).astype(F32)))
        f, n = R.exp2_parts((s * R.LOG2E).astype(F32))
        g = (f * np.asarray(vsh, dtype=F32)[None, :]).astype(F32)
    return s, f, n, g


def gb_of(g):
    """the P.V operand: bf16_rn(g) as fp32"""
    return bf(to_bf(np.asarray(g, dtype=F32)))


def exact_sums(f, n, g, v8h, valid):
    """rows [R, T] of one head, v8h int8 [T, hd], valid bool [R, T] -> the exact sums against each row's own maximum exponent M:
    O [R, hd] = sum_t gb_t v8[t] 2^(n_t - M), L [R] = sum_t f_t 2^(n_t - M), A [R, hd] = sum_t |gb_t v8[t]| 2^(n_t - M), in fp64 (every term is exact)"""
    with np.errstate(all="ignore"):
        M = np.where(valid, n, -np.inf).max(axis=1)
        e = R.shift(np.where(valid, n - M[:, None], 0.0))
        w = np.where(valid, np.ldexp(gb_of(g).astype(F64), e), 0.0)
        p = np.where(valid, np.ldexp(f.astype(F64), e), 0.0)
    v = np.asarray(v8h).astype(F64)
    return w @ v, p.sum(axis=1), np.abs(w) @ np.abs(v), M


def bound(O, L, A, N):
    """the derived bound on |out - O / L| for N keys (module docstring of tests/test_kv8_prefill_cpu.py): the bf16 store, the division, any-order fp32 sums"""
    N = np.asarray(N, dtype=F64).reshape(-1, 1)
    L = L.reshape(-1, 1)
    return (BF16_STORE + DIV) * np.abs(O / L) + 2.0 * N * U * (A + np.abs(O)) / L


def one_key(f0, g0, v8row):
    """a row with ONE key: nothing is summed -- bf16_rn(fl32(gb_0 * v8[0][d] / f_0)) exactly (uint16 [hd])"""
    o = (gb_of(g0) * np.asarray(v8row).astype(F32)).astype(F32)
    return to_bf((o / F32(f0)).astype(F32))


def attn_prefill_kv8(q_u16, k8, ks, v8, vs, pos0, n_head, n_kv, hd):
    """the prompt form on rows q_u16 [n, n_head * hd] (prepared bf16 queries) at positions pos0 .. pos0 + n - 1; k8 / v8 int8 [>= pos0 + n, >= n_kv * hd], ks / vs fp32
    [.., n_kv].  -> (ref fp64 [n, n_head * hd] = O / L, tol fp64 of the same shape, exact uint16 or None: row 0's bits when pos0 == 0)"""
    q_u16 = np.atleast_2d(np.asarray(q_u16, dtype=np.uint16))
    n, T, gq = q_u16.shape[0], pos0 + q_u16.shape[0], n_head // n_kv
    q8, sq = R.quant_heads(q_u16[:, :n_head * hd], hd)
    pos = pos0 + np.arange(n)
    valid = np.arange(T)[None, :] <= pos[:, None]
    ref, tol = np.zeros((n, n_head * hd)), np.zeros((n, n_head * hd))
    exact = np.zeros(n_head * hd, dtype=np.uint16) if pos0 == 0 else None
    for h in range(n_head):
        kvh = h // gq
        cols, hs = slice(kvh * hd, (kvh + 1) * hd), slice(h * hd, (h + 1) * hd)
        _, f, nn, g = batch_terms(q8[:, hs], sq[:, h], np.asarray(k8)[:T, cols], np.asarray(ks)[:T, kvh], np.asarray(vs)[:T, kvh], hd)
        O, L, A, _ = exact_sums(f, nn, g, np.asarray(v8)[:T, cols], valid)
        ref[:, hs], tol[:, hs] = O / L[:, None], bound(O, L, A, pos + 1)
        if exact is not None:
            exact[hs] = one_key(f[0, 0], g[0, 0], np.asarray(v8)[0, cols])
    return ref, tol, exact


def tiled_terms(f, n, g, tile):
    """ONE row's keys walked in tiles of `tile` with a running integer maximum m, in fp32 as the kernel holds them: what every key's (gb 2^(n - m), f 2^(n - m)) has
    become at the end of the walk -- scaled against the m of its tile, then multiplied by 2^(m_old - m_new) at every later move -- and the final m"""
    gb = gb_of(g)
    w, p, m = np.zeros_like(gb), np.zeros_like(gb), F32(-np.inf)
    for a in range(0, len(f), tile):
        sl = slice(a, a + tile)
        mn = max(m, n[sl].max())
        if mn > m and np.isfinite(m):
            sc = np.ldexp(F32(1.0), int(m - mn))
            w[:a], p[:a] = (w[:a] * sc).astype(F32), (p[:a] * sc).astype(F32)
        m = mn
        e = (n[sl] - m).astype(np.int64)
        w[sl], p[sl] = np.ldexp(gb[sl], e).astype(F32), np.ldexp(f[sl], e).astype(F32)
    return w, p, m


def eval_fp32(f, n, g, v8h, tile, order=None):
    """ONE row evaluated the way a kernel may: keys in `order` (default ascending), tiles of `tile` keys, running m, fp32 accumulators added tile by tile (numpy's own
    summation inside a tile), the fp32 division, the bf16 store -> uint16 [hd].  One of the many summation orders the bound must cover."""
    idx = np.arange(len(f)) if order is None else np.asarray(order)
    f, n, gb, v = f[idx], n[idx], gb_of(g)[idx], np.asarray(v8h)[idx].astype(F32)
    O, L, m = np.zeros(v.shape[1], dtype=F32), F32(0.0), F32(-np.inf)
    for a in range(0, len(f), tile):
        sl = slice(a, a + tile)
        mn = max(m, n[sl].max())
        if mn > m:
            sc = np.ldexp(F32(1.0), int(m - mn)) if np.isfinite(m) else F32(0.0)
            O, L = (O * sc).astype(F32), F32(L * sc)
        m = mn
        e = (n[sl] - m).astype(np.int64)
        wt, pt = np.ldexp(gb[sl], e).astype(F32), np.ldexp(f[sl], e).astype(F32)
        O = (O + (wt[:, None] * v[sl]).astype(F32).sum(axis=0, dtype=F32)).astype(F32)
        L = F32(L + pt.sum(dtype=F32))
    return to_bf((O / L).astype(F32))


class BatchAttention:
    """the batch-form attention of a layer on a kv8_restate.Cache8: the rows are put (quantised) first, then every row attends keys 0 .. its position -> the rounded
    reference bf16_rn(O / L) uint16 [n, n_head * hd] (what a model-level comparison against a tolerance uses)"""

    def __init__(self, n_head, n_kv, hd):
        self.n_head, self.n_kv, self.hd = n_head, n_kv, hd

    def __call__(self, cache, q_u16, pos0):
        ref, _, _ = attn_prefill_kv8(q_u16, cache.k8, cache.ks, cache.v8, cache.vs, pos0, self.n_head, self.n_kv, self.hd)
        return to_bf(ref.astype(F32))
