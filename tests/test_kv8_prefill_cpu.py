"""The int8 KV cache's prompt form without a GPU (include/kf_abi.h "int8 KV cache, the prompt form"; tests/kv8_prefill_restate.py): what the definition claims as exact
is checked as exact, and the bound the GPU test holds kf_attn_prefill_kv8 to is derived here and shown to be neither violated by an honest fp32 evaluation nor loose
enough to hide a wrong kernel.

THE BOUND.  For one output element let w_t = gb_t 2^(n_t - M) and x_t = w_t v8[t][d] (exact in fp32: 8 + 7 significant bits), O = sum_t x_t, L = sum_t p_t with
p_t = f_t 2^(n_t - M) > 0, A = sum_t |x_t|, N = p + 1 terms.  A kernel adds the x_t (and the p_t) in fp32 in SOME order; every addition commits a relative error of at
most u, and a term passes through at most N - 1 additions (a rescale by a power of two commits none).  To first order in u
    |O~ - O| <= (N - 1) u sum_t |x_t| <= N u A          |L~ - L| <= N u L            (all p_t > 0)
for ANY order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: the bound holds for every summation tree).  u = 2^-23 rather than 2^-24, so that an
accumulator that truncates is covered as well as one that rounds to nearest.  Then
    |O~ / L~ - O / L| <= |O~ - O| / L~ + |O| |1 / L~ - 1 / L| <= N u A / L + N u |O| / L   to first order;
the factor 2 on this term absorbs the second-order remainder (N u <= 2^-14 for every N <= 512 a test uses, so the neglected terms are below 2^-13 of the term itself)
and leaves the bound a little slack instead of none.  The quotient is one correctly rounded fp32 division (2^-24 |O / L|) and the result one bf16 store: bf16 has 8
significant bits, so round-to-nearest commits at most 2^-8 |O / L| -- and comes close to that for a value just above a power of two.  Altogether
    tol = (2^-8 + 2^-24) |O / L| + 2 N u (A + |O|) / L.
None of the constants comes from a run.

AGAINST THE DECODE FORM at the same position the only differences are gb = bf16_rn(g) in place of g (|gb - g| <= 2^-8 |g|, so the exact quotients differ by at most
2^-8 A / L to first order) and the two stores: decode's fl32 + bf16 store of its exact quotient, and this form's bf16 store -- 2^-8 of each value."""
import numpy as np
import pytest

import attn_plan_mirror as APM
import exact_inputs as E
import kv8_prefill_restate as P
import kv8_restate as R

F32, F64 = np.float32, np.float64
KEYS = [1, 65, 300]
SEEDS = [0, 1, 2]
_CASES = {}


def case(nh, nkv, hd, T, seed):
    """a cache of T quantised rows and one prepared query row at position T - 1, with every head's terms: drawn once, shared, never changed"""
    key = (nh, nkv, hd, T, seed)
    if key not in _CASES:
        rng = np.random.default_rng(seed * 100003 + nh * 1009 + nkv * 101 + hd + T)
        kvd = nkv * hd
        c = R.Cache8(T, nkv, hd)
        c.put(0, R.to_bf((rng.standard_normal((T, kvd)) * rng.uniform(0.25, 4.0, (T, 1))).astype(F32)), R.to_bf(rng.standard_normal((T, kvd)).astype(F32)))
        q = R.to_bf((0.5 * rng.standard_normal(nh * hd)).astype(F32))
        q8, sq = R.quant_heads(q, hd)
        heads = []
        for h in range(nh):
            kvh = h // (nh // nkv)
            cols, hs = slice(kvh * hd, (kvh + 1) * hd), slice(h * hd, (h + 1) * hd)
            s, f, n, g = P.batch_terms(q8[None, hs], sq[None, h], c.k8[:, cols], c.ks[:, kvh], c.vs[:, kvh], hd)
            heads.append((kvh, cols, hs, s[0], f[0], n[0], g[0]))
        _CASES[key] = (c, q, q8, sq, heads)
    return _CASES[key]


SHAPES = [(nh, nkv, hd) for nh, nkv in E.HEADS for hd in E.HEAD_DIMS]
bits = lambda a: np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("T", KEYS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_scores_and_weights_are_the_decode_definitions(nh, nkv, hd, T):
    for seed in SEEDS:
        c, q, q8, sq, heads = case(nh, nkv, hd, T, seed)
        for kvh, cols, hs, s, f, n, g in heads:
            fd, nd, gd = R.key_terms(q8[hs], sq[hs.start // hd], c.k8[:, cols], c.ks[:, kvh], c.vs[:, kvh], hd)
            assert np.array_equal(bits(f), bits(fd)) and np.array_equal(bits(n), bits(nd)) and np.array_equal(bits(g), bits(gd))
            # s itself: a bf16 value whose exp2 parts are (f, n)
            assert np.array_equal(bits(s), bits(R.bf(R.to_bf(s))))
            f2, n2 = R.exp2_parts((s * R.LOG2E).astype(F32))
            assert np.array_equal(bits(f2), bits(f)) and np.array_equal(bits(n2), bits(n))


@pytest.mark.parametrize("T", KEYS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_the_tiled_walk_scales_exactly(nh, nkv, hd, T):
    """64-key tiles with a running m against the one-pass evaluation: the same bits once both stand against the final maximum -- moving m is a power of two"""
    for seed in SEEDS:
        heads = case(nh, nkv, hd, T, seed)[4]
        for _, _, _, s, f, n, g in heads:
            w, p, m = P.tiled_terms(f, n, g, 64)
            e = (n - n.max()).astype(np.int64)
            assert m == n.max()
            assert np.array_equal(bits(w), bits(np.ldexp(P.gb_of(g), e))) and np.array_equal(bits(p), bits(np.ldexp(f, e)))
            assert e.min() > -100   # no weight of these inputs comes near the fp32 underflow the definition sets aside


def head_bound(c, head, T):
    kvh, cols, hs, s, f, n, g = head
    O, L, A, _ = P.exact_sums(f[None], n[None], g[None], c.v8[:, cols], np.ones((1, T), dtype=bool))
    return (O / L[:, None])[0], P.bound(O, L, A, [T])[0]


@pytest.mark.parametrize("T", KEYS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_fp32_summation_stays_inside_the_bound(nh, nkv, hd, T):
    for seed in SEEDS:
        c, q, q8, sq, heads = case(nh, nkv, hd, T, seed)
        rng = np.random.default_rng(seed + 17)
        orders = [None] + [rng.permutation(T) for _ in range(3)]
        for head in heads:
            kvh, cols, hs, s, f, n, g = head
            ref, tol = head_bound(c, head, T)
            for order in orders:
                for tile in (16, 64, 61):
                    got = R.bf(P.eval_fp32(f, n, g, c.v8[:, cols], tile, order)).astype(F64)
                    assert (np.abs(got - ref) <= tol).all(), "tile %d: %g over the bound" % (tile, float((np.abs(got - ref) - tol).max()))
            if T == 1:   # one key: nothing is summed, the bits are stated
                assert np.array_equal(P.eval_fp32(f, n, g, c.v8[:, cols], 64), P.one_key(f[0], g[0], c.v8[0, cols]))


@pytest.mark.parametrize("T", KEYS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_the_bound_catches_a_wrong_kernel(nh, nkv, hd, T):
    """one key dropped (the one with the largest weight: the key a broken causal bound or tile tail would lose), then g left without its VS (f used for g)"""
    for seed in SEEDS:
        c, q, q8, sq, heads = case(nh, nkv, hd, T, seed)
        for head in heads:
            kvh, cols, hs, s, f, n, g = head
            ref, tol = head_bound(c, head, T)
            v = c.v8[:, cols]
            if T > 1:
                keep = np.arange(T) != int(np.argmax(np.ldexp(f.astype(F64), (n - n.max()).astype(np.int64))))
                got = R.bf(P.eval_fp32(f[keep], n[keep], g[keep], v[keep], 64)).astype(F64)
                assert (np.abs(got - ref) > tol).any(), "a dropped key passed the bound"
            got = R.bf(P.eval_fp32(f, n, f, v, 64)).astype(F64)
            assert (np.abs(got - ref) > tol).any(), "g without VS passed the bound"


@pytest.mark.parametrize("T", KEYS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_against_the_decode_form(nh, nkv, hd, T):
    """the decode definition at the same position differs by the gb rounding and the two stores only"""
    for seed in SEEDS:
        c, q, q8, sq, heads = case(nh, nkv, hd, T, seed)
        dec = R.bf(R.attn_decode_kv8(q, c.k8, c.ks, c.v8, c.vs, T - 1, nh, nkv, hd)).astype(F64)
        ref, tol, exact = P.attn_prefill_kv8(q[None], c.k8, c.ks, c.v8, c.vs, T - 1, nh, nkv, hd)
        mine = R.bf(R.to_bf(ref[0].astype(F32))).astype(F64)
        for head in heads:
            kvh, cols, hs, s, f, n, g = head
            O, L, A, _ = P.exact_sums(f[None], n[None], g[None], c.v8[:, cols], np.ones((1, T), dtype=bool))
            lim = 2.0 ** -8 * (A / L[:, None])[0] + 2.0 ** -8 * (np.abs(dec[hs]) + np.abs(mine[hs]))
            assert (np.abs(dec[hs] - mine[hs]) <= lim).all()
        if T == 1:
            assert np.array_equal(exact, R.to_bf(ref[0].astype(F32)))   # one key: the stated bits are the rounded exact quotient


def test_plan_and_status():
    """the ATTN_PROMPT_KV8 entry of kf::attn_plan: one form for every n_tok, 64 / gq tokens per workgroup, no scratch; the refusals and kf_attn_prefill_kv8_status"""
    from koifish_amd import lib as L
    hip, _ = L.load()
    TILE_KV8 = APM.TILE_KV8

    def plan(nh, nkv, hd, pos0, n, al=3, q_stride=None, kv_stride=None):
        return APM.plan(hip, APM.PROMPT_KV8, nh, nkv, hd, pos0, n, al=al, q_stride=q_stride, kv_stride=kv_stride)

    for nh, nkv in E.HEADS:
        for hd in E.HEAD_DIMS:
            gq = nh // nkv
            for n in (1, 8, 33, 64, 65, 2047):
                for pos0 in (0, 100, 32768):
                    p = plan(nh, nkv, hd, pos0, n)
                    tq = 64 // gq
                    assert (p.status, p.route, p.gq, p.hd, p.kt, p.threads, p.scratch) == (0, TILE_KV8, gq, hd, 64, 256, 0)
                    assert list(p.grid) == [(n + tq - 1) // tq, nkv, 1]
                    assert p.lds == 64 * (hd + 16) + 2 * 64 * (hd + 16) + 512 + 64 * hd + 256 and p.lds <= 64 * 1024
            assert hip.kf_attn_prefill_kv8_status(nh, nkv, hd, 5) == 0
    INVALID, UNALIGN = -20, plan(4, 2, 64, 0, 4, kv_stride=136).status
    assert UNALIGN != 0 and UNALIGN != INVALID
    for bad in (plan(10, 2, 64, 0, 4), plan(4, 2, 96, 0, 4), plan(4, 3, 64, 0, 4), plan(4, 2, 64, -1, 4), plan(4, 2, 64, 0, 0)):
        assert bad.status == INVALID and bad.route == TILE_KV8
    for bad in (plan(4, 2, 64, 0, 4, al=1), plan(4, 2, 64, 0, 4, al=2), plan(4, 2, 64, 0, 4, q_stride=260)):
        assert bad.status == UNALIGN
    assert hip.kf_attn_prefill_kv8_status(10, 2, 64, 4) == INVALID and hip.kf_attn_prefill_kv8_status(4, 2, 96, 4) == INVALID
    assert hip.kf_attn_prefill_kv8_status(4, 2, 64, 0) == INVALID
