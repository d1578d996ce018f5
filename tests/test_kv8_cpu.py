"""The int8 KV cache without a GPU (include/kf_abi.h "int8 KV cache", restated by tests/kv8_restate.py): the row quantiser on its edge cases, the order freedom the
definition claims for its fp64 sums -- checked where the claim is made -- the accuracy of the restated attention against the oracle's canonical attention on the
unquantised rows, and the plan of kf_attn_block_kv8 (the ATTN_DECODE_KV8 entry of kf::attn_plan through kfdbg_kv8_plan) with its refusals."""
import ctypes as C

import numpy as np
import pytest

import exact_inputs as E
import kv8_restate as R
from a8_restate import quant_rows
from attn_plan_mirror import kv8_plan
from koifish_amd import lib as L
from oracle import oracle as O

SHAPES = [(4, 2, 64), (16, 8, 128)]
KEYS = [300, 2047]
# the largest |restatement - O.attn_decode(mode=ATTN_CANON) on the unquantised bf16 rows| over SHAPES x KEYS x SEEDS below, in units of max |v|, measured on the CPU by
# test_accuracy_against_the_unquantised_attention itself (it prints every figure): 0.00184 (16 / 8 heads x 128 at 300 keys, seed 1).  The assertion is twice that: the seeds
# are a sample, not a worst case.
MEASURED_MAX_ERR = 0.00184
SEEDS = [0, 1, 2]


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


def normal_case(nh, nkv, hd, T, seed):
    rng = np.random.default_rng(seed)
    draw = lambda *s: R.to_bf(rng.standard_normal(s).astype(np.float32))
    return draw(nh * hd), draw(T, nkv * hd), draw(T, nkv * hd)


_CASES = {}


def quantised_case(nh, nkv, hd, T, seed):
    """(q, k, v bf16, the rows in a Cache8, the one-pass output): computed once, shared"""
    key = (nh, nkv, hd, T, seed)
    if key not in _CASES:
        q, k, v = normal_case(nh, nkv, hd, T, seed)
        c = R.Cache8(T, nkv, hd)
        c.put(0, k, v)
        _CASES[key] = (q, k, v, c, c.attend(q, T - 1, nh))
    return _CASES[key]


def test_symbols_exist(hip):
    for f in ("kf_attn_block_kv8", "kf_attn_block_kv8_status", "kf_kv8_quant_rows", "kf_kv8_dequant_rows", "kfdbg_kv8_plan"):
        assert hasattr(hip, f), f
    host = L.load()[1]
    for f in ("kfh_set_kv_int8", "kfh_kv_int8", "kfh_kv8_codes", "kfh_kv8_steps"):
        assert hasattr(host, f), f


@pytest.mark.parametrize("hd", [64, 128])
def test_quantiser_edge_cases(hd):
    """quant_heads is quant_rows on hd-wide rows: a zero head, a head whose largest element is negative, exact .5 ties, amax landing on +-127"""
    rng = np.random.default_rng(hd)
    x = rng.standard_normal((5, 2 * hd)).astype(np.float32)
    x[0, :hd] = 0.0                                   # a zero head beside a live one
    x[1, :hd] = -np.abs(x[1, :hd])                     # every element negative: the ABSOLUTE maximum
    x[1, 3] = -7.0
    ties = np.arange(hd, dtype=np.float32) - hd // 2 + 0.5   # k + 0.5 with amax = 127: step 1, every element an exact tie
    ties[0] = 127.0
    x[2, :hd], x[2, hd:] = ties, -ties
    x[3, :hd] = np.clip(np.round(x[3, :hd] * 40), -126, 126)
    x[3, 5], x[3, 6] = 127.0, -127.0                   # amax = 127 on both signs: codes = the values
    u = R.to_bf(x)
    q, s = R.quant_heads(u, hd)
    qr, sr = quant_rows(u.reshape(-1, hd))
    assert np.array_equal(q.reshape(-1, hd), qr) and np.array_equal(s.reshape(-1), sr)
    assert s[0, 0] == 0 and not q[0, :hd].any() and s[0, 1] > 0
    assert s[1, 0] == np.float32(7.0) / np.float32(127.0) and q[1, 3] == -127 and q[1, :hd].max() <= 0
    f = R.bf(u)
    assert s[2, 0] == 1.0 and q[2, 0] == 127
    t = f[2, 1:hd]                                      # exact in bf16 (|t| < 64, one fractional bit): halves go away from zero
    assert np.array_equal(q[2, 1:hd], (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int8)) and np.array_equal(q[2, hd + 1:], -q[2, 1:hd])
    assert s[3, 0] == 1.0 and np.array_equal(q[3, :hd].astype(np.float32), f[3, :hd]) and q[3, 5] == 127 and q[3, 6] == -127
    # the dequantised row: one fp32 multiply, one rounding
    d = R.dequant_heads(q, s, hd)
    assert np.array_equal(R.bf(d[3, :hd]), f[3, :hd]) and not d[0, :hd].any()   # by value: a code 0 gives +0 where the row held -0
    assert np.array_equal(d, R.to_bf((q.astype(np.float32).reshape(5, 2, hd) * s[:, :, None]).astype(np.float32).reshape(5, -1)))


def test_exp2_parts_fma_is_exact():
    """the emulated fma against exact rational arithmetic on a sample, and kf_exp2_parts' parts against 2^y"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    c[::3] *= np.float32(2.0 ** -20)
    got = R.fma32(a, b, c)
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), i
    y = np.linspace(-30, 5, 4001).astype(np.float32)
    f, n = R.exp2_parts(y)
    assert np.array_equal(n, np.rint(y)) and np.abs(np.ldexp(f.astype(np.float64), n.astype(np.int64)) / np.exp2(y.astype(np.float64)) - 1).max() < 2e-7


@pytest.mark.parametrize("T", KEYS)
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_order_freedom(nh, nkv, hd, T):
    """one pass, slices of 61 and of 64 keys merged with canon_shift, the keys in reverse: equal bits -- every term of the fp64 sums is exact (24 + 7 bits), m is free"""
    q, k, v, c, one = quantised_case(nh, nkv, hd, T, 0)
    for kw in (dict(slice_keys=61), dict(slice_keys=64), dict(reverse=True)):
        got = R.attn_decode_kv8(q, c.k8, c.ks, c.v8, c.vs, T - 1, nh, nkv, hd, **kw)
        assert np.array_equal(got, one), (kw, int((got != one).sum()))


def test_accuracy_against_the_unquantised_attention():
    worst = 0.0
    for nh, nkv, hd in SHAPES:
        for T in KEYS:
            for seed in SEEDS:
                q, k, v, c, one = quantised_case(nh, nkv, hd, T, seed)
                ref = O.attn_decode(q, k, v, T - 1, nh, nkv, hd, mode=O.ATTN_CANON)
                err = float(np.abs(R.bf(one) - R.bf(ref)).max() / np.abs(R.bf(v)).max())
                print("%d / %d heads x %d, %d keys, seed %d: max error %.5f of max |v|" % (nh, nkv, hd, T, seed, err))
                worst = max(worst, err)
    print("largest: %.5f (recorded: %.5f)" % (worst, MEASURED_MAX_ERR))
    assert worst <= 2 * MEASURED_MAX_ERR


def test_plan_is_pinned(hip):
    """the slices are attn_slices' (one slice up to 192 keys, then ~64 keys per slice, at most 32), always 4 waves, at most two query heads per workgroup; the LDS holds the
    waves' fp64 partials, the prepared q heads and new key, their codes with the new rows' codes, the steps and the flag; the scratch is kf_attn_block's"""
    hip.kf_attn_scratch_bytes.restype = C.c_size_t
    for nh, nkv in E.HEADS + [(16, 8), (8, 8)]:
        for hd in E.HEAD_DIMS:
            for pos, nsp, chunk in ((0, 1, 1), (1, 1, 2), (63, 1, 64), (64, 1, 65), (191, 1, 192), (192, 4, 49), (193, 4, 49), (300, 5, 61), (2047, 32, 64), (32767, 32, 1024)):
                p = kv8_plan(hip, nh, nkv, hd, pos)
                gq = nh // nkv
                split = gq // 2 if gq > 2 else 1
                nsp_c = min(nsp, max(1, 512 // nkv)) if nsp > 1 else 1
                assert p.status == 0 and p.route == 5 and p.canon == 1 and p.nw == 4 and p.threads == 256 and p.hd == hd
                assert (p.gq, p.gq_split, p.n_splits, p.chunk) == (gq // split, split, nsp_c, chunk), (nh, nkv, hd, pos)
                assert list(p.grid) == [nsp_c, nkv * split, 1] and p.cnt_stride == min(64, 4096 // (nkv * split))
                g = p.gq
                assert p.lds == 8 * 4 * g * (hd + 2) + 2 * (g * hd + hd) + (g * hd + 2 * hd) + 4 * (g + 2) + 16
                assert p.scratch == hip.kf_attn_scratch_bytes(nh, hd)
    assert kv8_plan(hip, 16, 8, 128, 2047).lds == 9632 and kv8_plan(hip, 2, 2, 64, 0).lds == 2588
    # refusals: the entry's own answers, and the status function's
    for nh, nkv, hd in ((10, 2, 128), (16, 8, 96), (5, 2, 64), (4, 0, 64)):
        assert kv8_plan(hip, nh, nkv, hd, 10).status == -20, (nh, nkv, hd)          # KF_INVALID_ARGS
        assert hip.kf_attn_block_kv8_status(nh, nkv, hd) == -20
    assert kv8_plan(hip, 4, 2, 64, -1).status == -20
    assert kv8_plan(hip, 4, 2, 64, 10, kv_stride=136).status != 0 and kv8_plan(hip, 4, 2, 64, 10, kv_stride=144).status == 0
    for nh, nkv in E.HEADS:
        for hd in E.HEAD_DIMS:
            assert hip.kf_attn_block_kv8_status(nh, nkv, hd) == 0
    # the plans of the existing entries are untouched: tests/test_attn_plan_cpu.py and tests/test_exact_inputs_cpu.py pin them
