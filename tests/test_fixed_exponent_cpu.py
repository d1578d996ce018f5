"""The fixed reference exponent of the engine's canonical attention, without a GPU (koifish_amd/csrc/kf_attn_common.h, KF_CANON_FIX_LIM = 448).

The oracle's definition (kfo_attn_decode mode 2) scales every softmax weight by 2^-m, m the largest exponent of the sequence.  The persistent engine sums the same
weights against m = 0: p = ldexp(f, n), no maximum at any level.  tests/fixed_exponent_ref.c restates that, with the sums dealt as the engine deals them (64-key slices,
8 waves x 4 interleaved key groups, pairwise group adds, waves in order, slices in four quarters and two quad adds), and this file holds it against the oracle bit for
bit: 16 / 8 heads of 128, positions 0, 5, 63, 64, 200, 1000, 2047, values scaled x1 and x30, queries scaled until the largest |n| of the sequence stands in
[300, 440] -- and once beyond the limit, where the guard must be set (and the outputs are nobody's business).
Observed with these rows: queries x52 / x60 / x66 reach |n| = 346 / 398 / 439 at position 2047 (303 / 349 / 384 at 1000), x100 reaches 664 (and 505 from position 63 on:
the guard is set there; at positions 0 and 5 it reaches 381, the guard stays clear and the outputs are the oracle's)."""
import ctypes as C

import numpy as np
import pytest

from fixed_exponent import LIM, build_ref, load_ref
from oracle import oracle as O

N_HEAD, N_KV, HD, SEQ = 16, 8, 128, 2048
POSITIONS = (0, 5, 63, 64, 200, 1000, 2047)


@pytest.fixture(scope="module")
def fixed(tmp_path_factory):
    lib = load_ref(build_ref(tmp_path_factory.mktemp("fixed_exponent")))

    def run(q, kc, vc, pos):
        out = np.zeros(N_HEAD * HD, dtype=np.uint16)
        amax = C.c_float(0)
        g = lib.kfx_attn_decode_fixed(q.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data, pos, N_HEAD, N_KV, HD, N_KV * HD, C.byref(amax))
        assert g in (0, 1)
        return out, bool(g), float(amax.value)
    return run


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(20)
    q = rng.standard_normal(N_HEAD * HD).astype(np.float32)
    k = O.f32_to_bf16(rng.standard_normal((SEQ, N_KV * HD)).astype(np.float32))
    v = rng.standard_normal((SEQ, N_KV * HD)).astype(np.float32)
    return q, k, {1: O.f32_to_bf16(v), 30: O.f32_to_bf16(v * 30.0)}


def _compare(fixed, rows, q_scale, v_scale):
    """per position: (mismatching output elements against the oracle, guard, largest |n|)"""
    q0, k, vs = rows
    q = O.f32_to_bf16(q0 * np.float32(q_scale))
    res = []
    for pos in POSITIONS:
        ref = O.attn_decode(q, k, vs[v_scale], pos, N_HEAD, N_KV, HD, mode=O.ATTN_CANON)
        got, guard, amax = fixed(q, k, vs[v_scale], pos)
        assert guard == (not amax <= LIM), "the guard is the test !(|n| <= %g) on every valid key" % LIM
        res.append((int((got != ref).sum()), guard, amax))
    return res


@pytest.mark.parametrize("v_scale", [1, 30])
@pytest.mark.parametrize("q_scale", [1, 8, 24])
def test_fixed_exponent_equals_the_oracle_at_ordinary_scores(fixed, rows, q_scale, v_scale):
    res = _compare(fixed, rows, q_scale, v_scale)
    assert [r[0] for r in res] == [0] * len(POSITIONS), res
    assert not any(r[1] for r in res)


@pytest.mark.parametrize("v_scale", [1, 30])
@pytest.mark.parametrize("q_scale", [52, 60, 66])
def test_fixed_exponent_equals_the_oracle_with_exponents_in_300_to_440(fixed, rows, q_scale, v_scale):
    res = _compare(fixed, rows, q_scale, v_scale)
    print("q x%d v x%d: largest |n| per position %s" % (q_scale, v_scale, [r[2] for r in res]))
    assert 300.0 <= max(r[2] for r in res) <= 440.0, "the case does not reach the range it is about: %s" % (res,)
    assert [r[0] for r in res] == [0] * len(POSITIONS), res
    assert not any(r[1] for r in res)


@pytest.mark.parametrize("v_scale", [1, 30])
def test_guard_is_set_beyond_the_limit(fixed, rows, v_scale):
    res = _compare(fixed, rows, 100, v_scale)
    print("q x100 v x%d: largest |n| per position %s" % (v_scale, [r[2] for r in res]))
    assert res[-1][1] and res[-1][2] > LIM, "position 2047 must trip the guard: %s" % (res[-1],)
    for mism, guard, amax in res:   # wherever the guard stays clear the outputs are still the oracle's
        assert guard or mism == 0, (mism, guard, amax)
