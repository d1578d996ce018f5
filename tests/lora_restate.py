"""The yardstick of the adapter tests (tests/test_lora_cpu.py, tests/test_gpu_lora.py): kf_lora_forward and kf_lora_backward restated in numpy -- fp64 sums, bf16
roundings (nearest even) exactly where include/kf_abi.h writes them, a switch that turns the roundings off -- the exact-arithmetic case generator built on
tests/exact_inputs.py, and the error bound of the random-operand tests.  s multiplies BOTH products of a direction: the effective weight is s^2 b a.

    forward    ax = bf16(s x a^T)               y = bf16(y0 + s ax b^T)
    backward   adelta = bf16(s dIn b)           delta = bf16(delta0 + s adelta a)
               gB = bf16(gB0 + s dIn^T ax)      gA = bf16(gA0 + s adelta^T inp)            g = [gA | gB]

The bound (bound() below), derived from the arithmetic and not from any device result.  The device sums in fp32 where this file sums in fp64, and rounds where this
file rounds.  A device output is compared with the restated value BEFORE its own final store (store=False: two values that differ by next to nothing can still round to
neighbouring bf16 values, a whole ulp apart; against the unrounded value the store costs half an ulp).  The intermediates ax and adelta are rounded in the restatement
wherever they feed a second product.  For an output  out = bf16(v),  v = prior + s sum_k u_k v_k  of T terms:
  (1) the final store: half a bf16 ulp of the value the device rounds (bf16 keeps 8 significant bits: an ulp is at most 2^-7 |v|, half of it 2^-8 |v|; the device's v
      is the restated one up to (2) and (3));
  (2) the fp32 accumulation: every one of the T partial sums (and the scaling and the prior's addition: T + 2 operations) is rounded to fp32, each by at most
      2^-24 of a magnitude that never exceeds A = |prior| + |s| sum_k |u_k v_k|; doubled for the MFMA's internal order: (T + 2) 2^-23 A;
  (3) where one factor is itself a rounded intermediate (ax in y and gB, adelta in delta and gA): the device's intermediate may differ from this file's by one bf16
      ulp of it where the two fp32 / fp64 sums straddle a rounding boundary -- 2^-7 |t_k| per element -- which the second product carries through as
      |s| sum_k 2^-7 |t_k| |w_k| <= 2^-7 (A - |prior|).
ax and adelta themselves have only (1) and (2).  Not a test module: no test_ functions."""
import ctypes as C

import numpy as np

from koifish_amd import lib as L
from oracle import oracle as O
from tests import exact_inputs as E

RANKS = (16, 32, 64)


def _rb(v, on=True):
    """fp64 -> the nearest bf16 value, as fp64 (through fp32: the device rounds an fp32 sum)"""
    return O.bf16_to_f32(O.f32_to_bf16(np.asarray(v, dtype=np.float32))).astype(np.float64) if on else np.asarray(v, dtype=np.float64)


def lora_forward(a, b, x, y0, s, rounding=True, store=True):
    """a [r, IC], b [OC, r], x [n, IC], y0 [n, OC] (fp64) -> (ax [n, r], y [n, OC]).  store=False: the two results before their own final rounding (the ax inside y
    is rounded all the same)"""
    ax_v = s * (x @ a.T)
    ax = _rb(ax_v, rounding)
    return (ax if store else ax_v), _rb(y0 + s * (ax @ b.T), rounding and store)


def lora_backward(a, b, dIn, inp, ax, delta0, g0, s, rounding=True, store=True):
    """dIn [n, OC], inp [n, IC], ax [n, r] (as the forward stored it), delta0 [n, IC], g0 [r IC + OC r] (fp64) -> (adelta [n, r], delta [n, IC], g = [gA | gB]).
    store=False: the results before their own final rounding (the adelta inside delta and gA is rounded all the same)"""
    r, IC = a.shape
    adelta_v = s * (dIn @ b)
    adelta = _rb(adelta_v, rounding)
    delta = _rb(delta0 + s * (adelta @ a), rounding and store)
    gA = _rb(g0[:r * IC].reshape(r, IC) + s * (adelta.T @ inp), rounding and store)
    gB = _rb(g0[r * IC:].reshape(b.shape) + s * (dIn.T @ ax), rounding and store)
    return (adelta if store else adelta_v), delta, np.concatenate([gA.reshape(-1), gB.reshape(-1)])


def magnitudes(a, b, x, y0, dIn, inp, ax, adelta, delta0, g0, s):
    """A of the docstring for each of the six outputs: |prior| + |s| sum |u v|, and the number of terms T"""
    r, IC = a.shape
    ab = np.abs
    s = abs(s)
    return dict(ax=(s * (ab(x) @ ab(a).T), IC), y=(ab(y0) + s * (ab(ax) @ ab(b).T), r), adelta=(s * (ab(dIn) @ ab(b)), b.shape[0]),
                delta=(ab(delta0) + s * (ab(adelta) @ ab(a)), r),
                gA=(ab(g0[:r * IC]).reshape(r, IC) + s * (ab(adelta).T @ ab(inp)), x.shape[0]), gB=(ab(g0[r * IC:]).reshape(b.shape) + s * (ab(dIn).T @ ab(ax)), x.shape[0]))


def bound(ref, A, T, prior=None, second=False):
    """|device - ref| allowed for one output (see the module docstring): ref the restated value before its final store, A and T from magnitudes(), prior the |prior|
    inside A, second: one factor is a rounded intermediate"""
    acc = (T + 2) * 2.0 ** -23 * A
    if second:
        acc = acc + 2.0 ** -7 * (A - (0.0 if prior is None else np.abs(prior)))
    return 2.0 ** -8 * (np.abs(ref) + acc) + acc


def lora_plan(hip, r, OC, IC, n):
    """kf::lora_plan through kfdbg_lora_plan"""
    p = L.LoraPlan()
    assert hip.kfdbg_lora_plan(r, OC, IC, n, C.byref(p)) == 0
    return p


def slab_seams(p, n, which="B"):
    """the token rows at which two slabs of gB's (or gA's) cut of n meet: slab s owns the 64-row k-steps [nkt s / S, nkt (s + 1) / S)"""
    S, nkt = (p.SB if which == "B" else p.SA), n // 64
    return [64 * (nkt * k // S) for k in range(1, S)]


def lora_exact_case(OC, IC, n, r, s, seed, block_at=None):
    """Operands and exact results of both entries for integers whose every partial sum is an fp32 value in every order.  x (= inp), a and deltaIn ternary at density
    sqrt(2 / K) of their long contraction (IC, IC, OC), b ternary at density 0.5 (0.25 at rank 64), integer priors within +-8 (multiples of s) for y, delta and g; s 1 or 2.
    block_at: instead, x and deltaIn are dense +-1 on the 128 token rows astride row block_at (exact_inputs.block_rows) and zero elsewhere, so that both gradients sum
    128 consecutive non-zero terms across that row; a and b then carry 8 non-zeros per long contraction on average.
    Asserted: all six results (ax, y, adelta, delta, gA, gB) are bf16 values, every sum of absolute terms is below 2^23."""
    assert s in (1, 2) and r in RANKS
    rng = np.random.default_rng(seed)
    if block_at is None:
        x, a, dIn = E.ternary(rng, (n, IC), np.sqrt(2.0 / IC)), E.ternary(rng, (r, IC), np.sqrt(2.0 / IC)), E.ternary(rng, (n, OC), np.sqrt(2.0 / OC))
        b = E.ternary(rng, (OC, r), 0.25 if r == 64 else 0.5)
    else:
        rows = E.block_rows(n, block_at)
        x, dIn = np.zeros((n, IC)), np.zeros((n, OC))
        x[rows], dIn[rows] = rng.choice([-1.0, 1.0], size=(len(rows), IC)), rng.choice([-1.0, 1.0], size=(len(rows), OC))
        a, b = E.ternary(rng, (r, IC), 8.0 / IC), E.ternary(rng, (OC, r), 8.0 / OC)
    fs = float(s)   # the priors are multiples of s within +-8: with s = 2 every result is even, and even integers are bf16 values up to 512
    y0, delta0, g0 = (fs * E.small_ints(rng, sh, 8 // s) for sh in ((n, OC), (n, IC), r * (IC + OC)))
    ax, y = lora_forward(a, b, x, y0, fs, rounding=False)
    adelta, delta, g = lora_backward(a, b, dIn, x, ax, delta0, g0, fs, rounding=False)
    mags = magnitudes(a, b, x, y0, dIn, x, ax, adelta, delta0, g0, fs)
    assert all(m.max() < 2.0 ** 23 for m, _ in mags.values()), "a sum of absolute terms reaches 2^23"
    c = dict(OC=OC, IC=IC, n=n, r=r, s=fs, a=E.exact_bits(a), b=E.exact_bits(b), x=E.exact_bits(x), dIn=E.exact_bits(dIn), y0=E.exact_bits(y0), delta0=E.exact_bits(delta0),
             g0=E.exact_bits(g0), ax=E.exact_bits(ax), y=E.exact_bits(y), adelta=E.exact_bits(adelta), delta=E.exact_bits(delta), g=E.exact_bits(g))   # exact_bits asserts bf16 values
    c["f64"] = dict(ax=ax, adelta=adelta, y=y, delta=delta, g=g)
    return c


EXACT_SHAPES = [(128, 128, 64, 16, 1), (128, 256, 192, 32, 1), (320, 192, 448, 64, 2), (3072, 1024, 512, 16, 2)]   # (OC, IC, n, r, s)
BLOCK_SHAPE = (320, 192, 448, 64, 1)   # three slabs of 2, 2 and 3 k-steps for both gradients: the block lies astride the first seam
RANDOM_SHAPES = [(128, 256, 192, 32), (320, 192, 448, 64)]
_cache = {}


def exact_case(shape, block=False, hip=None):
    """one case per shape, computed once and shared (the tests copy what they modify)"""
    key = (shape, block)
    if key not in _cache:
        OC, IC, n, r, s = shape
        at = slab_seams(lora_plan(hip, r, OC, IC, n), n)[0] if block else None
        _cache[key] = lora_exact_case(OC, IC, n, r, s, seed=OC + 7 * IC + 13 * n + r + (1000 if block else 0), block_at=at)
    return _cache[key]
