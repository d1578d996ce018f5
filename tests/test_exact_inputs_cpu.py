"""Everything about the exact-arithmetic inputs (tests/exact_inputs.py) that can be settled without a GPU, for every case tests/test_gpu_exact_linear_backward.py,
tests/test_gpu_exact_linear_forward.py, tests/test_gpu_exact_attention.py, tests/test_gpu_exact_score.py and tests/test_gpu_exact_attention_decode.py run:

  preconditions   every operand is a bf16 value, every expected accumulator an integer (or half) inside the bound -- asserted by the helpers as the cases are built
  probabilities   an fp32 emulation of the softmax statistics AS THE KERNELS COMPUTE THEM (running maximum per key tile, exp2 of score x scale x log2 e - M,
                  L = (M + log2 l) ln 2, the forward's bf16 score store, the paired form's merge) gives exactly 0, 1/2 or 1 after the bf16 store and leaks exactly 0.0f
  references      the closed forms equal a plain fp64 softmax reference; that reference agrees with the oracle's attn_backward to a bf16 unit, bit for bit off the ties
  form coverage   the plan (kfdbg_gemm_plan / kfdbg_attn_plan) sends the case tables down every form the entry points have; what no small shape reaches is listed
  power           one term removed, doubled or moved, one key admitted or dropped, changes the expected BITS -- and passes the global-max bars used so far"""
import fnmatch

import numpy as np
import pytest

from koifish_amd import lib as L
from oracle import oracle as O
from tests import exact_inputs as E

LOG2E = np.float32(1.44269502162933349609375)
LN2 = np.float32(0.693147182464599609375)
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


def same_values(a_bits, b_bits):
    """bf16 arrays equal as numbers (an fp64 reference may reach a zero as -1e-50: -0.0 after the stores)"""
    return np.array_equal(E.f64(a_bits), E.f64(b_bits))


# ---------------------------------------------------------------------------------------------------------------- linear backward: preconditions, forms
@pytest.mark.parametrize("family", ["sparse", "block"])
@pytest.mark.parametrize("shape", list(E.LINEAR_CASES))
def test_linear_case_preconditions(hip, shape, family):
    c = E.linear_case(hip, shape, family)   # asserts integers inside the bound on every fp64 product it returns
    for name in ("delta", "delta_acc", "gW", "gb"):
        v = E.f64(c[name])
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= E.BOUND
    if family == "block":   # every output of the input gradient is a dense sum: 128 terms of +-1, an even integer
        d = E.f64(c["delta"])
        assert np.array_equal(d % 2, np.zeros_like(d)) and np.abs(d).max() > 16


def test_linear_twos_and_q4_grid(hip):
    c = E.linear_case(hip, (1024, 256, 1024), "sparse", twos=True)
    assert np.abs(c["f64"]["W"]).max() == 2
    w, ow = E.q4_grid_weight(*E.Q4_CASE[:2], seed=3)   # asserts dequant(quantize(w)) == w against the oracle
    assert w.min() == -7 and w.max() == 8
    E.linear_case(hip, E.Q4_CASE, "sparse", w=w)


# forms of kf_gemm_plan.h gemm_plan_backward that NO legal shape with every side <= 2048 reaches (test_linear_forms_below_2048 enumerates them), and why
BEYOND_2048 = {
    "KMAJOR/BIG/plain": "a 256 x 256 tile is chosen only when the 128 x 128 tiles number >= 410 (else those, or their split, are taken): at most 16 x 16 = 256 here",
    "KMAJOR/BIG/split": "as KMAJOR/BIG/plain",
    "KMAJOR/BIG/tails": "as KMAJOR/BIG/plain",
    "KMAJOR/SMALL/tails": "needs 257 .. 409 tiles of 128 x 128: at most 256 here",
}
# token-batch families tile_plan never returns for the transposed copies at ANY side <= 2048: the route is taken only when IC < 256 or the token side < 256
NEVER_TRANSPOSED = {
    "TRANSPOSE/G2": "ceil(M / 32) ceil(n / 32) <= 8 x 64 = 512 <= 1280: the direct kernel takes whatever the 64 x 64 tiles decline",
    "TRANSPOSE/STAGED": "as TRANSPOSE/G2",
    "TRANSPOSE/G3_MID": "needs >= 192 tiles of 64 x 128 with a side < 256: at most 4 x 16 = 64",
    "TRANSPOSE/G3_SMALL": "needs >= 256 tiles of 128 x 128 with a side < 256: at most 2 x 16 = 32",
    "TRANSPOSE/G3_BIG": "needs both sides >= 256: the K-major route has taken those",
}
WANTED = ["KMAJOR/BIG/plain", "KMAJOR/BIG/split", "KMAJOR/BIG/tails", "KMAJOR/SMALL/plain", "KMAJOR/SMALL/split"]


def test_linear_case_forms(hip):
    """the table names the form each case runs, and between them the cases run every wanted form in BOTH products"""
    got = {e: set() for e in (E.BWD_DX, E.BWD_DW)}
    for shape, want in E.LINEAR_CASES.items():
        for e, w in zip((E.BWD_DX, E.BWD_DW), want):
            p = E.backward_plan(hip, e, *shape)
            assert E.form_name(p) == w, (shape, e)
            got[e].add(w)
            K = shape[0] if e == E.BWD_DX else shape[2]
            if "split" in w:
                assert p.k.S >= 2 and K // p.k.S >= 512 and len(E.seams(p, K)) == p.k.S + 1   # pieces stay >= 512 deep
            if "tails" in w:
                assert p.k.kp > 0 and 64 * p.k.kp in E.seams(p, K) and len(E.seams(p, K)) > 3   # the hand-over and helper-to-helper cuts
    for e in got:
        assert set(WANTED) <= got[e] and "KMAJOR/SMALL/tails" in got[e]


def test_linear_forms_below_2048(hip):
    """every legal shape on a grid of 64 (and two ragged input widths) with every side <= 2048: the forms reached are exactly those of the case table minus
    BEYOND_2048, once per family tile_plan can return for the transposed copies; nothing in NEVER_TRANSPOSED is reached"""
    reached = {e: set() for e in (E.BWD_DX, E.BWD_DW)}
    sides = list(range(128, 2049, 64))
    for OC in sides:
        for IC in sides + [136, 200]:
            for n in sides:
                for e in reached:
                    reached[e].add(E.form_name(E.backward_plan(hip, e, OC, IC, n)))
    table = {e: {w[i] for w in E.LINEAR_CASES.values()} for i, e in enumerate((E.BWD_DX, E.BWD_DW))}
    for e in reached:
        assert reached[e] == table[e] - set(BEYOND_2048), (e, reached[e] ^ (table[e] - set(BEYOND_2048)))
        assert not reached[e] & set(NEVER_TRANSPOSED)
    assert all(max(s) > 2048 for s, w in E.LINEAR_CASES.items() if set(w) & set(BEYOND_2048))   # only those cases go past 2048


# ---------------------------------------------------------------------------------------------------------------- attention: forms
def test_attention_forward_forms(hip):
    """every forward case runs the MFMA tile kernel; 257 tokens of the small head counts run its paired form, FWD_TILE_LONG the unpaired one past 256 tokens"""
    routes = set()
    for nh, nkv in E.HEADS:
        for hd in E.HEAD_DIMS:
            for n in E.FWD_N:
                for n_seq in E.N_SEQ:
                    r = E.forward_route(hip, E.ATTN_BATCH, nh, nkv, hd, n, n_seq)
                    assert r == (E.ATTN_PAIRED if n >= 256 else E.ATTN_TILE)
                    routes.add(r)
                for pos0 in (0, E.FWD_POS0):
                    assert E.forward_route(hip, E.ATTN_PROMPT, nh, nkv, hd, n, 1, pos0) == (E.ATTN_PAIRED if n >= 256 else E.ATTN_TILE)
    assert routes == {E.ATTN_TILE, E.ATTN_PAIRED}
    t = E.FWD_TILE_LONG
    assert t["n"] >= 256 and E.forward_route(hip, E.ATTN_BATCH, t["nh"], t["nkv"], t["hd"], t["n"], t["n_seq"]) == E.ATTN_TILE


# ---------------------------------------------------------------------------------------------------------------- attention: the kernels' fp32 softmax statistics
def exp2f(x):
    """v_exp_f32 on fp32 x: 2^x rounded to fp32 (2^-160 and below: 0.0f, 2^(-inf) = 0)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(x.astype(np.float64)).astype(F32)


def raw_scores(c, s, h):
    """q . k of sequence s, head h: exact integers, every partial sum an fp32 value -> fp32 [T, tot]"""
    T, tot, hd, GQ = c["T"], c["tot"], c["hd"], c["nh"] // c["nkv"]
    q = c["q"][s * T:(s + 1) * T, h * hd:(h + 1) * hd]
    k = c["k"][s * tot:(s + 1) * tot, (h // GQ) * hd:(h // GQ + 1) * hd]
    assert (np.abs(q) @ np.abs(k).T).max() < 2.0 ** 24
    return (q @ k.T).astype(F32)


def walk(sc, tiles, kt, to_log2):
    """online softmax over the key tiles `tiles` of kt keys: (M, l, P) with P[i, j] = the probability key j entered its tile's products with (before any later rescale).
    sc [T, keys]: masked scores (-inf); to_log2: the exponent's unit -- the backward keeps scores in log2 units (1), the forward multiplies (s - M) by log2 e"""
    T = sc.shape[0]
    M, l, P = np.full(T, -np.inf, F32), np.zeros(T, F32), np.zeros(sc.shape, F32)
    for t in tiles:
        s = sc[:, t * kt:(t + 1) * kt]
        if s.shape[1] == 0:
            continue
        mt = s.max(axis=1)
        up = mt > M
        with np.errstate(invalid="ignore"):
            alpha = exp2f(((M - mt) * to_log2).astype(F32))
        l = np.where(up, l * np.where(up, alpha, F32(1)), l).astype(F32)
        rescaled = np.where(up[:, None], P * np.where(up, alpha, F32(1))[:, None], P)   # what earlier tiles contributed, as the kernel rescales O
        M = np.where(up, mt, M)
        Mref = np.where(np.isinf(M), F32(0), M)
        p = exp2f(((s - Mref[:, None]) * to_log2).astype(F32))
        for j in range(p.shape[1]):   # the kernel's adds, one probability at a time
            l = (l + p[:, j]).astype(F32)
        P = rescaled
        P[:, t * kt:(t + 1) * kt] = p
    return M, l, P


def expected_probs(c, s, h):
    T, tot = c["T"], c["tot"]
    w = np.zeros((T, tot))
    two = c["tb"][s, :, h] >= 0
    w[np.arange(T), c["ta"][s, :, h]] = np.where(two, 0.5, 1.0)
    w[np.arange(T)[two], c["tb"][s, two, h]] = 0.5
    return w


FWD_CASES = [(fam, n, nh, nkv, hd, n_seq, pos0) for fam in ("code", "ramp") for n in E.FWD_N for nh, nkv in E.HEADS for hd in E.HEAD_DIMS
             for n_seq, pos0 in ((1, 0), (1, E.FWD_POS0), (3, 0))]


def test_forward_probabilities_are_exact():
    """kf_attn_prefill.hip: score = bf16(fl32(q . k x fl32(1 / sqrt(hd)))), mask, running maximum per tile, p = exp2((s - M) log2 e), l += p, out = O / l.  Both walks: 32-key
    tiles in one pass, and the paired form's 64-key tiles in two halves (even / odd) merged at the end.  Every target enters with p == 1.0f, every other key with 0.0f,
    l == the number of targets: out = (sum of the targets' v) / l exactly."""
    t = E.FWD_TILE_LONG
    for fam, n, nh, nkv, hd, n_seq, pos0 in FWD_CASES + [(f, t["n"], t["nh"], t["nkv"], t["hd"], t["n_seq"], 0) for f in ("code", "ramp")]:
        c = E.attn_case(fam, n, nh, nkv, hd, n_seq, pos0, seed=n + nh + hd, vmax=2)
        rden = E.kernel_scale(hd)
        vis = np.arange(c["tot"])[None, :] <= (pos0 + np.arange(n))[:, None]
        for s in range(n_seq):
            for h in range(0, nh, max(1, nh // 8)):
                st = raw_scores(c, s, h)
                sc = np.where(vis, E.f64(E.bits(st * rden)).astype(F32), F32(-np.inf))
                want = expected_probs(c, s, h)
                cnt = (want > 0).sum(axis=1).astype(F32)
                nt32, nt64 = (c["tot"] + 31) // 32, (c["tot"] + 63) // 64
                M, l, P = walk(sc, range(nt32), 32, LOG2E)
                assert np.array_equal(P, (want > 0).astype(F32)) and np.array_equal(l, cnt), (fam, n, nh, hd, pos0)
                # paired: two partial softmaxes merged with a = exp2((M_half - max) log2 e)
                M0, l0, P0 = walk(sc, range(0, nt64, 2), 64, LOG2E)
                M1, l1, P1 = walk(sc, range(1, nt64, 2), 64, LOG2E)
                Mm = np.maximum(M0, M1)
                with np.errstate(invalid="ignore"):
                    a0, a1 = exp2f(((M0 - Mm) * LOG2E).astype(F32)), exp2f(((M1 - Mm) * LOG2E).astype(F32))
                assert np.isfinite(M0).all()   # the even half has seen key 0
                assert np.array_equal((l0 * a0 + l1 * a1).astype(F32), cnt)
                assert np.array_equal(P0 * a0[:, None] + P1 * a1[:, None], (want > 0).astype(F32))


BWD_CASES = [(fam, T, nh, nkv, hd, n_seq) for fam in ("code", "ramp") for T in E.BWD_T for nh, nkv in E.HEADS for hd in E.HEAD_DIMS for n_seq in E.N_SEQ]


def test_backward_probabilities_are_exact():
    """kf_attn_bwd_mfma.hip: pass A keeps scores in log2 units, sc = fl32(q . k x c1), c1 = fl32(scale x log2 e); running maximum M and l = sum exp2(sc - M) per 32-key tile;
    L = fl32(fl32(M + log2 l) x ln 2).  Both launches then recompute p = exp2(fma(q . k, c1, -fl32(L x log2 e))): NOT exactly 1 or 1/2 (L went through two roundings),
    but within 2^-12 of it, so that the bf16 P operand IS 1 or 1/2 and the bf16 dS operand IS w (dP - D) -- with a margin of 2^3 over what the stores need for the
    last bit of the hardware's exp2.  Every other visible key: exp2 of <= -160, exactly 0.0f; the leaked mass l - (number of targets) is exactly 0.0f."""
    for fam, T, nh, nkv, hd, n_seq in BWD_CASES:
        c = E.attn_case(fam, T, nh, nkv, hd, n_seq, seed=T + nh + hd)
        GQ = nh // nkv
        c1 = (E.kernel_scale(hd) * LOG2E).astype(F32)
        vis = np.tril(np.ones((T, T), bool))
        for s in range(n_seq):
            for h in range(nh):
                st = raw_scores(c, s, h)
                sc = np.where(vis, (st * c1).astype(F32), F32(-np.inf))
                want = expected_probs(c, s, h)
                M, l, P = walk(sc, range((T + 31) // 32), 32, F32(1))
                assert np.array_equal(l, (want > 0).sum(axis=1).astype(F32)), (fam, T, nh, hd)   # leaked mass 0.0f
                assert np.array_equal(P > 0, want > 0)
                Lrow = ((M + np.log2(l.astype(np.float64)).astype(F32)).astype(F32) * LN2).astype(F32)
                L2 = (Lrow * LOG2E).astype(F32)
                with np.errstate(over="ignore", invalid="ignore"):
                    arg = (st.astype(np.float64) * np.float64(c1) - L2[:, None].astype(np.float64)).astype(F32)   # the fma: one rounding
                    p = np.where(vis, exp2f(arg), F32(0))   # future keys may be +inf before the mask: selected away, never multiplied
                assert np.array_equal(p[want == 0], np.zeros((want == 0).sum(), F32))
                on = want > 0
                assert (np.abs(p[on].astype(np.float64) / want[on] - 1.0) <= 2.0 ** -12).all(), (fam, T, nh, hd)
                assert np.array_equal(E.f64(E.bits(p)), want)   # the P operand of dV
                # dS = p (dP - D), packed to bf16: the exact w (dP - D)
                hc, gc = slice(h * hd, (h + 1) * hd), slice((h // GQ) * hd, (h // GQ + 1) * hd)
                dOh = c["dO"][s * T:(s + 1) * T, hc]
                x = dOh @ c["v"][s * T:(s + 1) * T, gc].T - (dOh * c["o"][s * T:(s + 1) * T, hc]).sum(axis=1, keepdims=True)
                assert np.abs(x).max() <= 16
                dS = (p * x.astype(F32)).astype(F32)
                assert np.array_equal(E.f64(E.bits(dS)), want * x)


# ---------------------------------------------------------------------------------------------------------------- attention: closed forms, references, the oracle
def split_seq(c, s):
    T, tot = c["T"], c["tot"]
    return [c[k][s * T:(s + 1) * T] for k in ("q",)] + [c[k][s * tot:(s + 1) * tot] for k in ("k", "v")] + [c[k][s * T:(s + 1) * T] for k in ("o", "dO")]


def test_closed_forms_equal_the_fp64_reference():
    """every case of the GPU module: the closed-form expectation (which also asserts the accumulator bounds) against the plain fp64 softmax reference"""
    for fam, T, nh, nkv, hd, n_seq in BWD_CASES:
        c = E.attn_case(fam, T, nh, nkv, hd, n_seq, seed=T + nh + hd)
        want = E.closed_backward(c)
        for s in range(n_seq):
            q, k, v, o, dO = split_seq(c, s)
            for round_p in (False, True):
                ref = E.attn_backward_ref(q, k, v, o, dO, nh, nkv, hd, round_p=round_p)
                for name in ("dq", "dk", "dv"):
                    assert same_values(ref[name], want[name][s * T:(s + 1) * T]), (fam, T, nh, hd, name)
    for fam, n, nh, nkv, hd, n_seq, pos0 in FWD_CASES:
        c = E.attn_case(fam, n, nh, nkv, hd, n_seq, pos0, seed=n + nh + hd, vmax=2)
        want = E.closed_forward(c)
        assert np.array_equal(4 * want, np.rint(4 * want)) and np.abs(want).max() <= 2   # halves of sums of two small integers: bf16 values
        for s in range(n_seq):
            q, k, v, _, _ = split_seq(c, s)
            assert same_values(E.bits(E.attn_forward_ref(q, k, v, nh, nkv, hd, pos0)), E.bits(want[s * n:(s + 1) * n]))


def near_tie(x):
    """fp64 x within 2^-20 (relative) of the midpoint of two neighbouring bf16 values: where a last-bit difference before the store may round the other way"""
    with np.errstate(divide="ignore"):
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 7)
    r = np.abs(x) / ulp
    return np.abs(r - np.floor(r) - 0.5) <= 2.0 ** -20 * r


@pytest.mark.parametrize("T,nh,nkv,hd", [(19, 2, 2, 64), (40, 4, 2, 128), (33, 8, 1, 64), (70, 4, 1, 128)])
def test_reference_agrees_with_the_oracle(T, nh, nkv, hd):
    """attn_backward_ref against oracle.attn_backward (all fp64, one bf16 store): the only difference is the reference's fp32 multiply by fl32(scale), as the kernels make
    it -- so at most one bf16 unit, and bit-equal wherever the fp64 value is not at a rounding tie.  Random inputs and the exact families."""
    rng = np.random.default_rng(T)
    cases = [[E.f64(O.f32_to_bf16(rng.normal(0, 1.0, (T, w * hd)).astype(np.float32))) for w in (nh, nkv, nkv, nh, nh)]]
    cases += [split_seq(E.attn_case(fam, T, nh, nkv, hd, 1, seed=T), 0) for fam in ("code", "ramp")]
    from tests.conftest import ulp_diff_bf16
    for q, k, v, o, dO in cases:
        ref = E.attn_backward_ref(q, k, v, o, dO, nh, nkv, hd)
        odq, odk, odv = O.attn_backward(*(E.exact_bits(a) for a in (q, k, v, o, dO)), nh, hd, n_kv=nkv)
        for name, got in (("dq", odq), ("dk", odk), ("dv", odv)):
            d = ulp_diff_bf16(ref[name], got) * (E.f64(ref[name]) != E.f64(got))   # (+-0 are equal)
            assert d.max() <= 1, name
            x = ref["acc"][name] * (1.0 if name == "dv" else 1.0 / np.sqrt(float(hd)))
            assert near_tie(x[d > 0]).all(), name
            assert (d > 0).mean() <= 1e-3, name


# ---------------------------------------------------------------------------------------------------------------- power
def bar_accepts(got, ref, rel_max, rel_rms=None):
    """the criteria of tests/test_gpu_linear_backward.py (2^-8 of max|ref|) and tests/test_gpu_gpt2_ops.py's attention backward (2^-7 max, 2^-9 rms)"""
    ok = np.abs(got - ref).max() <= rel_max * np.abs(ref).max() + 1e-6
    return ok and (rel_rms is None or np.sqrt(((got - ref) ** 2).mean()) <= rel_rms * np.abs(ref).max())


@pytest.mark.parametrize("family", ["sparse", "block"])
@pytest.mark.parametrize("shape", [(1024, 256, 1024), (2048, 2176, 2048)])
def test_one_wrong_term_changes_the_bits(hip, shape, family):
    """the fp64 reference of each product (input gradient delta = deltaIn . W, weight gradient gW = prior + deltaIn^T . inp) with one non-zero term removed, doubled, or
    added to the neighbouring output column instead -- at sampled contraction indices and on both sides of every seam of the form: the expected bits change every time"""
    c = E.linear_case(hip, shape, family)
    f = c["f64"]
    rng = np.random.default_rng(1)
    for entry, a, b, name, K in ((E.BWD_DX, f["dIn"], f["W"], "delta", shape[0]), (E.BWD_DW, f["dIn"].T, f["inp"], "gW", shape[2])):   # y [r, col] = sum_k a[r, k] b[k, col]
        y = E.f64(c[name])
        assert np.abs(y).max() + 2 <= E.BOUND   # a result one term away is still an integer bf16 holds
        ks = [k for s in E.seams(E.backward_plan(hip, entry, *shape), K) for k in (s - 1, s) if 0 <= k < K] + list(rng.integers(0, K, 16))
        n_checked = 0
        for k in ks:
            rows, cols = np.nonzero(a[:, k])[0], np.nonzero(b[k])[0]
            if not len(rows) or not len(cols):
                continue
            r, col = rows[rng.integers(len(rows))], cols[rng.integers(len(cols))]
            term = a[r, k] * b[k, col]
            nb = col + 1 if col + 1 < y.shape[1] else col - 1
            for mut in ("removed", "doubled", "moved"):
                m = y[r].copy()
                m[col] += term if mut == "doubled" else -term
                if mut == "moved":
                    m[nb] += term
                assert E.bits(m)[col] != c[name][r, col], (name, k, mut)
                assert mut != "moved" or E.bits(m)[nb] != c[name][r, nb]
            n_checked += 1
        assert n_checked >= 8, name


def test_the_global_max_bar_accepts_one_wrong_term():
    """the record of why these tests exist: N(0, 1) operands, a contraction of 3072 (the GPT-2 shapes of tests/test_gpu_linear_backward.py) -- one product of typical
    size dropped from one output passes max|got - ref| <= 2^-8 max|ref|"""
    rng = np.random.default_rng(0)
    a = E.f64(O.f32_to_bf16(rng.normal(0, 1.0, (256, 3072)).astype(np.float32)))
    b = E.f64(O.f32_to_bf16(rng.normal(0, 1.0, (3072, 256)).astype(np.float32)))
    ref = a @ b
    bar = 2.0 ** -8 * np.abs(ref).max()
    terms = np.abs(a[7, :] * b[:, 9])
    k = int(np.argsort(terms)[len(terms) // 2])   # the median-sized term of that output
    got = ref.copy()
    got[7, 9] -= a[7, k] * b[k, 9]
    assert got[7, 9] != ref[7, 9] and bar_accepts(got, ref, 2.0 ** -8)
    assert (terms <= bar).mean() >= 0.5   # and so do most of its terms


@pytest.mark.parametrize("T,nh,nkv,hd,draw", [(130, 2, 2, 64, 2), (300, 4, 2, 128, 8)])
def test_one_wrong_mask_decision_changes_the_bits(T, nh, nkv, hd, draw):
    """exact families: a future key admitted at ONE row (ramp: it takes the whole row), the diagonal dropped at one row (code: a row whose target it is) -- dq, dk and dv
    all change.  And the record: on random peaked inputs (q scaled by 4) a future key admitted at one row in 32 changes hundreds of output values, and whether the
    2^-7 max / 2^-9 rms bars notice depends on the draw -- on whether an admitted key happens to score near its row's maximum.  Of the draws 0 .. 11 of this generator
    the error passes both bars on 2 and 6 at (T 130, hd 64) and on 8 at (T 300, hd 128), by a factor of up to 6; on others it misses them by up to 90 x.  The
    draws pinned here pass."""
    causal = np.tril(np.ones((T, T), bool))
    for fam in ("ramp", "code"):
        c = E.attn_case(fam, T, nh, nkv, hd, 1, seed=T)
        q, k, v, o, dO = split_seq(c, 0)
        want = E.closed_backward(c)
        diag = [i for i in range(1, T) if (c["ta"][0, i] == i).any()]   # code: rows with a head whose target is the diagonal -- the ones nearest the seams
        rows = [31, 32, 127, 128, T - 2] if fam == "ramp" else sorted({min(diag, key=lambda i: abs(i - at)) for at in (31, 32, 127, 128, T - 1)} | set(diag[::len(diag) // 4]))
        assert len(rows) >= 3
        for i in rows:
            vis = causal.copy()
            if fam == "ramp":
                vis[i, i + 1] = True
            else:
                vis[i, i] = False
            got = E.attn_backward_ref(q, k, v, o, dO, nh, nkv, hd, vis=vis, round_p=True)
            for name in ("dq", "dk", "dv"):
                assert not same_values(got[name], want[name]), (fam, i, name)
    rng = np.random.default_rng(draw)
    q, k, v, o, dO = (E.f64(O.f32_to_bf16((rng.normal(0, 1.0, (T, w * hd)) * g).astype(np.float32))) for w, g in ((nh, 4.0), (nkv, 1.0), (nkv, 1.0), (nh, 1.0), (nh, 1.0)))
    vis = causal.copy()
    for i in range(5, T - 1, 32):
        vis[i, i + 1] = True
    ref = E.attn_backward_ref(q, k, v, o, dO, nh, nkv, hd, round_p=True)
    got = E.attn_backward_ref(q, k, v, o, dO, nh, nkv, hd, vis=vis, round_p=True)
    for name in ("dq", "dk", "dv"):
        assert not np.array_equal(got[name], ref[name])
        assert bar_accepts(E.f64(got[name]), E.f64(ref[name]), 2.0 ** -7, 2.0 ** -9), name


# ---------------------------------------------------------------------------------------------------------------- forward token-batch GEMMs: storages, cases, forms, power
GROUP_STORAGES = [s for s, (t, lut, _, _) in E.STORAGES.items() if O.BITS[t] < 8 and not lut]


def _whole_groups(storage, K):
    """K is made of whole groups and (ternary, 1-bit) of whole 128-element tiles: the layouts the kernels take"""
    type_, row_lut, _, lgroup = E.STORAGES[storage]
    return row_lut or O.BITS[type_] >= 8 or (K % lgroup == 0 and (O.BITS[type_] == 4 or K % 128 == 0))


@pytest.mark.parametrize("storage,M,K", [(s, M, K) for s in E.STORAGES for M, K in ((40, 256), (96, 1600), (64, 192)) if _whole_groups(s, K)])
def test_exact_weight_holds_integers_in_every_storage(storage, M, K):
    """exact_weight asserts O.dequant(ow) == W itself; here what makes a wrong read visible: step in {1, 2} and integer zeros that differ from each group to the next, at
    least two codes per group, both qBias values of the 4-bit range, every nibble in use; a row codebook of 16 integers that differs from row to row"""
    type_, row_lut, symmetric, lgroup = E.STORAGES[storage]
    W, ow = E.exact_weight(storage, M, K, seed=M + K)
    assert np.array_equal(W, np.rint(W)) and np.abs(W).max() <= 32 and (W != 0).any()
    assert np.array_equal(E.f64(O.dequant(ow)), W)
    if row_lut:
        t = E.f64(ow.lut)
        assert t.shape == (M, 16) and np.array_equal(t, np.rint(t)) and (np.sort(t, axis=1) == np.arange(-8, 8)).all()
        assert (t[1:] != t[:-1]).any(axis=1).all()
    elif storage in GROUP_STORAGES:
        zero, step = E.f64(ow.zero), E.f64(ow.step)
        assert set(np.unique(step)) == {1.0, 2.0} and np.array_equal(zero, np.rint(zero)) and len(np.unique(zero)) >= 3
        assert ((zero[1:] != zero[:-1]) | (step[1:] != step[:-1])).all()
        codes = O.unpack(ow.data, O.BITS[type_]).reshape(-1, lgroup)
        assert (codes.min(axis=1) != codes.max(axis=1)).all()
        assert ow.qBias == ((8 if symmetric else 0) if type_ == O.Q4 else (1 if type_ == O.T_SIGN else 0))
        if type_ == O.Q4:
            assert set(np.unique(codes)) == set(range(16))


@pytest.fixture(scope="module")
def forward_cases(hip):
    """every case of the GPU module, built once: the helpers assert integer products inside the bound, term sums below 2^23, dequant == the integer weight, and the
    epilogue's intermediates as they go"""
    return {key: E.forward_case(hip, key) for key in E.FORWARD_CASES}


def test_forward_case_preconditions(forward_cases):
    for key, c in forward_cases.items():
        for part in [c] + c["more"]:
            y = E.f64(part["y"])
            assert np.array_equal(y, np.rint(y)) and np.abs(y).max() <= E.BOUND and (y != 0).mean() > 0.5, key
            assert np.array_equal(E.f64(O.dequant(part["ow"])), part["W"]), key
        x = c["f64"]["x"]
        assert set(np.unique(x)) == {-1.0, 0.0, 1.0}
        assert (np.abs(x) @ np.abs(c["W"]).T).max() < 2.0 ** 23, key   # the sum of the terms' magnitudes: every partial sum in every order is an fp32 value
        if key[5] == "block":   # every output a dense sum of 128 terms +-s: even
            assert np.array_equal(E.f64(c["y"]) % 2, np.zeros(c["y"].shape)) and np.abs(E.f64(c["y"])).max() > 16, key
            assert ((x != 0).sum(axis=1) == 128).all()
        if key[6] == "epi":
            e = c["f64_epi"]
            y1 = E.f64(E.bits(E.ALPHA * c["f64"]["acc"] + E.BETA * e["y0"] + e["bias"]))
            assert np.array_equal(c["y_epi"], E.bits(y1 + e["residual"])) and not np.array_equal(c["y_epi"], c["y"]), key
        if len(c["more"]):   # a distinct weight per matrix
            assert all(not np.array_equal(c["W"][:64], m["W"][:64]) for m in c["more"]), key


# every name the rule can give a kf_linear call with nothing lent (every in-register family on every format that has it: the producer / consumer kernel exists for
# bf16, f8 and 4-bit groups only), with the scratch kf_linear_scratch_bytes asks for, and on a resident copy whose k is too shallow to
# cut (K 256) -- test_forward_forms_reached enumerates them; the table holds a case of each.  With a deeper k the resident 64-row tiles run in 2 .. 8 pieces of one
# kernel: the table holds S 2, 3 and 6 and the owner / helper cut.
LINEAR_NAMES = {
    "": [fam + f for fam in ("TILE/DIRECT/32/", "TILE/STAGED/KS2/", "TILE/STAGED/KS1/") for f in ("bf16", "f8", "q4", "q2", "q1", "q4r")]
        + ["TILE/G2/bf16", "TILE/G2/f8", "TILE/G2/q4"] + ["TILE/G3/" + f for f in ("TINY", "MID", "SMALL", "BIG")] + ["MATVEC"],
    "scratch": ["DEQ_TILE/G3/SMALL", "DEQ_TILE/G3/BIG"],
    "arena": ["RESIDENT/DIRECT/32/bf16"] + ["RESIDENT/G3/" + f for f in ("TINY", "MID", "SMALL", "BIG")],
}
SPLIT_NAMES = ["RESIDENT/G3/TINY/S2", "RESIDENT/G3/TINY/S3", "RESIDENT/G3/TINY/S6", "RESIDENT/G3/MID/S2", "RESIDENT/G3/MID/tails"]
SHARED_NAMES = ["FUSED/DIRECT/32/q4", "FUSED/DIRECT/64/q4", "STACKED/G3/SMALL", "STACKED/G3/BIG", "FUSED/PAIRED/q4", "SWIGLU/G3/SMALL", "SWIGLU/G3/WIDE", "SWIGLU/G3/BIG",
                "ROPE/G3/SMALL"]


def test_forward_cases_are_pinned_against_the_plan(hip):
    """the table names the plan of each case as kf_abi.hip's entry makes it (the same scratch bytes, the same arena state), and between them the cases reach every name"""
    assert E.SK_WS_BYTES == hip.kf_resident_scratch_bytes()   # what the "arena" cases lend
    got = set()
    for key, want in E.FORWARD_CASES.items():
        p = E.case_plan(hip, key)
        assert E.forward_name(p) == want, key
        got.add(want)
        scratch, arena = E.case_setting(key)
        assert p.deq == (E.DQ_ARENA if arena else (E.DQ_SCRATCH if scratch else E.DQ_NONE)), key
        if arena:   # the second call finds the copy: the same kernel, nothing dequantised
            p2 = E.case_plan(hip, key, arena_hit=1)
            assert E.forward_name(p2) == want and p2.deq == E.DQ_RESIDENT and (p2.k.S, p2.k.kp, p2.k.R) == (p.k.S, p.k.kp, p.k.R), key
        if p.k.sk and p.k.S >= 2:
            S = int(want.rsplit("/S", 1)[1])
            assert p.k.S == S and key[3] // 64 // S >= 8 and len(E.seams(p, key[3])) == S + 1, key   # pieces stay >= 512 deep
        if want.endswith("/tails"):
            assert p.k.kp > 0 and 64 * p.k.kp in E.seams(p, key[3]) and len(E.seams(p, key[3])) > 3, key
        if key[1] in GROUP_STORAGES and p.k.fam in (1, 2, 3, 4) and p.deq == E.DQ_NONE:   # the in-register kernels index the group tables by block >> gshift
            epb = {4: 32, 2: 64, 1: 128}[O.BITS[E.STORAGES[key[1]][0]]]
            assert 1 << p.k.gshift == E.STORAGES[key[1]][3] // epb, key
    assert set(sum(LINEAR_NAMES.values(), []) + SPLIT_NAMES + SHARED_NAMES) <= got
    assert {(k[1], E.FORWARD_CASES[k].split("/")[1]) for k in E.FORWARD_CASES if k[6] == "epi"} == {("q4", "DIRECT"), ("q4", "STAGED"), ("q4", "G2"), ("bf16", "G3")}
    gshifts = {(k[1][:2], E.case_plan(hip, k).k.gshift) for k in E.FORWARD_CASES if k[1] in GROUP_STORAGES and E.FORWARD_CASES[k].startswith("TILE")}
    assert gshifts >= {("q4", 1), ("q4", 2), ("q4", 3), ("te", 1), ("bo", 0), ("bo", 1)}
    for name in E.FORWARD_UNREACHABLE:
        assert not any(fnmatch.fnmatchcase(g, name) for g in got), name


def test_forward_forms_reached(hip):
    """kf_linear over a grid of shapes (ragged and whole, 32 .. 65536 rows, 7 .. 65536 tokens, with a side below 128 against a very long one: where kf_gemm3.hip and
    the producer / consumer kernel decline), every storage: the names reached are exactly LINEAR_NAMES -- the table misses none, and nothing listed as unreachable is
    reached"""
    Ms = [32, 40, 96, 127, 128, 256, 512, 1024, 1056, 2048, 4096, 6400, 8192, 16384, 32768, 65536]
    ns = [7, 8, 64, 96, 127, 129, 224, 255, 256, 320, 512, 641, 1024, 1281, 1536, 1664, 2048, 2304, 2560, 4096, 8192, 16384, 32768, 65536]
    for setting, storages in (("", ("q4", "q4s", "f8", "tern", "bool1", "tbin", "bf16", "lut")), ("scratch", ("q4", "tern")), ("arena", ("q4", "tern"))):
        route = {"": ("TILE", "MATVEC"), "scratch": ("DEQ_TILE",), "arena": ("RESIDENT",)}[setting]
        reached = set()
        for st in storages:
            for M in Ms:
                for n in ns:
                    scratch, arena = E.case_setting(("linear", st, (M,), 256, n, "sparse", setting))
                    reached.add(E.forward_name(E.forward_plan(hip, "linear", st, (M,), 256, n, scratch=scratch, arena=arena)))
        reached = {r for r in reached if r.split("/")[0] in route}
        assert reached == set(LINEAR_NAMES[setting]), (setting, reached ^ set(LINEAR_NAMES[setting]))
        assert not any(fnmatch.fnmatchcase(r, u) for r in reached for u in E.FORWARD_UNREACHABLE)
    deep = {E.forward_name(E.forward_plan(hip, "linear", "q4", (M,), K, n, scratch=E.SK_WS_BYTES, arena=True)) for K in (1024, 2048, 3072, 4096) for M in Ms for n in ns}
    cut = {d for d in deep if d.startswith("RESIDENT/G3/") and d.count("/") == 3}
    assert set(SPLIT_NAMES) <= cut and {d.rsplit("/", 1)[0] for d in cut} == {"RESIDENT/G3/TINY", "RESIDENT/G3/MID"} and "RESIDENT/G3/TINY/tails" not in cut


def _neighbours_table(ow, g):
    """the weight dequantised with group g reading group g + 1's (zero, step): fp64 [M, K]"""
    z, s = ow.zero.copy(), ow.step.copy()
    z[g], s[g] = ow.zero[g + 1], ow.step[g + 1]
    return E.f64(O.dequant_q128(ow.data, z, s, ow.lGroup, 4, ow.qBias)).reshape(ow.ne0, ow.ne1)


def _gaussian(seed, M, K, n, lgroup=128, symmetric=False):
    """operands of tests/test_gpu_gemm.py's scale: w ~ N(0, 0.02) through the 4-bit RTN, x ~ N(0, 1) -> (oracle weight, its dequantised values, x), fp64"""
    rng = np.random.default_rng(seed)
    w = O.f32_to_bf16(rng.normal(0, 0.02, (M, K)).astype(np.float32))
    x = E.f64(O.f32_to_bf16(rng.normal(0, 1.0, (n, K)).astype(np.float32)))
    ow = O.quantize(w, M, K, O.Q4, lGroup=lgroup, symmetric=symmetric)
    return ow, E.f64(O.dequant(ow)), x


def test_the_last_64_contraction_indices_dropped_for_one_row_block(forward_cases):
    """K = 1600 (a half-empty last staged tile): the last 64 contraction indices lost for one block of 32 rows.  Exact inputs: two thirds of that block's outputs change
    their bits, on the direct and on the staged case.  The record for the old bar, observed, not assumed: on Gaussian operands of the existing tests' scale this fault
    is NOT subtle -- it moves an output by 0.17 .. 0.21 of max|exact| (draws 0 .. 3), 40 - 50 x the 2^-8 bar, which rejects it wherever a test runs such a K (none of
    tests/test_gpu_gemm.py's shapes has K % 128 != 0)."""
    for key in [k for k in E.FORWARD_CASES if k[3] == 1600 and k[1] == "q4g64"]:
        c = forward_cases[key]
        for rb in range(0, 96, 32):
            Wm = c["W"].copy()
            Wm[rb:rb + 32, 1536:] = 0
            got = E.bits(c["f64"]["x"] @ Wm.T)
            assert (got[:, rb:rb + 32] != c["y"][:, rb:rb + 32]).mean() > 0.5 and np.array_equal(np.delete(got, np.s_[rb:rb + 32], 1), np.delete(c["y"], np.s_[rb:rb + 32], 1))
    for draw in range(4):
        ow, deq, x = _gaussian(draw, 96, 1600, 40, lgroup=64)
        ref = x @ deq.T
        deq[32:64, 1536:] = 0
        got = E.f64(E.bits(x @ deq.T))
        assert 0.15 <= np.abs(got - ref).max() / np.abs(ref).max() <= 0.25 and not bar_accepts(got, ref, 2.0 ** -8)


def test_one_groups_table_index_shifted_by_one(forward_cases):
    """one 4-bit group reading its neighbour's (zero, step).  Exact inputs: all or nearly all of the group's 128 entries become other integers and the bits of most
    outputs of that weight row change (at K 256 nearly all) -- which q4_grid_weight, with step 1 and zero -7 in every group, could not show.  The record for the old bar, observed: with
    the asymmetric range (zero = -min of the group) the fault moves an output by 0.024 .. 0.56 of max|exact| on Gaussian operands and the 2^-8 bar rejects it on every
    draw tried; with the symmetric range (zero = 0, neighbouring steps a few per cent apart) it depends on the draw: at 2048 x 1024 x 128 tokens the error was 0.0032
    of max|exact| on draw 0 -- the bar ACCEPTED, with 86 output values changed -- and 0.0044 .. 0.092 on draws 1 .. 5 and 7, which it rejected (0.0044 by a hair).
    That last outcome is a property of the draws, so it is recorded here and printed, not asserted; asserted is that the exact bits change on every draw."""
    for key in (("linear", "q4", (40,), 256, 129, "sparse", ""), ("linear", "q4s", (40,), 256, 129, "sparse", ""), ("linear", "q4g64", (96,), 1600, 40, "sparse", "")):
        c = forward_cases[key]
        ow, K = c["ow"], key[3]
        for g in (0, 5, 38, ow.zero.size - 2):
            Wm = _neighbours_table(ow, g)
            row = g * ow.lGroup // K
            assert (Wm != c["W"]).sum() >= ow.lGroup * 3 // 4 and np.array_equal(np.delete(Wm, row, 0), np.delete(c["W"], row, 0))
            got = E.bits(c["f64"]["x"] @ Wm.T)
            assert (got[:, row] != c["y"][:, row]).mean() > 0.5, (key, g)
    for draw in range(6):
        for shape in ((40, 256, 129), (2048, 1024, 128)):
            ow, deq, x = _gaussian(draw, *shape)
            ref = x @ deq.T
            got = E.f64(E.bits(x @ _neighbours_table(ow, 5).T))
            assert not bar_accepts(got, ref, 2.0 ** -8) and np.abs(got - ref).max() >= 0.02 * np.abs(ref).max()
        ow, deq, x = _gaussian(draw, 2048, 1024, 128, symmetric=True)
        ref = x @ deq.T
        got = E.bits(x @ _neighbours_table(ow, 5).T)
        assert (got != E.bits(ref)).sum() >= 64
        print("symmetric range, draw %d: max error %.4f of max|exact|, the 2^-8 bar %s" % (draw, np.abs(E.f64(got) - ref).max() / np.abs(ref).max(),
                                                                                        "accepts" if bar_accepts(E.f64(got), ref, 2.0 ** -8) else "rejects"))


# ---------------------------------------------------------------------------------------------------------------- the scoring head: the level family
@pytest.fixture(scope="module")
def score_cases(hip):
    """every case of tests/test_gpu_exact_score.py, built once: level_case asserts integer logits within +-256, the winner sets, the gap and the zero rows as it goes"""
    return {key: E.score_case(hip, key) for key in E.SCORE_CASES}


def test_score_cases_are_pinned_against_the_plan(hip, score_cases):
    """the table names the plan of each case (route, tile form, vocabulary tiles x row blocks, or the panel's rows), and between them the cases reach both tile forms by
    the rule and by the knob, more than 64 and more than 128 partials per row, one k step and several, and the panel route for every reason it is taken"""
    names = set()
    for key, want in E.SCORE_CASES.items():
        p = E.score_plan(hip, key)
        assert E.score_name(p) == want, key
        names.add(want.rsplit("/", 1)[0])
        if p.route == E.SR_FUSED:
            assert (p.n_vt, p.n_rb) == (-(-key[1] // score_cases[key]["bm"]), -(-key[3] // score_cases[key]["bm"]))
    assert names == {"FUSED/SMALL", "FUSED/BIG", "PANEL"}
    fused = [E.score_plan(hip, k) for k in E.SCORE_CASES if k[4] == 0 and k[0] == "bf16" and k[2] % 64 == 0]
    assert {p.route for p in fused} == {E.SR_FUSED} and max(p.n_vt for p in fused if p.form == E.SCORE_SMALL) > 128 and max(p.n_vt for p in fused if p.form == E.SCORE_BIG) > 64
    assert {k[2] for k in E.SCORE_CASES if E.SCORE_CASES[k].startswith("FUSED")} == {64, 192, 1024}
    assert {k[0] for k in E.SCORE_CASES if E.SCORE_CASES[k].startswith("PANEL")} == {"bf16", "q4", "tern"}


def test_level_case_preconditions(score_cases):
    """what makes the closed form hold, and what makes a wrong fold visible, over every case: the gap to the winners is >= 88 > 87.33654 (kf_expf's exact zero), the
    field is not empty, the targets take every kind, the winner sets sit on the seams the family is about, and the expectation equals a plain restatement of the fold"""
    assert O.expf(np.float32([0.0]))[0] == 1.0 and O.expf(np.float32([-(E.LEVEL_TOP - E.LEVEL_FIELD)]))[0] == 0.0 and O.expf(np.float32([-87.3]))[0] > 0.0
    for key, c in score_cases.items():
        V, n, bm, lg = c["V"], c["n"], c["bm"], c["logits"]
        assert np.array_equal(E.f64(O.dequant(c["ow"])), c["W"]), key
        lev = c["level"]
        assert lev[0] and (n < 4 or not lev[E.ZERO_ROW_AT])
        field = np.where(lg == E.LEVEL_TOP, 0.0, lg)[lev]
        assert np.abs(field).max() <= E.LEVEL_FIELD and (field != 0).mean() > 0.3, key
        tg = c["targets"]
        assert ((tg >= -1) & (tg < V)).all()
        if n >= 16:
            assert (tg == -1).any() and (tg == 0).any() and (tg == V - 1).any() and len(set(tg.tolist())) >= 6, key
            t = lg[np.arange(n), np.maximum(tg, 0)]
            assert (t[lev & (tg >= 0)] == E.LEVEL_TOP).any() and ((t != E.LEVEL_TOP) & (t != 0))[lev & (tg >= 0)].any(), key   # winners and non-zero field values are scored
        w = c["winners"]
        half = bm // 2
        assert [len(s) for s in w[:4]] == [1, 1, 1, 1] and w[0][0] == 0 and w[1][0] == V - 1 and w[2][0] % bm == 0 and (w[3][0] % bm == bm - 1 or w[3][0] == V - 1)
        if V > bm:
            assert w[4][1] - w[4][0] == 1 and w[4][1] % bm == half and w[5][0] % 4 == 3 and w[5][1] - w[5][0] == 1 and w[6][0] % 16 == 15 and w[6][1] - w[6][0] == 1
            assert len(w[9]) == -(-V // bm) and (np.diff(w[9] // bm) == 1).all() and len(w[11]) == 64 and len(w[10]) == 3
            assert w[8][0] // bm != w[8][1] // bm and (w[8][0] // bm) % 64 != (w[8][1] // bm) % 64
        if -(-V // bm) > 65:
            assert w[7][1] // bm - w[7][0] // bm == 64
        if -(-V // bm) > 130:
            assert len(w[13]) == 3 and set(np.diff(w[13] // bm)) == {64}
        got = E.level_fold(lg, tg, V, bm)
        for a, b in zip(got, (c["lp"], c["lse"], c["top1"])):
            assert np.array_equal(a, b), key


MUTATION_KEYS = [("bf16", 4096 + 72, 64, 129, 0, -1), ("bf16", 128 * 130 + 5, 64, 40, 0, -1), ("bf16", 256 * 65 + 72, 64, 40, 0, E.SCORE_BIG), ("q4", 1000, 128, 130, 0, -1)]


@pytest.mark.parametrize("key", MUTATION_KEYS)
def test_one_wrong_fold_decision_changes_the_bits(score_cases, key):
    """a numpy restatement of the fold with ONE wrong decision -- a column dropped, a column counted twice, column V admitted (the tile loads clamp to row V - 1, so it
    reads as a copy of it), a tile left out (one that holds no winner of most rows: the zero rows and the rows with a winner in every tile see it), a tie sent to the higher index, the
    target's logit read from the neighbouring tile: every one changes expected bits, in the outputs named below.

    The record for the bar used so far (lse within d = 2^-7 max|logit| of the row, logprob within 2 d, top1 free within d), observed on the planted Gaussian rows of
    tests/test_gpu_score.py (33 x 4096 x 1024, seed 4129, and 130 x 4168 x 1024, seed 4298; 2 d is about 0.16), with each fault applied to EVERY row -- a finding, not
    an assertion:
      a column that is not the winner dropped, or counted twice    lse moves by at most 0.011 d: passes on every row
      a tile of 128 columns without the winner left out            lse moves by at most 0.48 d: passes on every row
      column V admitted (a copy of column V - 1)                   passes on every row but the one whose winner is V - 1 (1 of 33, 1 of 130)
      the winner dropped, counted twice, or its tile left out      lse moves by 7 .. 37 d: rejected on every row
      the target's logit read from the neighbouring tile           logprob moves by |t - t'|, 2.7 on average: rejected on 26 of 28 and 101 of 111 scored rows, passes on the rest
      a tie sent to the higher index                               invisible: the planted rows have no tie (one test holds ties, on 40 rows and two tiles)
    So the old bar sees a fault of the fold only where it touches the row's winner or a scored target."""
    c = score_cases[key]
    V, n, bm, lg, tg, lev = c["V"], c["n"], c["bm"], c["logits"], c["targets"], c["level"]
    want = (c["lp"], c["lse"], c["top1"])

    def changed(mut):
        got = E.level_fold(lg, tg, V, bm, mut)
        return [np.nonzero(a != b)[0] for a, b in zip(got, want)]
    zero = np.nonzero(~lev)[0]
    assert len(zero)
    for v in (0, V - 1, int(c["winners"][4][0]), int(c["winners"][9][len(c["winners"][9]) // 2])):
        rows = np.nonzero(lg[:, v] == np.where(lev, E.LEVEL_TOP, 0.0))[0]   # the rows that count column v: its winners' rows and every zero row
        assert set(zero) <= set(rows) and len(rows) > len(zero)
        for mut in ("drop", "twice"):
            lp, lse, top1 = changed((mut, v))
            assert set(lse) == set(rows) and set(top1) <= set(rows) and set(lp) <= set(rows), (mut, v)   # every row that counts v, and no other
    lp, lse, top1 = changed(("admit",))
    assert set(zero) <= set(lse) and {r for r in range(n) if lev[r] and V - 1 in c["winners"][r % E.LEVEL_P]} <= set(lse) and len(lse) > len(zero)
    t_skip = (c["winners"][9][-1] // bm) // 2 + 1 if V > bm else 0
    lp, lse, top1 = changed(("skip", int(t_skip)))
    assert set(zero) <= set(lse) and {r for r in range(n) if lev[r] and r % E.LEVEL_P == 9} <= set(lse)
    lp, lse, top1 = changed(("tie_high",))
    assert set(top1) == {r for r in range(n) if c["count"][r] > 1} and not len(lse) and not len(lp)
    lp, lse, top1 = changed(("neighbour",))
    assert len(lp) >= (1 if V <= bm else n // 4) and not len(lse) and not len(top1)


# ---------------------------------------------------------------------------------------------------------------- the decode kernels on the one-hot / two-hot families
def _decode_cases():
    """(family, pos, nh, nkv, hd, shift, nbits) of every kf_attn_decode call of tests/test_gpu_exact_attention_decode.py with the device position at the bound"""
    out = []
    for pos in E.DECODE_POS:
        for nh, nkv in E.HEADS:
            for hd in E.HEAD_DIMS:
                out += [("code", pos, nh, nkv, hd, sh, E.NBITS) for sh in range(0, E.DECODE_KINDS, nh)] + [("ramp", pos, nh, nkv, hd, 0, E.NBITS)]
    t = E.DECODE_LONG
    for hd in E.HEAD_DIMS:
        out += [("code", t["pos"], t["nh"], t["nkv"], hd, sh, t["nbits"]) for sh in range(0, E.DECODE_KINDS, t["nh"])] + [("ramp", t["pos"], t["nh"], t["nkv"], hd, 0, t["nbits"])]
    return out


def test_decode_plans_are_pinned(hip):
    """kfdbg_attn_plan against decode_slices (the rule restated) for every decode case in both orders, and the points the cases are about: one slice up to 192 keys with 8
    waves from 129 keys for GQ <= 2, four slices at 193 keys, 32 slices of 64 at 2047 keys, five of 61 for the bound 300; the per-token route below 8 tokens and for a q
    stride the tile kernel refuses.  Over the calls of a shape the targets take every kind; from two slices on they sit on the first and the last key of a slice and the
    two-hot pair straddles two slices."""
    for canon in (0, 1):
        for pos in E.DECODE_POS + [E.DECODE_LONG["pos"], E.DECODE_BOUND]:
            for nh, nkv in E.HEADS:
                for hd in E.HEAD_DIMS:
                    p = E.attn_plan(hip, E.ATTN_DECODE, nh, nkv, hd, 1, 1, pos, canon)
                    assert (p.route, p.n_splits, p.chunk, p.nw, p.gq_split) == (E.ATTN_SLICED,) + E.decode_slices(pos, nkv, nh // nkv, canon), (pos, nh, nkv, canon)
                    assert p.scratch == hip.kf_attn_scratch_bytes(nh, hd) and p.n_splits <= 32
    S = E.decode_slices
    assert [S(p, 2, 1, 0)[:3] for p in (128, 129, 191, 192, 193)] == [(1, 129, 8), (1, 130, 8), (1, 192, 8), (4, 49, 4), (4, 49, 4)]
    assert S(127, 2, 1, 0)[:3] == (1, 128, 4) and S(191, 1, 4, 0)[:3] == (1, 192, 4) and S(191, 2, 1, 0)[0] == 1 and S(192, 2, 1, 0)[0] == 4
    assert S(E.DECODE_LONG["pos"], E.DECODE_LONG["nkv"], 2, 0)[:2] == (32, 64) and S(E.DECODE_BOUND, 2, 2, 1)[:2] == (5, 61) and S(300, 1, 8, 1)[3] == 4
    for nh, nkv in E.HEADS:
        for hd in E.HEAD_DIMS:
            for pos0 in (0, E.FWD_POS0):
                for n in E.PER_TOKEN_N:
                    assert E.forward_route(hip, E.ATTN_PROMPT, nh, nkv, hd, n, 1, pos0) == E.ATTN_PER_TOKEN
                r = E.PER_TOKEN_REFUSED
                assert E.forward_route(hip, E.ATTN_PROMPT, nh, nkv, hd, r["n"], 1, pos0) == E.ATTN_TILE
                assert E.forward_route(hip, E.ATTN_PROMPT, nh, nkv, hd, r["n"], 1, pos0, q_stride=nh * hd + r["pad"]) == E.ATTN_PER_TOKEN
            for pos in (300, 511):
                nsp, chunk, _, _ = S(pos, nkv, nh // nkv, 0)
                ta = np.concatenate([E.decode_targets(pos, nh, chunk, sh)[0] for sh in range(0, E.DECODE_KINDS, nh)])
                tb = np.concatenate([E.decode_targets(pos, nh, chunk, sh)[1] for sh in range(0, E.DECODE_KINDS, nh)])
                assert len(ta) == E.DECODE_KINDS and nsp > 2
                assert (ta % chunk == 0).sum() >= 3 and (ta % chunk == chunk - 1).any() and 0 in ta and pos in ta and pos - 1 in ta
                two = tb >= 0
                assert two.sum() == 2 and (ta[two] // chunk != tb[two] // chunk).any() and (ta[two] % chunk == 0).any()
                assert all(bin(a ^ b).count("1") == 1 for a, b in zip(ta[two], tb[two]))


def kf_exp2_parts(y):
    """kf_device.h kf_exp2_parts on fp32 y: n = the nearest integer, f = 2^(y - n) from the degree-7 polynomial (each fma emulated in fp64 and rounded once more to fp32:
    the last bit of f may differ from the kernel's, which nothing below depends on)"""
    y = y.astype(F32)
    n = ((y + F32(12582912.0)).astype(F32) - F32(12582912.0)).astype(F32)
    r = (y - n).astype(F32)
    p = np.full(y.shape, F32(1.52527338e-5))
    for coef in (1.54035304e-4, 1.33335581e-3, 9.61812911e-3, 5.55041087e-2, 2.40226507e-1, 6.93147181e-1, 1.0):
        p = (p.astype(np.float64) * r.astype(np.float64) + np.float64(F32(coef))).astype(F32)
    return p, n


def _query_row(c, row):
    """per head, for query row `row` (position pos0 + row) of a case: raw q . k over the visible keys (exact integers in fp32), the bf16 score both orders take, the
    group's v [keys, hd], and which keys are the row's targets"""
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    GQ, ln = nh // nkv, c["pos0"] + row + 1
    rden = E.kernel_scale(hd)
    for h in range(nh):
        q = c["q"][row, h * hd:(h + 1) * hd]
        k = c["k"][:ln, (h // GQ) * hd:(h // GQ + 1) * hd]
        assert (np.abs(k) @ np.abs(q)).max() < 2.0 ** 24
        raw = (k @ q).astype(F32)
        on = np.zeros(ln, bool)
        on[c["ta"][0, row, h]] = True
        if c["tb"][0, row, h] >= 0:
            on[c["tb"][0, row, h]] = True
        yield h, raw, E.f64(E.bits((raw * rden).astype(F32))).astype(F32), c["v"][:ln, (h // GQ) * hd:(h // GQ + 1) * hd], on


def _canonical_out(s, v):
    """the canonical order on one head: weights f 2^(n - m) in fp64 (a shift below -1022 is clamped: canon_shift), fp64 sums, one conversion to fp32, one bf16 store"""
    f, n = kf_exp2_parts((s * LOG2E).astype(F32))
    w = np.ldexp(f.astype(np.float64), np.maximum(n - n.max(), -1022.0).astype(np.int64))
    return E.bits((w @ v / w.sum()).astype(F32)), w


def _both_orders(c, row, nsp, chunk, nw, what):
    """one query row through both orders' arithmetic -> (two-hot heads, slices that hold no target)"""
    hd = c["hd"]
    want = E.bits(E.closed_forward(c)[row])
    batch = 4 * nw * (64 // (hd // 8))
    n_two = n_without = 0
    for h, raw, s, v, on in _query_row(c, row):
        assert len(set(raw[on].tolist())) == 1 and len(set(s[on].tolist())) == 1, what                 # equal bit for bit
        assert ((s[on][0] - s[~on]) * LOG2E >= 150).all() if (~on).any() else True, what                # exp2 of <= -150 is 0.0f
        n_two += on.sum() == 2
        # fast order
        Ms, ls, Ps = [], [], []
        for sp in range(nsp):
            seg = s[None, sp * chunk:(sp + 1) * chunk]
            if seg.shape[1] == 0:
                continue   # a slice behind the position publishes a neutral partial: m = -inf, l = 0
            M, l, P = walk(seg, range(-(-seg.shape[1] // batch)), batch, LOG2E)
            Ms.append(M[0]), ls.append(l[0]), Ps.append(P[0])
            n_without += not on[sp * chunk:(sp + 1) * chunk].any()
        Mx = max(Ms)
        sc = [exp2f(np.asarray([(m - Mx) * LOG2E], F32))[0] for m in Ms]
        assert F32(sum(F32(l * a) for l, a in zip(ls, sc))) == on.sum(), what
        assert np.array_equal(np.concatenate([P * a for P, a in zip(Ps, sc)]), on.astype(F32)), what
        # canonical order
        got, w = _canonical_out(s, v)
        assert np.array_equal(got, want[h * hd:(h + 1) * hd]), what
        if (~on).any() and c["family"] == "code":
            assert (w[~on] > 0).all() and w[~on].max() / w[on][0] <= 2.0 ** -150, what                 # alive in fp64, gone after the two stores
    return n_two, n_without


def test_decode_probabilities_are_exact_in_both_orders(hip):
    """kf_attn.hip on the query row of every call tests/test_gpu_exact_attention_decode.py makes: the decode cases, the position below the bound, the per-token route.
    Both orders take score = bf16(fl32(q . k x fl32(1 / sqrt(hd)))); the two scores of a two-hot row are equal bit for bit, every other key's is lower by the gap.
    fast order:      per slice of `chunk` keys and batch of 4 x waves x (64 / (hd / 8)) keys a running maximum, p = exp2(fl32((s - M) log2 e)), slices merged with
                     exp2(fl32((M_slice - M) log2 e)): every target enters with exactly 1.0f, every other key and every slice without a target with exactly 0.0f
    canonical order: p = f 2^(n - m) from kf_exp2_parts(fl32(s log2 e)), fp64 sums: a non-target's weight of 2^-150 and less is NOT zero, but
                     bf16((float)(O / L)) is the closed form bit for bit -- because v > 0: on the [-2, 2] draw of the other modules the same emulation leaves -0.0
                     (0x8000) where the closed form is +0, the sign of what leaked"""
    n_two = n_without = 0
    for fam, pos, nh, nkv, hd, shift, nbits in _decode_cases():
        nsp, chunk, nw, _ = E.decode_slices(pos, nkv, nh // nkv, 0)
        c = E.decode_case(fam, pos, nh, nkv, hd, chunk, shift, nbits)
        a, b = _both_orders(c, pos, nsp, chunk, nw, (fam, pos, nh, hd, shift))
        n_two, n_without = n_two + a, n_without + b
        assert np.array_equal(c["want"], E.bits(E.closed_forward(c)[pos]))
        if pos in (0, 193, 511):   # (the oracle's two modes restate these orders: they agree with the closed form too)
            for mode in (O.ATTN_CANON, O.ATTN_FUSED):
                assert np.array_equal(O.attn_decode(E.exact_bits(c["q"][pos]), E.exact_bits(c["k"]), E.exact_bits(c["v"]), pos, nh, nkv, hd, mode=mode), c["want"])
    assert n_two > 50 and n_without > 1000
    for nh, nkv in E.HEADS:
        for hd in E.HEAD_DIMS:
            nsp, chunk, nw, _ = E.decode_slices(E.DECODE_BOUND, nkv, nh // nkv, 0)   # the slices of the bound; the keys of the position
            for fam in ("ramp", "code"):
                c = E.decode_case(fam, E.DECODE_BELOW, nh, nkv, hd, chunk, T=E.DECODE_BOUND + 1)
                _both_orders(c, E.DECODE_BELOW, nsp, chunk, nw, (fam, "below the bound", nh, hd))
                if fam == "ramp":   # every row behind the position scores above every visible key
                    q = c["q"][E.DECODE_BELOW, :hd]
                    sc = c["k"][:, :hd] @ q
                    assert sc[E.DECODE_BELOW + 1:].min() > sc[:E.DECODE_BELOW + 1].max()
                for pos0 in (0, E.FWD_POS0):
                    for n in E.PER_TOKEN_N + [E.PER_TOKEN_REFUSED["n"]]:
                        c = E.attn_case(fam, n, nh, nkv, hd, 1, pos0, seed=n + nh + hd, **E.DECODE_V)
                        for row in range(n):   # one slice per token: chunk = the launch's last position + 1
                            _both_orders(c, row, 1, pos0 + n, 8 if nh // nkv <= 2 and pos0 + n > 128 else 4, (fam, "per token", n, pos0, nh, hd))
    # the signed zero that v > 0 avoids
    c = E.attn_case("code", 301, 4, 2, 64, seed=7, vmax=2)
    neg = 0
    for h, raw, s, v, _ in _query_row(c, 300):
        got, _ = _canonical_out(s, v)
        want = E.bits(E.closed_forward(c)[300, h * 64:(h + 1) * 64])
        assert np.array_equal(E.f64(got), E.f64(want))
        neg += int(((got == 0x8000) & (want == 0)).sum())
    assert neg > 0
