"""Inputs whose arithmetic is EXACT in fp32 under every summation order, and their fp64 references (plain numpy, no GPU).

A bar scaled by a tensor's largest element cannot see one wrong term of a long contraction.  With operands made of small integers (and halves) every
product and every partial sum of a kernel's fp32 accumulation is representable, whatever the route, tile form, split-K cut or order, so the expected
output is bf16(exact) BIT FOR BIT and nothing is measured.  The groups:

  integer GEMM operands   entries in {-1, 0, 1} (optionally +-2) with the density chosen per contraction length, or a dense +-1 block of 128 consecutive
                          contraction indices placed on a seam of the form under test; small-integer prior values for the beta = 1 epilogues
  one-hot / two-hot attention   q, k built so that each row's softmax is exactly {1} or {1/2, 1/2} on chosen keys and exactly 0 elsewhere after the
                          kernels' own fp32 arithmetic (tests/test_exact_inputs_cpu.py emulates that arithmetic and asserts it)
  exact weights per storage   bf16, f8e5m2, 4-bit groups and row codebooks, ternary and 1-bit weights built from CHOSEN codes and CHOSEN (zero, step) tables that differ
                          from group to group, each dequantising to small integers: the forward token-batch GEMMs' operands, and their case table FORWARD_CASES
  level logits            the scoring head: integer logits, 128 on a row's winners and within +-40 elsewhere, so that every exponential of the log-softmax fold is exactly
                          0 or 1 and sum, maximum, first index and log-sum-exp are closed forms in every tile form, merge order and route (case table SCORE_CASES)

Every helper ASSERTS its precondition on the fp64 values it returns, so a badly chosen density or target pattern fails on the CPU, not on the GPU."""
import ctypes as C

import numpy as np

import attn_plan_mirror as APM
from oracle import oracle as O
from plan_structs import GemmMat as _Mat, GemmPlan as _Plan, GemmProblem as _Problem, ScorePlan as _ScorePlan, ScoreProblem as _ScoreProblem

BOUND = 256.0   # every integer of magnitude <= 256 is a bf16 value: the bf16 store of an exact result within the bound is that result


def bits(x):
    """fp64 / fp32 values -> bf16 bit patterns (round to nearest even)"""
    return O.f32_to_bf16(np.asarray(x, dtype=np.float32))


def exact_bits(x):
    """bf16 bit patterns of values that must BE bf16 values (operands, prior values)"""
    b = bits(x)
    assert np.array_equal(O.bf16_to_f32(b).astype(np.float64), np.asarray(x, dtype=np.float64)), "not representable in bf16"
    return b


def f64(b):
    return O.bf16_to_f32(b).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- integer GEMM operands
def density(K, second_moment=1.0):
    """non-zero fraction per operand for a contraction of length K: the sum of K products of two such entries has variance K d^2 m <= 400, so its maximum over
    a few million outputs (~5.5 sigma = 110) plus a prior value stays inside BOUND; at most 1/2"""
    return min(0.5, 20.0 / np.sqrt(K * second_moment))


def ternary(rng, shape, d, twos=False):
    """entries 0 with probability 1 - d, otherwise +-1 (twos: +-1 or +-2)"""
    mag = rng.integers(1, 3 if twos else 2, size=shape)
    return (np.where(rng.random(shape) < d, mag, 0) * rng.choice([-1, 1], size=shape)).astype(np.float64)


def small_ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def exact_product(a, b, prior=None, bound=BOUND):
    """fp64 a . b (+ prior): asserted to be integers within the bound, and with sum |terms| far below 2^24 -- so every partial sum in every order is an fp32 value"""
    y = a @ b
    if prior is not None:
        y = y + prior
    assert np.array_equal(y, np.rint(y)), "not an integer result"
    assert np.abs(y).max() <= bound, "exact result %g outside +-%g: lower the density" % (np.abs(y).max(), bound)
    assert a.shape[1] * np.abs(a).max() * np.abs(b).max() + (0 if prior is None else np.abs(prior).max()) < 2.0 ** 23
    return y


def block_rows(K, at, width=128):
    """the contraction indices of a dense block placed astride index `at` (first / last tile: clipped into [0, K))"""
    lo = min(max(at - width // 2, 0), K - width)
    return np.arange(lo, lo + width)


def linear_backward_case(OC, IC, n, family, seed, oc_blocks=(), n_blocks=(), twos=False, w=None):
    """operands and exact results of kf_linear_backward for W [OC, IC], deltaIn [n, OC], inp [n, IC]:
         delta [n, IC] = (prior) + deltaIn . W    (contraction over OC)        gW [OC, IC] = prior + deltaIn^T . inp   (contraction over n)
         gBias [OC] = prior + column sums of deltaIn
    family "sparse": random {-1, 0, 1} entries at density(K) of each contraction.
    family "block":  dense +-1 blocks of 128 contraction indices, zero elsewhere.  oc_blocks / n_blocks: the positions `at` (block_rows) along OC / n.  Token row t
                     multiplies block t mod len(oc_blocks) in the input gradient, output column o block o mod len(n_blocks) in the weight gradient, so one call
                     puts a 128-term dense sum on every listed seam.
    w: a given weight (fp64 integers [OC, IC]) instead of the family's."""
    rng = np.random.default_rng(seed)
    if family == "sparse":
        W = ternary(rng, (OC, IC), density(OC, 2.5 if twos else 1.0), twos) if w is None else w
        dIn = ternary(rng, (n, OC), min(density(OC), density(n)))
        inp = ternary(rng, (n, IC), density(n))
        kx, kw = slice(None), slice(None)
    else:
        assert family == "block" and len(oc_blocks) and len(n_blocks) and w is None
        ocb = [block_rows(OC, a) for a in oc_blocks]
        nb = [block_rows(n, a) for a in n_blocks]
        u_oc, u_n = np.unique(np.concatenate(ocb)), np.unique(np.concatenate(nb))
        A = np.zeros((n, OC), bool)   # row t: its block along OC
        for j, blk in enumerate(ocb):
            A[j::len(ocb), blk[0]:blk[-1] + 1] = True
        B = np.zeros((n, OC), bool)   # column o: its block along n
        for j, blk in enumerate(nb):
            B[blk[0]:blk[-1] + 1, j::len(nb)] = True
        both = np.zeros((n, OC), bool)
        both[np.ix_(u_n, u_oc)] = True
        mask = np.where(both, A, A | B)   # where the two unions cross, the row's rule alone: a token row never multiplies more than its own block
        dIn = np.where(mask, rng.choice([-1.0, 1.0], size=(n, OC)), 0.0)
        W = np.zeros((OC, IC))
        W[u_oc] = rng.choice([-1.0, 1.0], size=(len(u_oc), IC))
        inp = np.zeros((n, IC))
        inp[u_n] = rng.choice([-1.0, 1.0], size=(len(u_n), IC))
        kx, kw = u_oc, u_n   # the only contraction indices with a non-zero factor: the fp64 products below need no more
    delta0, gW0, gb0 = small_ints(rng, (n, IC)), small_ints(rng, (OC, IC)), small_ints(rng, OC)
    delta = exact_product(dIn[:, kx], W[kx], None)
    delta_acc = exact_product(dIn[:, kx], W[kx], delta0)
    gW = exact_product(np.ascontiguousarray(dIn[kw].T), inp[kw], gW0)
    gb = dIn.sum(axis=0) + gb0
    assert np.abs(gb).max() <= BOUND
    return dict(OC=OC, IC=IC, n=n, W=exact_bits(W), dIn=exact_bits(dIn), inp=exact_bits(inp), delta0=exact_bits(delta0), gW0=exact_bits(gW0), gb0=exact_bits(gb0),
                delta=exact_bits(delta), delta_acc=exact_bits(delta_acc), gW=exact_bits(gW), gb=exact_bits(gb),
                f64=dict(W=W, dIn=dIn, inp=inp, delta0=delta0, gW0=gW0, kx=kx, kw=kw))


def q4_grid_weight(OC, IC, seed):
    """a 4-bit weight that its own storage holds exactly: every 128-element group contains one -7 and one 8, so RTN's step is (8 - -7) / 15 = 1 and its zero -7, and the
    other entries are integers of the grid ({-1, 0, 1} mostly, so that the products stay inside BOUND).  Asserted against the oracle: dequant(quantize(w)) == w."""
    rng = np.random.default_rng(seed)
    w = ternary(rng, (OC * IC // 128, 128), density(OC, 2.0))
    at = np.argsort(rng.random(w.shape), axis=1)[:, :2]   # two distinct places per group (a fixed column would line the -7s up in one output)
    np.put_along_axis(w, at[:, :1], -7.0, axis=1)
    np.put_along_axis(w, at[:, 1:], 8.0, axis=1)
    w = w.reshape(OC, IC)
    ow = O.quantize(exact_bits(w), OC, IC, O.Q4)
    assert np.array_equal(O.dequant(ow), exact_bits(w)), "the 4-bit grid does not hold the weight exactly"
    return w, ow


# ---- the plan behind kf_linear_backward (kf_gemm_plan.h gemm_plan_backward through kfdbg_gemm_plan): which form a case runs, and where its k pieces meet
BF16_T, BWD_DX, BWD_DW = 3, 4, 5
ROUTES = {11: "KMAJOR", 12: "TRANSPOSE"}
FAMILIES = {0: "NONE", 1: "DIRECT", 2: "PAIRED", 3: "STAGED", 4: "G2", 5: "G3"}
G3_FORMS = {0: "BIG", 1: "SMALL", 2: "MID", 3: "TINY", 4: "WIDE"}


def _up256(v):
    return (v + 255) & ~255


def backward_plan(hip, entry, OC, IC, n):
    """the plan kf_linear_backward makes for this product: the scratch it lends is the middle region of kf_linear_backward_scratch_bytes"""
    hip.kfdbg_gemm_plan.argtypes = [C.POINTER(_Problem), C.POINTER(_Plan)]
    hip.kf_linear_backward_scratch_bytes.argtypes, hip.kf_linear_backward_scratch_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_size_t
    mid = hip.kf_linear_backward_scratch_bytes(OC, IC, n) - _up256(OC * IC * 2) - _up256((n + 255) // 256 * OC * 8)
    P = _Problem(entry=entry, n_w=1, n=n, x_al=1, scratch=mid)
    P.w[0] = _Mat(BF16_T, 0, 0, OC, IC, 0, 0, 3)
    out = _Plan()
    assert hip.kfdbg_gemm_plan(C.byref(P), C.byref(out)) == 0
    return out


def form_name(p):
    """"KMAJOR/BIG/plain", "KMAJOR/SMALL/split" (S >= 2 pieces), "KMAJOR/BIG/tails" (kp > 0: owners + helpers), "TRANSPOSE/DIRECT", "TRANSPOSE/G3_TINY", ..."""
    route, k = ROUTES[p.route], p.k
    if route == "KMAJOR":
        cut = "plain" if not k.sk else ("split" if k.S >= 2 else "tails")
        return "KMAJOR/%s/%s" % (G3_FORMS[k.form], cut)
    fam = FAMILIES[k.fam]
    return "TRANSPOSE/" + (fam if fam != "G3" else "G3_%s%s" % (G3_FORMS[k.form], "/split" if k.sk else ""))


def seams(p, K):
    """the contraction indices at which two workgroups' k pieces of one output tile meet (kf_gemm3.hip gemm3_sk_kernel): between the S equal pieces; or the
    owner / helper hand-over 64 kp and the cuts between two helpers' ranges of R steps inside the first tiles' tails.  Always with the first and the last k tile."""
    at = [0, K]
    k = p.k
    if k.sk:
        nkt = K // 64
        if k.S >= 2:
            at += [64 * (nkt * sp // k.S) for sp in range(1, k.S)]
        else:
            at.append(64 * k.kp)
            L = nkt - k.kp   # the tails [kp, nkt) of all tiles laid end to end are cut every R steps: the cuts that fall inside the first four tiles' tails
            at += [64 * (k.kp + b - t * L) for t in range(min(k.P, 4)) for b in range(0, k.P * L, k.R) if t * L < b < (t + 1) * L]
    return sorted(set(at))


# ---- the plan behind the attention entries (kf_attn_plan.h attn_plan through kfdbg_attn_plan): the forward's tile form or its paired form
ATTN_DECODE, ATTN_PROMPT, ATTN_BATCH = APM.DECODE, APM.PROMPT, APM.BATCH   # AttnProblem::entry: kf_attn_decode, kf_attn_prefill, kf_attn_prefill_batch(_strided)
ATTN_SLICED, ATTN_PER_TOKEN, ATTN_TILE, ATTN_PAIRED = APM.SLICED, APM.PER_TOKEN, APM.TILE, APM.PAIRED   # AttnPlan::route


def attn_plan(hip, entry, nh, nkv, hd, n, n_seq=1, pos0=0, canon=0, q_stride=None):
    """the plan of a forward launch with aligned rows (dense unless q_stride is given)"""
    out = APM.plan(hip, entry, nh, nkv, hd, pos0, n, n_seq, canon, q_stride=q_stride)
    assert out.status == 0
    return out


def forward_route(hip, entry, nh, nkv, hd, n, n_seq=1, pos0=0, q_stride=None):
    """the route of a forward launch with aligned rows (dense unless q_stride is given)"""
    return attn_plan(hip, entry, nh, nkv, hd, n, n_seq, pos0, 0, q_stride).route


# ---------------------------------------------------------------------------------------------------------------- one-hot / two-hot attention
NBITS = 9   # code words for up to 512 keys
GAP_LOG2 = 160.0   # two scores that differ differ by at least this many powers of two: exp2 of the difference is exactly 0.0f (fp32's smallest subnormal is 2^-149)
RAMP_G = 2048.0


GAIN_MAX = {9: 64.0, 11: 128.0}   # the largest q x k gain per code width (code_gains)


def code_gains(hd, nbits=NBITS):
    """(gq, gk, rep): q = gq x code, k = gk x code, every code bit repeated rep times.  Two distinct keys differ in >= 1 bit, i.e. by >= 2 rep gq gk in the raw score,
    times scale log2(e) in the exponent: gq gk is the smallest power of two that makes that >= GAP_LOG2.  The gain sits mostly in k so that dk's accumulators (sums of
    dS x q over many rows) stay small.  The bound on the gain: 64 at 9 bits, where the backward's accumulators carry it; 128 at 11 bits (head_dim 64 repeats a bit
    only 5 times), which only forward cases use -- there the gain enters nothing but the score, an integer below 2^24 (asserted), and k = gk x +-1 stays a bf16 integer."""
    rep = hd // nbits
    need = GAP_LOG2 / (2 * rep * np.log2(np.e) / np.sqrt(hd))
    g = 2.0 ** np.ceil(np.log2(need))
    assert g <= GAIN_MAX[nbits] and g * nbits * rep < 2.0 ** 24
    return 2.0, g / 2.0, rep


def codes(keys, hd, mask, nbits=NBITS):
    """+-1 code words of (key ^ mask), each of the nbits bits repeated rep times, the remaining head_dim - nbits rep entries 0"""
    rep = hd // nbits
    b = ((np.asarray(keys)[:, None] ^ mask) >> np.arange(nbits)[None, :]) & 1
    c = np.zeros((len(keys), hd))
    c[:, :nbits * rep] = np.repeat(2.0 * b - 1.0, rep, axis=1)
    return c


def code_targets(T, pos0, nh, seq):
    """the key(s) each (row, head) puts its whole probability on: ta [T, nh], tb [T, nh] (-1: one-hot).  Kinds, dealt over rows and heads: the diagonal; key 0 (one
    row in four of its turn: every row that names key 0 adds to dk[0]); key p - 1; the first key of p's 32-key tile, the last and the first key of the tile before
    it; the keys on either side of a multiple of 128; and two-hot {a, a - lowest set bit of a} on the next kind's key a.  A kind that does not exist for a row (no
    earlier tile, p < 128, ...) falls back to the diagonal, which also covers the last key of the row's own tile (rows with p % 32 == 31) and the ragged last rows."""
    ta = np.zeros((T, nh), np.int64)
    tb = np.full((T, nh), -1, np.int64)

    def one(kind, i, p):
        t32 = p // 32 * 32
        if kind == 1:
            return 0 if i % 4 == 0 else p
        if kind == 2:
            return p - 1
        if kind == 3:
            return t32
        if kind == 4:
            return t32 - 1
        if kind == 5:
            return t32 - 32
        if kind in (6, 7) and p >= 128:
            return 128 * (1 + i % (p // 128)) - (kind == 6)
        return p
    for i in range(T):
        p = pos0 + i
        for h in range(nh):
            kind = (i + 3 * h + seq) % 9
            a = one(kind if kind < 8 else (i // 9 + h) % 8, i, p)
            a = a if 0 <= a <= p else p
            ta[i, h] = a
            if kind == 8 and a > 0:
                tb[i, h] = a - (a & -a)
    return ta, tb


def attn_case(family, T, nh, nkv, hd, n_seq=1, pos0=0, seed=0, vmax=1, vmin=None, nbits=NBITS, last=None):
    """q [n_seq T, nh hd], k / v [n_seq (pos0 + T), nkv hd], o / dO [n_seq T, nh hd] as fp64 small integers (each a bf16 value), and the targets ta / tb [n_seq, T, nh].
    family "code": k_j = gk x the code word of j (a different bit mask per kv head and sequence), q_i = gq x the code of the target, or gq / 2 x the sum of two codes
                   one bit apart -- the two scores are then equal and every other key's is lower by >= the gap.
    family "ramp": score(i, j) = RAMP_G (j - p_i): k_j = (hi, lo, 1, 1, 0 ...) with j = 16 hi + lo, q_i = RAMP_G (16, 1, -16 hi_p, -lo_p, 0 ...).  The diagonal scores 0 and
                   is the visible maximum; EVERY masked future key scores higher than any visible one, so one future key admitted takes the whole row.
    o is NOT the forward's output: the backward takes it as an input, D = dO . o is an arbitrary integer.
    vmin: v in [vmin, vmax] instead of [-vmax, vmax] (the decode kernels' cases: v > 0, see decode_case); nbits: the code width, 2^nbits keys at the most;
    last = (ta [nh], tb [nh]): the code family's targets of the LAST row of every sequence, instead of code_targets' (decode_targets)."""
    assert family in ("code", "ramp") and pos0 + T <= 1 << nbits and nh % nkv == 0
    rng = np.random.default_rng(seed)
    GQ, tot = nh // nkv, pos0 + T
    q, k = np.zeros((n_seq * T, nh * hd)), np.zeros((n_seq * tot, nkv * hd))
    ta, tb = np.zeros((n_seq, T, nh), np.int64), np.full((n_seq, T, nh), -1, np.int64)
    gq, gk, _ = code_gains(hd, nbits)
    for s in range(n_seq):
        if family == "code":
            ta[s], tb[s] = code_targets(T, pos0, nh, s)
            if last is not None:
                ta[s, T - 1], tb[s, T - 1] = last
        else:
            ta[s] = (pos0 + np.arange(T))[:, None]
        for g in range(nkv):
            cols = slice(g * hd, (g + 1) * hd)
            if family == "code":
                mask = (37 * g + 73 * s + 11) & ((1 << nbits) - 1)
                k[s * tot:(s + 1) * tot, cols] = gk * codes(np.arange(tot), hd, mask, nbits)
            else:
                j = np.arange(tot)
                k[s * tot:(s + 1) * tot, g * hd + 0], k[s * tot:(s + 1) * tot, g * hd + 1] = j // 16, j % 16
                k[s * tot:(s + 1) * tot, g * hd + 2], k[s * tot:(s + 1) * tot, g * hd + 3] = 1.0, 1.0
            for h in range(g * GQ, (g + 1) * GQ):
                hc = slice(h * hd, (h + 1) * hd)
                if family == "code":
                    ca = codes(ta[s, :, h], hd, mask, nbits)
                    two = tb[s, :, h] >= 0
                    cb = codes(np.where(two, tb[s, :, h], 0), hd, mask, nbits)
                    q[s * T:(s + 1) * T, hc] = np.where(two[:, None], gq / 2 * (ca + cb), gq * ca)
                else:
                    p = pos0 + np.arange(T)
                    q[s * T:(s + 1) * T, h * hd + 0], q[s * T:(s + 1) * T, h * hd + 1] = 16 * RAMP_G, RAMP_G
                    q[s * T:(s + 1) * T, h * hd + 2], q[s * T:(s + 1) * T, h * hd + 3] = -16 * RAMP_G * (p // 16), -RAMP_G * (p % 16)
    v = rng.integers(-vmax if vmin is None else vmin, vmax + 1, size=(n_seq * tot, nkv * hd)).astype(np.float64)
    o = rng.integers(-1, 2, size=(n_seq * T, nh * hd)).astype(np.float64)
    dO = np.zeros((n_seq * T, nh, hd))
    for _ in range(2):   # two +-1 entries per (row, head) (where the two places coincide the row has one)
        idx = rng.integers(0, hd, size=(n_seq * T, nh))
        np.put_along_axis(dO, idx[:, :, None], rng.choice([-1.0, 1.0], size=(n_seq * T, nh, 1)), axis=2)
    dO = dO.reshape(n_seq * T, nh * hd)
    for a in (q, k, v, o, dO):
        exact_bits(a)
    return dict(family=family, T=T, nh=nh, nkv=nkv, hd=hd, n_seq=n_seq, pos0=pos0, tot=tot, q=q, k=k, v=v, o=o, dO=dO, ta=ta, tb=tb)


def kernel_scale(hd):
    """1.0f / sqrtf((float)hd), as the launchers compute it"""
    return np.float32(1.0) / np.sqrt(np.float32(hd))


def closed_forward(c):
    """out_i = bf16(v_a) or bf16((v_a + v_b) / 2): fp64 [n_seq T, nh hd]"""
    T, nh, nkv, hd, tot = c["T"], c["nh"], c["nkv"], c["hd"], c["tot"]
    GQ = nh // nkv
    out = np.zeros((c["n_seq"] * T, nh * hd))
    for s in range(c["n_seq"]):
        for h in range(nh):
            vg = c["v"][s * tot:(s + 1) * tot, (h // GQ) * hd:(h // GQ + 1) * hd]
            a, b = c["ta"][s, :, h], c["tb"][s, :, h]
            out[s * T:(s + 1) * T, h * hd:(h + 1) * hd] = np.where((b >= 0)[:, None], (vg[a] + vg[np.maximum(b, 0)]) / 2, vg[a])
    return out


def closed_backward(c, ta=None, tb=None, check=True):
    """the backward in closed form: per (row i, head h) the probability w = 1 or 1/2 sits on the target key(s) x; dP_x = dO_i . v_x, D = dO_i . o_i,
         dS_x = w (dP_x - D)       dq_i = sum_x dS_x k_x       dk_x += dS_x q_i       dv_x += w dO_i        (dk, dv: summed over the rows AND the group's heads)
    -> bit patterns of dq = bf16(fl32(acc) fl32(scale)), dk likewise, dv = bf16(acc), and the fp64 accumulators.  check: every accumulator is a multiple of 1/2 of magnitude
    <= BOUND, and its terms' magnitudes sum to < 2^23 halves, so every partial sum in every order is an fp32 value.  One exception, by construction: the ramp's q is
    RAMP_G times integers up to 16 x 31 (nothing smaller separates neighbouring keys by the gap), so ITS dk accumulators are multiples of RAMP_G, held to the same
    count of units; each has one term per head of the group."""
    assert c["pos0"] == 0
    T, nh, nkv, hd = c["T"], c["nh"], c["nkv"], c["hd"]
    GQ = nh // nkv
    ta = c["ta"] if ta is None else ta
    tb = c["tb"] if tb is None else tb
    rows = c["n_seq"] * T
    dq, dk, dv = np.zeros((rows, nh * hd)), np.zeros((rows, nkv * hd)), np.zeros((rows, nkv * hd))
    adq, adk, adv = np.zeros_like(dq), np.zeros_like(dk), np.zeros_like(dv)   # sums of |terms|
    for s in range(c["n_seq"]):
        r0 = s * T
        for h in range(nh):
            hc, gc = slice(h * hd, (h + 1) * hd), slice((h // GQ) * hd, (h // GQ + 1) * hd)
            qh, dOh, oh = c["q"][r0:r0 + T, hc], c["dO"][r0:r0 + T, hc], c["o"][r0:r0 + T, hc]
            kg, vg = c["k"][r0:r0 + T, gc], c["v"][r0:r0 + T, gc]
            D = (dOh * oh).sum(axis=1)
            two = tb[s, :, h] >= 0
            for x, on in ((ta[s, :, h], np.ones(T, bool)), (np.maximum(tb[s, :, h], 0), two)):
                w = np.where(two, 0.5, 1.0) * on
                dS = w * ((dOh * vg[x]).sum(axis=1) - D)
                dq[r0:r0 + T, hc] += dS[:, None] * kg[x]
                adq[r0:r0 + T, hc] += np.abs(dS[:, None] * kg[x])
                np.add.at(dk[r0:r0 + T, gc], x, dS[:, None] * qh)
                np.add.at(adk[r0:r0 + T, gc], x, np.abs(dS[:, None] * qh))
                np.add.at(dv[r0:r0 + T, gc], x, w[:, None] * dOh)
                np.add.at(adv[r0:r0 + T, gc], x, np.abs(w[:, None] * dOh))
    if check:
        for name, a, aa in (("dq", dq, adq), ("dk", dk, adk), ("dv", dv, adv)):
            unit = RAMP_G if (c["family"], name) == ("ramp", "dk") else 0.5
            assert np.array_equal(a / unit, np.rint(a / unit)), name
            assert aa.max() / unit < 2.0 ** 23, name
            if unit == 0.5:
                assert np.abs(a).max() <= BOUND, "%s accumulator %g outside +-%g" % (name, np.abs(a).max(), BOUND)
    sc = kernel_scale(hd)
    return dict(dq=bits(dq.astype(np.float32) * sc), dk=bits(dk.astype(np.float32) * sc), dv=bits(dv), acc=dict(dq=dq, dk=dk, dv=dv))


# ---- plain fp64 references of the same operations (one sequence): the closed forms are compared with them on the CPU, and attn_backward_ref with the oracle
def attn_forward_ref(q, k, v, nh, nkv, hd, pos0=0):
    """causal softmax attention in fp64: q [T, nh hd], k / v [pos0 + T, nkv hd] -> out fp64 [T, nh hd]"""
    T, GQ = q.shape[0], nh // nkv
    vis = np.arange(pos0 + T)[None, :] <= (pos0 + np.arange(T))[:, None]
    out = np.zeros((T, nh * hd))
    for h in range(nh):
        gc = slice((h // GQ) * hd, (h // GQ + 1) * hd)
        s = np.where(vis, q[:, h * hd:(h + 1) * hd] @ k[:, gc].T / np.sqrt(float(hd)), -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h * hd:(h + 1) * hd] = (p / p.sum(axis=1, keepdims=True)) @ v[:, gc]
    return out


def attn_backward_ref(q, k, v, o, dO, nh, nkv, hd, vis=None, round_p=False):
    """causal attention backward in fp64 from fp64 copies of the bf16 inputs; the one fp32 multiply by fl32(1 / sqrt(hd)) and the bf16 stores as the kernels make them:
    dq = bf16(fl32(sum dS k) fl32(scale)), dk likewise with the sum over the group's heads, dv = bf16(sum P dO).  vis [T, T]: the mask (default: causal) -- the
    mutation checks pass a wrong one.  round_p: P and dS rounded to bf16 before their products, the kernels' two rounding points.  -> bit patterns + accumulators"""
    T, GQ = q.shape[0], nh // nkv
    vis = np.tril(np.ones((T, T), bool)) if vis is None else vis
    rb = (lambda a: f64(bits(a))) if round_p else (lambda a: a)
    dq, dk, dv = np.zeros((T, nh * hd)), np.zeros((T, nkv * hd)), np.zeros((T, nkv * hd))
    for h in range(nh):
        hc, gc = slice(h * hd, (h + 1) * hd), slice((h // GQ) * hd, (h // GQ + 1) * hd)
        s = np.where(vis, q[:, hc] @ k[:, gc].T / np.sqrt(float(hd)), -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        dS = p * (dO[:, hc] @ v[:, gc].T - (dO[:, hc] * o[:, hc]).sum(axis=1, keepdims=True))
        dq[:, hc] = rb(dS) @ k[:, gc]
        dk[:, gc] += rb(dS).T @ q[:, hc]
        dv[:, gc] += rb(p).T @ dO[:, hc]
    sc = kernel_scale(hd)
    return dict(dq=bits(dq.astype(np.float32) * sc), dk=bits(dk.astype(np.float32) * sc), dv=bits(dv), acc=dict(dq=dq, dk=dk, dv=dv))


# ---------------------------------------------------------------------------------------------------------------- the cases the GPU modules run
# kf_linear_backward (OC, IC, n) -> the forms of its two products (input gradient, weight gradient), as kf_gemm_plan.h plans them; pinned by
# tests/test_exact_inputs_cpu.py.  The smallest shapes that reach each form: K-major needs IC and the token side >= 256, a split needs a contraction >= 1024.  No
# shape with every side <= 2048 reaches a 256 x 256 (BIG) tile or an owner / helper cut (the CPU module enumerates them all), so those six go past it.
LINEAR_CASES = {
    (128, 128, 128): ("TRANSPOSE/DIRECT", "TRANSPOSE/DIRECT"),
    (256, 256, 256): ("KMAJOR/SMALL/plain", "KMAJOR/SMALL/plain"),
    (1024, 256, 1024): ("KMAJOR/SMALL/split", "KMAJOR/SMALL/split"),
    (2048, 136, 2048): ("TRANSPOSE/G3_TINY", "TRANSPOSE/G3_TINY"),          # IC 136: a ragged last tile of 8 rows
    (2048, 2176, 2048): ("KMAJOR/SMALL/tails", "KMAJOR/SMALL/tails"),
    (512, 4096, 1600): ("KMAJOR/BIG/plain", "KMAJOR/SMALL/split"),          # 1600 = 6.25 big tiles; a 512-deep contraction is not cut
    (1600, 4096, 512): ("KMAJOR/SMALL/split", "KMAJOR/BIG/plain"),
    (1408, 4800, 1408): ("KMAJOR/BIG/split", "KMAJOR/BIG/split"),           # 19 x 6 = 114 ragged big tiles in two pieces
    (2176, 3968, 2176): ("KMAJOR/BIG/tails", "KMAJOR/BIG/tails"),           # 16 x 9 = 144 tiles: owners + 112 helpers
}
Q4_CASE = (1024, 256, 1024)


def linear_case(hip, shape, family, **kw):
    """the case of LINEAR_CASES[shape]: the block family's blocks sit on the seams of the two plans"""
    OC, IC, n = shape
    if family == "block":
        kw.update(oc_blocks=seams(backward_plan(hip, BWD_DX, OC, IC, n), OC), n_blocks=seams(backward_plan(hip, BWD_DW, OC, IC, n), n))
    return linear_backward_case(OC, IC, n, family, seed=OC + 3 * IC + 7 * n + len(family), **kw)


# attention: (n_head, n_kv) for GQ 1, 2, 4, 8
HEADS = [(2, 2), (4, 2), (4, 1), (8, 1)]
HEAD_DIMS = [64, 128]
FWD_N = [8, 31, 32, 33, 127, 128, 129, 160, 257]   # 257 tokens of these head counts make few workgroups: the plan pairs them (ATTN_PAIRED)
FWD_TILE_LONG = dict(n=257, nh=64, nkv=8, hd=64, n_seq=3)   # and the unpaired tile form past 256 tokens: 17 x 8 x 3 = 408 workgroups > 320
FWD_POS0 = 37       # kf_attn_prefill behind a prefix of cache rows
BWD_T = [8, 31, 33, 64, 129, 257, 300]
N_SEQ = [1, 3]


# ---------------------------------------------------------------------------------------------------------------- forward token-batch GEMMs: exact weights per storage
# storage name -> (kf type, row codebook, symmetric range (qBias 8), group size)
STORAGES = {
    "bf16": (O.BF16, False, False, 128), "f8": (O.F8E5M2, False, False, 128),
    "q4": (O.Q4, False, False, 128), "q4s": (O.Q4, False, True, 128), "q4g64": (O.Q4, False, False, 64), "q4sg64": (O.Q4, False, True, 64), "q4g256": (O.Q4, False, False, 256),
    "tern": (O.T_SIGN, False, False, 128), "bool1": (O.BOOL1, False, False, 128), "tbin": (O.T_BINARY, False, False, 128), "bool1g256": (O.BOOL1, False, False, 256),
    "lut": (O.Q4, True, False, 0),
}
# (lowest code, highest code, codes that may dequantise to 0, qBias): the code q' of an element is what the stream holds minus qBias
_RANGES = {(O.Q4, False): (0, 15, (2, 5), 0), (O.Q4, True): (-8, 7, (-3, 3), 8), (O.T_SIGN, False): (-1, 1, (-1, 1), 1), (O.BOOL1, False): (0, 1, (0, 1), 0),
           (O.T_BINARY, False): (0, 1, (0, 1), 0)}


def _group_weight(rng, type_, symmetric, lgroup, M, K, d, signs, edit=None):
    """a group-quantised weight built from CHOSEN codes and CHOSEN (zero, step) tables: group g has step s_g in {1, 2} and zero s_g q0_g, so code q' dequantises to
    s_g (q' - q0_g), an integer, and q0_g to 0.  (s, q0) is drawn per group and never equals the previous group's: two distinct maps q' -> s q' - zero agree on at
    most one code and every group holds at least two (sparse family), so a table read at the neighbouring group's index changes an integer.
    sparse (signs None): a fraction d of the entries holds another code -- 4-bit: q0 +- 1, q0 +- 2; ternary / 1-bit: one of the other codes of the range -- and, 4-bit,
    one entry per group ANY code of the range (all 16 nibbles occur).  signs [M, K] in {-1, 0, 1}: code q0 + sign (4-bit only).
    edit(q, q0, step) -> q, all [M, K] integers: the caller's last word on the codes q' (the level family plants its channels), held to the same range."""
    lo, hi, (z_lo, z_hi), qbias = _RANGES[(type_, symmetric)]
    nG = M * K // lgroup
    combos = np.array([(s, q) for s in (1, 2) for q in range(z_lo, z_hi + 1)])
    idx = (rng.integers(0, len(combos)) + np.concatenate([[0], np.cumsum(rng.integers(1, len(combos), size=nG - 1))])) % len(combos)
    assert (idx[1:] != idx[:-1]).all()
    step, q0 = combos[idx, 0][:, None], combos[idx, 1][:, None]
    if signs is not None:
        assert hi - lo == 15
        q = q0 + signs.reshape(nG, lgroup).astype(np.int64)
    else:
        on = rng.random((nG, lgroup)) < d
        on[np.arange(nG), rng.integers(0, lgroup, size=nG)] = True   # at least two distinct codes per group
        if hi - lo == 15:
            other = q0 + rng.choice([-2, -1, 1, 2], size=(nG, lgroup))
        else:
            other = lo + (q0 - lo + rng.integers(1, hi - lo + 1, size=(nG, lgroup))) % (hi - lo + 1)
        q = np.where(on, other, q0)
        if hi - lo == 15:
            q[np.arange(nG), rng.integers(0, lgroup, size=nG)] = rng.integers(lo, hi + 1, size=nG)
        assert (q.min(axis=1) != q.max(axis=1)).all()
    if edit is not None:
        q = edit(q.reshape(M, K), np.broadcast_to(q0, q.shape).reshape(M, K), np.broadcast_to(step, q.shape).reshape(M, K)).reshape(nG, lgroup)
    assert q.min() >= lo and q.max() <= hi
    W = (step * (q - q0)).astype(np.float64).reshape(M, K)
    ow = O.QWeight(type_, M, K, O.pack(q + qbias, O.BITS[type_]), exact_bits(step * q0).reshape(-1), exact_bits(step).reshape(-1), lgroup, qbias)
    return W, ow


def _lut_weight(rng, M, K, d):
    """4-bit row codebook: row r's table is its own permutation of -8 .. 7 (neighbouring rows differ); an entry is 0 with probability 1 - d, else +-1 or +-2, and one
    entry in 128 holds any of the 16 codes; the stream is MSB first, element 2 i in the high nibble of byte i"""
    table = np.stack([rng.permutation(16) - 8 for _ in range(M)])
    for r in np.nonzero((table[1:] == table[:-1]).all(axis=1))[0]:
        table[r + 1] = np.roll(table[r + 1], 1)
    assert not (table[1:] == table[:-1]).all(axis=1).any()
    W = ternary(rng, (M, K), d, twos=True)
    any_code = rng.random((M, K)) < 1.0 / 128
    W = np.where(any_code, rng.integers(-8, 8, size=(M, K)), W)
    code = np.argsort(table, axis=1)[np.arange(M)[:, None], W.astype(np.int64) + 8]   # the place of value v in the row's table
    assert np.array_equal(np.take_along_axis(table, code, axis=1), W)
    data = (code[:, 0::2] << 4 | code[:, 1::2]).astype(np.uint8)
    return W, O.LutWeight(M, K, data, exact_bits(table), 4)


def exact_weight(storage, M, K, seed, signs=None, d=None, edit=None):
    """(W fp64 integers [M, K], the oracle weight that holds exactly W) for every storage the tile kernels unpack (STORAGES).  d: the fraction of non-zero entries
    (default density(K) on the second moment of the storage's non-zero values); signs [M, K] in {-1, 0, 1}: the block family's pattern -- bf16, f8 and the row codebook
    hold it as it is, a 4-bit group g holds s_g x signs.  edit(q, q0, step) -> q: see _group_weight; bf16 and f8 pass the values themselves with q0 = 0, step = 1.
    Asserted on the CPU: O.dequant(ow) == W."""
    type_, row_lut, symmetric, lgroup = STORAGES[storage]
    rng = np.random.default_rng(seed)
    if row_lut:
        assert signs is None and edit is None
        W, ow = _lut_weight(rng, M, K, density(K, 2.5) if d is None else d)
    elif type_ in (O.BF16, O.F8E5M2):
        W = ternary(rng, (M, K), density(K, 2.5) if d is None else d, twos=True) if signs is None else signs.astype(np.float64)
        if edit is not None:
            W = edit(W.astype(np.int64), np.zeros((M, K), np.int64), np.ones((M, K), np.int64)).astype(np.float64)
        # (bf16 has no groups: the weight as O.quantize returns it, without its whole-groups precondition -- the level family's vocabulary is odd)
        ow = O.QWeight(O.BF16, M, K, exact_bits(W).reshape(-1)) if type_ == O.BF16 else O.quantize(exact_bits(W), M, K, type_)
    else:
        assert K % lgroup == 0 or lgroup % K == 0
        m = {15: 2.5 * 2.5, 2: 2.5 * 2.5, 1: 2.5}[_RANGES[(type_, symmetric)][1] - _RANGES[(type_, symmetric)][0]]   # E[s^2] = 2.5 times E[(q' - q0)^2]
        W, ow = _group_weight(rng, type_, symmetric, lgroup, M, K, density(K, m) if d is None else d, signs, edit)
    assert np.array_equal(O.dequant(ow), exact_bits(W)), "storage %s does not hold the weight exactly" % storage
    return W, ow


ALPHA, BETA = 0.5, 2.0   # the epilogue case


def linear_forward_case(M, K, n, storage, seed, family="sparse", at=(), epilogue=False):
    """operands and exact results of y [n, M] = x [n, K] . W^T, everything in fp64:
    family "sparse": W by exact_weight, x random {-1, 0, 1} at the density that keeps the sum of K products' variance K d_x mean(W^2) <= 400 (density()'s bound)
    family "block":  dense +-1 blocks of 128 contraction indices at the positions `at` (block_rows): W is +-1 (4-bit group g: +-s_g) on the union of the blocks' columns
                     and 0 elsewhere, token row t is +-1 on block t mod len(at) and 0 elsewhere -- every output is a 128-term dense sum, one per listed seam
    epilogue: also y0, bias [M], residual (small integers) and y_epi = bits(f64(bits(ALPHA acc + BETA y0 + bias)) + residual), with every intermediate asserted a
              multiple of 1/2 below 2^23 in gemm_epilogue's order (alpha, beta y, bias, store, residual add, store)"""
    rng = np.random.default_rng(seed)
    if family == "sparse":
        W, ow = exact_weight(storage, M, K, seed + 1)
        x = ternary(rng, (n, K), min(0.5, 400.0 / (K * (W * W).mean())))
        kk = slice(None)
    else:
        assert family == "block" and len(at)
        blocks = [block_rows(K, a) for a in at]
        kk = np.unique(np.concatenate(blocks))
        signs = np.zeros((M, K))
        signs[:, kk] = rng.choice([-1.0, 1.0], size=(M, len(kk)))
        W, ow = exact_weight(storage, M, K, seed + 1, signs=signs)
        x = np.zeros((n, K))
        for j, blk in enumerate(blocks):
            x[j::len(blocks), blk[0]:blk[-1] + 1] = rng.choice([-1.0, 1.0], size=(len(x[j::len(blocks)]), len(blk)))
    acc = exact_product(x[:, kk], np.ascontiguousarray(W[:, kk].T))
    c = dict(M=M, K=K, n=n, storage=storage, W=W, ow=ow, x=exact_bits(x), y=exact_bits(acc), f64=dict(x=x, acc=acc))
    if epilogue:
        y0, bias, res = small_ints(rng, (n, M)), small_ints(rng, M), small_ints(rng, (n, M))
        v = acc
        for step in (lambda v: ALPHA * v, lambda v: v + BETA * y0, lambda v: v + bias):
            v = step(v)
            assert np.array_equal(2 * v, np.rint(2 * v)) and np.abs(v).max() < 2.0 ** 23
        y1 = f64(bits(v))   # the store may round a half above 128: the fp32 value it rounds is exact, so the rounding is the kernel's
        v = y1 + res
        assert np.array_equal(2 * v, np.rint(2 * v)) and np.abs(v).max() < 2.0 ** 23
        c.update(y0=exact_bits(y0), bias=exact_bits(bias), residual=exact_bits(res), y_epi=bits(v), f64_epi=dict(y0=y0, bias=bias, residual=res))
    return c


# ---- the plan behind the forward entries (kf_gemm_plan.h gemm_plan through kfdbg_gemm_plan), the problem filled as kf_abi.hip problem_of fills it
GE = dict(linear=0, multi=1, gateup=2, rope=3, rope_seqs=3)
FWD_ROUTES = {0: "MATVEC", 1: "AWQ", 2: "ROWFORM", 3: "RESIDENT", 4: "DEQ_TILE", 5: "TILE", 6: "STACKED", 7: "SWIGLU", 8: "ROPE", 9: "FUSED", 10: "SEPARATE"}
FMTS = {0: "bf16", 1: "f8", 2: "q4", 3: "q2", 4: "q1", 6: "q4r"}
DQ_NONE, DQ_SCRATCH, DQ_ARENA, DQ_RESIDENT = range(4)
SK_WS_BYTES = 256 * 256 * 256 * 4 + 8192   # gemm3_sk_ws_bytes(), kf_resident_scratch_bytes()
ARENA_ROOM = 1 << 30


def storage_mat(storage, M, K):
    """kf::mat_of of an uploaded weight of this storage: data and row tables 16-byte aligned, gama present on the quantised forms"""
    type_, row_lut, _, lgroup = STORAGES[storage]
    return _Mat(type_, 1 if row_lut else 0, 0, M, K, lgroup, int(O.BITS[type_] < 8), 3)


def forward_plan(hip, entry, storage, Ms, K, n, scratch=0, arena=False, arena_hit=0, arena_free=ARENA_ROOM):
    """the plan of kf_linear / kf_linear_multi / kf_gateup_swiglu_batch / kf_qkv_rope_batch(_seqs) for weights [Ms[i], K] of one storage at n token rows: x, act, q and k
    aligned, head_dim 128 with whole heads, `scratch` bytes lent through kf_set_scratch, an arena set or not and the copy found in it or not"""
    hip.kfdbg_gemm_plan.argtypes = [C.POINTER(_Problem), C.POINTER(_Plan)]
    P = _Problem(entry=GE[entry], n_w=len(Ms), n=n, x_al=1, y_al=1, rope_ok=int(GE[entry] == 3), arena=int(arena), arena_hit=arena_hit,
                 arena_free=arena_free if arena else 0, scratch=scratch)
    for i, M in enumerate(Ms):
        P.w[i] = storage_mat(storage, M, K)
    out = _Plan()
    assert hip.kfdbg_gemm_plan(C.byref(P), C.byref(out)) == 0 and out.status == 0
    return out


def forward_name(p):
    """"TILE/DIRECT/32/q4", "TILE/STAGED/KS2/q2", "TILE/G2/f8", "RESIDENT/G3/TINY/S2", "RESIDENT/G3/SMALL/tails", "SWIGLU/G3/WIDE", "FUSED/PAIRED/q4", "MATVEC", ...: route,
    family, form, then the format the kernel unpacks (the kf_gemm3.hip tiles read bf16 only) or its split-K cut"""
    route, k = FWD_ROUTES[p.route], p.k
    fam = FAMILIES[k.fam]
    if fam == "NONE":
        return route
    if fam == "G3":
        return "%s/G3/%s%s" % (route, G3_FORMS[k.form], "" if not k.sk else ("/S%d" % k.S if k.S >= 2 else "/tails"))
    form = {"DIRECT": "%d/" % k.form, "STAGED": "KS%d/" % k.form}.get(fam, "")
    return "%s/%s/%s%s" % (route, fam, form, FMTS[k.fmt])


# ---- the cases tests/test_gpu_exact_linear_forward.py runs: (entry, storage, rows of each matrix, K, n, family, setting) -> the plan's name (forward_name), pinned by
# tests/test_exact_inputs_cpu.py.  setting: "" nothing lent; "scratch": what kf_linear_scratch_bytes / kf_linear_multi_scratch_bytes asks for (2 bytes per weight);
# "arena": a dequant arena set and gemm3_sk_ws_bytes() lent (run filling, then finding the resident copy); "epi": the epilogue case (alpha, beta, bias, residual).
# The smallest shapes that reach each form, K 256 unless the case is about K: the form does not depend on K apart from % 64, % 128 and the split-K depth.
FORWARD_CASES = {}
_IN_REGISTER = ("q4", "q4s", "f8", "tern", "bool1", "bf16")


def _cases(want, entry, storages, shapes, K=256, family="sparse", setting=""):
    for st in storages:
        for Ms, n in shapes:
            Ms = (Ms,) if isinstance(Ms, int) else tuple(Ms)
            key = (entry, st, Ms, K, n, family, setting)
            assert key not in FORWARD_CASES
            FORWARD_CASES[key] = want.replace("*", FMTS[{O.BF16: 0, O.F8E5M2: 1, O.Q4: 6 if STORAGES[st][1] else 2, O.T_SIGN: 3}.get(STORAGES[st][0], 4)])


# kf_linear on the weight as stored.  40 x 129: ragged rows and a one-row last token tile; 96 x 8: the first batch past the mat-vec loop
_cases("TILE/DIRECT/32/*", "linear", _IN_REGISTER + ("tbin", "lut", "q4g256", "bool1g256"), [(40, 129), (96, 8)])
_cases("TILE/DIRECT/32/*", "linear", ("lut",), [(96, 64)])
_cases("TILE/STAGED/KS2/*", "linear", ("q4", "q4s", "f8", "tern", "bool1", "lut"), [(2048, 641), (1056, 1281)])
_cases("TILE/STAGED/KS2/*", "linear", ("tbin",), [(2048, 641)])
# bf16 storage on the in-register kernels past the direct kernel's size: kf_gemm3.hip declines a side below 128, the producer / consumer kernel 255 tokens or fewer
_cases("TILE/STAGED/KS2/*", "linear", ("bf16",), [(16384, 96), (96, 16384)])
_cases("TILE/STAGED/KS1/*", "linear", ("bf16", "q4", "f8"), [(65536, 96)])                # 512 staged tiles of which none is a producer / consumer tile: n < 256
_cases("TILE/G2/*", "linear", ("bf16", "q4"), [(96, 32768)])                             # one ragged row tile of 96, 128 token tiles
_cases("TILE/STAGED/KS2/*", "linear", ("q4g256", "bool1g256"), [(2048, 641)])
_cases("TILE/STAGED/KS1/*", "linear", ("tern", "bool1", "tbin", "lut"), [(4096, 2048)])  # from 256 tokens only the formats without a producer / consumer kernel get here
_cases("TILE/G2/*", "linear", ("q4", "q4s", "f8"), [(4096, 1024), (16384, 256)])
_cases("TILE/G3/TINY", "linear", ("bf16",), [(1024, 256), (1056, 1281)])                 # 1056 x 1281: ragged both ways
_cases("TILE/G3/MID", "linear", ("bf16",), [(2048, 641), (6400, 224)])                   # 6400 x 224: n < 256 past the direct kernel's size
_cases("TILE/G3/SMALL", "linear", ("bf16",), [(4096, 1024), (2048, 2304)])
_cases("TILE/G3/BIG", "linear", ("bf16",), [(4096, 2560)])
# K a multiple of 64 only: the half-empty last staged tile of 128 and the clamped address (4-bit in groups of 64)
for _K in (1600, 192):
    _cases("TILE/DIRECT/32/*", "linear", ("q4g64", "q4sg64", "f8", "bf16", "lut"), [(96, 40)], K=_K)   # "lut": the clamped unit is zeroed by masking the fragment
_cases("TILE/STAGED/KS2/*", "linear", ("q4g64", "f8", "lut"), [(1056, 1281)], K=1600)
_cases("TILE/G3/TINY", "linear", ("bf16",), [(1056, 1281)], K=1600)
_cases("MATVEC", "linear", _IN_REGISTER + ("lut",), [(96, 7)])                           # below GEMM_MIN: the mat-vec loop, the same expected bits
_cases("TILE/DIRECT/32/*", "linear", ("q4",), [(40, 129)], setting="epi")
_cases("TILE/STAGED/KS2/*", "linear", ("q4",), [(2048, 641)], setting="epi")
_cases("TILE/G2/*", "linear", ("q4",), [(4096, 1024)], setting="epi")
_cases("TILE/G3/SMALL", "linear", ("bf16",), [(4096, 1024)], setting="epi")
_cases("TILE/G3/BIG", "linear", ("bf16",), [(4096, 2560)], setting="epi")
# kf_linear on a bf16 copy: dequantised into the caller's scratch; resident in the arena with the 64-row tiles in k pieces (S of them, or the owner / helper cut)
_cases("DEQ_TILE/G3/SMALL", "linear", ("q4", "tern"), [(4096, 2048), (1024, 4096)], setting="scratch")
_cases("DEQ_TILE/G3/BIG", "linear", ("q4", "tern"), [(4096, 2560)], setting="scratch")
for _fam in ("sparse", "block"):
    _cases("RESIDENT/G3/TINY/S2", "linear", ("q4",), [(1024, 320)], K=1024, family=_fam, setting="arena")
    _cases("RESIDENT/G3/TINY/S6", "linear", ("q4",), [(1024, 512)], K=3072, family=_fam, setting="arena")
    _cases("RESIDENT/G3/MID/S2", "linear", ("q4",), [(1024, 1536)], K=1024, family=_fam, setting="arena")
    _cases("RESIDENT/G3/MID/tails", "linear", ("q4",), [(2048, 1664)], K=2048, family=_fam, setting="arena")   # 32 x 13 = 416 tiles of 64 x 128: between 1/2 and 4/5 of 768
    _cases("RESIDENT/G3/TINY/S3", "linear", ("q4",), [(1024, 1281)], K=2048, family=_fam, setting="arena")   # 32 k tiles in three pieces: cuts at 10 and 21
_cases("RESIDENT/G3/TINY/S2", "linear", ("tern",), [(1024, 320)], K=1024, setting="arena")
_cases("RESIDENT/DIRECT/32/bf16", "linear", ("q4",), [(128, 320)], setting="arena")      # K 256 is too shallow to cut: the copy on the plain forms
_cases("RESIDENT/G3/TINY", "linear", ("q4",), [(1024, 320)], setting="arena")
_cases("RESIDENT/G3/MID", "linear", ("q4",), [(1024, 1536)], setting="arena")
_cases("RESIDENT/G3/SMALL", "linear", ("q4",), [(4096, 1024)], setting="arena")
_cases("RESIDENT/G3/BIG", "linear", ("q4",), [(4096, 2560)], setting="arena")
# kf_linear_multi: a distinct weight per matrix
_cases("FUSED/DIRECT/32/*", "multi", ("q4", "tern"), [((256, 128, 128), 40)])
_cases("FUSED/DIRECT/64/*", "multi", ("q4", "bool1"), [((1024, 256, 256), 321)])
_cases("STACKED/G3/SMALL", "multi", ("q4",), [((512, 256, 256), 1024)], setting="scratch")
_cases("STACKED/G3/BIG", "multi", ("q4",), [((4096, 4096), 2560)], setting="scratch")
# kf_gateup_swiglu_batch: rows = ffn, twice
_cases("FUSED/PAIRED/*", "gateup", ("q4", "tern"), [((288, 288), 100)])                  # ragged
_cases("FUSED/PAIRED/*", "gateup", ("q4",), [((3072, 3072), 672)])                       # the largest paired grid
_cases("SWIGLU/G3/SMALL", "gateup", ("q4",), [((768, 768), 1024)], setting="scratch")
_cases("SWIGLU/G3/WIDE", "gateup", ("q4",), [((3072, 3072), 1536)], setting="scratch")
_cases("SWIGLU/G3/BIG", "gateup", ("q4",), [((2560, 2560), 2049)], setting="scratch")
# kf_qkv_rope_batch / kf_qkv_rope_seqs: head_dim 128, 4 heads over 2 kv heads
_cases("ROPE/G3/SMALL", "rope", ("q4",), [((512, 256, 256), 1024), ((512, 256, 256), 1280)], setting="scratch")
_cases("ROPE/G3/SMALL", "rope_seqs", ("q4",), [((512, 256, 256), 1024), ((512, 256, 256), 1280)], setting="scratch")
ROPE_SEQ_LEN = {1024: 64, 1280: 160}   # tokens per sequence at each n: sequences that begin inside a 128-token tile

# what the rule cannot reach, and why (tile_plan, g3_plain, gemm_plan_linear).  Every in-register family is reachable on every format that has it: bf16 storage
# leaves kf_gemm3.hip for the staged and producer / consumer kernels with a side below 128, 4-bit and f8 reach staged KS 1 below 256 tokens -- cases above.
FORWARD_UNREACHABLE = {
    "TILE/G2/q2": "the ternary, 1-bit and row-codebook formats have no producer / consumer form",
    "TILE/G2/q1": "as TILE/G2/q2", "TILE/G2/q4r": "as TILE/G2/q2",
    "TILE/G3/WIDE": "192 x 256 tiles are the SwiGLU epilogue's alone (swiglu_kern)",
    "DEQ_TILE/G3/TINY": "the route asks for >= 128 tiles of 256 x 256 or >= 256 of 128 x 128: never fewer than 256 small tiles, so never the 64-row forms",
    "DEQ_TILE/G3/MID": "as DEQ_TILE/G3/TINY",
    "RESIDENT/G3/SMALL/S*": "g3_plain lends the workspace to the 64-row tiles only",
    "RESIDENT/G3/BIG/S*": "as RESIDENT/G3/SMALL/S*",
    "RESIDENT/G3/TINY/tails": "the owner / helper cut needs more than 640 of the 1280 resident 64 x 64 tiles, i.e. more than 320 tiles of 64 x 128: those are taken from 192",
}


def case_setting(key):
    """(scratch bytes lent, arena set) of a case, as its GPU test sets them"""
    entry, st, Ms, K, n, family, setting = key
    if setting == "scratch":
        return (sum(Ms) if entry != "linear" else Ms[0]) * K * 2, False
    return (SK_WS_BYTES, True) if setting == "arena" else (0, False)


def case_plan(hip, key, arena_hit=0):
    scratch, arena = case_setting(key)
    return forward_plan(hip, key[0], key[1], key[2], key[3], key[4], scratch=scratch, arena=arena, arena_hit=arena_hit)


def forward_case(hip, key):
    """the operands of a case: one linear_forward_case per matrix sharing x (a distinct weight each); the block family's blocks on the seams of the case's own plan"""
    entry, st, Ms, K, n, family, setting = key
    seed = sum(Ms) + 3 * K + 7 * n + len(family) + sum(map(ord, st))
    at = seams(case_plan(hip, key), K) if family == "block" else ()
    c = linear_forward_case(Ms[0], K, n, st, seed, family, at, epilogue=setting == "epi")
    c["more"] = []
    for i, M in enumerate(Ms[1:]):
        W, ow = exact_weight(st, M, K, seed + 101 * (i + 1))
        acc = exact_product(c["f64"]["x"], np.ascontiguousarray(W.T))
        c["more"].append(dict(M=M, W=W, ow=ow, y=exact_bits(acc)))
    return c


# ---------------------------------------------------------------------------------------------------------------- the scoring head: the "level" family
# kf_head_logprob's fold has no fp32 sum of products to make exact -- its sums are of exponentials.  The level family makes every exponential 0 or 1: a row's logits are
# exact integers, LEVEL_TOP on the row's winners and within +-LEVEL_FIELD everywhere else.  kf_expf(x) is exactly 0.0f for x < -87.33654 and kf_expf(0) exactly 1, so
# whatever the tile form, the lane order, the merge order or the route:  max = 128, sum = the number of winners c, top1 = the lowest winner,
#     lse = fl32(128 + logf(c))        logprob = fl32(fl32(t - 128) - logf(c))        (t: the target's integer logit; logf: the project's fixed kf_logf, from the oracle)
# A partial whose own maximum is a field value holds some finite sum, and is multiplied by exactly 0 when it meets a winner's.  The second row kind, x = 0, has every
# logit 0: sum = V (an integer below 2^24), top1 = 0, lse = logf(V) -- it counts every column exactly once.
LEVEL_P = 16                             # channels: contraction indices that only a row's own winners answer
LEVEL_TOP, LEVEL_FIELD = 128.0, 40.0     # the gap 88 > 87.33654
ZERO_ROW_EVERY, ZERO_ROW_AT = 7, 3       # rows r with r % 7 == 3 are zero rows
# storage -> (contraction indices per channel, the row's x on them).  A winner's weight on its channel: bf16 holds 16 (x 8); a 4-bit group of step s holds the code
# q0 + 8 / s, i.e. 8 (x 16); a ternary group has no non-zero value common to every (zero, step) table, so a channel is TWO indices with x = (64, -64) and the winner holds
# two codes whose values differ by 2: (1, -1) at step 1, (1, 0) at step 2.  Everybody else holds the code of 0 on every channel index.
LEVEL_FORMS = {"bf16": (1, (8.0,)), "q4": (1, (16.0,)), "tern": (2, (64.0, -64.0))}


def level_winners(V, bm):
    """LEVEL_P winner sets (sorted column arrays), one per channel, for a vocabulary of V columns in tiles of bm (the fused route's G3 form; the panel route has no
    tiles: 128).  Where the vocabulary has too few tiles for a set it falls back to a set that still exists; every set is asserted non-empty and inside [0, V)."""
    n_vt, half = (V + bm - 1) // bm, bm // 2
    full = max(V // bm - 1, 0)               # the last tile that is surely whole (tile 0 when the only tile is ragged: its columns are clipped below)
    mid = min(n_vt // 2, full)

    def tile(t):
        return min(t, n_vt - 1) * bm
    far = (1, 65) if n_vt > 65 else (0, n_vt - 1)
    near = (2, 3) if n_vt > 3 else (0, n_vt - 1)
    sets = [
        [0],                                                         # 0  a single winner at column 0
        [V - 1],                                                     # 1  ... at V - 1, inside the ragged last tile
        [tile(1)],                                                   # 2  ... at the first column of a tile
        [tile(mid) + bm - 1],                                        # 3  ... at the last column of a tile
        [tile(mid) + half - 1, tile(mid) + half],                    # 4  either side of the wave-half seam (64 k - 1 | 64 k of 128 rows, 128 k - 1 | 128 k of 256)
        [tile(n_vt // 3) + 7, tile(n_vt // 3) + 8],                  # 5  either side of a lane seam: 4 q4 + 3 | 4 q4 + 4
        [tile(mid) + 15, tile(mid) + 16],                            # 6  ... 15 | 16: the last lane of one 16-row block, the first of the next
        [tile(far[0]) + 5, tile(far[1]) + 70],                       # 7  tiles l and l + 64: the same merge lane folds both
        [tile(near[0]) + 33, tile(near[1]) + 2],                     # 8  tiles that different merge lanes fold
        [t * bm + (7 * t + 3) % min(bm, V - t * bm) for t in range(n_vt)],   # 9  one winner in every tile: c = n_vt
        [V // 5, V // 2, V - 2],                                     # 10 three winners
        list(np.linspace(0, V - 1, 64).astype(np.int64)),            # 11 64 winners spread out
        [tile(mid) + half + 31, tile(mid) + half + 32],              # 12 a seam between two 16-row blocks of the second wave half
        [tile(2) + 1, tile(66) + 1, tile(130) + 1],                  # 13 three tiles of one merge lane (131 tiles and more)
        [V - 2, V - 1],                                              # 14 the last two columns
        [0, V - 1],                                                  # 15 the first and the last
    ]
    out = []
    for s in sets:
        a = np.unique(np.minimum(np.asarray(s, np.int64), V - 1))
        assert len(a) and a[0] >= 0 and a[-1] < V
        out.append(a)
    assert len(out) == LEVEL_P
    return out


def level_targets(n, V, bm, winners, logits):
    """a target per row, dealt independently of the row's channel: a winner (the highest of the set: not top1 where there are several); a field column in the winner's
    tile; one in another tile; column 0; column V - 1; the first and the last column of a tile; -1 (not scored).  A field column: nobody's winner, and where the tile
    has one, a column whose logit in this row is not 0 (columns 0 and V - 1 and the tiles' corners are other channels' winners: they score 0)."""
    n_vt = (V + bm - 1) // bm
    tg = np.zeros(n, np.int32)
    anybody = np.zeros(V, bool)
    anybody[np.concatenate(winners)] = True

    def field_in(r, t):
        cols = np.arange(t * bm, min((t + 1) * bm, V))
        cols = cols[~anybody[cols]]
        assert len(cols), "no field column in tile %d" % t
        nz = cols[logits[r, cols] != 0]
        return int(nz[0] if len(nz) else cols[0])
    for r in range(n):
        tw = int(winners[r % LEVEL_P][0]) // bm
        kind = (5 * r + r // 16) % 8
        t = r % n_vt
        tg[r] = [int(winners[r % LEVEL_P][-1]), field_in(r, tw), field_in(r, (tw + 1) % n_vt), 0, V - 1, t * bm, min((t + 1) * bm, V) - 1, -1][kind]
    return tg


def level_case(storage, V, K, n, bm, seed):
    """head W [V, K] (exact_weight of the storage, channels planted through its edit hook), rows x [n + 2, K] (two poison rows behind row n that would score 4 x the
    winners on every channel), targets, and the expected outputs as bit patterns: lp, lse (uint32 views of fp32) and top1 [n].  Asserted here on the fp64 product:
    integer logits within +-256, every level row's set of columns at LEVEL_TOP equal to its winner set and every other logit within +-LEVEL_FIELD, every zero row all
    0, the terms' magnitudes summing to < 2^23."""
    width, xs = LEVEL_FORMS[storage]
    nch = LEVEL_P * width
    assert K > nch + 8 and V < 2 ** 24
    winners = level_winners(V, bm)
    rng = np.random.default_rng(seed)

    def edit(q, q0, step):
        q = q.copy()
        q[:, :nch] = q0[:, :nch]                       # nobody but a winner answers a channel
        for cols in winners:
            q[cols] = q0[cols]                         # a winner: 0 on the field
        for c, cols in enumerate(winners):
            i = c * width
            if storage == "bf16":
                q[cols, i] = 16
            elif storage == "q4":
                q[cols, i] = q0[cols, i] + 8 // step[cols, i]
            else:
                q[cols, i], q[cols, i + 1] = 1, np.where(step[cols, i] == 1, -1, 0)
        return q
    W, ow = exact_weight(storage, V, K, seed + 1, edit=edit)
    x = np.zeros((n + 2, K))
    level = np.arange(n) % ZERO_ROW_EVERY != ZERO_ROW_AT
    dx = 0.5
    while True:   # the field's density: the largest that keeps the field within +-LEVEL_FIELD (asserted below either way)
        xf = ternary(rng, (n, K - nch), dx) * level[:, None]
        if np.abs(xf @ W[:, nch:].T).max() <= LEVEL_FIELD or dx < 1e-3:
            break
        dx /= 2
    x[:n, nch:] = xf
    for r in np.nonzero(level)[0]:
        x[r, (r % LEVEL_P) * width:(r % LEVEL_P + 1) * width] = xs
    x[n:, :nch] = np.tile(np.asarray(xs) * 4, LEVEL_P)
    logits = x[:n] @ W.T
    assert np.array_equal(logits, np.rint(logits)) and np.abs(logits).max() <= BOUND
    assert (np.abs(x[:n]) @ np.abs(W).T).max() < 2.0 ** 23
    assert (np.abs(xf) > 0).any() or n < 3
    c = np.ones(n)
    first = np.zeros(n, np.int32)
    for r in range(n):
        if level[r]:
            win = winners[r % LEVEL_P]
            assert np.array_equal(np.nonzero(logits[r] == LEVEL_TOP)[0], win), "row %d: the winner set" % r
            assert np.abs(np.delete(logits[r], win)).max() <= LEVEL_FIELD, "row %d: field %g: lower the density" % (r, np.abs(np.delete(logits[r], win)).max())
            c[r], first[r] = len(win), win[0]
        else:
            assert not logits[r].any()
            c[r] = V
    tg = level_targets(n, V, bm, winners, logits)
    m = np.where(level, np.float32(LEVEL_TOP), np.float32(0.0)).astype(np.float32)
    lg = O.logf(c.astype(np.float32)).astype(np.float32)
    t = logits[np.arange(n), np.maximum(tg, 0)].astype(np.float32)
    lp = np.where(tg >= 0, ((t - m).astype(np.float32) - lg).astype(np.float32), np.float32(0.0)).astype(np.float32)
    lse = (m + lg).astype(np.float32)
    return dict(storage=storage, V=V, K=K, n=n, bm=bm, W=W, ow=ow, x=x, targets=tg, winners=winners, level=level, logits=logits, count=c,
                lp=lp.view(np.uint32), lse=lse.view(np.uint32), top1=first)


def level_fold(logits, targets, V, bm, mutate=None):
    """a plain numpy restatement of the fold (per tile {max, sum exp, first index, target logit}, tiles merged in order) on exact logits, with kf_expf's two exact
    values: exp(0) = 1, exp(d) = 0 for d < -87.33654 (the family's rows make no other difference).  mutate: one wrong decision --
    ("drop", v) column v left out; ("twice", v) counted twice; ("admit",) column V read as a copy of column V - 1 (the tile loads clamp to the last row);
    ("skip", t) tile t left out; ("tie_high",) ties of the maximum go to the higher index; ("neighbour",) the target's logit read from the next tile.
    -> (lp, lse, top1) as level_case returns them"""
    n = logits.shape[0]
    kind = mutate[0] if mutate else None
    lg = np.concatenate([logits, logits[:, -1:]], axis=1) if kind == "admit" else logits
    cols = list(range(lg.shape[1]))
    if kind == "drop":
        cols.remove(mutate[1])
    if kind == "twice":
        cols.append(mutate[1])
    if kind == "skip":
        cols = [v for v in cols if v // bm != mutate[1]]
    cols = np.asarray(cols)
    lp, lse, top1 = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    for r in range(n):
        row = lg[r, cols]
        m = row.max()
        d = row - m
        live = d[d >= -87.34]   # all 0 on the family's rows; a mutation that removes a row's only winner leaves the field, summed here in one of the possible orders
        s = np.float32((d == 0).sum()) if not live.any() else np.float32(O.expf(live.astype(np.float32)).sum(dtype=np.float32))
        at = cols[row == m]
        top1[r] = at.max() if kind == "tie_high" else at.min()
        lgs = O.logf(np.asarray([s], np.float32))[0]
        tgt = int(targets[r])
        if kind == "neighbour" and tgt >= 0:
            tgt = min(tgt + bm, V - 1)
        t = np.float32(logits[r, tgt]) if tgt >= 0 else np.float32(0)
        lp[r] = (np.float32(t - np.float32(m)) - lgs) if tgt >= 0 else np.float32(0)
        lse[r] = np.float32(m) + lgs
    return lp.view(np.uint32), lse.view(np.uint32), top1


# ---- the plan behind kf_head_logprob (kf_score_plan.h score_plan through kfdbg_score_plan), the problem filled as kf_abi.hip score_problem fills it
SR_FUSED, SR_PANEL = 0, 1
SCORE_BIG, SCORE_SMALL = 0, 1            # G3 forms; the "score_form" knob: < 0 the rule


def score_plan(hip, key):
    storage, V, K, n, force, form = key
    hip.kfdbg_score_plan.argtypes = [C.POINTER(_ScoreProblem), C.POINTER(_ScorePlan)]
    out = _ScorePlan()
    assert hip.kfdbg_score_plan(C.byref(_ScoreProblem(storage_mat(storage, V, K), n, 1, force, form)), C.byref(out)) == 0 and out.status == 0
    return out


def score_name(p):
    """"FUSED/SMALL/33x2" (vocabulary tiles x row blocks), "PANEL/128" (rows per panel)"""
    return "FUSED/%s/%dx%d" % ({SCORE_BIG: "BIG", SCORE_SMALL: "SMALL"}[p.form], p.n_vt, p.n_rb) if p.route == SR_FUSED else "PANEL/%d" % p.panel_rows


# (storage, V, K, rows, "score_route" knob, "score_form" knob) -> the plan's name, pinned by tests/test_exact_inputs_cpu.py and asserted before every call.  The smallest
# shapes that reach each path, K = 64 unless the case is about K.  4168 = 32.56 tiles of 128 = 16.28 of 256: ragged either way.
SCORE_CASES = {}
for _n in (1, 127, 128, 129, 257):
    SCORE_CASES[("bf16", 4096 + 72, 64, _n, 0, -1)] = "FUSED/SMALL/33x%d" % ((_n + 127) // 128)
SCORE_CASES.update({
    ("bf16", 128, 64, 40, 0, -1): "FUSED/SMALL/1x1",                       # one tile
    ("bf16", 128 * 130 + 5, 64, 40, 0, -1): "FUSED/SMALL/131x1",           # more than 64 partials per row, three for merge lanes 0 .. 2
    ("bf16", 4096 + 72, 64, 513, 0, -1): "FUSED/BIG/17x3",                 # the 256-row tile by the rule
    ("bf16", 4096 + 72, 64, 40, 0, SCORE_BIG): "FUSED/BIG/17x1",           # ... forced
    ("bf16", 256 * 65 + 72, 64, 40, 0, SCORE_BIG): "FUSED/BIG/66x1",       # 66 partials per row
    ("bf16", 4096 + 72, 192, 129, 0, -1): "FUSED/SMALL/33x2",              # three k steps
    ("bf16", 4096 + 72, 1024, 129, 0, -1): "FUSED/SMALL/33x2",
    ("bf16", 4096 + 72, 64, 130, 1, -1): "PANEL/128",                      # a bf16 head forced to the panel route: a panel of 128 rows and one of 2
    ("bf16", 1000, 64, 9, 1, -1): "PANEL/9",                               # V no multiple of 256, the row kernel's thread stride
    ("bf16", 1000, 200, 130, 0, -1): "PANEL/128",                          # dim 200: no multiple of the tile's k step
    ("q4", 1000, 128, 130, 0, -1): "PANEL/128",
    ("tern", 1000, 128, 33, 0, -1): "PANEL/33",
})


def score_case(hip, key):
    storage, V, K, n, force, form = key
    p = score_plan(hip, key)
    bm = {SCORE_BIG: 256, SCORE_SMALL: 128}[p.form] if p.route == SR_FUSED else 128
    return level_case(storage, V, K, n, bm, seed=V + 3 * K + 7 * n + 11 * force + form)


# ---------------------------------------------------------------------------------------------------------------- the decode kernels on the one-hot / two-hot families
# kf_attn_decode (kf_attn.hip attn_kernel / attn_fast_kernel, route ATTN_SLICED) takes ONE query row: the last row of an attn_case with T = pos + 1.  Its v is drawn from
# [1, 4]: the canonical order sums in fp64, where a weight of 2^-160 does NOT vanish -- it vanishes in the fp32 conversion of O / L, and where the exact output is 0 what
# is left of it there is a signed zero whose sign is the leak's.  With v > 0 no output is 0 and (float)(O / L) is the closed form bit for bit in both orders
# (tests/test_exact_inputs_cpu.py emulates both and shows the signed zero on the [-2, 2] draw).
DECODE_POS = [0, 1, 63, 64, 128, 129, 191, 192, 193, 255, 256, 300, 511]   # 129 .. 191: one slice of > 128 keys (8 waves for GQ <= 2); 192 | 193 keys (positions 191 | 192): one slice | four
DECODE_LONG = dict(pos=2046, nh=4, nkv=2, nbits=11)                        # 2047 keys: the largest slice count (KF_ATTN_MAX_SPLITS = 32)
DECODE_BOUND, DECODE_BELOW = 300, 130                                      # a launch laid out for position 300 whose device position is 130
DECODE_KINDS = 8
DECODE_V = dict(vmin=1, vmax=4)
PER_TOKEN_N = [1, 3, 7]                                                    # below ATTN_TILE_MIN_TOK
PER_TOKEN_REFUSED = dict(n=33, pad=4)                                      # a q row stride of n_head head_dim + 4 elements: no multiple of 8, the tile kernel refuses it


def decode_slices(pos_bound, nkv, gq, canon):
    """kf_attn_plan.h attn_slices + attn_plan restated: (n_splits, chunk, nw, gq_split) of a kf_attn_decode launch laid out for positions up to pos_bound; asserted
    against kfdbg_attn_plan before every call, so a moved threshold fails loudly"""
    ln, nsp = pos_bound + 1, 1
    if ln > 192:
        nsp = min((ln + 63) // 64, 512 // nkv, 32)
    chunk = (ln + nsp - 1) // nsp
    return nsp, chunk, 8 if gq <= 2 and chunk > 128 else 4, gq // 2 if canon and gq > 2 else 1


def decode_targets(pos, nh, chunk, shift):
    """the last row's targets (ta [nh], tb [nh]) by kind (head + shift) % DECODE_KINDS: the diagonal; key 0; key pos - 1; the first key of a middle slice; the last key
    of a slice; the first key of the slice that holds pos; two-hot {a, a - lowest set bit of a} with a the first key of a slice, so that the pair straddles two slices
    (a = pos where the launch has one slice); two-hot on the diagonal.  chunk: keys per slice, as the plan reports it."""
    ta, tb = np.full(nh, pos, np.int64), np.full(nh, -1, np.int64)
    s_pos = pos // chunk
    for h in range(nh):
        kind = (h + shift) % DECODE_KINDS
        a = [pos, 0, pos - 1, chunk * ((s_pos + 1) // 2), chunk * (s_pos // 2 + 1) - 1, chunk * s_pos, chunk * max(s_pos, 1) if s_pos else pos, pos][kind]
        a = a if 0 <= a <= pos else pos
        ta[h] = a
        if kind >= 6 and a > 0:
            tb[h] = a - (a & -a)
    return ta, tb


def decode_case(family, pos, nh, nkv, hd, chunk, shift=0, nbits=NBITS, T=None):
    """an attn_case of T = pos + 1 rows (or more: rows behind pos stay in the cache) whose row `pos` is the query of a decode call, and that row's closed-form output
    as bit patterns"""
    T = pos + 1 if T is None else T
    last = decode_targets(pos, nh, chunk, shift) if family == "code" and T == pos + 1 else None
    c = attn_case(family, T, nh, nkv, hd, seed=pos + nh + hd, nbits=nbits, last=last, **DECODE_V)
    c["want"] = bits(closed_forward(c)[pos])
    return c
