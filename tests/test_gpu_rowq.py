"""The 3- / 2-bit row forms multiplied from the packed stream (kf_set_row_unpack) on the GPU, through the C ABI.

The backbone: every such weight has a 4-BIT TWIN (tests/rowq_twin.py: the same ids as nibbles, a 16-entry table whose first 8 / 4 entries are the row's own), the
library sums over the weight exactly as over its twin, and the oracle already defines the canonical order of the twin's storage.  So
  canonical order   kf_linear == O.linear(twin, x) bit for bit, and == kf_linear on the uploaded twin;
  v_dot2c order     == kf_linear on the uploaded twin bit for bit; within 1 bf16 ulp of O.linear(weight, x) and 2^-8 max|exact| of the fp64 product (tests/test_gpu_lut.py's bars);
  fused entries, token batches: bit-equal to the twin; inputs with exact arithmetic (tests/exact_inputs.py's constructions): every output == bf16(exact).
Every case runs twice against pattern-filled outputs with guard rows before and behind."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_inputs as E
import rowq_twin as T
import test_gemv_plan_cpu as G
from conftest import bf16_t, ulp_diff_bf16
from koifish_amd import lib as L

pytestmark = pytest.mark.gpu
KINDS = ["nf3", "lut2", "rtn2"]
GR = 2                                              # guard rows
PAT = 0xABCD
UNSUPPORTED, UNALIGN = -1000, -2000
# (kind, M, K): 4 units (fewer than lanes); 12 units, M no multiple of the rows per slot; 96 units (a partly filled second step); 256 x 512; then the shapes whose
# stand-in plan keeps two and four slots in flight per wave (random ids: no quantiser run)
SMALL = [(8, 128), (40, 384), (9, 3072), (256, 512)]
G2_SHAPE, G4_SHAPE = (65552, 128), (786448, 128)
ONE_TOKEN = [(kind, m, k) for kind in KINDS for (m, k) in SMALL] + [("ids3", *G2_SHAPE), ("ids3", *G4_SHAPE)]


@pytest.fixture
def rq(ctx):
    """the session context with the switch on; switch and order are put back"""
    ctx.set_row_unpack(1)
    try:
        yield ctx
    finally:
        ctx.set_row_unpack(0)
        ctx.set_canonical(True)


def weight(rng, kind, m, k):
    return T.random_nf3_ids(rng, m, k) if kind == "ids3" else T.random_weight(rng, kind, m, k)


def vec(O, rng, *shape, std=1.0):
    return O.f32_to_bf16(rng.normal(0, std, size=shape).astype(np.float32))


def twice(ctx, rows, m, fn, init=None):
    """fn(y) on two fresh pattern-filled buffers [GR + rows + GR, m] (y = the rows in the middle, preset to init): the guards stay, both runs agree -> y as uint16"""
    outs = []
    for _ in range(2):
        buf = torch.full((rows + 2 * GR, m), int(np.uint16(PAT).astype(np.int16)), dtype=torch.int16, device=ctx.device)
        y = buf[GR:GR + rows].view(torch.bfloat16)
        if init is not None:
            y.copy_(init)
        fn(y)
        ctx.sync()
        b = buf.cpu().numpy().view(np.uint16)
        assert (b[:GR] == PAT).all() and (b[GR + rows:] == PAT).all(), "a guard row was written"
        outs.append(b[GR:GR + rows].copy())
    assert np.array_equal(outs[0], outs[1]), "two runs differ"
    return outs[0]


def k_linear(ctx, dw, x, y, n=1, bias=None, alpha=1.0, beta=0.0, residual=None):
    ctx.linear_scratch(dw, n)
    d = dw.desc()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L.check(ctx.hip.kf_linear(ctx.h, C.byref(d), p(x), p(y), p(bias), n, alpha, beta, L.KF_EPI_RESIDUAL if residual is not None else 0, p(residual)), "kf_linear")


def k_norm_linear(ctx, x, nw, ws, ys):
    descs = [w.desc() for w in ws]
    wp = (C.c_void_p * len(ws))(*[C.addressof(d) for d in descs])
    yp = (C.c_void_p * len(ws))(*[y.data_ptr() for y in ys])
    return ctx.hip.kf_norm_linear(ctx.h, C.c_void_p(x.data_ptr()), None if nw is None else C.c_void_p(nw.data_ptr()), 1e-6, len(ws), wp, yp, None, 0, None)


def stand_in_plan(ctx, m, k, canon):
    """kf::gemv_plan's answer for the 4-bit stand-in of an [m, k] row form (one matrix, plain)"""
    ctx.hip.kfdbg_gemv_plan.argtypes = [C.POINTER(G.Problem), C.POINTER(G.Plan)]
    P = G.Problem(mode=G.PLAIN, n_w=1, canon=int(canon), q4_perm=1, q2_tab=1, q1_tab=1, xf2=1)
    P.w[0] = G.mat(m, k, type=G.Q4, quant=G.ROW_LUT, lgroup=0, al=3)
    out = G.Plan()
    assert ctx.hip.kfdbg_gemv_plan(C.byref(P), C.byref(out)) == 0 and out.status == 0
    return out


def exact_rows(O, ow, x, chunk=65536):
    """fp64 W . x by row chunks of the dequantised weight"""
    per = ow.data.size // ow.ne0
    out = np.empty(ow.ne0)
    xf = O.bf16_to_f32(x).astype(np.float64)
    for r0 in range(0, ow.ne0, chunk):
        r1 = min(r0 + chunk, ow.ne0)
        sub = O.LutWeight(r1 - r0, ow.ne1, ow.data[r0 * per:r1 * per], ow.lut[r0:r1], bits=ow.bits, rtn=ow.rtn)
        out[r0:r1] = O.bf16_to_f32(O.dequant(sub)).astype(np.float64).reshape(r1 - r0, ow.ne1) @ xf
    return out


@pytest.mark.parametrize("kind,m,k", ONE_TOKEN)
def test_one_token_both_orders(rq, O, kind, m, k):
    rng = np.random.default_rng(m * 7 + k)
    ow = weight(rng, kind, m, k)
    dw, dt, tw = T.upload(rq, ow)
    assert T.in_register(rq.hip, dw)
    x = vec(O, rng, k)
    xt = bf16_t(x, rq.device)
    if (m, k) == G2_SHAPE:
        assert stand_in_plan(rq, m, k, 1).G == 2 and stand_in_plan(rq, m, k, 0).G == 2
    if (m, k) == G4_SHAPE:
        assert stand_in_plan(rq, m, k, 1).G == 4 and stand_in_plan(rq, m, k, 0).G == 4
    if (m, k) in SMALL:
        assert stand_in_plan(rq, m, k, 1).G == 1
    # canonical order: the oracle's pattern for the twin, and the twin on the device
    rq.set_canonical(True)
    y = twice(rq, 1, m, lambda y: k_linear(rq, dw, xt, y))[0]
    yt = twice(rq, 1, m, lambda y: k_linear(rq, dt, xt, y))[0]
    with O.canonical():
        ref = O.linear(tw, x)
    assert np.array_equal(y, ref), "%d of %d outputs differ from the oracle's canonical pattern for the twin" % ((y != ref).sum(), m)
    assert np.array_equal(y, yt)
    # v_dot2c order
    rq.set_canonical(False)
    y = twice(rq, 1, m, lambda y: k_linear(rq, dw, xt, y))[0]
    yt = twice(rq, 1, m, lambda y: k_linear(rq, dt, xt, y))[0]
    assert np.array_equal(y, yt)
    d = ulp_diff_bf16(y, O.linear(ow, x))
    assert d.max() <= 1, "max ulp %d" % d.max()
    exact = exact_rows(O, ow, x)
    assert np.abs(O.bf16_to_f32(y) - exact).max() <= 2.0 ** -8 * np.abs(exact).max() + 1e-6


@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_forms_and_epilogues_equal_the_twin(rq, O, kind, canon):
    rng = np.random.default_rng(51)
    k, ms = 512, (256, 128, 128)
    ows = [weight(rng, kind, m, k) for m in ms]
    ups = [T.upload(rq, ow) for ow in ows]
    assert all(T.in_register(rq.hip, u[0]) for u in ups)
    x, nw = vec(O, rng, k), O.f32_to_bf16((1 + 0.1 * rng.normal(size=k)).astype(np.float32))
    xt, nwt = bf16_t(x, rq.device), bf16_t(nw, rq.device)
    rq.set_canonical(canon)

    def norm_linear(ws):
        def run(y):
            ys, o = [], 0
            for w in ws:   # the outputs back to back inside the guarded row
                ys.append(y[0, o:o + w.ne0])
                o += w.ne0
            assert k_norm_linear(rq, xt, nwt, ws, ys) == 0, rq.hip.kf_last_error()
        return twice(rq, 1, sum(w.ne0 for w in ws), run)[0]
    for n_w in (1, 3):
        got, want = norm_linear([u[0] for u in ups[:n_w]]), norm_linear([u[1] for u in ups[:n_w]])
        assert np.array_equal(got, want), "kf_norm_linear, %d matrices" % n_w
    if canon:   # and the oracle's pattern: the launch's rows decide the lanes per row
        xn = O.rmsnorm(x, nw)
        with O.canonical(rows=sum(ms)):
            ref = np.concatenate([O.linear(u[2], xn) for u in ups])
        assert np.array_equal(norm_linear([u[0] for u in ups]), ref)

    def gateup(a, b):
        def run(y):
            da, db = a.desc(), b.desc()
            L.check(rq.hip.kf_norm_gateup_swiglu(rq.h, C.c_void_p(xt.data_ptr()), C.c_void_p(nwt.data_ptr()), 1e-6, C.byref(da), C.byref(db), C.c_void_p(y.data_ptr())), "kf_norm_gateup_swiglu")
        return twice(rq, 1, a.ne0, run)[0]
    assert np.array_equal(gateup(ups[1][0], ups[2][0]), gateup(ups[1][1], ups[2][1])), "kf_norm_gateup_swiglu"
    # epilogues of the one-token kf_linear: bias, alpha / beta on a prior y, residual
    m = ms[0]
    b, y0, res = vec(O, rng, m, std=0.1), vec(O, rng, m, std=0.5), vec(O, rng, m, std=0.5)
    bt, y0t, rest = bf16_t(b, rq.device), bf16_t(y0, rq.device), bf16_t(res, rq.device)
    for kw in (dict(bias=bt), dict(bias=bt, alpha=0.5, beta=2.0), dict(residual=rest), dict(bias=bt, alpha=0.5, beta=2.0, residual=rest)):
        got = twice(rq, 1, m, lambda y: k_linear(rq, ups[0][0], xt, y, **kw), init=y0t)[0]
        want = twice(rq, 1, m, lambda y: k_linear(rq, ups[0][1], xt, y, **kw), init=y0t)[0]
        assert np.array_equal(got, want), sorted(kw)
    if canon:
        got = twice(rq, 1, m, lambda y: k_linear(rq, ups[0][0], xt, y, bias=bt, alpha=0.5, beta=2.0), init=y0t)[0]
        with O.canonical():
            assert np.array_equal(got, O.linear(ups[0][2], x, bias=b, alpha=0.5, beta=2.0, y=y0))


# n, M, K -> the family the stand-in's plan names (asserted): the mat-vec loop below 8 rows, the direct kernel, then the staged kernel in both its forms
BATCHES = [(5, 384, 512, "MATVEC"), (32, 384, 512, "TILE/DIRECT/32/q4r"), (33, 384, 512, "TILE/DIRECT/32/q4r"), (64, 384, 512, "TILE/DIRECT/32/q4r"),
           (200, 384, 512, "TILE/DIRECT/32/q4r"), (1024, 1312, 128, "TILE/STAGED/KS2/q4r"), (1024, 8192, 128, "TILE/STAGED/KS1/q4r")]


@pytest.mark.parametrize("n,m,k,family", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_token_batches_equal_the_twin(rq, O, kind, n, m, k, family):
    assert E.forward_name(E.forward_plan(rq.hip, "linear", "lut", [m], k, n)) == family
    rng = np.random.default_rng(61)
    ow = T.random_nf3_ids(rng, m, k) if (kind == "nf3" and m > 1000) else weight(rng, kind, m, k)
    dw, dt, _ = T.upload(rq, ow)
    assert T.in_register(rq.hip, dw)
    xt, bt = bf16_t(vec(O, rng, n, k), rq.device), bf16_t(vec(O, rng, m, std=0.1), rq.device)
    got = twice(rq, n, m, lambda y: k_linear(rq, dw, xt, y, n=n, bias=bt))
    want = twice(rq, n, m, lambda y: k_linear(rq, dt, xt, y, n=n, bias=bt))
    assert np.array_equal(got, want)
    if m <= 1312:
        W = O.bf16_to_f32(O.dequant(ow)).astype(np.float64).reshape(m, k)
        exact = O.bf16_to_f32(u16np(xt)).astype(np.float64) @ W.T + O.bf16_to_f32(u16np(bt)).astype(np.float64)
        assert np.abs(O.bf16_to_f32(got) - exact).max() <= 2.0 ** -8 * np.abs(exact).max() + 1e-6


def u16np(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("kind", KINDS)
def test_shared_input_batches_equal_the_twin(rq, O, kind):
    """kf_linear_multi (the fused direct launch over Q | K | V) and kf_gateup_swiglu_batch (the paired direct kernel) at 40 token rows"""
    rng = np.random.default_rng(62)
    n, k, ms = 40, 256, (128, 64, 64)
    assert E.forward_name(E.forward_plan(rq.hip, "multi", "lut", list(ms), k, n)) == "FUSED/DIRECT/32/q4r"
    assert E.forward_name(E.forward_plan(rq.hip, "gateup", "lut", [ms[1], ms[1]], k, n)) == "FUSED/PAIRED/q4r"
    ups = [T.upload(rq, weight(rng, kind, m, k)) for m in ms]
    assert all(T.in_register(rq.hip, u[0]) for u in ups)
    xt = bf16_t(vec(O, rng, n, k), rq.device)

    def multi(which):
        ws = [u[which] for u in ups]
        ys = [torch.zeros(n, w.ne0, dtype=torch.bfloat16, device=rq.device) for w in ws]
        descs = [w.desc() for w in ws]
        wp = (C.c_void_p * 3)(*[C.addressof(d) for d in descs])
        yp = (C.c_void_p * 3)(*[y.data_ptr() for y in ys])
        assert rq.hip.kf_linear_multi(rq.h, 3, wp, C.c_void_p(xt.data_ptr()), yp, n) == 0, rq.hip.kf_last_error()
        return [u16np(y) for y in ys]
    for a, b in zip(multi(0), multi(1)):
        assert np.array_equal(a, b)

    def gateup(which):
        def run(act):
            up = torch.zeros(n, ms[1], dtype=torch.bfloat16, device=rq.device)
            dg, du = ups[1][which].desc(), ups[2][which].desc()
            assert rq.hip.kf_gateup_swiglu_batch(rq.h, C.byref(dg), C.byref(du), C.c_void_p(xt.data_ptr()), C.c_void_p(act.data_ptr()), C.c_void_p(up.data_ptr()), n) == 0, rq.hip.kf_last_error()
        return twice(rq, n, ms[1], run)
    assert np.array_equal(gateup(0), gateup(1))


# ---- inputs whose arithmetic is exact in fp32 (tests/exact_inputs.py): chosen ids, chosen tables that differ from row to row
def exact_weight(O, rng, kind, M, K):
    """(W fp64 integers [M, K], the oracle weight holding exactly W): 3-bit rows hold a permutation of -4 .. 3, 2-bit rows one of -2 .. 1, row RTN zero in {-2, -1} and
    step 1; an entry is 0 with probability 1 - d, else +-1 (3-bit: or +-2), and one entry in 128 holds any code"""
    nb = 3 if kind == "nf3" else 2
    lo = -(1 << (nb - 1))
    if kind == "rtn2":
        zero = rng.choice([-2, -1], size=M)
        table = zero[:, None] + np.arange(4)[None, :]
        lut = E.exact_bits(np.stack([zero, np.ones(M)], axis=1).astype(np.float64))
    else:
        table = np.stack([rng.permutation(1 << nb) + lo for _ in range(M)])
        for r in np.nonzero((table[1:] == table[:-1]).all(axis=1))[0]:
            table[r + 1] = np.roll(table[r + 1], 1)
        lut = E.exact_bits(table.astype(np.float64))
    W = E.ternary(rng, (M, K), E.density(K, 2.5 if nb == 3 else 1.0), twos=(nb == 3))
    any_code = rng.random((M, K)) < 1.0 / 128
    W = np.where(any_code, np.take_along_axis(table, rng.integers(0, 1 << nb, size=(M, K)), axis=1), W)
    code = np.argsort(table, axis=1)[np.arange(M)[:, None], (W - table.min(axis=1)[:, None]).astype(np.int64)]   # the place of value v in the row's table
    assert np.array_equal(np.take_along_axis(table, code, axis=1), W)
    data = np.packbits(((code[..., None] >> np.arange(nb - 1, -1, -1)) & 1).astype(np.uint8).reshape(-1))
    ow = O.LutWeight(M, K, data, lut, bits=nb, rtn=(kind == "rtn2"))
    assert np.array_equal(O.dequant(ow).reshape(M, K), E.exact_bits(W)), "the storage does not hold the weight exactly"
    return W, ow


@pytest.mark.parametrize("n,M,K,family", [(1, 40, 384, "MATVEC"), (1, 9, 3072, "MATVEC"), (33, 72, 256, "TILE/DIRECT/32/q4r"), (1024, 1312, 128, "TILE/STAGED/KS2/q4r"),
                                          (1024, 8192, 128, "TILE/STAGED/KS1/q4r")])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_inputs(rq, O, kind, n, M, K, family):
    assert E.forward_name(E.forward_plan(rq.hip, "linear", "lut", [M], K, n)) == family
    rng = np.random.default_rng(71)
    W, ow = exact_weight(O, rng, kind, M, K)
    x = E.ternary(rng, (n, K), min(0.5, 400.0 / (K * (W * W).mean())))
    want = E.exact_bits(E.exact_product(x, np.ascontiguousarray(W.T)))
    dw = T.DevRowWeight(rq, ow)
    assert T.in_register(rq.hip, dw)
    xt = bf16_t(E.exact_bits(x), rq.device)
    for canon in ((True, False) if n == 1 else (True,)):
        rq.set_canonical(canon)
        got = twice(rq, n, M, lambda y: k_linear(rq, dw, xt, y, n=n))
        assert np.array_equal(got, want), "%d outputs are not bf16(exact)" % (got != want).sum()


def test_switch_and_refusals(ctx, O):
    rng = np.random.default_rng(81)
    m, k = 16, 128
    d3 = ctx.upload_lut_blob(m, k, T.blob(T.random_weight(rng, "nf3", m, k)), bits=3)
    x = torch.zeros(k, dtype=torch.bfloat16, device=ctx.device)
    y = torch.zeros(m, dtype=torch.bfloat16, device=ctx.device)
    assert ctx.hip.kf_get_row_unpack(ctx.h) == 0                                       # the default
    assert k_norm_linear(ctx, x, None, [d3], [y]) == UNSUPPORTED                       # off: as ever
    ctx.set_row_unpack(1)
    try:
        assert ctx.hip.kf_get_row_unpack(ctx.h) == 1
        assert k_norm_linear(ctx, x, None, [d3], [y]) == 0
        # the shape rule: K = 64 runs through the dequantised copy in kf_linear, and the fused entries refuse it
        d64 = ctx.upload_lut_blob(m, 64, T.blob(T.random_weight(rng, "nf3", m, 64)), bits=3)
        x64 = bf16_t(vec(O, rng, 64), ctx.device)
        assert k_norm_linear(ctx, x64, None, [d64], [y]) == UNALIGN
        dg, du = d64.desc(), d64.desc()
        assert ctx.hip.kf_norm_gateup_swiglu(ctx.h, C.c_void_p(x64.data_ptr()), None, 1e-6, C.byref(dg), C.byref(du), C.c_void_p(y.data_ptr())) == UNALIGN
        ow64 = T.random_weight(rng, "nf3", m, 64)
        got = ctx.linear(ctx.upload_lut_blob(m, 64, T.blob(ow64), bits=3), x64)
        assert ulp_diff_bf16(u16np(got), O.linear(ow64, u16np(x64))).max() <= 1
        # tables that are not aligned to their size: the same
        d = d3.desc()
        d.gama += 2
        assert k_norm_linear_desc(ctx, x, d, y) == UNALIGN
        # a 3-bit matrix next to a 4-bit row codebook in one launch
        d4 = ctx.upload_lut_blob(m, k, T.blob(T.twin(T.random_weight(rng, "nf3", m, k))), bits=4)
        assert k_norm_linear(ctx, x, None, [d3, d4], [y, y.clone()]) < 0
        # what stays refused: the embedding, the LM head forms, the masked forms, the row entries
        d = d3.desc()
        out = torch.zeros(k, dtype=torch.bfloat16, device=ctx.device)
        assert ctx.hip.kf_embed(ctx.h, C.byref(d), 1, None, C.c_void_p(out.data_ptr())) == UNSUPPORTED
        with pytest.raises(L.KFError):
            ctx.lm_head(d3, x)
        state = torch.zeros(2, dtype=torch.int32, device=ctx.device)
        assert ctx.hip.kf_norm_lm_head(ctx.h, C.c_void_p(x.data_ptr()), None, 1e-6, C.byref(d), C.c_void_p(y.data_ptr()), C.c_void_p(state.data_ptr()), None,
                                       C.c_void_p(ctx._head_ws.data_ptr())) == UNSUPPORTED
        rows = torch.arange(4, dtype=torch.int32, device=ctx.device)
        assert ctx.hip.kf_linear_masked(ctx.h, C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), None, C.c_void_p(rows.data_ptr()), 4) == UNSUPPORTED
        assert ctx.hip.kf_norm_gateup_swiglu_masked(ctx.h, C.c_void_p(x.data_ptr()), None, 1e-6, C.byref(d), C.byref(d), C.c_void_p(y.data_ptr()), C.c_void_p(rows.data_ptr()),
                                                    4) == UNSUPPORTED
        with pytest.raises(L.KFError):
            ctx.linear_rows(d3, x.view(1, k))
    finally:
        ctx.set_row_unpack(0)
    assert k_norm_linear(ctx, x, None, [d3], [y]) == UNSUPPORTED                       # off again: refused as before
    ctx.sync()


def k_norm_linear_desc(ctx, x, d, y):
    wp = (C.c_void_p * 1)(C.addressof(d))
    yp = (C.c_void_p * 1)(y.data_ptr())
    return ctx.hip.kf_norm_linear(ctx.h, C.c_void_p(x.data_ptr()), None, 1e-6, 1, wp, yp, None, 0, None)
