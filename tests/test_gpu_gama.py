"""kf_gama_backward (SLP::Back's "train_target": "gama" branch -> CU_GamaBack_2) through the C ABI against the fp64 restatement of tests/gama_ref.py (itself checked
against autograd in tests/test_gama_cpu.py).  The weight comes from the device quantiser; q - qBias is read back from its packed bytes with oracle.unpack.

Random data is held to a DERIVED bound, |got - ref| <= 2^-8 |ref| + (n + 128) 2^-23 A[g] (gama_ref.bound); a one-hot dW is held to exact equality, which pins the group
indexing and the Packed128 element order that a tolerance can blur.

Shapes (OC, IC, n): one group per row and one k-step; OC no multiple of 128 with three groups per row (all four storages); several 128 x 128 tiles with ragged edges and a
cut of 7 k-steps into 3 slabs; and the smallest ragged shape that the plan (kf_gama_plan.h) sends to the 256 x 256 tile form (160 tiles or more), whose last IC tile is
half outside the matrix."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from koifish_amd.runtime import AWQDevWeight, DevWeight, LutDevWeight
from oracle import oracle as O
from tests.conftest import bf16_t, u16
from tests.gama_ref import bound, gama_grads

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, UNALIGN = -20, -1000, -2000
STORAGES = {"q4": (L.Q4, False), "q4sym": (L.Q4, True), "tsign": (L.T_SIGN, False), "bool1": (L.BOOL1, False)}
BF = lambda a: O.f32_to_bf16(np.asarray(a, dtype=np.float32))
F64 = lambda h: O.bf16_to_f32(h).astype(np.float64)


def make_weight(ctx, OC, IC, storage, seed):
    """a device-quantised weight and q - qBias [OC, IC] as read back from its packed bytes"""
    type_, sym = STORAGES[storage]
    rng = np.random.default_rng(seed)
    dw = ctx.quantize(bf16_t(BF(rng.normal(0, 0.05, (OC, IC))), ctx.device), type_, symmetric=sym)
    ctx.sync()
    q = O.unpack(dw.blob[:dw.szData].cpu().numpy(), L.BITS[type_]).reshape(OC, IC)
    assert dw.qBias == {"q4": 0, "q4sym": 8, "tsign": 1, "bool1": 0}[storage]
    return dw, (q - dw.qBias).astype(np.float64)


class Scratch:
    def __init__(self, ctx, OC, IC, n):
        self.bytes = ctx.hip.kf_gama_backward_scratch_bytes(OC, IC, n)
        assert self.bytes > 0 and self.bytes % 256 == 0
        self.t = torch.zeros(self.bytes + 256, dtype=torch.uint8, device=ctx.device)
        self.ptr = (self.t.data_ptr() + 255) & ~255


def run(ctx, dw, dIn, inp, g, n, sc, scale=1.0):
    d = dw.desc()
    rc = ctx.hip.kf_gama_backward(ctx.h, C.byref(d), dIn.data_ptr(), inp.data_ptr(), g.data_ptr(), n, scale, sc.ptr)
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    return F64(u16(g))


@pytest.mark.parametrize("OC,IC,n,storage", [(128, 128, 64, "q4"), (192, 384, 192, "q4"), (192, 384, 192, "q4sym"), (192, 384, 192, "tsign"), (192, 384, 192, "bool1"),
                                             (320, 640, 448, "q4"), (3776, 2688, 128, "q4")])
def test_random_data_within_the_derived_bound(ctx, OC, IC, n, storage):
    dw, qmb = make_weight(ctx, OC, IC, storage, 11)
    rng = np.random.default_rng(OC + IC + n)
    inp, dIn = BF(rng.normal(0, 1.0, (n, IC))), BF(rng.normal(0, 2.0 ** -6, (n, OC)))
    ref, A = gama_grads(F64(dIn), F64(inp), qmb)
    sc = Scratch(ctx, OC, IC, n)
    g = torch.zeros(2 * dw.nGroup, dtype=torch.bfloat16, device=ctx.device)
    got = run(ctx, dw, bf16_t(dIn, ctx.device), bf16_t(inp, ctx.device), g, n, sc)
    err, lim = np.abs(got - ref), bound(ref, A, n)
    print("%s %dx%d n=%d: worst err / bound %.3f, max |ref| %.3g" % (storage, OC, IC, n, (err / lim).max(), np.abs(ref).max()))
    assert ref[:dw.nGroup].any() and ref[dw.nGroup:].any() and got.any()
    assert (err <= lim).all(), "worst err / bound %.3f at element %d" % ((err / lim).max(), int((err / lim).argmax()))


@pytest.mark.parametrize("storage", list(STORAGES))
def test_one_hot_is_exact(ctx, storage):
    """dW has a single non-zero at (r, c): the hit group's pair is bf16(-/+ delta x (1 | q - qBias)) exactly, every other group 0"""
    OC, IC, n = 192, 384, 192
    dw, qmb = make_weight(ctx, OC, IC, storage, 12)
    sc = Scratch(ctx, OC, IC, n)
    delta, x = 1.3125, -0.8125   # bf16 values whose product (273 / 256) is not one: the store's rounding is part of the check
    nG, gpr = dw.nGroup, IC // 128
    for i0, r in ((0, 0), (n - 1, OC - 1)):
        for c in (0, 31, 32, 127, 128, IC - 1):
            dIn, inp = np.zeros((n, OC), np.float32), np.zeros((n, IC), np.float32)
            dIn[i0, r], inp[i0, c] = delta, x
            g = torch.zeros(2 * nG, dtype=torch.bfloat16, device=ctx.device)
            run(ctx, dw, bf16_t(BF(dIn), ctx.device), bf16_t(BF(inp), ctx.device), g, n, sc)
            want = np.zeros(2 * nG, np.float32)
            hit = r * gpr + c // 128
            want[hit], want[nG + hit] = -delta * x, delta * x * qmb[r, c]
            want = want + np.float32(0.0)   # gGama starts at +0: a product with q - qBias = 0 is -0, and 0 + (-0) = +0 is what is stored
            assert np.array_equal(u16(g), BF(want)), (storage, r, c, qmb[r, c], np.flatnonzero(u16(g) != BF(want))[:8])


def test_accumulates_is_deterministic_and_stays_inside_its_output(ctx):
    OC, IC, n = 320, 640, 448   # three slabs: the scratch holds partials that are summed
    dw, qmb = make_weight(ctx, OC, IC, "q4", 13)
    nG = dw.nGroup
    rng = np.random.default_rng(3)
    inp, dIn = bf16_t(BF(rng.normal(0, 1.0, (n, IC))), ctx.device), bf16_t(BF(rng.normal(0, 2.0 ** -6, (n, OC))), ctx.device)
    sc = Scratch(ctx, OC, IC, n)
    assert sc.bytes == 3 * 2 * nG * 4
    # 64 guard elements on either side of gGama
    buf = torch.zeros(64 + 2 * nG + 64, dtype=torch.bfloat16, device=ctx.device)
    buf.view(torch.int16)[:64] = 0x7E5A
    buf.view(torch.int16)[-64:] = 0x7E5A
    g = buf[64:64 + 2 * nG]
    run(ctx, dw, dIn, inp, g, n, sc)
    first = u16(g).copy()
    assert first.any() and (u16(buf)[:64] == 0x7E5A).all() and (u16(buf)[-64:] == 0x7E5A).all()
    # bit-equal from a zeroed gGama, whatever the scratch held before
    g.zero_()
    sc.t.fill_(0xFF)
    run(ctx, dw, dIn, inp, g, n, sc)
    assert np.array_equal(u16(g), first)
    # accumulation, exactly: a one-hot dW whose fp32 sum S is known, on top of arbitrary old values, with a scale
    old = BF(rng.normal(0, 1.0, 2 * nG))
    g.copy_(bf16_t(old, ctx.device))
    r, c, i0, delta, x, scale = 77, 300, 200, 1.3125, -0.8125, 0.5
    d1, x1 = np.zeros((n, OC), np.float32), np.zeros((n, IC), np.float32)
    d1[i0, r], x1[i0, c] = delta, x
    run(ctx, dw, bf16_t(BF(d1), ctx.device), bf16_t(BF(x1), ctx.device), g, n, sc, scale=scale)
    S = np.zeros(2 * nG, np.float32)
    hit = r * (IC // 128) + c // 128
    S[hit], S[nG + hit] = -delta * x, delta * x * qmb[r, c]
    assert np.array_equal(u16(g), BF(O.bf16_to_f32(old) + np.float32(scale) * S))
    # and on random data a second call lands on bf16(old + sum) up to the sum's own bound
    g.zero_()
    run(ctx, dw, dIn, inp, g, n, sc)
    twice = run(ctx, dw, dIn, inp, g, n, sc)
    ref, A = gama_grads(F64(u16(dIn)), F64(u16(inp)), qmb)
    assert (np.abs(twice - (F64(first) + ref)) <= 2.0 ** -8 * np.abs(F64(first) + ref) + (n + 128) * 2.0 ** -23 * A).all()


def test_refusals_launch_nothing(ctx):
    hip, dev = ctx.hip, ctx.device
    OC, IC, n = 192, 384, 192
    dw, _ = make_weight(ctx, OC, IC, "q4", 14)
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
    dIn, inp = z(n + 1, OC), z(n + 1, IC)
    g = torch.full((2 * dw.nGroup + 8,), 3.0, dtype=torch.bfloat16, device=dev)
    sc = Scratch(ctx, OC, IC, n)

    def call(w, dIn_p=dIn.data_ptr(), inp_p=inp.data_ptr(), g_p=g.data_ptr(), n_=n, sp=sc.ptr):
        d = w.desc()
        rc = hip.kf_gama_backward(ctx.h, C.byref(d), dIn_p, inp_p, g_p, n_, 1.0, sp)
        ctx.sync()
        assert (u16(g) == 0x4040).all(), "gGama was written by a refused call (%d)" % rc
        return rc
    fake = lambda type_, ne0, ne1: DevWeight(type_, ne0, ne1, torch.zeros(DevWeight.blob_bytes(type_, ne0, ne1), dtype=torch.uint8, device=dev))
    # shapes: KF_INVALID_ARGS
    assert call(fake(L.Q4, 128, 192)) == INVALID          # IC % 128
    assert call(fake(L.Q4, 160, 128)) == INVALID          # OC % 64
    assert call(fake(L.Q4, 64, 128)) == INVALID           # OC < 128
    assert call(dw, n_=96) == INVALID                     # n % 64
    assert hip.kf_gama_backward_scratch_bytes(OC, IC, 96) == 0
    # null pointers, a missing scratch
    assert call(dw, dIn_p=None) == INVALID and call(dw, inp_p=None) == INVALID and call(dw, sp=None) == INVALID
    d = dw.desc()
    assert hip.kf_gama_backward(ctx.h, C.byref(d), dIn.data_ptr(), inp.data_ptr(), None, n, 1.0, sc.ptr) == INVALID
    assert hip.kf_gama_backward(ctx.h, None, dIn.data_ptr(), inp.data_ptr(), g.data_ptr(), n, 1.0, sc.ptr) == INVALID
    # storages: KF_UNSUPPORTED_DATATYPE
    assert call(fake(L.BF16, OC, IC)) == UNSUPPORTED and call(fake(L.F8E5M2, OC, IC)) == UNSUPPORTED
    assert call(LutDevWeight(OC, IC, torch.zeros(LutDevWeight.blob_bytes(OC, IC, 4), dtype=torch.uint8, device=dev), 4)) == UNSUPPORTED          # row-LUT
    assert call(LutDevWeight(OC, IC, torch.zeros(OC * IC // 4 + (OC + IC + 2 * OC) * 2, dtype=torch.uint8, device=dev), 2, rtn=True)) == UNSUPPORTED   # row-RTN
    awq = AWQDevWeight(OC, IC, torch.zeros(IC, OC // 8, dtype=torch.int32, device=dev), torch.zeros(IC // 128, OC // 8, dtype=torch.int32, device=dev),
                       torch.zeros(IC // 128, OC, dtype=torch.float16, device=dev))
    assert call(awq) == UNSUPPORTED
    # alignment: KF_BLAS_UNALIGN
    assert call(dw, dIn_p=dIn.data_ptr() + 2) == UNALIGN and call(dw, inp_p=inp.data_ptr() + 2) == UNALIGN
    assert call(dw, g_p=g.data_ptr() + 2) == UNALIGN and call(dw, sp=sc.ptr + 16) == UNALIGN
    # the Python wrapper sizes the scratch itself (the entry is not told its size) and refuses tensors that do not fit the weight
    with pytest.raises(L.KFError):
        ctx.gama_backward(dw, dIn[:n], inp[:n], g[:8])
    out = ctx.gama_backward(dw, dIn[:n], inp[:n], z(2 * dw.nGroup))
    ctx.sync()
    assert not u16(out).any()   # zero operands: zero gradients
