"""kf_gama_backward without a GPU: the two symbols are exported and mirrored, the scratch size is a host function (0 for a refused shape, the plan's slabs otherwise), and
the numpy restatement the GPU tests measure against (tests/gama_ref.py) is itself checked against torch fp64 autograd of w = step (q - qBias) - zero."""
import ctypes as C

import numpy as np
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from tests.gama_ref import gama_grads


def test_symbols_exported_and_mirrored():
    hip, host = L.load()
    for f in ("kf_gama_backward", "kf_gama_backward_scratch_bytes", "kf_dequant_arena_bytes"):
        assert f in L.ABI_SYMBOLS and hasattr(hip, f), f
    assert hip.kf_gama_backward_scratch_bytes.restype is C.c_size_t and len(hip.kf_gama_backward.argtypes) == 8
    for f in ("kfh_gpt2_set_param_gama", "kfh_gpt2_set_gama_scratch"):
        assert hasattr(host, f), f


def test_scratch_bytes_on_the_host():
    hip, _ = L.load()
    sb = hip.kf_gama_backward_scratch_bytes
    up = lambda v: (v + 255) & ~255
    slab = lambda OC, IC: 2 * (OC * IC // 128) * 4   # one slab of partials: [2][nGroup] fp32
    # refused shapes: IC % 128, OC % 64, OC < 128, n % 64, nothing at all
    for OC, IC, n in ((128, 192, 64), (160, 128, 64), (64, 128, 64), (128, 128, 96), (128, 128, 0), (0, 128, 64), (128, 0, 64), (6400, 1600, 8192)):
        assert sb(OC, IC, n) == 0, (OC, IC, n)
    # too few k-steps to cut: one slab; 7 k-steps on 15 tiles: three slabs (2 + 2 + 3 steps)
    assert sb(128, 128, 64) == up(slab(128, 128))
    assert sb(192, 384, 192) == up(slab(192, 384))
    assert sb(320, 640, 448) == up(3 * slab(320, 640))
    # the benchmark's shapes: never more than eight slabs
    for OC, IC, n in ((1600, 6400, 8192), (3072, 1024, 2048), (1024, 3072, 2048)):
        b = sb(OC, IC, n)
        assert b % 256 == 0 and slab(OC, IC) <= b <= up(8 * slab(OC, IC)), (OC, IC, n, b)
    assert hip.kf_gama_backward(None, None, None, None, None, 64, 1.0, None) == -20   # no context: refused, nothing dereferenced


def test_numpy_restatement_matches_autograd():
    """128 x 256 matrix, n = 64: q from oracle.unpack, zero / step from oracle.quantize; the restatement agrees with autograd of the dequantisation formula to 1e-12"""
    OC, IC, n = 128, 256, 64
    rng = np.random.default_rng(5)
    for type_, sym in ((L.Q4, False), (L.Q4, True), (L.T_SIGN, False), (L.BOOL1, False)):
        W = O.f32_to_bf16(rng.normal(0, 0.05, (OC, IC)).astype(np.float32))
        ow = O.quantize(W, OC, IC, type_, symmetric=sym)
        q = O.unpack(ow.data, ow.bits).reshape(OC, IC).astype(np.float64)
        assert q.min() >= 0 and q.max() <= (1 << ow.bits) - 1 and (sym is False or ow.qBias == 8)
        qmb = q - ow.qBias
        dIn = O.bf16_to_f32(O.f32_to_bf16(rng.normal(0, 2.0 ** -6, (n, OC)).astype(np.float32))).astype(np.float64)
        inp = O.bf16_to_f32(O.f32_to_bf16(rng.normal(0, 1.0, (n, IC)).astype(np.float32))).astype(np.float64)
        got, _ = gama_grads(dIn, inp, qmb)
        zero = torch.tensor(O.bf16_to_f32(ow.zero).astype(np.float64), requires_grad=True)
        step = torch.tensor(O.bf16_to_f32(ow.step).astype(np.float64), requires_grad=True)
        Wt = (step[:, None] * torch.tensor(qmb).reshape(-1, 128) - zero[:, None]).reshape(OC, IC)
        ((torch.tensor(inp) @ Wt.T) * torch.tensor(dIn)).sum().backward()
        ref = np.concatenate([zero.grad.numpy(), step.grad.numpy()])
        assert (np.abs(got - ref) <= 1e-12 * np.abs(ref)).all(), (type_, sym, np.abs((got - ref) / ref).max())
        # and the formula is the oracle's dequantisation up to its bf16 roundings (one per product, one per subtraction)
        deq = O.bf16_to_f32(O.dequant(ow)).astype(np.float64)
        assert np.abs(deq - Wt.detach().numpy()).max() <= 2.0 ** -7 * np.abs(deq).max()
