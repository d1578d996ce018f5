"""What tests/test_gpu_w4a8.py and tests/test_gpu_w4a8_tiles.py share: per (shape, qBias) ONE quantised weight on the device, ONE draw of 70 activation rows and the
restatement's product of all 70 (tests/w4a8_restate.py), computed once and left unchanged; the hand-built blobs; the guarded launch."""
import numpy as np
import torch

from koifish_amd import lib as L
from oracle import oracle as O
from w4a8_restate import IntW4, large_sum_case, linear_w4a8, quant_rows, to_bf

FILL = 0x7fc1      # a bf16 NaN pattern no kernel stores
# (M, K): one group and the row tail of a 64-row tile | 3 groups, fewer than lanes per row | 10 groups: the masked tail of the last step, a second chunk of 2 groups |
# 8 lanes per row, one step | 64 lanes per row
SHAPES = [(80, 128), (130, 384), (64, 1280), (72, 1024), (64, 8192)]
_CASE = {}


def t_bf16(u16_, dev):
    return torch.from_numpy(np.ascontiguousarray(u16_).view(np.int16)).to(dev).view(torch.bfloat16)


def u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def upload(ctx, ow):
    return ctx.upload_blob(L.Q4, ow.ne0, ow.ne1, ow.blob(), symmetric=ow.qBias == 8)


def case(ctx, M, K, qBias):
    """weights with a per-group offset, so that ZERO != 0 in every group; qBias 8 reads the same codes, ZERO and STEP with 8 taken off every code (the symmetric
    quantiser itself writes ZERO = 0)"""
    key = (M, K, qBias)
    if key not in _CASE:
        rng = np.random.default_rng(5 + M + K)
        w = rng.normal(0, 0.05, (M, K)).astype(np.float32) + np.repeat(rng.choice([-1.0, 1.0], (M, K // 128)) * rng.uniform(0.03, 0.08, (M, K // 128)), 128, axis=1).astype(np.float32)
        ow = O.quantize(to_bf(w), M, K, L.Q4)
        assert ow.qBias == 0 and (ow.zero & 0x7fff).all()
        if qBias:
            ow = O.QWeight(L.Q4, M, K, ow.data, ow.zero, ow.step, 128, qBias)
        iw = IntW4(ow)
        q, s = quant_rows(to_bf(np.random.default_rng(M * K).normal(0, 1, (70, K)).astype(np.float32)))
        dw = upload(ctx, ow)
        assert dw.qBias == qBias
        _CASE[key] = (dw, iw, q, s, linear_w4a8(iw, q, s))
    return _CASE[key]


def saturating(qBias):
    """(QWeight, q, step_x, the |I_g| every group must reach): all codes 15 under qBias 0 against q = 127 (I_g = 243 840, S_g = 16 256), all codes 0 under qBias 8 against
    q = -127 (I_g = 130 048, S_g = -16 256); every other token row flips the sign of q, a few steps of x"""
    M, K, n = 8, 384, 17
    G = K // 128
    rng = np.random.default_rng(9 + qBias)
    codes = np.full((M, K), 0 if qBias else 15, dtype=np.int32)
    step_w = to_bf(rng.uniform(0.01, 0.2, M * G).astype(np.float32))
    zero_w = to_bf(rng.normal(0, 0.3, M * G).astype(np.float32))
    ow = O.QWeight(L.Q4, M, K, O.pack(codes, 4), zero_w, step_w, 128, qBias)
    q = np.full((n, K), -127 if qBias else 127, dtype=np.int8)
    q[1::2] = -q[1::2]
    step = np.resize(np.array([1.0, 0.37, 2.5e-3, 11.0, 1.0], dtype=np.float32), n)
    return ow, q, step, (8 if qBias else 15) * 127 * 128


def run(ctx, entry, dw, q, step, bias=None, residual=None, alias=False):
    """one launch into a buffer pre-filled with FILL that has two guard rows behind the outputs; alias: the residual is y itself"""
    n, M = q.shape[0], dw.ne0
    buf = t_bf16(np.full((n + 2, M), FILL, dtype=np.uint16), ctx.device)
    y = buf[:n]
    if alias:
        y.copy_(t_bf16(residual, ctx.device))
    dq, ds = torch.from_numpy(np.ascontiguousarray(q)).to(ctx.device), torch.from_numpy(np.ascontiguousarray(step)).to(ctx.device)
    res = y if alias else None if residual is None else t_bf16(residual, ctx.device)
    getattr(ctx, entry)(dw, dq, ds, bias=None if bias is None else t_bf16(bias, ctx.device), residual=res, y=y)
    ctx.sync()
    out = u16(buf)
    assert (out[n:] == FILL).all(), "%s wrote behind its %d token rows" % (entry, n)
    return out[:n]


__all__ = ["FILL", "SHAPES", "IntW4", "case", "large_sum_case", "linear_w4a8", "run", "saturating", "t_bf16", "u16", "upload"]
