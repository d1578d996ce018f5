"""The numpy restatement of the int8-activation arithmetic (include/kf_abi.h "int8 activations"), stated ONCE for the test files that need it: tests/test_a8_cpu.py
checks the properties the definition's exactness claims rest on, tests/test_gpu_a8.py holds the kernels and the model switch to it bit for bit.  Nothing here calls the
library; the oracle is used for its bf16 conversion and for unpacking the stored codes only."""
import numpy as np

from koifish_amd import lib as L
from oracle import oracle as O

BITS = {L.T_SIGN: 2, L.BOOL1: 1, L.T_BINARY: 1}


def bf(u):
    return O.bf16_to_f32(np.asarray(u, dtype=np.uint16))


def to_bf(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def quant_rows(x_u16):
    """bf16 rows (uint16 bit patterns) -> (q int8 [rows, dim], step fp32 [rows])"""
    return quant_rows_f32(bf(x_u16))


def quant_rows_f32(x):
    """fp32 rows -> (q int8 [rows, dim], step fp32 [rows]): absolute maximum, amax / 127 and x / step as correctly rounded fp32 divisions, halves away from zero, +-127"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    amax = np.abs(x).max(axis=1)
    step = (amax / np.float32(127.0)).astype(np.float32)
    q = np.zeros(x.shape, dtype=np.int8)
    for r in range(x.shape[0]):
        if amax[r] != 0:
            d = (x[r] / step[r]).astype(np.float32).astype(np.float64)
            q[r] = np.clip(np.sign(d) * np.floor(np.abs(d) + 0.5), -127, 127).astype(np.int8)
    return q, step


class IntW:
    """integer weights t_w = code - qBias [M, K] from the oracle's unpack, and the bf16 group steps as fp32 [M, K / 128]"""

    def __init__(self, ow):
        self.M, self.K = ow.ne0, ow.ne1
        self.t = (O.unpack(ow.data, BITS[ow.type]).reshape(self.M, self.K) - ow.qBias).astype(np.int64)
        self.step = bf(ow.step).reshape(self.M, self.K // 128)
        assert not (np.asarray(ow.zero) & 0x7fff).any()


def linear_a8(w, q, step, bias=None, residual=None):
    """y [nTok, M] uint16: I_g exact, acc = acc + step_w[g] * I_g for g = 0, 1, .. (ONE ascending fp32 chain), y = bf16(step_x * acc [+ bias]), then the residual epilogue"""
    q = np.atleast_2d(q).astype(np.int64)
    G = w.K // 128
    I = np.einsum("mgc,tgc->tmg", w.t.reshape(w.M, G, 128), q.reshape(-1, G, 128))
    assert np.abs(I).max() <= 16256
    acc = np.zeros(I.shape[:2], dtype=np.float32)
    for g in range(G):
        acc = (acc + (w.step[None, :, g] * I[:, :, g].astype(np.float32)).astype(np.float32)).astype(np.float32)
    v = (np.asarray(step, dtype=np.float32).reshape(-1, 1) * acc).astype(np.float32)
    if bias is not None:
        v = (v + bf(bias)[None, :]).astype(np.float32)
    y = to_bf(v)
    if residual is not None:
        y = to_bf((bf(residual).reshape(y.shape) + bf(y)).astype(np.float32))
    return y
