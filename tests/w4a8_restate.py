"""The numpy restatement of the W4.A8 arithmetic (include/kf_abi.h "int8 activations for 4-bit layers"), stated ONCE for the test files that need it:
tests/test_w4a8_cpu.py holds it against exact rational arithmetic, the GPU tests hold the kernels and the model switch to it bit for bit.  float32 / int64, plain IEEE
operations, no fma.  Nothing here calls the library; the oracle is used for its bf16 conversion and for unpacking the stored codes only; the activation quantiser is
tests/a8_restate.py's."""
import numpy as np

from a8_restate import bf, quant_rows, quant_rows_f32, to_bf  # noqa: F401  (re-exported for the tests)
from oracle import oracle as O


class IntW4:
    """codes minus qBias [M, K] (int64) from the oracle's unpack, and the bf16 group ZERO and STEP as fp32 [M, K / 128]"""

    def __init__(self, ow):
        assert ow.lGroup == 128 and ow.qBias in (0, 8)
        self.M, self.K, self.qBias = ow.ne0, ow.ne1, ow.qBias
        code = O.unpack(ow.data, 4).reshape(self.M, self.K)
        assert code.min() >= 0 and code.max() <= 15
        self.t = (code - ow.qBias).astype(np.int64)
        self.step = bf(ow.step).reshape(self.M, self.K // 128)
        self.zero = bf(ow.zero).reshape(self.M, self.K // 128)


def group_sums(w, q):
    """(I [nTok, M, G], S [nTok, G]) as int64: I_g = sum (code - qBias) * q, S_g = sum q"""
    q = np.atleast_2d(q).astype(np.int64)
    G = w.K // 128
    qg = q.reshape(-1, G, 128)
    # per group a float64 matrix product: every partial sum is an integer below 2^18, so it is exact in any order -- the int64 einsum's values, at BLAS speed
    tg = w.t.reshape(w.M, G, 128).astype(np.float64)
    I = np.stack([qg[:, g].astype(np.float64) @ tg[:, g].T for g in range(G)], axis=2).astype(np.int64)
    S = qg.sum(axis=2)
    assert np.abs(I).max() <= 243840 and np.abs(S).max() <= 16256
    return I, S


def chain(w, q):
    """acc fp32 [nTok, M]: per group p = STEP * I (one rounding), z = ZERO * S (exact), c = p - z, acc = acc + c, g ascending"""
    I, S = group_sums(w, q)
    f32 = np.float32
    acc = np.zeros(I.shape[:2], dtype=f32)
    for g in range(w.K // 128):
        p = (w.step[None, :, g] * I[:, :, g].astype(f32)).astype(f32)
        z = (w.zero[None, :, g] * S[:, None, g].astype(f32)).astype(f32)
        c = (p - z).astype(f32)
        acc = (acc + c).astype(f32)
    return acc


def linear_w4a8(w, q, step, bias=None, residual=None):
    """y [nTok, M] uint16: y = bf16(step_x * acc [+ bias]), then the residual epilogue bf16(residual + bf16(y)) -- as tests/a8_restate.py linear_a8 writes it"""
    acc = chain(w, q)
    v = (np.asarray(step, dtype=np.float32).reshape(-1, 1) * acc).astype(np.float32)
    if bias is not None:
        v = (v + bf(bias)[None, :]).astype(np.float32)
    y = to_bf(v)
    if residual is not None:
        y = to_bf((bf(residual).reshape(y.shape) + bf(y)).astype(np.float32))
    return y


def large_sum_case(M, K, n, seed, qBias=0):
    """(QWeight, q int8 [n, K], step_x fp32 [n]) on a hand-built blob: random codes (high ones under qBias 8), random bf16 STEP and ZERO, activations of one sign near +-127 -- |I_g| reaches 17 and
    18 significant bits, so STEP * I_g does round (random weights against random activations stay below 2^16, where the product is exact and an fma would go unnoticed)"""
    rng = np.random.default_rng(seed)
    G = K // 128
    codes = rng.integers(12 if qBias else 0, 16, (M, K)).astype(np.int32)   # qBias 8: codes 12 .. 15, so that code - qBias keeps one sign too
    step_w = to_bf(rng.uniform(0.01, 0.2, M * G).astype(np.float32))
    zero_w = to_bf(rng.normal(0, 0.3, M * G).astype(np.float32))
    ow = O.QWeight(14, M, K, O.pack(codes, 4), zero_w, step_w, 128, qBias)   # 14 = KF_Q4
    q = rng.integers(90, 128, (n, K)).astype(np.int8)
    q[1::2] = -q[1::2]
    step_x = rng.uniform(1e-3, 2.0, n).astype(np.float32)
    return ow, q, step_x
