"""The restatement of the fp8-activation arithmetic (include/kf_abi.h "fp8 activations for f8e5m2 layers"), stated ONCE for tests/test_f8a8_cpu.py and the GPU tests.
numpy with torch-CPU for the one e4m3 rounding; nothing here calls the library.  bf / to_bf: the oracle's bf16 conversions (tests/a8_restate.py)."""
import numpy as np
import torch

from a8_restate import bf, to_bf  # noqa: F401  (re-exported for the tests)

E4M3_MAX = 448.0
E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()   # code -> value (0x7f, 0xff: NaN)
E5M2 = np.arange(256, dtype=np.uint16).__lshift__(8).view(np.float16).astype(np.float64)          # stored byte -> value: the high byte of a half


def quant_rows_f32(v):
    """(codes uint8 [rows, dim], step fp32 [rows]) of fp32 rows: e the smallest integer with amax * 2^-e <= 448, step = 2^e, code = e4m3_rne(v * 2^-e); a zero row: step 0"""
    v = np.atleast_2d(np.asarray(v, dtype=np.float32))
    amax = np.abs(v).max(axis=1).astype(np.float64)
    fr, ex = np.frexp(amax)                                  # amax = fr * 2^ex, fr in [0.5, 1); 448 = 0.875 * 2^9
    e = np.where(amax > 0, ex - np.where(fr <= 0.875, 9, 8), 0)
    scaled = np.where(amax[:, None] > 0, np.ldexp(v.astype(np.float64), -e[:, None]), 0.0)   # exact
    assert np.abs(scaled).max(initial=0.0) <= E4M3_MAX
    q = torch.from_numpy(scaled.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, np.where(amax > 0, np.ldexp(1.0, e), 0.0).astype(np.float32)


def quant_rows(x_bf16, norm_w=None, eps=1e-6):
    """the same from bf16 rows (uint16), with the RMSNorm prologue as kf_rmsnorm stores it (the oracle's rmsnorm) when norm_w is given"""
    x = np.atleast_2d(x_bf16)
    if norm_w is not None:
        from oracle import oracle as O
        x = O.rmsnorm(x, norm_w, eps)
    return quant_rows_f32(bf(x))


def product(wbytes, q):
    """acc float64 [nTok, M] = sum_k e4m3(q[t][k]) * e5m2(W[m][k]): every term is exact in float64 and so is any sum of them at the tests' sizes but for the last bits"""
    return E4M3[np.atleast_2d(q)] @ E5M2[wbytes].T


def epilogue(acc, step, bias=None, residual=None):
    """y uint16 [nTok, M] from an fp32 accumulator: bf16(step * acc [+ bias]), then bf16(residual + bf16(y))"""
    v = (np.asarray(step, dtype=np.float32).reshape(-1, 1) * np.asarray(acc, dtype=np.float32)).astype(np.float32)
    if bias is not None:
        v = (v + bf(bias)[None, :]).astype(np.float32)
    y = to_bf(v)
    if residual is not None:
        y = to_bf((bf(residual).reshape(y.shape) + bf(y)).astype(np.float32))
    return y
