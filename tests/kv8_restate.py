"""The numpy restatement of the int8 KV cache arithmetic (include/kf_abi.h "int8 KV cache"), stated ONCE for the test files that need it: tests/test_kv8_cpu.py checks the
properties the definition's exactness claims rest on, tests/test_gpu_kv8.py and tests/test_gpu_kv8_model.py hold the kernels and the model switch to it bit for bit.
float32 / float64 / int64, plain IEEE operations; the one fused multiply-add the definition has (kf_exp2_parts' polynomial) is emulated exactly.  Nothing here calls the
library; the row quantiser is tests/a8_restate.py's (quant_rows) on hd-wide rows."""
import numpy as np

from a8_restate import bf, quant_rows, to_bf  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64
LOG2E = F32(1.44269502162933349609375)


def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 arrays, correctly rounded: the product of two fp32 values is exact in fp64; the fp64 sum with c is made round-to-odd (its error term from
    the two-sum decides the last bit), after which the conversion to fp32 rounds once"""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64) + np.zeros_like(p)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def exp2_parts(y):
    """kf_device.h kf_exp2_parts on fp32 y: n = the nearest integer (ties to even), f = 2^(y - n) from the degree-7 polynomial in fma form"""
    y = np.asarray(y, dtype=F32)
    n = ((y + F32(12582912.0)).astype(F32) - F32(12582912.0)).astype(F32)
    r = (y - n).astype(F32)
    p = np.full(y.shape, F32(1.52527338e-5))
    for coef in (1.54035304e-4, 1.33335581e-3, 9.61812911e-3, 5.55041087e-2, 2.40226507e-1, 6.93147181e-1, 1.0):
        p = fma32(p, r, np.full(y.shape, F32(coef)))
    return p, n


def rden(hd):
    """the value canon_score multiplies by: 1.0f / sqrtf(hd), two correctly rounded fp32 operations"""
    return F32(1.0) / np.sqrt(F32(hd))


def quant_heads(x_u16, hd):
    """bf16 rows [..., n * hd] (uint16) -> (codes int8 of the same shape, steps fp32 [..., n]): quant_rows on every hd-wide head"""
    x = np.asarray(x_u16, dtype=np.uint16)
    q, step = quant_rows(x.reshape(-1, hd))
    return q.reshape(x.shape), step.reshape(x.shape[:-1] + (x.shape[-1] // hd,))


def dequant_heads(q8, step, hd):
    """the dequantised row of the token batches: bf16_rn(fl32(fp32(code) * step)) -> uint16 of q8's shape"""
    q = np.asarray(q8).astype(F32).reshape(-1, hd)
    return to_bf((q * np.asarray(step, dtype=F32).reshape(-1, 1)).astype(F32)).reshape(np.asarray(q8).shape)


def key_terms(q8h, sqh, k8h, ksh, vsh, hd):
    """one query head against keys [T]: (f, n, g) fp32 [T] -- the exact integer dot, three separate fp32 multiplies, the bf16 score, kf_exp2_parts, g = f * VS"""
    I = k8h.astype(np.int64) @ q8h.astype(np.int64)
    assert np.abs(I).max(initial=0) < 2 ** 24
    c = (F32(sqh) * ksh.astype(F32)).astype(F32)
    d = (I.astype(F32) * c).astype(F32)
    s = bf(to_bf((d * rden(hd)).astype(F32)))
    f, n = exp2_parts((s * LOG2E).astype(F32))
    return f, n, (f * vsh.astype(F32)).astype(F32)


def shift(d):
    """canon_shift: the exponent of an exact rescale, clamped so that the scaled value underflows to 0"""
    return np.maximum(d, -1022.0).astype(np.int64)


def partial(f, n, g, v8h):
    """fp64 sums of a run of keys against the run's own maximum exponent: (O [hd], L, m)"""
    m = n.max()
    e = shift(n - m)
    return np.ldexp(g.astype(F64), e) @ v8h.astype(F64), np.ldexp(f.astype(F64), e).sum(), m


def merge(parts):
    """partials (O, L, m) rescaled exactly to their common maximum exponent and summed"""
    M = max(p[2] for p in parts)
    O = sum(np.ldexp(p[0], int(shift(p[2] - M))) for p in parts)
    L = sum(np.ldexp(p[1], int(shift(p[2] - M))) for p in parts)
    return O, L


def attn_decode_kv8(q_u16, k8, ks, v8, vs, pos, n_head, n_kv, hd, slice_keys=0, reverse=False):
    """the decode attention of the definition: q_u16 the normed, roped bf16 query [n_head * hd]; k8 / v8 int8 [T, >= n_kv * hd], ks / vs fp32 [T, n_kv]; keys 0 .. pos.
    slice_keys > 0: the keys in runs of that many, merged as the kernel merges its slices; reverse: the keys in descending order.  -> out uint16 [n_head * hd]"""
    gq = n_head // n_kv
    q8, sq = quant_heads(q_u16, hd)
    order = np.arange(pos + 1)[::-1] if reverse else np.arange(pos + 1)
    out = np.zeros(n_head * hd, dtype=np.uint16)
    for h in range(n_head):
        kvh = h // gq
        cols = slice(kvh * hd, (kvh + 1) * hd)
        k8h, v8h = np.asarray(k8)[order, cols], np.asarray(v8)[order, cols]
        f, n, g = key_terms(q8[h * hd:(h + 1) * hd], sq[h], k8h, np.asarray(ks)[order, kvh], np.asarray(vs)[order, kvh], hd)
        step = slice_keys if slice_keys > 0 else pos + 1
        O, L = merge([partial(f[a:a + step], n[a:a + step], g[a:a + step], v8h[a:a + step]) for a in range(0, pos + 1, step)])
        out[h * hd:(h + 1) * hd] = to_bf((O / L).astype(F32))
    return out


class Cache8:
    """one layer's int8 pair as the library keeps it: zero-filled codes [n_ctx, kv_dim] and steps [n_ctx, n_kv]"""

    def __init__(self, n_ctx, n_kv, hd):
        self.n_kv, self.hd = n_kv, hd
        self.k8 = np.zeros((n_ctx, n_kv * hd), dtype=np.int8)
        self.v8 = np.zeros_like(self.k8)
        self.ks = np.zeros((n_ctx, n_kv), dtype=F32)
        self.vs = np.zeros_like(self.ks)

    def put(self, pos, k_u16, v_u16):
        """rows [n, kv_dim] (or one row) quantised into positions pos .."""
        k_u16, v_u16 = np.atleast_2d(k_u16), np.atleast_2d(v_u16)
        n = k_u16.shape[0]
        self.k8[pos:pos + n], self.ks[pos:pos + n] = quant_heads(k_u16, self.hd)
        self.v8[pos:pos + n], self.vs[pos:pos + n] = quant_heads(v_u16, self.hd)

    def rows(self, n):
        """rows 0 .. n - 1 dequantised: (k, v) uint16 [n, kv_dim]"""
        return dequant_heads(self.k8[:n], self.ks[:n], self.hd), dequant_heads(self.v8[:n], self.vs[:n], self.hd)

    def attend(self, q_u16, pos, n_head):
        return attn_decode_kv8(q_u16, self.k8, self.ks, self.v8, self.vs, pos, n_head, self.n_kv, self.hd)
