"""NOT a test module: the numpy restatement of kf_distill_classifier's stated order of operations (include/kf_abi.h), thread by thread, vectorised over rows and
over the 1024 threads of a row's workgroup.  Independent of the kernel's code and of oracle/: the fixed exp / log recipes are stated again here on arrays
(tests/test_distill_cpu.py pins them to the oracle's scalar ones bit for bit), an fma is an exact float64 product and a sum rounded to odd, then rounded once to
float32.  Everything else is float32 numpy arithmetic, which is IEEE round-to-nearest-even, one rounding per operation -- what the kernel's instructions do."""
import numpy as np

f32, f64 = np.float32, np.float64
NTHREADS = 1024
IGNORE = 0x10000


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(f32)


def f32_to_bf16(x):
    """round to nearest even; NaN stays NaN (quiet)"""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + (0x7fff + ((u >> 16) & 1))) >> 16).astype(np.uint16)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def fma(a, b, c):
    """float32 fma(a, b, c) on arrays: a * b is exact in float64; the float64 sum is rounded to odd (TwoSum gives its error exactly), so the final rounding to
    float32 is the single rounding of the exact a * b + c (53 >= 24 + 2 bits)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p, c = a.astype(f64) * b.astype(f64), c.astype(f64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.view(np.uint64) if s.ndim else np.array(s).view(np.uint64)
    fix = (err != 0) & ((bits & np.uint64(1)) == 0) & np.isfinite(s)
    grow = (err > 0) == (s > 0)   # the exact sum lies further from zero than s
    bits = np.where(fix, np.where(grow, bits + np.uint64(1), bits - np.uint64(1)), bits)
    return bits.view(f64).astype(f32)


def expf(x):
    """the fixed fp32 exp (Cody-Waite reduction, degree-7 Taylor in Horner / fma form, two-step power-of-two scaling) on an array"""
    x = np.asarray(x, dtype=f32)
    hi, lo, nan = x > f32(88.72283), x < f32(-87.33654), x != x
    xs = np.where(hi | lo | nan, f32(0), x)
    t = xs * f32(1.44269502162933349609375)
    n = (t + f32(12582912.0)) - f32(12582912.0)
    r = fma(n, f32(-0.693145751953125), xs)
    r = fma(n, f32(-1.428606765330187045e-06), r)
    p = np.full_like(xs, f32(1.98412701138295233249664306640625e-4))
    for c in (1.38888892251998186111450195312500e-3, 8.33333376795053482055664062500000e-3, 4.16666679084300994873046875000000e-2,
              1.66666671633720397949218750000000e-1, 0.5, 1.0, 1.0):
        p = fma(p, r, f32(c))
    e = n.astype(np.int32)
    e1 = np.sign(e) * (np.abs(e) // 2)   # C's e / 2: towards zero
    e2 = e - e1
    s1 = ((e1 + 127).astype(np.uint32) << 23).view(f32)
    s2 = ((e2 + 127).astype(np.uint32) << 23).view(f32)
    y = (p * s1) * s2
    y = np.where(hi, f32(np.inf), np.where(lo, f32(0), y))
    return np.where(nan, x, y).astype(f32)


def logf(x):
    """the fixed fp32 natural log of the cross-entropy loss on an array"""
    x = np.atleast_1d(np.asarray(x, dtype=f32)).copy()
    bad, zero, inf = (x != x) | (x < 0), x == 0, x == np.inf
    xs = np.where(bad | zero | inf, f32(1), x)
    u = xs.view(np.uint32)
    sub = u < 0x00800000
    xs = np.where(sub, np.where(sub, xs, f32(1)) * f32(8388608.0), xs)
    e = np.where(sub, -23, 0).astype(np.int32)
    u = xs.view(np.uint32)
    e = e + (u >> 23).astype(np.int32) - 127
    m = ((u & 0x007fffff) | 0x3f800000).view(f32)
    big = m > f32(1.41421353816986083984375)
    m = np.where(big, m * f32(0.5), m)
    e = e + big.astype(np.int32)
    f = m - f32(1)
    s = f / (f32(2) + f)
    z = s * s
    p = np.full_like(z, f32(9.0909093618392944336e-2))
    for c in (1.1111111193895339966e-1, 1.4285714924335479736e-1, 2.0000000298023223877e-1, 3.3333334326744079590e-1):
        p = fma(p, z, f32(c))
    s2 = s + s
    fe = e.astype(f32)
    lo = fma(s2 * z, p, fe * f32(9.058001351536227e-6))
    y = fma(fe, f32(6.9313812255859375e-1), s2 + lo)
    y = np.where(zero, f32(-np.inf), np.where(inf, f32(np.inf), y))
    return np.where(bad, f32(np.nan), y).astype(f32)


def _butterfly(v, is_max):
    """[..., 32] -> [...]: xor butterfly, offsets 16, 8, 4, 2, 1; every lane ends with the same value"""
    lane = np.arange(32)
    for off in (16, 8, 4, 2, 1):
        o = v[..., lane ^ off]
        v = np.maximum(v, o) if is_max else v + o
    return v[..., 0]


def block_reduce(v, is_max):
    """[rows, 1024] -> [rows]: the butterfly inside each group of 32 consecutive threads, then over the 32 group results"""
    return _butterfly(_butterfly(v.reshape(v.shape[0], 32, 32), is_max), is_max)


def _visits(V):
    """yields (e [1024] int, valid [1024] bool): the element every thread visits at each step of its chain -- vectors ceil(V/8) + t - 1024, - 1024, ... highest first,
    the elements of a vector ascending"""
    nv = (V + 7) // 8
    t = np.arange(NTHREADS)
    for j in range((nv + NTHREADS - 1) // NTHREADS):
        i = nv + t - NTHREADS * (j + 1)
        for k in range(8):
            e = i * 8 + k
            valid = (i >= 0) & (e < V)
            yield np.where(valid, e, 0), valid


def distill_classifier(logits, teacher, losses, targets, V, dloss, ce_weight, kd_weight, temperature, mask=None, write_dlogits=True):
    """logits uint16 [rows, P], teacher uint16 [rows, ld] or None (kd_weight == 0), losses float32 [rows], targets int [rows] or None (ce_weight == 0).
    Returns (losses, kd, logits) as new arrays: the accumulated losses, the KL rows (zeros where the kernel writes none) and the rows with the gradient bits over
    their first V columns; masked rows and padding columns as they came."""
    logits, losses = np.array(logits, dtype=np.uint16), np.array(losses, dtype=f32)
    rows = logits.shape[0]
    a, b, tau, dloss = f32(ce_weight), f32(kd_weight), f32(temperature), f32(dloss)
    ce, kd_on = a != 0, b != 0
    it = f32(1) / tau
    live = np.ones(rows, bool) if mask is None else (np.asarray(mask) & IGNORE) == 0
    z = bf16_to_f32(logits[:, :V])
    u = bf16_to_f32(np.asarray(teacher)[:, :V]) if kd_on else None
    ninf = f32(-np.inf)
    with np.errstate(all="ignore"):
        # 1. the fused classifier's running (max, sum) per thread; the teacher's running max
        tmax, tsum, umax = np.full((rows, NTHREADS), ninf), np.zeros((rows, NTHREADS), f32), np.full((rows, NTHREADS), ninf)
        for e, valid in _visits(V):
            v = z[:, e]
            new = valid & (v > tmax)
            resc = new & (tmax != ninf)
            tsum = np.where(resc, tsum * expf(np.where(resc, tmax - v, f32(0))), tsum)
            tmax = np.where(new, v, tmax)
            tsum = np.where(valid, tsum + expf(np.where(valid, v - tmax, f32(0))), tsum)
            if kd_on:
                umax = np.where(valid, np.maximum(umax, u[:, e]), umax)
        mz = block_reduce(tmax, True)
        tsum = tsum * expf(tmax - mz[:, None])
        r1 = f32(1) / block_reduce(tsum, False)
        kl = np.zeros(rows, f32)
        if kd_on:
            # 2. both temperature sums and A through one chain and one tree
            mu = block_reduce(umax, True)
            st, ut, at = (np.zeros((rows, NTHREADS), f32) for _ in range(3))
            for e, valid in _visits(V):
                dz, du = z[:, e] - mz[:, None], u[:, e] - mu[:, None]
                eu = expf(du * it)
                st = np.where(valid, st + expf(dz * it), st)
                ut = np.where(valid, ut + eu, ut)
                at = np.where(valid, fma(eu, (du - dz) * it, at), at)
            St, Ut, At = block_reduce(st, False), block_reduce(ut, False), block_reduce(at, False)
            kl = (At / Ut - logf(Ut)) + logf(St)
            rt, ru = f32(1) / St, f32(1) / Ut
        # 3. the loss
        c = np.zeros(rows, f32)
        ix = np.full(rows, -1, dtype=np.int64)
        if ce:
            ix = np.asarray(targets).astype(np.int64)
            zt = z[np.arange(rows), np.where(live, ix, 0)]
            c = a * -logf(expf(zt - mz) * r1)
        if kd_on:
            w = (b * tau) * tau
            c = fma(np.full(rows, w), kl, c) if ce else w * kl
        losses = np.where(live, losses + c, losses).astype(f32)
        kd = np.where(live & kd_on, kl, f32(0)).astype(f32)
        # 4. the gradient over the logits
        if write_dlogits:
            dz = z - mz[:, None]
            g = np.zeros_like(z)
            if ce:
                onehot = (np.arange(V)[None, :] == ix[:, None]).astype(f32)
                g = a * (expf(dz) * r1[:, None] - onehot)
            if kd_on:
                g = fma(np.full_like(z, b * tau), expf(dz * it) * rt[:, None] - expf((u - mu[:, None]) * it) * ru[:, None], g)
            gb = f32_to_bf16(g * dloss)
            logits[:, :V] = np.where(live[:, None], gb, logits[:, :V])
    return losses, kd, logits


def reference64(logits, teacher, targets, V, ce_weight, kd_weight, temperature):
    """the objective in float64, closed form (checked against torch fp64 autograd in tests/test_distill_cpu.py): a dict of per-row CE, KL, A / Ut, log Ut, log St
    and per-element p, pt, qt, and the gradient per unit dloss"""
    z = bf16_to_f32(np.asarray(logits)[:, :V]).astype(f64)
    rows = z.shape[0]
    tau = float(temperature)
    zz = z - z.max(1, keepdims=True)
    p = np.exp(zz) / np.exp(zz).sum(1, keepdims=True)
    out = dict(p=p, pt=np.zeros_like(p), qt=np.zeros_like(p), kl=np.zeros(rows), a_over_u=np.zeros(rows), log_u=np.zeros(rows), log_s=np.zeros(rows), ce=np.zeros(rows))
    g = np.zeros_like(p)
    if ce_weight != 0:
        ix = np.asarray(targets).astype(np.int64)
        out["ce"] = -np.log(p[np.arange(rows), ix])
        oh = np.zeros_like(p)
        oh[np.arange(rows), ix] = 1.0
        g = ce_weight * (p - oh)
    if kd_weight != 0:
        u = bf16_to_f32(np.asarray(teacher)[:, :V]).astype(f64)
        uu = u - u.max(1, keepdims=True)
        es, eu = np.exp(zz / tau), np.exp(uu / tau)
        S, U = es.sum(1), eu.sum(1)
        A = (eu * (uu - zz) / tau).sum(1)
        out.update(pt=es / S[:, None], qt=eu / U[:, None], a_over_u=A / U, log_u=np.log(U), log_s=np.log(S))
        out["kl"] = A / U - np.log(U) + np.log(S)
        g = g + kd_weight * tau * (out["pt"] - out["qt"])
    out["g"] = g
    out["loss"] = ce_weight * out["ce"] + kd_weight * tau * tau * out["kl"]
    return out
