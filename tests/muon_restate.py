"""The Muon update restated for the tests (tests/test_gpu_muon.py, tests/test_gpu_muon_step.py): the two elementwise kernels in numpy, bit for bit (the seeded
stochastic bf16 store stated as tests/test_oracle_adamw.py's oracle states it: SquirrelNoise5 keyed on the TASKA_1p1 geometry, one 16-bit threshold per thread),
and the Newton-Schulz iteration in torch on the CPU with a bf16 store at every point where the device stores one."""
import numpy as np
import torch

A_, B_, C_ = 3.4445, -4.7750, 2.0315   # Pipe.hpp:131


def f32(u):
    return (np.asarray(u).astype(np.uint32) << 16).view(np.float32)


def rne_bf16(x):
    """fp32 array -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def squirrel5(pos, seed):
    b = np.asarray(pos, dtype=np.uint64) & 0xFFFFFFFF
    M = np.uint64(0xFFFFFFFF)
    b = (b * np.uint64(0xd2a80a3f)) & M
    b = (b + np.uint64(seed & 0xFFFFFFFF)) & M
    b ^= b >> np.uint64(9)
    b = (b + np.uint64(0xa884f197)) & M
    b ^= b >> np.uint64(11)
    b = (b * np.uint64(0x6C736F4B)) & M
    b ^= b >> np.uint64(13)
    b = (b + np.uint64(0xB79F3ABB)) & M
    b ^= b >> np.uint64(15)
    b = (b * np.uint64(0x1b56c4f5)) & M
    b ^= b >> np.uint64(17)
    return b.astype(np.uint32)


def thresholds(n, seed):
    """per ELEMENT: thread t = element // 8, threadIdx = t % 512, block = t // 512: noise(threadIdx + 198491317 * (block * 512), seed) & 0xFFFF"""
    t = np.arange(n // 8, dtype=np.uint64)
    pos = (t % 512) + np.uint64(198491317) * ((t // 512) * 512)
    return np.repeat(squirrel5(pos, seed) & np.uint32(0xFFFF), 8)


def sr(x, thr):
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    u = np.where((u & 0xFFFF) > thr, u | np.uint32(0xFFFF), u & np.uint32(0xFFFF0000)).astype(np.uint32)
    return rne_bf16(u.view(np.float32))


def momentum(mG, g, mui, seed):
    """CU_muon_mG: returns (mG', X) bit patterns; every product and sum a separate fp32 operation"""
    thr = thresholds(mG.size, seed)
    m, gg = f32(mG), f32(g)
    s1, mu = np.float32(1.0) - np.float32(mui), np.float32(mui)
    m2 = sr(m + s1 * (gg - m), thr)
    x = sr(gg + mu * (f32(m2) - gg), thr)
    return m2, x


def apply(p, x, lr, wd, seed):
    """CU_muon_update: p' bit patterns"""
    thr = thresholds(p.size, seed)
    s1, s2 = np.float32(1.0) - np.float32(lr) * np.float32(wd), -np.float32(lr)
    return sr(s1 * f32(p) + s2 * f32(x), thr)


def sumsq(u):
    return float(np.sum(f32(u).astype(np.float64) ** 2))


def alpha_minus_1(ss, eps):
    """alpha in fp64, narrowed to float, then the 1 taken off in float (Optimizer.cu:522-530)"""
    return np.float32(1.0 / (np.sqrt(np.float64(ss)) + np.float64(np.float32(eps)))) - np.float32(1.0)


def prescale(x_u16, ss, eps):
    x = f32(x_u16)
    return rne_bf16(x + alpha_minus_1(ss, eps) * x)


def newton_schulz(x_u16, ne0, ne1, eps, n_iter, dtype, a=A_, b=B_, c=C_):
    """torch on the CPU, products summed in `dtype` (float32 or float64), a bf16 store wherever the device stores one: the pre-scaled X, A, c A A, B, X B, X'.
    Returns (X [ne0, ne1] as float64 tensor of bf16 values, A, B of the last iteration)."""
    bf = lambda t: t.to(torch.float32).to(torch.bfloat16).to(dtype)
    f = lambda v: torch.tensor(float(np.float32(v)), dtype=torch.float32)
    X = torch.from_numpy(f32(prescale(x_u16, sumsq(x_u16), eps)).reshape(ne0, ne1).copy()).to(dtype)
    A = Bm = None
    for _ in range(n_iter):
        A = bf(X.T @ X)
        AA = bf(f(c) * (A @ A).to(torch.float32))
        Bm = bf(f(b) * A.to(torch.float32) + AA.to(torch.float32))
        XB = bf(X @ Bm)
        X = bf(f(a) * X.to(torch.float32) + XB.to(torch.float32))
    return X.to(torch.float64), A, Bm
