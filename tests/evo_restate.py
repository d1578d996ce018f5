"""kf_evolve restated in numpy for the tests (tests/test_evo_cpu.py, tests/test_gpu_evo.py, tests/test_gpu_evo_step.py), bit for bit: the counter-based draw (one
SquirrelNoise5 hash per element, keyed on the flat row-major index and the seed), fp32 arithmetic with every multiply and add rounded on its own, and a
round-to-nearest-even bf16 store.  All tensors are uint16 bf16 bit patterns.  Imports nothing of the package under test."""
import math

import numpy as np

PSO, MIX, PSO_GA = 1, 2, 4   # the live members of Fuyou_params::ALGORITHM
ALGORITHMS = {"pso": PSO, "mix": MIX, "pso_ga": PSO_GA}


def f32(u):
    return (np.asarray(u).astype(np.uint32) << 16).view(np.float32)


def rne_bf16(x):
    """fp32 array -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def squirrel5(pos, seed):
    """SquirrelNoise5 on uint32 arrays (64-bit intermediates masked back to 32 bits)"""
    M = np.uint64(0xFFFFFFFF)
    b = np.asarray(pos, dtype=np.uint64) & M
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


def draw(n, seed):
    """(s3, r, b3) of the n elements: s3 = b0 + b1 + b2 (0 .. 765), r = float32(s3) * float32(1 / 765), b3 = the high byte"""
    h = squirrel5(np.arange(n, dtype=np.uint64), seed)
    s3 = (h & np.uint32(255)) + ((h >> np.uint32(8)) & np.uint32(255)) + ((h >> np.uint32(16)) & np.uint32(255))
    r = s3.astype(np.float32) * (np.float32(1.0) / np.float32(765.0))
    return s3, r, (h >> np.uint32(24)).astype(np.uint32)


def threshold(t_cross):
    return int(min(max(math.floor(float(np.float32(t_cross)) * 256.0 + 0.5), 0), 256))


def evolve(x, head, algorithm, alpha=0.9, social=2.0, t_cross=0.6, seed=0):
    """x, head: uint16 arrays of one shape.  Returns the new x (the argument is not modified)."""
    algorithm = ALGORITHMS.get(algorithm, algorithm)
    shape = np.asarray(x).shape
    xb, gb = np.asarray(x, dtype=np.uint16).reshape(-1), np.asarray(head, dtype=np.uint16).reshape(-1)
    xf, gf = f32(xb), f32(gb)
    if algorithm == MIX:
        a = np.float32(alpha)
        beta = np.float32(1.0 - float(a))
        return rne_bf16((a * xf).astype(np.float32) + (beta * gf).astype(np.float32)).reshape(shape)
    assert algorithm in (PSO, PSO_GA), algorithm
    s3, r, b3 = draw(xb.size, seed)
    t = (np.float32(social) * r).astype(np.float32)
    d = (gf - xf).astype(np.float32)
    td = (t * d).astype(np.float32)
    out = np.where(s3 != 0, rne_bf16((xf + td).astype(np.float32)), xb)
    if algorithm == PSO_GA:
        out = np.where(b3 < threshold(t_cross), gb, out)
    return out.astype(np.uint16).reshape(shape)
