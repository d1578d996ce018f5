"""kf_grad_norms restated for the tests (tests/test_gradnorm_cpu.py, tests/test_gpu_gradnorm.py, tests/test_gpu_clip_step.py): the summation order of
include/kf_abi.h "gradient norms" in numpy, bit for bit, and the narrowing and division rules of the three clip modes.  Not a test.

Every addition is one fp64 numpy operation; the square of a bf16 value is exact in fp64 (16 significant bits at most), so fma(x, x, ss) is ss + x * x."""
import numpy as np

from muon_restate import f32

CHUNK, T, EPT = 4096, 512, 8
REPORT, TENSOR, GLOBAL = 1, 2, 3   # enum kf_clip_mode


def sq(u16):
    """the exact squares of bf16 bit patterns, fp64 (muon_restate.sumsq's terms before it adds them)"""
    return f32(u16).astype(np.float64) ** 2


def chunk_partials(u16):
    """one fp64 partial per 4096-element chunk: thread t of a chunk adds its 8 squares in element order from 0 (a thread at or past n holds 0); the 64 lanes of a
    wave in six pairwise levels of adjacent blocks; the 8 waves in wave order from 0"""
    n = u16.size
    assert n >= 8 and n % 8 == 0
    nch = (n + CHUNK - 1) // CHUNK
    s = np.zeros(nch * CHUNK, np.float64)
    s[:n] = sq(u16.reshape(-1))
    s = s.reshape(nch, T, EPT)
    th = np.zeros((nch, T), np.float64)
    for e in range(EPT):
        th = th + s[:, :, e]
    w = th.reshape(nch, T // 64, 64)
    for _ in range(6):
        w = w[:, :, 0::2] + w[:, :, 1::2]
    w = w[:, :, 0]
    tot = np.zeros(nch, np.float64)
    for k in range(T // 64):
        tot = tot + w[:, k]
    return tot


def sum_partials(p):
    """muon_sum_kernel's order: 256 contiguous runs of ceil(np / 256) partials, each added in order from 0, then the runs in order from 0"""
    np_ = p.size
    per = (np_ + 255) // 256
    a = np.zeros(256 * per, np.float64)
    a[:np_] = p   # + 0.0 where a run is short or empty: exact
    a = a.reshape(256, per)
    runs = np.zeros(256, np.float64)
    for j in range(per):
        runs = runs + a[:, j]
    tot = np.float64(0.0)
    for r in runs:
        tot = tot + r
    return tot


def tensor_sumsq(u16):
    return sum_partials(chunk_partials(u16))


def norms(tensors):
    """tensors: list of bf16 bit-pattern arrays -> (sumsq fp64 [n + 1], gnorm fp32 [n + 1]); the last entry is the whole list's: the per-tensor sums added in
    tensor order from 0.  gnorm = (float)sqrt(sumsq): the root in fp64, narrowed once."""
    ss = np.zeros(len(tensors) + 1, np.float64)
    tot = np.float64(0.0)
    for i, t in enumerate(tensors):
        ss[i] = tensor_sumsq(np.asarray(t).reshape(-1))
        tot = tot + ss[i]
    ss[-1] = tot
    with np.errstate(invalid="ignore"):
        gn = np.sqrt(ss).astype(np.float32)
    return ss, gn


def scales(gnorm, mode, gclip, no_clip=None):
    """scale fp32 [n]: the comparison is > (a norm equal to gclip is not scaled), the division fp32; NaN compares false (1.0), +inf gives 0.0"""
    n = gnorm.size - 1
    c = np.float32(gclip)
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == REPORT:
            s = np.full(n, one, np.float32)
        elif mode == TENSOR:
            g = gnorm[:n].astype(np.float32)
            s = np.where(g > c, c / np.where(g > c, g, one), one).astype(np.float32)
        elif mode == GLOBAL:
            g = np.float32(gnorm[n])
            s = np.full(n, c / g if g > c else one, np.float32)
        else:
            raise ValueError(mode)
    if no_clip is not None:
        s = np.where(np.asarray(no_clip, bool), one, s).astype(np.float32)
    return s
