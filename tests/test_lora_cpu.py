"""Low-rank adapters without a GPU: the restatement the GPU tests measure against (tests/lora_restate.py) agrees with torch fp64 autograd of y = x (W + s^2 b a)^T;
the symbols are exported and mirrored; the scratch size and the plan are host functions with the properties the kernels rely on; the exact-arithmetic generator holds its
own preconditions at every shape the GPU tests run; the argument errors of the steps come before any context is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from koifish_amd.train_step import GPT2Step, Q3_MATS, Qwen3Step
from tests import lora_restate as R


@pytest.mark.parametrize("r", R.RANKS)
def test_restatement_matches_autograd(r):
    OC, IC, n, s = 192, 128, 64, 0.5
    rng = np.random.default_rng(r)
    W, a, b, x, dIn = (rng.normal(0, sd, sh) for sd, sh in ((0.05, (OC, IC)), (0.1, (r, IC)), (0.1, (OC, r)), (1.0, (n, IC)), (0.02, (n, OC))))
    ax, y = R.lora_forward(a, b, x, x @ W.T, s, rounding=False)
    adelta, delta, g = R.lora_backward(a, b, dIn, x, ax, dIn @ W, np.zeros(r * (IC + OC)), s, rounding=False)
    ta, tb, tx = (torch.tensor(v, requires_grad=True) for v in (a, b, x))
    ty = tx @ (torch.tensor(W) + s * s * (tb @ ta)).T
    (ty * torch.tensor(dIn)).sum().backward()
    close = lambda got, ref: (np.abs(got - ref) <= 1e-12 * np.abs(ref).max()).all()
    assert close(y, ty.detach().numpy())
    assert close(g[:r * IC].reshape(r, IC), ta.grad.numpy()) and close(g[r * IC:].reshape(OC, r), tb.grad.numpy()) and close(delta, tx.grad.numpy())
    # the roundings change something, and only a little
    ax_r, y_r = R.lora_forward(a, b, x, x @ W.T, s)
    assert not np.array_equal(y_r, y) and np.abs(y_r - y).max() <= 2.0 ** -6 * np.abs(y).max()


def test_symbols_exported_and_mirrored():
    hip, host = L.load()
    for f in ("kf_lora_forward", "kf_lora_backward", "kf_lora_backward_scratch_bytes"):
        assert f in L.ABI_SYMBOLS and hasattr(hip, f), f
    assert hip.kf_lora_backward_scratch_bytes.restype is C.c_size_t and len(hip.kf_lora_forward.argtypes) == 11 and len(hip.kf_lora_backward.argtypes) == 14
    for f in ("kfh_qwen3t_set_param_lora", "kfh_qwen3t_set_lora_scratch"):
        assert hasattr(host, f), f


def test_scratch_bytes_on_the_host():
    hip, _ = L.load()
    sb = hip.kf_lora_backward_scratch_bytes
    for r, OC, IC, n in ((8, 128, 128, 64), (24, 128, 128, 64), (128, 256, 256, 64), (16, 64, 128, 64), (16, 128, 192 + 32, 64), (16, 128, 128, 96), (0, 128, 128, 64),
                         (16, 0, 128, 64), (16, 128, 0, 64), (16, 128, 128, 0), (0, 0, 0, 0)):
        assert sb(r, OC, IC, n) == 0, (r, OC, IC, n)
    for OC, IC, n, r, _ in R.EXACT_SHAPES + [(3072, 1024, 8192, 64, 1), (1024, 3072, 8192, 16, 1)]:
        nb = sb(r, OC, IC, n)
        assert nb % 256 == 0 and nb >= n * r * 2, (r, OC, IC, n, nb)
    assert hip.kf_lora_forward(None, None, None, 16, 128, 128, None, None, None, 64, 1.0) == -20   # no context: refused, nothing dereferenced
    assert hip.kf_lora_backward(None, None, None, 16, 128, 128, None, None, None, None, None, 64, 1.0, None) == -20


@pytest.mark.parametrize("shape", [(128, 128, 64, 16), (128, 256, 192, 32), (320, 192, 448, 64), (3072, 1024, 512, 16), (3072, 1024, 8192, 64), (1024, 3072, 8192, 16)])
def test_plan_properties(shape):
    hip, _ = L.load()
    OC, IC, n, r = shape
    p = R.lora_plan(hip, r, OC, IC, n)
    assert p.status == 0 and p.scratch == hip.kf_lora_backward_scratch_bytes(r, OC, IC, n)
    nkt = n // 64
    for S in (p.SA, p.SB):   # the slabs cover [0, n) exactly once, none empty
        cuts = [64 * (nkt * k // S) for k in range(S + 1)]
        assert 1 <= S <= 32 and cuts[0] == 0 and cuts[-1] == n and all(b_ > a_ for a_, b_ in zip(cuts, cuts[1:]))
    assert 0 < p.rows_lds <= 160 * 1024 and 0 < p.w_lds <= 160 * 1024
    assert p.rows_gx * p.tm == n and p.rows_block == 512
    assert p.tilesA * 64 == IC and p.tilesB * 64 == OC and p.w_gx == p.tilesA * p.SA + p.tilesB * p.SB > 0
    assert p.tr_gx * 256 >= r * (IC + OC) and p.fin_gx * 256 >= r * (IC + OC)
    offs = [p.off_adelta, p.off_aT, p.off_bT, p.off_partA, p.off_partB, p.scratch]   # the parts in order, 256-byte aligned, each long enough
    need = [n * r * 2, IC * r * 2, OC * r * 2, p.SA * r * IC * 4, p.SB * OC * r * 4]
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and all(b_ - a_ >= nb for a_, b_, nb in zip(offs, offs[1:], need))
    if shape == (320, 192, 448, 64):
        assert p.SA == 3 and p.SB == 3   # seven k-steps in slabs of 2, 2 and 3: a cut that does not divide evenly
    if shape == (3072, 1024, 8192, 64):
        assert p.rows_gx == 256          # 8192 rows fill the 256 CUs
    refused = R.lora_plan(hip, 24, OC, IC, n)
    assert refused.status == -20 and refused.scratch == 0 and refused.w_gx == 0


@pytest.mark.parametrize("shape", R.EXACT_SHAPES, ids=lambda s: "%dx%dx%d_r%d_s%d" % s)
def test_exact_generator_holds_its_preconditions(shape):
    """lora_exact_case asserts bf16 results and sums below 2^23 itself; here: the results are non-trivial, so that a dropped term shows"""
    c = R.exact_case(shape)
    f = c["f64"]
    for k in ("ax", "adelta"):
        assert 0.5 <= (f[k] != 0).mean() <= 0.99, (k, (f[k] != 0).mean())
    assert max(np.abs(v).max() for v in f.values()) <= 512
    assert not np.array_equal(c["y"], c["y0"]) and not np.array_equal(c["delta"], c["delta0"]) and not np.array_equal(c["g"], c["g0"])


def test_exact_block_case():
    hip, _ = L.load()
    OC, IC, n, r, _ = R.BLOCK_SHAPE
    seam = R.slab_seams(R.lora_plan(hip, r, OC, IC, n), n)[0]
    c = R.exact_case(R.BLOCK_SHAPE, block=True, hip=hip)
    x = R.E.f64(c["x"])
    rows = np.flatnonzero(np.abs(x).sum(1))
    assert len(rows) == 128 and rows[0] == seam - 64 and rows[-1] == seam + 63 and (np.abs(x[rows]) == 1).all() and (np.abs(R.E.f64(c["dIn"])[rows]) == 1).all()


CFG = dict(dim=128, n_layer=2, n_head=4, n_kv=2, head_dim=64, ffn=256, vocab=250, theta=10000.0, rms_eps=1e-6)


def test_argument_errors_come_before_any_context():
    bf = torch.bfloat16
    with pytest.raises(ValueError, match="lora_rank"):
        Qwen3Step(None, CFG, 2, 64, train_target="lora", lora_rank=8)
    with pytest.raises(ValueError, match="lora_rank"):
        Qwen3Step(None, CFG, 2, 64, train_target="lora", lora_rank=64)           # 2 x 64 >= dim 128
    with pytest.raises(ValueError, match="lora_rank"):
        Qwen3Step(None, dict(CFG, dim=256), 2, 64, train_target="lora", lora_rank=128)
    with pytest.raises(ValueError, match="lora_targets"):
        Qwen3Step(None, CFG, 2, 64, train_target="lora", lora_targets=("q", "w"))
    with pytest.raises(ValueError, match="does not take"):
        Qwen3Step(None, CFG, 1, 96, train_target="lora")                          # 96 rows
    with pytest.raises(ValueError, match="does not take"):
        Qwen3Step(None, dict(CFG, ffn=288), 2, 64, train_target="lora")           # ffn no multiple of 64
    with pytest.raises(ValueError, match="adapters"):
        Qwen3Step(None, CFG, 2, 64, train_target="lora", lora_targets=("q",), adapters={"l0.k.w": (torch.zeros(16, 128, dtype=bf), torch.zeros(128, 16, dtype=bf))})
    with pytest.raises(ValueError, match="adapters"):
        Qwen3Step(None, CFG, 2, 64, train_target="lora", adapters={"l0.q.w": (torch.zeros(16, 128, dtype=bf), torch.zeros(128, 16, dtype=bf))})   # q is [256, 128]
    with pytest.raises(ValueError, match="train_target"):
        Qwen3Step(None, CFG, 2, 64, train_target="adapters")
    with pytest.raises(ValueError, match="train_target"):
        GPT2Step(None, 128, 2, 2, 250, 256, 2, 64, train_target="lora")
    assert Qwen3Step._check_lora_args(CFG, 2, 64, 16, 1.0, Q3_MATS, None) == Q3_MATS
