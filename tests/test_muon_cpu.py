"""Muon without a GPU: the entries exist and refuse before they touch a device, and the restatement the GPU tests hold the kernels to (tests/muon_restate.py) says what
the issue's arithmetic says -- its stochastic store is the oracle's, and five Newton-Schulz steps bring the singular values of a rectangular random matrix into
[0.6, 1.25] in either summation order."""
import ctypes as C

import numpy as np
import torch

import muon_restate as R
from oracle import oracle as O


def test_entries_are_exported_and_size_the_scratch():
    from koifish_amd import lib as L
    hip, host = L.load()
    for f in ("kf_muon_scratch_bytes", "kf_muon_momentum", "kf_newton_schulz", "kf_muon_apply", "kf_muon"):
        assert f in L.ABI_SYMBOLS and hasattr(hip, f)
    assert hasattr(host, "kfh_gpt2_set_optimizer")
    up = lambda v: (v + 255) & ~255
    for ne0, ne1 in ((64, 64), (320, 192), (6400, 1600)):
        n = ne0 * ne1
        assert hip.kf_muon_scratch_bytes(ne0, ne1) == 2 * up(2 * ne1 * ne1) + 2 * up(2 * n) + up(8 * ((n + 4095) // 4096)) + 256
    for ne0, ne1 in ((64, 128), (96, 64), (128, 96), (0, 0), (64, -64)):
        assert hip.kf_muon_scratch_bytes(ne0, ne1) == 0
    assert hip.kf_muon(None, None, None, None, 64, 64, 0.1, 0.0, 0.95, 1e-7, 5, 1, None, 0, None) == -20   # no context: refused, nothing dereferenced


def test_stochastic_store_is_the_oracles():
    lib = O.lib()
    lib.kfo_noise2d.restype = C.c_uint32
    n = 8 * (512 * 2 + 5)
    thr = R.thresholds(n, 4242)
    for t in (0, 1, 63, 511, 512, 1027, 1028):
        assert int(thr[8 * t]) == lib.kfo_noise2d(t % 512, (t // 512) * 512, 4242) & 0xFFFF and (thr[8 * t: 8 * t + 8] == thr[8 * t]).all()
    x = np.random.default_rng(0).normal(0, 1, 4096).astype(np.float32)
    assert np.array_equal(R.rne_bf16(x), O.f32_to_bf16(x))
    p = O.f32_to_bf16(x)
    assert np.array_equal(R.sr(R.f32(p), thr[:4096]), p)   # a bf16 value has no low bits: the store is exact under any threshold


def test_restated_iteration_orthogonalises():
    g = torch.Generator()
    g.manual_seed(1000 * 320 + 192)
    x = (0.02 * torch.randn(320, 192, generator=g)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).reshape(-1)
    r32 = R.newton_schulz(x, 320, 192, 1e-7, 5, torch.float32)[0]
    r64 = R.newton_schulz(x, 320, 192, 1e-7, 5, torch.float64)[0]
    d0 = float(torch.linalg.norm(r32 - r64) / torch.linalg.norm(r64))
    assert 0.0 < d0 < 0.05
    for m in (r32, r64):
        sv = torch.linalg.svdvals(m)
        assert 0.6 <= float(sv.min()) and float(sv.max()) <= 1.25
    x0 = R.f32(R.prescale(x, R.sumsq(x), 1e-7)).astype(np.float64)
    assert abs(np.sqrt((x0 ** 2).sum()) - 1.0) < 2.0 ** -8   # the pre-scale brings the Frobenius norm to 1 up to the bf16 stores
