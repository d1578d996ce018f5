"""Gradient norms and clipping without a GPU: the table kf::gradnorm_plan lays out (kfdbg_gradnorm_plan), the refusals of the three kf_grad_norms* entries and of the
trainers' set_grad_clip that return before they touch a device (the context is a zeroed buffer, as in tests/test_trainers_cpu.py), and the restatement the GPU tests
hold the kernels to (tests/gradnorm_restate.py) against a plain fp64 sum."""
import ctypes as C

import numpy as np
import pytest

import gradnorm_restate as G
from koifish_amd import lib as L
from tests import exact_inputs as E
from tests.test_trainers_cpu import TRAINERS, _fake_ctx

INVALID_ARGS = -20
SIZES = [8, 4088, 4096, 4104, 3 * 4096 + 8]
up256 = lambda v: (v + 255) & ~255


def _plan(hip, sizes):
    n = (C.c_longlong * len(sizes))(*sizes)
    p = L.GradNormPlan()
    total = sum((s + 4095) // 4096 for s in sizes)
    wg0 = (C.c_int * (len(sizes) + 1))()
    owner = (C.c_int * max(total, 1))()
    assert hip.kfdbg_gradnorm_plan(len(sizes), n, C.byref(p), wg0, owner) == 0
    return p, list(wg0), list(owner)[:total]


def test_plan_table_and_lookup():
    hip, _ = L.load()
    p, wg0, owner = _plan(hip, SIZES)
    assert p.status == 0 and p.n_tensors == 5
    assert wg0 == [0, 1, 2, 3, 5, 9] and p.total_wg == 9   # 8, 4088, 4096: one chunk each; 4104: two; 3 x 4096 + 8: four
    assert owner == [0, 1, 2, 3, 3, 4, 4, 4, 4]
    # every workgroup's lookup lands in its tensor, on a longer list too (a binary search over more than a few levels)
    rng = np.random.default_rng(5)
    sizes = [int(8 * rng.integers(1, 3000)) for _ in range(301)]
    p, wg0, owner = _plan(hip, sizes)
    assert wg0[0] == 0 and all(wg0[i + 1] - wg0[i] == (sizes[i] + 4095) // 4096 for i in range(len(sizes))) and p.total_wg == wg0[-1]
    assert all(wg0[owner[w]] <= w < wg0[owner[w] + 1] for w in range(p.total_wg))
    # the layout: the table (24 bytes a row, one sentinel row), then one fp64 partial per chunk, both rounded up to 256
    assert p.off_table == 0 and p.off_part == up256(24 * (len(sizes) + 1)) and p.bytes == p.off_part + up256(8 * p.total_wg)


def test_scratch_bytes_grow_with_the_list():
    hip, _ = L.load()
    sb = lambda sizes: hip.kf_grad_norms_scratch_bytes(len(sizes), (C.c_longlong * max(len(sizes), 1))(*sizes))
    got = [sb(SIZES[:k]) for k in range(1, len(SIZES) + 1)]
    assert got == [up256(24 * (k + 1)) + up256(8 * sum((s + 4095) // 4096 for s in SIZES[:k])) for k in range(1, len(SIZES) + 1)]
    assert sb([1 << 20] * 40) > sb([1 << 20] * 20) > sb([1 << 20]) >= got[0] > 0
    assert sb([1 << 20] * 40) == up256(24 * 41) + up256(8 * 40 * 256)
    # lists the entries refuse
    assert sb([]) == 0 and sb([8, 12]) == 0 and sb([0]) == 0 and sb([-8]) == 0
    assert hip.kf_grad_norms_scratch_bytes(1, None) == 0


def test_entries_refuse_before_they_touch_a_device():
    hip, _ = L.load()
    for f in ("kf_grad_norms_scratch_bytes", "kf_grad_norms_plan", "kf_grad_norms", "kf_grad_norms_forget", "kf_adamw_scaled"):
        assert f in L.ABI_SYMBOLS and hasattr(hip, f)
    keep, ctx = _fake_ctx()
    why = lambda: hip.kf_last_error().decode()
    mem = C.create_string_buffer(1 << 16)
    base = up256(C.addressof(mem))
    P = lambda off=0: C.c_void_p(base + off)
    n2 = (C.c_longlong * 2)(16, 4096)
    g2 = (C.c_void_p * 2)(base + 1024, base + 2048)
    sc, nb = P(8192), hip.kf_grad_norms_scratch_bytes(2, n2)
    plan = lambda *a: hip.kf_grad_norms_plan(*a)
    assert plan(None, 2, g2, n2, None, sc, nb) == INVALID_ARGS                                  # no context
    assert plan(ctx, 0, g2, n2, None, sc, nb) == INVALID_ARGS and "n_tensors" in why()
    assert plan(ctx, 4097, g2, n2, None, sc, nb) == INVALID_ARGS and "n_tensors" in why()   # above the cap: refused before the lists are read
    assert hip.kf_grad_norms_scratch_bytes(4097, (C.c_longlong * 4097)(*([8] * 4097))) == 0 < hip.kf_grad_norms_scratch_bytes(4096, (C.c_longlong * 4096)(*([8] * 4096)))
    assert hip.kf_grad_norms_forget(None, sc) == INVALID_ARGS and hip.kf_grad_norms_forget(ctx, sc) == 0   # nothing remembered: nothing to do
    assert plan(ctx, 2, None, n2, None, sc, nb) == INVALID_ARGS and "null" in why()
    assert plan(ctx, 2, g2, None, None, sc, nb) == INVALID_ARGS and "null" in why()
    for bad in (12, 0, -8):
        assert plan(ctx, 2, g2, (C.c_longlong * 2)(16, bad), None, sc, nb) == INVALID_ARGS and "n[1]" in why() and "multiple of 8" in why()
    assert plan(ctx, 2, (C.c_void_p * 2)(base + 1024, None), n2, None, sc, nb) == INVALID_ARGS and "grads[1] is null" in why()
    assert plan(ctx, 2, (C.c_void_p * 2)(base + 1024, base + 2048 + 8), n2, None, sc, nb) == INVALID_ARGS and "grads[1] is not 16-byte aligned" in why()
    assert plan(ctx, 2, g2, n2, None, None, nb) == INVALID_ARGS and "scratch" in why()
    assert plan(ctx, 2, g2, n2, None, P(8192 + 128), nb) == INVALID_ARGS and "256-byte aligned" in why()
    assert plan(ctx, 2, g2, n2, None, sc, nb - 1) == INVALID_ARGS and "kf_grad_norms_scratch_bytes" in why()
    # kf_grad_norms
    out = (P(16384), P(16384 + 256), P(16384 + 512))
    run = lambda *a: hip.kf_grad_norms(*a)
    assert run(None, sc, 2, G.TENSOR, 1.0, *out) == INVALID_ARGS
    assert run(ctx, None, 2, G.TENSOR, 1.0, *out) == INVALID_ARGS and "null" in why()
    for k in range(3):
        o = list(out)
        o[k] = None
        assert run(ctx, sc, 2, G.TENSOR, 1.0, *o) == INVALID_ARGS and "null" in why()
    assert run(ctx, sc, 0, G.TENSOR, 1.0, *out) == INVALID_ARGS and "n_tensors" in why()
    assert run(ctx, P(8192 + 64), 2, G.TENSOR, 1.0, *out) == INVALID_ARGS and "256-byte aligned" in why()
    assert run(ctx, sc, 2, G.TENSOR, 1.0, P(16384 + 4), out[1], out[2]) == INVALID_ARGS and "misaligned" in why()
    for mode in (0, 4, -1):
        assert run(ctx, sc, 2, mode, 1.0, *out) == INVALID_ARGS and "mode" in why()
    for mode in (G.TENSOR, G.GLOBAL):
        for c in (0.0, -1.0, float("nan"), float("inf")):
            assert run(ctx, sc, 2, mode, c, *out) == INVALID_ARGS and "gclip" in why()
    assert run(ctx, sc, 2, G.REPORT, 0.0, *out) == INVALID_ARGS and "kf_grad_norms_plan first" in why()   # report takes any gclip; the scratch was never planned
    # kf_adamw_scaled: kf_adamw's refusals, and the scale pointer
    t = P(1024)
    ad = lambda p, s, n=16: hip.kf_adamw_scaled(ctx, p, t, t, t, n, L.BF16, 1e-3, 0.9, 0.95, 0.1, 0.05, 1e-8, 0.0, s, 1, None)
    assert ad(t, None) == INVALID_ARGS and "null" in why()
    assert ad(None, t) == INVALID_ARGS
    assert ad(t, t, 12) == INVALID_ARGS
    assert ad(t, P(1024 + 2)) != 0 and "4-byte" in why()
    del keep


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_set_grad_clip_refusals(which):
    _, host = L.load()
    family, create, n_params = TRAINERS[which]
    f = lambda name: getattr(host, "kfh_%s_%s" % (family, name))
    why = lambda: f("last_error")().decode()
    keep, ctx = _fake_ctx()
    h = create(host, ctx)
    mem = C.create_string_buffer(1 << 16)
    base = up256(C.addressof(mem))
    sc = C.c_void_p(base + 4096)
    out = (C.c_float * (n_params + 1))()
    try:
        # an unregistered trainer: no byte count, no table; off is accepted with no scratch
        assert f("grad_clip_scratch_bytes")(h) == 0
        assert f("set_grad_clip")(h, L.CLIP_TENSOR, 1.0, sc, 1 << 15) == INVALID_ARGS and "registered" in why()
        assert f("set_grad_clip")(h, L.CLIP_OFF, 1.0, None, 0) == 0
        p = C.c_void_p(base)
        for i in range(n_params):
            assert f("set_param")(h, i, p, p, p, p, 16, 0, None, 0) == 0
        nb = f("grad_clip_scratch_bytes")(h)
        n16 = (C.c_longlong * n_params)(*([16] * n_params))
        assert nb == L.load()[0].kf_grad_norms_scratch_bytes(n_params, n16) + up256(8 * (n_params + 1)) + up256(4 * (n_params + 1)) + up256(4 * n_params)
        for mode in (4, -1, 17):
            assert f("set_grad_clip")(h, mode, 1.0, sc, nb) == INVALID_ARGS and "mode" in why()
        for mode in (L.CLIP_TENSOR, L.CLIP_GLOBAL):
            for c in (0.0, -0.5, float("nan")):
                assert f("set_grad_clip")(h, mode, c, sc, nb) == INVALID_ARGS and "gclip" in why()
        for mode in (L.CLIP_REPORT, L.CLIP_TENSOR, L.CLIP_GLOBAL):
            assert f("set_grad_clip")(h, mode, 1.0, None, nb) == INVALID_ARGS and "scratch" in why()
            assert f("set_grad_clip")(h, mode, 1.0, C.c_void_p(base + 4096 + 16), nb) == INVALID_ARGS and "256-byte" in why()
            assert f("set_grad_clip")(h, mode, 1.0, sc, nb - 1) == INVALID_ARGS and "shorter" in why()
        assert f("set_grad_clip")(h, L.CLIP_OFF, 0.0, None, 0) == 0 and why() == ""
        # no norms to read while clipping is off
        assert f("grad_norms")(h, out, n_params + 1) == INVALID_ARGS and "set_grad_clip" in why()
    finally:
        f("destroy")(h)
    del keep


def test_restatement_is_exact_where_every_order_is():
    """inputs from the exact grid (small integers and halves: tests/exact_inputs.py): every partial sum is an fp64 value, so the stated order and numpy's agree bit for bit"""
    rng = np.random.default_rng(11)
    for n in (8, 4088, 4104, 3 * 4096 + 8, 1 << 18):
        for x in (E.small_ints(rng, n, 8), E.ternary(rng, n, 0.5, twos=True), E.small_ints(rng, n, 16) / 2):
            u = E.exact_bits(x)
            assert G.tensor_sumsq(u) == np.sum(E.f64(u) ** 2) == np.sum(x * x)
    ss, gn = G.norms([E.exact_bits(np.full(16, 0.25)), E.exact_bits(np.zeros(8)), E.exact_bits(np.full(8, 3.0))])
    assert ss.tolist() == [1.0, 0.0, 72.0, 73.0] and gn.tolist() == [1.0, 0.0, float(np.float32(np.sqrt(72.0))), float(np.float32(np.sqrt(73.0)))]


def test_restatement_close_to_a_plain_sum_on_random_bf16():
    """non-negative terms: any summation order of n terms is within n 2^-53 relative of the exact sum; 2^-30 leaves margin at n <= 2^22"""
    rng = np.random.default_rng(12)
    for n in (4104, 1 << 16, (1 << 20) + 8, 1 << 22):
        x = (rng.normal(0, 1, n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
        u = E.bits(x)
        ref = np.sum(E.f64(u) ** 2)
        got = G.tensor_sumsq(u)
        assert abs(got - ref) <= 2.0 ** -30 * ref, (n, got, ref)


def test_scale_rules():
    gn = np.array([0.5, 1.0, 2.0, np.inf, np.nan, 0.0, 3.0], np.float32)
    one = np.float32(1.0)
    assert (G.scales(gn, G.REPORT, 1.0) == one).all()
    s = G.scales(gn, G.TENSOR, 1.0)
    assert s.dtype == np.float32 and s.tolist() == [1.0, 1.0, 0.5, 0.0, 1.0, 1.0]   # > and not >=; +inf -> 0; NaN compares false
    assert G.scales(gn, G.GLOBAL, 1.0).tolist() == [float(one / np.float32(3.0))] * 6
    assert G.scales(gn, G.GLOBAL, 4.0).tolist() == [1.0] * 6
    assert G.scales(gn, G.TENSOR, 1.0, no_clip=[0, 0, 1, 1, 0, 0]).tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    c = np.float32(0.3)
    assert G.scales(np.array([0.7, 0.0], np.float32), G.TENSOR, 0.3)[0] == c / np.float32(0.7)   # the division in fp32
