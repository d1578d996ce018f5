"""The decode attention kernels (kf_attn.hip attn_kernel and attn_fast_kernel: kf_attn_decode's slices, and the per-token route of kf_attn_prefill) on the one-hot /
two-hot families of tests/exact_inputs.py, in BOTH summation orders (kf_set_canonical 1 and 0): the softmax of the query row is exactly {1} or {1/2, 1/2} on chosen
keys and exactly 0 elsewhere after the kernels' own arithmetic (tests/test_exact_inputs_cpu.py emulates both orders), v is a small positive integer, so the output is
v_a or (v_a + v_b) / 2 BIT FOR BIT.  No tolerance, and no oracle: the expectation is a closed form, so kernel and oracle cannot share a mistake here.

  code family   the chosen key is the diagonal, key 0, key pos - 1, the first and the last key of a slice for the chunk the plan reports, or a pair one code bit apart
                that straddles two slices: a key dropped at a slice seam, a slice left out of the merge or merged twice loses or halves the row
  ramp family   the score grows with the key index: the position itself is the visible maximum and EVERY row behind it scores higher -- with the device position
                below the launch's bound those rows are in the cache, and one of them admitted takes the whole output

The plan of every launch (slices, keys per slice, waves, heads per workgroup) is asserted against a restatement of the rule before the call.  Outputs are pre-filled
with a value no result equals; everything around the result must keep it.  The scratch is zeroed once (the context's) and reused by every call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import exact_inputs as E
from tests.conftest import bf16_t
from tests.test_gpu_exact_attention import S_BITS, _check_out, _filled, _padded

pytestmark = pytest.mark.gpu


@pytest.fixture
def orders(ctx):
    """sets the summation order of the session's context; puts back what it found"""
    was = ctx.hip.kf_get_canonical(ctx.h)
    yield ctx.set_canonical
    ctx.set_canonical(was)


def _assert_plan(ctx, bound, nh, nkv, hd, canon):
    p = E.attn_plan(ctx.hip, E.ATTN_DECODE, nh, nkv, hd, 1, 1, bound, canon)
    want = E.decode_slices(bound, nkv, nh // nkv, canon)
    assert (p.route, p.n_splits, p.chunk, p.nw, p.gq_split) == (E.ATTN_SLICED,) + want, "the plan moved: bound %d heads %d/%d is now %s" % (
        bound, nh, nkv, (p.route, p.n_splits, p.chunk, p.nw, p.gq_split))
    return p


def _decode(ctx, orders, c, row, bound, d_pos=None):
    """kf_attn_decode of row `row` of the case against its cache, laid out for positions up to `bound`, in both orders: the closed form bit for bit, twice"""
    nh, nkv, hd, dev = c["nh"], c["nkv"], c["hd"], ctx.device
    Cq, ks = nh * hd, nkv * hd + 8
    assert c["tot"] > bound and not (c["want"] == S_BITS).any()
    q = bf16_t(E.exact_bits(c["q"][row]), dev)
    kc, vc = _padded(c["k"], c["tot"], ks, dev), _padded(c["v"], c["tot"], ks, dev)
    dp = None if d_pos is None else torch.tensor([d_pos], dtype=torch.int32, device=dev)
    ws = ctx._ws(nh, hd)   # zeroed when it was made, never again: the kernels leave their arrival counters at zero
    for canon in (1, 0):
        orders(canon)
        _assert_plan(ctx, bound, nh, nkv, hd, canon)
        for _ in range(2):
            out = _filled(3, Cq + 8, dev)
            rc = ctx.hip.kf_attn_decode(ctx.h, C.c_void_p(q.data_ptr()), C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), C.c_void_p(out.data_ptr()), bound,
                                        None if dp is None else C.c_void_p(dp.data_ptr()), nh, nkv, hd, ks, C.c_void_p(ws.data_ptr()))
            assert rc == 0, ctx.hip.kf_last_error()
            ctx.sync()
            _check_out(out, c["want"][None, :], "%s row %d bound %d heads %d/%d hd %d %s order" % (c["family"], row, bound, nh, nkv, hd, "canonical" if canon else "fast"))


def _shifts(nh):
    return range(0, E.DECODE_KINDS, nh)   # between them the heads of the calls take every kind of decode_targets


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
@pytest.mark.parametrize("pos", E.DECODE_POS)
def test_attn_decode_exact(ctx, orders, pos, nh, nkv, hd):
    """out = bf16(v_a) or bf16((v_a + v_b) / 2) for the last row of a case of pos + 1 keys: one slice up to 192 keys (8 waves from 129 for GQ <= 2), ceil(len / 64) from 193"""
    chunk = _assert_plan(ctx, pos, nh, nkv, hd, 0).chunk
    for shift in _shifts(nh):
        _decode(ctx, orders, E.decode_case("code", pos, nh, nkv, hd, chunk, shift), pos, pos)
    _decode(ctx, orders, E.decode_case("ramp", pos, nh, nkv, hd, chunk), pos, pos)


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
def test_attn_decode_exact_2047_keys(ctx, orders, hd):
    """11-bit codes: 2047 keys in the plan's largest slice count, 32 slices of 64"""
    t = E.DECODE_LONG
    p = _assert_plan(ctx, t["pos"], t["nh"], t["nkv"], hd, 0)
    assert p.n_splits == 32 and p.chunk == 64
    for shift in _shifts(t["nh"]):
        _decode(ctx, orders, E.decode_case("code", t["pos"], t["nh"], t["nkv"], hd, p.chunk, shift, nbits=t["nbits"]), t["pos"], t["pos"])
    _decode(ctx, orders, E.decode_case("ramp", t["pos"], t["nh"], t["nkv"], hd, p.chunk, nbits=t["nbits"]), t["pos"], t["pos"])


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_attn_decode_position_below_the_bound(ctx, orders, nh, nkv, hd):
    """a launch laid out for position 300 (five slices of 61 keys, loaded before the position is known) whose device position is 130: rows 131 .. 300 are in the cache,
    and in the ramp family every one of them scores above every visible key"""
    bound, pos = E.DECODE_BOUND, E.DECODE_BELOW
    chunk = _assert_plan(ctx, bound, nh, nkv, hd, 0).chunk
    assert pos // chunk < bound // chunk   # whole slices lie behind the position, and the position's own slice is cut short
    for fam in ("ramp", "code"):
        _decode(ctx, orders, E.decode_case(fam, pos, nh, nkv, hd, chunk, T=bound + 1), pos, bound, d_pos=pos)


def _per_token(ctx, orders, fam, n, pos0, nh, nkv, hd, pad):
    dev, Cq, ks = ctx.device, nh * hd, nkv * hd + 8
    qs = Cq + pad
    c = E.attn_case(fam, n, nh, nkv, hd, 1, pos0, seed=n + nh + hd, **E.DECODE_V)
    want = E.bits(E.closed_forward(c))
    assert not (want == S_BITS).any()
    assert E.forward_route(ctx.hip, E.ATTN_PROMPT, nh, nkv, hd, n, 1, pos0, q_stride=qs) == E.ATTN_PER_TOKEN
    q, kc, vc = _padded(c["q"], n + 2, qs, dev), _padded(c["k"], c["tot"], ks, dev), _padded(c["v"], c["tot"], ks, dev)
    for canon in (1, 0):
        orders(canon)
        out = _filled(n + 2, qs, dev)
        assert ctx.hip.kf_attn_prefill(ctx.h, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), pos0, n, qs, nh, nkv, hd, ks) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        _check_out(out, want, "kf_attn_prefill per token: %s n %d pos0 %d heads %d/%d hd %d canonical %d" % (fam, n, pos0, nh, nkv, hd, canon))


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
def test_attn_prefill_per_token_route_exact(ctx, orders, nh, nkv, hd):
    """the route of every ragged last chunk of a chunked prefill: fewer than 8 tokens, at position 0 and behind a prefix of cache rows; and 33 tokens whose q rows are
    n_head head_dim + 4 elements apart, which the tile kernel refuses"""
    for fam in ("code", "ramp"):
        for pos0 in (0, E.FWD_POS0):
            for n in E.PER_TOKEN_N:
                _per_token(ctx, orders, fam, n, pos0, nh, nkv, hd, 16)
            _per_token(ctx, orders, fam, E.PER_TOKEN_REFUSED["n"], pos0, nh, nkv, hd, E.PER_TOKEN_REFUSED["pad"])
