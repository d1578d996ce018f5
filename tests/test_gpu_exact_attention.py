"""The attention kernels of the training path on one-hot / two-hot inputs (tests/exact_inputs.py): q and k are built so that every row's softmax is exactly {1} or
{1/2, 1/2} on chosen keys and exactly 0 elsewhere after the kernels' own fp32 arithmetic (tests/test_exact_inputs_cpu.py emulates that arithmetic for every case
here), and v, o, dO are small integers -- so the forward output and all three gradients have closed forms whose accumulators are exact in fp32 in any order.  Every
element of every row and head is compared BIT FOR BIT; there is no tolerance.

  code family   the chosen keys are the diagonal, key 0, key i - 1, the first / last key of 32-key tiles, the keys on either side of multiples of 128: a visible key
                dropped by a mask decision (a wave's `full` shortcut, key <= tok, qi >= key, a seam of the 32-column waves or the 128-column workgroups) loses a row
  ramp family   the score grows with the key index by the same gap per step: the visible maximum is the diagonal and EVERY masked future key scores higher, so one
                future key admitted, or a row clamped to T - 1 and read again, takes the row over

Outputs are pre-filled with a value no result equals; rows behind the last token and padding columns must keep it."""
import numpy as np
import pytest
import torch

from tests import exact_inputs as E
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu

SENTINEL = 77.0   # a bf16 value; forward results are halves within +-2, gradients never 77 (asserted on each expectation)
S_BITS = 0x429A


def _filled(rows, cols, dev):
    return torch.full((rows, cols), SENTINEL, dtype=torch.bfloat16, device=dev)


def _padded(a, rows, cols, dev):
    """fp64 small integers [r, c] -> bf16 device tensor [rows, cols], the rest zero"""
    buf = np.zeros((rows, cols), np.uint16)
    buf[:a.shape[0], :a.shape[1]] = E.exact_bits(a)
    return bf16_t(buf, dev)


def _check_out(out, want_bits, what):
    """out [rows + 2, stride]: the result block bit for bit, everything else untouched"""
    got = u16(out)
    r, w = want_bits.shape
    assert np.array_equal(got[:r, :w], want_bits), "%s: %d of %d values differ" % (what, int((got[:r, :w] != want_bits).sum()), want_bits.size)
    assert (got[r:] == S_BITS).all() and (got[:, w:] == S_BITS).all(), what + ": wrote outside its rows / columns"


def _forward(ctx, fam, n, nh, nkv, hd, n_seq):
    dev, Cq, Ck = ctx.device, nh * hd, nkv * hd
    rows = n_seq * n
    for pos0 in ((0, E.FWD_POS0) if n_seq == 1 else (0,)):
        c = E.attn_case(fam, n, nh, nkv, hd, n_seq, pos0, seed=n + nh + hd, vmax=2)
        want = E.bits(E.closed_forward(c))
        assert not (want == S_BITS).any()
        if n_seq == 1:   # kf_attn_prefill: q and out share one (padded) row stride, the cache rows another
            qs, ks = Cq + 16, Ck + 8
            q, kc, vc = _padded(c["q"], rows + 2, qs, dev), _padded(c["k"], c["tot"], ks, dev), _padded(c["v"], c["tot"], ks, dev)
            out = _filled(rows + 2, qs, dev)
            assert ctx.hip.kf_attn_prefill(ctx.h, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), pos0, n, qs, nh, nkv, hd, ks) == 0, ctx.hip.kf_last_error()
            ctx.sync()
            _check_out(out, want, "kf_attn_prefill pos0 %d" % pos0)
        if pos0:
            continue
        # the batch entries read q | k | v out of one fused buffer [rows, (nh + 2 nkv) hd]
        W = Cq + 2 * Ck
        qkv = _padded(np.concatenate([c["q"], c["k"], c["v"]], axis=1), rows + 2, W, dev)
        qc = qkv[:, :Cq].contiguous()
        out = _filled(rows + 2, Cq, dev)
        assert ctx.hip.kf_attn_prefill_batch(ctx.h, qc.data_ptr(), qkv[:, Cq:].data_ptr(), qkv[:, Cq + Ck:].data_ptr(), out.data_ptr(), n, Cq, nh, nkv, hd, W, n_seq) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        _check_out(out, want, "kf_attn_prefill_batch")
        out = _filled(rows + 2, Cq + 8, dev)   # a row stride of its own for out: the 8 padding columns stay
        assert ctx.hip.kf_attn_prefill_batch_strided(ctx.h, qkv.data_ptr(), qkv[:, Cq:].data_ptr(), qkv[:, Cq + Ck:].data_ptr(), out.data_ptr(), n, W, Cq + 8, nh, nkv, hd, W,
                                                     n_seq) == 0, ctx.hip.kf_last_error()
        ctx.sync()
        _check_out(out, want, "kf_attn_prefill_batch_strided")


@pytest.mark.parametrize("n_seq", E.N_SEQ)
@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
@pytest.mark.parametrize("n", E.FWD_N)
def test_attention_forward_exact(ctx, n, nh, nkv, hd, n_seq):
    """out_i = bf16(v_a) or bf16((v_a + v_b) / 2) through kf_attn_prefill (pos0 = 0 and behind a prefix of cache rows), kf_attn_prefill_batch and
    kf_attn_prefill_batch_strided; n = 257 runs the paired form (two key halves merged)"""
    for fam in ("code", "ramp"):
        _forward(ctx, fam, n, nh, nkv, hd, n_seq)


def test_attention_forward_exact_long_tile_form(ctx):
    """more than 256 tokens in the UNPAIRED tile form: enough workgroups (17 x 8 kv heads x 3 sequences) that the plan does not pair them"""
    t = E.FWD_TILE_LONG
    for fam in ("code", "ramp"):
        _forward(ctx, fam, t["n"], t["nh"], t["nkv"], t["hd"], t["n_seq"])


def _backward(ctx, c, fused):
    T, nh, nkv, hd, n_seq, dev = c["T"], c["nh"], c["nkv"], c["hd"], c["n_seq"], ctx.device
    Cq, Ck, rows = nh * hd, nkv * hd, c["n_seq"] * c["T"]
    want = E.closed_backward(c)
    assert not any((want[k] == S_BITS).any() for k in ("dq", "dk", "dv"))
    o, dO = _padded(c["o"], rows, Cq + 8, dev), _padded(c["dO"], rows, Cq + 8, dev)
    nb = ctx.hip.kf_attn_backward_scratch_bytes(T, nh, n_seq)
    scratch = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device=dev)   # the rows' L and D of an earlier call, or anything else
    if fused:   # q | k | v column blocks of one buffer, dq | dk | dv of another
        W = Cq + 2 * Ck
        qkv = _padded(np.concatenate([c["q"], c["k"], c["v"]], axis=1), rows, W, dev)
        d = _filled(rows + 2, W, dev)
        ptrs = (qkv.data_ptr(), qkv[:, Cq:].data_ptr(), qkv[:, Cq + Ck:].data_ptr())
        dptrs = (d.data_ptr(), d[:, Cq:].data_ptr(), d[:, Cq + Ck:].data_ptr())
        ld = ldd = W
    else:       # three tensors of the common row stride n_head * head_dim: k / v, dk / dv use its first n_kv * head_dim columns
        q, k, v = (_padded(c[x], rows, Cq, dev) for x in ("q", "k", "v"))
        ds = [_filled(rows + 2, Cq, dev) for _ in range(3)]
        ptrs, dptrs = (q.data_ptr(), k.data_ptr(), v.data_ptr()), tuple(x.data_ptr() for x in ds)
        ld = ldd = Cq
    assert ctx.hip.kf_attn_backward(ctx.h, *ptrs, ld, o.data_ptr(), dO.data_ptr(), Cq + 8, *dptrs, ldd, T, nh, nkv, hd, n_seq, scratch.data_ptr()) == 0, ctx.hip.kf_last_error()
    ctx.sync()
    what = "%s T %d heads %d/%d hd %d x %d %s" % (c["family"], T, nh, nkv, hd, n_seq, "fused" if fused else "separate")
    if fused:
        got = u16(d)
        assert np.array_equal(got[:rows], np.concatenate([want["dq"], want["dk"], want["dv"]], axis=1)), what
        assert (got[rows:] == S_BITS).all(), what
    else:
        for x, name in zip(ds, ("dq", "dk", "dv")):
            _check_out(x, want[name], what + " " + name)


@pytest.mark.parametrize("n_seq", E.N_SEQ)
@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", E.HEADS)
@pytest.mark.parametrize("T", E.BWD_T)
def test_attention_backward_exact(ctx, T, nh, nkv, hd, n_seq):
    """kf_attn_backward: dq = bf16(fl32(sum dS k) fl32(scale)), dk likewise with the sum over the group's heads inside one accumulator, dv = sum p dO -- GQA and
    batching together, fused and separate layouts, o an arbitrary integer tensor (D = dO . o is an input to the entry, not the forward's output).  Ramp family: no
    trace of any future key in any row."""
    for fam in ("code", "ramp"):
        c = E.attn_case(fam, T, nh, nkv, hd, n_seq, seed=T + nh + hd)
        for fused in (True, False):
            _backward(ctx, c, fused)
