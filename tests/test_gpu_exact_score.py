"""kf_head_logprob on the level family (tests/exact_inputs.py): logits that are exact integers, 128 on a row's winners and within +-40 everywhere else, so that every
exponential the fold takes is exactly 0 or 1 -- whatever the tile form, the lane order, the merge order or the route.  The expectations are closed forms: sum = the
number of winners, max = 128, top1 = the lowest winner, lse = fl32(128 + logf(c)), logprob = fl32(fl32(t - 128) - logf(c)); a zero row (x = 0) counts every column
once: sum = V, top1 = 0, lse = logf(V).  Every element of logprob and lse (as uint32) and of top1 is compared for EQUALITY; there is no tolerance.

The winner sets sit where the fold has a seam: column 0, column V - 1 inside the ragged last tile, the first and the last column of a tile, either side of the wave
halves and of the lanes of a row, tiles one merge lane folds and tiles two lanes fold, a winner in every tile, 3 and 64 winners.  tests/test_exact_inputs_cpu.py pins
the plan of every case and shows which single wrong decision changes these bits.  Before each call the plan of that very call is asserted; outputs arrive two rows
longer than n and filled with sentinels, the scratch filled with 0xA5, x has two poison rows behind row n, a bf16 head lies in a buffer whose rows behind V score 256
on every channel, and every case runs twice to the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from koifish_amd import lib as L
from tests import exact_inputs as E
from tests.conftest import bf16_t, u16

pytestmark = pytest.mark.gpu
LP_FILL, LSE_FILL, TOP_FILL = 7.0, 7.0e9, -5
HOSTILE_ROWS = 256   # rows behind V in the bf16 head's buffer: up to the end of either tile form's last tile


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _upload(ctx, c):
    """the head on the device.  bf16: a descriptor over the first V rows of a buffer whose next HOSTILE_ROWS rows score 256 on every channel for every level row (a column
    >= V admitted anywhere takes the row, and a zero row counts it).  Quantised: the constructed blob; kf_dequant gives back the integer weight."""
    type_, _, symmetric, lgroup = E.STORAGES[c["storage"]]
    V, K, ow = c["V"], c["K"], c["ow"]
    if c["storage"] == "bf16":
        hostile = np.zeros((HOSTILE_ROWS, K))
        hostile[:, :E.LEVEL_P] = 32.0
        buf = bf16_t(np.concatenate([E.exact_bits(c["W"]), E.exact_bits(hostile)]), ctx.device)
        from koifish_amd.runtime import DevWeight
        dw = DevWeight(L.BF16, V, K, buf.view(torch.uint8).reshape(-1)[:V * K * 2])
        dw._whole = buf
        assert dw.desc().data == buf.data_ptr() and buf.data_ptr() % 16 == 0
    else:
        dw = ctx.upload_blob(type_, V, K, ow.blob(), lgroup, symmetric)
        assert dw.desc().qBias == ow.qBias
    assert np.array_equal(u16(ctx.dequant(dw)), E.exact_bits(c["W"]))
    return dw


def _run(ctx, dw, c, x_t, tg):
    n = c["n"]
    d = dw.desc()
    need = ctx.hip.kf_head_logprob_scratch_bytes(C.byref(d), n)
    assert need > 0
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=ctx.device)   # stale partials of an earlier call would show
    lp = torch.full((n + 2,), LP_FILL, dtype=torch.float32, device=ctx.device)
    lse = torch.full((n + 2,), LSE_FILL, dtype=torch.float32, device=ctx.device)
    top1 = torch.full((n + 2,), TOP_FILL, dtype=torch.int32, device=ctx.device)
    ctx.linear_scratch(dw, min(n, 128))
    rc = ctx.hip.kf_head_logprob(ctx.h, C.byref(d), _ptr(x_t), c["K"], n, _ptr(tg), _ptr(lp), _ptr(lse), _ptr(top1), _ptr(ws))
    assert rc == 0, ctx.hip.kf_last_error()
    ctx.sync()
    assert (ws[need:] == 0xA5).all(), "wrote behind the scratch it asked for"
    return lp.cpu().numpy(), lse.cpu().numpy(), top1.cpu().numpy()


@pytest.mark.parametrize("key", list(E.SCORE_CASES), ids=["%s-V%d-K%d-n%d-route%d-form%d" % k for k in E.SCORE_CASES])
def test_head_logprob_exact(ctx, key):
    storage, V, K, n, force, form = key
    ctx.hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    c = E.score_case(ctx.hip, key)
    assert E.score_name(E.score_plan(ctx.hip, key)) == E.SCORE_CASES[key], "the plan moved: %s is now %s" % (key, E.score_name(E.score_plan(ctx.hip, key)))
    dw = _upload(ctx, c)
    x_t = bf16_t(E.exact_bits(c["x"]), ctx.device)
    tg = torch.from_numpy(np.concatenate([c["targets"], [0, 0]]).astype(np.int32)).to(ctx.device)
    ctx.hip.kfdbg_set_knob(b"score_route", force)
    ctx.hip.kfdbg_set_knob(b"score_form", form)
    try:
        runs = [_run(ctx, dw, c, x_t, tg) for _ in range(2)]
    finally:
        ctx.hip.kfdbg_set_knob(b"score_route", 0)
        ctx.hip.kfdbg_set_knob(b"score_form", -1)
    for lp, lse, top1 in runs:
        assert lp[n:].tolist() == [LP_FILL] * 2 and lse[n:].tolist() == [np.float32(LSE_FILL)] * 2 and top1[n:].tolist() == [TOP_FILL] * 2, "wrote behind row n"
        for name, got, want in (("top1", top1[:n], c["top1"]), ("lse", lse[:n].view(np.uint32), c["lse"]), ("logprob", lp[:n].view(np.uint32), c["lp"])):
            bad = np.nonzero(got != want)[0]
            assert not len(bad), "%s: %d of %d rows differ, first row %d (channel %d, target %d): got %s, want %s" % (
                name, len(bad), n, bad[0], bad[0] % E.LEVEL_P, c["targets"][bad[0]], got[bad[0]], want[bad[0]])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two runs differ"
