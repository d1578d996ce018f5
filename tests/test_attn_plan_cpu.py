"""The attention plan without a GPU: kf::attn_plan (through kfdbg_attn_plan) is the one rule behind every attention launch -- one token against the cache
(kf_attn_decode, kf_attn_block), a prompt against the cache (kf_attn_prefill), a batch of independent sequences (kf_attn_prefill_batch(_strided)) and the
backward: the route, the kernel form, the slices, the counter stride, grid, threads, LDS and scratch.  Pinned here on each side of every boundary; each expected
value is what the launchers chose before the rule (attn_launch with attn_splits and the KF_ATTN_GO ladder, attn_prefill_mfma_launch with ap_launch_gq, and
kf_attn_prefill's try-the-tile-kernel-then-fall-back) for the same inputs, at the knobs' shipped values."""
import ctypes as C
import functools

import pytest

import attn_plan_mirror as A
from attn_plan_mirror import BACKWARD, BATCH, BWD, DECODE, OUT_AL, PAIRED, PER_TOKEN, PROMPT, Q_AL, SLICED, TILE
from koifish_amd import lib as L

OK, INVALID_ARGS, UNSUPPORTED = 0, -20, -1000


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def plan(hip):
    return functools.partial(A.plan, hip)


def dec(p):
    """(route, kernel query heads, waves, slices, keys per slice, workgroups per kv-head and slice, grid)"""
    return (p.route, p.gq, p.nw, p.n_splits, p.chunk, p.gq_split, tuple(p.grid))


# ---- slices: one up to 192 keys, then 64-key slices, at most 512 / n_kv of them and at most 32
@pytest.mark.parametrize("n_head,n_kv,pos,want", [
    (16, 8, 191, (SLICED, 2, 8, 1, 192, 1, (1, 8, 1))),     # 192 keys: one slice of 192 (> 128 keys at GQ 2: 8 waves)
    (16, 8, 192, (SLICED, 2, 4, 4, 49, 1, (4, 8, 1))),      # 193 keys: ceil(193 / 64) slices
    (32, 16, 2047, (SLICED, 2, 4, 32, 64, 1, (32, 16, 1))), # 512 / 16 = 32
    (32, 32, 2047, (SLICED, 1, 4, 16, 128, 1, (16, 32, 1))),# 512 / 32 = 16 slices of 128 keys
    (34, 17, 2047, (SLICED, 2, 4, 30, 69, 1, (30, 17, 1))), # 512 / 17 = 30
    (600, 600, 2047, (SLICED, 1, 8, 1, 2048, 1, (1, 600, 1))),  # 512 / 600 = 0: one slice
    (64, 8, 2047, (SLICED, 8, 4, 32, 64, 1, (32, 8, 1))),
    (64, 8, 2048, (SLICED, 8, 4, 32, 65, 1, (32, 8, 1))),   # 33 slices by keys: capped at 32
    (64, 8, 4095, (SLICED, 8, 4, 32, 128, 1, (32, 8, 1))),  # 64 by keys and by 512 / 8: 32
])
def test_slices(plan, n_head, n_kv, pos, want):
    p = plan(DECODE, n_head, n_kv, pos=pos)
    assert p.status == OK and dec(p) == want


# ---- 8 waves once a slice holds more than 128 keys, at 1 or 2 query heads per kv-head
@pytest.mark.parametrize("gq", [1, 2, 4, 8])
@pytest.mark.parametrize("canon", [0, 1])
def test_waves(plan, gq, canon):
    few = gq <= 2
    for pos, nw in ((127, 4), (128, 8 if few else 4)):                         # one slice of 128 / 129 keys
        assert plan(DECODE, 8 * gq, 8, pos=pos, canon=canon).nw == nw
    for pos, nw in ((4095, 4), (4096, 8 if few else 4)):                       # 32 slices of 128 / 129 keys
        p = plan(DECODE, 8 * gq, 8, pos=pos, canon=canon)
        assert (p.n_splits, p.chunk, p.nw, p.threads) == (32, 128 if pos == 4095 else 129, nw, 64 * nw)
    for pos0, n_tok, nw in ((100, 28, 4), (100, 29, 8 if few else 4)):         # per-token form: one slice of pos0 + n_tok keys
        p = plan(PROMPT, 8 * gq, 8, pos=pos0, n_tok=n_tok, canon=canon, al=0)
        assert (p.route, p.chunk, p.nw) == (PER_TOKEN, pos0 + n_tok, nw)


# ---- the canonical order deals the query heads of GQA-4 / GQA-8 to workgroups of two; the fp32 order keeps them together
@pytest.mark.parametrize("gq,canon,split", [(1, 0, 1), (2, 0, 1), (4, 0, 1), (8, 0, 1), (1, 1, 1), (2, 1, 1), (4, 1, 2), (8, 1, 4)])
def test_query_head_split(plan, gq, canon, split):
    p = plan(DECODE, 4 * gq, 4, pos=500, canon=canon)
    assert (p.status, p.canon, p.gq_split, p.gq, p.grid[1]) == (OK, canon, split, gq // split, 4 * split)
    p = plan(PROMPT, 4 * gq, 4, pos=10, n_tok=3, canon=canon)
    assert (p.route, p.gq_split, p.gq, tuple(p.grid)) == (PER_TOKEN, split, gq // split, (1, 4 * split, 3))


# ---- arrival counters: 4096 ints over n_kv * gq_split (kv-head, part) pairs, at most 64 apart, refused below 1
@pytest.mark.parametrize("n_head,n_kv,canon,want", [
    (8, 8, 0, (OK, 64)), (64, 64, 0, (OK, 64)), (65, 65, 0, (OK, 63)),
    (4096, 4096, 0, (OK, 1)), (4097, 4097, 0, (INVALID_ARGS, None)),
    (8192, 1024, 1, (OK, 1)), (8200, 1025, 1, (INVALID_ARGS, None)),     # canonical GQA-8: 4 parts per kv-head
    (8200, 1025, 0, (OK, 3)),
])
def test_counter_stride(plan, n_head, n_kv, canon, want):
    for entry, n_tok in ((DECODE, 1), (PROMPT, 2)):                          # the per-token form checks it too
        p = plan(entry, n_head, n_kv, pos=300, n_tok=n_tok, canon=canon)
        assert p.status == want[0]
        if want[0] == OK:
            assert p.cnt_stride == want[1]


# ---- LDS and threads of each form
@pytest.mark.parametrize("n_head,n_kv,hd,pos,canon,want", [
    (8, 8, 128, 100, 1, (1, 4, 4688)),      # canonical: 8 NW gq (hd + 2) + 2 (gq hd + hd) + 16
    (16, 8, 128, 100, 1, (2, 4, 9104)),
    (32, 8, 128, 100, 1, (2, 4, 9104)),     # GQA-4: two workgroups of two heads
    (64, 8, 128, 100, 1, (2, 4, 9104)),     # GQA-8: four of two
    (8, 8, 64, 150, 1, (1, 8, 4496)),
    (16, 8, 128, 150, 1, (2, 8, 17424)),
    (64, 8, 128, 100, 0, (8, 4, 19344)),    # fp32: 2 (gq hd + hd) + 4 (NW gq + 4 + NW gq (hd + 4))
    (32, 8, 64, 100, 0, (4, 4, 5072)),
    (8, 8, 128, 150, 0, (1, 8, 4784)),
    (16, 8, 64, 100, 0, (2, 4, 2608)),
])
def test_decode_lds(plan, n_head, n_kv, hd, pos, canon, want):
    p = plan(DECODE, n_head, n_kv, hd=hd, pos=pos, canon=canon)
    assert (p.gq, p.nw, p.lds, p.threads, p.hd) == want + (64 * want[1], hd)


# ---- refusals of the decode kernel: head_dim 64 / 128, n_head a multiple of n_kv, GQ 1 / 2 / 4 / 8
@pytest.mark.parametrize("n_head,n_kv,hd", [(8, 8, 32), (8, 8, 96), (8, 8, 256), (8, 0, 128), (12, 8, 128), (24, 8, 128), (128, 8, 128), (0, 8, 128)])
def test_decode_refusals(plan, n_head, n_kv, hd):
    for canon in (0, 1):
        assert plan(DECODE, n_head, n_kv, hd=hd, pos=100, canon=canon).status == INVALID_ARGS
        assert plan(PROMPT, n_head, n_kv, hd=hd, pos=100, n_tok=16, canon=canon).status == INVALID_ARGS


# ---- prompts: the tile kernel from 8 tokens on a covered shape, else the per-token form
@pytest.mark.parametrize("kw,tile", [
    (dict(n_tok=7), False), (dict(n_tok=8), True),
    (dict(n_tok=8, hd=64), True),
    (dict(n_tok=8, al=OUT_AL), False),                  # q not 16-byte aligned
    (dict(n_tok=8, al=Q_AL), False),                    # out not 8-byte aligned
    (dict(n_tok=8, q_stride=2052), False),              # q rows: 4 elements off 16 bytes
    (dict(n_tok=8, q_stride=2056), True),
    (dict(n_tok=8, kv_stride=1028), False),
    (dict(n_tok=8, q_stride=0), True),
])
def test_prompt_route(plan, kw, tile):
    a = dict(hd=128, pos=40)
    a.update(kw)
    p = plan(PROMPT, 16, 8, **a)
    assert p.status == OK and p.route == (TILE if tile else PER_TOKEN)
    if not tile:
        assert (tuple(p.grid), p.n_splits, p.chunk, p.scratch) == ((1, 8, a["n_tok"]), 1, 40 + a["n_tok"], 0)


@pytest.mark.parametrize("gq", [1, 2, 3, 4, 8, 16])
def test_prompt_query_heads(plan, gq):
    p = plan(PROMPT, 4 * gq, 4, pos=0, n_tok=64)
    assert p.status == (OK if gq in (1, 2, 4, 8) else INVALID_ARGS)
    if p.status == OK:
        assert (p.route, p.gq, tuple(p.grid)) == (TILE, gq, ((64 + 128 // gq - 1) // (128 // gq), 4, 1))
    b = plan(BATCH, 4 * gq, 4, n_tok=64, n_seq=3)
    assert b.status == (OK if gq in (1, 2, 4, 8) else INVALID_ARGS)


# ---- a batch of sequences takes the tile kernel only
@pytest.mark.parametrize("kw,status", [
    (dict(), OK), (dict(n_tok=1), OK), (dict(hd=64), OK),
    (dict(hd=96), INVALID_ARGS), (dict(hd=256), INVALID_ARGS), (dict(n_kv=0), INVALID_ARGS), (dict(n_head=12), INVALID_ARGS),
    (dict(al=OUT_AL), INVALID_ARGS), (dict(al=Q_AL), INVALID_ARGS),
    (dict(q_stride=3076), INVALID_ARGS), (dict(kv_stride=1028), INVALID_ARGS),
    (dict(out_stride=2050), INVALID_ARGS),              # out rows: 2 elements off 8 bytes
    (dict(out_stride=2052), OK),                         # 8-byte rows suffice for out
    (dict(q_stride=3072, out_stride=2048), OK),          # the training step's fused [rows, 3C] q
])
def test_batch_refusals(plan, kw, status):
    a = dict(n_head=16, n_kv=8, hd=128, n_tok=100, n_seq=2)
    a.update(kw)
    p = plan(BATCH, **a)
    assert p.status == status
    if status == OK:
        assert p.route == TILE and p.scratch == 0


# ---- the paired form: at most 320 workgroups and at least 256 tokens; half blocks from the front and back, (half blocks + 1) / 2 workgroups
@pytest.mark.parametrize("entry,n_head,n_kv,n_tok,n_seq,want", [
    (BATCH, 16, 8, 255, 1, (TILE, (4, 8, 1))),
    (BATCH, 16, 8, 256, 1, (PAIRED, (4, 8, 1))),
    (PROMPT, 16, 8, 255, 1, (TILE, (4, 8, 1))),
    (PROMPT, 16, 8, 256, 1, (PAIRED, (4, 8, 1))),
    (PROMPT, 16, 8, 2047, 1, (PAIRED, (32, 8, 1))),     # 64 half blocks of 32 tokens
    (BATCH, 1, 1, 40960, 1, (PAIRED, (320, 1, 1))),      # 320 workgroups: 640 half blocks of 64
    (BATCH, 1, 1, 40961, 1, (TILE, (321, 1, 1))),        # 321
    (BATCH, 1, 1, 256, 160, (PAIRED, (2, 1, 160))),
    (BATCH, 1, 1, 300, 107, (TILE, (3, 1, 107))),        # 321 over the sequences
    (BATCH, 1, 1, 300, 106, (PAIRED, (3, 1, 106))),      # 318: 5 half blocks
    (BATCH, 32, 4, 300, 1, (PAIRED, (19, 4, 1))),        # GQ 8: 38 half blocks of 8 tokens
    (BATCH, 32, 4, 260, 1, (PAIRED, (17, 4, 1))),        # 33 half blocks
])
def test_paired(plan, entry, n_head, n_kv, n_tok, n_seq, want):
    p = plan(entry, n_head, n_kv, n_tok=n_tok, n_seq=n_seq)
    assert p.status == OK and (p.route, tuple(p.grid)) == want
    kh = 2 if want[0] == PAIRED else 1
    assert (p.kh, p.kt, p.threads) == (kh, 32 * kh, 256 * kh)


@pytest.mark.parametrize("hd,kh,lds", [(64, 1, 21504), (128, 1, 37888), (64, 2, 86016), (128, 2, 151552)])
def test_tile_lds(plan, hd, kh, lds):
    p = plan(BATCH, 16, 8, hd=hd, n_tok=256 if kh == 2 else 100)
    assert (p.kh, p.lds) == (kh, lds)


# ---- backward: dQ over (128-row blocks, heads, sequences), dK / dV over (blocks, kv-heads, sequences); head_dim 64 / 128 only
@pytest.mark.parametrize("T,hd,want", [(128, 128, 1), (129, 128, 2), (300, 64, 3), (1024, 128, 8)])
def test_backward(plan, T, hd, want):
    p = plan(BACKWARD, 16, 8, hd=hd, n_tok=T, n_seq=2)
    assert (p.status, p.route, p.gq, p.hd, p.threads, p.lds) == (OK, BWD, 2, hd, 256, 0)
    assert tuple(p.grid) == (want, 16, 2) and tuple(p.grid_kv) == (want, 8, 2)
    assert p.scratch == 4 * 2 * T * 16 * 2


@pytest.mark.parametrize("n_head,n_kv,hd", [(16, 8, 96), (16, 8, 256), (16, 8, 32), (16, 0, 128), (12, 8, 128)])
def test_backward_refusals(plan, n_head, n_kv, hd):
    assert plan(BACKWARD, n_head, n_kv, hd=hd, n_tok=64, n_seq=1).status == UNSUPPORTED


# ---- the scratch queries of the ABI are the plan's figures
def test_scratch(hip, plan):
    hip.kf_attn_scratch_bytes.restype = C.c_size_t
    hip.kf_attn_scratch_bytes.argtypes = [C.c_int, C.c_int]
    hip.kf_attn_backward_scratch_bytes.restype = C.c_size_t
    hip.kf_attn_backward_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    assert hip.kf_attn_scratch_bytes(16, 128) == 8 * 16 * 32 * 130 + 16384 == 548864
    assert hip.kf_attn_scratch_bytes(16, 64) == 8 * 16 * 32 * 66 + 16384 == 286720
    assert plan(DECODE, 16, 8, hd=128, pos=3000).scratch == 548864
    assert plan(DECODE, 16, 8, hd=64, pos=10).scratch == 286720
    assert plan(PROMPT, 16, 8, hd=128, pos=10, n_tok=3).scratch == 0
    assert hip.kf_attn_backward_scratch_bytes(300, 16, 2) == 76800
    for T, h, s in ((0, 16, 2), (300, 0, 2), (300, 16, 0)):
        assert hip.kf_attn_backward_scratch_bytes(T, h, s) == 0


def test_attention_knobs_removed(hip):
    hip.kfdbg_set_knob.argtypes = [C.c_char_p, C.c_long]
    assert hip.kfdbg_set_knob(b"attn_gq_split", 4) == -1
    assert hip.kfdbg_set_knob(b"attn_pair_min", 256) == -1
