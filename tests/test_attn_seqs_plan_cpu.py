"""The plan of kf_attn_block_seqs without a GPU (kf::attn_plan's ATTN_DECODE_SEQS entry through kfdbg_attn_plan): the grid over (slices of the longest sequence,
sequence x kv-head x part), four waves always, one decode scratch per sequence, the refusals -- at the head geometries of the GPU test -- and the plans of the seven
older entries on fixed problems, as the commit before the entry made them."""
import functools

import pytest

import attn_plan_mirror as A
import exact_inputs as E
from koifish_amd import lib as L

DECODE_SEQS, VERIFY, SLICED_SEQS = 7, 6, 7      # the enumerators behind attn_plan_mirror's
OK, INVALID_ARGS, UNALIGN = 0, -20, -2000
POSITIONS = [0, 1, 63, 64, 191, 192, 193, 300, 2047]


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def plan(hip):
    return functools.partial(A.plan, hip)


@pytest.mark.parametrize("hd", E.HEAD_DIMS)
@pytest.mark.parametrize("n_head,n_kv", E.HEADS)
@pytest.mark.parametrize("n_seq", [1, 3, 8, 32])
def test_grid_scratch_lds(hip, plan, n_head, n_kv, hd, n_seq):
    GQ = n_head // n_kv
    gq, split = min(GQ, 2), max(GQ // 2, 1)
    for pos in POSITIONS:
        one = plan(A.DECODE, n_head, n_kv, hd=hd, pos=pos, canon=1)      # the slice rule is the one-sequence entry's, asked at the longest sequence
        for canon in (0, 1):                                             # not read: one arithmetic
            p = plan(DECODE_SEQS, n_head, n_kv, hd=hd, pos=pos, n_seq=n_seq, canon=canon, out_stride=n_head * hd)
            assert (p.status, p.route, p.canon, p.gq, p.gq_split, p.nw, p.threads, p.hd) == (OK, SLICED_SEQS, 1, gq, split, 4, 256, hd)
            assert (p.n_splits, p.chunk, p.cnt_stride) == (one.n_splits, one.chunk, one.cnt_stride) and p.n_splits == (1 if pos < 192 else -(-(pos + 1) // 64))
            assert tuple(p.grid) == (p.n_splits, n_seq * n_kv * split, 1) and p.lds == 8 * 4 * gq * (hd + 2) + 2 * (gq * hd + hd) + 16
            assert p.scratch == n_seq * one.scratch == n_seq * (8 * n_head * 32 * (hd + 2) + 16384) == hip.kf_attn_seqs_scratch_bytes(n_head, hd, n_seq)
    p = plan(DECODE_SEQS, n_head, n_kv, hd=hd, pos=-1, n_seq=n_seq)      # every sequence parked: an empty grid, not a refusal
    assert (p.status, p.n_splits, p.grid[0]) == (OK, 0, 0)


@pytest.mark.parametrize("kw,status", [
    (dict(n_seq=0), INVALID_ARGS), (dict(n_seq=33), INVALID_ARGS), (dict(n_seq=32), OK),
    (dict(hd=96), INVALID_ARGS), (dict(hd=256), INVALID_ARGS), (dict(n_kv=0), INVALID_ARGS), (dict(n_head=12), INVALID_ARGS), (dict(n_head=128), INVALID_ARGS),
    (dict(kv_stride=1028), UNALIGN), (dict(q_stride=2052), UNALIGN), (dict(out_stride=2050), UNALIGN), (dict(kv_stride=1032, q_stride=2056, out_stride=2056), OK),
    (dict(al=0), OK),                                   # q and out rows need no more than their strides' 8 elements
])
def test_refusals(hip, plan, kw, status):
    assert plan(DECODE_SEQS, **dict(dict(n_head=16, n_kv=8, hd=128, pos=300, n_seq=4), **kw)).status == status
    assert hip.kf_attn_seqs_scratch_bytes(16, 128, 0) == 0 == hip.kf_attn_seqs_scratch_bytes(16, 128, 33)


# (entry, arguments) -> (status, route, gq, nw, n_splits, chunk, gq_split, cnt_stride, grid, threads, lds, scratch): the plans of the commit before the entry existed
@pytest.mark.parametrize("args,kw,want", [
    ((A.DECODE, 16, 8), dict(pos=2047, canon=1), (OK, A.SLICED, 2, 4, 32, 64, 1, 64, (32, 8, 1), 256, 9104, 548864)),
    ((A.DECODE, 32, 8), dict(pos=191, canon=0, hd=64), (OK, A.SLICED, 4, 4, 1, 192, 1, 64, (1, 8, 1), 256, 5072, 557056)),
    ((A.PROMPT, 16, 8), dict(pos=40, n_tok=7), (OK, A.PER_TOKEN, 2, 4, 1, 47, 1, 64, (1, 8, 7), 256, 5040, 0)),
    ((A.PROMPT, 16, 8), dict(pos=0, n_tok=2047), (OK, A.PAIRED, 2, 0, 0, 0, 0, 0, (32, 8, 1), 512, 151552, 0)),
    ((A.BATCH, 16, 8), dict(n_tok=100, n_seq=2), (OK, A.TILE, 2, 0, 0, 0, 0, 0, (2, 8, 2), 256, 37888, 0)),
    ((A.BACKWARD, 16, 8), dict(n_tok=300, n_seq=2, hd=64), (OK, A.BWD, 2, 0, 0, 0, 0, 0, (3, 16, 2), 256, 0, 76800)),
    ((A.DECODE_KV8, 16, 8), dict(pos=300), (OK, A.SLICED_KV8, 2, 4, 5, 61, 1, 64, (5, 8, 1), 256, 9632, 548864)),
    ((A.PROMPT_KV8, 16, 8), dict(pos=3, n_tok=100), (OK, A.TILE_KV8, 2, 0, 0, 0, 0, 0, (4, 8, 1), 256, 36608, 0)),
    ((VERIFY, 32, 8), dict(pos=190, n_tok=4, canon=1), (OK, A.SLICED, 2, 4, 4, 49, 2, 64, (4, 16, 4), 256, 9104, 4 * 1081344)),
])
def test_older_entries_unchanged(plan, args, kw, want):
    p = plan(*args, **kw)
    assert (p.status, p.route, p.gq, p.nw, p.n_splits, p.chunk, p.gq_split, p.cnt_stride, tuple(p.grid), p.threads, p.lds, p.scratch) == want
