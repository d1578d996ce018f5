"""The ATTN_VERIFY entry of kf::attn_plan without a GPU (kf_attn_decode_rows: R consecutive queries of one sequence in one launch): the sliced canonical decode
kernel with the query on grid z, the grid's x and the waves those of the LAST query (every query takes its own slices inside the kernel), one decode scratch per
query.  The pinned entries of tests/test_attn_plan_cpu.py are another file's; here only that ATTN_DECODE answers what it answered for the same position."""
import pytest

import attn_plan_mirror as A
from attn_plan_mirror import DECODE, SLICED
from koifish_amd import lib as L

VERIFY = 6   # AttnProblem::entry ATTN_VERIFY
OK, INVALID_ARGS = 0, -20


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.mark.parametrize("n_head,n_kv,hd,pos0,R", [
    (4, 2, 64, 188, 8),      # the batch straddles 192 keys: the last query has 4 slices, the first four have one
    (8, 2, 128, 188, 8),     # GQA-4: two workgroups of two query heads per kv-head
    (64, 32, 64, 2044, 8),   # 16 slices that pass 128 keys inside the batch: the last query's 8 waves
    (64, 32, 64, 2040, 8),   # ... and not yet
    (4, 2, 64, 0, 8),
    (16, 8, 128, 2040, 5),
    (16, 8, 128, 2047, 1),
])
def test_the_geometry_is_the_last_querys(hip, n_head, n_kv, hd, pos0, R):
    v = A.plan(hip, VERIFY, n_head, n_kv, hd=hd, pos=pos0, n_tok=R, canon=1)
    d = A.plan(hip, DECODE, n_head, n_kv, hd=hd, pos=pos0 + R - 1, canon=1)
    assert v.status == OK and d.status == OK and v.route == SLICED and v.canon == 1
    assert (v.gq, v.nw, v.gq_split, v.n_splits, v.chunk, v.cnt_stride, v.threads, v.lds) == (d.gq, d.nw, d.gq_split, d.n_splits, d.chunk, d.cnt_stride, d.threads, d.lds)
    assert tuple(v.grid) == (d.grid[0], d.grid[1], R)
    assert v.scratch == R * d.scratch
    # the slice count never falls as the position grows: the last query's grid covers every query's own slices
    assert all(A.plan(hip, DECODE, n_head, n_kv, hd=hd, pos=pos0 + r, canon=1).n_splits <= v.n_splits for r in range(R))


def test_pinned(hip):
    v = A.plan(hip, VERIFY, 4, 2, hd=64, pos=188, n_tok=8, canon=1)
    assert (v.n_splits, v.chunk, v.nw, tuple(v.grid)) == (4, 49, 4, (4, 2, 8))
    v = A.plan(hip, VERIFY, 64, 32, hd=64, pos=2044, n_tok=8, canon=1)
    assert (v.n_splits, v.chunk, v.nw, tuple(v.grid)) == (16, 129, 8, (16, 32, 8))


@pytest.mark.parametrize("kw", [
    dict(n_tok=0), dict(n_tok=9), dict(pos=-1), dict(canon=0), dict(hd=96), dict(n_head=6, n_kv=4), dict(n_head=48, n_kv=16),
])
def test_refusals(hip, kw):
    a = dict(n_head=4, n_kv=2, hd=64, pos=10, n_tok=4, canon=1)
    a.update(kw)
    assert A.plan(hip, VERIFY, a.pop("n_head"), a.pop("n_kv"), **a).status == INVALID_ARGS
