"""Packed documents without a GPU: kf_attn_docs_plan (the pure host rule of csrc/kf_attn_docs_plan.h behind the C ABI) and Qwen3Step.check_documents.
The layout of every test: documents of 1, 63, 65, 129 and 96 rows with 0, 0, 3, 0 and 5 gap rows in front of them, in 384 rows -- a 22-row gap behind the last."""
import ctypes as C

import numpy as np
import pytest

from koifish_amd import lib as L
from koifish_amd.train_step import Qwen3Step

LENS, GAPS, N, T = [1, 63, 65, 129, 96], [0, 0, 3, 0, 5], 384, 256
ROWS = [int(sum(LENS[:d]) + sum(GAPS[:d + 1])) for d in range(len(LENS))]
GEOMS = [(hd, gq) for hd in (64, 128) for gq in (1, 2, 4, 8)]
WHICH = ("forward", "dq", "dkv")


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _plan(rows, lens, n_rows, max_len, n_head, n_kv, hd, n_doc=None, fill=0xA5):
    """(return code, the table bytes kf_attn_docs_plan wrote into a buffer pre-filled with `fill`)"""
    hip, _ = L.load()
    r, l = _i32(rows), _i32(lens)
    n_doc = len(l) if n_doc is None else n_doc
    nb = hip.kf_attn_docs_table_bytes(r.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), n_doc, n_rows, max_len, n_head, n_kv, hd)
    buf = np.full(max(nb, 4096), fill, dtype=np.uint8)
    rc = hip.kf_attn_docs_plan(r.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), n_doc, n_rows, max_len, n_head, n_kv, hd, buf.ctypes.data_as(C.c_void_p), buf.size)
    return rc, nb, buf


def _tables(buf):
    h = L.AttnDocsHeader.from_buffer_copy(buf[:64].tobytes())
    e = buf.view(np.int32).reshape(-1, 4)
    return h, [e[h.off[w]:h.off[w] + h.n[w]] for w in range(3)]


@pytest.mark.parametrize("hd,gq", GEOMS)
def test_tables_cover_every_row_once_longest_first(hd, gq):
    n_kv = 2
    rc, nb, buf = _plan(ROWS, LENS, N, T, n_kv * gq, n_kv, hd)
    assert rc == 0 and nb > 64 and nb % 16 == 0
    h, tabs = _tables(buf)
    assert (h.magic, h.n_rows, h.n_head, h.n_kv, h.head_dim, h.n_doc, h.max_len) == (L.ATTN_DOCS_MAGIC, N, n_kv * gq, n_kv, hd, len(LENS), T)
    assert (h.doc_rows, h.gap_rows) == (sum(LENS), N - sum(LENS)) and h.gap_rows == sum(GAPS) + 22
    assert 64 + 16 * sum(h.n) == nb and (buf[nb:] == 0xA5).all(), "the table is the header and the three tables, and nothing is written behind it"
    in_doc = np.zeros(N, dtype=bool)
    for r, n in zip(ROWS, LENS):
        in_doc[r:r + n] = True
    for w, tab in enumerate(tabs):
        tile = 128 // gq if w == 0 else 128
        seen_doc, seen_gap, walks = np.zeros(N, dtype=int), np.zeros(N, dtype=int), []
        n_docs_entries = int((tab[:, 3] == 0).sum())
        assert (tab[:n_docs_entries, 3] == 0).all() and (tab[n_docs_entries:, 3] == 1).all(), "%s: the gap entries come last" % WHICH[w]
        for row0, ln, t, gap in tab:
            lo, hi = t * tile, min((t + 1) * tile, ln)
            assert 0 <= lo < hi <= ln and row0 >= 0 and row0 + ln <= N, "%s: an entry reaches outside its run" % WHICH[w]
            if gap:
                assert not in_doc[row0:row0 + ln].any()
                seen_gap[row0 + lo:row0 + hi] += 1
            else:
                assert (int(row0), int(ln)) in list(zip(ROWS, LENS)), "%s: an entry of no document" % WHICH[w]
                seen_doc[row0 + lo:row0 + hi] += 1
                walks.append(ln - lo if w == 2 else hi)   # the keys (dK/dV: the queries) the tile's workgroup walks
        assert np.array_equal(seen_doc, in_doc.astype(int)), "%s: every document row exactly once" % WHICH[w]
        assert np.array_equal(seen_gap, (~in_doc).astype(int)), "%s: every gap row exactly once" % WHICH[w]
        assert walks == sorted(walks, reverse=True), "%s: longest key range first" % WHICH[w]
    rc2, nb2, buf2 = _plan(ROWS, LENS, N, T, n_kv * gq, n_kv, hd)
    assert rc2 == 0 and nb2 == nb and np.array_equal(buf[:nb], buf2[:nb]), "a second call gives the same bytes"


BAD = {
    "no document": dict(n_doc=0),
    "length 0": dict(lens=[1, 0, 65, 129, 96]),
    "length above max_len": dict(max_len=128),
    "overlap": dict(rows=[0, 1, 63, 132, 266]),
    "descending": dict(rows=[0, 67, 1, 132, 266]),
    "past n_rows": dict(rows=[0, 1, 67, 132, 289]),
    "head_dim 96": dict(hd=96),
    "3 query heads per kv-head": dict(n_head=6),
    "n_head no multiple of n_kv": dict(n_head=5),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_plan_refusals_write_nothing(case):
    a = dict(rows=ROWS, lens=LENS, n_rows=N, max_len=T, n_head=4, n_kv=2, hd=64, n_doc=None)
    a.update(BAD[case])
    rc, nb, buf = _plan(**a)
    assert rc == -20 and nb == 0, case          # KF_INVALID_ARGS
    assert (buf == 0xA5).all(), "%s: a refusal leaves the table untouched" % case
    hip, _ = L.load()
    assert hip.kf_last_error().startswith(b"kf_attn_docs_plan")


def test_plan_refuses_a_short_table_and_null_pointers():
    hip, _ = L.load()
    rc, nb, _ = _plan(ROWS, LENS, N, T, 4, 2, 64)
    assert rc == 0
    r, l = _i32(ROWS), _i32(LENS)
    small = np.full(nb, 0xA5, dtype=np.uint8)
    args = (r.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), len(LENS), N, T, 4, 2, 64)
    assert hip.kf_attn_docs_plan(*args, small.ctypes.data_as(C.c_void_p), nb - 16) == -20 and (small == 0xA5).all()
    assert hip.kf_attn_docs_plan(*args, None, nb) == -20
    assert hip.kf_attn_docs_plan(None, args[1], *args[2:], small.ctypes.data_as(C.c_void_p), nb) == -20 and (small == 0xA5).all()
    assert hip.kf_attn_backward_docs_scratch_bytes(N, 4) == 2 * 4 * N * 4 and hip.kf_attn_backward_docs_scratch_bytes(0, 4) == 0


CFG = dict(dim=128, n_layer=2, n_head=4, n_kv=2, head_dim=64, ffn=256, vocab=250)
B_, T_ = 3, 128     # 384 rows, documents of up to 128 rows: the 129-row document of the layout above is one too long here


def test_check_documents_derives_positions_mask_and_n_valid():
    lens, rows = [1, 63, 65, 128, 96], ROWS
    rng = np.random.default_rng(5)
    mask = rng.random(N) < 0.5
    d = Qwen3Step.check_documents(CFG, B_, T_, lens, rows, mask)
    pos, in_doc = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
    for r, n in zip(rows, lens):
        pos[r:r + n], in_doc[r:r + n] = np.arange(n), True
    assert d["pos"].dtype == np.int32 and np.array_equal(d["pos"], pos)
    assert d["mask"].dtype == np.int32 and np.array_equal(d["mask"], np.where(mask & in_doc, 0, 0x10000))
    assert d["n_valid"] == int((mask & in_doc).sum()) and 0 < d["n_valid"] < in_doc.sum()
    assert np.array_equal(d["rows"], rows) and np.array_equal(d["lens"], lens)
    # no mask: every document row counts, no gap row does; no rows: back to back from row 0
    d = Qwen3Step.check_documents(CFG, B_, T_, lens, rows)
    assert d["n_valid"] == sum(lens) and np.array_equal(d["mask"] == 0, in_doc)
    d = Qwen3Step.check_documents(CFG, B_, T_, [5, 128, 7])
    assert d["rows"].tolist() == [0, 5, 133] and d["n_valid"] == 140 and d["pos"][:6].tolist() == [0, 1, 2, 3, 4, 0] and not d["pos"][140:].any()
    assert (d["mask"][140:] == 0x10000).all()


@pytest.mark.parametrize("why,kw", [
    ("at least one document", dict(doc_lens=[])),
    ("1 .. 128", dict(doc_lens=[1, 0, 5])),
    ("1 .. 128", dict(doc_lens=[1, 129])),
    ("ascending, no overlap", dict(doc_lens=[10, 10], doc_rows=[0, 9])),
    ("ascending, no overlap", dict(doc_lens=[10, 10], doc_rows=[20, 0])),
    ("past the step's 384 rows", dict(doc_lens=[10, 100], doc_rows=[0, 285])),
    ("2 lengths but 1 first rows", dict(doc_lens=[10, 10], doc_rows=[0])),
    ("sequences of ints", dict(doc_lens=[10.5])),
    ("sequences of ints", dict(doc_lens=7)),
    ("loss_mask must be bool", dict(doc_lens=[10], loss_mask=np.ones(N - 1, dtype=bool))),
    ("loss_mask must be bool", dict(doc_lens=[10], loss_mask=np.ones(N, dtype=np.int32))),
    ("no row counts", dict(doc_lens=[10], loss_mask=np.zeros(N, dtype=bool))),
    ("no row counts", dict(doc_lens=[10], doc_rows=[4], loss_mask=np.arange(N) < 4)),     # the mask selects gap rows only
])
def test_check_documents_raises_with_the_reason(why, kw):
    with pytest.raises(ValueError, match=why):
        Qwen3Step.check_documents(CFG, B_, T_, **kw)


def test_check_documents_refuses_a_head_geometry_the_attention_does_not_take():
    with pytest.raises(ValueError, match="heads of 96"):
        Qwen3Step.check_documents(dict(CFG, head_dim=96), B_, T_, [10])
    with pytest.raises(ValueError, match="6 / 2 heads"):
        Qwen3Step.check_documents(dict(CFG, n_head=6), B_, T_, [10])


def test_gpt2_step_has_no_documents():
    from koifish_amd.train_step import GPT2Step
    assert not hasattr(GPT2Step, "set_documents") and hasattr(Qwen3Step, "set_documents")
    _, host = L.load()
    assert hasattr(host, "kfh_qwen3t_set_documents") and not hasattr(host, "kfh_gpt2_set_documents")
