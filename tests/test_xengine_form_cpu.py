"""The kernel form of the XCD-confined engines without a GPU: kf::xengine_form (through kfdbg_xengine_form) is the one rule behind both kf_xengine_create's
refusal of a model too deep for its sequence count and the instantiation every launch runs.  Pinned here: the form chosen on each side of every sequence-count boundary,
the hooks (stamps, two decoders per XCD) where a shape and storage have forms for them, and the deepest model each row serves -- every shallower one served, the next refused."""
import ctypes as C

import pytest

from koifish_amd import lib as L

Q4P, Q1T, Q2T = 5, 7, 8                                          # kf_kernels.h FMT_*
S06, S256, S17, S4B, S8B, SGQA8, TP32, TP8, TP4 = range(1, 10)  # shape classes (kf_xengine.hip xe_shapes)


@pytest.fixture(scope="module")
def form():
    hip = L.load()[0]
    hip.kfdbg_xengine_form.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)]

    def f(sc, n_seq, n_layer, fmt=Q4P, stamps=False, two=False):
        """(waves, ring depth, decoders per XCD, sequences per decoder, stamps), None: refused"""
        out = (C.c_int * 5)()
        return tuple(out) if hip.kfdbg_xengine_form(sc, fmt, n_seq, n_layer, int(stamps), int(two), out) == 0 else None
    return f


def deepest(form, sc, n_seq, **kw):
    served = [n for n in range(1, 700) if form(sc, n_seq, n, **kw)]
    assert served == list(range(1, len(served) + 1)), "refused below a served depth"
    return len(served)


def form_at(nwv, depth, nb, wpc=1, dbg=0):
    return (nwv, depth, wpc, nb, dbg)


# (shape, storage, hooks, sequence counts, form, deepest model served): one row per sequence-count range
ROWS = [
    (S06, Q4P, {}, (1, 8), form_at(12, 2, 1), 477),
    (S06, Q4P, {}, (9, 16), form_at(12, 4, 2), 335),
    (S06, Q4P, dict(two=True), (9, 16), form_at(8, 4, 1, wpc=2), 149),
    (S256, Q4P, {}, (1, 8), form_at(12, 2, 1), 642),
    (S256, Q4P, {}, (9, 16), form_at(12, 4, 2), 610),
    (S256, Q4P, dict(two=True), (9, 16), form_at(8, 4, 1, wpc=2), 295),
    (S06, Q1T, {}, (1, 8), form_at(12, 2, 1), 459),
    (S06, Q1T, {}, (9, 16), form_at(12, 4, 2), 317),
    (S06, Q1T, {}, (17, 32), form_at(12, 2, 4), 32),
    (S06, Q2T, {}, (17, 32), form_at(12, 2, 4), 42),
    (S17, Q4P, {}, (1, 8), form_at(12, 6, 1), 348),
    (S17, Q4P, {}, (9, 16), form_at(8, 8, 2), 114),
    (S17, Q4P, dict(two=True), (9, 16), form_at(8, 4, 1, wpc=2), 84),
    (S4B, Q4P, {}, (1, 8), form_at(12, 6, 1), 93),
    (S8B, Q4P, {}, (1, 8), form_at(12, 6, 1), 177),
    (SGQA8, Q4P, {}, (1, 8), form_at(12, 6, 1), 584),
    (TP32, Q4P, {}, (8, 8), form_at(12, 6, 1), 214),
    (TP8, Q4P, {}, (8, 8), form_at(12, 6, 1), 270),
    (TP4, Q4P, {}, (8, 8), form_at(12, 2, 1), 352),
]


@pytest.mark.parametrize("sc,fmt,hooks,seqs,chosen,depth", ROWS)
def test_each_row_picks_its_form_up_to_its_deepest_model(form, sc, fmt, hooks, seqs, chosen, depth):
    for n_seq in seqs:
        assert form(sc, n_seq, 1, fmt, **hooks) == chosen
        assert form(sc, n_seq, depth, fmt, **hooks) == chosen
        assert deepest(form, sc, n_seq, fmt=fmt, **hooks) == depth


def test_four_sequences_per_decoder_fall_to_four_compute_waves_past_51_layers(form):
    for sc, last12, depth in ((S06, 51, 88), (S256, 547, 566)):
        for n_seq in (17, 32):
            for two in (False, True):   # (the A/B hook is for 9 .. 16 sequences only)
                assert form(sc, n_seq, last12, two=two) == form_at(12, 2, 4)
                assert form(sc, n_seq, last12 + 1, two=two) == form_at(8, 8, 4)
                assert deepest(form, sc, n_seq, two=two) == depth


def test_stamps_take_the_stamped_twin_where_there_is_one(form):
    for sc in (S06, S256):
        assert form(sc, 8, 28, stamps=True) == form_at(12, 2, 1, dbg=1)
        assert form(sc, 9, 28, stamps=True) == form_at(12, 4, 2, dbg=1)
        assert form(sc, 16, 28, stamps=True, two=True) == form_at(8, 4, 1, wpc=2, dbg=1)
    # 17 .. 32 sequences: always the 12-wave form -- no stamped 4 + 4-wave twin, so a model past 51 layers is refused
    assert form(S06, 32, 51, stamps=True) == form_at(12, 2, 4, dbg=1)
    assert form(S06, 32, 52, stamps=True) is None
    assert form(TP32, 8, 64, stamps=True) == form_at(12, 6, 1, dbg=1)
    # every other shape and storage: no effect
    for sc, fmt, n_seq in ((S17, Q4P, 8), (S17, Q4P, 16), (S4B, Q4P, 8), (S8B, Q4P, 8), (SGQA8, Q4P, 8), (TP8, Q4P, 8), (TP4, Q4P, 8), (S06, Q1T, 8), (S06, Q1T, 32),
                            (S256, Q2T, 16)):
        for two in (False, True):
            assert form(sc, n_seq, 3, fmt, stamps=True, two=two) == form(sc, n_seq, 3, fmt, two=two)


def test_what_no_form_serves_is_refused(form):
    for n_seq in (17, 32):
        assert form(S17, n_seq, 3) is None                   # the 1.7B shape: at most 16 sequences
    for sc in (S4B, S8B, SGQA8):
        assert form(sc, 8, 3) is not None and form(sc, 9, 3) is None   # the GQA-4 / GQA-8 shapes: at most 8
    for sc in (S17, S4B, S8B, SGQA8, TP32, TP8, TP4):
        for fmt in (Q1T, Q2T):
            assert form(sc, 1, 3, fmt) is None               # low-bit storage: the 0.6B and 256-wide shapes only
    assert form(0, 1, 3) is None and form(10, 1, 3) is None  # no such shape
