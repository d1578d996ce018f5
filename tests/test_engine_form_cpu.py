"""The kernel form of the persistent decode engine without a GPU: kf::engine_form (through kfdbg_engine_form) is the one rule behind both kf_engine_create's
refusal of a model whose storage the shape is not instantiated for, or that is too deep for the LDS, and the instantiation every launch runs.  Pinned here: the form for
every shape class, storage and order, the stamps where a stamped twin exists, and the deepest model each row serves -- every shallower one served, the next refused."""
import ctypes as C

import pytest

from koifish_amd import lib as L

Q4, Q4P, Q1T, Q2T = 2, 5, 7, 8   # kf_kernels.h FMT_*
S06, S256, S17 = 1, 2, 3         # shape classes (kf_engine.hip eng_shapes)


@pytest.fixture(scope="module")
def form():
    hip = L.load()[0]
    hip.kfdbg_engine_form.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]

    def f(sc, fmt, n_layer, canon=True, stamps=False, lds=False):
        """(shape class, storage, canonical, stamps) [+ launch LDS], None: refused"""
        out = (C.c_int * 5)()
        if hip.kfdbg_engine_form(sc, fmt, int(canon), int(stamps), n_layer, out) != 0:
            return None
        return tuple(out) if lds else tuple(out)[:4]
    return f


# (shape, storage, LDS of a one-layer model, deepest model served): the depths of the LDS rule as it stood before the table of forms
ROWS = [
    (S06, Q4P, 64656, 436),
    (S06, Q1T, 68752, 418),
    (S06, Q2T, 66704, 427),
    (S256, Q4P, 32016, 579),
    (S256, Q1T, 36112, 561),
    (S256, Q2T, 34064, 570),
    (S17, Q4P, 93328, 310),
]


@pytest.mark.parametrize("sc,fmt,lds1,depth", ROWS)
def test_each_row_serves_both_orders_up_to_its_deepest_model(form, sc, fmt, lds1, depth):
    for canon in (True, False):
        assert form(sc, fmt, 1, canon) == (sc, fmt, int(canon), 0)
        assert form(sc, fmt, 1, canon, lds=True)[4] == lds1
        assert form(sc, fmt, depth, canon, lds=True)[4] <= 160 * 1024
        served = [n for n in range(1, 700) if form(sc, fmt, n, canon)]
        assert served == list(range(1, depth + 1)), "refused below a served depth, or the deepest model moved"
        assert form(sc, fmt, 1 + depth, canon) is None


def test_stamps_take_the_stamped_twin_on_the_benchmark_shape_and_storage_only(form):
    for canon in (True, False):
        assert form(S06, Q4P, 28, canon, stamps=True) == (S06, Q4P, int(canon), 1)
        assert form(S06, Q4P, 436, canon, stamps=True) == (S06, Q4P, int(canon), 1)
        assert form(S06, Q4P, 437, canon, stamps=True) is None
    for sc, fmt in ((S06, Q1T), (S06, Q2T), (S256, Q4P), (S256, Q1T), (S256, Q2T), (S17, Q4P)):
        for canon in (True, False):
            assert form(sc, fmt, 3, canon, stamps=True) == form(sc, fmt, 3, canon) == (sc, fmt, int(canon), 0)


def test_what_no_form_serves_is_refused(form):
    for canon in (True, False):
        for fmt in (Q1T, Q2T):
            assert form(S17, fmt, 3, canon) is None   # the 1.7B shape: 4-bit register-table storage only
        for sc in (S06, S256, S17):
            assert form(sc, Q4, 3, canon) is None     # no arithmetic-form 4-bit instantiation: every 4-bit model the engine takes has groups of 128
    assert form(0, Q4P, 3) is None and form(4, Q4P, 3) is None   # no such shape
