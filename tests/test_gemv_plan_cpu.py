"""The one-token mat-vec plan without a GPU: kf::gemv_plan (through kfdbg_gemv_plan) is the one rule behind every gemv_launch -- the per-layer decode launches, the LM
head, the TP rank shards, the sparse forward and kf_linear's per-token fallback: the refusals, the storage form, the lanes per row, the slots per wave, the kernel form,
grid and LDS.  Pinned here on each side of every boundary; each expected value is what gemv_launch chose before the rule (gemv_launch_dot2 / gemv_launch_canon and
their launch_m .. launch_x ladder) for the same inputs.  The lanes per row fix the canonical summation order, so they are also checked against the oracle's own
statement of the rule."""
import ctypes as C

import pytest

from koifish_amd import lib as L
from oracle import oracle as O
from plan_structs import GemmMat as Mat, GemvPlan as Plan, GemvProblem as Problem

BF16, F8, Q4, Q3, Q2, T_SIGN, BOOL1, T_BINARY = 3, 4, 14, 15, 16, 17, 19, 20   # kf_dtype
GROUP, ROW_LUT, ROW_RTN = 0, 1, 2                                              # quant forms
FMT_BF16, FMT_F8, FMT_Q4, FMT_Q2, FMT_Q1, FMT_Q4P, FMT_Q4R, FMT_Q1T, FMT_Q2T = range(9)   # kf_kernels.h FMT_*
PLAIN, PAIRED, ARGMAX = range(3)                                               # GEMV_*
OK, INTERNAL_ERR, INVALID_ARGS, QUANT_ERR, UNSUPPORTED, UNALIGN = 0, -11, -20, -701, -1000, -2000
NONE = 0x7fffffff                                                              # slot0 of a job the launch does not have


def mat(M, K, type=Q4, quant=GROUP, lgroup=128, gama=1, al=3, awq=0):
    return Mat(type, quant, awq, M, K, lgroup, gama, al)


@pytest.fixture(scope="module")
def plan():
    hip = L.load()[0]
    hip.kfdbg_gemv_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]

    def f(mats, mode=PLAIN, sparse=0, n_hot=0, norm=0, canon=1, q4_perm=1, q2_tab=1, q1_tab=1, xf2=1):
        P = Problem(mode=mode, n_w=len(mats), sparse=sparse, n_hot=n_hot, norm=norm, canon=canon, q4_perm=q4_perm, q2_tab=q2_tab, q1_tab=q1_tab, xf2=xf2)
        for i, m in enumerate(mats):
            P.w[i] = m
        out = Plan()
        assert hip.kfdbg_gemv_plan(C.byref(P), C.byref(out)) == 0
        return out
    return f


def geo(p):
    """(storage form, lanes per row log2, steps per row, slots in flight G, slots per wave, workgroups, LDS bytes)"""
    return (p.fmt, p.lpr_log2, p.iters, p.G, p.spw, p.grid, p.lds)


def form(p):
    """(mode, sparse, onejob, njobs, xf, xf2)"""
    return (p.mode, p.sparse, p.onejob, p.njobs, p.xf, p.xf2)


# ---- the refusals, in the launcher's order: storage, K % elements per block, matrices that differ, AWQ, alignment, the 2^32-block index, row codebooks without gama,
# malformed groups, paired matrices of different heights, arg-max partials, LDS
@pytest.mark.parametrize("mats,kw,want", [
    ([mat(64, 1024, type=Q3)], {}, UNSUPPORTED),
    ([mat(64, 1024, type=Q2, quant=ROW_RTN)], {}, UNSUPPORTED),
    ([mat(64, 1024, type=Q3, quant=ROW_LUT)], {}, UNSUPPORTED),
    ([mat(64, 1040)], {}, INVALID_ARGS),                                  # 1040 % 32
    ([mat(64, 1028, type=BF16)], {}, INVALID_ARGS),                       # 1028 % 8
    ([mat(64, 1024, type=T_SIGN, lgroup=128)] * 1 + [mat(64, 1024)], {}, INVALID_ARGS),   # a second matrix of another storage
    ([mat(64, 1024), mat(64, 2048)], {}, INVALID_ARGS),                   # ... of another width
    ([mat(64, 1024, awq=1, al=0)], {}, UNSUPPORTED),                      # AWQ before alignment
    ([mat(64, 1024, al=0, gama=0)], {}, UNALIGN),                         # alignment before the groups
    ([mat(64, 1024, type=Q4, quant=ROW_LUT, al=1)], {}, UNALIGN),         # the row codebooks unaligned
    ([mat(64, 1024, type=Q4, quant=ROW_LUT, gama=0, al=1)], {}, QUANT_ERR),
    ([mat(4194304, 8192, type=BF16)], {}, INVALID_ARGS),                  # 2^22 rows x 1024 blocks = 2^32
    ([mat(64, 1024, gama=0)], {}, QUANT_ERR),
    ([mat(64, 1024, lgroup=0)], {}, QUANT_ERR),
    ([mat(64, 1024, lgroup=48)], {}, QUANT_ERR),                          # 48 % 32
    ([mat(64, 1024, lgroup=96)], {}, QUANT_ERR),                          # 3 blocks per group
    ([mat(3, 1024, lgroup=2048)], {}, QUANT_ERR),                         # 3 x 1024 weights are not whole groups
    ([mat(64, 1024), mat(32, 1024)], {"mode": PAIRED}, INVALID_ARGS),
    ([mat(10923, 512, type=BF16), mat(10923, 512, type=BF16), mat(10922, 512, type=BF16)], {"mode": ARGMAX}, INTERNAL_ERR),   # 4097 partials
    ([mat(64, 81800, type=BF16)], {}, INVALID_ARGS),                      # 163856 bytes of LDS
])
def test_refusals(plan, mats, kw, want):
    assert plan(mats, **kw).status == want


def test_limits_accept(plan):
    assert plan([mat(4194303, 8192, type=BF16)]).status == OK
    assert plan([mat(64, 1024, type=Q4, quant=ROW_LUT, al=3, lgroup=0)]).status == OK
    assert plan([mat(64, 1024, lgroup=256)]).status == OK
    p = plan([mat(10923, 512, type=BF16), mat(10923, 512, type=BF16), mat(10922, 512, type=BF16)])   # the same launch, plain: 4097 workgroups
    assert (p.status, p.grid, p.spw, list(p.slot0), p.total_slots) == (OK, 4097, 2, [0, 10924, 21848], 32770)
    p = plan([mat(10922, 512, type=BF16)] * 3, mode=ARGMAX)
    assert (p.status, p.grid) == (OK, 4096)
    p = plan([mat(64, 81792, type=BF16)])
    assert (p.status, p.lds) == (OK, 163840)


# ---- every storage at 1024 x 1024, dot2 order: the lanes per row (1- / 2-bit: the rule at K / 32 less two / one), the table forms and their LDS, the group shift
@pytest.mark.parametrize("type,quant,want,gshift", [
    (BF16, GROUP, (FMT_BF16, 6, 2, 1, 1, 256, 2304), 0),
    (F8, GROUP, (FMT_F8, 6, 1, 1, 1, 256, 2304), 0),
    (Q4, GROUP, (FMT_Q4P, 5, 1, 1, 1, 128, 2304), 2),
    (Q4, ROW_LUT, (FMT_Q4R, 5, 1, 1, 1, 128, 2304), 0),
    (T_SIGN, GROUP, (FMT_Q2T, 4, 1, 1, 1, 64, 4352), 1),
    (BOOL1, GROUP, (FMT_Q1T, 3, 1, 1, 1, 32, 6400), 0),
    (T_BINARY, GROUP, (FMT_Q1T, 3, 1, 1, 1, 32, 6400), 0),
])
def test_storages(plan, type, quant, want, gshift):
    p = plan([mat(1024, 1024, type=type, quant=quant)], canon=0)
    assert (p.status, geo(p), p.gshift, p.lgroup) == (OK, want, gshift, 128 if quant == GROUP and type != BF16 and type != F8 else 0)


@pytest.mark.parametrize("type,knob,want", [(Q4, "q4_perm", (FMT_Q4, 2304)), (T_SIGN, "q2_tab", (FMT_Q2, 2304)), (BOOL1, "q1_tab", (FMT_Q1, 2304))])
def test_arithmetic_forms_by_knob(plan, type, knob, want):
    p = plan([mat(1024, 1024, type=type)], canon=0, **{knob: 0})
    assert (p.fmt, p.lds) == want


def test_table_forms_by_lds(plan):
    assert (plan([mat(64, 80768, type=T_SIGN)]).fmt, plan([mat(64, 80768, type=T_SIGN)]).lds) == (FMT_Q2T, 163840)
    assert (plan([mat(64, 80832, type=T_SIGN)]).fmt, plan([mat(64, 80832, type=T_SIGN)]).lds) == (FMT_Q2, 161920)
    assert (plan([mat(64, 79744, type=BOOL1)]).fmt, plan([mat(64, 79744, type=BOOL1)]).lds) == (FMT_Q1T, 163840)
    assert (plan([mat(64, 79872, type=BOOL1)]).fmt, plan([mat(64, 79872, type=BOOL1)]).lds) == (FMT_Q1, 160000)


def test_register_table_geometry(plan):
    assert plan([mat(1024, 1024, lgroup=64)], canon=0).fmt == FMT_Q4         # groups of 64: two per lane quad
    assert plan([mat(1024, 1056)], canon=0).fmt == FMT_Q4                    # 1056 % 128
    assert plan([mat(1024, 1152)], canon=0).fmt == FMT_Q4P


# ---- the lanes per row: more lanes for short launches while that saves a step (0.6B down_proj 1024 x 3072: 6 below 2048 rows, 5 from there)
@pytest.mark.parametrize("M,want", [(1024, (6, 2)), (2047, (6, 2)), (2048, (5, 3))])
def test_lanes_for_short_launches(plan, M, want):
    p = plan([mat(M, 3072)], canon=0)
    assert (p.lpr_log2, p.iters) == want


def test_lanes_per_row_against_the_oracle(plan):
    """the plan's lanes per row = the oracle's kfo_lpr_log2 at K / elements per block, 1- / 2-bit blocks: at K / 32 less two / one (kfo_lpr_log2_epb)"""
    for type, epb in ((BF16, 8), (F8, 16), (Q4, 32), (T_SIGN, 64), (BOOL1, 128)):
        for K in (128, 256, 384, 512, 640, 896, 1024, 1536, 2048, 2560, 3072, 4096, 5120, 6144, 8192, 9728, 12288, 17408, 25600):
            for rows in (1, 16, 64, 256, 1000, 1023, 1024, 1025, 2047, 2048, 4096, 32768, 151936):
                want = O.lpr_log2(K // epb, rows) if epb <= 32 else max(0, O.lpr_log2(K // 32, rows) - (2 if epb == 128 else 1))
                p = plan([mat(rows, K, type=type)])
                assert (p.status, p.lpr_log2) == (OK, want), (type, K, rows)


def test_lanes_per_row_counts_every_job(plan):
    """rows of the launch: Q | K | V together, the gate alone for the paired gate | up"""
    assert plan([mat(1024, 3072)] * 2, canon=0).lpr_log2 == 5                   # 2048 rows
    assert plan([mat(1024, 3072)] * 2, mode=PAIRED, canon=0).lpr_log2 == 6      # 1024


# ---- the waves a launch aims for: 4096, 16384 from 2^19 blocks x rows per slot, 8192 from 4 M (not sparse, not the row codebooks); G 1 / 2 / 4 from the slots per wave
@pytest.mark.parametrize("mats,kw,want,stream_ok", [
    ([mat(8191, 512, type=BF16)], {}, (FMT_BF16, 6, 1, 2, 2, 1024, 1280), 1),        # 524224 blocks: 4096 waves, 2 slots each
    ([mat(8192, 512, type=BF16)], {}, (FMT_BF16, 6, 1, 1, 1, 2048, 1280), 0),        # 2^19: 16384 waves
    ([mat(40000, 512, type=BF16)], {}, (FMT_BF16, 6, 1, 2, 4, 2500, 1280), 1),       # 3 slots per wave -> G 2, 4 slots
    ([mat(31249, 1024, type=BF16)], {}, (FMT_BF16, 6, 2, 2, 2, 3907, 2304), 1),      # 3999872 blocks
    ([mat(31250, 1024, type=BF16)], {}, (FMT_BF16, 6, 2, 4, 4, 1954, 2304), 1),      # 4 M: 8192 waves
    ([mat(31250, 1024, type=BF16)], {"sparse": 1, "n_hot": 31250}, (FMT_BF16, 6, 2, 2, 2, 3907, 2304), 0),
    ([mat(31250, 4096, type=Q4, quant=ROW_LUT)], {}, (FMT_Q4R, 6, 2, 2, 2, 3907, 8448), 0),
    ([mat(131072, 1024)] * 2, {"mode": PAIRED, "canon": 0}, (FMT_Q4P, 5, 1, 2, 8, 2048, 2304), 1),   # 8 slots per wave: G 4, paired: 2
    ([mat(131072, 1024)], {"canon": 0}, (FMT_Q4P, 5, 1, 4, 8, 2048, 2304), 1),
])
def test_waves_and_slots(plan, mats, kw, want, stream_ok):
    p = plan(mats, **kw)
    assert (p.status, geo(p), p.stream_ok) == (OK, want, stream_ok)


# ---- the buffer-load form: every byte offset a wave can form below 2^31, groups inside rows
def test_stream_reach(plan):
    p = plan([mat(131051, 8192, type=BF16)])
    assert (geo(p), p.stream_ok) == ((FMT_BF16, 6, 16, 4, 16, 2048, 16640), 1)     # (131051 + 20) x 1024 x 16 < 2^31
    assert plan([mat(131052, 8192, type=BF16)]).stream_ok == 0
    p = plan([mat(32770, 1152, lgroup=256)], canon=0)                               # 1152 % 256: a group straddles two rows
    assert (geo(p), p.stream_ok, p.gshift) == ((FMT_Q4, 5, 2, 2, 2, 2049, 2560), 0, 3)
    p = plan([mat(32770, 1152)], canon=0)
    assert (geo(p), p.stream_ok, p.gshift) == ((FMT_Q4P, 5, 2, 2, 2, 2049, 2560), 1, 2)


# ---- the launch forms: ONEJOB for one matrix, arg-max and sparse launches; paired launches read job 1 by name; the sparse forms are plain or paired
@pytest.mark.parametrize("n_w,kw,want", [
    (1, {}, (PLAIN, 0, 1, 1)),
    (3, {}, (PLAIN, 0, 0, 3)),
    (2, {"mode": PAIRED}, (PAIRED, 0, 0, 1)),
    (1, {"mode": ARGMAX}, (ARGMAX, 0, 1, 1)),
    (1, {"sparse": 1, "n_hot": 100}, (PLAIN, 1, 1, 1)),
    (2, {"mode": PAIRED, "sparse": 1, "n_hot": 100}, (PAIRED, 1, 0, 1)),
    (1, {"mode": ARGMAX, "sparse": 1, "n_hot": 100}, (PLAIN, 1, 1, 1)),
])
def test_launch_forms(plan, n_w, kw, want):
    p = plan([mat(3072, 1024)] * n_w, canon=0, **kw)
    assert form(p)[:4] == want


def test_jobs_and_slots(plan):
    p = plan([mat(2048, 1024), mat(1024, 1024), mat(1024, 1024)], canon=0)          # Q | K | V of the 0.6B model: 2 rows per slot
    assert (geo(p), list(p.M), list(p.slot0), p.total_slots) == ((FMT_Q4P, 5, 1, 1, 1, 512, 2304), [2048, 1024, 1024], [0, 1024, 1536], 2048)
    p = plan([mat(3072, 1024)] * 2, mode=PAIRED, canon=0)
    assert (list(p.M), list(p.slot0), p.total_slots, p.grid) == ([3072, 3072, 0], [0, NONE, NONE], 1536, 384)
    p = plan([mat(3072, 1024)], sparse=1, n_hot=100, canon=0)                       # slots for the hot rows only; the lanes from all 3072
    assert (p.lpr_log2, list(p.M), p.total_slots, p.grid) == (5, [100, 0, 0], 50, 13)


# ---- the canonical 4-bit forms: x as fp32 while 4 K + 256 bytes fit 48 KiB (XF); longer rows of one-slot, one-matrix, norm-free plain launches half the block columns at
# a time (XF2) while the first window holds a whole round of four steps and the second fits 54 KiB
@pytest.mark.parametrize("M,K,kw,want", [
    (1024, 12224, {}, (FMT_Q4, 6, 6, 1, 1, 256, 49152, 1, 0)),
    (1024, 12256, {}, (FMT_Q4, 6, 6, 1, 1, 256, 24768, 0, 0)),
    (1024, 12224, {"canon": 0}, (FMT_Q4, 6, 6, 1, 1, 256, 24704, 0, 0)),
    (1024, 1024, {"mode": PAIRED}, (FMT_Q4P, 5, 1, 1, 1, 128, 4352, 1, 0)),
    (1024, 1024, {"sparse": 1, "n_hot": 1024}, (FMT_Q4P, 5, 1, 1, 1, 128, 4352, 1, 0)),
    (1024, 1024, {"mode": ARGMAX}, (FMT_Q4P, 5, 1, 1, 1, 128, 4352, 1, 0)),
    (1024, 1024, {"q4_perm": 0}, (FMT_Q4, 5, 1, 1, 1, 128, 4352, 1, 0)),
    (8192, 16384, {}, (FMT_Q4P, 6, 8, 1, 1, 2048, 33024, 1, 1)),                      # 25600-wide down_proj's kind: 4 + 4 steps
    (8193, 16384, {}, (FMT_Q4P, 6, 8, 2, 2, 1025, 33024, 0, 0)),                      # two slots per wave
    (8192, 16384, {"norm": 1}, (FMT_Q4P, 6, 8, 1, 1, 2048, 33024, 0, 0)),
    (8192, 16384, {"xf2": 0}, (FMT_Q4P, 6, 8, 1, 1, 2048, 33024, 0, 0)),
    (8192, 16384, {"sparse": 1, "n_hot": 8192}, (FMT_Q4P, 6, 8, 1, 1, 2048, 33024, 0, 0)),
    (1024, 14336, {}, (FMT_Q4P, 6, 7, 1, 1, 256, 28928, 0, 0)),                       # 7 steps: 0 in the first window
    (1024, 20480, {}, (FMT_Q4P, 6, 10, 1, 1, 256, 49408, 1, 1)),                      # 4 + 6 steps: 6 x 8 KiB + 256
    (1024, 22528, {}, (FMT_Q4P, 6, 11, 1, 1, 256, 45312, 0, 0)),                      # 4 + 7: 57600 bytes
    (5120, 25600, {}, (FMT_Q4P, 5, 25, 1, 1, 640, 53504, 1, 1)),                      # Qwen3-32B down_proj: 12 + 13 steps of 32 lanes
])
def test_canonical_4bit_forms(plan, M, K, kw, want):
    p = plan([mat(M, K)] * (2 if kw.get("mode") == PAIRED else 1), **kw)
    assert (p.status, geo(p) + (p.xf, p.xf2)) == (OK, want)


def test_canonical_forms_are_4bit_only(plan):
    for type, quant in ((BF16, GROUP), (F8, GROUP), (Q4, ROW_LUT), (T_SIGN, GROUP), (BOOL1, GROUP)):
        p = plan([mat(1024, 1024, type=type, quant=quant)])
        assert (p.canon, p.xf, p.xf2) == (1, 0, 0), type
