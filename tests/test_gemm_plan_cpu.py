"""The token-batch GEMM plan without a GPU: kf::gemm_plan (through kfdbg_gemm_plan) is the one rule behind kf_linear, kf_linear_multi, kf_gateup_swiglu_batch,
kf_qkv_rope_seqs and kf_linear_backward -- the route, the kernel family and its form, the grid, the split-K cut, the dequantise target.  Pinned here on each side of every
boundary; each expected value is what the launch chain before the rule (kf_linear -> gemm_launch -> gemm3_launch / gemm2_launch, ...) chose for the same inputs.
Also the two scratch queries, which size Fish's scratch and so must keep their values."""
import ctypes as C

import pytest

from koifish_amd import lib as L
from plan_structs import GemmKern as Kern, GemmMat as Mat, GemmPlan as Plan, GemmProblem as Problem

BF16, F8, Q4, Q3, T_SIGN = 3, 4, 14, 15, 17             # kf_dtype
GROUP, ROW_LUT = 0, 1                                     # quant forms
FMT_BF16, FMT_Q4, FMT_Q2, FMT_Q4R = 0, 2, 3, 6            # kf_kernels.h FMT_*
LINEAR, MULTI, GATEUP, ROPE, BWD_DX, BWD_DW = range(6)    # GemmEntry
(MATVEC, AWQ, ROWFORM, RESIDENT, DEQ_TILE, TILE, STACKED, SWIGLU, ROPE_EPI, FUSED, SEPARATE, KMAJOR, TRANSPOSE) = range(13)   # GemmRoute
NONE, DIRECT, PAIRED, STAGED, G2, G3 = range(6)           # GemmFamily
DQ_NONE, DQ_SCRATCH, DQ_ARENA, DQ_RESIDENT = range(4)
BIG, SMALL, MID, TINY, WIDE = range(5)                    # G3 forms
STACK, ILV = 0, 1
SK_BYTES = 256 * 256 * 256 * 4 + 8192                     # gemm3_sk_ws_bytes()
LOTS = 1 << 30


def mat(M, K, type=Q4, quant=GROUP, lgroup=128, al=3, awq=0):
    return Mat(type, quant, awq, M, K, lgroup, 1, al)


@pytest.fixture(scope="module")
def hip():
    return L.load()[0]


@pytest.fixture(scope="module")
def plan(hip):
    hip.kfdbg_gemm_plan.argtypes = [C.POINTER(Problem), C.POINTER(Plan)]

    def f(entry, mats, n, x_al=1, y_al=1, rope_ok=0, scratch=0, arena=0, arena_free=0, arena_hit=0, capturing=0):
        P = Problem(entry=entry, n_w=len(mats), n=n, x_al=x_al, y_al=y_al, rope_ok=rope_ok, arena=arena, capturing=capturing, arena_hit=arena_hit,
                    arena_free=arena_free, scratch=scratch)
        for i, m in enumerate(mats):
            P.w[i] = m
        out = Plan()
        assert hip.kfdbg_gemm_plan(C.byref(P), C.byref(out)) == 0
        return out
    return f


def kern(p):
    """(family, form, grid x, grid y, block, LDS) of a plan's launch"""
    k = p.k
    return (k.fam, k.form, k.gx, k.gy, k.block, k.lds)


def sk(p):
    return (p.k.sk, p.k.P, p.k.S, p.k.kp, p.k.R, p.k.gx)


# ---- kf_linear on the weight as stored (gemm_launch): direct while ceil(M/32) ceil(n/32) <= 1280, then the producer / consumer kernel (4-bit, bf16, f8, n >= 256,
# >= 128 workgroups of 128 x 256), then the staged kernel (KS 2 below 512 tiles of 128 rows x 128 tokens)
@pytest.mark.parametrize("M,n,want", [
    (1024, 1280, (DIRECT, 32, 32, 40, 512, 32768)),          # 32 x 40 = 1280 direct workgroups
    (1024, 1281, (STAGED, 2, 16, 11, 256, 69632)),           # 32 x 41 > 1280; producer / consumer 8 x 6 < 128; staged 8 x 11 < 512: KS 2, 64 rows per workgroup
    (1024, 4096, (G2, 0, 8, 16, 512, 110592)),               # 8 x 16 = 128 producer / consumer workgroups
    (1024, 3840, (STAGED, 2, 16, 30, 256, 69632)),           # 8 x 15 = 120 < 128
    (16384, 255, (STAGED, 2, 256, 2, 256, 69632)),           # n < 256: no producer / consumer tile; 128 x 2 < 512
    (16384, 256, (G2, 0, 128, 1, 512, 110592)),
])
def test_linear_q4_kernels(plan, M, n, want):
    p = plan(LINEAR, [mat(M, 1024)], n)
    assert (p.route, p.status, p.deq) == (TILE, 0, DQ_NONE)
    assert kern(p) == want
    assert (p.k.fmt, p.k.gshift) == (FMT_Q4, 2)               # 128-element groups of 32-element blocks


@pytest.mark.parametrize("n,want", [(2048, (STAGED, 1, 32, 16)), (1920, (STAGED, 2, 64, 15))])
def test_staged_ks(plan, n, want):
    """2-bit (no producer / consumer form): KS 1 from 32 x 16 = 512 staged tiles"""
    p = plan(LINEAR, [mat(4096, 1024, type=T_SIGN)], n)
    assert (p.route, p.k.fmt) == (TILE, FMT_Q2)
    assert kern(p)[:4] == want


def test_gemm_min(plan):
    assert plan(LINEAR, [mat(1024, 1024)], 7).route == MATVEC
    assert plan(LINEAR, [mat(1024, 1024)], 8).route == TILE


# ---- bf16 operands: the kf_gemm3.hip tiles first from 256 rows (g3_first), big tiles from 160 of them, 128 x 128, 64 x 128 from 192 of those, 64 x 64 below
@pytest.mark.parametrize("M,n,want", [
    (1024, 255, (DIRECT, 32, 32, 8, 512, 32768)),            # below 256 rows and direct-sized: the global_load_lds tiles are not tried
    (1024, 256, (G3, TINY, 64, 1, 256, 32768)),              # 8 x 2 small tiles < 32 but 16 x 4 = 64 tiny ones; 16 x 2 mid tiles < 192
    (1024, 1024, (G3, TINY, 256, 1, 256, 32768)),            # 16 x 8 = 128 mid < 192
    (1024, 1408, (G3, TINY, 352, 1, 256, 32768)),            # 16 x 11 = 176 mid
    (1024, 1536, (G3, MID, 192, 1, 256, 49152)),             # 16 x 12 = 192 mid
    (4096, 2304, (G3, SMALL, 576, 1, 256, 65536)),           # 16 x 9 = 144 big < 160; 32 x 18 small >= 256
    (4096, 2560, (G3, BIG, 160, 1, 512, 131072)),            # 16 x 10 = 160 big
    (128, 256, (DIRECT, 32, 4, 8, 512, 32768)),              # 1 x 2 small < 32 and 2 x 4 tiny < 64: kf_gemm3.hip declines, the direct kernel takes it
    (6400, 224, (G3, MID, 200, 1, 256, 49152)),              # n < 256 past the direct size (200 x 7 > 1280): kf_gemm3.hip without a workspace
])
def test_linear_bf16_kernels(plan, M, n, want):
    p = plan(LINEAR, [mat(M, 1024, type=BF16)], n, scratch=LOTS)
    assert (p.route, p.deq) == (TILE, DQ_NONE)
    assert kern(p) == want
    assert p.k.sk == 0                                        # no workspace is lent on this route


# ---- the resident route (an arena, from 320 rows): the scratch lends the split-K slots of the 64-row tiles
def test_resident_split_k(plan):
    Q = [mat(1024, 3072)]
    p = plan(LINEAR, Q, 512, arena=1, arena_free=LOTS, scratch=SK_BYTES)
    assert (p.route, p.deq, p.deq_bytes, p.ws_bytes) == (RESIDENT, DQ_ARENA, 1024 * 3072 * 2, SK_BYTES)
    assert kern(p)[:2] == (G3, TINY)
    # 16 x 8 = 128 tiny tiles < 4/5 of 1280 resident workgroups: S = 10 cut down while 48 k-steps / S < 8 -> 6 pieces, 768 workgroups
    assert sk(p) == (1, 128, 6, 0, 1, 768)
    p = plan(LINEAR, Q, 512, arena=1, arena_free=LOTS, scratch=SK_BYTES - 1)
    assert (p.route, p.ws_bytes, sk(p)) == (RESIDENT, 0, (0, 0, 0, 0, 0, 128))
    p = plan(LINEAR, Q, 512, arena=1, arena_hit=1 << STACK, scratch=SK_BYTES)
    assert (p.route, p.deq) == (RESIDENT, DQ_RESIDENT)


def test_resident_bounds(plan):
    Q = [mat(1024, 3072)]
    assert plan(LINEAR, Q, 319, arena=1, arena_free=LOTS).route == TILE
    assert plan(LINEAR, Q, 320, arena=1, arena_free=LOTS).route == RESIDENT
    assert plan(LINEAR, Q, 512, arena=1, arena_free=1024 * 3072 * 2 - 1, scratch=LOTS).route == TILE     # no room: the arena-only copy is not made in the scratch
    assert plan(LINEAR, Q, 512, arena=1, arena_free=LOTS, capturing=1).route == TILE                     # a capture would replay the fill
    assert plan(LINEAR, [mat(127, 3072)], 512, arena=1, arena_free=LOTS).route == TILE
    assert plan(LINEAR, [mat(1024, 3072, type=BF16)], 512, arena=1, arena_free=LOTS).route == TILE
    assert plan(LINEAR, [mat(1024, 64)], 512, arena=1, arena_free=LOTS, scratch=LOTS).route == MATVEC   # K 64: no tile kernel takes the copy either


# ---- dequantise + tile into the scratch: from 2048 rows, M >= 256, and >= 128 big or >= 256 small tiles
@pytest.mark.parametrize("M,n,route", [
    (1024, 4096, DEQ_TILE),      # 4 x 16 = 64 big, 8 x 32 = 256 small
    (1024, 4095, DEQ_TILE),
    (1024, 3968, TILE),          # 8 x 31 = 248 small
    (1024, 2048, TILE),          # 32 big, 128 small
    (4096, 2048, DEQ_TILE),      # 16 x 8 = 128 big
    (4096, 2047, TILE),          # below 2048 rows
    (255, 1 << 16, TILE),        # M < 256
])
def test_deq_tile(plan, M, n, route):
    p = plan(LINEAR, [mat(M, 1024)], n, scratch=LOTS)
    assert p.route == route
    if route == DEQ_TILE:
        assert (p.deq, p.deq_bytes, p.ws_bytes, p.k.fam, p.k.sk) == (DQ_SCRATCH, M * 1024 * 2, 0, G3, 0)


def test_deq_tile_scratch(plan):
    assert plan(LINEAR, [mat(1024, 1024)], 4096, scratch=1024 * 1024 * 2).route == DEQ_TILE
    p = plan(LINEAR, [mat(1024, 1024)], 4096, scratch=1024 * 1024 * 2 - 1)
    assert (p.route, kern(p)[:3]) == (TILE, (G2, 0, 8))


# ---- storage forms
def test_storage_forms(plan):
    assert plan(LINEAR, [mat(1024, 1024, awq=1)], 64).route == AWQ
    p = plan(LINEAR, [mat(1024, 1024, type=Q3, quant=ROW_LUT)], 64)                # 3-bit row codebook: GetDataX into the scratch, the bf16 direct kernel on the copy
    assert (p.route, p.deq, p.deq_bytes, kern(p)[:4]) == (ROWFORM, DQ_SCRATCH, 1024 * 1024 * 2, (DIRECT, 32, 32, 2))
    p = plan(LINEAR, [mat(1024, 1024, type=Q3, quant=ROW_LUT)], 1)                 # one token: the mat-vec on the copy
    assert (p.route, p.k.fam) == (ROWFORM, NONE)
    p = plan(LINEAR, [mat(1024, 1024, quant=ROW_LUT)], 64)                         # 4-bit row codebook: unpacked in registers
    assert (p.route, p.k.fmt, kern(p)[:2]) == (TILE, FMT_Q4R, (DIRECT, 32))
    p = plan(LINEAR, [mat(1024, 96, quant=ROW_LUT)], 64, scratch=LOTS)             # K 96: no tile kernel, nothing dequantised
    assert (p.route, p.deq) == (MATVEC, DQ_NONE)
    assert plan(LINEAR, [mat(1024, 1024, quant=ROW_LUT, al=1)], 64).route == MATVEC   # row tables not 16-byte aligned, no scratch lent
    # row tables not 16-byte aligned (a 50257 x 768 head: the tables sit right behind the nibble stream) with the scratch lent: GetDataX into it, the bf16 tiles on the
    # copy -- 197 x 2 = 394 big tiles at 512 rows
    p = plan(LINEAR, [mat(50257, 768, quant=ROW_LUT, al=1)], 512, scratch=50257 * 768 * 2)
    assert (p.route, p.deq, p.deq_bytes, kern(p)) == (ROWFORM, DQ_SCRATCH, 50257 * 768 * 2, (G3, BIG, 394, 1, 512, 131072))
    p = plan(LINEAR, [mat(1024, 1024, quant=ROW_LUT, al=1)], 64, scratch=1024 * 1024 * 2)   # the same below 256 rows: the bf16 direct kernel
    assert (p.route, p.deq, kern(p)[:4]) == (ROWFORM, DQ_SCRATCH, (DIRECT, 32, 32, 2))
    assert plan(LINEAR, [mat(1024, 1024, quant=ROW_LUT, al=1)], 64, scratch=1024 * 1024 * 2 - 1).route == MATVEC
    assert plan(LINEAR, [mat(1024, 1024, quant=ROW_LUT, al=1)], 7, scratch=LOTS).route == MATVEC             # below GEMM_MIN rows: the mat-vec reads the stream
    p = plan(LINEAR, [mat(1024, 1024, lgroup=96)], 64)                             # a group the tile kernels cannot index
    assert (p.route, p.status) == (TILE, -701)
    assert plan(LINEAR, [mat(1024, 1024, lgroup=96)], 512, arena=1, arena_free=LOTS).route == RESIDENT
    assert plan(LINEAR, [mat(1024, 1024)], 64, x_al=0).route == MATVEC            # misaligned x
    assert plan(LINEAR, [mat(1024, 1600, type=T_SIGN, lgroup=64)], 64).route == MATVEC   # 2-bit needs K a multiple of 128
    assert plan(LINEAR, [mat(1024, 1600, lgroup=64)], 64).route == TILE               # 4-bit: 64 is enough (GPT-2's 1600)


# ---- several matrices sharing x
QKV = [mat(1024, 1024), mat(256, 1024), mat(256, 1024)]       # 32 + 8 + 8 = 48 row blocks


@pytest.mark.parametrize("n,want", [
    (320, (FUSED, (DIRECT, 32, 48, 10, 512, 32768))),        # 48 x 5 64-token tiles = 240 < 256
    (321, (FUSED, (DIRECT, 64, 48, 6, 512, 65536))),
    (1344, (FUSED, (DIRECT, 64, 48, 21, 512, 65536))),       # 48 x 42 = 2016 <= GD_FUSED_MAX
    (1345, (SEPARATE, (NONE, 0, 0, 0, 0, 0))),               # 48 x 43 = 2064
])
def test_multi_fused(plan, n, want):
    p = plan(MULTI, QKV, n)
    assert (p.route, kern(p)) == want


def test_paired(plan):
    GU = [mat(3072, 1024), mat(3072, 1024)]
    p = plan(GATEUP, GU, 672)
    assert (p.route, kern(p)) == (FUSED, (PAIRED, 32, 96, 21, 512, 65536))   # 96 x 21 = 2016
    assert plan(GATEUP, GU, 673).route == SEPARATE
    assert plan(GATEUP, [mat(3072, 1024), mat(3072, 1024, type=F8)], 64).route == SEPARATE
    assert plan(GATEUP, [mat(1024, 1024, type=BF16)] * 2, 255).route == FUSED   # bf16 storage: the fused launch below 256 rows only (g3_first)
    assert plan(GATEUP, [mat(1024, 1024, type=BF16)] * 2, 256).route == SEPARATE
    assert plan(MULTI, [mat(1024, 1024, type=BF16)] * 3, 255).route == FUSED
    assert plan(MULTI, [mat(1024, 1024, type=BF16)] * 3, 256).route == SEPARATE
    assert plan(MULTI, QKV, 320, x_al=0).route == SEPARATE
    assert plan(MULTI, [mat(1024, 1024), mat(256, 1024, lgroup=96)], 64).status == -701


def test_stacked(plan):
    Q3 = [mat(1024, 1024)] * 3                                # 3072 rows
    p = plan(MULTI, Q3, 1024, scratch=LOTS)                   # 12 x 4 = 48 big tiles < 64 but 24 x 8 = 192 small
    assert (p.route, p.deq, p.deq_form, p.deq_bytes, kern(p)) == (STACKED, DQ_SCRATCH, STACK, 3 * 1024 * 1024 * 2, (G3, SMALL, 192, 1, 256, 65536))
    assert plan(MULTI, Q3, 1023, scratch=LOTS).route == SEPARATE                   # no arena: from 1024 rows; 96 x 32 > GD_FUSED_MAX
    assert plan(MULTI, Q3, 1024, scratch=3 * 1024 * 1024 * 2 - 1).route == SEPARATE
    p = plan(MULTI, Q3, 320, arena=1, arena_free=LOTS)        # with an arena from 320 rows
    assert (p.route, p.deq) == (STACKED, DQ_ARENA)
    assert plan(MULTI, Q3, 319, arena=1, arena_free=LOTS).route == FUSED
    p = plan(MULTI, [mat(4096, 1024)] * 2, 2560, scratch=LOTS)   # 32 x 10 = 320 big tiles
    assert kern(p)[:3] == (G3, BIG, 320)
    p = plan(MULTI, [mat(4096, 1024), mat(1024, 1024)], 8192, scratch=LOTS)   # 20 x 32 = 640 big
    assert kern(p)[:3] == (G3, BIG, 640)
    p = plan(MULTI, [mat(2048, 1024), mat(1024, 1024)], 2048, scratch=LOTS)   # 12 x 8 = 96 big < 160: 24 x 16 small
    assert kern(p)[:3] == (G3, SMALL, 384)
    # 64-tile floor: 2 x 256 rows -- 2 x 8 big and 4 x 16 = 64 small at 2048 rows, 60 at 1920
    assert plan(MULTI, [mat(256, 1024)] * 2, 2048, scratch=LOTS).route == STACKED
    assert plan(MULTI, [mat(256, 1024)] * 2, 1920, scratch=LOTS).route == FUSED
    assert plan(MULTI, [mat(1024, 1024), mat(1024, 1024), mat(384, 1024)], 4096, scratch=LOTS).route == SEPARATE   # 384 rows: not a multiple of 256
    assert plan(MULTI, Q3, 1024, scratch=LOTS, x_al=0).route == SEPARATE


def test_gateup_swiglu(plan):
    GU = [mat(1024, 1024)] * 2
    p = plan(GATEUP, GU, 1024, scratch=LOTS)                  # 2048 interleaved rows: 8 x 4 = 32 big < 160, 2048 % 192 != 0: 16 x 8 small
    assert (p.route, p.deq, p.deq_form, kern(p)) == (SWIGLU, DQ_SCRATCH, ILV, (G3, SMALL, 128, 1, 256, 65536))
    p = plan(GATEUP, GU, 1024, scratch=LOTS, y_al=0)          # act not 8-byte aligned: the stacked route, nothing dequantised interleaved
    assert (p.route, p.deq_form) == (STACKED, STACK)
    p = plan(GATEUP, GU, 1024, arena=1, arena_free=LOTS, arena_hit=1 << STACK)
    assert (p.route, p.deq) == (SWIGLU, DQ_ARENA)
    p = plan(GATEUP, GU, 1024, arena=1, arena_free=0, arena_hit=1 << STACK)   # no room for the interleaved copy: the resident stacked one
    assert (p.route, p.deq) == (STACKED, DQ_RESIDENT)
    assert plan(GATEUP, [mat(1152, 1024)] * 2, 1024, scratch=LOTS).route == FUSED   # 1152 rows: not a multiple of 256; 36 x 32 paired workgroups


@pytest.mark.parametrize("ffn,n,want", [
    (3072, 2047, (G3, WIDE, 256, 1, 512, 114688)),           # 24 x 8 = 192 big in 160 .. 255, 32 x 8 = 256 wide
    (3072, 2049, (G3, BIG, 216, 1, 512, 131072)),            # 32 x 9 = 288 wide > 256
    (3072, 1536, (G3, WIDE, 192, 1, 512, 114688)),           # 24 x 6 = 144 big, but 48 x 12 = 576 small > 512 and 32 x 6 = 192 wide >= 160
    (3072, 1280, (G3, SMALL, 480, 1, 256, 65536)),           # 48 x 10 = 480 small
    (4096, 2048, (G3, BIG, 256, 1, 512, 131072)),            # 32 x 8 = 256 big
])
def test_gateup_tiles(plan, ffn, n, want):
    p = plan(GATEUP, [mat(ffn, 1024)] * 2, n, scratch=LOTS)
    assert (p.route, kern(p)) == (SWIGLU, want)


def test_rope(plan):
    QKV = [mat(2048, 1024), mat(1024, 1024), mat(1024, 1024)]
    p = plan(ROPE, QKV, 4096, rope_ok=1, scratch=LOTS)        # always the head-sized 128 x 128 tile: 32 x 32
    assert (p.route, p.deq, kern(p)) == (ROPE_EPI, DQ_SCRATCH, (G3, SMALL, 1024, 1, 256, 65536))
    assert kern(plan(MULTI, QKV, 4096, scratch=LOTS))[:3] == (G3, BIG, 256)   # the plain stacked launch: 16 x 16 big
    p = plan(ROPE, QKV, 4096, rope_ok=1, y_al=0, scratch=LOTS)   # q / k not 8-byte aligned: kf_linear_multi, nothing dequantised here
    assert (p.route, p.deq) == (SEPARATE, DQ_NONE)
    assert plan(ROPE, QKV, 4096, rope_ok=0, scratch=LOTS).route == SEPARATE
    assert plan(ROPE, QKV, 1023, rope_ok=1, scratch=LOTS).route == SEPARATE
    assert plan(ROPE, QKV, 320, rope_ok=1, arena=1, arena_free=LOTS).route == ROPE_EPI


# ---- kf_linear_backward: kf_gemm3.hip on the k-major operands, 128 x 128 tiles when the big ones fill < 4/5 of the CUs and the small ones make (nearly) whole
# rounds of 512 or split-K applies; the transposed copies on the token-batch tiles below 256 rows
def bwd(plan, entry, OC, IC, n):
    return plan(entry, [mat(OC, IC, type=BF16)], n, scratch=SK_BYTES)


def test_backward_kmajor(plan):
    p = bwd(plan, BWD_DX, 1024, 1024, 2048)                   # 4 x 8 big; 8 x 16 = 128 small, split-K: 16 k-steps, S 4 -> 2
    assert (p.route, p.k.akm, p.k.bkm, kern(p)[:2], sk(p)) == (KMAJOR, 1, 0, (G3, SMALL), (1, 128, 2, 0, 1, 256))
    p = bwd(plan, BWD_DW, 1024, 1024, 2048)                   # M 1024 x K 2048 x 1024: 8 x 8 small, S 8 -> 4 (32 k-steps)
    assert (p.route, p.k.akm, p.k.bkm, kern(p)[:2], sk(p)) == (KMAJOR, 1, 1, (G3, SMALL), (1, 64, 4, 0, 1, 256))
    p = bwd(plan, BWD_DX, 4096, 4096, 8192)                   # 16 x 32 = 512 big: plain
    assert (kern(p)[:3], p.k.sk) == ((G3, BIG, 512), 0)
    p = bwd(plan, BWD_DX, 1024, 3072, 4096)                   # 12 x 16 = 192 big; 768 small in 2 rounds: big, owner steps 12 of 16 < 32: plain
    assert (kern(p)[:3], p.k.sk) == ((G3, BIG, 192), 0)
    p = bwd(plan, BWD_DX, 1024, 2048, 3584)                   # 16 x 28 = 448 small: 20 x 448 >= 17 x 512
    assert (kern(p)[:3], p.k.sk) == ((G3, SMALL, 448), 0)
    p = bwd(plan, BWD_DX, 1024, 2048, 3328)                   # 416 small < 17/20 of a round, 5 x 416 >= 2048: big 8 x 13 = 104 split S 2
    assert (kern(p)[:2], sk(p)) == ((G3, BIG), (1, 104, 2, 0, 1, 208))


def test_backward_transpose(plan):
    p = bwd(plan, BWD_DX, 1024, 1024, 128)                    # n < 256
    assert (p.route, kern(p)[:4]) == (TRANSPOSE, (DIRECT, 32, 32, 4))
    p = bwd(plan, BWD_DW, 128, 1024, 2048)                    # OC 128 token rows < 256: y [128, 1024] over K = 2048
    assert (p.route, kern(p)[:4]) == (TRANSPOSE, (DIRECT, 32, 32, 4))
    assert bwd(plan, BWD_DX, 1024, 200, 2048).route == TRANSPOSE   # IC 200 < 256 rows


# ---- the scratch queries: exactly the parent's values
@pytest.mark.parametrize("type,quant,M,K,n,want", [
    (Q4, GROUP, 1024, 1024, 2048, 1024 * 1024 * 2),   # non-bf16 group storage, >= 2048 rows, M >= 256, K % 64 == 0
    (Q4, GROUP, 256, 1024, 2048, 256 * 1024 * 2),     # the over-ask: the route's tile-count test (1 x 8 big, 2 x 16 small) then declines
    (Q4, GROUP, 1024, 1024, 2047, 0),
    (Q4, GROUP, 255, 1024, 4096, 0),
    (Q4, GROUP, 1024, 1600, 4096, 1024 * 1600 * 2),
    (Q4, GROUP, 1024, 96, 4096, 0),
    (BF16, GROUP, 1024, 1024, 4096, 0),
    (T_SIGN, GROUP, 1024, 1024, 4096, 1024 * 1024 * 2),
    (Q4, ROW_LUT, 1024, 1024, 1, 1024 * 1024 * 2),    # row forms: at any batch, the 4-bit row codebook too
    (Q3, ROW_LUT, 512, 256, 64, 512 * 256 * 2),
    (Q4, GROUP, 1024, 1024, 0, 0),
])
def test_linear_scratch_bytes(hip, type, quant, M, K, n, want):
    w = L.Weight()
    w.type, w.quant, w.ne0, w.ne1, w.lGroup = type, quant, M, K, 128
    assert hip.kf_linear_scratch_bytes(C.byref(w), n) == want


def test_multi_scratch_bytes(hip):
    def q(shapes, n):
        ws = [L.Weight() for _ in shapes]
        for w, (M, K) in zip(ws, shapes):
            w.type, w.quant, w.ne0, w.ne1, w.lGroup = Q4, GROUP, M, K, 128
        arr = (C.POINTER(L.Weight) * len(ws))(*[C.pointer(w) for w in ws])
        return hip.kf_linear_multi_scratch_bytes(len(ws), C.cast(arr, C.c_void_p), n)
    qkv = [(2048, 1024), (1024, 1024), (1024, 1024)]
    for n in (1, 512, 1023):
        assert q(qkv, n) == 0                                  # below 1024 rows (the query assumes no arena)
    for n in (1024, 2048, 8192):
        assert q(qkv, n) == 4096 * 1024 * 2
    assert q([(256, 1024)] * 2, 2048) == 2 * 256 * 1024 * 2   # 4 x 16 = 64 small tiles
    assert q([(256, 1024)] * 2, 1920) == 0                    # 60
    assert q([(1024, 1024), (384, 1024)], 4096) == 0          # 384: not a multiple of 256
    assert q([(1024, 1024), (1024, 1088)], 4096) == 0         # input widths differ
    assert q([(1024, 1024)], 4096) == 0                       # one matrix
    assert q([(1024, 1024), (1024, 96)], 4096) == 0
