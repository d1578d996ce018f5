// kf_a8.h -- the int8-activation products (include/kf_abi.h "int8 activations", "int8 activations for 4-bit layers"): kf_linear_a8 / kf_linear_a8_tiles (1-bit / ternary
// weights, the low-bit family) and kf_linear_w4a8 / kf_linear_w4a8_tiles (4-bit group weights, the q4 family), each on two routes: a mat-vec on v_dot4c_i32_i8 and int8
// MFMA tiles.  kf::a8_plan, one pure host function, makes every decision for all four -- the refusals, the lanes per row (rows per wave), the token rows per weight pass,
// tiles, chunk, grid and LDS; the launchers (kf_gemv_a8.hip, kf_gemm_a8.hip, kf_gemv_w4a8.hip, kf_gemm_w4a8.hip, behind kf::a8_launch) carry out what it returns and decide
// nothing.  Below the plan: the launch, and the device text the four kernels share without a change to their code -- the element maps and the output epilogue; the
// staging loops stay in the kernels: moved into a shared template they compiled to other code.
// The bits do NOT depend on any of the plan's figures: a 128-weight group's integer sums (I_g, and the q4 family's S_g) are exact whatever lanes or MFMA steps form them,
// and the group's fp32 term -- step_w[g] * I_g for the low-bit family, STEP[g] * I_g - ZERO[g] * S_g (one multiply, one exact multiply, one subtract) for q4 -- is added to
// the row's accumulator in ONE ascending chain over the group index g = 0 .. K/128 - 1 (A8_ORDER_CHAIN), whoever holds it: no split-K, no accumulator across a group
// boundary.  `order` and `n_groups` name that order: functions of K alone.
#pragma once
#include "kf_kernels.h"

namespace kf {

enum { A8_ORDER_CHAIN = 1 };            /* acc = 0; acc = acc + (the group's term) for g = 0, 1, ... (fp32, one add per group) */
enum { A8_LOWBIT = 1, A8_Q4 = 2 };      /* the family: KF_T_SIGN / KF_BOOL1 / KF_T_BINARY, or KF_Q4 */
enum { A8_MATVEC = 0, A8_TILES = 1 };   /* the route */
constexpr int A8_GROUP = 128;           /* weights per group = per lane and step: one 16-byte block of 1-bit codes, two of 2-bit codes, four of 4-bit codes */
constexpr int A8_TOK_TILE = 4;          /* token rows a weight block is dotted against once unpacked (mat-vec, nTok > 1) */
constexpr int A8_THREADS = 256;         /* four waves per workgroup */
constexpr int A8_LPR_MIN_LOG2 = 3;      /* a row whose group count has no larger power-of-two factor gets min(8, groups) lanes, the tail of the last step masked */
constexpr int A8_GROUP_LDS = 144;       /* bytes of LDS per group and token row: 128 staged int8 + its sum (int32) + pad; 36 dwords apart keeps 16 lanes' 16-byte reads on distinct banks */
constexpr int A8_GDW = A8_GROUP_LDS / 4; /* the same in dwords; dword 32 = the group's sum of q (the low-bit tiles: qBias times it) */
constexpr size_t A8_LDS_MAX = 160 * 1024;
constexpr int W4A8_BLOCKS = 4;          /* 16-byte Packed128 blocks of 32 codes per 128-weight group of 4-bit codes */
// the tile route: a wave owns 16 output rows (the A operand of v_mfma_i32_16x16x64_i8) and every token of the workgroup's token tile (16 tokens per B operand); the
// workgroup's four waves share the staged activations; the row's K is walked in chunks of at most A8T_CHUNK groups, staged in LDS chunk by chunk
constexpr int A8T_MIN_TOK = KF_A8_TILE_MIN;  /* the host's default threshold (Fish::Group): token batches of at least this many rows take the tiles: the smallest batch timed, and the tiles were the faster entry at every layer shape from there */
constexpr int A8T_ROWS_PER_WAVE = 16;        /* the M of one MFMA tile */
constexpr int A8T_TOK_PER_MFMA = 16;         /* the N of one MFMA tile */
constexpr int A8T_WAVES = 4;                 /* waves of a workgroup: they share the staged activations */
constexpr int A8T_THREADS = A8T_WAVES * 64;
constexpr int A8T_ROW_TILE = A8T_WAVES * A8T_ROWS_PER_WAVE;
constexpr int A8T_MAX_TOK_TILES = 4;         /* MFMA token tiles per wave: 1, 2 or 4 (the kernels' instantiations) */
constexpr int A8T_CHUNK = 8;                 /* groups staged in LDS at a time */
constexpr int A8T_FILL = 256;                /* workgroups a launch should have before the token tile widens: one per CU of an MI355X */

struct A8Problem {
    GemmMat w;
    int nTok;
    int qbias; /* kf_weight::qBias: what comes off every code */
    int route; /* A8_MATVEC or A8_TILES */
};
struct A8Plan {
    int status;           /* KF_OK, or the refusal: everything below but family, route and min_tok is 0 then */
    int family, route;    /* A8_LOWBIT / A8_Q4 (from w.type); the problem's route.  The figures of the route not taken are 0 */
    int bits;             /* 1, 2 or 4 */
    int qbias;            /* the problem's; q4: 0 or 8 */
    int order, n_groups;  /* the per-row summation order: A8_ORDER_CHAIN over n_groups = K / 128 -- functions of K only */
    int lpr_log2, iters;  /* mat-vec: lanes per row and the steps each makes */
    int rows_per_wave, rows_per_wg, tok_tiles;
    int row_tile, waves;  /* tiles: output rows and waves (16 rows each) of one workgroup */
    int mfma_tok, chunk;  /* tiles: 16-token MFMA tiles per wave; groups staged at a time */
    int min_tok;          /* tiles: A8T_MIN_TOK, for callers that route */
    int tok_tile;         /* token rows of one workgroup */
    int grid_x, grid_y, block, lds;
};

// lanes per row (log2) of the mat-vecs: the largest power of two <= 64 that divides the row's groups; a row without such a factor of at least 8 gets min(8, groups) lanes
// rounded down to a power of two, the tail of the last step masked
inline int a8_lanes_log2(int n_groups) {
    int l = 6;
    while (l > 0 && (n_groups % (1 << l)) != 0) l--;
    if (l < A8_LPR_MIN_LOG2) {
        l = A8_LPR_MIN_LOG2;
        while ((1 << l) > n_groups) l--;
    }
    return l;
}
// 16-token MFMA tiles per wave of the tile kernels: the widest token tile (an unpacked weight operand serves 4, 2 or 1 MFMA tiles) that still leaves A8T_FILL workgroups,
// and no wider than the batch: a small launch is one serial walk over K per workgroup, so there the narrow tile (more workgroups, each a quarter of the work) is the faster one
inline int a8t_mfma_tok(int M, int n) {
    const long gx = (M + A8T_ROW_TILE - 1) / A8T_ROW_TILE;
    int t = A8T_MAX_TOK_TILES;
    while (t > 1 && ((t / 2) * A8T_TOK_PER_MFMA >= n || gx * ((n + t * A8T_TOK_PER_MFMA - 1) / (t * A8T_TOK_PER_MFMA)) < A8T_FILL)) t /= 2;
    return t;
}

// the refusals come in one order for both families and both routes: the storage, the groups (q4: and qBias), the shape, the alignment, the mat-vec's LDS bound -- the tile
// route takes the mat-vec route's status, that last refusal included, so a matrix is served by both routes or by neither
inline A8Plan a8_plan(const A8Problem& P) {
    A8Plan p = {};
    const GemmMat& m = P.w;
    p.family = m.type == KF_Q4 ? A8_Q4 : (m.type == KF_T_SIGN || m.type == KF_BOOL1 || m.type == KF_T_BINARY) ? A8_LOWBIT : 0;
    p.route = P.route, p.min_tok = P.route == A8_TILES ? A8T_MIN_TOK : 0;
    auto refuse = [&p](int status) {
        p.status = status;
        return p;
    };
    if (!(m.quant == KF_QUANT_GROUP && !m.awq && p.family)) return refuse(KF_UNSUPPORTED_DATATYPE);
    if (m.lgroup != A8_GROUP || !m.gama || (p.family == A8_Q4 && P.qbias != 0 && P.qbias != 8)) return refuse(KF_QUANT_ERR);
    if (m.K < A8_GROUP || m.K % A8_GROUP != 0 || m.M < 1 || P.nTok < 1) return refuse(KF_INVALID_ARGS);
    if (!(m.al & GM_DATA_AL)) return refuse(KF_BLAS_UNALIGN);
    const int G = m.K / A8_GROUP, mv_tok = P.nTok > 1 ? A8_TOK_TILE : 1, mv_lds = mv_tok * G * A8_GROUP_LDS;
    if ((size_t)mv_lds > A8_LDS_MAX) return refuse(KF_INVALID_ARGS);
    p.bits = m.type == KF_Q4 ? 4 : m.type == KF_T_SIGN ? 2 : 1, p.qbias = P.qbias;
    p.order = A8_ORDER_CHAIN, p.n_groups = G;
    if (P.route == A8_MATVEC) {
        const int l = a8_lanes_log2(G);
        p.lpr_log2 = l, p.iters = (G + (1 << l) - 1) >> l;
        p.rows_per_wave = 64 >> l, p.rows_per_wg = p.rows_per_wave * (A8_THREADS / 64);
        p.tok_tile = mv_tok, p.tok_tiles = (P.nTok + mv_tok - 1) / mv_tok;
        p.lds = mv_lds;
        p.grid_x = (m.M + p.rows_per_wg - 1) / p.rows_per_wg, p.grid_y = p.tok_tiles, p.block = A8_THREADS;
    } else {
        p.waves = A8T_WAVES, p.row_tile = A8T_ROW_TILE;
        p.mfma_tok = a8t_mfma_tok(m.M, P.nTok);
        p.tok_tile = p.mfma_tok * A8T_TOK_PER_MFMA;
        p.chunk = G < A8T_CHUNK ? G : A8T_CHUNK;
        /* the staged activations (with each group's sum of q) + the chunk's weight steps as fp32 (q4: STEP and ZERO) */
        p.lds = p.tok_tile * p.chunk * A8_GROUP_LDS + (p.family == A8_Q4 ? 2 : 1) * p.row_tile * p.chunk * 4;
        p.grid_x = (m.M + p.row_tile - 1) / p.row_tile, p.grid_y = (P.nTok + p.tok_tile - 1) / p.tok_tile, p.block = A8T_THREADS;
    }
    return p;
}

// ---- the launchers: each carries out what it is given; KF_OK or KF_HIP_CHECK.  a8_launch switches on the plan's (family, route) into the four kernel files.
int a8_matvec_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok);   /* kf_gemv_a8.hip */
int a8_tiles_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok);    /* kf_gemm_a8.hip */
int w4a8_matvec_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok); /* kf_gemv_w4a8.hip */
int w4a8_tiles_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok);  /* kf_gemm_w4a8.hip */
inline int a8_launch(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok) {
    if (p.status != KF_OK) return p.status;
    if ((p.family != A8_LOWBIT && p.family != A8_Q4) || (p.route != A8_MATVEC && p.route != A8_TILES)) return KF_INVALID_ARGS; /* not a plan of a8_plan */
    if (p.family == A8_LOWBIT) return (p.route == A8_MATVEC ? a8_matvec_run : a8_tiles_run)(st, p, w, q, step, y, bias, residual, nTok);
    return (p.route == A8_MATVEC ? w4a8_matvec_run : w4a8_tiles_run)(st, p, w, q, step, y, bias, residual, nTok);
}
int act_quant_launch(hipStream_t st, const uint16_t* x, long long ldx, const uint16_t* norm_w, float eps, int rows, int dim, int8_t* q, float* step);

// raises the dynamic-LDS limit where the plan needs it, launches, folds the errors
template <class Kern, class Args>
inline int a8_go(Kern kern, const A8Plan& p, hipStream_t st, const Args& a) {
    hipError_t e = hipSuccess;
    if (p.lds > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
    if (e == hipSuccess) hipLaunchKernelGGL(kern, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, a);
    return (e == hipSuccess && hipGetLastError() == hipSuccess) ? KF_OK : KF_HIP_CHECK;
}

// ---- device side: the text the four kernels share
// The activations are staged in LDS in the order the kernels' masks leave the codes in, so the product loops hold no per-weight reversal: a8_elem / w4a8_elem give the element
// (inside its 128-weight group) whose activation sits in byte b of staged dword j -- the element whose code the mask of (dword, shift) j leaves in byte b.  ONE statement per
// width for the mat-vec and the tile kernel: they must stage in the same order for their bits to agree.
template <int BITS>
__device__ __forceinline__ int a8_elem(int j, int b) {
    if (BITS == 1) return (3 - (j >> 3)) * 32 + 31 - 8 * b - (j & 7);                   /* (D >> s) & 0x01010101; j = dword * 8 + bit */
    return (j >> 4) * 64 + (3 - ((j >> 2) & 3)) * 16 + 15 - 4 * b - (j & 3);            /* (D >> 2c) & 0x03030303; j = block * 16 + dword * 4 + code */
}
// (D >> 4c) & 0x0F0F0F0F; j = block * 8 + dword * 2 + c.  A block's dword 3 holds elements 0 .. 7 with element 0 in bits 28 .. 31 (kf_gemv_blocks.h dot_q4_dword)
__device__ __forceinline__ int w4a8_elem(int j, int b) { return (j >> 3) * 32 + (3 - ((j >> 1) & 3)) * 8 + 7 - 2 * b - (j & 1); }

// the epilogue of one output element o = tok * M + row: y = bf16(step_x * acc (+ bias)), then CU_add3: bf16(x + bf16(W.x)), as kf_linear.  The element is read and written
// by this lane alone (residual may be y).
__device__ __forceinline__ void a8_store(uint16_t* y, const uint16_t* bias, const uint16_t* residual, float sx, float acc, long row, size_t o) {
    y[o] = linear_out_bf16(sx * acc, /* alpha */ 1.0f, /* beta, y */ 0.0f, nullptr, 0, bias, row, residual, o);
}

}  // namespace kf
