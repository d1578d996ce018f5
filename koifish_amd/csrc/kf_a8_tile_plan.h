// kf_a8_tile_plan.h -- how kf_linear_a8_tiles (1-bit / ternary weights x int8 activations on the int8 MFMA, include/kf_abi.h "int8 activations") is launched:
// kf::a8_tile_plan, one pure host function, makes every decision; the launcher (kf_gemm_a8.hip) carries out what it returns and decides nothing.
//   * the refusals are kf::a8_plan's: this function calls it and takes its status -- there is no second copy of the served-storage rule;
//   * a wave owns 16 output rows (the A operand of v_mfma_i32_16x16x64_i8) and every token of the workgroup's token tile (16 tokens per B operand); the workgroup's four
//     waves share the staged activations; the token tile is 64, 32 or 16 tokens: the widest that still leaves a workgroup per CU; the row's K is walked in chunks of at most A8T_CHUNK groups, staged in LDS chunk by chunk;
//   * the bits do NOT depend on any of these figures: per group the int32 accumulators start from zero and take exactly that group's 128 weights (two MFMA steps), and the
//     group's I_g is folded ONCE into the row's fp32 chain in ascending g by the one lane that holds the output element (A8_ORDER_CHAIN, as kf_a8_plan.h): no split-K,
//     no accumulator across a group boundary.  `order` and `n_groups` are a8_plan's: functions of K alone.
#pragma once
#include "kf_a8_plan.h"

namespace kf {

constexpr int A8T_MIN_TOK = KF_A8_TILE_MIN;  /* the host's default threshold (Fish::A8Group): token batches of at least this many rows take the tiles: the smallest batch timed, and the tiles were the faster entry at every layer shape from there */
constexpr int A8T_ROWS_PER_WAVE = 16;        /* the M of one MFMA tile */
constexpr int A8T_TOK_PER_MFMA = 16;         /* the N of one MFMA tile */
constexpr int A8T_WAVES = 4;                 /* waves of a workgroup: they share the staged activations */
constexpr int A8T_THREADS = A8T_WAVES * 64;
constexpr int A8T_ROW_TILE = A8T_WAVES * A8T_ROWS_PER_WAVE;
constexpr int A8T_MAX_TOK_TILES = 4;         /* MFMA token tiles per wave: 1, 2 or 4 (the kernel's instantiations) */
constexpr int A8T_CHUNK = 8;                 /* groups staged in LDS at a time */
constexpr int A8T_FILL = 256;                /* workgroups a launch should have before the token tile widens: one per CU of an MI355X */

struct A8TilePlan {
    int status;              /* kf::a8_plan's: KF_OK, or the refusal */
    int bits;                /* 1 or 2 */
    int order, n_groups;     /* a8_plan's: A8_ORDER_CHAIN over K / 128 groups -- functions of K only */
    int row_tile, tok_tile;  /* output rows and token rows of one workgroup */
    int waves, mfma_tok;     /* waves of a workgroup (16 rows each); 16-token MFMA tiles per wave */
    int chunk;               /* groups staged at a time */
    int grid_x, grid_y, block, lds;
    int min_tok;             /* A8T_MIN_TOK, for callers that route */
};

// 16-token MFMA tiles per wave of the int8 tile kernels (this plan and kf_w4a8_plan.h): the widest token tile that still leaves A8T_FILL workgroups, and no wider than the batch
inline int a8t_mfma_tok(int M, int n) {
    const long gx = (M + A8T_ROW_TILE - 1) / A8T_ROW_TILE;
    int t = A8T_MAX_TOK_TILES;
    while (t > 1 && ((t / 2) * A8T_TOK_PER_MFMA >= n || gx * ((n + t * A8T_TOK_PER_MFMA - 1) / (t * A8T_TOK_PER_MFMA)) < A8T_FILL)) t /= 2;
    return t;
}

inline A8TilePlan a8_tile_plan(const A8Problem& P) {
    A8TilePlan p = {};
    const A8Plan v = a8_plan(P);
    p.status = v.status, p.min_tok = A8T_MIN_TOK;
    if (v.status != KF_OK) return p;
    p.bits = v.bits, p.order = v.order, p.n_groups = v.n_groups;
    const int M = P.w.M, n = P.nTok;
    p.waves = A8T_WAVES, p.row_tile = A8T_ROW_TILE;
    /* the widest token tile (an unpacked weight operand serves 4, 2 or 1 MFMA tiles) that still leaves A8T_FILL workgroups, and no wider than the batch: a small launch is
       one serial walk over K per workgroup, so there the narrow tile (more workgroups, each a quarter of the work) is the faster one */
    p.mfma_tok = a8t_mfma_tok(M, n);
    p.tok_tile = p.mfma_tok * A8T_TOK_PER_MFMA;
    p.chunk = p.n_groups < A8T_CHUNK ? p.n_groups : A8T_CHUNK;
    p.lds = p.tok_tile * p.chunk * A8_GROUP_LDS + p.row_tile * p.chunk * 4; /* the staged activations (with each group's sum of q) + the chunk's weight steps as fp32 */
    p.grid_x = (M + p.row_tile - 1) / p.row_tile, p.grid_y = (n + p.tok_tile - 1) / p.tok_tile, p.block = A8T_THREADS;
    return p;
}

// ---- the launcher (kf_gemm_a8.hip): carries out what it is given; KF_OK or KF_HIP_CHECK
int a8_tiles_launch(hipStream_t st, const A8TilePlan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual,
                    int nTok);

}  // namespace kf
