// kf_w4a8_plan.h -- how kf_linear_w4a8 and kf_linear_w4a8_tiles (4-bit group weights x int8 activations, include/kf_abi.h "int8 activations for 4-bit layers") are
// launched: kf::w4a8_plan (mat-vec on v_dot4c_i32_i8) and kf::w4a8_tile_plan (int8 MFMA tiles), pure host functions that make every decision -- the refusals, the lanes
// per row, the token rows per weight pass, tiles, chunk, grid and LDS; the launchers (kf_gemv_w4a8.hip, kf_gemm_w4a8.hip) carry out what they return and decide nothing.
// The bits do NOT depend on any of these figures: a 128-weight group's integer sums I_g and S_g are exact whatever lanes form them, and the group's fp32 term
// c_g = STEP[g] * I_g - ZERO[g] * S_g (one multiply, one exact multiply, one subtract) is added to the row's accumulator in ONE ascending chain over g = 0 .. K/128 - 1
// (A8_ORDER_CHAIN, as kf_a8_plan.h), whoever holds it.  `order` and `n_groups` name that order: functions of K alone.
#pragma once
#include "kf_a8_tile_plan.h"

namespace kf {

constexpr int W4A8_BLOCKS = 4; /* 16-byte Packed128 blocks of 32 codes per 128-weight group */

// element (inside its 128-weight group) whose activation sits in byte b of staged dword j = block * 8 + dword * 2 + c: the element whose code the mask
// (D >> 4c) & 0x0F0F0F0F leaves in byte b.  A block's dword 3 holds elements 0 .. 7 with element 0 in bits 28 .. 31 (kf_gemv_blocks.h dot_q4_dword).  ONE statement for
// both kernels: they must stage in the same order for their bits to agree.
__host__ __device__ inline int w4a8_elem(int j, int b) { return (j >> 3) * 32 + (3 - ((j >> 1) & 3)) * 8 + 7 - 2 * b - (j & 1); }

struct W4A8Problem {
    GemmMat w;
    int nTok;
    int qbias; /* kf_weight::qBias: what comes off every code */
};
struct W4A8Plan {
    int status;           /* KF_OK, or the refusal */
    int qbias;            /* 0 or 8 */
    int order, n_groups;  /* the per-row summation order: A8_ORDER_CHAIN over n_groups = K / 128 -- functions of K only */
    int lpr_log2, iters;  /* lanes per row and the steps each makes */
    int rows_per_wave, rows_per_wg;
    int tok_tile, tok_tiles;
    int grid_x, grid_y, block, lds;
};

// the refusals come in a8_plan's order and with its codes: the storage, the groups, the shape, the alignment
inline W4A8Plan w4a8_plan(const W4A8Problem& P) {
    W4A8Plan p = {};
    auto refuse = [&p](int status) {
        p.status = status;
        return p;
    };
    const GemmMat& m = P.w;
    if (!(m.quant == KF_QUANT_GROUP && !m.awq && m.type == KF_Q4)) return refuse(KF_UNSUPPORTED_DATATYPE);
    if (m.lgroup != A8_GROUP || !m.gama || (P.qbias != 0 && P.qbias != 8)) return refuse(KF_QUANT_ERR);
    if (m.K < A8_GROUP || m.K % A8_GROUP != 0 || m.M < 1 || P.nTok < 1) return refuse(KF_INVALID_ARGS);
    if (!(m.al & GM_DATA_AL)) return refuse(KF_BLAS_UNALIGN);
    p.qbias = P.qbias;
    p.order = A8_ORDER_CHAIN, p.n_groups = m.K / A8_GROUP;
    const int l = a8_lanes_log2(p.n_groups); /* a8_plan's lanes per row */
    p.lpr_log2 = l, p.iters = (p.n_groups + (1 << l) - 1) >> l;
    p.rows_per_wave = 64 >> l, p.rows_per_wg = p.rows_per_wave * (A8_THREADS / 64);
    p.tok_tile = P.nTok > 1 ? A8_TOK_TILE : 1;
    p.tok_tiles = (P.nTok + p.tok_tile - 1) / p.tok_tile;
    p.lds = p.tok_tile * p.n_groups * A8_GROUP_LDS;
    if ((size_t)p.lds > A8_LDS_MAX) return refuse(KF_INVALID_ARGS);
    p.grid_x = (m.M + p.rows_per_wg - 1) / p.rows_per_wg, p.grid_y = p.tok_tiles, p.block = A8_THREADS;
    return p;
}

struct W4A8TilePlan {
    int status;              /* kf::w4a8_plan's: KF_OK, or the refusal */
    int qbias;
    int order, n_groups;     /* w4a8_plan's */
    int row_tile, tok_tile;  /* output rows and token rows of one workgroup */
    int waves, mfma_tok;     /* waves of a workgroup (16 rows each); 16-token MFMA tiles per wave */
    int chunk;               /* groups staged at a time */
    int grid_x, grid_y, block, lds;
    int min_tok;             /* A8T_MIN_TOK, for callers that route */
};

// the tile geometry is a8_tile_plan's (16 rows per wave, four waves, 1 / 2 / 4 token tiles of 16, chunks of A8T_CHUNK groups); LDS holds, per chunk, the staged
// activations with each group's sum of q, and the chunk's STEP and ZERO of the workgroup's rows as fp32
inline W4A8TilePlan w4a8_tile_plan(const W4A8Problem& P) {
    W4A8TilePlan p = {};
    const W4A8Plan v = w4a8_plan(P);
    p.status = v.status, p.min_tok = A8T_MIN_TOK;
    if (v.status != KF_OK) return p;
    p.qbias = v.qbias, p.order = v.order, p.n_groups = v.n_groups;
    const int M = P.w.M, n = P.nTok;
    p.waves = A8T_WAVES, p.row_tile = A8T_ROW_TILE;
    p.mfma_tok = a8t_mfma_tok(M, n); /* a8_tile_plan's token tile */
    p.tok_tile = p.mfma_tok * A8T_TOK_PER_MFMA;
    p.chunk = p.n_groups < A8T_CHUNK ? p.n_groups : A8T_CHUNK;
    p.lds = p.tok_tile * p.chunk * A8_GROUP_LDS + 2 * p.row_tile * p.chunk * 4;
    p.grid_x = (M + p.row_tile - 1) / p.row_tile, p.grid_y = (n + p.tok_tile - 1) / p.tok_tile, p.block = A8T_THREADS;
    return p;
}

// ---- the launchers (kf_gemv_w4a8.hip, kf_gemm_w4a8.hip): each carries out what it is given; KF_OK or KF_HIP_CHECK
int w4a8_launch(hipStream_t st, const W4A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok);
int w4a8_tiles_launch(hipStream_t st, const W4A8TilePlan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual,
                      int nTok);

}  // namespace kf
