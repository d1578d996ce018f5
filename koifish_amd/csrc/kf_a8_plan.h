// kf_a8_plan.h -- how kf_linear_a8 (1-bit / ternary weights x int8 activations, include/kf_abi.h "int8 activations") is launched: kf::a8_plan, one pure host function,
// makes every decision -- the refusals, the lanes per row (rows per wave), the token rows per weight pass, grid and LDS; the launcher (kf_gemv_a8.hip) carries out what it
// returns and decides nothing.
// The bits do NOT depend on any of these figures: a 128-weight group's integer sum I_g is exact whatever lanes form it, and the fp32 products step_w[g] * I_g of a row are
// added in ONE ascending chain over the group index g = 0 .. K/128 - 1 (A8_ORDER_CHAIN), whoever holds them.  `order` and `n_groups` name that order: functions of K alone.
#pragma once
#include "kf_kernels.h"

namespace kf {

enum { A8_ORDER_CHAIN = 1 };            /* acc = 0; acc = acc + step_w[g] * I_g for g = 0, 1, ... (fp32, one add per group) */
constexpr int A8_GROUP = 128;           /* weights per group = per lane and step: one 16-byte block of 1-bit codes, two of 2-bit codes */
constexpr int A8_TOK_TILE = 4;          /* token rows a weight block is dotted against once unpacked (nTok > 1) */
constexpr int A8_THREADS = 256;         /* four waves per workgroup */
constexpr int A8_LPR_MIN_LOG2 = 3;      /* a row whose group count has no larger power-of-two factor gets min(8, groups) lanes, the tail of the last step masked */
constexpr int A8_GROUP_LDS = 144;       /* bytes of LDS per group and token row: 128 staged int8 + its sum (int32) + pad; 36 dwords apart keeps 16 lanes' 16-byte reads on distinct banks */
constexpr size_t A8_LDS_MAX = 160 * 1024;

struct A8Problem {
    GemmMat w;
    int nTok;
};
struct A8Plan {
    int status;           /* KF_OK, or the refusal */
    int bits;             /* 1 or 2 */
    int order, n_groups;  /* the per-row summation order: A8_ORDER_CHAIN over n_groups = K / 128 -- functions of K only */
    int lpr_log2, iters;  /* lanes per row and the steps each makes */
    int rows_per_wave, rows_per_wg;
    int tok_tile, tok_tiles;
    int grid_x, grid_y, block, lds;
};

// lanes per row (log2) of the integer mat-vecs (this plan and kf_w4a8_plan.h): the largest power of two <= 64 that divides the row's groups; a row without such a factor of
// at least 8 gets min(8, groups) lanes rounded down to a power of two, the tail of the last step masked
inline int a8_lanes_log2(int n_groups) {
    int l = 6;
    while (l > 0 && (n_groups % (1 << l)) != 0) l--;
    if (l < A8_LPR_MIN_LOG2) {
        l = A8_LPR_MIN_LOG2;
        while ((1 << l) > n_groups) l--;
    }
    return l;
}

inline A8Plan a8_plan(const A8Problem& P) {
    A8Plan p = {};
    auto refuse = [&p](int status) {
        p.status = status;
        return p;
    };
    const GemmMat& m = P.w;
    const bool served = m.quant == KF_QUANT_GROUP && !m.awq && (m.type == KF_T_SIGN || m.type == KF_BOOL1 || m.type == KF_T_BINARY);
    if (!served) return refuse(KF_UNSUPPORTED_DATATYPE);
    if (m.lgroup != A8_GROUP || !m.gama) return refuse(KF_QUANT_ERR);
    if (m.K < A8_GROUP || m.K % A8_GROUP != 0 || m.M < 1 || P.nTok < 1) return refuse(KF_INVALID_ARGS);
    if (!(m.al & GM_DATA_AL)) return refuse(KF_BLAS_UNALIGN);
    p.bits = m.type == KF_T_SIGN ? 2 : 1;
    p.order = A8_ORDER_CHAIN, p.n_groups = m.K / A8_GROUP;
    const int l = a8_lanes_log2(p.n_groups);
    p.lpr_log2 = l, p.iters = (p.n_groups + (1 << l) - 1) >> l;
    p.rows_per_wave = 64 >> l, p.rows_per_wg = p.rows_per_wave * (A8_THREADS / 64);
    p.tok_tile = P.nTok > 1 ? A8_TOK_TILE : 1;
    p.tok_tiles = (P.nTok + p.tok_tile - 1) / p.tok_tile;
    p.lds = p.tok_tile * p.n_groups * A8_GROUP_LDS;
    if ((size_t)p.lds > A8_LDS_MAX) return refuse(KF_INVALID_ARGS);
    p.grid_x = (m.M + p.rows_per_wg - 1) / p.rows_per_wg, p.grid_y = p.tok_tiles, p.block = A8_THREADS;
    return p;
}

// ---- the launchers (kf_gemv_a8.hip, kf_act_quant.hip): each carries out what it is given; KF_OK or KF_HIP_CHECK
int a8_launch(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok);
int act_quant_launch(hipStream_t st, const uint16_t* x, long long ldx, const uint16_t* norm_w, float eps, int rows, int dim, int8_t* q, float* step);

}  // namespace kf
