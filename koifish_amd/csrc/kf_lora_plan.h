// kf_lora_plan.h -- how kf_lora_forward and kf_lora_backward run: kf::lora_plan, one pure host function, returns the row tile, the cut of the n token rows into slabs,
// the grids, the LDS and the scratch; kf_lora.hip and the entries in kf_abi.hip execute what it returns and decide nothing.
//   * rows kernel (the forward, and the row side of the backward): a workgroup of LORA_ROW_WAVES waves owns LORA_TM token rows.  It walks the long contraction once
//     (wave w the 64-wide chunks w, w + 8, ...), the waves' partial tiles meet in LDS in wave order, the rounded [TM][r] tile is stored to memory and to LDS, then the
//     waves walk the output's 32-column blocks.  8192 rows are 256 workgroups: one per CU.  LDS: 8 partial tiles [TM][r] fp32 and the bf16 tile with padded rows.
//   * the backward's row side is THE SAME kernel on transposed copies of b and a (bT [r, OC] in a's place, aT [IC, r] in b's): the contraction index of both of its
//     products is the slow index of the adapter matrix, so the 16-byte fragments the forward reads straight from memory do not exist there.  One small launch writes
//     the two copies into the scratch first.
//   * weight side: G [M, r] = U^T . V over the n token rows (gB: U = deltaIn, V = ax, M = OC; gA^T: U = inp, V = adelta, M = IC), one launch for both.  A workgroup owns
//     LORA_BM rows of G and one slab of n; slab s of S owns the k-steps (of LORA_BK token rows) [nkt s / S, nkt (s + 1) / S).  S: enough workgroups for LORA_WG_TARGET,
//     at most LORA_MAX_SLABS, each slab at least LORA_MIN_STEPS k-steps deep.  The fp32 partials are written in the gradient's own layout ([S][r IC] for gA, [S][OC r]
//     for gB); the finish launch adds a gradient's slabs in index order and stores bf16(g + s sum).  No atomics; every partial is written before it is read.
//   * scratch, in this order, each part rounded up to 256 bytes:  adelta bf16 [n][r]  |  aT bf16 [IC][r]  |  bT bf16 [r][OC]  |  partA fp32 [SA][r][IC]  |  partB fp32 [SB][OC][r]
#pragma once
#include "kf_gemm_plan.h"

namespace kf {

constexpr int LORA_TM = 32;         /* token rows of a rows-kernel workgroup */
constexpr int LORA_ROW_WAVES = 8;   /* its waves */
constexpr int LORA_KC = 64;         /* a wave's chunk of the long contraction */
constexpr int LORA_BM = 64;         /* rows of G per weight-side workgroup: four waves of 16 */
constexpr int LORA_BK = 64;         /* token rows per k-step of the weight side */
constexpr int LORA_MAX_SLABS = 32;
constexpr int LORA_MIN_STEPS = 2;
constexpr int LORA_WG_TARGET = 512; /* two 256-thread workgroups per CU */
constexpr int LORA_FIN_BLOCK = 256; /* threads of the finish and transpose launches, one element each */

struct LoraPlan {
    int status;                   /* KF_OK, or KF_INVALID_ARGS for a shape the entries refuse */
    int tm;                       /* LORA_TM */
    int rows_gx, rows_block;      /* the rows kernel: n / tm workgroups */
    int rows_lds;
    int tr_gx;                    /* the transposes: r (IC + OC) elements */
    int SA, SB;                   /* slabs over n of gA and of gB */
    int tilesA, tilesB;           /* IC / LORA_BM, OC / LORA_BM */
    int w_gx, w_block, w_lds;     /* the weight side: tilesB SB + tilesA SA workgroups */
    int fin_gx;                   /* the finish: r (IC + OC) elements */
    long long off_adelta, off_aT, off_bT, off_partA, off_partB; /* byte offsets into the scratch */
    long long scratch;            /* bytes */
};

inline bool lora_shape_ok(int r, int OC, int IC, int n) {
    return (r == 16 || r == 32 || r == 64) && OC >= 128 && OC % 64 == 0 && IC >= 128 && IC % 64 == 0 && n >= 64 && n % 64 == 0;
}

inline int lora_rows_lds(int r) { return LORA_ROW_WAVES * LORA_TM * r * 4 + LORA_TM * (r + 8) * 2; }
inline int lora_w_lds(int r) { return LORA_BK * (LORA_BM * 2 + 16) + LORA_BK * (r * 2 + 16); }
inline int lora_slabs(int tiles, int nkt) {
    int S = (int)cdiv(LORA_WG_TARGET, tiles);
    const int deep = nkt / LORA_MIN_STEPS;
    S = S < LORA_MAX_SLABS ? S : LORA_MAX_SLABS;
    S = S < deep ? S : deep;
    return S > 1 ? S : 1;
}

inline LoraPlan lora_plan(int r, int OC, int IC, int n) {
    LoraPlan p = {};
    if (!lora_shape_ok(r, OC, IC, n)) {
        p.status = KF_INVALID_ARGS;
        return p;
    }
    p.tm = LORA_TM;
    p.rows_gx = n / LORA_TM, p.rows_block = 64 * LORA_ROW_WAVES, p.rows_lds = lora_rows_lds(r);
    const long long ne = (long long)r * ((long long)IC + OC);
    p.tr_gx = (int)cdiv(ne, LORA_FIN_BLOCK), p.fin_gx = p.tr_gx;
    const int nkt = n / LORA_BK;
    p.tilesA = IC / LORA_BM, p.tilesB = OC / LORA_BM;
    p.SA = lora_slabs(p.tilesA, nkt), p.SB = lora_slabs(p.tilesB, nkt);
    p.w_gx = p.tilesB * p.SB + p.tilesA * p.SA, p.w_block = 256, p.w_lds = lora_w_lds(r);
    p.off_adelta = 0;
    p.off_aT = up256((long long)n * r * 2);
    p.off_bT = p.off_aT + up256((long long)IC * r * 2);
    p.off_partA = p.off_bT + up256((long long)OC * r * 2);
    p.off_partB = p.off_partA + up256((long long)p.SA * r * IC * 4);
    p.scratch = p.off_partB + up256((long long)p.SB * OC * r * 4);
    return p;
}

// ---- kf_lora_apply (inference: kf_lora_apply.hip): kf::lora_apply_plan, one pure host function, picks the form from n and returns ONE adapter's share of the launch
//   * tile form, n >= 2: the rows kernel above with a row bound -- cdiv(n, LORA_TM) workgroups, rows >= n of the last tile load as zero and store nothing.
//   * vector form, n == 1: up to LORA_APPLY_MAX adapters that share the input row in one launch.  A workgroup of LORA_VEC_WAVES waves owns LORA_VEC_ROWS output rows of
//     one adapter (OC / LORA_VEC_ROWS workgroups per adapter, laid side by side in the grid); every workgroup recomputes the r dot products itself, so no workgroup waits
//     for another.  Wave w takes the ranks w, w + 16, ...; r bf16 in LDS; then one lane of wave 0 per output row.
constexpr int LORA_APPLY_MAX = 3;  /* adapters per vector-form launch: q | k | v */
constexpr int LORA_VEC_WAVES = 16; /* 1024 threads: at most r / 16 ranks per wave, so that a wave's loads of a are few and the CU hides their latency with waves */
constexpr int LORA_VEC_ROWS = 64;  /* output rows per vector-form workgroup: a lane of wave 0 each */
enum { LORA_FORM_TILE = 0, LORA_FORM_VEC = 1 };

struct LoraApplyPlan {
    int status;         /* KF_OK, or KF_INVALID_ARGS for what the entry refuses */
    int form;           /* LORA_FORM_TILE (n >= 2) or LORA_FORM_VEC (n == 1) */
    int gx, block, lds; /* this adapter's workgroups (the vector form's grid is the sum over the launch's adapters), threads, dynamic LDS bytes */
};

inline LoraApplyPlan lora_apply_plan(int r, int OC, int IC, int n, int n_w) {
    LoraApplyPlan p = {};
    const bool shape = (r == 16 || r == 32 || r == 64) && OC >= 128 && OC % 64 == 0 && IC >= 128 && IC % 64 == 0;
    if (!shape || n < 1 || n_w < 1 || n_w > LORA_APPLY_MAX || (n_w > 1 && n != 1)) {
        p.status = KF_INVALID_ARGS;
        return p;
    }
    if (n == 1)
        p.form = LORA_FORM_VEC, p.gx = OC / LORA_VEC_ROWS, p.block = 64 * LORA_VEC_WAVES, p.lds = 0;
    else
        p.form = LORA_FORM_TILE, p.gx = (int)cdiv(n, LORA_TM), p.block = 64 * LORA_ROW_WAVES, p.lds = lora_rows_lds(r);
    return p;
}

// ---- the launchers (kf_lora.hip, kf_lora_apply.hip): execute a plan, nothing else; KF_OK or KF_HIP_CHECK
// p[i] is adapter i's plan (all of one form; the tile form has n_w == 1); a / b / OC / y per adapter, r, IC, x, n and s shared; ax (tile form only) may be NULL
int lora_apply_launch(hipStream_t st, const LoraApplyPlan* p, int n_w, const uint16_t* const* a, const uint16_t* const* b, int r, const int* OC, int IC, const uint16_t* x,
                      uint16_t* const* y, uint16_t* ax, int n, float s);
int lora_forward_launch(hipStream_t st, const LoraPlan& p, const uint16_t* a, const uint16_t* b, int r, int OC, int IC, const uint16_t* x, uint16_t* y, uint16_t* ax, int n, float s);
int lora_backward_launch(hipStream_t st, const LoraPlan& p, const uint16_t* a, const uint16_t* b, int r, int OC, int IC, const uint16_t* deltaIn, const uint16_t* inp,
                         const uint16_t* ax, uint16_t* delta, uint16_t* g, int n, float s, unsigned char* scratch);

}  // namespace kf
