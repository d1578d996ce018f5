// kf_f8a8.h -- fp8 activations for f8e5m2 layers (include/kf_abi.h "fp8 activations for f8e5m2 layers"): kf_act_quant_f8 (per-token e4m3 codes with a power-of-two step,
// kf_act_quant.hip) and kf_linear_f8a8 (codes x the stored e5m2 bytes on v_mfma_f32_16x16x128_f8f6f4, kf_gemm_f8a8.hip).  kf::f8a8_plan, one pure host function, makes
// every decision -- the refusals, the tile form, grid, block, LDS; the launcher carries out what it returns and decides nothing.
// The bits do NOT depend on any of the plan's figures: an output element's fp32 accumulator takes the row's 128-byte steps in ONE ascending chain of n_steps MFMA
// instructions (F8A8_ORDER_CHAIN), element k always in slot k % 128 of step k / 128, whatever tile form holds it: no split-K, no second accumulator.  `order` and
// `n_steps` name that order: functions of K alone.
#pragma once
#include "kf_kernels.h"

namespace kf {

enum { F8A8_ORDER_CHAIN = 1 };          /* acc = 0; acc = mfma(codes of step s, weight bytes of step s, acc) for s = 0, 1, ... n_steps - 1 */
enum { F8A8_TOK16 = 0, F8A8_TOK32 = 1, F8A8_TOK64 = 2, F8A8_WIDE = 3, F8A8_N_FORMS = 4 };   /* the tile forms */
constexpr int F8A8_STEP = 128;          /* bytes of K per MFMA step: the K of v_mfma_f32_16x16x128_f8f6f4 */
constexpr int F8A8_K_UNIT = 64;         /* K is a multiple of this: a row's last step is whole or half, the half zero-filled in LDS */
constexpr int F8A8_ROW_TILE = 128;      /* weight rows of one workgroup, every form */
constexpr int F8A8_THREADS = 256;       /* four waves */
constexpr int F8A8_STAGES = 2;          /* LDS buffers: the loads of step s + 1 fly while step s is multiplied */
constexpr int F8A8_FILL = 256;          /* workgroups a launch should have before the token tile widens: one per CU of an MI355X */
constexpr int F8A8_MIN_TOK = KF_F8A8_TILE_MIN; /* the host's default threshold (Fish::Group): token batches of at least this many rows take this route */

// a form: WR x WT waves, each MT x NT MFMA tiles of 16 weight rows x 16 tokens.  WR * MT * 16 = F8A8_ROW_TILE for every form.
struct F8A8Form {
    int wr, wt, mt, nt, tok_tile;
};
constexpr F8A8Form F8A8_FORMS[F8A8_N_FORMS] = {{4, 1, 2, 1, 16}, {4, 1, 2, 2, 32}, {4, 1, 2, 4, 64}, {2, 2, 4, 4, 128}};
constexpr int f8a8_stage_bytes(int form) { return (F8A8_ROW_TILE + F8A8_FORMS[form].tok_tile) * F8A8_STEP; }

struct F8A8Problem {
    GemmMat w;
    int nTok;
    int q_al; /* the codes are 16-byte aligned */
};
struct F8A8Plan {
    int status;          /* KF_OK, or the refusal: everything below but min_tok is 0 then */
    int order, n_steps;  /* F8A8_ORDER_CHAIN over n_steps = ceil(K / 128): functions of K only */
    int half_tail;       /* the last step holds 64 bytes of K; its upper half is zero-filled */
    int form;            /* F8A8_TOK16 .. F8A8_WIDE */
    int row_tile, tok_tile, stages;
    int grid_x, grid_y, block, lds;
    int min_tok;
};

// the widest token tile that still leaves F8A8_FILL workgroups, and no wider than the batch (a8t_mfma_tok's rule, kf_a8.h): a small launch is one serial walk over K
// per workgroup, so there the narrow tile is the faster one
inline int f8a8_form(int M, int n) {
    const long gx = (M + F8A8_ROW_TILE - 1) / F8A8_ROW_TILE;
    int f = F8A8_WIDE;
    while (f > F8A8_TOK16 && (F8A8_FORMS[f - 1].tok_tile >= n || gx * ((n + F8A8_FORMS[f].tok_tile - 1) / F8A8_FORMS[f].tok_tile) < F8A8_FILL)) f--;
    return f;
}

// the refusals come in one order: the storage, the shape, the alignment
inline F8A8Plan f8a8_plan(const F8A8Problem& P) {
    F8A8Plan p = {};
    const GemmMat& m = P.w;
    p.min_tok = F8A8_MIN_TOK;
    auto refuse = [&p](int status) {
        p.status = status;
        return p;
    };
    if (!(m.type == KF_F8E5M2 && m.quant == KF_QUANT_GROUP && !m.awq)) return refuse(KF_UNSUPPORTED_DATATYPE);
    if (m.K < F8A8_STEP || m.K % F8A8_K_UNIT != 0 || m.M < 1 || P.nTok < 1) return refuse(KF_INVALID_ARGS);
    if (!(m.al & GM_DATA_AL) || !P.q_al) return refuse(KF_BLAS_UNALIGN);
    p.order = F8A8_ORDER_CHAIN, p.n_steps = (m.K + F8A8_STEP - 1) / F8A8_STEP, p.half_tail = m.K % F8A8_STEP != 0;
    p.form = f8a8_form(m.M, P.nTok);
    p.row_tile = F8A8_ROW_TILE, p.tok_tile = F8A8_FORMS[p.form].tok_tile, p.stages = F8A8_STAGES;
    p.lds = F8A8_STAGES * f8a8_stage_bytes(p.form);
    p.grid_x = (m.M + p.row_tile - 1) / p.row_tile, p.grid_y = (P.nTok + p.tok_tile - 1) / p.tok_tile, p.block = F8A8_THREADS;
    return p;
}

// the launchers: each carries out what it is given; KF_OK or KF_HIP_CHECK
int f8a8_run(hipStream_t st, const F8A8Plan& p, const kf_weight* w, const uint8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok); /* kf_gemm_f8a8.hip */
int act_quant_f8_launch(hipStream_t st, const uint16_t* x, long long ldx, const uint16_t* norm_w, float eps, int rows, int dim, uint8_t* q, float* step);                        /* kf_act_quant.hip */

}  // namespace kf
