// kf_gemv_rows_plan.h -- how the mat-vec of R = 1 .. 8 activation rows against ONE pass over the packed weights is launched (the verify pass of speculative decoding:
// a token and its drafted continuations): kf::gemv_rows_plan, one pure host function beside kf::gemv_plan.  It takes the one-token plan of the same matrices and mode
// and keeps what fixes the bits -- the storage form, the lanes per row, the steps per row, the group shift -- so row r of the launch carries every bit of the one-token
// launch on row r; it adds the rows per workgroup pass (NR), the activation form in LDS, the cut of the rows into panels and a geometry of its own (slots per wave, grid).
// The launcher (kf_gemv_rows.hip) carries out what it returns and decides nothing.  Canonical order only (the order whose bits do not depend on the launch geometry).
#pragma once
#include "kf_gemv_plan.h"

namespace kf {

constexpr int GEMV_ROWS_MAX = 8; /* from 8 token rows up kf_linear belongs to the MFMA tiles, whose summation order differs */
// ---- the thresholds (measured: scratch/ub_verify.py)
// The activations of a panel in LDS: 80 KiB leave two workgroups (eight waves) per CU of 160 KiB.  Rows that do not fit are cut into panels of equal size, one weight
// pass each: a second pass costs more than the lost workgroup (the 4B down_proj, 2560 x 9728: four rows in one 76 KiB panel 33.7 us, five rows in panels of 3 + 2
// 49.1 us), so the cap is the largest that still overlaps two workgroups.  Smaller caps were not measured.
constexpr size_t GEMV_ROWS_LDS_MAX = 80 * 1024;
// x as fp32 in LDS (pairs_dot's form: 8 ds_read_b128 per row and block, no widening) while THREE workgroups per CU stay resident, else bf16 (4 reads, 32 widenings per
// row and block).  Measured with fp32 up to 80 KiB: the step from three resident workgroups to two costs more than the widenings save -- gate | up of the 1.7B shape
// 43.6 us at 6 rows (48 KiB) against 62.9 us at 7 (56 KiB); of the 4B shape 40.3 us at 5 rows (50 KiB), 54.1 at 6 (60 KiB), 59.1 at 7 (70 KiB) and 57.4 us at 8 rows
// as bf16 (40 KiB); its o_proj 21.3 us at 4 rows as fp32 (64 KiB) against 19.6 us at 5 rows as bf16 (40 KiB).
constexpr size_t GEMV_ROWS_XF_LDS_MAX = 53 * 1024;
constexpr int GEMV_ROWS_NR_SMALL = 4; /* the kernel is instantiated for up to 4 and up to 8 rows (accumulators and arg-max state are registers per row) */
constexpr long GEMV_ROWS_WAVES = 4096; /* waves a launch aims for, as GEMV_WAVES: 16 per CU */

struct GemvRowsProblem {
    GemvProblem one; /* the one-token problem of the same matrices, mode and order */
    int n_rows;      /* R */
};

struct GemvRowsPlan {
    int status;  /* KF_OK, or the refusal */
    int shared;  /* 1: gemv_rows_kernel, every 16-byte block unpacked once for the rows of a panel; 0: the one-token launch row by row (same bits, no sharing) */
    int fmt, mode, xf, NR; /* gemv_rows_kernel<fmt, NR, mode, xf> */
    int K, nBlk, lpr_log2, iters, lgroup, gshift; /* = the one-token plan's */
    int norm_regs; /* the one-token kernel's RMSNorm prologue sums its squares from registers (one slot per wave and K <= 4096), else in its strided pass: the same path here */
    int njobs, M[3], slot0[3], spw, total_slots;
    int n_panels, panel_rows; /* rows [i * panel_rows, min(R, (i + 1) * panel_rows)) per launch */
    int grid, lds;
};

inline GemvRowsPlan gemv_rows_plan(const GemvRowsProblem& P) {
    GemvRowsPlan p = {};
    auto refuse = [&p](int status) {
        p.status = status;
        return p;
    };
    if (P.n_rows < 1 || P.n_rows > GEMV_ROWS_MAX || P.one.sparse) return refuse(KF_INVALID_ARGS);
    const GemvPlan o = gemv_plan(P.one);
    if (o.status) return refuse(o.status);
    p.fmt = o.fmt, p.mode = o.mode, p.K = o.K, p.nBlk = o.nBlk, p.lpr_log2 = o.lpr_log2, p.iters = o.iters, p.lgroup = o.lgroup, p.gshift = o.gshift;
    p.norm_regs = o.G == 1 && (o.K >> 3) <= 512;
    p.njobs = o.njobs;
    for (int j = 0; j < 3; j++) p.M[j] = o.M[j];
    p.n_panels = P.n_rows, p.panel_rows = 1;
    // row by row: the v_dot2c order, a storage the row kernel does not take, one row, or a row too long for one panel row in LDS
    const size_t row_bf16 = (size_t)o.K * 2;
    const bool taken = o.fmt == FMT_BF16 || o.fmt == FMT_Q4 || o.fmt == FMT_Q4P;
    if (!o.canon || !taken || P.n_rows == 1 || row_bf16 + GEMV_RED_BYTES > GEMV_ROWS_LDS_MAX) return p;
    p.shared = 1;
    const int cap = (int)((GEMV_ROWS_LDS_MAX - GEMV_RED_BYTES) / row_bf16);
    p.n_panels = (P.n_rows + cap - 1) / cap;
    p.panel_rows = (P.n_rows + p.n_panels - 1) / p.n_panels;
    p.NR = p.panel_rows <= GEMV_ROWS_NR_SMALL ? GEMV_ROWS_NR_SMALL : GEMV_ROWS_MAX;
    p.xf = o.fmt != FMT_BF16 && (size_t)p.panel_rows * row_bf16 * 2 + GEMV_RED_BYTES <= GEMV_ROWS_XF_LDS_MAX;
    p.lds = (int)((size_t)p.panel_rows * row_bf16 * (p.xf ? 2 : 1) + GEMV_RED_BYTES);
    // the geometry: one slot at a time per wave, every job on a wave boundary (as gemv_plan)
    const int RPS = 64 >> o.lpr_log2;
    long rows_slots[3] = {0, 0, 0}, raw_slots = 0;
    for (int j = 0; j < p.njobs; j++) rows_slots[j] = (p.M[j] + RPS - 1) / RPS, raw_slots += rows_slots[j];
    long spw = (raw_slots + GEMV_ROWS_WAVES - 1) / GEMV_ROWS_WAVES;
    if (spw < 1) spw = 1;
    long slots = 0;
    for (int j = 0; j < 3; j++) {
        p.slot0[j] = j < p.njobs ? (int)slots : 0x7fffffff;
        if (j < p.njobs) slots += (rows_slots[j] + spw - 1) / spw * spw;
    }
    p.spw = (int)spw, p.total_slots = (int)slots;
    p.grid = (int)((slots / spw + 3) / 4); /* four waves per workgroup; <= 1025: inside KF_MAX_ARGMAX_PARTIALS per row */
    return p;
}

// ---- the launcher (kf_gemv_rows.hip)
struct GemvRowsArgs {
    GemvJob job[3];
    long long y_row_stride[3]; /* elements between the outputs of consecutive rows (beside job.y_pos_stride per position) */
    int njobs;
    int K, nBlk, lpr_log2, iters, gshift;
    int spw, total_slots;
    const uint16_t* x; /* row r at x + r * x_stride */
    long long x_stride;
    const uint16_t* norm_w;
    float eps, inv_dim;
    const uint16_t* residual; /* row r at residual + r * res_stride; may alias job[0].y */
    long long res_stride;
    int pos0, nr, norm_regs;
    float* amax_val; /* [nr][grid] */
    int* amax_idx;
};
struct GemvRowsLaunch {
    GemvRowsArgs args;
    const kf_weight* w[3];
    int n, mode, n_rows;
};
GemvRowsProblem gemv_rows_problem(const GemvRowsLaunch& L, int canon);
// one launch per panel of p (p.shared); amax_* [n_rows][p.grid] when the mode is GEMV_ARGMAX.  KF_OK, p.status or KF_HIP_CHECK
int gemv_rows_launch(hipStream_t st, GemvRowsLaunch& L, const GemvRowsPlan& p);
void argmax_rows_finish_launch(hipStream_t st, const float* val, const int* idx, int n, int n_rows, int32_t* d_top1);

}  // namespace kf
