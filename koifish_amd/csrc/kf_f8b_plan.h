// kf_f8b_plan.h -- the e4m3 block-scaled storage (include/kf_abi.h "FP8 block-scaled layers"): its shape rule and the launch plans of kf_f8b.hip, stated once.
// Plain C++: no HIP, no device code.  A weight is KF_F8E4M3 bytes [ne0, ne1] row-major with one fp32 scale per 128 x 128 block, qscales [ceil(ne0 / 128)][ne1 / 128].
#pragma once
#include "../../include/kf_abi.h"

namespace kf {

constexpr int F8B_BLOCK = 128;    /* rows and columns of a scale block */
constexpr int F8B_ROW_ALIGN = 16; /* ne0: an MFMA fragment of 16 rows never straddles a scale row */
constexpr int F8B_TILE_MIN = 8;   /* kf_linear: token rows from which the MFMA tiles take over from the mat-vec per row */
constexpr int F8B_CUS = 256;      /* MI355X */
inline const char* f8b_shape_rule() { return "the e4m3 block-scaled storage needs in % 128 == 0 and out % 16 == 0 (whole 128-wide k-blocks, 16-row fragments inside one scale row)"; }
inline bool f8b_shape_ok(long long ne0, long long ne1) { return ne0 > 0 && ne1 > 0 && ne1 % F8B_BLOCK == 0 && ne0 % F8B_ROW_ALIGN == 0; }
inline long long f8b_scale_rows(long long ne0) { return (ne0 + F8B_BLOCK - 1) / F8B_BLOCK; }
inline long long f8b_scale_count(long long ne0, long long ne1) { return f8b_scale_rows(ne0) * (ne1 / F8B_BLOCK); }

// the storage form of a kf_weight: KF_OK, or the refusal (KF_QUANT_ERR: not this form's fields; KF_BLAS_UNALIGN: the shape rule or an unaligned pointer)
inline int f8b_check(const kf_weight* w, const char** why) {
    *why = "";
    if (w->qzeros) return *why = "KF_F8E4M3 with qzeros: qzeros and qscales together are the AutoAWQ layout, which is KF_Q4", KF_QUANT_ERR;
    if (!w->qscales) return *why = "KF_F8E4M3 without qscales: the storage has one fp32 scale per 128 x 128 block", KF_QUANT_ERR;
    if (w->quant != KF_QUANT_GROUP || w->lGroup != F8B_BLOCK || w->gama) return *why = "KF_F8E4M3 is served with quant = KF_QUANT_GROUP, lGroup = 128 and no gama", KF_QUANT_ERR;
    if (!f8b_shape_ok(w->ne0, w->ne1)) return *why = f8b_shape_rule(), KF_BLAS_UNALIGN;
    if (((uintptr_t)w->data & 15) || ((uintptr_t)w->qscales & 3)) return *why = "KF_F8E4M3: data not 16-byte or qscales not 4-byte aligned", KF_BLAS_UNALIGN;
    return KF_OK;
}

// ---- one token: waves own output rows.  A wave keeps `rows` consecutive rows (1, 2 or 4: they share x reads and the scale line) for the whole of K; a workgroup of four
// waves stages x as fp32 in panels of F8B_PANEL elements.  `rows` is the largest that still leaves two workgroups per CU; short K (few pieces per wave) gains nothing
// from more rows and keeps one.  The summation order of a row does not depend on any of this (include/kf_abi.h).
constexpr int F8B_PANEL = 8192, F8B_WAVES = 4;
struct F8bVecPlan {
    int rows, groups, grid; /* rows per wave; row groups over all matrices of the launch; workgroups */
};
inline F8bVecPlan f8b_vec_plan(const int* M, int n_mat, int K, bool paired) {
    long long total = 0;
    for (int i = 0; i < (paired ? 1 : n_mat); i++) total += M[i];
    int rows = 1;
    if (K >= 1024)
        for (int r = paired ? 2 : 4; r > 1; r >>= 1)
            if (total / (r * F8B_WAVES) >= 2 * F8B_CUS) { rows = r; break; }
    F8bVecPlan p;
    p.rows = rows, p.groups = 0;
    for (int i = 0; i < (paired ? 1 : n_mat); i++) p.groups += M[i] / rows; /* M % 16 == 0 */
    p.grid = (p.groups + F8B_WAVES - 1) / F8B_WAVES;
    return p;
}

// ---- token batches: a workgroup of 2 x 2 waves owns [32 tm rows of W] x [32 tn tokens]; a wave tm x tn accumulator tiles of 16 x 16.  The largest form that still
// fills the CUs, else the smallest: few tokens are bound by the stream of W and want workgroups over `out`.
struct F8bTilePlan {
    int tm, tn, gx, gy;
};
inline F8bTilePlan f8b_tile_plan(int M, int n) {
    static const int forms[3][2] = {{4, 4}, {2, 2}, {1, 1}};
    F8bTilePlan p = {1, 1, 0, 0};
    for (int f = 0; f < 3; f++) {
        const int bm = 32 * forms[f][0], bn = 32 * forms[f][1];
        p.tm = forms[f][0], p.tn = forms[f][1], p.gx = (M + bm - 1) / bm, p.gy = (n + bn - 1) / bn;
        if ((long long)p.gx * p.gy >= F8B_CUS && n > bn / 2) break;
    }
    return p;
}

}  // namespace kf
