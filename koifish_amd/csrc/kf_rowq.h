// kf_rowq.h -- how the 3- / 2-bit row forms are planned when they unpack in registers (kf_set_row_unpack): no rule of their own.  A weight is planned AS THE 4-BIT
// ROW CODEBOOK OF THE SAME M x K -- kf::gemv_plan, kf::gemm_plan and kf::tile_plan see the stand-in built here and answer as they always did -- and the entry swaps
// FMT_Q4R for the weight's real format when it launches: same lanes per row, same slots, same tiles, so every sum is formed in the order of the 4-bit twin (the
// same ids as nibbles, a 16-entry table whose first entries are the row's own).
#pragma once
#include "kf_gemm_plan.h"

namespace kf {

constexpr int ROWQ_K_UNIT = 128; /* the shape rule of the in-register routes: K a multiple of 128 (four units: every row starts 16-byte aligned, a staged k tile is whole) */

// FMT_Q3R / FMT_Q2R / FMT_Q2N of a stored weight, -1: not a 3- / 2-bit row form
inline int rowq_fmt(const kf_weight* w) {
    if (!w) return -1;
    if (w->quant == KF_QUANT_ROW_LUT && w->type == KF_Q3) return FMT_Q3R;
    if (w->quant == KF_QUANT_ROW_LUT && w->type == KF_Q2) return FMT_Q2R;
    if (w->quant == KF_QUANT_ROW_RTN && w->type == KF_Q2) return FMT_Q2N;
    return -1;
}
// The stand-in of w in *m and its real format in *fmt.  Its alignment bits carry the shape rule: GM_DATA_AL when K is a multiple of 128 (and the data 16-byte
// aligned), GM_TAB_AL when the row tables start aligned to their own size (16 / 8 / 4 bytes) -- so a plan function refuses what cannot run in registers with the
// code it has for a misaligned row codebook.  KF_OK: both bits set; KF_BLAS_UNALIGN: one is missing (kf_linear keeps the dequantise route, the fused entries
// refuse); KF_UNSUPPORTED_DATATYPE: not a 3- / 2-bit row form, or the AutoAWQ layout.
inline int rowq_standin(const kf_weight* w, GemmMat* m, int* fmt) {
    const int f = rowq_fmt(w);
    if (fmt) *fmt = f;
    if (f < 0 || w->qzeros || w->qscales) return KF_UNSUPPORTED_DATATYPE;
    const uintptr_t tab = (uintptr_t)(w->gama + w->ne0 + w->ne1);
    const bool data_al = w->ne1 >= ROWQ_K_UNIT && w->ne1 % ROWQ_K_UNIT == 0 && ((uintptr_t)w->data & 15) == 0;
    const bool tab_al = w->gama && (tab & (uintptr_t)(rowq_tab_elems(f) * 2 - 1)) == 0;
    *m = GemmMat{KF_Q4, KF_QUANT_ROW_LUT, 0, w->ne0, w->ne1, w->lGroup, w->gama != nullptr, (data_al ? GM_DATA_AL : 0) | (tab_al ? GM_TAB_AL : 0)};
    return data_al && tab_al ? KF_OK : KF_BLAS_UNALIGN;
}
// the matrices of one launch (they share x): all of ONE row form -> their stand-ins in m[] and the format returned; otherwise -1 and m[] untouched.  strict: every
// stand-in must be runnable (kf_linear's choice between the routes); otherwise a stand-in with a missing bit goes to the plan, which refuses it (the fused entries).
inline int rowq_standins(int n, const kf_weight* const* w, GemmMat* m, bool strict) {
    GemmMat t[3];
    int fmt = -1;
    for (int i = 0; i < n && i < 3; i++) {
        int f;
        const int rc = rowq_standin(w[i], &t[i], &f);
        if (rc == KF_UNSUPPORTED_DATATYPE || (i && f != fmt) || (strict && rc != KF_OK)) return -1;
        fmt = f;
    }
    for (int i = 0; i < n && i < 3; i++) m[i] = t[i];
    return fmt;
}
// a plan's kernel with the stand-in's format swapped for the real one
inline GemmKern rowq_kern(GemmKern k, int fmt) {
    if (fmt >= 0 && k.fmt == FMT_Q4R) k.fmt = fmt;
    return k;
}

}  // namespace kf
