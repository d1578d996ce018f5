// kf_linear_bwd_plan.h -- how kf_linear_backward runs: kf::linear_bwd_plan, one pure host function, decides which shapes are served, where every region of the scratch
// lies, the plan of each wanted product and where the W operand comes from; kf_linear_bwd.hip and the entry in kf_abi.hip execute what it returns and decide nothing.
//   * served: linear_bwd_shape_ok -- the MFMA kernels contract over multiples of 64 and want 16-byte aligned rows: OC (the input gradient's contraction) a multiple of
//     64 and >= 128, IC a multiple of 8, and n (the weight gradient's contraction) a multiple of 64 and >= 128 only when gW is wanted.  AutoAWQ-layout weights are
//     inference-only.  A product no tile kernel covers is a refusal too, known before anything is launched: a refused call writes nothing.
//   * scratch: [W bf16 OC IC] [middle] [bias slabs fp64 ceil(n / 256) OC], each region 256-byte aligned.  The middle is lent to whichever route a product takes: the
//     transposed copies [W^T bf16 IC OC] [deltaIn^T bf16 OC n] [inp^T bf16 IC n] of GR_TRANSPOSE, or the partial-tile slots of the large tile kernel's split-K form
//     (gemm3_sk_ws_bytes) -- so it is the larger of the two, and the scratch does not depend on which outputs are wanted.
//   * products: gemm_plan (kf_gemm_plan.h gemm_plan_backward) for GE_BWD_DX / GE_BWD_DW with the middle lent as the split-K workspace.
//   * W: the input gradient reads the stored bf16 as it lies on the k-major route; a quantised weight is dequantised into the first region; the transpose route reads
//     that region, so a bf16 weight is copied into it first (dequant_launch of a bf16 weight is that copy).
#pragma once
#include "kf_gemm_plan.h"

namespace kf {

struct LinearBwdProblem {
    GemmMat w;                          /* the weight as it is stored: OC = w.M rows of IC = w.K */
    int n;                              /* token rows */
    int want_delta, want_gw, want_bias; /* the outputs the caller asks for */
};
enum LinearBwdRefusal { LBR_NONE = 0, LBR_AWQ, LBR_NOTHING, LBR_SHAPE, LBR_DX_UNCOVERED, LBR_DW_UNCOVERED }; /* the rule that refused, in the order they are tried */
enum { LBW_STORED = 0, LBW_DEQUANT, LBW_COPY }; /* W of the input gradient: the stored bf16 as it lies (also: no input gradient), the dequantised copy, the copy of a bf16 weight */
struct LinearBwdPlan {
    int status, refusal; /* KF_OK, or KF_INVALID_ARGS / KF_UNSUPPORTED_DATATYPE and the LinearBwdRefusal behind it */
    int w_from;          /* LBW_*: anything but LBW_STORED is one dequant_launch into the region at 0 */
    long long off_mid, off_dInT, off_inpT, off_slabs; /* W bf16 at 0; the middle: split-K slots, or W^T at off_mid, deltaIn^T, inp^T; the bias slabs */
    long long mid_bytes, bytes;                       /* the middle region; the whole scratch (0: OC, IC or n < 1) */
    GemmPlan dx, dw;     /* the wanted products (the others zeroed) */
};

// the shapes served (kf_gama_plan.h shares the OC rule)
inline bool linear_bwd_shape_ok(int OC, int IC, int n, bool want_gw) {
    return OC % 64 == 0 && OC >= 128 && IC % 8 == 0 && (!want_gw || (n % 64 == 0 && n >= 128));
}

inline LinearBwdPlan linear_bwd_plan(const LinearBwdProblem& P) {
    LinearBwdPlan p = {};
    const long long OC = P.w.M, IC = P.w.K, n = P.n;
    const auto refuse = [&p](int status, int rule) { return p.status = status, p.refusal = rule, p; };
    if (P.w.awq) return refuse(KF_UNSUPPORTED_DATATYPE, LBR_AWQ);
    if (OC < 1 || IC < 1 || n < 1) return refuse(KF_INVALID_ARGS, LBR_SHAPE);
    const long long w_bytes = up256(OC * IC * 2), copies = w_bytes + up256(OC * n * 2) + up256(IC * n * 2), slots = up256((long long)gemm3_sk_ws_bytes());
    p.off_mid = w_bytes, p.off_dInT = p.off_mid + w_bytes, p.off_inpT = p.off_dInT + up256(OC * n * 2);
    p.mid_bytes = copies > slots ? copies : slots;
    p.off_slabs = p.off_mid + p.mid_bytes;
    p.bytes = p.off_slabs + up256(cdiv(n, 256) * OC * 8);
    if (!P.want_delta && !P.want_gw && !P.want_bias) return refuse(KF_INVALID_ARGS, LBR_NOTHING);
    if (!linear_bwd_shape_ok(P.w.M, P.w.K, P.n, P.want_gw)) return refuse(KF_INVALID_ARGS, LBR_SHAPE);
    GemmProblem G = {};
    G.n_w = 1, G.w[0] = P.w, G.n = P.n, G.x_al = 1, G.scratch = p.mid_bytes;
    if (P.want_delta) {
        G.entry = GE_BWD_DX, p.dx = gemm_plan(G);
        if (p.dx.k.fam == GK_NONE) return refuse(KF_INVALID_ARGS, LBR_DX_UNCOVERED);
        p.w_from = P.w.type != KF_BF16 ? LBW_DEQUANT : (p.dx.route == GR_KMAJOR ? LBW_STORED : LBW_COPY);
    }
    if (P.want_gw) {
        G.entry = GE_BWD_DW, p.dw = gemm_plan(G);
        if (p.dw.k.fam == GK_NONE) return refuse(KF_INVALID_ARGS, LBR_DW_UNCOVERED);
    }
    return p;
}

// ---- the launcher (kf_linear_bwd.hip): executes a plan, nothing else, in the order bias column sums, dequantise, input gradient, weight gradient; KF_OK or the
// first launch's error.  NULL delta / gW / gBias: the outputs the plan's problem did not want
int linear_backward_launch(hipStream_t st, const LinearBwdPlan& p, const kf_weight* w, const uint16_t* deltaIn, const uint16_t* inp, uint16_t* delta, uint16_t* gW, uint16_t* gBias,
                           int n, int accumulate, void* scratch);

}  // namespace kf
