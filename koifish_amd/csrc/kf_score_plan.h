// kf_score_plan.h -- how kf_head_logprob scores a batch of rows against an LM head: kf::score_plan, one pure host function, picks the route, the tile form, the grid,
// the LDS and the scratch; kf_head_score.hip and the entry in kf_abi.hip execute what it returns and decide nothing.
//   SR_FUSED   the hot path: a bf16 head, dim a multiple of the tile's k step.  The kf_gemm3.hip tiles over [vocabulary x rows] with the log-softmax in the epilogue --
//              no logit is stored.  A workgroup leaves one 16-byte partial {max, sum exp, first-max index, target logit} per row and vocabulary tile, a second launch
//              merges a row's partials in a fixed order.  Scratch: rows x 128-row vocabulary tiles x 16 bytes = 1/16 of the bf16 logit matrix (the 256-row tile uses half of it).
//   SR_PANEL   everything else (quantised heads, AutoAWQ, row forms, odd dims): kf_linear into the lent scratch, panel by panel, and a row-reduce launch per panel.
//              The panels are cut along the ROWS (SCORE_PANEL_ROWS of them x the whole vocabulary): a quantised head's group / row tables are indexed over the whole
//              matrix, a slice of its vocabulary has no kf_weight of its own.  Scratch: min(rows, SCORE_PANEL_ROWS) x vocabulary x 2 bytes.
// Both routes round a logit to bf16 as kf_linear / kf_lm_head store it and use the fixed kf_expf / kf_logf; they differ in the fp32 order of the dot products only.
#pragma once
#include "kf_gemm_plan.h"

namespace kf {

enum ScoreRoute { SR_FUSED = 0, SR_PANEL = 1 };
constexpr int SCORE_BIG_MIN_ROWS = 512; /* the fused route's 256 x 256 tile from this many rows */
constexpr int SCORE_PANEL_ROWS = 128;   /* rows of logits the panel route holds at a time */
constexpr int SCORE_PARTIAL_BYTES = 16; /* {float max, float sum, int32 index, float target logit} */
constexpr int SCORE_MERGE_ROWS = 4;     /* rows per 256-thread workgroup of the merge and the row-reduce launches: one wave each */

struct ScoreProblem {
    GemmMat w;   /* the head: M = vocabulary, K = dim */
    int n;       /* rows */
    int x_al;    /* x 16-byte aligned and its row stride a multiple of 8 elements */
    int force;   /* test hook (kfdbg_set_knob "score_route"): 0 the rule, 1 the panel route */
    int form;    /* test hook ("score_form"): < 0 the rule, else G3_BIG / G3_SMALL on the fused route */
};
struct ScorePlan {
    int route;              /* ScoreRoute */
    int status;             /* KF_OK or KF_INVALID_ARGS (no rows, no vocabulary) -- never "unsupported" */
    int form;               /* SR_FUSED: G3_SMALL / G3_BIG */
    int n_vt, n_rb;         /* SR_FUSED: vocabulary tiles (= partials per row), row blocks */
    int gx, block, lds;     /* SR_FUSED: the tile launch */
    int panel_rows;         /* SR_PANEL: rows per kf_linear call */
    long long scratch;      /* bytes kf_head_logprob needs lent */
};

// the fused route's shape: what kf_gemm3.hip's k-contiguous tiles need of both operands
inline bool score_fused_shape(const ScoreProblem& P) {
    const GemmMat& m = P.w;
    return m.type == KF_BF16 && !m.awq && m.quant == KF_QUANT_GROUP && m.K >= G3_BK && m.K % G3_BK == 0 && (m.al & GM_DATA_AL) && P.x_al;
}
inline ScorePlan score_plan(const ScoreProblem& P) {
    ScorePlan p = {};
    if (P.n < 1 || P.w.M < 1 || P.w.K < 1) {
        p.route = SR_PANEL, p.status = KF_INVALID_ARGS;
        return p;
    }
    if (!P.force && score_fused_shape(P)) {
        // 256 x 256 tiles from SCORE_BIG_MIN_ROWS rows, 128 x 128 below (measured on the 151 936 x 1024 head, scratch/ub_score.py: 128 rows 108 us on the small tile
        // against 151 on the big one -- one ragged row block of 256 is half empty --, 512 rows 274 against 238, 2047 rows 984 against 862)
        const int f = P.form >= 0 ? (P.form == G3_BIG ? G3_BIG : G3_SMALL) : (P.n >= SCORE_BIG_MIN_ROWS ? G3_BIG : G3_SMALL);
        const G3Form& c = G3_FORMS[f];
        p.route = SR_FUSED, p.form = f;
        p.n_vt = (int)cdiv(P.w.M, c.bm), p.n_rb = (int)cdiv(P.n, c.bn);
        p.gx = p.n_vt * p.n_rb, p.block = c.nth, p.lds = c.lds;
        // sized for the 128-row tile whatever the form: the answer then grows with the rows, and a caller that sized its scratch for its largest batch
        // (Fish::ScoreReady) has enough for every smaller one, on either tile
        p.scratch = up256((long long)P.n * cdiv(P.w.M, G3_FORMS[G3_SMALL].bm) * SCORE_PARTIAL_BYTES);
        return p;
    }
    p.route = SR_PANEL;
    p.panel_rows = P.n < SCORE_PANEL_ROWS ? P.n : SCORE_PANEL_ROWS;
    p.scratch = up256((long long)p.panel_rows * P.w.M * 2);
    return p;
}

// ---- the launchers (kf_head_score.hip): each executes a plan, nothing else; KF_OK or KF_HIP_CHECK
// SR_FUSED: W [V][K] bf16, x [n][ldx] bf16; partials [n][n_vt] into scratch, then the merge: logprob / lse / top1 [n] (lse, top1 may be NULL)
int score_fused_launch(hipStream_t st, const ScorePlan& p, const uint16_t* W, int V, int K, const uint16_t* x, long long ldx, int n, const int32_t* targets, float* logprob,
                       float* lse, int32_t* top1, void* scratch);
// SR_PANEL: one panel of materialised bf16 logits [n][ldl] (V columns used) folded into logprob / lse / top1 [n]
int score_rows_launch(hipStream_t st, const uint16_t* logits, long long ldl, int V, int n, const int32_t* targets, float* logprob, float* lse, int32_t* top1);

}  // namespace kf
