// kf_kernels.h -- internal launch interfaces between the ABI layer (kf_abi.hip) and the kernel files.
#pragma once
#include "../../include/kf_abi.h"
#include "kf_device.h"

namespace kf {

enum {
    FMT_BF16 = 0, FMT_F8 = 1, FMT_Q4 = 2, FMT_Q2 = 3, FMT_Q1 = 4,
    FMT_Q4P = 5, /* 4-bit through the register-table lookup (mat-vec only) */
    FMT_Q4R = 6, /* 4-bit row codebook (KF_QUANT_ROW_LUT): byte-packed nibbles + 16 bf16 table entries per row */
    FMT_Q1T = 7, /* 1-bit through an LDS table of v_perm selectors (mat-vec only; bit-identical to FMT_Q1) */
    FMT_Q2T = 8, /* 2-bit, the same way (bit-identical to FMT_Q2) */
    // 3- / 2-bit row forms unpacked in registers (kf_set_row_unpack; units of 32 weights, include/kf_abi.h): never named by a plan -- an entry plans the weight as the
    // 4-bit row codebook of its shape (kf_rowq.h) and launches the FMT_Q4R form's kernel in one of these
    FMT_Q3R = 9,  /* 8-entry row codebook (KF_Q3 + KF_QUANT_ROW_LUT): 12 bytes per unit */
    FMT_Q2R = 10, /* 4-entry row codebook (KF_Q2 + KF_QUANT_ROW_LUT): 8 bytes per unit */
    FMT_Q2N = 11  /* 2-bit row RTN (KF_Q2 + KF_QUANT_ROW_RTN): the row's (zero, step) becomes a 4-entry table when it is loaded */
};
constexpr bool fmt_rowq(int fmt) { return fmt >= FMT_Q3R && fmt <= FMT_Q2N; }
constexpr int rowq_unit_bytes(int fmt) { return fmt == FMT_Q3R ? 12 : 8; }                     /* a unit of 32 weights in the stream */
constexpr int rowq_tab_elems(int fmt) { return fmt == FMT_Q3R ? 8 : (fmt == FMT_Q2R ? 4 : 2); } /* bf16 elements of a row's table */
inline bool is_row_lut(const kf_weight* w) { return w->quant != KF_QUANT_GROUP; } /* any row-wise card (kf_lut.hip); the mat-vec kernel takes Q4 + ROW_LUT, and the 3- / 2-bit forms behind kf_set_row_unpack */
enum { GEMV_PLAIN = 0, GEMV_PAIRED = 1, GEMV_ARGMAX = 2 };
constexpr int KF_MAX_ARGMAX_PARTIALS = 4096;
constexpr int KF_ATTN_MAX_SPLITS = 32;

struct GemvJob {
    const void* w;
    const uint16_t* zero;
    const uint16_t* step;
    uint16_t* y;
    long long y_pos_stride; /* elements added per position (KV-cache row aliasing), 0 otherwise */
    int M;
    int qBias;
    int slot0;
};

// a weight as the launch plans see it (kf_gemm_plan.h, kf_gemv_plan.h)
enum { GM_DATA_AL = 1, GM_TAB_AL = 2 };
struct GemmMat {
    int type, quant, awq; /* kf_weight type and quant form; AutoAWQ layout (qzeros / qscales) */
    int M, K;             /* ne0, ne1 */
    int lgroup, gama;     /* group size; gama present */
    int al;               /* GM_DATA_AL: data 16-byte aligned; GM_TAB_AL: the row tables (gama + ne0 + ne1) 16-byte aligned */
};
inline GemmMat mat_of(const kf_weight* w) {
    const bool tab_al = w->gama && ((uintptr_t)(w->gama + w->ne0 + w->ne1) & 15) == 0;
    return GemmMat{w->type, w->quant, w->qzeros || w->qscales, w->ne0, w->ne1, w->lGroup, w->gama != nullptr, (((uintptr_t)w->data & 15) == 0 ? GM_DATA_AL : 0) | (tab_al ? GM_TAB_AL : 0)};
}

struct TpPushDev { /* one per (rank, exchange index), written once by kf_tp_commit */
    unsigned long long* peer[8]; /* this rank's slot of the exchange's buffer in every rank's receive area */
    const unsigned* step;        /* device word: generation */
    unsigned per_step, index;
    int world, pad_;
};
struct GemvArgs {
    GemvJob job[3];
    int njobs;
    int K, nBlk, lpr_log2, iters, lGroup, gshift;
    int spw, total_slots;
    const uint16_t* x;
    const uint16_t* norm_w; /* non-NULL: RMSNorm prologue */
    float eps, inv_dim;
    const uint16_t* residual;
    const uint16_t* bias;
    float* yf; /* non-NULL: write fp32 row dots here instead of bf16 outputs (single job) */
    float alpha, beta;
    const int* d_pos;
    int pos;
    float* amax_val;
    int* amax_idx;
    // tensor-parallel push (kf_linear_f32_push): the un-rounded fp32 row dot goes, tagged, into this rank's slot of every rank's receive area.  ONE pointer to a
    // descriptor in device memory: kernel arguments are fetched before a launch's first load, and the 96 bytes of the descriptor inside this struct cost every
    // mat-vec launch of the decode step 0.37 us (measured: 0.742 -> 0.782 ms per step on the per-layer path).
    const struct TpPushDev* tp; /* NULL: no push */
    int stream_ok;          /* long dense launches: buffer-load form allowed (offsets < 2^31, groups inside rows) */
    const int32_t* row_map; /* non-NULL: the sparse forward -- slot rows index this list of hot rows (job.M = their number); weights and outputs use row_map[row] */
};

// tensor-parallel exchange (kf_tp.hip)
int tp_reduce_recv_launch(hipStream_t st, const unsigned long long* slots, int R, int n_max, int n, const unsigned* d_step, unsigned per_step, unsigned index,
                          const uint16_t* residual, uint16_t* out, int* d_err);
int tp_argmax_push_launch(hipStream_t st, const float* val, const int* idx, int n, int row0, unsigned long long* const* peers, int R, const unsigned* d_step,
                          unsigned per_step, unsigned index);
int tp_pick_launch(hipStream_t st, const unsigned long long* pairs, int R, unsigned* d_step, unsigned per_step, unsigned index, int32_t* d_state, int32_t* d_tokens_out,
                   int* d_err, int vocab);
void argmax_finish_launch(hipStream_t st, const float* val, const int* idx, int n, int32_t* d_argmax, int32_t* d_state, int32_t* d_tokens_out);

// ---- token-batch GEMM on MFMA: kf_gemm_plan.h (the rule and the launchers)

// ---- attention (kf_attn.hip)
struct AttnArgs {
    const uint16_t* q;     /* raw or prepared q [n_head*hd] */
    const uint16_t* k_raw; /* NULL: keys come from the cache only */
    uint16_t* kcache;
    const uint16_t* vcache;
    const uint16_t* wq_norm;
    const uint16_t* wk_norm;
    const float* rope_table; /* NULL: q is already normed+roped */
    float* part;             /* [n_head][n_splits][hd + 2] fp64 partials {O, L, m} (kf_attn.hip reads it as doubles) */
    int* counters;           /* [n_kv] arrival counters, zero between launches */
    uint16_t* out;
    const int* d_pos;
    int pos;
    int n_head, n_kv, hd, kv_stride, n_splits, chunk, cnt_stride;
    float eps, inv_sqrt_hd_den;
    int n_tok;          /* token batch (prefill): position pos + token */
    int one_slice;      /* every (kv-head, token) is handled by one workgroup: no scratch, no hand-off */
    long long q_stride; /* elements between the q (and out) rows of consecutive tokens */
    int canon;          /* the canonical softmax (fp64 sums, exact rescales; bit-exact against the oracle's CANON mode) instead of the fp32 form */
    int gq_split;       /* the query heads of a kv-head are dealt to this many workgroups (blockIdx.y = kv-head * gq_split + part), each with GQ / gq_split heads
                           (kf_attn_plan.h ATTN_CANON_GQ_WG) */
};
// the attention launchers: kf_attn_plan.h (the rule and the launchers)
int qknorm_rope_launch(hipStream_t st, uint16_t* q, uint16_t* k, const uint16_t* wq, const uint16_t* wk, const float* table, int pos,
                       const int* d_pos, int n_head, int n_kv, int hd, float eps, int n_tok = 1, long long q_stride = 0, long long k_stride = 0, int seq_len = 0,
                       float* rstd_q = nullptr, float* rstd_k = nullptr);
int qknorm_rope_pos_launch(hipStream_t st, uint16_t* q, uint16_t* k, const uint16_t* wq, const uint16_t* wk, const float* table, const int* row_pos, int n_head, int n_kv, int hd,
                           float eps, int n_tok, long long q_stride, long long k_stride, float* rstd_q, float* rstd_k); /* token t at position row_pos[t] */

// Development knobs (process-wide, default = the product's choice).  Not part of the ABI and never read from the environment: tests and the scripts under
// scratch/ set them through kfdbg_set_knob (kf_abi.hip) to compare a kernel form with the form it replaces inside one process.
struct Knobs {
    int q4_perm = 1;      /* 4-bit mat-vec through the register-table lookup (0: the arithmetic form; same bits) */
    int q2_tab = 1;       /* 2-bit mat-vec through the LDS selector table (0: the arithmetic form; same bits) */
    int q1_tab = 1;       /* 1-bit mat-vec through the LDS selector table (0: the per-bit select form; same bits) */
    int gemv_xf2 = 1;     /* canonical 4-bit rows too long for fp32 activations in 48 KiB of LDS: two windows of half the block columns (0: bf16 activations, widened per product) */
    int score_route = 0;  /* kf_head_logprob: 1 sends a head the fused route would take down the panel route (kf_score_plan.h; the two are compared by tests/test_gpu_score.py) */
    int score_form = -1;  /* kf_head_logprob's fused route: >= 0 the tile form (G3_BIG / G3_SMALL) instead of the rule's (scratch/ub_score.py measures both) */
};
extern Knobs g_knobs;
// ---- the decode engines.  Two families, two kernels, each with its own host side below; the host rules both state -- served descriptors, heads and embedding tables, the
// layer table, the error word, the per-device LDS ceiling -- are kf_engine_host.h
enum { ENG_BUILD = 0, ENG_DRY = 1, ENG_DRY_NO_DEVICE = 2 }; /* engine_build / xengine_build: create; validate only; validate without asking the device for its CUs */
// ---- the persistent decode engine: one sequence on every CU (kf_engine.hip)
struct EngineHost;
struct CPlan { /* one mat-vec phase of an engine, a compile-time figure of its model shape (kf_engine_common.h c_plan, PlanT) */
    int K, nBlk, lpr_log2, iters, njobs, M[3], slot0[3], total, spg;
};
// one form the engine can launch (an engine_kernel<EngCfg<...>> instantiation, built from its EngCfg by eng_form): what it serves, its phase plans, its LDS, its launcher
struct EngForm {
    int shape_class, fmt;
    bool canon, dbg;             /* the canonical order; the per-phase stamps */
    CPlan plan[4];               /* q | k | v, o_proj, gate | up, down_proj */
    size_t (*smem)(int n_layer); /* dynamic LDS of a launch */
    int (*go)(EngineHost* E, hipStream_t st);
};
// THE choice of form, at create and when the order or the stamps change (no HIP call): nullptr = refused (no form for this shape and storage, or its LDS does not fit)
const EngForm* engine_form(int shape_class, int fmt, bool canon, bool stamps, int n_layer);
size_t engine_ws_bytes(const kf_engine_desc* d);
int engine_build(const kf_engine_desc* d, void* ws, size_t ws_bytes, hipStream_t st, EngineHost** out, const char** why, int mode = ENG_BUILD);
int engine_tune(EngineHost* E, hipStream_t st, uint16_t* x_out, const int32_t* d_state, int pos_bound, int passes, float* us_before, float* us_after);
int engine_stats(EngineHost* E, hipStream_t st, int pos_bound, int* out14);
int engine_step(EngineHost* E, hipStream_t st, const uint16_t* x_in, uint16_t* x_out, const int32_t* d_state, int pos_bound, int with_head = 0, int n_steps = 1); /* 1: not served */
int engine_set_head(EngineHost* E, const kf_weight* w, const uint16_t* norm_w, uint16_t* logits, int32_t* d_tokens_out);
int engine_set_embedding(EngineHost* E, const kf_weight* w, const int32_t* d_forced);
// the int8 screen of the in-launch head (kf_head_screen.hip): size of the caller's buffer, the build (one launch), the setter (buf == NULL: off; builds the copy from the head
// that is set) and the counters since create / reset: {screened steps, rows re-ranked, workgroup fall-backs}
size_t head_screen_bytes(int vocab, int dim);
int head_screen_build(const uint16_t* head, int vocab, int dim, void* buf, size_t bytes, hipStream_t st);
int engine_set_head_screen(EngineHost* E, void* buf, size_t bytes, hipStream_t st);
int engine_screen_stats(EngineHost* E, hipStream_t st, long long* out3);
int engine_error_word(EngineHost* E, hipStream_t st, int* h_err);
void engine_set_canonical(EngineHost* E, int on); /* every phase: canonical order (1, the default) or the v_dot2c / fp32 forms */
int engine_reset(EngineHost* E, hipStream_t st); /* after a timed-out poll: exchange state re-initialised, error word cleared */
void engine_free(EngineHost* E);
int engine_debug_read(EngineHost* E, unsigned long long* h_out, int n_words);
int engine_debug_enable(EngineHost* E, int wg);       /* per-phase stamps of workgroup wg from the next launch on (the diagnostic instantiation of the kernel) */
void engine_set_delays(EngineHost* E, const int* d6); /* tuning runs */

// ---- XCD-confined decode engines: up to eight independent sequences per launch, one per XCD (kf_xengine.hip)
struct XEngineHost;
// one form an engine can launch (an xengine_kernel<XCfg<...>> instantiation, built from its XCfg by xe_form): what it serves, its shape, its LDS, its launcher
struct XForm {
    int shape_class, fmt;
    int nwv, depth, wpc, nb;     /* waves per workgroup, ring depth, decoders per XCD, sequences per decoder */
    bool dbg;                    /* the per-phase stamps */
    size_t (*smem)(int n_layer); /* dynamic LDS of one workgroup at launch */
    int (*go)(XEngineHost* E, hipStream_t st);
};
// THE choice of form, at create and at every launch (no HIP call): nullptr = refused (no form for this shape, storage and count, or none fits the LDS at this depth)
const XForm* xengine_form(int shape_class, int fmt, int n_seq, int n_layer, bool stamps, bool two_wpc);
size_t xengine_ws_bytes(const kf_engine_desc* d);
int xengine_build(const kf_engine_desc* d, int n_seq, long long kv_seq_stride, void* ws, size_t ws_bytes, hipStream_t st, XEngineHost** out, const char** why, int mode = ENG_BUILD);
int xengine_steps(XEngineHost* E, hipStream_t st, int32_t* d_state, uint16_t* x_out, int with_head, int n_steps);
size_t xengine_ws_bytes_tp(const kf_engine_desc* rank0);                                /* tensor parallel over the XCDs: one sequence, rank r on XCD r */
int xengine_build_tp(const kf_engine_desc* const* ranks, int world, void* ws, size_t ws_bytes, hipStream_t st, XEngineHost** out, const char** why);
int xengine_set_head_tp(XEngineHost* E, const kf_weight* const* shards, const int* row0, const uint16_t* norm_w, uint16_t* logits, int32_t* d_tokens_out, int tokens_stride);
int xengine_set_embedding(XEngineHost* E, const kf_weight* w, const int32_t* d_forced, int forced_stride);
int xengine_set_head(XEngineHost* E, const kf_weight* w, const uint16_t* norm_w, uint16_t* logits, int32_t* d_tokens_out, int tokens_stride);
int xengine_error_word(XEngineHost* E, hipStream_t st, int* h_err);
int xengine_reset(XEngineHost* E, hipStream_t st);
void xengine_free(XEngineHost* E);
int xengine_set_variant(XEngineHost* E, int nwv, int depth);              /* A/B hook: nwv -2 = two decoders per XCD for 9 .. 16 sequences (depth != 0); else -1 */
int xengine_debug_enable(XEngineHost* E, int seq, int wg, int max_steps); /* per-phase stamps of one workgroup of one decoder (seq < 0: off) */
int xengine_debug_read(XEngineHost* E, unsigned long long* h_out, int n_words);

// ---- small ops (kf_ops.hip)
int rmsnorm_launch(hipStream_t st, const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int dim, float eps, float* rstd);
int layernorm_launch(hipStream_t st, const uint16_t* x, const uint16_t* w, const uint16_t* b, uint16_t* y, int rows, int dim, float eps, float* mean, float* rstd);
int gelu_launch(hipStream_t st, const uint16_t* x, uint16_t* y, size_t n);
int rope_backward_launch(hipStream_t st, uint16_t* d, const float* table, int pos0, int n_tok, int seq_len, long long stride, int n_head, int hd);
int gelu_backward_launch(hipStream_t st, uint16_t* d_in_out, const uint16_t* x, size_t n);
int swiglu_backward_launch(hipStream_t st, uint16_t* delta_in_out, uint16_t* delta_gate, const uint16_t* gate, const uint16_t* up, size_t n);
// LayerNorm / RMSNorm backward (kf_norm_bwd.hip); scratch: norm_backward_groups(rows) * (mean ? 2 : 1) * C doubles
int norm_backward_groups(int rows);
int norm_backward_launch(hipStream_t st, uint16_t* dinp, uint16_t* dweight, uint16_t* dbias, const uint16_t* dout, const uint16_t* inp, const uint16_t* weight,
                         const float* mean, const float* rstd, int rows, int C, double* scratch);
int norm_backward_reduce_launch(hipStream_t st, uint16_t* dweight, const double* part, int G, int C); /* dweight[c] = bf16(sum_g part[g][c] + dweight[c]) */
// q/k-norm + RoPE backward in one pass (kf_qknorm_rope_bwd.hip); scratch: qknorm_rope_backward_scratch_bytes (0: a shape the launch refuses)
size_t qknorm_rope_backward_scratch_bytes(int n_tok, int n_head, int n_kv, int hd);
int qknorm_rope_backward_launch(hipStream_t st, const uint16_t* dq, const uint16_t* dk, const uint16_t* dv, long long ld_d, const uint16_t* q_raw, long long ld_qraw,
                                const uint16_t* k_raw, long long ld_kraw, const uint16_t* wq, const uint16_t* wk, const float* rstd_q, const float* rstd_k, const float* table,
                                int n_tok, int seq_len, int n_head, int n_kv, int hd, uint16_t* dq_raw, uint16_t* dk_raw, uint16_t* dv_out, uint16_t* dwq, uint16_t* dwk,
                                double* scratch, const int* pos = nullptr);
int bias_residual_launch(hipStream_t st, uint16_t* y, const uint16_t* bias, const uint16_t* residual, size_t n, int M); /* kf_ops.hip */
// linear backward helpers (kf_linear_bwd.hip)
int transpose_bf16_launch(hipStream_t st, const uint16_t* in, uint16_t* out, int R, int C);
int colsum_add_launch(hipStream_t st, const uint16_t* x, uint16_t* dst, int n, int C, double* scratch); /* scratch: ceil(n / 256) * C doubles */
// embedding backward (kf_embed_bwd.hip)
int argmax_rows_state_launch(hipStream_t st, const uint16_t* logits, long long ld, int n, int n_rows, const int* d_seq, int32_t* states, int32_t* tokens_out, int tokens_stride);
int copy_blocks_launch(hipStream_t st, void* const* dst_table, size_t dst_offset, const void* src, size_t src_stride, size_t block_bytes, int n_blocks);
int embed_pos_launch(hipStream_t st, const uint16_t* wte, long long ldw, const uint16_t* wpe, const int* tokens, int B, int T, int C, int V, uint16_t* out);
int embed_backward_launch(hipStream_t st, uint16_t* dwte, long long ldw, uint16_t* dwpe, const uint16_t* dout, const int* tokens, int B, int T, int C, int V);
// fused classifier (kf_loss.hip): cross-entropy loss per row + logit gradient in place
int fused_classifier_launch(hipStream_t st, uint16_t* logits, float* losses, uint16_t* probs, float dloss, const int* targets, long rows, int V, int P,
                            const int* mask, int write_dlogits);
int zero_ignored_rows_launch(hipStream_t st, uint16_t* buf, long rows, int P, const int* mask); /* zeros to the rows the classifier skipped, and to no other */
// distilling classifier (kf_distill.hip): a CE + b tau^2 KL(teacher || student) per row + its logit gradient in place; kd_weight == 0: no teacher is read
int distill_classifier_launch(hipStream_t st, uint16_t* logits, const uint16_t* teacher, long teacher_ld, float* losses, float* kd, float dloss, const int* targets,
                              long rows, int V, int P, const int* mask, float ce_weight, float kd_weight, float temperature, int write_dlogits);
int swiglu_launch(hipStream_t st, const uint16_t* gate, const uint16_t* up, uint16_t* out, int n);
int add_launch(hipStream_t st, const uint16_t* a, const uint16_t* b, uint16_t* out, int n);
int embed_launch(hipStream_t st, const kf_weight* w, int token, const int32_t* d_token, const int32_t* d_state, const int32_t* d_forced,
                 uint16_t* out, int n_tok = 1);
int dequant_launch(hipStream_t st, const kf_weight* w, uint16_t* out, int ilv_n = 1, int ilv_i = 0); /* ilv_n > 1: rows interleaved with ilv_n - 1 other matrices in blocks of 16 (kf_ops.hip) */
int adamw_launch(hipStream_t st, uint16_t* params, uint16_t* grads, void* gm, void* gv, size_t n, int mv_bf16, float lr, float beta1, float beta2, float b1c,
                 float b2c, float eps, float wd, float grad_scale, unsigned int seed, int* status, const float* d_grad_scale = nullptr); /* d_grad_scale != NULL: *d_grad_scale replaces grad_scale */
// ---- Muon (kf_muon.hip): PIPE_Muon::CU_core.  One scratch per tensor shape: A, B [ne1][ne1] bf16, two X buffers [ne0][ne1] bf16, one fp64 partial per 4096 elements, two doubles
struct MuonLayout {
    size_t A, B, X0, X1, part, dbl, bytes; /* byte offsets, each a multiple of 256 */
};
constexpr int KF_MUON_MAX_PARTIALS = 1 << 16; /* the context's own partial sums for kf_muon_momentum / kf_muon_apply: n <= 2^28 elements */
MuonLayout muon_layout(int ne0, int ne1);
int muon_momentum_launch(hipStream_t st, uint16_t* mG, const uint16_t* grads, uint16_t* X, size_t n, float mui, unsigned int seed, double* partials, double* d_sumsq);
int muon_apply_launch(hipStream_t st, uint16_t* params, uint16_t* grads, const uint16_t* X, size_t n, float lr, float wd, unsigned int seed, double* partials, double* d_wnormsq);
int newton_schulz_launch(hipStream_t st, uint16_t* X, int ne0, int ne1, const double* d_sumsq, float eps, int n_iter, float a, float b, float c, void* scratch);
// ---- EOE (kf_evo.hip): Fuyou::Exploitation over one follower matrix (thr: the crossover threshold out of 256, beta = 1 - alpha), and the ensemble mean of losses
int evolve_launch(hipStream_t st, uint16_t* x, const uint16_t* head, size_t n, int algorithm, float alpha, float beta, float social, unsigned int thr, unsigned int seed);
int loss_mean_launch(hipStream_t st, float* acc, const float* losses, size_t n, int index, int count);
int sample_launch(hipStream_t st, const uint16_t* logits, int n, int top_k, float temperature, float top_p, unsigned long long* rng, int32_t* d_token,
                  int32_t* d_state, int32_t* d_tokens_out, const int32_t* d_forced, int n_forced, int true_topk = 0);
int quantize_launch(hipStream_t st, const kf_weight* w, const uint16_t* src, int symmetric);
// row-codebook 4-bit storage (kf_lut.hip): NF4 quantiser, dequant, embedding rows
int lut_quantize_launch(hipStream_t st, const kf_weight* w, const uint16_t* src);
int lut_dequant_launch(hipStream_t st, const kf_weight* w, uint16_t* out);
int lut_embed_launch(hipStream_t st, const kf_weight* w, int token, const int32_t* d_token, const int32_t* d_state, const int32_t* d_forced, uint16_t* out, int n_tok);
// ---- AutoAWQ layout (kf_awq.hip)
size_t awq_scratch_bytes(const kf_weight* w);
int awq_linear_launch(hipStream_t st, const kf_weight* w, const uint16_t* x, uint16_t* y, const uint16_t* bias, float alpha, float beta,
                      const uint16_t* residual, float* scratch);
int awq_dequant_launch(hipStream_t st, const kf_weight* w, uint16_t* out);

int set_state_launch(hipStream_t st, int32_t* d_state, int token, int pos);
int hot_rows_launch(hipStream_t st, const int32_t* hot, int n, int32_t* rows, int32_t* count);
int cold_fill_launch(hipStream_t st, uint16_t* y, const uint16_t* bias, int n);
int cold_cols_launch(hipStream_t st, uint16_t* y, const int32_t* hot, int rows, int cols);
int tp_reduce_launch(hipStream_t st, const float* partials, int R, int n, const uint16_t* residual, uint16_t* out);

}  // namespace kf
