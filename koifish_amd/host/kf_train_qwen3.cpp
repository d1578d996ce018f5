// kf_train_qwen3.cpp -- ONE whole training step of the Qwen3 family (training form), sequenced in C++ behind the C ABI (part of libkf_host.so):
// koifish::GPT2Trainer's counterpart for the decoder everything else in this project serves.  The reference trains this family in its own goldens (cases/test_lite.py,
// cases/tutorial/tutorial_qwen3.md: Qwen3-596M, plain and 4-bit with "train_target": "gama"); the step is Fish::ForwardOnRLS / BackwardOnRLS / Optimizer::UpdateTensorParam
// as in kf_train.cpp, over the Qwen3 neurons.  The caller registers every trained tensor and every kept activation once; forward / backward / update are ABI calls only --
// no allocation, no host <-> device copy, no host sync.  The table of tensors, both registration forms, LinBack, the optimiser switch and the update loop (seed
// + 7919 t + index) are TrainerCore's (kf_train_common.hpp), shared with the GPT-2 trainer.
//
// Order of the registered tensors (kfh_qwen3t_set_param index):  per layer l, 11 in a row: q.w k.w v.w o.w gate.w up.w down.w n1 n2 qn kn;  then wte, nf, and head when
// the head is untied (Qwen3-8B and larger).  A tied head multiplies wte's blob and adds its gradient into wte's.
//
// Forward, per layer: RMSNorm (rstd kept) -> q, k, v products, each dense; q and k ARE the kept pre-norm copies -> the three blocks copied into the fused q | k | v rows
// (kf_d2d_rows: kf_attn_backward takes ONE row stride for q, k and v, and GQA makes the blocks differ in width) -> kf_qknorm_rope_train in place on the fused rows
// (rstd_q / rstd_k kept) -> kf_attn_prefill_batch_strided -> o_proj + residual -> RMSNorm -> gate, up -> kf_swiglu (gate and up kept) -> down + residual.  Then the final
// RMSNorm, the head product and kf_fused_classifier with dloss = 1 / N (kf_distill_classifier under kfh_qwen3t_set_distill; kfh_qwen3t_forward_logits stops after the
// head product: TrainerCore::SetDistill / ForwardLogits).  Under kfh_qwen3t_set_documents (supervised fine-tuning on packed documents) the q/k-norm + RoPE and the
// attention, forward and backward, are their _pos / _docs forms and the loss is the mean over the rows that count; every other operator is row-wise and unchanged.
// Backward, the reverse: every matrix through LinBack (a gama-registered one takes the gama branch); gate's and up's input gradients accumulate into one dh, q's, k's and
// v's into one dh (accumulate_delta); dq | dk | dv of kf_attn_backward go through ONE kf_qknorm_rope_backward (RoPE^T + q/k-norm backward + the dense copies); the
// embedding backward last, with no position table.
//
// Options: the optimiser switch of the GPT-2 trainer ("muon": a layer matrix with ne0 >= ne1 and a bf16 master through kf_muon -- q, k, v, gate, up at the 0.6B shape; o,
// down, norms, embeddings and every gama tensor on AdamW); "train_target": "gama" for any of the seven matrices (a context that holds a dequant arena is refused as soon
// as one is registered); a low-rank adapter beside any of the seven (kfh_qwen3t_set_param_lora: the base frozen, [a | b] one AdamW tensor, a dequant arena accepted).
// EOE layer-section branches are NOT offered on this trainer.
#include <cstring>
#include <string>

#include "kf_train_common.hpp"
#include "../../include/kf_host_abi.h"

namespace koifish {

static thread_local std::string g_q3t_err;  // why the last kfh_qwen3t_* call refused (kfh_qwen3t_last_error); a refusal of a kf_* entry underneath: kf_last_error

// what one layer keeps for its backward (nothing is recomputed)
struct Q3Acts {
    kf_bf16 *x, *h1, *qraw, *kraw, *qkv, *att, *x2, *h2, *gate, *up, *act;
    float *r1, *rq, *rk, *r2;
};

struct Qwen3Trainer : TrainerCore {
    int dim = 0, H = 0, KV = 0, hd = 0, ffn = 0, NL = 0, Cq = 0, Ck = 0, W = 0;
    bool tied = true;
    float eps = 1e-6f;
    std::vector<Q3Acts> acts;
    kf_bf16 *xf = nullptr, *dx = nullptr, *dqkv = nullptr, *datt = nullptr, *dact = nullptr, *dgate = nullptr, *vtmp = nullptr, *dqr = nullptr, *dkr = nullptr, *dvd = nullptr;
    float* rf = nullptr;
    const float* table = nullptr;  // kf_rope_table_host layout, T positions
    void *sc_ln = nullptr, *sc_at = nullptr, *sc_qk = nullptr;
    // packed documents (SetDocuments; the layout: include/kf_abi.h): the header of kf_attn_docs_plan's table (a copy), the table's device copy and the rows' positions
    kf_attn_docs_header doc_hdr = {};
    const void* doc_tab = nullptr;
    const int32_t* doc_pos = nullptr;

    enum { Q_W = 0, K_W, V_W, O_W, GATE_W, UP_W, DOWN_W, N1, N2, QN, KN, PER_LAYER };
    TrainTensor& P(int l, int k) { return params[(size_t)l * PER_LAYER + k]; }
    TrainTensor& Wte() { return params[(size_t)NL * PER_LAYER]; }
    TrainTensor& Nf() { return params[(size_t)NL * PER_LAYER + 1]; }
    TrainTensor& Head() { return params[(size_t)NL * PER_LAYER + (tied ? 0 : 2)]; }

    int Ready() const override {
        KF_TRY(ParamsReady());
        for (const Q3Acts& a : acts)
            if (!a.x || !a.h1 || !a.qraw || !a.kraw || !a.qkv || !a.att || !a.x2 || !a.h2 || !a.gate || !a.up || !a.act || !a.r1 || !a.rq || !a.rk || !a.r2) return KF_INVALID_ARGS;
        if (!xf || !hf || !logits || !dx || !dh || !dqkv || !datt || !dact || !dgate || !vtmp || !dqr || !dkr || !dvd || !rf || !losses || !table || !sc_lin || !sc_ln || !sc_at || !sc_qk)
            return KF_INVALID_ARGS;
        if (!params[(size_t)NL * PER_LAYER].has_blob || (!tied && !params[(size_t)NL * PER_LAYER + 2].has_blob)) return KF_INVALID_ARGS;
        return KF_OK;
    }
    // d_table == NULL: back to B sequences of T rows, the plain step bit for bit with no extra launch.  Otherwise Forward / Backward call kf_attn_prefill_docs,
    // kf_attn_backward_docs and the _pos forms of the q/k-norm + RoPE entries, and the loss is the mean over the n_valid rows whose mask word lacks 0x10000.
    // h_header: the head of the host table (copied); d_table, d_pos [N], d_mask [N]: device memory the caller keeps alive.  A refusal changes nothing.
    int SetDocuments(const kf_attn_docs_header* h_header, const void* d_table, const int32_t* d_pos, const int32_t* d_mask, int n_valid_, std::string* why) {
        auto refuse = [why](const char* msg) {
            if (why) *why = msg;
            return (int)KF_INVALID_ARGS;
        };
        if (!d_table) {
            doc_tab = nullptr, doc_pos = nullptr, loss_mask = nullptr, n_valid = 0, doc_hdr = kf_attn_docs_header{};
            return KF_OK;
        }
        if (teacher) return refuse("set_documents: a teacher is set (set_distill): its forward would need the same layout -- switch distillation off first");
        if (!h_header || !d_pos || !d_mask) return refuse("set_documents: the header, the positions and the mask words must not be NULL");
        if (((uintptr_t)d_table & 15) || ((uintptr_t)d_pos & 3) || ((uintptr_t)d_mask & 3)) return refuse("set_documents: the table must be 16-byte aligned, positions and mask words 4-byte aligned");
        if (h_header->magic != KF_ATTN_DOCS_MAGIC || h_header->n_rows != N || h_header->n_head != H || h_header->n_kv != KV || h_header->head_dim != hd || h_header->max_len > T)
            return refuse("set_documents: the table was not planned (kf_attn_docs_plan) for this trainer's rows, heads and rope table");
        if (n_valid_ < 1 || n_valid_ > h_header->doc_rows) return refuse("set_documents: n_valid must be between 1 and the number of document rows");
        doc_hdr = *h_header, doc_tab = d_table, doc_pos = d_pos, loss_mask = d_mask, n_valid = n_valid_;
        return KF_OK;
    }
    int Lin(TrainTensor& w, const kf_bf16* x, kf_bf16* y, const kf_bf16* res) { return LinForw(w, x, y, res); }  // an adapted matrix: + kf_lora_forward on the same y
    int Rms(const kf_bf16* x, TrainTensor& w, kf_bf16* y, float* rstd) { return kf_rmsnorm(ctx, x, w.p, y, N, dim, eps, rstd); }
    // kf_norm_backward ADDS into dweight: the per-tensor gradients are zero here (kf_adamw zeroes what it consumed)
    int RmsBack(kf_bf16* dxx, const kf_bf16* dout, const kf_bf16* inp, TrainTensor& w, const float* rstd) {
        return kf_norm_backward(ctx, dxx, w.g, nullptr, dout, inp, w.p, nullptr, rstd, N, dim, sc_ln);
    }

    TrainTensor& HeadTensor() override { return Head(); }
    // the embedding, the layers and the final RMSNorm: hf.  TrainerCore::Forward and ForwardLogits go on from there
    int Trunk(const int32_t* d_ids) override {
        KF_TRY(kf_embed_batch(ctx, &Wte().blob, d_ids, N, acts[0].x));
        for (int l = 0; l < NL; l++) {
            Q3Acts& a = acts[l];
            KF_TRY(Rms(a.x, P(l, N1), a.h1, a.r1));
            KF_TRY(Lin(P(l, Q_W), a.h1, a.qraw, nullptr));
            KF_TRY(Lin(P(l, K_W), a.h1, a.kraw, nullptr));
            KF_TRY(Lin(P(l, V_W), a.h1, vtmp, nullptr));
            KF_TRY(kf_d2d_rows(ctx, a.qkv, (size_t)W * 2, a.qraw, (size_t)Cq * 2, (size_t)Cq * 2, (size_t)N)); /* q | k | v: column blocks of the fused rows */
            KF_TRY(kf_d2d_rows(ctx, a.qkv + Cq, (size_t)W * 2, a.kraw, (size_t)Ck * 2, (size_t)Ck * 2, (size_t)N));
            KF_TRY(kf_d2d_rows(ctx, a.qkv + Cq + Ck, (size_t)W * 2, vtmp, (size_t)Ck * 2, (size_t)Ck * 2, (size_t)N));
            if (doc_tab) { /* packed documents: a row's position and the rows it attends to are data */
                KF_TRY(kf_qknorm_rope_train_pos(ctx, a.qkv, a.qkv + Cq, P(l, QN).p, P(l, KN).p, table, N, doc_pos, W, W, H, KV, hd, eps, a.rq, a.rk));
                KF_TRY(kf_attn_prefill_docs(ctx, a.qkv, a.qkv + Cq, a.qkv + Cq + Ck, a.att, &doc_hdr, doc_tab, W, Cq, H, KV, hd, W));
            } else {
                KF_TRY(kf_qknorm_rope_train(ctx, a.qkv, a.qkv + Cq, P(l, QN).p, P(l, KN).p, table, N, T, W, W, H, KV, hd, eps, a.rq, a.rk));
                KF_TRY(kf_attn_prefill_batch_strided(ctx, a.qkv, a.qkv + Cq, a.qkv + Cq + Ck, a.att, T, W, Cq, H, KV, hd, W, B));
            }
            KF_TRY(Lin(P(l, O_W), a.att, a.x2, a.x));
            KF_TRY(Rms(a.x2, P(l, N2), a.h2, a.r2));
            KF_TRY(Lin(P(l, GATE_W), a.h2, a.gate, nullptr));
            KF_TRY(Lin(P(l, UP_W), a.h2, a.up, nullptr));
            KF_TRY(kf_swiglu(ctx, a.gate, a.up, a.act, N * ffn));
            KF_TRY(Lin(P(l, DOWN_W), a.act, l + 1 < NL ? acts[l + 1].x : xf, a.x2));
        }
        return Rms(xf, Nf(), hf, rf);
    }
    int Backward() override {
        KF_TRY(Ready());
        KF_TRY(HeadBack(Head()));
        KF_TRY(kf_memset(ctx, dx, 0, (size_t)N * dim * 2));
        KF_TRY(RmsBack(dx, dh, xf, Nf(), rf));
        for (int l = NL - 1; l >= 0; l--) {
            Q3Acts& a = acts[l];
            KF_TRY(LinBack(P(l, DOWN_W), dx, a.act, dact, nullptr));
            KF_TRY(kf_swiglu_backward(ctx, dact, dgate, a.gate, a.up, (size_t)N * ffn)); /* dact becomes d(up) */
            KF_TRY(LinBack(P(l, UP_W), dact, a.h2, dh, nullptr));
            KF_TRY(LinBack(P(l, GATE_W), dgate, a.h2, dh, nullptr, 1));
            KF_TRY(RmsBack(dx, dh, a.x2, P(l, N2), a.r2));
            KF_TRY(LinBack(P(l, O_W), dx, a.att, datt, nullptr));
            if (doc_tab) { /* sc_at: kf_attn_backward_docs_scratch_bytes(N, H) = kf_attn_backward_scratch_bytes(T, H, B) */
                KF_TRY(kf_attn_backward_docs(ctx, a.qkv, a.qkv + Cq, a.qkv + Cq + Ck, W, a.att, datt, Cq, dqkv, dqkv + Cq, dqkv + Cq + Ck, W, &doc_hdr, doc_tab, H, KV, hd, sc_at));
                KF_TRY(kf_qknorm_rope_backward_pos(ctx, dqkv, dqkv + Cq, dqkv + Cq + Ck, W, a.qraw, Cq, a.kraw, Ck, P(l, QN).p, P(l, KN).p, a.rq, a.rk, table, N, doc_pos, H, KV, hd,
                                                   dqr, dkr, dvd, P(l, QN).g, P(l, KN).g, sc_qk));
            } else {
                KF_TRY(kf_attn_backward(ctx, a.qkv, a.qkv + Cq, a.qkv + Cq + Ck, W, a.att, datt, Cq, dqkv, dqkv + Cq, dqkv + Cq + Ck, W, T, H, KV, hd, B, sc_at));
                KF_TRY(kf_qknorm_rope_backward(ctx, dqkv, dqkv + Cq, dqkv + Cq + Ck, W, a.qraw, Cq, a.kraw, Ck, P(l, QN).p, P(l, KN).p, a.rq, a.rk, table, N, T, H, KV, hd, dqr,
                                               dkr, dvd, P(l, QN).g, P(l, KN).g, sc_qk));
            }
            KF_TRY(LinBack(P(l, Q_W), dqr, a.h1, dh, nullptr));
            KF_TRY(LinBack(P(l, K_W), dkr, a.h1, dh, nullptr, 1));
            KF_TRY(LinBack(P(l, V_W), dvd, a.h1, dh, nullptr, 1));
            KF_TRY(RmsBack(dx, dh, a.x, P(l, N1), a.r1));
        }
        return kf_embed_backward(ctx, Wte().g, dim, nullptr, dx, ids, B, T, dim, Vp);
    }
};

}  // namespace koifish

using koifish::Core;
using koifish::Qwen3Trainer;
static Qwen3Trainer* Q3(void* h) { return static_cast<Qwen3Trainer*>(Core(h)); }  // for the entries only this family has

extern "C" {
// V: the vocabulary; Vp >= V its padded row count (a multiple of 64 for kf_linear_backward); B sequences of T tokens per step; tied != 0: the head is wte
void* kfh_qwen3t_create(kf_ctx* ctx, int dim, int n_layer, int n_head, int n_kv, int head_dim, int ffn, int V, int Vp, int B, int T, float rms_eps, int tied) {
    koifish::g_q3t_err.clear();
    if (!ctx || dim < 8 || (dim % 8) || n_layer < 1 || n_head < 1 || n_kv < 1 || n_head % n_kv || (head_dim != 64 && head_dim != 128) || ffn < 8 || (ffn % 8) || V < 1 || Vp < V || B < 1 ||
        T < 1 || (long long)B * T * (ffn > dim ? ffn : dim) > 0x7FFFFFFFLL) {
        koifish::g_q3t_err = "kfh_qwen3t_create: needs a context, dim and ffn multiples of 8, n_head a multiple of n_kv, head_dim 64 or 128, Vp >= V >= 1, B, T >= 1 and B * T * max(dim, ffn) below 2^31";
        return nullptr;
    }
    Qwen3Trainer* g = new Qwen3Trainer;
    g->ctx = ctx, g->dim = dim, g->NL = n_layer, g->H = n_head, g->KV = n_kv, g->hd = head_dim, g->ffn = ffn, g->V = V, g->Vp = Vp, g->B = B, g->T = T, g->N = B * T;
    g->Cq = n_head * head_dim, g->Ck = n_kv * head_dim, g->W = g->Cq + 2 * g->Ck, g->eps = rms_eps, g->tied = tied != 0;
    g->params.resize((size_t)n_layer * Qwen3Trainer::PER_LAYER + (tied ? 2 : 3));
    g->wmat.assign(g->params.size(), 0);
    for (int l = 0; l < n_layer; l++)
        for (int k = Qwen3Trainer::Q_W; k <= Qwen3Trainer::DOWN_W; k++) g->wmat[(size_t)l * Qwen3Trainer::PER_LAYER + k] = 1;
    g->acts.resize(n_layer);
    memset(g->acts.data(), 0, sizeof(koifish::Q3Acts) * n_layer);
    return static_cast<koifish::TrainerCore*>(g);
}
void kfh_qwen3t_destroy(void* h) { delete Core(h); }
int kfh_qwen3t_n_params(void* h) { return (int)Core(h)->params.size(); }
// as kfh_gpt2_set_param
int kfh_qwen3t_set_param(void* h, int index, void* p, void* g, void* m, void* v, long long n, int decay, const kf_weight* blob, int requant) {
    return Core(h)->SetParam(index, p, g, m, v, n, decay, blob, requant);
}
// "train_target": "gama" for one of a layer's seven matrices, with the refusals of kfh_gpt2_set_param_gama; a context that holds a dequant arena is refused here already
int kfh_qwen3t_set_param_gama(void* h, int index, void* g, void* m, void* v, const kf_weight* blob) {
    Qwen3Trainer* t = Q3(h);
    koifish::g_q3t_err.clear();
    if (kf_dequant_arena_bytes(t->ctx) > 0) {
        koifish::g_q3t_err = "kfh_qwen3t_set_param_gama: the context holds a dequant arena (kf_set_dequant_arena): its resident bf16 copies of a gama-trained matrix would go stale "
                             "with every update -- switch the arena off (kf_set_dequant_arena(ctx, NULL, 0)) for training";
        return KF_INVALID_ARGS;
    }
    const int rc = t->SetParamGama(index, g, m, v, blob);
    if (rc != KF_OK) koifish::g_q3t_err = "kfh_qwen3t_set_param_gama: index " + std::to_string(index) + " is no layer matrix, a null pointer, or a blob that is no KF_Q4 / KF_T_SIGN / KF_BOOL1 group storage";
    return rc;
}
int kfh_qwen3t_set_gama_scratch(void* h, void* scratch, size_t bytes) { return Core(h)->SetGamaScratch(scratch, bytes); }
// a low-rank adapter beside one of a layer's seven matrices (TrainerCore::SetParamLora): p / g / m / v are [a (rank x IC) | b (OC x rank)] bf16 each, ax [B T, rank] bf16
int kfh_qwen3t_set_param_lora(void* h, int index, void* p, void* g, void* m, void* v, int rank, float s, void* ax, const kf_weight* blob) {
    koifish::g_q3t_err.clear();
    const int rc = Core(h)->SetParamLora(index, p, g, m, v, rank, s, ax, blob);
    if (rc != KF_OK)
        koifish::g_q3t_err = "kfh_qwen3t_set_param_lora: index " + std::to_string(index) + " is no layer matrix, a null pointer, a rank other than 16 / 32 / 64, or a matrix whose sides "
                             "are not multiples of 64 and >= 128";
    return rc;
}
int kfh_qwen3t_set_lora_scratch(void* h, void* scratch, size_t bytes) {
    koifish::g_q3t_err.clear();
    const int rc = Core(h)->SetLoraScratch(scratch, bytes);
    if (rc != KF_OK) koifish::g_q3t_err = "kfh_qwen3t_set_lora_scratch: the scratch is missing or not 256-byte aligned";
    return rc;
}
// ptrs: x h1 r1 qraw kraw qkv rq rk att x2 h2 r2 gate up act
int kfh_qwen3t_set_layer_acts(void* h, int layer, void* const* ptrs) {
    Qwen3Trainer* t = Q3(h);
    if (layer < 0 || layer >= t->NL || !ptrs) return KF_INVALID_ARGS;
    koifish::Q3Acts& a = t->acts[layer];
    a.x = (kf_bf16*)ptrs[0], a.h1 = (kf_bf16*)ptrs[1], a.r1 = (float*)ptrs[2], a.qraw = (kf_bf16*)ptrs[3], a.kraw = (kf_bf16*)ptrs[4], a.qkv = (kf_bf16*)ptrs[5];
    a.rq = (float*)ptrs[6], a.rk = (float*)ptrs[7], a.att = (kf_bf16*)ptrs[8], a.x2 = (kf_bf16*)ptrs[9], a.h2 = (kf_bf16*)ptrs[10], a.r2 = (float*)ptrs[11];
    a.gate = (kf_bf16*)ptrs[12], a.up = (kf_bf16*)ptrs[13], a.act = (kf_bf16*)ptrs[14];
    return KF_OK;
}
// ptrs: xf hf rf logits losses dx dh dqkv datt dact dgate vtmp dq_raw dk_raw dv_dense rope_table scratch_linear_backward scratch_norm_backward scratch_attn_backward
// scratch_qknorm_rope_backward
int kfh_qwen3t_set_buffers(void* h, void* const* ptrs) {
    Qwen3Trainer* t = Q3(h);
    if (!ptrs) return KF_INVALID_ARGS;
    t->xf = (kf_bf16*)ptrs[0], t->hf = (kf_bf16*)ptrs[1], t->rf = (float*)ptrs[2], t->logits = (kf_bf16*)ptrs[3], t->losses = (float*)ptrs[4];
    t->dx = (kf_bf16*)ptrs[5], t->dh = (kf_bf16*)ptrs[6], t->dqkv = (kf_bf16*)ptrs[7], t->datt = (kf_bf16*)ptrs[8], t->dact = (kf_bf16*)ptrs[9], t->dgate = (kf_bf16*)ptrs[10];
    t->vtmp = (kf_bf16*)ptrs[11], t->dqr = (kf_bf16*)ptrs[12], t->dkr = (kf_bf16*)ptrs[13], t->dvd = (kf_bf16*)ptrs[14], t->table = (const float*)ptrs[15];
    t->sc_lin = ptrs[16], t->sc_ln = ptrs[17], t->sc_at = ptrs[18], t->sc_qk = ptrs[19];
    return KF_OK;
}
int kfh_qwen3t_forward(void* h, const int32_t* d_ids, const int32_t* d_tgt) { return Core(h)->Forward(d_ids, d_tgt); }
int kfh_qwen3t_backward(void* h) { return Core(h)->Backward(); }
int kfh_qwen3t_update(void* h, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
    return Core(h)->Update(lr, beta1, beta2, eps, wd, seed);
}
int kfh_qwen3t_step(void* h, const int32_t* d_ids, const int32_t* d_tgt, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
    return Core(h)->Step(d_ids, d_tgt, lr, beta1, beta2, eps, wd, seed);
}
// as kfh_gpt2_set_optimizer
int kfh_qwen3t_set_optimizer(void* h, int method, float lr_scale, float mui, float eps_muon, int tp_decay, void* scratch, size_t scratch_bytes) {
    return Core(h)->SetOptimizer(method, lr_scale, mui, eps_muon, tp_decay, scratch, scratch_bytes);
}
long long kfh_qwen3t_steps_taken(void* h) { return Core(h)->t; }
// gradient norms and clipping: TrainerCore::SetGradClip / GradClipScratchBytes / GradNorms (kf_train_common.hpp)
KFH_GRAD_CLIP_ENTRIES(qwen3t, koifish::g_q3t_err)
// distillation against a teacher's logits: TrainerCore::SetDistill / ForwardLogits
KFH_DISTILL_ENTRIES(qwen3t, koifish::g_q3t_err)
// packed documents: Qwen3Trainer::SetDocuments (d_table NULL: off).  The GPT-2 trainer has no such entry: its positions are learned
int kfh_qwen3t_set_documents(void* h, const void* h_header, const void* d_table, const int32_t* d_pos, const int32_t* d_mask, int n_valid) {
    koifish::g_q3t_err.clear();
    return Q3(h)->SetDocuments((const kf_attn_docs_header*)h_header, d_table, d_pos, d_mask, n_valid, &koifish::g_q3t_err);
}
const char* kfh_qwen3t_last_error(void) { return koifish::g_q3t_err.c_str(); }
}
