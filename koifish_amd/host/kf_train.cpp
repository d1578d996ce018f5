// kf_train.cpp -- ONE whole training step of the hybrid-precision GPT-2 of BASELINE config 3, sequenced in C++ behind the C ABI (part of libkf_host.so).
//
// The reference's step ("training"):  Fish::Train -> Optimizer loop -> Fish::ForwardOnRLS (gLLM.cpp:722-787: the neurons in graph order) ->
// BackwardOnRLS (gLLM.cpp:656-686: the reverse walk, SLP::Back NeuronFuse.cu:495-563) -> Optimizer::UpdateTensorParam -> CU_adamw_ (Optimizer.cu:135-160) ->
// the re-quantisation of every updated matrix (CU_XtoQ128_ / Float2T<f8e5>, T.cu:105-175).  Here the same order as three straight loops over a TABLE of device
// pointers: the caller (Python owns the buffers: koifish_amd/train_step.py; a C++ host would kf_malloc them) registers every trained tensor {master, gradient, two
// moments, optional quantised blob} and every kept activation once; a step is then ABI calls only -- no allocation, no host <-> device copy, no host sync.
//
// Order of the registered tensors (kfh_gpt2_set_param index):  per block l, 12 in a row: qkv.w qkv.b proj.w proj.b fc.w fc.b proj2.w proj2.b ln1.w ln1.b ln2.w
// ln2.b;  then wte, wpe, lnf.w, lnf.b.   The AdamW seed of tensor i at optimizer step t is seed + 7919 t + i (one seed per launch, as the reference draws one per
// tensor update).
//
// What is trained of a quantised matrix is a choice per tensor.  kfh_gpt2_set_param registers the SHADOW-WEIGHT form: a bf16 master, its [OC, IC] gradient and moments, the
// blob re-quantised after every update.  kfh_gpt2_set_param_gama registers the reference's "train_target": "gama" (SLP::Back with w->gama_param, NeuronFuse.cu:538-549;
// GTensor::InitGamaParam, GTensor.cpp:903-945; PIPE_Adamw on the slice, Optimizer.cu:646-662): the packed integers stay frozen, the parameter is the blob's own
// [ZERO nGroup][STEP nGroup] slice, its gradient and moments are 2 nGroup long, LinBack is kf_linear_backward(gW = NULL) + kf_gama_backward(scale 1: the chain rule's value,
// not the reference's 1 / nSample), the update is the same kf_adamw launch on the slice -- no weight decay (a decayed step shrinks every weight of its group), no
// re-quantisation, never Muon.  Resident dequantised copies (kf_set_dequant_arena) would go stale with every update: a trainer with a gama tensor refuses a context that has an arena.
//
// The optimiser is a switch (kfh_gpt2_set_optimizer): AdamW on everything (the default), or the reference's default "muon" (OPT_Muon, Optimizer.cpp:1014-1056;
// PIPE_Muon::Update, Pipe.cpp:16-57): MUON_params_::isAdamW restated -- a block's weight matrix with ne0 >= ne1 goes through kf_muon, everything else keeps kf_adamw.
//
// EOE, "Evolutionary Optimization of Experts" (kfh_gpt2_set_branches / _set_active_branch / _evolve / _eval): the NL layers are cut into NL / layers_in_branch sections
// (RLSchedule::InitBranch / UpdateBackbone, Scheduler.cpp:522-656); a section together with the shared embedding, final norm and head is a shallow model of its own, a
// "Fuyou".  Forward / Backward / Update walk the ACTIVE section only: the 0 .. NL loops are l0 .. l1, the embedding writes acts[l0].x, Update leaves every tensor of
// another section alone (no momentum, no weight decay; its seed index is skipped, not renumbered).  Evolve is Fuyou::UpdateFollower over the swarm
// (ExploreOptimization, Scheduler.cpp:430-486): the head branch pulls the four weight matrices (isWMAT) of every layer of every other branch towards its own with
// kf_evolve, and every follower blob is re-quantised.  Eval is the evaluation half of Fish::ForwardOnRLS (gLLM.cpp:722-787): one branch, or the mean over all of
// them.  Which branch trains when, and which one is the head, is the caller's loop.  One branch (the default) is the code above, bit for bit.
//
// Distillation from a teacher's logits (kfh_gpt2_set_distill / _forward_logits) is TrainerCore's (SetDistill, ForwardLogits): with a teacher set the forward ends in
// kf_distill_classifier.  It and the layer sections exclude each other: Eval shares the one `losses` buffer with the step.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "kf_train_common.hpp"
#include "../../include/kf_host_abi.h"

namespace koifish {

static thread_local std::string g_train_err;  // why the last kfh_gpt2_evolve / _set_branches / _set_active_branch / _eval refused (kfh_gpt2_last_error)

// the activations one block keeps for its backward (nothing is recomputed)
struct BlockActs {
    kf_bf16 *x, *h1, *qkv, *att, *x2, *h2, *f, *g;
    float *m1, *r1, *m2, *r2;
};

// TrainTensor, the registration, LinBack, the optimiser switch, Update, Step and the head's forward / backward are TrainerCore's (kf_train_common.hpp), shared with
// koifish::Qwen3Trainer
struct GPT2Trainer : TrainerCore {
    int C = 0, H = 0, NL = 0, hd = 0;
    std::vector<BlockActs> acts;
    kf_bf16 *xf = nullptr, *dx = nullptr, *dqkv = nullptr, *datt = nullptr, *d4 = nullptr;
    float *mf = nullptr, *rf = nullptr;
    void *sc_ln = nullptr, *sc_at = nullptr;
    // EOE: sections of LIS layers; branch b owns layers [b LIS, (b + 1) LIS); [l0, l1) is the active one.  One branch (LIS = NL): the whole depth
    int LIS = 0, branch = 0, l0 = 0, l1 = 0;
    enum { ENSEMBLE_AGGREGATION = 0, ENSEMBLE_BRANCH = 1 };  // Fuyou_params::ENSEMBLE: AGGREGATION; FUYOU_BEST and RANDOM_1 are BRANCH with the caller's choice of branch
    int NBranch() const { return NL / LIS; }
    bool InSection(size_t i) const override { return i >= (size_t)NL * PER_BLOCK || ((int)(i / PER_BLOCK) >= l0 && (int)(i / PER_BLOCK) < l1); }

    enum { QKV_W = 0, QKV_B, PROJ_W, PROJ_B, FC_W, FC_B, PROJ2_W, PROJ2_B, LN1_W, LN1_B, LN2_W, LN2_B, PER_BLOCK };
    TrainTensor& P(int l, int k) { return params[(size_t)l * PER_BLOCK + k]; }
    TrainTensor& Wte() { return params[(size_t)NL * PER_BLOCK]; }
    TrainTensor& Wpe() { return params[(size_t)NL * PER_BLOCK + 1]; }
    TrainTensor& LnfW() { return params[(size_t)NL * PER_BLOCK + 2]; }
    TrainTensor& LnfB() { return params[(size_t)NL * PER_BLOCK + 3]; }

    int Ready() const override {
        KF_TRY(ParamsReady());
        for (const BlockActs& a : acts)
            if (!a.x || !a.h1 || !a.qkv || !a.att || !a.x2 || !a.h2 || !a.f || !a.g || !a.m1 || !a.r1 || !a.m2 || !a.r2) return KF_INVALID_ARGS;
        if (!xf || !hf || !logits || !dx || !dh || !dqkv || !datt || !d4 || !mf || !rf || !losses || !sc_lin || !sc_ln || !sc_at) return KF_INVALID_ARGS;
        return params[(size_t)NL * PER_BLOCK].has_blob ? KF_OK : KF_INVALID_ARGS;
    }
    // SLP::Forw (NeuronFuse.cu:305-381): y = x . W^T + b (+ residual)
    int Lin(TrainTensor& w, const kf_bf16* x, kf_bf16* y, TrainTensor* bias, const kf_bf16* res) {
        return kf_linear(ctx, &w.blob, x, y, bias ? bias->p : nullptr, N, 1.0f, 0.0f, res ? 1u : 0u, res);
    }
    int LN(const kf_bf16* x, TrainTensor& w, TrainTensor& b, kf_bf16* y, float* mean, float* rstd) { return kf_layernorm(ctx, x, w.p, b.p, y, N, C, 1e-5f, mean, rstd); }
    // kf_norm_backward ADDS into dweight / dbias: the per-tensor gradients are zero here (kf_adamw zeroes what it consumed)
    int LNBack(kf_bf16* dxx, const kf_bf16* dout, const kf_bf16* inp, TrainTensor& w, TrainTensor& b, const float* mean, const float* rstd) {
        return kf_norm_backward(ctx, dxx, w.g, b.g, dout, inp, w.p, mean, rstd, N, C, sc_ln);
    }

    // TokenEmbed, NL x [LayerNorm, qkv, causal attention, proj + residual, LayerNorm, fc, GELU, proj2 + residual], LayerNorm, tied head, fused classifier:
    // (TrainerCore::Forward: per-row losses in `losses`, the logit gradients of the MEAN loss in `logits`).  Trunk: up to hf, the final LayerNorm's output
    TrainTensor& HeadTensor() override { return Wte(); }
    bool Sectioned() const override { return LIS != NL; }
    int Trunk(const int32_t* d_ids) override {
        KF_TRY(kf_embed_pos(ctx, Wte().p, C, Wpe().p, d_ids, B, T, C, Vp, acts[l0].x));
        for (int l = l0; l < l1; l++) {
            BlockActs& a = acts[l];
            KF_TRY(LN(a.x, P(l, LN1_W), P(l, LN1_B), a.h1, a.m1, a.r1));
            KF_TRY(Lin(P(l, QKV_W), a.h1, a.qkv, &P(l, QKV_B), nullptr));
            KF_TRY(kf_attn_prefill_batch_strided(ctx, a.qkv, a.qkv + C, a.qkv + 2 * C, a.att, T, 3 * (int64_t)C, C, H, H, hd, 3 * C, B)); /* q / k / v: column blocks of the fused rows */
            KF_TRY(Lin(P(l, PROJ_W), a.att, a.x2, &P(l, PROJ_B), a.x));
            KF_TRY(LN(a.x2, P(l, LN2_W), P(l, LN2_B), a.h2, a.m2, a.r2));
            KF_TRY(Lin(P(l, FC_W), a.h2, a.f, &P(l, FC_B), nullptr));
            KF_TRY(kf_gelu(ctx, a.f, a.g, (size_t)N * 4 * C));
            KF_TRY(Lin(P(l, PROJ2_W), a.g, l + 1 < l1 ? acts[l + 1].x : xf, &P(l, PROJ2_B), a.x2));
        }
        return LN(xf, LnfW(), LnfB(), hf, mf, rf);
    }
    int Backward() override {
        KF_TRY(Ready());
        KF_TRY(HeadBack(Wte()));
        KF_TRY(kf_memset(ctx, dx, 0, (size_t)N * C * 2));
        KF_TRY(LNBack(dx, dh, xf, LnfW(), LnfB(), mf, rf));
        for (int l = l1 - 1; l >= l0; l--) {
            BlockActs& a = acts[l];
            KF_TRY(LinBack(P(l, PROJ2_W), dx, a.g, d4, &P(l, PROJ2_B)));
            KF_TRY(kf_gelu_backward(ctx, d4, a.f, (size_t)N * 4 * C));
            KF_TRY(LinBack(P(l, FC_W), d4, a.h2, dh, &P(l, FC_B)));
            KF_TRY(LNBack(dx, dh, a.x2, P(l, LN2_W), P(l, LN2_B), a.m2, a.r2));
            KF_TRY(LinBack(P(l, PROJ_W), dx, a.att, datt, &P(l, PROJ_B)));
            KF_TRY(kf_attn_backward(ctx, a.qkv, a.qkv + C, a.qkv + 2 * C, 3 * (long long)C, a.att, datt, C, dqkv, dqkv + C, dqkv + 2 * C, 3 * (long long)C, T, H, H, hd, B, sc_at));
            KF_TRY(LinBack(P(l, QKV_W), dqkv, a.h1, dh, &P(l, QKV_B)));
            KF_TRY(LNBack(dx, dh, a.x, P(l, LN1_W), P(l, LN1_B), a.m1, a.r1));
        }
        return kf_embed_backward(ctx, Wte().g, C, Wpe().g, dx, ids, B, T, C, Vp);
    }
    int SetBranches(int layers_in_branch) {
        if (layers_in_branch == 0) layers_in_branch = NL;
        if (layers_in_branch < 0 || layers_in_branch > NL || NL % layers_in_branch) {
            g_train_err = "kfh_gpt2_set_branches: " + std::to_string(NL) + " layers do not divide into sections of " + std::to_string(layers_in_branch);
            return KF_INVALID_ARGS;
        }
        if (teacher && layers_in_branch != NL) {
            g_train_err = "kfh_gpt2_set_branches: the trainer distils from a teacher (set_distill), which layer sections do not offer -- switch distillation off first";
            return KF_INVALID_ARGS;
        }
        LIS = layers_in_branch;
        return SetActive(0);
    }
    int SetActive(int b) {
        if (b < 0 || b >= NBranch()) {
            g_train_err = "kfh_gpt2_set_active_branch: branch " + std::to_string(b) + " of " + std::to_string(NBranch());
            return KF_INVALID_ARGS;
        }
        branch = b, l0 = b * LIS, l1 = l0 + LIS;
        ids = nullptr; /* the kept activations belong to the branch that ran: a Backward needs a Forward of this one first */
        return KF_OK;
    }
    // Fuyou::UpdateFollower for every follower of `head` (RLSchedule::ExploreOptimization): launches only -- no allocation, no host sync
    int Evolve(int head, int algorithm, float alpha, float social, float t_cross, uint32_t seed) {
        KF_TRY(Ready());
        if (head < 0 || head >= NBranch()) {
            g_train_err = "kfh_gpt2_evolve: head branch " + std::to_string(head) + " of " + std::to_string(NBranch());
            return KF_INVALID_ARGS;
        }
        if (algorithm != KF_EVO_PSO && algorithm != KF_EVO_PSO_GA && algorithm != KF_EVO_MIX) {
            g_train_err = "kfh_gpt2_evolve: unknown algorithm " + std::to_string(algorithm);
            return KF_INVALID_ARGS;
        }
        if (NBranch() == 1) return KF_OK; /* fuyouSwarm.size() <= 1: ExploreOptimization returns early */
        for (int l = 0; l < NL; l++)
            for (int k : {QKV_W, PROJ_W, FC_W, PROJ2_W})
                if (P(l, k).gama) {
                    g_train_err = "kfh_gpt2_evolve: layer " + std::to_string(l) + " matrix " + std::to_string(k) + " is gama-trained (train_target \"gama\"): its parameter is " +
                                  "the blob's (zero, step) slice over frozen packed integers, not a matrix kf_evolve could move towards another branch's -- nothing was changed";
                    return KF_UNSUPPORTED_DATATYPE;
                }
        for (int l = 0; l < NL; l++)
            for (int k : {QKV_W, PROJ_W, FC_W, PROJ2_W}) {
                const TrainTensor &e = P(l, k), &h = P(head * LIS + l % LIS, k);
                if (!e.has_blob || (long long)e.blob.ne0 * e.blob.ne1 != e.n || e.n != h.n || e.blob.ne0 != h.blob.ne0) {
                    g_train_err = "kfh_gpt2_evolve: layer " + std::to_string(l) + " matrix " + std::to_string(k) + " has no [ne0, ne1] master of its head's shape -- nothing was changed";
                    return KF_INVALID_ARGS;
                }
            }
        for (int f = 0; f < NBranch(); f++) {
            if (f == head) continue;
            for (int j = 0; j < LIS; j++)
                for (int k : {QKV_W, PROJ_W, FC_W, PROJ2_W}) {
                    const size_t i = (size_t)(f * LIS + j) * PER_BLOCK + k;
                    TrainTensor& e = params[i];
                    KF_TRY(kf_evolve(ctx, e.p, P(head * LIS + j, k).p, e.blob.ne0, e.blob.ne1, algorithm, alpha, social, t_cross, (uint32_t)((seed + (unsigned long long)i) & 0xFFFFFFFFull)));
                    if (e.requant) KF_TRY(kf_quantize(ctx, &e.blob, e.p, 0));
                }
        }
        return KF_OK;
    }
    // the evaluation half of Fish::ForwardOnRLS: per-row losses of one branch, or their mean over all branches (added in branch order in fp32, divided by nBranch), into the
    // caller's fp32 [B T] device buffer; the active branch is put back.  The kept activations are those of the last branch run: a Backward needs a new Forward.
    int Eval(const int32_t* d_ids, const int32_t* d_tgt, int mode, int b, float* d_out) {
        KF_TRY(Ready());
        if (!d_out || d_out == losses) return KF_INVALID_ARGS;
        if (teacher) {
            g_train_err = "kfh_gpt2_eval: not offered while the trainer distils from a teacher (set_distill): switch distillation off first";
            return KF_INVALID_ARGS;
        }
        if (mode != ENSEMBLE_AGGREGATION && mode != ENSEMBLE_BRANCH) {
            g_train_err = "kfh_gpt2_eval: unknown ensemble mode " + std::to_string(mode);
            return KF_INVALID_ARGS;
        }
        if (mode == ENSEMBLE_BRANCH && (b < 0 || b >= NBranch())) {
            g_train_err = "kfh_gpt2_eval: branch " + std::to_string(b) + " of " + std::to_string(NBranch());
            return KF_INVALID_ARGS;
        }
        const int keep = branch, b0 = mode == ENSEMBLE_BRANCH ? b : 0, nb = mode == ENSEMBLE_BRANCH ? 1 : NBranch();
        int rc = KF_OK;
        for (int k = 0; k < nb && rc == KF_OK; k++) {
            SetActive(b0 + k);
            rc = Forward(d_ids, d_tgt);
            if (rc == KF_OK) rc = kf_loss_mean(ctx, d_out, losses, (size_t)N, k, nb);
        }
        SetActive(keep);
        return rc;
    }
};

}  // namespace koifish

using koifish::Core;
using koifish::GPT2Trainer;
static GPT2Trainer* Gpt2(void* h) { return static_cast<GPT2Trainer*>(Core(h)); }  // for the entries only this family has

extern "C" {
void* kfh_gpt2_create(kf_ctx* ctx, int C, int H, int NL, int V, int Vp, int B, int T) {
    if (!ctx || C < 8 || H < 1 || C % H || NL < 1 || V < 1 || Vp < V || B < 1 || T < 1) return nullptr;
    GPT2Trainer* g = new GPT2Trainer;
    g->ctx = ctx, g->C = C, g->H = H, g->NL = NL, g->V = V, g->Vp = Vp, g->B = B, g->T = T, g->N = B * T, g->hd = C / H;
    g->params.resize((size_t)NL * GPT2Trainer::PER_BLOCK + 4);
    g->wmat.assign(g->params.size(), 0);
    for (int l = 0; l < NL; l++)
        for (int k : {GPT2Trainer::QKV_W, GPT2Trainer::PROJ_W, GPT2Trainer::FC_W, GPT2Trainer::PROJ2_W}) g->wmat[(size_t)l * GPT2Trainer::PER_BLOCK + k] = 1;
    g->acts.resize(NL);
    g->LIS = NL, g->l1 = NL;
    memset(g->acts.data(), 0, sizeof(koifish::BlockActs) * NL);
    return static_cast<koifish::TrainerCore*>(g);
}
void kfh_gpt2_destroy(void* h) { delete Core(h); }
int kfh_gpt2_n_params(void* h) { return (int)Core(h)->params.size(); }
// blob: the descriptor of what the forward reads (null: the tensor is not multiplied as a weight); requant != 0: kf_quantize(blob, master) after every update
int kfh_gpt2_set_param(void* h, int index, void* p, void* g, void* m, void* v, long long n, int decay, const kf_weight* blob, int requant) {
    return Core(h)->SetParam(index, p, g, m, v, n, decay, blob, requant);
}
// "train_target": "gama" for one of a block's four weight matrices (index as kfh_gpt2_set_param): blob a PackedQ group storage; the parameter is ITS [ZERO nGroup][STEP nGroup]
// slice (gama + ne0 + ne1), g / m / v are 2 nGroup bf16 each.  No weight decay, no re-quantisation, AdamW whatever the optimiser switch says.
int kfh_gpt2_set_param_gama(void* h, int index, void* g, void* m, void* v, const kf_weight* blob) {
    return Core(h)->SetParamGama(index, g, m, v, blob);
}
// kf_gama_backward's scratch (device memory, 256-byte aligned, the caller's): at least kf_gama_backward_scratch_bytes of every gama tensor at the step's B * T rows
int kfh_gpt2_set_gama_scratch(void* h, void* scratch, size_t bytes) {
    return Core(h)->SetGamaScratch(scratch, bytes);
}
// ptrs: x h1 m1 r1 qkv att x2 h2 m2 r2 f g
int kfh_gpt2_set_block_acts(void* h, int layer, void* const* ptrs) {
    GPT2Trainer* t = Gpt2(h);
    if (layer < 0 || layer >= t->NL || !ptrs) return KF_INVALID_ARGS;
    koifish::BlockActs& a = t->acts[layer];
    a.x = (kf_bf16*)ptrs[0], a.h1 = (kf_bf16*)ptrs[1], a.m1 = (float*)ptrs[2], a.r1 = (float*)ptrs[3], a.qkv = (kf_bf16*)ptrs[4], a.att = (kf_bf16*)ptrs[5];
    a.x2 = (kf_bf16*)ptrs[6], a.h2 = (kf_bf16*)ptrs[7], a.m2 = (float*)ptrs[8], a.r2 = (float*)ptrs[9], a.f = (kf_bf16*)ptrs[10], a.g = (kf_bf16*)ptrs[11];
    return KF_OK;
}
// ptrs: xf hf mf rf logits losses dx dh dqkv datt d4 scratch_linear_backward scratch_norm_backward scratch_attn_backward
int kfh_gpt2_set_buffers(void* h, void* const* ptrs) {
    GPT2Trainer* t = Gpt2(h);
    if (!ptrs) return KF_INVALID_ARGS;
    t->xf = (kf_bf16*)ptrs[0], t->hf = (kf_bf16*)ptrs[1], t->mf = (float*)ptrs[2], t->rf = (float*)ptrs[3], t->logits = (kf_bf16*)ptrs[4], t->losses = (float*)ptrs[5];
    t->dx = (kf_bf16*)ptrs[6], t->dh = (kf_bf16*)ptrs[7], t->dqkv = (kf_bf16*)ptrs[8], t->datt = (kf_bf16*)ptrs[9], t->d4 = (kf_bf16*)ptrs[10];
    t->sc_lin = ptrs[11], t->sc_ln = ptrs[12], t->sc_at = ptrs[13];
    return KF_OK;
}
int kfh_gpt2_forward(void* h, const int32_t* d_ids, const int32_t* d_tgt) { return Core(h)->Forward(d_ids, d_tgt); }
int kfh_gpt2_backward(void* h) { return Core(h)->Backward(); }
int kfh_gpt2_update(void* h, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
    return Core(h)->Update(lr, beta1, beta2, eps, wd, seed);
}
int kfh_gpt2_step(void* h, const int32_t* d_ids, const int32_t* d_tgt, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
    return Core(h)->Step(d_ids, d_tgt, lr, beta1, beta2, eps, wd, seed);
}
// method 0: AdamW on every tensor (the default); 1: Muon (the reference's default) on the Muon tensors, AdamW on the rest.  Call after every kfh_gpt2_set_param:
// scratch (device memory, 256-byte aligned, the caller's) must hold kf_muon_scratch_bytes of the largest Muon tensor; KF_INVALID_ARGS otherwise, nothing changes.
int kfh_gpt2_set_optimizer(void* h, int method, float lr_scale, float mui, float eps_muon, int tp_decay, void* scratch, size_t scratch_bytes) {
    return Core(h)->SetOptimizer(method, lr_scale, mui, eps_muon, tp_decay, scratch, scratch_bytes);
}
long long kfh_gpt2_steps_taken(void* h) { return Core(h)->t; }
// ---- EOE.  Every refusal leaves the trainer as it was; kfh_gpt2_last_error says why (a refusal of a kf_* entry underneath: kf_last_error).
// layers_in_branch must divide NL (KF_INVALID_ARGS otherwise); 0 or NL: one branch, the whole depth -- the default.  Branch 0 becomes the active one.
int kfh_gpt2_set_branches(void* h, int layers_in_branch) {
    koifish::g_train_err.clear();
    return Gpt2(h)->SetBranches(layers_in_branch);
}
int kfh_gpt2_n_branches(void* h) { return Gpt2(h)->NBranch(); }
// forward / backward / update / step from here on run embed -> the layers of branch b -> lnf -> tied head and touch the shared tensors and that section's only
int kfh_gpt2_set_active_branch(void* h, int b) {
    koifish::g_train_err.clear();
    return Gpt2(h)->SetActive(b);
}
int kfh_gpt2_active_branch(void* h) { return Gpt2(h)->branch; }
// for every branch f != head_branch, every layer offset j, each of qkv.w proj.w fc.w proj2.w: kf_evolve(follower master, head master, ..., seed + the follower tensor's
// index in the registered order), then kf_quantize of the follower's blob.  Biases and norms are not touched (isWMAT).  A gama-trained matrix in ANY section:
// KF_UNSUPPORTED_DATATYPE before anything is launched.  One branch: KF_OK, nothing is done.  algorithm: enum kf_evo_algorithm.
int kfh_gpt2_evolve(void* h, int head_branch, int algorithm, float alpha, float social, float t_cross, uint32_t seed) {
    koifish::g_train_err.clear();
    return Gpt2(h)->Evolve(head_branch, algorithm, alpha, social, t_cross, seed);
}
// mode 0 (AGGREGATION): every branch forward in index order, d_loss_out = their mean; mode 1 (BRANCH): the given branch alone.  d_loss_out: fp32 [B T], the caller's.
int kfh_gpt2_eval(void* h, const int32_t* d_ids, const int32_t* d_tgt, int mode, int branch, float* d_loss_out) {
    koifish::g_train_err.clear();
    return Gpt2(h)->Eval(d_ids, d_tgt, mode, branch, d_loss_out);
}
// gradient norms and clipping: TrainerCore::SetGradClip / GradClipScratchBytes / GradNorms (kf_train_common.hpp)
KFH_GRAD_CLIP_ENTRIES(gpt2, koifish::g_train_err)
// distillation against a teacher's logits: TrainerCore::SetDistill / ForwardLogits
KFH_DISTILL_ENTRIES(gpt2, koifish::g_train_err)
const char* kfh_gpt2_last_error(void) { return koifish::g_train_err.c_str(); }
}
