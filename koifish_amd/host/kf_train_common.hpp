// kf_train_common.hpp -- what the training-step sequencers of libkf_host.so share (koifish::GPT2Trainer, kf_train.cpp; koifish::Qwen3Trainer, kf_train_qwen3.cpp): the
// table of trained tensors, its registration in its three forms (shadow weights / "train_target": "gama" / a low-rank adapter beside a frozen matrix), SLP::Back for one matrix, the optimiser switch and the update loop
// with its seed rule -- and the step around them: Update, Step, the head product + fused classifier that ends every Forward (HeadLoss), the head's backward that starts
// every Backward (HeadBack).  A trainer adds its own activations, Ready, Forward and Backward, and says which registered indices are layer weight matrices (wmat).
// Distillation lives here as well (SetDistill, ForwardLogits): a teacher's logits beside the hard labels, kf_distill_classifier in HeadLoss's place of kf_fused_classifier.
// Gradient norms and clipping (SetGradClip) live here too: one kf_grad_norms call at the head of the update, the clip factors read on the device by kf_adamw_scaled.
// The handle behind the C ABI of both families is the TrainerCore*: the entries the families share call through it (Core), a family's own cast down from it.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "kf_host.hpp"

namespace koifish {

struct TrainTensor {
    kf_bf16 *p = nullptr, *g = nullptr;
    void *m = nullptr, *v = nullptr;
    long long n = 0;
    bool decay = false, has_blob = false, requant = false;
    bool gama = false;  // p is the blob's [ZERO][STEP] slice (n = 2 nGroup): SetParamGama
    bool lora = false;  // blob is the frozen base; p / g / m / v are ONE vector [a (rank ne1) | b (ne0 rank)] (n = rank (ne1 + ne0)): SetParamLora
    int rank = 0;       // of the adapter
    float s = 1.0f;     // the reference's sAB: multiplies both products of a direction
    kf_bf16* ax = nullptr;  // [N, rank], written by the forward and read by the backward (the reference's Ax)
    kf_weight blob;  // what the forward multiplies (f8e5m2 / 4-bit PackedQ / the bf16 master itself for a bf16 head)
};

struct TrainerCore {
    kf_ctx* ctx = nullptr;
    int N = 0;  // token rows of a step: B sequences of T tokens
    int V = 0, Vp = 0, B = 0, T = 0;  // the vocabulary and its padded row count
    kf_bf16 *hf = nullptr, *logits = nullptr, *dh = nullptr;  // the final norm's output, the logits (their gradient after the classifier), the gradient of a norm's output
    float* losses = nullptr;
    const int32_t* ids = nullptr;  // of the last Forward (the embedding backward scatters by them)
    std::vector<TrainTensor> params;
    std::vector<char> wmat;  // per registered index: one of a layer's weight matrices (a Muon / gama candidate)
    void* sc_lin = nullptr;  // kf_linear_backward's scratch
    long long t = 0;         // optimizer steps taken
    // Muon (SetOptimizer): lr_scale, mui, eps_muon, tpDecay of MUON_params_; the caller owns the scratch (sized for the largest Muon tensor)
    enum { OPT_ADAMW = 0, OPT_MUON = 1 };
    int method = OPT_ADAMW, tp_decay = 1;
    float lr_scale = 1.0f, mui = 0.95f, eps_muon = 1e-7f;
    void* sc_muon = nullptr;
    size_t sc_muon_bytes = 0;
    void* sc_gama = nullptr;  // kf_gama_backward's slab partials, sized for the largest gama tensor (SetGamaScratch)
    size_t sc_gama_bytes = 0;
    void* sc_lora = nullptr;  // kf_lora_backward's scratch, sized for the largest adapted matrix (SetLoraScratch)
    size_t sc_lora_bytes = 0;
    // gradient norms and clipping (SetGradClip): CLIP_REPORT / _TENSOR / _GLOBAL are kf_clip_mode's values.  The caller's scratch holds kf_grad_norms' table and
    // partials, then d_sumsq [n + 1] fp64, d_gnorm [n + 1] float, d_scale [n] float (each part rounded up to 256 bytes); n = params.size()
    enum { CLIP_OFF = 0, CLIP_REPORT = KF_CLIP_REPORT, CLIP_TENSOR = KF_CLIP_TENSOR, CLIP_GLOBAL = KF_CLIP_GLOBAL };
    int clip_mode = CLIP_OFF;
    float gclip = 1.0f;
    bool clip_stale = false;   // a tensor was registered again, or the optimiser switched, after SetGradClip: the table or its Muon mask no longer holds
    bool norms_valid = false;  // an update has filled d_gnorm since SetGradClip
    void* sc_clip = nullptr;
    double* d_sumsq = nullptr;
    float *d_gnorm = nullptr, *d_scale = nullptr;
    // distillation (SetDistill): with a teacher set, HeadLoss ends in kf_distill_classifier instead of kf_fused_classifier.  The teacher's logits [N, teacher_ld] bf16
    // and the KL rows [N] fp32 are the caller's; who fills the teacher's rows before a Forward is the caller's business too (another trainer's ForwardLogits)
    const kf_bf16* teacher = nullptr;
    long long teacher_ld = 0;
    float ce_weight = 1.0f, kd_weight = 0.0f, temperature = 1.0f;
    float* kd_rows = nullptr;
    // packed documents (Qwen3Trainer::SetDocuments): the mask words of the step's rows (bit 0x10000, F_IGNORE_LOSS: the row's target does not count) and the number
    // of rows that count.  With a mask HeadLoss takes the mean over n_valid rows and leaves exact zeros in the ignored rows of `logits`
    const int32_t* loss_mask = nullptr;
    int n_valid = 0;

    virtual ~TrainerCore() {}  // touches no context (it may be gone already): the owner of a clip scratch switches clipping off before it frees the scratch
    virtual bool InSection(size_t) const { return true; }  // Update leaves a tensor outside the active section alone (EOE)
    virtual int Ready() const = 0;  // everything registered that a step reads (ParamsReady + the trainer's own activations and buffers)
    virtual int Trunk(const int32_t* d_ids) = 0;  // the family's forward up to hf, the final norm's output: the embedding and the layer loop, written once
    virtual TrainTensor& HeadTensor() = 0;        // what the head product multiplies
    virtual bool Sectioned() const { return false; }  // EOE layer sections are set (GPT-2 only)
    virtual int Backward() = 0;
    // per-row losses in `losses`, the logit gradients of the MEAN loss in `logits`
    int Forward(const int32_t* d_ids, const int32_t* d_tgt) {
        KF_TRY(Ready());
        if (!d_ids || !d_tgt) return KF_INVALID_ARGS;
        KF_TRY(Trunk(d_ids));
        return HeadLoss(HeadTensor(), d_ids, d_tgt);
    }
    // the forward through the head product only: raw logits in `logits`, no classifier, nothing a Backward could start from (ids is cleared: HeadBack refuses)
    int ForwardLogits(const int32_t* d_ids, std::string* why) {
        if (Ready() != KF_OK || !d_ids) {
            if (why) *why = "forward_logits: every tensor and buffer must be registered, and ids must not be NULL";
            return KF_INVALID_ARGS;
        }
        ids = nullptr;
        KF_TRY(Trunk(d_ids));
        return kf_linear(ctx, &HeadTensor().blob, hf, logits, nullptr, N, 1.0f, 0.0f, 0u, nullptr);
    }
    // teacher_logits == NULL: distillation off, the plain path bit for bit.  Otherwise every Forward from here on ends in kf_distill_classifier over (logits, teacher):
    // losses[row] = ce_weight CE + kd_weight temperature^2 KL, kd_rows[row] (may be NULL) = KL, the gradient of their mean in `logits`.  A refusal changes nothing;
    // *why says which.  Eval shares the one `losses` buffer with the step and is not defined under distillation: a trainer with EOE sections is refused.
    int SetDistill(const kf_bf16* teacher_logits, long long ld, float ce_w, float kd_w, float tau, float* kd_out, std::string* why) {
        auto refuse = [why](const char* msg) {
            if (why) *why = msg;
            return (int)KF_INVALID_ARGS;
        };
        if (!teacher_logits) {
            teacher = nullptr, teacher_ld = 0, kd_rows = nullptr, ce_weight = 1.0f, kd_weight = 0.0f, temperature = 1.0f;
            return KF_OK;
        }
        if (loss_mask) return refuse("set_distill: documents are set (set_documents): the teacher's forward would need the same layout -- switch them off first");
        if (Ready() != KF_OK) return refuse("set_distill: every tensor and buffer must be registered first");
        if (Sectioned()) return refuse("set_distill: a trainer with EOE layer sections (layers_in_branch) is not distilled: eval shares the step's loss buffer");
        if (!(std::isfinite(ce_w) && std::isfinite(kd_w) && ce_w >= 0.0f && kd_w >= 0.0f) || (ce_w == 0.0f && kd_w == 0.0f))
            return refuse("set_distill: ce_weight and kd_weight must be finite and >= 0, and not both zero");
        if (!(std::isfinite(tau) && tau > 0.0f)) return refuse("set_distill: the temperature must be finite and > 0");
        if (ld < V || (ld & 7) || ((uintptr_t)teacher_logits & 15)) return refuse("set_distill: teacher rows must be 16-byte aligned, teacher_ld >= V a multiple of 8");
        const uintptr_t z0 = (uintptr_t)logits, z1 = z0 + (size_t)N * Vp * 2, u0 = (uintptr_t)teacher_logits, u1 = u0 + (size_t)N * (size_t)ld * 2;
        if (z0 < u1 && u0 < z1) return refuse("set_distill: the teacher's logits overlap the trainer's own (a trainer cannot be its own teacher)");
        if (kd_out && ((uintptr_t)kd_out & 3)) return refuse("set_distill: kd_rows is not 4-byte aligned");
        teacher = teacher_logits, teacher_ld = ld, ce_weight = ce_w, kd_weight = kd_w, temperature = tau, kd_rows = kd_out;
        return KF_OK;
    }

    // MUON_params_::isAdamW restated: a Muon tensor is one of a layer's weight matrices with ne0 >= ne1 (the registered blob descriptor carries the shape) and a
    // [ne0, ne1] bf16 master; embeddings, biases, norms, matrices with ne0 < ne1 and gama-trained tensors stay on AdamW.  An adapter is never a Muon tensor: its
    // parameter is the vector [a | b], not a matrix kf_muon could orthogonalise
    bool IsMuon(size_t i) const {
        if (method != OPT_MUON || i >= wmat.size() || !wmat[i]) return false;
        const TrainTensor& e = params[i];
        return !e.gama && !e.lora && e.has_blob && e.blob.ne0 >= e.blob.ne1 && (long long)e.blob.ne0 * e.blob.ne1 == e.n;
    }
    int SetOptimizer(int method_, float lr_scale_, float mui_, float eps_muon_, int tp_decay_, void* scratch, size_t scratch_bytes) {
        if (method_ != OPT_ADAMW && method_ != OPT_MUON) return KF_INVALID_ARGS;
        if (method_ == OPT_MUON) {
            if (!(lr_scale_ > 0.0f) || !scratch) return KF_INVALID_ARGS;
            const int keep = method;
            method = OPT_MUON;
            size_t need = 0;
            bool ok = true;
            for (size_t i = 0; i < params.size(); i++)
                if (IsMuon(i)) {
                    const size_t b = kf_muon_scratch_bytes(params[i].blob.ne0, params[i].blob.ne1);
                    ok = ok && b > 0;
                    need = b > need ? b : need;
                }
            method = keep;
            if (!ok || scratch_bytes < need) return KF_INVALID_ARGS;
        }
        if (clip_mode != CLIP_OFF && method_ != method) clip_stale = true; /* the table masks the Muon tensors */
        method = method_, lr_scale = lr_scale_, mui = mui_, eps_muon = eps_muon_, tp_decay = tp_decay_, sc_muon = scratch, sc_muon_bytes = scratch_bytes;
        return KF_OK;
    }
    // ---- gradient norms and clipping.  The reference: a norm per tensor with a blocking read-back (GTensor::Length), grad_scale = gnorm > gclip ? gclip / gnorm : 1
    // on the host (Optimizer.cu:756-774), Optimizer::gClip over the whole gradient (Optimizer.cpp:276-308), |g| = sqrt(sum gnorm^2) printed with the loss.
    static size_t Up256(size_t v) { return (v + 255) & ~(size_t)255; }
    bool AllRegistered() const {
        for (const TrainTensor& e : params)
            if (!e.p || !e.g || !e.m || !e.v || e.n < 8 || (e.n & 7)) return false;
        return !params.empty();
    }
    // the table and partials of kf_grad_norms over the registered lengths, then the three output arrays; 0 before every tensor is registered
    size_t GradClipScratchBytes() const {
        if (!AllRegistered()) return 0;
        std::vector<long long> n(params.size());
        for (size_t i = 0; i < params.size(); i++) n[i] = params[i].n;
        const size_t tab = kf_grad_norms_scratch_bytes((int)n.size(), n.data());
        return tab ? tab + Up256(8 * (n.size() + 1)) + Up256(4 * (n.size() + 1)) + Up256(4 * n.size()) : 0;
    }
    // mode CLIP_OFF: nothing is launched by the update (the default; scratch is not looked at).  Otherwise the table over EVERY registered tensor's g / n is written
    // to the caller's scratch (device memory, 256-byte aligned, at least GradClipScratchBytes()), the Muon tensors masked to 1.0f: the reference's Muon path reads the
    // raw gradient.  They still count in the total, which is the reported |g|.  A refusal changes nothing; *why says which (empty: kf_last_error does).
    int SetGradClip(int mode, float gclip_, void* scratch, size_t scratch_bytes, std::string* why) {
        auto refuse = [why](const char* msg) {
            if (why) *why = msg;
            return (int)KF_INVALID_ARGS;
        };
        if (mode != CLIP_OFF && mode != CLIP_REPORT && mode != CLIP_TENSOR && mode != CLIP_GLOBAL) return refuse("set_grad_clip: unknown mode (0 off, 1 report, 2 tensor, 3 global)");
        if (mode == CLIP_OFF) {
            if (sc_clip) (void)kf_grad_norms_forget(ctx, sc_clip);
            clip_mode = CLIP_OFF, clip_stale = false, norms_valid = false, sc_clip = nullptr, d_sumsq = nullptr, d_gnorm = d_scale = nullptr;
            return KF_OK;
        }
        if (mode != CLIP_REPORT && !(std::isfinite(gclip_) && gclip_ > 0.0f)) return refuse("set_grad_clip: gclip must be finite and > 0");
        const size_t need = GradClipScratchBytes();
        if (!need) return refuse("set_grad_clip: every tensor must be registered first");
        if (!scratch || ((uintptr_t)scratch & 255)) return refuse("set_grad_clip: scratch is missing or not 256-byte aligned");
        if (scratch_bytes < need) return refuse("set_grad_clip: scratch shorter than grad_clip_scratch_bytes");
        const size_t nt = params.size();
        std::vector<long long> n(nt);
        std::vector<const kf_bf16*> g(nt);
        std::vector<uint8_t> mask(nt);
        for (size_t i = 0; i < nt; i++) n[i] = params[i].n, g[i] = params[i].g, mask[i] = IsMuon(i) ? 1 : 0;
        const size_t tab = kf_grad_norms_scratch_bytes((int)nt, n.data());
        KF_TRY(kf_grad_norms_plan(ctx, (int)nt, g.data(), n.data(), mask.data(), scratch, tab));
        if (sc_clip && sc_clip != scratch) (void)kf_grad_norms_forget(ctx, sc_clip); /* the scratch this one replaces is the caller's to free from here on */
        char* const sc = (char*)scratch;
        sc_clip = scratch, d_sumsq = (double*)(sc + tab), d_gnorm = (float*)(sc + tab + Up256(8 * (nt + 1))), d_scale = (float*)(sc + tab + Up256(8 * (nt + 1)) + Up256(4 * (nt + 1)));
        clip_mode = mode, gclip = mode == CLIP_REPORT ? 1.0f : gclip_, clip_stale = false, norms_valid = false;
        return KF_OK;
    }
    // the one host read: d_gnorm of the last update, h_out [params.size() + 1] (registration order, then |g| of the whole gradient).  Never inside Update.
    int GradNorms(float* h_out, int n) {
        if (!h_out || clip_mode == CLIP_OFF || !norms_valid || n != (int)params.size() + 1) return KF_INVALID_ARGS;
        return kf_d2h(ctx, h_out, d_gnorm, sizeof(float) * (size_t)n);
    }
    // blob: the descriptor of what the forward reads (null: the tensor is not multiplied as a weight); requant != 0: kf_quantize(blob, master) after every update
    int SetParam(int index, void* p, void* g, void* m, void* v, long long n, int decay, const kf_weight* blob, int requant) {
        if (index < 0 || index >= (int)params.size() || !p || !g || !m || !v || n < 8 || (n & 7)) return KF_INVALID_ARGS;
        TrainTensor& e = params[index];
        e.p = (kf_bf16*)p, e.g = (kf_bf16*)g, e.m = m, e.v = v, e.n = n, e.decay = decay != 0, e.has_blob = blob != nullptr, e.requant = blob && requant, e.gama = false, e.lora = false;
        if (blob) e.blob = *blob;
        if (clip_mode != CLIP_OFF) clip_stale = true;
        return KF_OK;
    }
    // "train_target": "gama" for one of a layer's weight matrices: blob a PackedQ group storage; the parameter is ITS [ZERO nGroup][STEP nGroup] slice
    // (gama + ne0 + ne1), g / m / v are 2 nGroup bf16 each.  No weight decay, no re-quantisation, AdamW whatever the optimiser switch says.
    int SetParamGama(int index, void* g, void* m, void* v, const kf_weight* blob) {
        if (index < 0 || index >= (int)params.size() || !wmat[index] || !g || !m || !v || !blob) return KF_INVALID_ARGS;
        if (!blob->gama || blob->qzeros || blob->qscales || blob->quant != KF_QUANT_GROUP || (blob->type != KF_Q4 && blob->type != KF_T_SIGN && blob->type != KF_BOOL1)) return KF_UNSUPPORTED_DATATYPE;
        if (blob->nGroup < 4 || (blob->nGroup & 3) || (long long)blob->nGroup * blob->lGroup != (long long)blob->ne0 * blob->ne1) return KF_INVALID_ARGS;
        TrainTensor& e = params[index];
        e.blob = *blob;
        e.p = const_cast<kf_bf16*>(blob->gama) + blob->ne0 + blob->ne1, e.g = (kf_bf16*)g, e.m = m, e.v = v, e.n = 2LL * blob->nGroup;
        e.decay = false, e.has_blob = true, e.requant = false, e.gama = true, e.lora = false;
        if (clip_mode != CLIP_OFF) clip_stale = true;
        return KF_OK;
    }
    // kf_gama_backward's scratch (device memory, 256-byte aligned, the caller's): at least kf_gama_backward_scratch_bytes of every gama tensor at the step's rows
    int SetGamaScratch(void* scratch, size_t bytes) {
        if (!scratch || ((uintptr_t)scratch & 255)) return KF_INVALID_ARGS;
        sc_gama = scratch, sc_gama_bytes = bytes;
        return KF_OK;
    }
    // a low-rank adapter beside one of a layer's weight matrices (SLP's LORA branch): blob the frozen base in any storage kf_linear / kf_linear_backward serve, never
    // re-quantised; p / g / m / v one vector [a (rank x ne1) | b (ne0 x rank)] each, so the update, the seed rule, the norms and the clipping see ONE tensor; decayed
    // like any other 2-D tensor (the reference registers a and b as ordinary gensors); AdamW whatever the optimiser switch says.  ax: [N, rank] bf16, this tensor's own.
    int SetParamLora(int index, void* p, void* g, void* m, void* v, int rank_, float s_, void* ax_, const kf_weight* blob) {
        if (index < 0 || index >= (int)params.size() || !wmat[index] || !p || !g || !m || !v || !ax_ || !blob || !std::isfinite(s_)) return KF_INVALID_ARGS;
        if (kf_lora_backward_scratch_bytes(rank_, blob->ne0, blob->ne1, 64) == 0) return KF_INVALID_ARGS; /* the rank or the matrix is none the entries take */
        TrainTensor& e = params[index];
        e.blob = *blob;
        e.p = (kf_bf16*)p, e.g = (kf_bf16*)g, e.m = m, e.v = v, e.n = (long long)rank_ * ((long long)blob->ne0 + blob->ne1);
        e.decay = true, e.has_blob = true, e.requant = false, e.gama = false, e.lora = true, e.rank = rank_, e.s = s_, e.ax = (kf_bf16*)ax_;
        if (clip_mode != CLIP_OFF) clip_stale = true;
        return KF_OK;
    }
    // kf_lora_backward's scratch (device memory, 256-byte aligned, the caller's): at least kf_lora_backward_scratch_bytes of every adapter at the step's rows
    int SetLoraScratch(void* scratch, size_t bytes) {
        if (!scratch || ((uintptr_t)scratch & 255)) return KF_INVALID_ARGS;
        sc_lora = scratch, sc_lora_bytes = bytes;
        return KF_OK;
    }
    // every tensor registered; every gama tensor a shape the entry takes, with scratch; no dequant arena beside a gama tensor; the clip table, if any, still the
    // registered tensors'
    int ParamsReady() const {
        if (clip_stale) return KF_INVALID_ARGS;
        for (const TrainTensor& e : params)
            if (!e.p || !e.g || !e.m || !e.v || e.n < 8 || (e.n & 7)) return KF_INVALID_ARGS;
        for (size_t i = 0; i < params.size(); i++)
            if (wmat[i] && !params[i].has_blob) return KF_INVALID_ARGS;
        bool any_gama = false;
        for (const TrainTensor& e : params)
            if (e.gama) {
                const size_t b = kf_gama_backward_scratch_bytes(e.blob.ne0, e.blob.ne1, N);
                if (b == 0 || !sc_gama || sc_gama_bytes < b) return KF_INVALID_ARGS; /* a shape the entry refuses, or no / too small a scratch */
                any_gama = true;
            }
        if (any_gama && kf_dequant_arena_bytes(ctx) > 0) return KF_INVALID_ARGS; /* resident dequantised copies would go stale with the first update */
        for (const TrainTensor& e : params)
            if (e.lora) { /* an adapter's base never changes: a dequant arena beside it stays valid and is not refused */
                const size_t b = kf_lora_backward_scratch_bytes(e.rank, e.blob.ne0, e.blob.ne1, N);
                if (b == 0 || !sc_lora || sc_lora_bytes < b) return KF_INVALID_ARGS;
            }
        return KF_OK;
    }
    // SLP::Forw for one matrix: the base product with its epilogue, then -- LORA branch -- the adapter's two products on the same y (ax kept)
    int LinForw(TrainTensor& w, const kf_bf16* x, kf_bf16* y, const kf_bf16* res) {
        KF_TRY(kf_linear(ctx, &w.blob, x, y, nullptr, N, 1.0f, 0.0f, res ? 1u : 0u, res));
        if (!w.lora) return KF_OK;
        return kf_lora_forward(ctx, w.p, w.p + (size_t)w.rank * w.blob.ne1, w.rank, w.blob.ne0, w.blob.ne1, x, y, w.ax, N, w.s);
    }
    // SLP::Back (NeuronFuse.cu:495-563): weight / bias gradients into the tensors' own buffers, delta (accumulate: on top of what it holds) to the layer below
    int LinBack(TrainTensor& w, const kf_bf16* dIn, const kf_bf16* inp, kf_bf16* delta, TrainTensor* bias, int accumulate = 0) {
        if (w.gama) { /* the gama branch of SLP::Back: delta and the bias gradient as ever, no gW; then the (zero, step) gradients from the same two operands */
            KF_TRY(kf_linear_backward(ctx, &w.blob, dIn, inp, delta, nullptr, bias ? bias->g : nullptr, N, accumulate, sc_lin));
            return kf_gama_backward(ctx, &w.blob, dIn, inp, w.g, N, 1.0f, sc_gama);
        }
        if (w.lora) { /* the LORA branch: the frozen base gives delta (and the bias gradient) and no gW; the adapter then adds its share of delta and its two gradients */
            KF_TRY(kf_linear_backward(ctx, &w.blob, dIn, inp, delta, nullptr, bias ? bias->g : nullptr, N, accumulate, sc_lin));
            return kf_lora_backward(ctx, w.p, w.p + (size_t)w.rank * w.blob.ne1, w.rank, w.blob.ne0, w.blob.ne1, dIn, inp, w.ax, delta, w.g, N, w.s, sc_lora);
        }
        return kf_linear_backward(ctx, &w.blob, dIn, inp, delta, w.g, bias ? bias->g : nullptr, N, accumulate, sc_lin);
    }
    // CU_adamw_ on every tensor (its own master, moments and gradient; seeded stochastic rounding: seed + 7919 t + the tensor's index, one seed per launch as the
    // reference draws one per tensor update), then the re-quantisation of every quantised matrix from its updated master.  kf_adamw zeroes the gradients it has
    // consumed.  With the Muon switch a Muon tensor takes PIPE_Muon::CU_core instead (kf_muon: mG is its m buffer, v is not touched; lr x lr_scale, the weight decay
    // by tpDecay, Pipe.cpp:23-37; the same seed as its AdamW launch would have had).
    // With SetGradClip: first ONE kf_grad_norms over every registered tensor (a tensor outside the active section holds a zero gradient and adds nothing), then
    // every AdamW tensor -- gama tensors among them -- reads its clip factor on the device (kf_adamw_scaled); a Muon tensor is left as it is.  No host read.
    int UpdateParams(float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
        t++;
        if (clip_mode != CLIP_OFF) {
            KF_TRY(kf_grad_norms(ctx, sc_clip, (int)params.size(), clip_mode, gclip, d_sumsq, d_gnorm, d_scale));
            norms_valid = true;
        }
        const float b1c = (float)(1.0 - std::pow(beta1, (double)t)), b2c = (float)(1.0 - std::pow(beta2, (double)t)); /* the bias corrections, in double like the host side of the reference */
        for (size_t i = 0; i < params.size(); i++) {
            if (!InSection(i)) continue; /* a tensor of another branch: not touched, its seed index skipped */
            TrainTensor& e = params[i];
            const uint32_t sd = (uint32_t)((seed + 7919ull * (unsigned long long)t + i) & 0xFFFFFFFFull);
            if (IsMuon(i)) {
                const float wd0 = e.decay ? wd : 0.0f, wd_muon = tp_decay == 0 ? 0.0f : (tp_decay == 1 ? wd0 / lr_scale : wd0);
                KF_TRY(kf_muon(ctx, e.p, e.g, (kf_bf16*)e.m, e.blob.ne0, e.blob.ne1, lr * lr_scale, wd_muon, mui, eps_muon, 5, sd, sc_muon, sc_muon_bytes, nullptr));
                if (e.requant) KF_TRY(kf_quantize(ctx, &e.blob, e.p, 0));
                continue;
            }
            if (clip_mode != CLIP_OFF)
                KF_TRY(kf_adamw_scaled(ctx, e.p, e.g, e.m, e.v, (size_t)e.n, KF_BF16, lr, (float)beta1, (float)beta2, b1c, b2c, eps, e.decay ? wd : 0.0f,
                                       d_scale + i, sd, nullptr));
            else
                KF_TRY(kf_adamw(ctx, e.p, e.g, e.m, e.v, (size_t)e.n, KF_BF16, lr, (float)beta1, (float)beta2, b1c, b2c, eps, e.decay ? wd : 0.0f, 1.0f,
                                sd, nullptr));
            if (e.requant) KF_TRY(kf_quantize(ctx, &e.blob, e.p, 0));
        }
        return KF_OK;
    }
    int Update(float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
        KF_TRY(Ready());
        return UpdateParams(lr, beta1, beta2, eps, wd, seed);
    }
    int Step(const int32_t* d_ids, const int32_t* d_tgt, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed) {
        KF_TRY(Forward(d_ids, d_tgt));
        KF_TRY(Backward());
        return Update(lr, beta1, beta2, eps, wd, seed);
    }
    // the end of every Forward: logits = hf . head^T, then the fused classifier -- the distilling one under SetDistill --: per-row losses in `losses`, the logit gradients
    // of the MEAN loss in `logits`
    int HeadLoss(TrainTensor& head, const int32_t* d_ids, const int32_t* d_tgt) {
        KF_TRY(kf_linear(ctx, &head.blob, hf, logits, nullptr, N, 1.0f, 0.0f, 0u, nullptr));
        KF_TRY(kf_memset(ctx, losses, 0, (size_t)N * 4));
        if (teacher)
            KF_TRY(kf_distill_classifier(ctx, logits, teacher, teacher_ld, losses, kd_rows, 1.0f / (float)N, d_tgt, B, T, V, Vp, nullptr, ce_weight, kd_weight, temperature, 1));
        else if (loss_mask) { /* the classifier skips an ignored row entirely: its raw logits would be read as a gradient by HeadBack */
            KF_TRY(kf_fused_classifier(ctx, logits, losses, nullptr, 1.0f / (float)n_valid, d_tgt, B, T, V, Vp, loss_mask, 1));
            KF_TRY(kf_zero_ignored_rows(ctx, logits, N, Vp, loss_mask));
        } else
            KF_TRY(kf_fused_classifier(ctx, logits, losses, nullptr, 1.0f / (float)N, d_tgt, B, T, V, Vp, nullptr, 1));
        ids = d_ids;
        return KF_OK;
    }
    // the start of every Backward (after Ready): refused without a Forward; the head's weight gradient, and dh = the gradient of hf
    int HeadBack(TrainTensor& head) {
        if (!ids) return KF_INVALID_ARGS;
        if (Vp > V) KF_TRY(kf_memset2d(ctx, logits + V, (size_t)Vp * 2, 0, (size_t)(Vp - V) * 2, (size_t)N)); /* the padded vocabulary columns carry no gradient */
        return LinBack(head, logits, hf, dh, nullptr);
    }
};

inline TrainerCore* Core(void* h) { return static_cast<TrainerCore*>(h); }  // the handle of kfh_gpt2_* / kfh_qwen3t_*

// The distillation entries of a family, from one place: kfh_<fam>_set_distill (teacher_logits NULL: off; the reason of a refusal in the family's error string, which
// kfh_<fam>_last_error hands out) and kfh_<fam>_forward_logits (a refusal of a kf_* entry underneath: kf_last_error).
#define KFH_DISTILL_ENTRIES(fam, err)                                                                                                                         \
    int kfh_##fam##_set_distill(void* h, const void* teacher_logits, int64_t teacher_ld, float ce_weight, float kd_weight, float temperature, void* kd_rows) { \
        (err).clear();                                                                                                                                        \
        return koifish::Core(h)->SetDistill((const kf_bf16*)teacher_logits, teacher_ld, ce_weight, kd_weight, temperature, (float*)kd_rows, &(err));          \
    }                                                                                                                                                         \
    int kfh_##fam##_forward_logits(void* h, const int32_t* d_ids) {                                                                                           \
        (err).clear();                                                                                                                                        \
        return koifish::Core(h)->ForwardLogits(d_ids, &(err));                                                                                                \
    }

// The gradient-clipping entries of a family, from one place: kfh_<fam>_set_grad_clip (mode 0 off, else kf_clip_mode; the reason of a refusal in the family's error
// string `err`, which kfh_<fam>_last_error hands out), kfh_<fam>_grad_clip_scratch_bytes, kfh_<fam>_grad_norms (h_out: float [n_params + 1], the last one |g|).
#define KFH_GRAD_CLIP_ENTRIES(fam, err)                                                                                         \
    int kfh_##fam##_set_grad_clip(void* h, int mode, float gclip, void* scratch, size_t scratch_bytes) {                        \
        (err).clear();                                                                                                          \
        return koifish::Core(h)->SetGradClip(mode, gclip, scratch, scratch_bytes, &(err));                                      \
    }                                                                                                                           \
    size_t kfh_##fam##_grad_clip_scratch_bytes(void* h) { return koifish::Core(h)->GradClipScratchBytes(); }                    \
    int kfh_##fam##_grad_norms(void* h, float* h_out, int n) {                                                                  \
        (err).clear();                                                                                                          \
        const int rc = koifish::Core(h)->GradNorms(h_out, n);                                                                   \
        if (rc == KF_INVALID_ARGS) (err) = "grad_norms: needs set_grad_clip, an update since, and room for n_params + 1 floats"; \
        return rc;                                                                                                              \
    }

}  // namespace koifish
