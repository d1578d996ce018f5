// kf_host.cpp -- see kf_host.hpp.  Plain C++17, no HIP headers; every device action is a kf_* ABI call.
#include "kf_host.hpp"
#include "../../include/kf_host_abi.h"

#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace koifish {

// ------------------------------------------------------------------------------------------------ GTensor
kf_weight GTensor::desc() const {
    kf_weight w;
    std::memset(&w, 0, sizeof(w));
    w.data = data;
    w.gama = gama_T();
    w.type = (int32_t)type;
    w.ne0 = ne[0], w.ne1 = ne[1];
    w.lGroup = quant.T_group;
    w.nGroup = nGroup();
    w.qMin = quant.qMin, w.qMax = quant.qMax, w.qBias = quant.qBias;
    if (quant.isNormalFloat) w.quant = KF_QUANT_ROW_LUT, w.nGroup = 0, w.lGroup = 0;
    if (qZero && qScale) w.qzeros = qZero->data, w.qscales = qScale->data, w.nGroup = (int)(size() / 128), w.gama = nullptr;
    return w;
}
int GTensor::Alloc(kf_ctx* c, size_t nbytes) {
    ctx = c;
    const int rc = mem.Alloc(c, nbytes);
    data = mem; /* the view follows the block: NULL when refused */
    return rc;
}
int GTensor::LoadBlob(kf_ctx* c, const void* h_blob, size_t nbytes) {
    KF_TRY(Alloc(c, nbytes));
    return kf_h2d(c, data, h_blob, nbytes);
}
static size_t type_bytes(typNUMBER tp) { /* F32 .. I64 in typNUMBER's order; 0: a packed type behind them, sized by its quant card, not here */
    static const uint8_t kBytes[] = {4, 8, 2, 2, 1, 1, 1, 1, 2, 2, 4, 4, 8, 8};
    return (size_t)tp < sizeof(kBytes) ? kBytes[(size_t)tp] : 0;
}
hGTensor GT(kf_ctx* c, const std::string& name, typNUMBER tp, int n0, int n1) {
    auto t = std::make_shared<GTensor>();
    t->name = name, t->type = tp, t->ne[0] = n0, t->ne[1] = n1;
    if (!type_bytes(tp)) return nullptr;
    const size_t bytes = (size_t)n0 * n1 * type_bytes(tp);
    t->szData = bytes;
    if (t->Alloc(c, bytes) != KF_OK) return nullptr;
    kf_memset(c, t->data, 0, bytes);
    return t;
}

// ------------------------------------------------------------------------------------------------ KVCache
int KVCache::Init(kf_ctx* c, int nl, int ms, int kvd) {
    n_layer = nl, max_seq_len = ms, kv_dim = kvd;
    key = GT(c, "kv.key", typNUMBER::BF16, nl * ms, kvd);
    val = GT(c, "kv.val", typNUMBER::BF16, nl * ms, kvd);
    return (key && val) ? KF_OK : KF_OUTOF_GPUMEMORY;
}
int KVCache::Init8(kf_ctx* c, int nkv) {
    if (k8) return KF_OK;
    n_kv = nkv;
    const int rows = n_layer * max_seq_len;
    hGTensor a = GT(c, "kv.k8", typNUMBER::I8, rows, kv_dim), b = GT(c, "kv.v8", typNUMBER::I8, rows, kv_dim);
    hGTensor sa = GT(c, "kv.ks", typNUMBER::F32, rows, nkv), sb = GT(c, "kv.vs", typNUMBER::F32, rows, nkv);
    hGTensor ta = GT(c, "kv.stage_k", typNUMBER::BF16, max_seq_len, kv_dim), tb = GT(c, "kv.stage_v", typNUMBER::BF16, max_seq_len, kv_dim);
    if (!a || !b || !sa || !sb || !ta || !tb) return KF_OUTOF_GPUMEMORY;
    k8 = a, v8 = b, ks = sa, vs = sb, stage_k = ta, stage_v = tb;
    return KF_OK;
}
void* KVCache::Get(CTYPE type, int layer, int pos) const {
    floatX* base = ToX(type == KV_KEY ? key : val);
    return base + ((size_t)layer * max_seq_len + pos) * kv_dim;
}

// ------------------------------------------------------------------------------------------------ sampler, sequence buffers
bool CHAT_SAMPLER::Valid(int vocab) const {
    if (greedy()) return true;
    const int k = top_k < vocab ? top_k : vocab;
    return !(k < 2 || k >= vocab / 2 || k > 1024 || !(temperature > 0.0f) || !(top_p > 0.0f));
}
CHAT_SAMPLER CHAT_SAMPLER::FromArgs(float temperature, float top_p, int top_k, uint64_t seed) {
    CHAT_SAMPLER s;
    s.temperature = temperature, s.top_p = top_p, s.top_k = top_k & 0xFFFF, s.seed = seed;
    s.true_topk = (top_k & 0x10000) != 0;  // bit 16 of top_k: candidates = the k largest logits (kf_sample_topk)
    return s;
}
int CHAT_SAMPLER::Draw(kf_ctx* c, const floatX* logits, int vocab, uint64_t* rng, int32_t* state, int32_t* ids, const int32_t* forced, int n_ctx) const {
    return (true_topk ? kf_sample_topk : kf_sample)(c, logits, vocab, top_k, temperature, top_p, rng, nullptr, state, ids, forced, n_ctx);
}

// ---- the sets.  A set commits whole or not at all: its Alloc fills a FRESH object, moved over the held one only after every allocation succeeded
template <class Set, class... A>
static int Commit(Set& held, A&&... a) {
    Set fresh;
    KF_TRY(fresh.Alloc(a...));
    held = std::move(fresh);
    return KF_OK;
}
int TokenBatch::Alloc(kf_ctx* c, int n, int dim, int q_dim, int ffn) {
    bX = GT(c, "bX", typNUMBER::BF16, dim, n), bNorm = GT(c, "bNorm", typNUMBER::BF16, dim, n);
    bQ = GT(c, "bQ", typNUMBER::BF16, q_dim, n), bAttn = GT(c, "bAttn", typNUMBER::BF16, q_dim, n);
    bGate = GT(c, "bGate", typNUMBER::BF16, ffn, n), bUp = GT(c, "bUp", typNUMBER::BF16, ffn, n);
    if (!bX || !bNorm || !bQ || !bAttn || !bGate || !bUp) return KF_OUTOF_GPUMEMORY;
    KF_TRY(d_ptok.Alloc(c, (size_t)n * 4));
    rows = n;
    return KF_OK;
}
int VerifyRows::Alloc(kf_ctx* c, const MODEL_CARD& card, const kf_weight& head) {
    const int R = KF_SPEC_MAX_K + 1, qd = card.n_head * card.head_dim;
    vX = GT(c, "vX", typNUMBER::BF16, card.nEmbed, R), vQ = GT(c, "vQ", typNUMBER::BF16, qd, R), vAttn = GT(c, "vAttn", typNUMBER::BF16, qd, R);
    vGate = GT(c, "vGate", typNUMBER::BF16, card.n_ff, R);
    v_attn_ws = GT(c, "v_attn_ws", typNUMBER::F32, (int)((kf_attn_rows_scratch_bytes(card.n_head, card.head_dim, R) + 3) / 4)); /* zero-filled once */
    v_head_ws = GT(c, "v_head_ws", typNUMBER::F32, (int)((kf_head_rows_scratch_bytes(&head) + 3) / 4));
    if (!vX || !vQ || !vAttn || !vGate || !v_attn_ws || !v_head_ws) return KF_OUTOF_GPUMEMORY;
    return d_vtok.Alloc(c, (size_t)2 * R * 4);
}

// ------------------------------------------------------------------------------------------------ neurons
hGTensor LayerNormal::cuFlow(hGTensor inp, int) {
    // P_CHAT_1 && nHead == 0  ->  CU_rms_infer (T.cu:569-573)
    if (kf_rmsnorm(hFish->ctx, ToX(inp), ToX(w), ToX(out), 1, ldTH, rms_eps, nullptr) != KF_OK) return nullptr;
    return out;
}
int Relu::Forw(hGTensor out, hGTensor gate, hGTensor inp, int) {
    return kf_swiglu(hFish->ctx, ToX(gate), ToX(inp), ToX(out), inp->ne[0]) == KF_OK ? 0 : -1;
}
int SLP::Forw(floatX* rhs, const floatX* lhs, uint32_t epilogue, const floatX* residual) {
    kf_weight wd = w->desc();
    return kf_linear(hFish->ctx, &wd, lhs, rhs, b ? ToX(b) : nullptr, 1, 1.0f, 0.0f, epilogue, residual) == KF_OK ? 0 : -1;
}
int SLP::Forw(hGTensor rhs, hGTensor lhs, hGTensor toGelu, Relu*, int) {
    floatX* dst = toGelu ? ToX(toGelu) : ToX(rhs);  // rhs = to_gelu ? to_gelu : rhs (NeuronFuse.cu:332)
    return Forw(dst, ToX(lhs));
}

hGTensor ROPE::cuInfer(SelfAttention* hQKV, uint32_t, int pos, int) {
    Fish* f = hFish;
    floatX* q = ToX(hQKV->Q.out);
    floatX* k = reinterpret_cast<floatX*>(hQKV->hCache->Get(KVCache::KV_KEY, hQKV->layid - 1, pos));
    int rc = kf_qknorm_rope(f->ctx, q, k, hnQ ? ToX(hnQ->w) : nullptr, hnK ? ToX(hnK->w) : nullptr, f->rope_table, pos, nullptr, n_head, n_head_kv, head_dim,
                            hnQ ? hnQ->rms_eps : 1e-6f);
    return rc == KF_OK ? hQKV->Q.out : nullptr;
}

void SelfAttention::_devQKV(int) { /* K.out/V.out are resolved per launch from the cache base + pos (see cuInfer) */ }

hGTensor SelfAttention::cuInfer(hGTensor inpL, int) {
    Fish* f = hFish;
    kf_ctx* c = f->ctx;
    const int pos = f->tok_pos, L = layid - 1;
    floatX* key_cache = reinterpret_cast<floatX*>(hCache->Get(KVCache::KV_KEY, L, 0));
    floatX* val_cache = reinterpret_cast<floatX*>(hCache->Get(KVCache::KV_VAL, L, 0));
    f->gBUFF.residual = inpL;
    const int32_t* d_pos = f->graph_mode ? f->d_state + 1 : nullptr;
    const int bound = f->graph_mode ? f->pos_bound() : pos;
    if (f->EagerOnly()) {  // int8 activations: [norm + quantise] -> Q, K, V -> [q/k-norm + RoPE + attention] -> [quantise] -> proj_cat + residual; 7 launches
                           // adapters: norm -> Q, K, V -> their adapters (one launch, on the raw rows) -> [q/k-norm + RoPE + attention] -> proj_cat + residual -> its adapter; 8 launches
        if (f->graph_mode) return nullptr;  // cache rows are resolved on the host
        SLP* qkv[3] = {&Q, &K, &V};
        floatX* ys[3] = {ToX(Q.out), ToX(f->gBUFF.kraw), val_cache + (size_t)pos * kv_dim};
        if (f->Group(ToX(inpL), ToX(norm.w), norm.rms_eps, 1, f->config.nEmbed, ToX(f->gBUFF.normed), 3, qkv, ys, nullptr) != KF_OK) return nullptr;
        if (kf_attn_block(c, ToX(Q.out), ToX(f->gBUFF.kraw), key_cache, val_cache, ToX(f->gBUFF.scratch), normQ.w ? ToX(normQ.w) : nullptr,
                          normK.w ? ToX(normK.w) : nullptr, f->rope_table, pos, nullptr, n_head, n_head_kv, head_dim, kv_dim, normQ.rms_eps,
                          f->gBUFF.attn_ws->data) != KF_OK)
            return nullptr;
        SLP* o[1] = {&proj_cat};
        floatX* yo[1] = {ToX(out)};
        if (f->Group(ToX(f->gBUFF.scratch), nullptr, 0.0f, 1, q_dim, nullptr, 1, o, yo, ToX(inpL)) != KF_OK) return nullptr;
        return out;
    }
    if (f->fuse_level == 0) {
        if (f->graph_mode) return nullptr;  // the per-kernel path resolves cache rows on the host
        hGTensor inpQ = norm.cuFlow(inpL);
        if (!inpQ) return nullptr;
        floatX* krow = key_cache + (size_t)pos * kv_dim;
        floatX* vrow = val_cache + (size_t)pos * kv_dim;
        if (Q.Forw(ToX(Q.out), ToX(inpQ)) || K.Forw(krow, ToX(inpQ)) || V.Forw(vrow, ToX(inpQ))) return nullptr;
        if (!rope.cuInfer(this, 42, pos)) return nullptr;
        if (kf_attn_decode(c, ToX(Q.out), key_cache, val_cache, ToX(Q.out), pos, nullptr, n_head, n_head_kv, head_dim, kv_dim, f->gBUFF.attn_ws->data) != KF_OK)
            return nullptr;
        if (proj_cat.Forw(ToX(f->gBUFF.scratch), ToX(Q.out))) return nullptr;
        if (kf_add(c, ToX(f->gBUFF.residual), ToX(f->gBUFF.scratch), ToX(out), f->config.nEmbed) != KF_OK) return nullptr;  // CU_add3
        return out;
    }
    // fused: [norm + Q,K,V] -> [q/k-norm + RoPE + attention] -> [proj_cat + residual]
    kf_weight wq = Q.w->desc(), wk = K.w->desc(), wv = V.w->desc(), wo = proj_cat.w->desc();
    const kf_weight* ws[3] = {&wq, &wk, &wv};
    if (f->kv_int8) {  // int8 KV cache: q, the raw k and the raw v into scratch rows (no row of the cache is aliased), then [q/k-norm + RoPE + quantise the new rows +
                       // integer-score attention] in one launch; graph mode works as below: the position comes from d_pos, the bound fixes the slices
        kf_bf16* y8[3] = {ToX(Q.out), ToX(f->gBUFF.kraw), ToX(f->gBUFF.vraw)};
        const int64_t none[3] = {0, 0, 0};
        if (kf_norm_linear(c, ToX(inpL), ToX(norm.w), norm.rms_eps, 3, ws, y8, none, bound, d_pos) != KF_OK) return nullptr;
        if (kf_attn_block_kv8(c, ToX(Q.out), ToX(f->gBUFF.kraw), ToX(f->gBUFF.vraw), hCache->Codes(KVCache::KV_KEY, L), hCache->Codes(KVCache::KV_VAL, L),
                              hCache->Steps(KVCache::KV_KEY, L), hCache->Steps(KVCache::KV_VAL, L), ToX(f->gBUFF.scratch), normQ.w ? ToX(normQ.w) : nullptr,
                              normK.w ? ToX(normK.w) : nullptr, f->rope_table, bound, d_pos, n_head, n_head_kv, head_dim, kv_dim, normQ.rms_eps,
                              f->gBUFF.attn_ws->data) != KF_OK)
            return nullptr;
        if (kf_linear(c, &wo, ToX(f->gBUFF.scratch), ToX(out), nullptr, 1, 1.0f, 0.0f, KF_EPI_RESIDUAL, ToX(inpL)) != KF_OK) return nullptr;
        return out;
    }
    kf_bf16* ys[3] = {ToX(Q.out), ToX(f->gBUFF.kraw), val_cache};
    const int64_t strides[3] = {0, 0, (int64_t)kv_dim};
    if (kf_norm_linear(c, ToX(inpL), ToX(norm.w), norm.rms_eps, 3, ws, ys, strides, bound, d_pos) != KF_OK) return nullptr;
    if (kf_attn_block(c, ToX(Q.out), ToX(f->gBUFF.kraw), key_cache, val_cache, ToX(f->gBUFF.scratch), normQ.w ? ToX(normQ.w) : nullptr,
                      normK.w ? ToX(normK.w) : nullptr, f->rope_table, bound, d_pos, n_head, n_head_kv, head_dim, kv_dim, normQ.rms_eps,
                      f->gBUFF.attn_ws->data) != KF_OK)
        return nullptr;
    if (kf_linear(c, &wo, ToX(f->gBUFF.scratch), ToX(out), nullptr, 1, 1.0f, 0.0f, KF_EPI_RESIDUAL, ToX(inpL)) != KF_OK) return nullptr;
    return out;
}

hGTensor FFN::cuInfer(hGTensor hIn, int) {
    Fish* f = hFish;
    kf_ctx* c = f->ctx;
    f->gBUFF.residual = hIn;
    if (f->EagerOnly()) {  // int8 activations: [norm + quantise] -> gate, up -> SwiGLU -> [quantise] -> down + residual; 6 launches (no hot-row masks: the modes exclude them)
                           // adapters: norm -> gate, up -> their adapters (one launch) -> SwiGLU -> down + residual -> its adapter; 7 launches (no hot-row masks either)
        SLP* gu[2] = {&gate, &up};
        floatX* ys[2] = {ToX(f->gBUFF.scratch), ToX(f->gBUFF.upOut)};
        if (f->Group(ToX(hIn), ToX(norm.w), norm.rms_eps, 1, f->config.nEmbed, ToX(f->gBUFF.normed), 2, gu, ys, nullptr) != KF_OK) return nullptr;
        if (kf_swiglu(c, ToX(f->gBUFF.scratch), ToX(f->gBUFF.upOut), ToX(f->gBUFF.scratch), latent) != KF_OK) return nullptr;
        SLP* d[1] = {&down};
        floatX* yd[1] = {ToX(out)};
        if (f->Group(ToX(f->gBUFF.scratch), nullptr, 0.0f, 1, latent, nullptr, 1, d, yd, ToX(hIn)) != KF_OK) return nullptr;
        return out;
    }
    if (f->fuse_level == 0) {
        hGTensor xn = norm.cuFlow(hIn);
        if (!xn) return nullptr;
        hGTensor tGelu = f->gBUFF.scratch, up_out = f->gBUFF.upOut;
        if (n_hot >= 0) {  // D_matmul_sparse on both projections
            kf_weight wg = gate.w->desc(), wu = up.w->desc();
            const int32_t* rows = reinterpret_cast<const int32_t*>(hot_rows->data);
            if (kf_linear_masked(c, &wg, ToX(xn), ToX(tGelu), nullptr, rows, n_hot) != KF_OK || kf_linear_masked(c, &wu, ToX(xn), ToX(up_out), nullptr, rows, n_hot) != KF_OK)
                return nullptr;
        } else if (gate.Forw(tGelu, xn) || up.Forw(up_out, xn))
            return nullptr;
        if (relu.Forw(tGelu, tGelu, up_out)) return nullptr;
        if (down.Forw(ToX(f->gBUFF.delta), ToX(tGelu))) return nullptr;
        if (kf_add(c, ToX(f->gBUFF.residual), ToX(f->gBUFF.delta), ToX(out), f->config.nEmbed) != KF_OK) return nullptr;
        return out;
    }
    kf_weight wg = gate.w->desc(), wu = up.w->desc(), wd = down.w->desc();
    if (n_hot >= 0) {
        if (kf_norm_gateup_swiglu_masked(c, ToX(hIn), ToX(norm.w), norm.rms_eps, &wg, &wu, ToX(f->gBUFF.scratch), reinterpret_cast<const int32_t*>(hot_rows->data),
                                         n_hot) != KF_OK)
            return nullptr;
    } else if (kf_norm_gateup_swiglu(c, ToX(hIn), ToX(norm.w), norm.rms_eps, &wg, &wu, ToX(f->gBUFF.scratch)) != KF_OK)
        return nullptr;
    if (kf_linear(c, &wd, ToX(f->gBUFF.scratch), ToX(out), nullptr, 1, 1.0f, 0.0f, KF_EPI_RESIDUAL, ToX(hIn)) != KF_OK) return nullptr;
    return out;
}

// ---- token batches (prefill)
int SelfAttention::cuFlow(floatX* bx, int pos0, int n) {
    Fish* f = hFish;
    kf_ctx* c = f->ctx;
    const int L = layid - 1, C = f->config.nEmbed;
    floatX* key_cache = reinterpret_cast<floatX*>(hCache->Get(KVCache::KV_KEY, L, 0));
    floatX* val_cache = reinterpret_cast<floatX*>(hCache->Get(KVCache::KV_VAL, L, 0));
    floatX* krows = key_cache + (size_t)pos0 * kv_dim;
    floatX* vrows = val_cache + (size_t)pos0 * kv_dim;
    floatX *bn = ToX(f->gBUFF.bNorm), *bq = ToX(f->gBUFF.bQ), *ba = ToX(f->gBUFF.bAttn);
    kf_weight wq = Q.w->desc(), wk = K.w->desc(), wv = V.w->desc(), wo = proj_cat.w->desc();
    if (f->EagerOnly()) {  // the unfused sequence: quantise, the integer products on tiles of token rows, then the existing q/k-norm + RoPE, prompt attention, residual epilogue
                           // adapters: kf_rmsnorm, kf_linear per matrix, kf_lora_apply per adapted matrix -- on the RAW k / v rows in the cache, before q/k-norm + RoPE, as the trainer's forward
        SLP* qkv[3] = {&Q, &K, &V};
        floatX* ys[3] = {bq, krows, vrows};
        KF_TRY(f->Group(bx, ToX(norm.w), norm.rms_eps, n, C, bn, 3, qkv, ys, nullptr));
        KF_TRY(kf_qknorm_rope_batch(c, bq, krows, normQ.w ? ToX(normQ.w) : nullptr, normK.w ? ToX(normK.w) : nullptr, f->rope_table, pos0, n, q_dim, kv_dim, n_head, n_head_kv,
                                    head_dim, normQ.rms_eps));
        KF_TRY(kf_attn_prefill(c, bq, key_cache, val_cache, ba, pos0, n, q_dim, n_head, n_head_kv, head_dim, kv_dim));
        SLP* o[1] = {&proj_cat};
        floatX* yo[1] = {bx};
        return f->Group(ba, nullptr, 0.0f, n, q_dim, nullptr, 1, o, yo, bx);
    }
    KF_TRY(kf_rmsnorm(c, bx, ToX(norm.w), bn, n, C, norm.rms_eps, nullptr));
    if (f->kv_int8) {  // int8 KV cache: the batch's K / V rows into the staging pair, quantised into the cache, then rows 0 .. pos0 + n - 1 dequantised over the staging
                       // pair -- every key, the batch's own included, is attended in its dequantised form -- and the existing prompt attention on the staging pair
        floatX *sk = ToX(hCache->stage_k), *sv = ToX(hCache->stage_v);
        int8_t *k8 = hCache->Codes(KVCache::KV_KEY, L), *v8 = hCache->Codes(KVCache::KV_VAL, L);
        float *ks = hCache->Steps(KVCache::KV_KEY, L), *vs = hCache->Steps(KVCache::KV_VAL, L);
        KF_TRY(kf_qkv_rope_batch(c, &wq, &wk, &wv, bn, bq, sk + (size_t)pos0 * kv_dim, sv + (size_t)pos0 * kv_dim, n, normQ.w ? ToX(normQ.w) : nullptr,
                                 normK.w ? ToX(normK.w) : nullptr, f->rope_table, pos0, n_head, n_head_kv, head_dim, normQ.rms_eps));
        KF_TRY(kf_kv8_quant_rows(c, sk + (size_t)pos0 * kv_dim, sv + (size_t)pos0 * kv_dim, kv_dim, n, n_head_kv, head_dim, k8, v8, ks, vs, pos0, kv_dim));
        f->kv8_count[f->kv_int8_prefill ? 0 : 1]++;
        if (f->kv_int8_prefill) {  // the prompt form: the int8 rows themselves, integer scores as the decode kernel's; nothing is dequantised, no earlier row is rewritten
            KF_TRY(kf_attn_prefill_kv8(c, bq, k8, v8, ks, vs, ba, pos0, n, q_dim, n_head, n_head_kv, head_dim, kv_dim));
            return kf_linear(c, &wo, ba, bx, nullptr, n, 1.0f, 0.0f, KF_EPI_RESIDUAL, bx);
        }
        KF_TRY(kf_kv8_dequant_rows(c, k8, v8, ks, vs, pos0 + n, n_head_kv, head_dim, kv_dim, sk, sv, kv_dim));
        KF_TRY(kf_attn_prefill(c, bq, sk, sv, ba, pos0, n, q_dim, n_head, n_head_kv, head_dim, kv_dim));
        return kf_linear(c, &wo, ba, bx, nullptr, n, 1.0f, 0.0f, KF_EPI_RESIDUAL, bx);
    }
    KF_TRY(kf_qkv_rope_batch(c, &wq, &wk, &wv, bn, bq, krows, vrows, n, normQ.w ? ToX(normQ.w) : nullptr, normK.w ? ToX(normK.w) : nullptr, f->rope_table, pos0, n_head, n_head_kv,
                             head_dim, normQ.rms_eps));
    KF_TRY(kf_attn_prefill(c, bq, key_cache, val_cache, ba, pos0, n, q_dim, n_head, n_head_kv, head_dim, kv_dim));
    return kf_linear(c, &wo, ba, bx, nullptr, n, 1.0f, 0.0f, KF_EPI_RESIDUAL, bx);
}

int FFN::cuFlow(floatX* bx, int n) {
    Fish* f = hFish;
    kf_ctx* c = f->ctx;
    const int C = f->config.nEmbed;
    floatX *bn = ToX(f->gBUFF.bNorm), *bg = ToX(f->gBUFF.bGate), *bu = ToX(f->gBUFF.bUp);
    kf_weight wg = gate.w->desc(), wu = up.w->desc(), wd = down.w->desc();
    if (f->EagerOnly()) {
        SLP* gu[2] = {&gate, &up};
        floatX* ys[2] = {bg, bu};
        KF_TRY(f->Group(bx, ToX(norm.w), norm.rms_eps, n, C, bn, 2, gu, ys, nullptr));
        KF_TRY(kf_swiglu(c, bg, bu, bg, n * latent));
        SLP* d[1] = {&down};
        floatX* yd[1] = {bx};
        return f->Group(bg, nullptr, 0.0f, n, latent, nullptr, 1, d, yd, bx);
    }
    KF_TRY(kf_rmsnorm(c, bx, ToX(norm.w), bn, n, C, norm.rms_eps, nullptr));
    KF_TRY(kf_gateup_swiglu_batch(c, &wg, &wu, bn, bg, bu, n));
    if (n_hot >= 0) KF_TRY(kf_zero_cold_columns(c, bg, reinterpret_cast<const int32_t*>(hot_mask->data), n, wg.ne0));  // D_matmul_sparse for every token row, as cuInfer
    return kf_linear(c, &wd, bg, bx, nullptr, n, 1.0f, 0.0f, KF_EPI_RESIDUAL, bx);
}

hGTensor TokenEmbed::cuInfer(int token, int) {
    Fish* f = hFish;
    kf_weight wd = w->desc();
    int rc = (f->graph_mode || f->state_tokens) ? kf_embed_state(f->ctx, &wd, f->d_state, f->d_forced, ToX(out)) : kf_embed(f->ctx, &wd, token, nullptr, ToX(out));
    return rc == KF_OK ? out : nullptr;
}

hGTensor Head4Token::cuInfer_1(hGTensor inp_, int) {
    Fish* f = hFish;
    kf_weight wd = proj.w->desc();
    int rc;
    if (f->fuse_level == 0 && !f->state_tokens) {
        hGTensor xn = f->final_norm.cuFlow(inp_);
        if (!xn) return nullptr;
        rc = kf_lm_head(f->ctx, &wd, ToX(xn), ToX(preLogits), f->d_state + 2, f->gBUFF.head_ws->data);
    } else {
        rc = f->HeadAndPick(ToX(inp_));
    }
    return rc == KF_OK ? preLogits : nullptr;
}

// ------------------------------------------------------------------------------------------------ Fish
// Only what has an order: graphs and engine before the workspace and head screen they point into; the IPC mappings (no allocations) closed.  The context goes last.
Fish::~Fish() {
    DropGraphs(), tp.group_graphs.clear(), engine.reset();
    if (ctx)
        for (void* p : tp.opened) kf_tp_ipc_close(ctx, p);
}

bool Fish::ShapeServed(const MODEL_CARD& c, std::string& why) {
    const int gq = c.n_head_kv > 0 ? c.n_head / c.n_head_kv : 0;
    if (c.n_head_kv <= 0 || c.n_head % c.n_head_kv != 0 || !(gq == 1 || gq == 2 || gq == 4 || gq == 8)) {
        why = "query heads per kv head = " + std::to_string(c.n_head) + " / " + std::to_string(c.n_head_kv) + " (served: 1, 2, 4, 8)";
        return false;
    }
    if (c.head_dim != 64 && c.head_dim != 128) {
        why = "head_dim " + std::to_string(c.head_dim) + " (served: 64, 128)";
        return false;
    }
    if (c.nEmbed % 8 != 0 || c.n_ff % 8 != 0) {
        why = "hidden / intermediate size must be a multiple of 8";
        return false;
    }
    return true;
}
static thread_local std::string g_host_err;
int Fish::Build(const MODEL_CARD& card, int device, void* stream) {
    if (!ShapeServed(card, g_host_err)) {
        g_host_err = "Fish::Build: " + g_host_err;
        return KF_UNSUPPORTED_DATATYPE;
    }
    config = card;
    KF_TRY(kf_init(device, stream, &ctx));
    const int C = card.nEmbed, hd = card.head_dim, qd = card.n_head * hd, kvd = card.n_head_kv * hd;
    KF_TRY(cache.Init(ctx, card.nLayer, card.n_ctx, kvd));
    x = GT(ctx, "x", typNUMBER::BF16, C);
    gBUFF.tmpFF1 = GT(ctx, "tmpFF1", typNUMBER::BF16, qd);
    gBUFF.kraw = GT(ctx, "kraw", typNUMBER::BF16, kvd);
    gBUFF.scratch = GT(ctx, "scratch", typNUMBER::BF16, std::max(std::max(qd, C), card.n_ff));
    gBUFF.delta = GT(ctx, "delta", typNUMBER::BF16, C);
    gBUFF.upOut = GT(ctx, "upOut", typNUMBER::BF16, card.n_ff);
    gBUFF.normed = GT(ctx, "normed", typNUMBER::BF16, C);
    gBUFF.attn_ws = GT(ctx, "attn_ws", typNUMBER::F32, (int)(kf_attn_scratch_bytes(card.n_head, hd) / 4));
    gBUFF.head_ws = GT(ctx, "head_ws", typNUMBER::F32, (int)(kf_head_scratch_bytes() / 4));
    if (!x || !gBUFF.tmpFF1 || !gBUFF.kraw || !gBUFF.scratch || !gBUFF.delta || !gBUFF.upOut || !gBUFF.normed || !gBUFF.attn_ws || !gBUFF.head_ws)
        return KF_OUTOF_GPUMEMORY;
    // RoPE (cos,sin) table on the host libm, uploaded once
    {
        std::vector<float> tab((size_t)card.n_ctx * hd);
        KF_TRY(kf_rope_table_host(tab.data(), card.n_ctx, hd, card.rope_theta));
        KF_TRY(rope_table.Alloc(ctx, tab.size() * 4));
        KF_TRY(kf_h2d(ctx, rope_table, tab.data(), tab.size() * 4));
    }
    KF_TRY(Commit<SeqBuffers>(*this, ctx, 1, card.n_ctx, 0xff));

    embed.hFish = this, embed.name = "embed_tokens", embed.out = x;
    for (int l = 0; l < card.nLayer; l++) {
        auto a = std::make_unique<SelfAttention>();
        a->hFish = this, a->layid = l + 1, a->name = "layers." + std::to_string(l) + ".self_attn";
        a->n_head = card.n_head, a->n_head_kv = card.n_head_kv, a->head_dim = hd, a->q_dim = qd, a->kv_dim = kvd;
        a->hCache = &cache, a->out = x;
        a->norm.hFish = this, a->norm.ldTH = C, a->norm.rms_eps = card.rms_eps, a->norm.out = gBUFF.normed;
        a->normQ.hFish = a->normK.hFish = this, a->normQ.nHead = card.n_head, a->normK.nHead = card.n_head_kv;
        a->normQ.ldTH = a->normK.ldTH = hd, a->normQ.rms_eps = a->normK.rms_eps = card.qk_eps;
        for (SLP* s : {&a->Q, &a->K, &a->V, &a->proj_cat}) s->hFish = this;
        a->Q.out = gBUFF.tmpFF1, a->Q.nIn = C, a->Q.nOut = qd;
        a->rope.hFish = this, a->rope.hnQ = &a->normQ, a->rope.hnK = &a->normK;
        a->rope.n_head = card.n_head, a->rope.n_head_kv = card.n_head_kv, a->rope.head_dim = hd, a->rope.theta = card.rope_theta;
        attn.push_back(std::move(a));
        auto m = std::make_unique<FFN>();
        m->hFish = this, m->layid = l + 1, m->name = "layers." + std::to_string(l) + ".mlp", m->latent = card.n_ff, m->out = x;
        m->norm.hFish = this, m->norm.ldTH = C, m->norm.rms_eps = card.rms_eps, m->norm.out = gBUFF.normed;
        for (SLP* s : {&m->gate, &m->up, &m->down}) s->hFish = this;
        m->relu.hFish = this;
        ffn.push_back(std::move(m));
    }
    final_norm.hFish = this, final_norm.ldTH = C, final_norm.rms_eps = card.rms_eps, final_norm.out = gBUFF.normed;
    head.hFish = this, head.proj.hFish = this;
    head.preLogits = GT(ctx, "preLogits", typNUMBER::BF16, card.vocab);
    return head.preLogits ? KF_OK : KF_OUTOF_GPUMEMORY;
}

// ---- the modes (kf_host_modes.hpp)
unsigned Fish::Modes() const {
    return (tp.world > 1 ? mode_bit(MODE_TP) : 0u) | (act_int8 ? mode_bit(MODE_ACT_INT8) : 0u) | (n_adapters > 0 ? mode_bit(MODE_ADAPTERS) : 0u) |
           (kv_int8 ? mode_bit(MODE_KV_INT8) : 0u) | (masked_layers > 0 ? mode_bit(MODE_HOT_MASK) : 0u) | (fuse_level == 0 ? mode_bit(MODE_FUSE0) : 0u);
}
void Fish::ModeChanged() {
    DropEngineTable(); /* the captured graphs and the engine's table belong to the other arithmetic (or hold the old masks) */
    weights_gen++;     /* XcdReplicas / XcdTP built on this Fish re-check at their next use */
}
// a setter's own refusal: "<entry>: <msg>" into why, rc back
static int refused(std::string& why, const char* entry, int rc, const std::string& msg) {
    why = std::string(entry) + ": " + msg;
    return rc;
}
std::array<SLP*, 7> Fish::LayerMatrices(int l) const {
    SelfAttention* a = attn[l].get();
    FFN* m = ffn[l].get();
    return {&a->Q, &a->K, &a->V, &a->proj_cat, &m->gate, &m->up, &m->down};
}
static bool is_row3(const hGTensor& t) { return t && t->quant.isNormalFloat && t->type == typNUMBER::Q3; }
static const char* kRow3Why = "a layer matrix is a 3-bit row codebook (NF3): such layers run on the per-layer launches (kf_set_row_unpack), not in this path";
bool Fish::HasRow3() const {
    for (int l = 0; l < config.nLayer; l++)
        for (const SLP* s : LayerMatrices(l))
            if (is_row3(s->w)) return true;
    return false;
}
SLP* Fish::LayerMatrix(int layer, int slot) const { return layer >= 0 && layer < config.nLayer && slot >= 0 && slot < 7 ? LayerMatrices(layer)[slot] : nullptr; }

// ---- int8 activations (kfh_set_act_int8, kfh_set_act_int8_q4)
static const char* kf_last_error_hint(int st) {
    return st == KF_QUANT_ERR ? "groups of 128 weights with their gama are required" : st == KF_BLAS_UNALIGN ? "data not 16-byte aligned" : "rows must be whole 128-weight groups";
}
// a matrix takes int8 activations unless kf::a8_plan (asked through kf_linear_a8_status: the one served-storage rule) says its storage has no integer form
static bool a8_type(const kf_weight& w) { return kf_linear_a8_status(&w, 1) != KF_UNSUPPORTED_DATATYPE; }
int Fish::A8Ready(int rows) {
    if (a8.q && a8.rows >= rows) return KF_OK;
    KF_TRY(kf_sync(ctx));
    a8 = A8Rows(); /* the old rows go first (they can be large): a refusal below leaves the set empty, rows 0 */
    return Commit(a8, ctx, rows, (size_t)std::max(std::max(config.n_head * config.head_dim, config.nEmbed), config.n_ff));
}
// where a matrix goes in a batch of n token rows: 2 = kf_linear_w4a8(_tiles), 1 = kf_linear_a8(_tiles), 0 = kf_rmsnorm + kf_linear (every matrix while both switches are off)
int Fish::A8Route(const kf_weight& w, int n) const {
    if (act_int8_q4 && kf_linear_w4a8_status(&w, n) == KF_OK) return 2; /* asked with the batch's n: the plan's LDS bound depends on it, and a refused matrix keeps kf_linear */
    return (act_int8_t && a8_type(w)) ? 1 : 0;
}
int Fish::Group(const floatX* x, const floatX* norm_w, float eps, int n, int dim, floatX* normed, int n_w, SLP* const* s, floatX* const* y, const floatX* residual) {
    bool any8 = false, other = false;
    kf_weight wd[3];
    int route[3];
    for (int i = 0; i < n_w; i++) wd[i] = s[i]->w->desc(), route[i] = A8Route(wd[i], n), (route[i] ? any8 : other) = true;
    if (any8) {
        KF_TRY(A8Ready(n));
        KF_TRY(kf_act_quant_i8(ctx, x, dim, norm_w, eps, n, dim, a8.q, a8.step));
    }
    const floatX* xb = x;
    if (other && norm_w) {
        KF_TRY(kf_rmsnorm(ctx, x, norm_w, normed, n, dim, eps, nullptr));
        xb = normed;
    }
    const floatX *a[3], *b[3];
    floatX* ya[3];
    int OC[3], na = 0;
    for (int i = 0; i < n_w; i++) {
        const floatX* bias = s[i]->b ? ToX(s[i]->b) : nullptr;
        if (route[i]) {
            const bool tiles = n > 1 && a8_tile_min >= 0 && n >= a8_tile_min; /* n = 1 (decode) always takes the mat-vec */
            static constexpr decltype(&kf_linear_a8) entry[2][2] = {{kf_linear_a8, kf_linear_a8_tiles}, {kf_linear_w4a8, kf_linear_w4a8_tiles}}; /* [A8Route - 1][tiles] */
            KF_TRY(entry[route[i] - 1][tiles](ctx, &wd[i], a8.q, a8.step, y[i], bias, residual, n));
            a8_count[tiles ? 0 : 1]++;
        } else
            KF_TRY(kf_linear(ctx, &wd[i], xb, y[i], bias, n, 1.0f, 0.0f, residual ? KF_EPI_RESIDUAL : KF_EPI_NONE, residual));
        if (s[i]->lora_a) a[na] = s[i]->lora_a, b[na] = s[i]->lora_b, ya[na] = y[i], OC[na] = wd[i].ne0, na++;
    }
    if (na == 0) return KF_OK;
    if (n == 1) return kf_lora_apply(ctx, na, a, b, lora_r, OC, dim, xb, ya, nullptr, 1, lora_s); /* the group's adapters share the row: one launch */
    for (int i = 0; i < na; i++) KF_TRY(kf_lora_apply(ctx, 1, a + i, b + i, lora_r, OC + i, dim, xb, ya + i, nullptr, n, lora_s));
    return KF_OK;
}
int Fish::SetActInt8(bool q4, bool on, std::string& why) {
    const char* entry = q4 ? "kfh_set_act_int8_q4" : "kfh_set_act_int8";
    if (on) {
        KF_TRY(Admit(MODE_ACT_INT8, entry, why));
        int served = 0;
        std::vector<uint16_t> zero;
        for (int l = 0; l < config.nLayer; l++)
            for (SLP* s : LayerMatrices(l)) {
                if (!s->w) return refused(why, entry, KF_INVALID_ARGS, "a layer matrix is missing");
                const kf_weight w = s->w->desc();
                if (q4) { /* the group ZERO is part of this arithmetic: no zero check */
                    served += kf_linear_w4a8_status(&w, 1) == KF_OK;
                    continue;
                }
                if (!a8_type(w)) continue;
                if (const int st = kf_linear_a8_status(&w, 1))
                    return refused(why, entry, st, "layer " + std::to_string(l) + ": kf_linear_a8 refuses a ternary / 1-bit matrix with " + std::to_string(st) + " (" + kf_last_error_hint(st) + ")");
                zero.resize(w.nGroup);
                KF_TRY(kf_d2h(ctx, zero.data(), w.gama + w.ne0 + w.ne1, (size_t)w.nGroup * 2)); /* gama_T(ZERO) */
                for (uint16_t z : zero)
                    if (z & 0x7fff)
                        return refused(why, entry, KF_QUANT_ERR, "layer " + std::to_string(l) + ": a group zero is not 0 -- the integer product has no zero point (YinYang and the symmetric quantiser write 0)");
                served++;
            }
        if (!served)
            return refused(why, entry, KF_UNSUPPORTED_DATATYPE,
                           q4 ? "no layer matrix is 4-bit group storage that kf_linear_w4a8 serves (KF_Q4, groups of 128 with gama, qBias 0 or 8): nothing would take int8 activations"
                              : "no layer matrix is ternary (KF_T_SIGN) or 1-bit (KF_BOOL1 / KF_T_BINARY): nothing would take int8 activations");
        KF_TRY(A8Ready(1));
        a8_count[0] = a8_count[1] = 0;
    }
    const bool was = act_int8;
    (q4 ? act_int8_q4 : act_int8_t) = on;
    act_int8 = act_int8_t || act_int8_q4;
    if (act_int8 != was) ModeChanged();
    return KF_OK;
}

// ---- int8 KV cache (kfh_set_kv_int8)
int Fish::SetKVInt8(bool on, std::string& why) {
    if (on) {
        KF_TRY(Admit(MODE_KV_INT8, "kfh_set_kv_int8", why));
        if (const int st = kf_attn_block_kv8_status(config.n_head, config.n_head_kv, config.head_dim))
            return refused(why, "kfh_set_kv_int8", st,
                           "kf_attn_block_kv8 refuses " + std::to_string(config.n_head) + " / " + std::to_string(config.n_head_kv) + " heads x " + std::to_string(config.head_dim));
        if (!cache.k8) KF_TRY(kf_sync(ctx)); /* never inside a launch sequence */
        KF_TRY(cache.Init8(ctx, config.n_head_kv));
        if (!gBUFF.vraw) gBUFF.vraw = GT(ctx, "vraw", typNUMBER::BF16, config.n_head_kv * config.head_dim);
        if (!gBUFF.vraw) return KF_OUTOF_GPUMEMORY;
    }
    if (kv_int8 != on) {
        kv_int8 = on;
        if (!on) kv_int8_prefill = false; /* the sub-setting goes with the cache */
        ModeChanged();
    }
    return KF_OK;
}
int Fish::SetKVInt8Prefill(bool on, std::string& why) {
    if (on) {
        if (!kv_int8)
            return refused(why, "kfh_set_kv_int8_prefill", KF_INVALID_ARGS, "the int8 prompt attention is a sub-setting of the int8 KV cache: switch kfh_set_kv_int8 on first");
        if (const int st = kf_attn_prefill_kv8_status(config.n_head, config.n_head_kv, config.head_dim, 1))
            return refused(why, "kfh_set_kv_int8_prefill", st,
                           "kf_attn_prefill_kv8 refuses " + std::to_string(config.n_head) + " / " + std::to_string(config.n_head_kv) + " heads x " + std::to_string(config.head_dim));
    }
    if (kv_int8_prefill != on) {
        kv_int8_prefill = on;
        ModeChanged(); /* as kfh_set_kv_int8: captured graphs dropped, XcdReplicas / XcdTP built on this Fish re-check */
    }
    return KF_OK;
}

// ---- low-rank adapters at inference (kfh_set_adapter / kfh_clear_adapters)
int Fish::SetAdapter(int layer, int slot, const floatX* a, const floatX* b, int r, float s, std::string& why) {
    const char* entry = "kfh_set_adapter";
    SLP* m = LayerMatrix(layer, slot);
    if (!m || !m->w || !a || !b)
        return refused(why, entry, KF_INVALID_ARGS,
                       "adapters: no such layer matrix (layer " + std::to_string(layer) + ", slot " + std::to_string(slot) + "), its weight is not set, or a null pointer");
    KF_TRY(Admit(MODE_ADAPTERS, entry, why));
    if (!std::isfinite(s)) return refused(why, entry, KF_INVALID_ARGS, "adapters: s is not finite");
    if (n_adapters - (m->lora_a ? 1 : 0) > 0 && (r != lora_r || s != lora_s)) /* another matrix carries one already */
        return refused(why, entry, KF_INVALID_ARGS, "adapters: one rank and one s per model (attached: rank " + std::to_string(lora_r) + ")");
    if (const int st = kf_lora_apply_status(r, m->nOut, m->nIn, 1, 1))
        return refused(why, entry, st,
                       "adapters: kf_lora_apply refuses rank " + std::to_string(r) + " beside a " + std::to_string(m->nOut) + " x " + std::to_string(m->nIn) +
                           " matrix (rank 16, 32 or 64; sides multiples of 64 and >= 128)");
    if (((uintptr_t)a | (uintptr_t)b) & 15) return refused(why, entry, KF_BLAS_UNALIGN, "adapters: a and b must be 16-byte aligned");
    if (!m->lora_a) n_adapters++;
    m->lora_a = a, m->lora_b = b, lora_r = r, lora_s = s;
    ModeChanged();
    return KF_OK;
}
void Fish::ClearAdapters() {
    if (!n_adapters) return;
    for (int l = 0; l < config.nLayer; l++)
        for (SLP* m : LayerMatrices(l)) m->lora_a = m->lora_b = nullptr;
    n_adapters = 0, lora_r = 0, lora_s = 0.0f;
    ModeChanged();
}

// position buckets: one captured graph each; the bound fixes the attention slice count of that graph
static const int kBuckets[] = {64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072};
static int bucket_of(int pos) {
    int i = 0;
    while (kBuckets[i] <= pos) i++;
    return i;
}
int Fish::pos_bound() const {
    int b = kBuckets[bucket_of(tok_pos)] - 1;
    return b < config.n_ctx - 1 ? b : config.n_ctx - 1;
}

int Fish::GrowScratch(size_t need) {
    if (need <= lin_scratch.bytes()) return KF_OK;
    KF_TRY(kf_sync(ctx));
    DevBuf<> p; /* the old block stays the context's scratch until the new one is accepted */
    KF_TRY(p.Alloc(ctx, need));
    KF_TRY(kf_set_scratch(ctx, p, need));
    lin_scratch = std::move(p);
    return KF_OK;
}

int Fish::EngineTable(floatX* kbase, floatX* vbase, bool masks, std::string& why, std::vector<kf_engine_layer>& L, kf_engine_desc& d) const {
    const size_t layer_rows = (size_t)config.n_ctx * config.n_head_kv * config.head_dim;
    L.assign(config.nLayer, kf_engine_layer{});
    for (int l = 0; l < config.nLayer; l++) {
        SelfAttention* a = attn[l].get();
        FFN* m = ffn[l].get();
        const auto s = LayerMatrices(l);
        for (int j = 0; j < 7; j++) {
            if (!s[j]->w || s[j]->b) {
                why = "a layer matrix is missing or carries a bias";
                return KF_ENGINE_NOT_SERVED;
            }
            if (is_row3(s[j]->w)) { /* the engines (persistent and XCD) serve group-quantised storage */
                why = kRow3Why;
                return KF_ENGINE_NOT_SERVED;
            }
            L[l].w[j] = s[j]->w->desc();
        }
        if (!a->norm.w || !m->norm.w || (!masks && m->n_hot >= 0)) {
            why = masks ? "a norm weight is missing" : "a norm weight is missing or a hot-row mask is set";
            return KF_ENGINE_NOT_SERVED;
        }
        L[l].hot_ffn = m->n_hot >= 0 ? reinterpret_cast<const int32_t*>(m->hot_mask->data) : nullptr; /* the sparse forward inside the launch: cold gate / up rows never read, zeros published */
        L[l].norm_in = ToX(a->norm.w), L[l].norm_post = ToX(m->norm.w);
        L[l].q_norm = a->normQ.w ? ToX(a->normQ.w) : nullptr, L[l].k_norm = a->normK.w ? ToX(a->normK.w) : nullptr;
        L[l].kcache = kbase + l * layer_rows, L[l].vcache = vbase + l * layer_rows;
    }
    std::memset(&d, 0, sizeof(d));
    d.n_layer = config.nLayer, d.dim = config.nEmbed, d.n_head = config.n_head, d.n_kv = config.n_head_kv, d.head_dim = config.head_dim, d.ffn = config.n_ff;
    d.kv_stride = config.n_head_kv * config.head_dim;
    d.max_seq = config.n_ctx;
    d.rms_eps = config.rms_eps, d.qk_eps = config.qk_eps, d.rope_table = rope_table, d.layers = L.data();
    return KF_OK;
}

// The persistent decode engine over this model's layers: built on first use (every weight must be set), not while capturing.
int Fish::EnsureEngine() {
    if (engine_state != 0) return engine_state > 0 ? KF_OK : KF_ENGINE_NOT_SERVED;
    engine_state = -1;
    KF_TRY(EngineRefusal(engine_why));
    std::vector<kf_engine_layer> L;
    kf_engine_desc d;
    KF_TRY(EngineTable(ToX(cache.key), ToX(cache.val), true, engine_why, L, d));
    {
        char why[320];
        why[0] = 0;
        const int served = kf_engine_served(ctx, &d, why, sizeof(why));
        engine_why = why;
        if (served != KF_OK) return KF_ENGINE_NOT_SERVED;
    }
    const size_t bytes = kf_engine_workspace_bytes(&d);
    DevBuf<> ws;
    kf_engine* e = nullptr;
    if (ws.Alloc(ctx, bytes) != KF_OK) return KF_OUTOF_GPUMEMORY;
    if (kf_engine_create(ctx, &d, ws, bytes, &e) != KF_OK) return KF_ENGINE_NOT_SERVED;
    engine.reset(e), engine_ws = std::move(ws);
    engine_state = 1;
    // a bf16 embedding table is read inside the launch (graph-mode steps): one launch less per token; other storages keep kf_embed_state
    kf_weight we = embed.w->desc();
    engine_embed = kf_engine_set_embedding(ctx, engine.get(), &we, d_forced) == KF_OK;
    // final norm + bf16 LM head + greedy pick as trailing phases of the same launch (other head storages keep kf_norm_lm_head)
    engine_head = false;
    if (head.proj.w && final_norm.w && head.preLogits && final_norm.rms_eps == config.rms_eps) {
        kf_weight wh = head.proj.w->desc();
        engine_head = kf_engine_set_head(ctx, engine.get(), &wh, ToX(final_norm.w), ToX(head.preLogits), d_tokens_out) == KF_OK;
    }
    return KF_OK;
}
// the int8 screen of the engine's head, under the caller's promise only; no room or a refusal is not an error: every step then streams the bf16 head
void Fish::EnsureHeadScreen() {
    if (head_screen || head_screen_tried || !prefill_resident || !engine || !engine_head) return;
    head_screen_tried = true;
    const kf_weight wh = head.proj.w->desc();
    const size_t bytes = kf_engine_head_screen_bytes(wh.ne0, wh.ne1);
    if (bytes == 0 || bytes + deq_arena.bytes() > resident_max_bytes) return;
    DevBuf<> p;
    if (p.Alloc(ctx, bytes) != KF_OK || kf_engine_set_head_screen(ctx, engine.get(), p, bytes) != KF_OK) return;
    head_screen = std::move(p);
}
void Fish::DropHeadScreen() {
    if (head_screen) {
        kf_sync(ctx);
        if (engine) kf_engine_set_head_screen(ctx, engine.get(), nullptr, 0);
        head_screen.Free();
    }
    head_screen_tried = false;
}
void Fish::DropEngineTable() {
    DropGraphs();
    DropHeadScreen();
    if (engine) {
        kf_sync(ctx); /* the deleter does not: a launch may still be running */
        engine.reset();
    }
    engine_ws.Free();
    engine_state = 0, engine_embed = engine_head = false;
}
void Fish::DropEngine() {
    weights_gen++; /* what XcdReplicas / XcdTP objects built on this Fish compare their own copy with */
    DropEngineTable();
    bucket_tuned.clear(); /* the measured delays belonged to that engine */
    DropResident(); /* the resident bf16 copies are keyed by the old tensors' addresses too */
}
void Fish::DropResident() {
    if (deq_arena) {
        kf_sync(ctx);
        kf_set_dequant_arena(ctx, nullptr, 0);
        deq_arena.Free();
    }
    resident_tried = false;
}
// Resident bf16 copies of the layers' quantised matrices for long prompts (kf_set_dequant_arena): 2 bytes per weight -- 0.9 GB for Qwen3-0.6B, 62 GB for Qwen3-32B -- of a
// 288 GB part, instead of five dequantise launches per layer and prompt.  Sized and allocated by the first Prefill after the weights were set (never inside a launch
// sequence); skipped when the copies would not fit `resident_max_bytes` or the allocation fails (the per-call scratch route stays).
int Fish::EnsureResident(int PC) {
    if (deq_arena || resident_tried || !prefill_resident || PC < 1024) return KF_OK;
    resident_tried = true;
    size_t total = 0;
    for (int l = 0; l < config.nLayer; l++)
        for (const SLP* s : LayerMatrices(l)) {
            if (!s->w) continue;
            const kf_weight d = s->w->desc();
            if (d.type != KF_BF16 && d.quant == KF_QUANT_GROUP && !d.qzeros) total += ((size_t)d.ne0 * d.ne1 * 2 + 255) & ~(size_t)255;
        }
    if (total == 0 || total + head_screen.bytes() > resident_max_bytes) return KF_OK;
    KF_TRY(kf_sync(ctx));
    DevBuf<> p;
    if (p.Alloc(ctx, total) != KF_OK) return KF_OK; /* no room: not an error, the scratch route serves */
    KF_TRY(kf_set_dequant_arena(ctx, p, total));
    deq_arena = std::move(p);
    return GrowScratch(kf_resident_scratch_bytes()); /* the scratch holds no dequantised copy any more: it lends the small tile kernels their split-K slots */
}
int Fish::EngineCheck() {
    if (!engine || engine_steps == 0) return KF_OK;
    const int rc = kf_engine_check(ctx, engine.get());
    if (rc == KF_INTERNAL_ERR) { /* the word latches: every launch since the failure was a no-op.  Report it once, start over from a clean hand-off state */
        DropGraphs();
        kf_engine_reset(ctx, engine.get());
    }
    return rc;
}

// ------------------------------------------------------------------------------------------------ tensor parallel
int Fish::TPInit(int rank, int world, int vocab_row0) {
    if (world < 2 || world > 8 || rank < 0 || rank >= world) return KF_INVALID_ARGS;
    KF_TRY(Admit(MODE_TP, "kfh_tp_init", g_host_err));
    std::memset(&tp.comm, 0, sizeof(tp.comm));
    tp.rank = rank, tp.world = world, tp.vocab_row0 = vocab_row0;
    tp.comm.rank = rank, tp.comm.world = world, tp.comm.n_max = config.nEmbed, tp.comm.per_step = 2u * (uint32_t)config.nLayer + 1u;
    const size_t bytes = kf_tp_recv_bytes(world, config.nEmbed);
    const size_t pbytes = kf_tp_push_bytes(tp.comm.per_step);
    KF_TRY(tp.area.AllocUncached(ctx, bytes + 64 + pbytes)); /* + the generation and error words and the push descriptors behind the area */
    tp.comm.d_push = tp.area + bytes + 64;
    tp.comm.recv = tp.area, tp.comm.peer[rank] = tp.area;
    tp.comm.d_step = reinterpret_cast<uint32_t*>(tp.area + bytes);
    tp.comm.d_err = reinterpret_cast<int32_t*>(tp.area + bytes + 32);
    use_engine = false; /* the persistent engine serves whole layers of one GPU */
    return KF_OK;
}
int Fish::TPSetPeer(int r, void* area) {
    if (tp.world < 2 || r < 0 || r >= tp.world || !area) return KF_INVALID_ARGS;
    tp.comm.peer[r] = area;
    tp.committed = false;
    return KF_OK;
}
int Fish::TPCommit() { /* the push descriptors are written once, when every peer's area is known (never inside a capture) */
    if (tp.committed || tp.world < 2) return KF_OK;
    for (int r = 0; r < tp.world; r++)
        if (!tp.comm.peer[r]) return KF_INVALID_ARGS;
    KF_TRY(kf_tp_commit(ctx, &tp.comm));
    tp.committed = true;
    return KF_OK;
}
int Fish::TPPhase(int phase, int l) {
    KF_TRY(TPCommit());
    const int32_t* d_pos = graph_mode ? d_state + 1 : nullptr;
    const int bound = graph_mode ? pos_bound() : tok_pos;
    const int C = config.nEmbed;
    switch (phase) {
        case 0: return embed.cuInfer(-1) ? KF_OK : KF_INTERNAL_ERR;
        case 1: {  // [norm + q,k,v rows of this rank] -> [q/k-norm + RoPE + attention over the local kv heads] -> o_proj column shard, pushed
            SelfAttention* a = attn[l].get();
            floatX* key_cache = reinterpret_cast<floatX*>(cache.Get(KVCache::KV_KEY, l, 0));
            floatX* val_cache = reinterpret_cast<floatX*>(cache.Get(KVCache::KV_VAL, l, 0));
            kf_weight wq = a->Q.w->desc(), wk = a->K.w->desc(), wv = a->V.w->desc(), wo = a->proj_cat.w->desc();
            const kf_weight* ws[3] = {&wq, &wk, &wv};
            kf_bf16* ys[3] = {ToX(a->Q.out), ToX(gBUFF.kraw), val_cache};
            const int64_t strides[3] = {0, 0, (int64_t)a->kv_dim};
            KF_TRY(kf_norm_linear(ctx, ToX(x), ToX(a->norm.w), a->norm.rms_eps, 3, ws, ys, strides, bound, d_pos));
            KF_TRY(kf_attn_block(ctx, ToX(a->Q.out), ToX(gBUFF.kraw), key_cache, val_cache, ToX(gBUFF.scratch), a->normQ.w ? ToX(a->normQ.w) : nullptr,
                                 a->normK.w ? ToX(a->normK.w) : nullptr, rope_table, bound, d_pos, a->n_head, a->n_head_kv, a->head_dim, a->kv_dim, a->normQ.rms_eps,
                                 gBUFF.attn_ws->data));
            return kf_linear_f32_push(ctx, &wo, ToX(gBUFF.scratch), &tp.comm, 2u * (uint32_t)l);
        }
        case 2: return kf_tp_reduce_recv(ctx, &tp.comm, 2u * (uint32_t)l, C, ToX(x), ToX(x));
        case 3: {
            FFN* m = ffn[l].get();
            kf_weight wg = m->gate.w->desc(), wu = m->up.w->desc(), wd = m->down.w->desc();
            KF_TRY(kf_norm_gateup_swiglu(ctx, ToX(x), ToX(m->norm.w), m->norm.rms_eps, &wg, &wu, ToX(gBUFF.scratch)));
            return kf_linear_f32_push(ctx, &wd, ToX(gBUFF.scratch), &tp.comm, 2u * (uint32_t)l + 1u);
        }
        case 4: return kf_tp_reduce_recv(ctx, &tp.comm, 2u * (uint32_t)l + 1u, C, ToX(x), ToX(x));
        case 5: {
            kf_weight wh = head.proj.w->desc();
            return kf_tp_lm_head(ctx, ToX(x), ToX(final_norm.w), final_norm.rms_eps, &wh, ToX(head.preLogits), tp.vocab_row0, &tp.comm, gBUFF.head_ws->data);
        }
        case 6: return kf_tp_pick(ctx, &tp.comm, d_state, d_tokens_out);
    }
    return KF_INVALID_ARGS;
}
int Fish::EnqueueStepTP() {
    KF_TRY(TPPhase(0, 0));
    for (int l = 0; l < config.nLayer; l++)
        for (int ph = 1; ph <= 4; ph++) KF_TRY(TPPhase(ph, l));
    KF_TRY(TPPhase(5, 0));
    return TPPhase(6, 0);
}
// ranks of one process on one stream: phase by phase across the ranks
static int tp_group_enqueue(Fish** fs, int R) {
    for (int r = 0; r < R; r++) KF_TRY(fs[r]->TPPhase(0, 0));
    for (int l = 0; l < fs[0]->config.nLayer; l++)
        for (int ph = 1; ph <= 4; ph++)
            for (int r = 0; r < R; r++) KF_TRY(fs[r]->TPPhase(ph, l));
    for (int r = 0; r < R; r++) KF_TRY(fs[r]->TPPhase(5, 0));
    for (int r = 0; r < R; r++) KF_TRY(fs[r]->TPPhase(6, 0));
    return KF_OK;
}

int Fish::LayersAndHead(hGTensor cur) {
    for (int l = 0; l < config.nLayer && cur; l++) {
        cur = attn[l]->cuInfer(cur);
        if (cur) cur = ffn[l]->cuInfer(cur);
    }
    return cur && head.cuInfer_1(cur) ? KF_OK : KF_INTERNAL_ERR;
}

int Fish::EnqueueStep(int bound) {
    if (tp.world > 1) return EnqueueStepTP(); /* never an eager-only mode: both exclude a TP rank */
    if (EagerOnly() && engine_state == 0) EnsureEngine(); /* records why the engine is not used: engine_state < 0 below */
    if (use_engine && fuse_level >= 1 && engine_state > 0 && engine_embed && (graph_mode || state_tokens)) { /* embedding row read inside the launch */
        if (engine_head) { /* ... and the final norm, the LM head and the greedy pick: ONE launch per token */
            const int rc = kf_engine_step_head(ctx, engine.get(), nullptr, ToX(x), d_state, bound, samp_params.greedy() ? 1 : 0);
            if (rc < 0) return rc;
            if (rc == KF_OK) {
                engine_steps++;
                if (samp_params.greedy()) return KF_OK;
                return samp_params.Draw(ctx, ToX(head.preLogits), config.vocab, d_rng, d_state, d_tokens_out, d_forced, config.n_ctx);
            }
        } else {
            const int rc = kf_engine_step(ctx, engine.get(), nullptr, ToX(x), d_state, bound);
            if (rc < 0) return rc;
            if (rc == KF_OK) {
                engine_steps++;
                return head.cuInfer_1(x) ? KF_OK : KF_INTERNAL_ERR;
            }
        }
    }
    hGTensor cur = embed.cuInfer(-1);
    if (!cur) return KF_INTERNAL_ERR;
    if (use_engine && fuse_level >= 1 && engine_state > 0 && !(engine_embed && (graph_mode || state_tokens))) {
        const int rc = kf_engine_step(ctx, engine.get(), ToX(cur), ToX(x), d_state, bound);
        if (rc < 0) return rc;
        if (rc == KF_OK) {
            engine_steps++;
            return head.cuInfer_1(x) ? KF_OK : KF_INTERNAL_ERR;
        }
    }
    return LayersAndHead(cur);
}

int Fish::ForwardOnRLS(int token, int pos) {
    if (pos < 0 || pos >= config.n_ctx || token < 0 || token >= config.vocab) return KF_INVALID_ARGS;
    tok_pos = pos;
    graph_mode = false;
    KF_TRY(kf_set_state(ctx, d_state, token, pos));
    return LayersAndHead(embed.cuInfer(token));
}

int Fish::SetState(int token, int pos) { return kf_set_state(ctx, d_state, token, pos); }

// one launch sequence captured into `out`: `enqueue` runs between kf_graph_begin and kf_graph_end; the first refusal's code back, and then no graph is kept
template <class F>
static int Capture(kf_ctx* c, hGraph& out, F enqueue) {
    KF_TRY(kf_graph_begin(c));
    int rc = enqueue();
    kf_graph* g = nullptr;
    const int rc2 = kf_graph_end(c, &g);
    hGraph captured(g);
    if (rc == KF_OK && (rc = rc2) == KF_OK) out = std::move(captured);
    return rc;
}
kf_graph* Fish::GraphFor(int pos) {
    const int b = bucket_of(pos);
    if ((int)graphs.size() <= b) graphs.resize(b + 1);
    if (!graphs[b]) {
        if (use_engine && engine_state == 0) EnsureEngine(); /* not while capturing */
        tok_pos = pos;
        graph_mode = true;
        const int save = fuse_level;
        fuse_level = 1;
        const int rc = Capture(ctx, graphs[b], [&] { return EnqueueStep(pos_bound()); });
        fuse_level = save;
        graph_mode = false;
        if (rc != KF_OK) return nullptr;
    }
    return graphs[b].get();
}

// A step that is ONE kernel launch (the engine with the embedding row, the LM head and the greedy pick inside) gains nothing from a captured graph: replaying a
// one-node graph costs ~6 us more per step than the launch itself (measured, scratch/graph_vs_eager.py: 0.4222 vs 0.4158 ms at positions 1900-2040).
bool Fish::OneLaunchStep() {
    if (tp.world > 1 || !use_engine || fuse_level == 0) return false;
    if (engine_state == 0) EnsureEngine();
    return engine_state > 0 && engine_embed && engine_head && samp_params.greedy();
}

int Fish::RunSteps(int pos, int n, bool use_graph) {
    if (pos < 0 || pos + n > config.n_ctx) return KF_INVALID_ARGS;
    KF_TRY(TPCommit());
    if (use_graph && n > 1 && !EagerOnly() && OneLaunchStep()) { /* runs of steps inside one position bucket: ONE launch each (kf_engine_steps_head), at most kStepsPerLaunch steps */
        constexpr int kStepsPerLaunch = 16;
        int i = 0;
        while (i < n) {
            const int p = pos + i, b = bucket_of(p);
            int m = 1;
            while (i + m < n && m < kStepsPerLaunch && bucket_of(pos + i + m) == b) m++;
            tok_pos = p;
            if (m > 1) EnsureHeadScreen();
            if (engine_autotune > 0 && engine_embed) { /* once per position bucket: the hand-off delays measured at the first step inside it */
                if (bucket_tuned.empty()) bucket_tuned.assign((size_t)bucket_of(config.n_ctx - 1) + 1, 0);
                if (!bucket_tuned[b]) {
                    bucket_tuned[b] = 1;
                    const int trc = kf_engine_tune(ctx, engine.get(), ToX(x), d_state, pos_bound(), engine_autotune, nullptr, nullptr);
                    if (trc < 0) { /* a tuning problem (a poll timed out while a delay was being tried) is not a decode error: the built-in delays stay (kf_engine_tune restored
                                      them), the latched error word is cleared, and the step below runs */
                        if (kf_engine_reset(ctx, engine.get()) != KF_OK) return trc;
                        engine_autotune = 0;
                    }
                }
            }
            const int rc = kf_engine_steps_head(ctx, engine.get(), ToX(x), d_state, pos_bound(), m);
            if (rc < 0) return rc;
            if (rc != KF_OK) break; /* not served at this position: the per-step path below takes the rest */
            engine_steps += m;
            i += m;
        }
        if (i == n) return KF_OK;
        pos += i, n -= i;
    }
    for (int i = 0; i < n; i++) {
        const int p = pos + i;
        if (fuse_level == 0 || EagerOnly()) {  // per-kernel launches only (AutoAWQ weights; the eager-only modes): eager, position from the host, token from the device state
            tok_pos = p;
            graph_mode = false, state_tokens = true;
            int rc = EnqueueStep(pos_bound());
            state_tokens = false;
            KF_TRY(rc);
        } else if (use_graph && !OneLaunchStep()) {
            kf_graph* g = GraphFor(p);
            if (!g) return KF_INTERNAL_ERR;
            KF_TRY(kf_graph_launch(ctx, g));
        } else {
            if (use_engine && engine_state == 0) EnsureEngine();
            tok_pos = p;
            graph_mode = true;  // positions/tokens still come from d_state, launches are eager
            const int save = fuse_level;
            fuse_level = 1;
            int rc = EnqueueStep(pos_bound());
            fuse_level = save;
            graph_mode = false;
            KF_TRY(rc);
        }
    }
    return KF_OK;
}

int Fish::Prefill(const int* tokens, int n, int pos0) {
    if (n < 1 || pos0 < 0 || pos0 + n > config.n_ctx) return KF_INVALID_ARGS;
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= config.vocab) return KF_INVALID_ARGS;
    const int PC = prefill_chunk < config.n_ctx ? prefill_chunk : config.n_ctx;
    KF_TRY(PrefillReady());
    int m = 0;
    for (int c0 = 0; c0 < n; c0 += PC) {
        m = n - c0 < PC ? n - c0 : PC;
        KF_TRY(FlowChunk(tokens + c0, m, pos0 + c0));
    }
    return FlowEnd(m - 1, tokens[n - 1], pos0 + n - 1);
}
int Fish::FlowChunk(const int* tokens, int m, int pos) {
    floatX* bx = ToX(gBUFF.bX);
    const kf_weight we = embed.w->desc();
    KF_TRY(kf_h2d(ctx, gBUFF.d_ptok, tokens, (size_t)m * 4));
    KF_TRY(kf_embed_batch(ctx, &we, gBUFF.d_ptok, m, bx));
    for (int l = 0; l < config.nLayer; l++) {
        KF_TRY(attn[l]->cuFlow(bx, pos, m));
        KF_TRY(ffn[l]->cuFlow(bx, m));
    }
    return KF_OK;
}
// head on the last token (row `last` of the batch buffer, `token` at `pos`); the state update leaves {next token, pos + 1}
int Fish::FlowEnd(int last, int token, int pos) {
    const int C = config.nEmbed;
    KF_TRY(kf_d2d(ctx, x->data, ToX(gBUFF.bX) + (size_t)last * C, (size_t)C * 2));
    KF_TRY(SetState(token, pos));
    tok_pos = pos;
    return HeadAndPick(ToX(x));
}

int Fish::ScoreReady() {
    KF_TRY(PrefillReady());
    const int R = gBUFF.rows;
    if (gBUFF.score_rows >= R) return KF_OK;
    KF_TRY(kf_sync(ctx));
    static_cast<ScoreBuffers&>(gBUFF) = ScoreBuffers(); /* the old set goes first, as it always did */
    kf_weight wh = head.proj.w->desc();
    return Commit<ScoreBuffers>(gBUFF, ctx, R, kf_head_logprob_scratch_bytes(&wh, R));
}

int Fish::Score(const int* tokens, int n, int pos0, float* logprob_out, int* top1_out) {
    if (n < 2 || pos0 < 0 || pos0 + n > config.n_ctx || !tokens || !logprob_out) return KF_INVALID_ARGS;
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= config.vocab) return KF_INVALID_ARGS;
    const int PC = prefill_chunk < config.n_ctx ? prefill_chunk : config.n_ctx, C = config.nEmbed;
    KF_TRY(ScoreReady());
    floatX* bx = ToX(gBUFF.bX);
    const kf_weight wh = head.proj.w->desc();
    std::vector<int32_t> tgt(PC);
    int m = 0;
    for (int c0 = 0; c0 < n; c0 += PC) {
        m = n - c0 < PC ? n - c0 : PC;
        KF_TRY(FlowChunk(tokens + c0, m, pos0 + c0));
        // row i of the chunk predicts token c0 + i + 1: the first token of the next chunk for the chunk's last row, nothing for the last row of all
        const int ns = c0 + m < n ? m : m - 1;
        if (ns < 1) continue;
        for (int i = 0; i < m; i++) tgt[i] = i < ns ? tokens[c0 + i + 1] : -1;
        KF_TRY(kf_h2d(ctx, gBUFF.d_stgt, tgt.data(), (size_t)m * 4));
        KF_TRY(kf_rmsnorm(ctx, bx, ToX(final_norm.w), ToX(gBUFF.bNorm), ns, C, final_norm.rms_eps, nullptr));
        KF_TRY(kf_head_logprob(ctx, &wh, ToX(gBUFF.bNorm), C, ns, gBUFF.d_stgt, gBUFF.d_slp, nullptr, top1_out ? gBUFF.d_stop1.get() : nullptr, gBUFF.score_ws));
        KF_TRY(kf_d2h(ctx, logprob_out + c0, gBUFF.d_slp, (size_t)ns * 4));
        if (top1_out) KF_TRY(kf_d2h(ctx, top1_out + c0, gBUFF.d_stop1, (size_t)ns * 4));
    }
    return FlowEnd(m - 1, tokens[n - 1], pos0 + n - 1); /* Prefill's own ending */
}

int Fish::EvalPPL(const int* tokens, long long n, int window, double* ppl, double* pplerr, long long* n_scored) {
    if (!tokens || n < 2 || !ppl) return KF_INVALID_ARGS;
    const int W = window <= 0 || window > config.n_ctx ? config.n_ctx : window;
    if (W < 2) return KF_INVALID_ARGS;
    std::vector<float> lp(W);
    double sum = 0.0, ss = 0.0;
    long long nz = 0;
    for (long long w0 = 0; w0 + 1 < n; w0 += W) {
        const int m = (int)(n - w0 < W ? n - w0 : W);
        KF_TRY(Score(tokens + w0, m, 0, lp.data(), nullptr));
        for (int i = 0; i < m - 1; i++) sum += (double)lp[i], ss += (double)lp[i] * (double)lp[i], nz++;
    }
    *ppl = exp(-sum / (double)nz);
    if (pplerr) *pplerr = *ppl * sqrt((ss - sum * sum / (double)nz) / (double)nz / (double)nz);
    if (n_scored) *n_scored = nz;
    return KF_OK;
}

// the token-batch buffers ([prefill_chunk rows]) and the tile kernels' scratch / resident copies: allocated by the first prefill, never inside a later one
int Fish::PrefillReady(int min_rows) {
    int PC = prefill_chunk < config.n_ctx ? prefill_chunk : config.n_ctx; /* one prompt never has more rows than the context; a batch of prompts (XcdReplicas::PrefillBatch) may */
    const int C = config.nEmbed, qd = config.n_head * config.head_dim;
    if (min_rows > prefill_chunk) return KF_INVALID_ARGS;
    PC = min_rows > PC ? min_rows : PC;
    if (gBUFF.bX && gBUFF.rows < PC) { /* a later, larger batch: the buffers grow once (never inside a captured region: prefill launches are eager) */
        KF_TRY(kf_sync(ctx));
        static_cast<TokenBatch&>(gBUFF) = TokenBatch(); /* the old set goes first (it can be large): a refusal below leaves it empty, rows 0 */
        if (!deq_arena) resident_tried = false; /* the larger batch may be one the resident bf16 copies serve (>= 1024 rows) */
    }
    if (!gBUFF.bX) {
        TokenBatch fresh;
        KF_TRY(fresh.Alloc(ctx, PC, C, qd, config.n_ff));
        // the stacked large-batch routes (Q | K | V and gate | up dequantised back to back, one tile-GEMM launch each): their workspace, sized here -- the first
        // Prefill allocates the batch buffers anyway; the launches themselves never allocate.  The set is committed behind it: rows are never held without their scratch
        for (int l = 0; l < config.nLayer; l++) {
            kf_weight wq = attn[l]->Q.w->desc(), wk = attn[l]->K.w->desc(), wv = attn[l]->V.w->desc(), wg = ffn[l]->gate.w->desc(), wu = ffn[l]->up.w->desc();
            const kf_weight* qkv[3] = {&wq, &wk, &wv};
            const kf_weight* gu[2] = {&wg, &wu};
            const size_t need = kf_linear_multi_scratch_bytes(3, qkv, PC), need2 = kf_linear_multi_scratch_bytes(2, gu, PC);
            KF_TRY(GrowScratch(need > need2 ? need : need2));
        }
        static_cast<TokenBatch&>(gBUFF) = std::move(fresh);
    }
    return EnsureResident(gBUFF.rows);
}

int Fish::HeadAndPick(const floatX* x_last) {
    kf_weight wh = head.proj.w->desc();
    if (samp_params.greedy())
        return kf_norm_lm_head(ctx, x_last, ToX(final_norm.w), final_norm.rms_eps, &wh, ToX(head.preLogits), d_state, d_tokens_out, gBUFF.head_ws->data);
    KF_TRY(kf_norm_lm_head(ctx, x_last, ToX(final_norm.w), final_norm.rms_eps, &wh, ToX(head.preLogits), nullptr, nullptr, gBUFF.head_ws->data));
    return samp_params.Draw(ctx, ToX(head.preLogits), config.vocab, d_rng, d_state, d_tokens_out, d_forced, config.n_ctx);
}

int Fish::SetSampler(const CHAT_SAMPLER& s) {
    if (!s.Valid(config.vocab)) return KF_INVALID_ARGS;
    const bool was_greedy = samp_params.greedy();
    samp_params = s;
    if (!was_greedy || !s.greedy()) DropGraphs(); /* the captured step graphs end in a different pick, or hold the old sampler arguments */
    if (!d_rng) KF_TRY(d_rng.Alloc(ctx, 8));
    return kf_h2d(ctx, d_rng, &samp_params.seed, 8);
}

int Fish::Generate(const int* prompt, int n_prompt, int n_new, int* out, bool use_graph) {
    if (n_prompt < 1 || n_new < 1 || n_prompt + n_new - 1 > config.n_ctx) return KF_INVALID_ARGS;
    std::vector<int32_t> forced(config.n_ctx, -1);
    for (int i = 0; i < n_prompt; i++) forced[i] = prompt[i];
    KF_TRY(kf_h2d(ctx, d_forced, forced.data(), forced.size() * 4));
    const int total = n_prompt + n_new - 1;
    if (prefill_mode == 1 && n_prompt > 1) {
        KF_TRY(Prefill(prompt, n_prompt, 0));
        if (n_new > 1) KF_TRY(RunSteps(n_prompt, n_new - 1, use_graph));
    } else {
        KF_TRY(SetState(prompt[0], 0));
        KF_TRY(RunSteps(0, total, use_graph));
    }
    std::vector<int32_t> toks(config.n_ctx);
    KF_TRY(kf_d2h(ctx, toks.data(), d_tokens_out, toks.size() * 4));
    KF_TRY(EngineCheck()); /* a launch that could not become resident leaves an error word, never a hang */
    for (int i = 0; i < n_new; i++) out[i] = toks[n_prompt - 1 + i];
    return KF_OK;
}

// ------------------------------------------------------------------------------------------------ speculative decoding: the verify pass and the rounds
int Fish::Verify(const int* tokens, int n, int pos0, int* top1, floatX* logits, std::string& why) {
    if (!tokens || !top1 || n < 1 || n > KF_SPEC_MAX_K + 1 || pos0 < 0 || pos0 + n > config.n_ctx)
        return refused(why, "kfh_verify", KF_INVALID_ARGS, "1 .. 8 tokens at positions inside the context, and a place for their ids");
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= config.vocab) return refused(why, "kfh_verify", KF_INVALID_ARGS, "a token id outside the vocabulary");
    if (!embed.w || !head.proj.w) return refused(why, "kfh_verify", KF_INVALID_ARGS, "the model has no weights yet");
    if (HasRow3()) return refused(why, "kfh_verify", KF_UNSUPPORTED_DATATYPE, kRow3Why); /* the row entries (kf_*_rows) do not unpack the 3-bit stream */
    const int rcm = verify_refusal(Modes(), samp_params.greedy(), "kfh_verify", why);
    if (rcm != KF_OK) return Kv8Note(why), rcm;
    if (!vrows.vX) KF_TRY(Commit(vrows, ctx, config, head.proj.w->desc())); /* allocated by the first Verify */
    if (logits && !vLogits && !(vLogits = GT(ctx, "vLogits", typNUMBER::BF16, config.vocab, KF_SPEC_MAX_K + 1))) return KF_OUTOF_GPUMEMORY;
    const int C = config.nEmbed, hd = config.head_dim, nh = config.n_head, nkv = config.n_head_kv, qd = nh * hd, kvd = nkv * hd, F = config.n_ff;
    floatX *bx = ToX(vrows.vX), *bq = ToX(vrows.vQ), *ba = ToX(vrows.vAttn), *bg = ToX(vrows.vGate);
    int32_t *d_vtok = vrows.d_vtok, *d_top1 = d_vtok + KF_SPEC_MAX_K + 1;
    int64_t before[2], after[2];
    KF_TRY(kf_rows_route_counts(ctx, before));
    const kf_weight we = embed.w->desc();
    KF_TRY(kf_h2d(ctx, d_vtok, tokens, (size_t)n * 4));
    KF_TRY(kf_embed_batch(ctx, &we, d_vtok, n, bx));
    for (int l = 0; l < config.nLayer; l++) {
        SelfAttention* a = attn[l].get();
        FFN* m = ffn[l].get();
        floatX* kc = reinterpret_cast<floatX*>(cache.Get(KVCache::KV_KEY, l, 0));
        floatX* vc = reinterpret_cast<floatX*>(cache.Get(KVCache::KV_VAL, l, 0));
        const kf_weight wq = a->Q.w->desc(), wk = a->K.w->desc(), wv = a->V.w->desc(), wo = a->proj_cat.w->desc();
        const kf_weight wg = m->gate.w->desc(), wu = m->up.w->desc(), wd = m->down.w->desc();
        const kf_weight* qkv[3] = {&wq, &wk, &wv};
        kf_bf16* ys[3] = {bq, kc, vc}; /* the raw K rows and the V rows straight into cache rows pos0 + r */
        const int64_t row_stride[3] = {qd, 0, 0}, pos_stride[3] = {0, kvd, kvd};
        KF_TRY(kf_norm_linear_rows(ctx, bx, C, ToX(a->norm.w), a->norm.rms_eps, 3, qkv, ys, row_stride, pos_stride, pos0, n));
        // every K row of the batch normed and rotated in place BEFORE the attention: query r reads the keys of rows 0 .. r - 1
        KF_TRY(kf_qknorm_rope_batch(ctx, bq, kc + (size_t)pos0 * kvd, a->normQ.w ? ToX(a->normQ.w) : nullptr, a->normK.w ? ToX(a->normK.w) : nullptr, rope_table, pos0, n, qd, kvd,
                                    nh, nkv, hd, a->normQ.rms_eps));
        KF_TRY(kf_attn_decode_rows(ctx, bq, qd, kc, vc, ba, pos0, n, nh, nkv, hd, kvd, vrows.v_attn_ws->data));
        KF_TRY(kf_linear_rows(ctx, &wo, ba, qd, bx, C, n, KF_EPI_RESIDUAL, bx, C));
        KF_TRY(kf_norm_gateup_swiglu_rows(ctx, bx, C, ToX(m->norm.w), m->norm.rms_eps, &wg, &wu, bg, F, n));
        KF_TRY(kf_linear_rows(ctx, &wd, bg, F, bx, C, n, KF_EPI_RESIDUAL, bx, C));
    }
    const kf_weight wh = head.proj.w->desc();
    KF_TRY(kf_norm_lm_head_rows(ctx, bx, C, ToX(final_norm.w), final_norm.rms_eps, &wh, logits ? ToX(vLogits) : nullptr, config.vocab, d_top1, n, vrows.v_head_ws->data));
    KF_TRY(kf_d2h(ctx, top1, d_top1, (size_t)n * 4)); /* the round's one read */
    if (logits) KF_TRY(kf_d2h(ctx, logits, vLogits->data, (size_t)n * config.vocab * 2));
    KF_TRY(kf_rows_route_counts(ctx, after));
    verify_rows[0] += after[0] - before[0], verify_rows[1] += after[1] - before[1];
    return KF_OK;
}

int SpecDecoder::Propose(const std::vector<int>& ids, int kk, int* out) {
    const int n = (int)ids.size();
    if (kk < 1) return 0;
    if (kind == 0) return spec_lookup(ids.data(), n, ngram, kk, out);
    if (kind == 2) {
        const int m = fn ? fn(ids.data(), n, kk, out, user) : 0;
        return m < 0 ? 0 : m > kk ? kk : m;
    }
    // another Fish: the ids it has not consumed yet are teacher-forced (rows draft_rows .. n - 1), then kk - 1 free-running steps; the step at row p gives the id of
    // row p + 1, so rows n - 1 .. n + kk - 2 give the kk proposals.  Rows past the accepted ones are rewritten by a later round before anything reads them
    Fish* d = draft;
    const int p0 = draft_rows, steps = n - p0 + kk - 1;
    if (kf_h2d(d->ctx, d->d_forced + p0, ids.data() + p0, (size_t)(n - p0) * 4) != KF_OK) return -1;
    if (d->SetState(ids[p0], p0) != KF_OK || d->RunSteps(p0, steps, true) != KF_OK) return -1;
    if (kf_d2h(d->ctx, out, d->d_tokens_out + (n - 1), (size_t)kk * 4) != KF_OK || d->EngineCheck() != KF_OK) return -1;
    return kk;
}

int SpecDecoder::Generate(const int* prompt, int n_prompt, int n_new, int* out, std::string& why) {
    Fish* f = target;
    if (!f || !prompt || !out || n_prompt < 1 || n_new < 1 || n_prompt + n_new - 1 > f->config.n_ctx)
        return refused(why, "kfh_spec_generate", KF_INVALID_ARGS, "a prompt and a number of new ids that fit the context");
    if (k < 1 || k > KF_SPEC_MAX_K) return refused(why, "kfh_spec_generate", KF_INVALID_ARGS, "k outside 1 .. 7");
    for (int i = 0; i < n_prompt; i++)
        if (prompt[i] < 0 || prompt[i] >= f->config.vocab) return refused(why, "kfh_spec_generate", KF_INVALID_ARGS, "a prompt id outside the vocabulary");
    int n_ctx = f->config.n_ctx;
    if (kind == 1) {
        if (!draft || draft == f || draft->config.vocab != f->config.vocab) return refused(why, "kfh_spec_generate", KF_INVALID_ARGS, "the drafter is another Fish with the target's vocabulary");
        if (!draft->samp_params.greedy()) return refused(why, "kfh_spec_generate", KF_INVALID_ARGS, "the drafter proposes greedy ids: kfh_set_sampler with temperature 0 on it first");
        if (draft->config.n_ctx < n_ctx) n_ctx = draft->config.n_ctx; /* rounds stop drafting where the drafter's cache ends */
        std::vector<int32_t> free_run((size_t)draft->config.n_ctx, -1);
        KF_TRY(kf_h2d(draft->ctx, draft->d_forced, free_run.data(), free_run.size() * 4));
        draft_rows = 0;
    }
    const int rcm = verify_refusal(f->Modes(), f->samp_params.greedy(), "kfh_spec_generate", why); /* before the prompt runs: a refused call changes nothing */
    if (rcm != KF_OK) return f->Kv8Note(why), rcm;
    // the prompt, as Generate runs it: the ids forced, token-serial steps up to the last prompt token (prefill_mode 1: the token batch, which also gives the first new id)
    std::vector<int32_t> forced(f->config.n_ctx, -1);
    for (int i = 0; i < n_prompt; i++) forced[i] = prompt[i];
    KF_TRY(kf_h2d(f->ctx, f->d_forced, forced.data(), forced.size() * 4));
    std::vector<int> ids(prompt, prompt + n_prompt); /* the context: every id that is settled; the last one is not in the caches yet */
    int n_out = 0;
    if (f->prefill_mode == 1 && n_prompt > 1) {
        KF_TRY(f->Prefill(prompt, n_prompt, 0));
        int32_t st[4];
        KF_TRY(kf_d2h(f->ctx, st, f->d_state, 16));
        ids.push_back(st[0]), out[n_out++] = st[0];
    } else if (n_prompt > 1) {
        KF_TRY(f->SetState(prompt[0], 0));
        KF_TRY(f->RunSteps(0, n_prompt - 1, true));
    }
    int drafts[KF_SPEC_MAX_K + 1], rows[KF_SPEC_MAX_K + 1], top1[KF_SPEC_MAX_K + 1];
    while (n_out < n_new) {
        const int pos = (int)ids.size() - 1; /* the row of the last settled id */
        const int kk = spec_clip_k(k, n_new - n_out, pos, n_ctx);
        const int m = Propose(ids, kk, drafts);
        if (m < 0) return refused(why, "kfh_spec_generate", KF_INTERNAL_ERR, "the drafter's steps failed");
        rows[0] = ids.back();
        for (int i = 0; i < m; i++) {
            if (drafts[i] < 0 || drafts[i] >= f->config.vocab) return refused(why, "kfh_spec_generate", KF_INVALID_ARGS, "the drafter proposed an id outside the vocabulary");
            rows[1 + i] = drafts[i];
        }
        KF_TRY(f->Verify(rows, m + 1, pos, top1, nullptr, why));
        const int n_acc = spec_accept(drafts, m, top1);
        for (int i = 0; i <= n_acc; i++) ids.push_back(top1[i]), out[n_out++] = top1[i];
        rounds++, proposed += m, accepted += n_acc;
        if (kind == 1 && m > 0) draft_rows = n_acc + 1 < m ? pos + n_acc + 1 : pos + m; /* its steps took rows up to pos + m - 1: those whose input was a kept id stay */
    }
    // behind the last id, as Generate leaves the target: the ids in d_tokens_out (the id produced at each position), the state on the last of them
    const int last = (int)ids.size() - 1;
    KF_TRY(kf_h2d(f->ctx, f->d_tokens_out + (n_prompt - 1), out, (size_t)n_new * 4));
    KF_TRY(f->SetState(ids[last], last));
    return f->EngineCheck();
}

// ------------------------------------------------------------------------------------------------ XCD engines
// n_kv K / V caches of the card's layout (XcdReplicas: one per sequence; XcdTP: one per rank), then per sequence: logits, residual stream, state, forced ids, ids out
int XcdSeqs::Alloc(kf_ctx* c, const MODEL_CARD& card, int n_kv, int n_seq, int vocab) {
    const int kvd = card.n_head_kv * card.head_dim;
    key = GT(c, "xcd.key", typNUMBER::BF16, kvd, card.n_ctx * card.nLayer * n_kv);
    val = GT(c, "xcd.val", typNUMBER::BF16, kvd, card.n_ctx * card.nLayer * n_kv);
    logits = GT(c, "xcd.logits", typNUMBER::BF16, vocab, n_seq);
    x = GT(c, "xcd.x", typNUMBER::BF16, card.nEmbed, n_seq);
    if (!key || !val || !logits || !x) return KF_OUTOF_GPUMEMORY;
    KF_TRY(kf_memset(c, key->data, 0, key->szData));
    KF_TRY(kf_memset(c, val->data, 0, val->szData));
    return SeqBuffers::Alloc(c, n_seq, card.n_ctx, 0);
}
int XcdReplicas::BatchRows::Alloc(kf_ctx* c, int kv_dim, int rows, int vocab, int n_seq) {
    bK = GT(c, "xr.bK", typNUMBER::BF16, kv_dim, rows), bV = GT(c, "xr.bV", typNUMBER::BF16, kv_dim, rows);
    if (!bK || !bV) return KF_OUTOF_GPUMEMORY;
    KF_TRY(d_dst.Alloc(c, (size_t)3 * n_seq * sizeof(void*) + (size_t)n_seq * 4)); /* three tables of destinations (K, V, logits) + the slots */
    bL = GT(c, "xr.bL", typNUMBER::BF16, vocab, n_seq);
    return bL ? KF_OK : KF_OUTOF_GPUMEMORY;
}
int XcdEngine::LaunchSteps(int n) {
    for (int i = 0; i < n;) {
        const int m = n - i < steps_per_launch ? n - i : steps_per_launch;
        KF_TRY(kf_xengine_steps(ctx, engine.get(), ToX(x), d_state, m, 1));
        i += m;
    }
    return KF_OK;
}
int XcdEngine::SetStepsPerLaunch(int n) {
    if (n < 1 || n > 4096) return KF_INVALID_ARGS;
    steps_per_launch = n;
    return KF_OK;
}
int XcdEngine::Check() {
    if (!engine) return KF_OK;
    const int rc = kf_xengine_check(ctx, engine.get());
    if (rc == KF_INTERNAL_ERR) kf_xengine_reset(ctx, engine.get());
    return rc;
}

// ---- XCD-confined replicas
size_t XcdReplicas::kv_seq_elems() const {
    const MODEL_CARD& c = hFish->config;
    return (size_t)c.nLayer * c.n_ctx * c.n_head_kv * c.head_dim;
}
// the engine over the Fish's weights AS THEY ARE NOW (their device addresses go into the engine's layer table; the GQA-4 forms copy q | k | v): called by Build, and again by
// the first use after the Fish's weights changed (kfh_weights_changed / a weight set again: Fish::weights_gen) -- a decode through this object never reads stale weights
int XcdReplicas::MakeEngine(bool allocate) {
    Fish* f = hFish;
    const MODEL_CARD& c = f->config;
    std::vector<kf_engine_layer> L;
    kf_engine_desc d;
    KF_TRY(f->EngineRefusal(why));
    KF_TRY(f->EngineTable(ToX(f->cache.key), ToX(f->cache.val), true, why, L, d)); /* the Fish's own K / V rows stand in for the validation below: a refused model allocates nothing */
    {
        char w[320];
        w[0] = 0;
        const int served = kf_xengine_served(ctx, &d, w, sizeof(w));
        why = w;
        if (served != KF_OK) return served < 0 ? served : KF_ENGINE_NOT_SERVED;
    }
    if (!f->embed.w || !f->head.proj.w || !f->final_norm.w || f->final_norm.rms_eps != c.rms_eps) {
        why = "embedding / head / final norm missing";
        return KF_ENGINE_NOT_SERVED;
    }
    if (allocate) KF_TRY(Commit<XcdSeqs>(*this, ctx, c, n_seq, n_seq, c.vocab));
    KF_TRY(f->EngineTable(ToX(key), ToX(val), true, why, L, d)); /* the table again, on this object's rows */
    KF_TRY(EnsureWorkspace(kf_xengine_workspace_bytes(&d)));
    kf_xengine* e = nullptr;
    int rc = kf_xengine_create(ctx, &d, n_seq, (int64_t)kv_seq_elems(), engine_ws, engine_ws.bytes(), &e);
    if (rc != KF_OK) {
        why = kf_last_error();
        return rc;
    }
    engine.reset(e);
    kf_weight we = f->embed.w->desc(), wh = f->head.proj.w->desc();
    rc = kf_xengine_set_embedding(ctx, engine.get(), &we, d_forced, c.n_ctx);
    if (rc == KF_OK) rc = kf_xengine_set_head(ctx, engine.get(), &wh, ToX(f->final_norm.w), ToX(logits), d_tokens_out, c.n_ctx);
    if (rc != KF_OK) {
        why = "the embedding table and the LM head must be bf16 (read inside the launch)";
        return rc == KF_UNSUPPORTED_DATATYPE ? KF_ENGINE_NOT_SERVED : rc;
    }
    built_gen = f->weights_gen;
    return KF_OK;
}
int XcdReplicas::Build(Fish* f, int n_seq_) {
    if (!f || n_seq_ < 1 || n_seq_ > KF_XENGINE_MAX_SEQ) return KF_INVALID_ARGS;
    hFish = f, ctx = f->ctx, n_seq = n_seq_;
    return MakeEngine(true);
}
int XcdReplicas::Fresh() {
    if (engine && built_gen == hFish->weights_gen) return KF_OK;
    if (engine) {
        KF_TRY(kf_sync(ctx)); /* the deleter does not */
        engine.reset();
    }
    const int rc = MakeEngine(false); /* caches, states, forced ids and ids out stay: the sequences go on where they stand, on the new weights */
    if (rc != KF_OK) g_host_err = "XcdReplicas: " + why; /* a switch moved on the Fish since the engine was built (int8 activations, adapters, the int8 KV cache): kfh_host_error says which */
    return rc;
}
int XcdReplicas::SetForced(int seq, const int32_t* ids, int n) {
    if (seq < 0 || seq >= n_seq || n < 0 || n > hFish->config.n_ctx) return KF_INVALID_ARGS;
    std::vector<int32_t> row(hFish->config.n_ctx, -1);
    for (int i = 0; i < n; i++) row[i] = ids[i];
    return kf_h2d(ctx, d_forced + (size_t)seq * hFish->config.n_ctx, row.data(), row.size() * 4);
}
int XcdReplicas::SetState(int seq, int token, int pos) {
    if (seq < 0 || seq >= n_seq || pos < 0 || pos >= hFish->config.n_ctx || token < 0 || token >= hFish->config.vocab) return KF_INVALID_ARGS;
    KF_TRY(kf_memset32(ctx, d_state + 4 * seq + 3, 0, 1)); /* the status word of the re-aimed sequence */
    return kf_set_state(ctx, d_state + 4 * seq, token, pos);
}
// CHAT_SAMPLER for Chat (greedy by default): one rng word per sequence, seeded per request
int XcdReplicas::SetSampler(const CHAT_SAMPLER& sp) {
    if (!sp.Valid(hFish->config.vocab)) return KF_INVALID_ARGS;
    if (!sp.greedy() && !d_rng) KF_TRY(d_rng.Alloc(ctx, (size_t)n_seq * 8));
    samp_params = sp;
    return KF_OK;
}
// A parked sequence is skipped by the launches (the others decode on); its cache, state and ids stay.  Status: 0, or 64 = the last launch would have left the
// sequence's cache rows and skipped it (kf_abi.h: d_state [n_seq][4] = {token, pos, parked, status}).
int XcdReplicas::Park(int seq, bool on) {
    if (seq < 0 || seq >= n_seq) return KF_INVALID_ARGS;
    return kf_memset32(ctx, d_state + 4 * seq + 2, on ? 1 : 0, 1); /* on the stream, no host sync: the queue flips these between launches */
}
int XcdReplicas::Status(int seq, int32_t* out4) {
    if (seq < 0 || seq >= n_seq || !out4) return KF_INVALID_ARGS;
    return kf_d2h(ctx, out4, d_state + 4 * seq, 16);
}
// The prompt half of "prefill + decode" for one of the sequences: the model's own batched prefill (Fish::Prefill: the reference prefills token by token through the decode
// path, GoPT.cpp:1139-1146), then the prompt's K / V rows of every layer move into the sequence's cache and the sequence stands at {first generated id, n}.
int XcdReplicas::Prefill(int seq, const int* tokens, int n) {
    const MODEL_CARD& c = hFish->config;
    if (seq < 0 || seq >= n_seq || !tokens || n < 1 || n >= c.n_ctx) return KF_INVALID_ARGS;
    KF_TRY(Fresh());
    {   /* the sequence's cache has the model's own layout ([layer][row][kv_dim]): for the length of the call the model's cache IS the sequence's, the rows land where they stay */
        struct Aim {
            KVCache& kc;
            void *k0, *v0;
            Aim(KVCache& c_, void* k, void* v) : kc(c_), k0(c_.key->data), v0(c_.val->data) { kc.key->data = k, kc.val->data = v; }
            ~Aim() { kc.key->data = k0, kc.val->data = v0; }
        } aim(hFish->cache, ToX(key) + (size_t)seq * kv_seq_elems(), ToX(val) + (size_t)seq * kv_seq_elems());
        KF_TRY(hFish->Prefill(tokens, n, 0));
    }
    KF_TRY(kf_d2d(ctx, ToX(logits) + (size_t)seq * c.vocab, ToX(hFish->head.preLogits), (size_t)c.vocab * 2));   /* the last prompt token's logits */
    KF_TRY(kf_d2d(ctx, d_state + 4 * seq, hFish->d_state, 8));                                                   /* {the id picked behind the prompt, n} */
    KF_TRY(kf_memset(ctx, d_state + 4 * seq + 3, 0, 4));                                                         /* status: clear */
    KF_TRY(kf_d2d(ctx, d_tokens_out + (size_t)seq * c.n_ctx + (n - 1), hFish->d_tokens_out + (n - 1), 4));      /* ids out: position n - 1 holds that id, as after decode steps */
    return KF_OK;
}
int XcdReplicas::PrefillBatch(const int* slots, const int32_t* tokens, const int* lens, int S, int stride) {
    Fish* f = hFish;
    const MODEL_CARD& c = f->config;
    if (!slots || !tokens || !lens || S < 1 || S > n_seq || stride < 1) return KF_INVALID_ARGS;
    int T = 0;
    for (int i = 0; i < S; i++) {
        if (slots[i] < 0 || slots[i] >= n_seq || lens[i] < 1 || lens[i] > stride || lens[i] >= c.n_ctx) return KF_INVALID_ARGS;
        for (int j = 0; j < i; j++)
            if (slots[j] == slots[i]) return KF_INVALID_ARGS;
        for (int t = 0; t < lens[i]; t++)
            if (tokens[(size_t)i * stride + t] < 0 || tokens[(size_t)i * stride + t] >= c.vocab) return KF_INVALID_ARGS;
        T = lens[i] > T ? lens[i] : T;
    }
    /* rows of a prompt behind its end (padding up to the batch's longest): finite values that nobody reads before a decode step rewrites them */
    const int R = S * T, C = c.nEmbed;
    const int qd = c.n_head * c.head_dim, kvd = c.n_head_kv * c.head_dim;
    if (T >= c.n_ctx || R > f->prefill_chunk) return KF_INVALID_ARGS;
    KF_TRY(Fresh());
    KF_TRY(f->PrefillReady(R));
    if (!pb.bK || pb.bK->ne[1] < R) {
        KF_TRY(kf_sync(ctx));
        KF_TRY(Commit(pb, ctx, kvd, f->gBUFF.rows, c.vocab, n_seq));
    }
    std::vector<int32_t> rows((size_t)R, 0);
    std::vector<void*> dst((size_t)3 * n_seq + (n_seq + 1) / 2, nullptr); /* the slots ride behind the pointer tables as int32 */
    int32_t* h_slots = reinterpret_cast<int32_t*>(dst.data() + (size_t)3 * n_seq);
    for (int i = 0; i < S; i++) {
        memcpy(rows.data() + (size_t)i * T, tokens + (size_t)i * stride, (size_t)lens[i] * 4);
        dst[i] = ToX(key) + (size_t)slots[i] * kv_seq_elems(), dst[n_seq + i] = ToX(val) + (size_t)slots[i] * kv_seq_elems();
        dst[2 * n_seq + i] = ToX(logits) + (size_t)slots[i] * c.vocab;
        h_slots[i] = slots[i];
    }
    const int32_t* d_slots = reinterpret_cast<const int32_t*>(pb.d_dst + (size_t)3 * n_seq);
    KF_TRY(kf_h2d(ctx, f->gBUFF.d_ptok, rows.data(), (size_t)R * 4));
    KF_TRY(kf_h2d(ctx, pb.d_dst, dst.data(), (size_t)3 * n_seq * sizeof(void*) + (size_t)n_seq * 4));
    floatX *bx = ToX(f->gBUFF.bX), *bn = ToX(f->gBUFF.bNorm), *bq = ToX(f->gBUFF.bQ), *ba = ToX(f->gBUFF.bAttn), *bk = ToX(pb.bK), *bv = ToX(pb.bV);
    kf_weight we = f->embed.w->desc();
    KF_TRY(kf_embed_batch(ctx, &we, f->gBUFF.d_ptok, R, bx));
    for (int l = 0; l < c.nLayer; l++) {
        SelfAttention& a = *f->attn[l];
        kf_weight wq = a.Q.w->desc(), wk = a.K.w->desc(), wv = a.V.w->desc(), wo = a.proj_cat.w->desc();
        KF_TRY(kf_rmsnorm(ctx, bx, ToX(a.norm.w), bn, R, C, a.norm.rms_eps, nullptr));
        KF_TRY(kf_qkv_rope_seqs(ctx, &wq, &wk, &wv, bn, bq, bk, bv, R, T, a.normQ.w ? ToX(a.normQ.w) : nullptr, a.normK.w ? ToX(a.normK.w) : nullptr, f->rope_table, 0, c.n_head,
                                c.n_head_kv, c.head_dim, a.normQ.rms_eps)); /* positions restart with every prompt */
        KF_TRY(kf_attn_prefill_batch(ctx, bq, bk, bv, ba, T, qd, c.n_head, c.n_head_kv, c.head_dim, kvd, S)); /* the rows of a prompt see that prompt's keys only */
        const size_t off = (size_t)l * c.n_ctx * kvd * 2, blk = (size_t)T * kvd * 2;
        KF_TRY(kf_copy_blocks(ctx, pb.d_dst, off, bk, blk, blk, S));
        KF_TRY(kf_copy_blocks(ctx, pb.d_dst + n_seq, off, bv, blk, blk, S));
        KF_TRY(kf_linear(ctx, &wo, ba, bx, nullptr, R, 1.0f, 0.0f, KF_EPI_RESIDUAL, bx));
        KF_TRY(f->ffn[l]->cuFlow(bx, R));
    }
    // the head on every prompt's last row: state {last prompt token, len - 1} -> {picked id, len}, ids out [len - 1] = that id, the row's logits into the slot's
    // (the head matrix -- 311 MB on Qwen3-0.6B -- is read ONCE for all prompts: the last rows normed side by side, one product, one pick launch, one scatter of the logits)
    kf_weight wh = f->head.proj.w->desc();
    const bool together = S > 1 && c.vocab % 8 == 0;
    for (int i = 0; i < S; i++) {
        const int s = slots[i], n = lens[i];
        KF_TRY(kf_set_state(ctx, d_state + 4 * s, tokens[(size_t)i * stride + n - 1], n - 1));
        KF_TRY(kf_memset(ctx, d_state + 4 * s + 3, 0, 4));
        if (together)
            KF_TRY(kf_rmsnorm(ctx, bx + ((size_t)i * T + n - 1) * C, ToX(f->final_norm.w), bn + (size_t)i * C, 1, C, f->final_norm.rms_eps, nullptr));
        else
            KF_TRY(kf_norm_lm_head(ctx, bx + ((size_t)i * T + n - 1) * C, ToX(f->final_norm.w), f->final_norm.rms_eps, &wh, ToX(logits) + (size_t)s * c.vocab, d_state + 4 * s,
                                   d_tokens_out + (size_t)s * c.n_ctx, f->gBUFF.head_ws->data));
    }
    if (together) {
        KF_TRY(kf_linear(ctx, &wh, bn, ToX(pb.bL), nullptr, S, 1.0f, 0.0f, 0u, nullptr));
        KF_TRY(kf_argmax_rows_state(ctx, ToX(pb.bL), c.vocab, c.vocab, S, d_slots, d_state, d_tokens_out, c.n_ctx));
        KF_TRY(kf_copy_blocks(ctx, pb.d_dst + 2 * n_seq, 0, ToX(pb.bL), (size_t)c.vocab * 2, (size_t)c.vocab * 2, S));
    }
    return KF_OK;
}
int XcdReplicas::RunSteps(int n) {
    if (n < 1) return KF_INVALID_ARGS;
    KF_TRY(Fresh());
    KF_TRY(LaunchSteps(n));
    steps_run += n;
    return KF_OK;
}
// A queue of prompts answered through the sequences' slots: what Fish::Chat does round by round over DEBUG.prompts (GoPT.cpp:1111-1180: prefill the prompt, then sample
// until the tokenizer's EOS or the context is full, then the next prompt), with n_seq rounds in flight at once.  A free slot takes the next prompt (Prefill), the launches
// decode every occupied slot, a finished round's slot is parked until the queue refills it; an answer ends at `eos` (eos < 0: never), at max_new ids, or at the last cache
// row.  out [n_req][max_new] (-1 behind an answer's end), out_len [n_req]; every answer equals Fish::Generate's on the same prompt (same prefill, same decode arithmetic).
// With eos >= 0 the ids of each launch are read back (one sync per launch) and a sequence may run up to steps_per_launch - 1 ids past its EOS before its slot is freed --
// those ids are dropped; stats [4] = {launches, steps, prefills, sequence-steps decoded and dropped}.
//
// With a non-greedy sampler (SetSampler: GeneratOnPrompt::Sample, GoPT.cpp:614-630 -- temperature, top-k, top-p, xorshift coin) the launches run ONE step each and leave the
// logits (pick = 0); kf_sample then draws every occupied slot's id from its own logits with the slot's own rng state, seeded at the request's start with seed + request
// index: answer r equals Fish::Generate's on prompt r under SetSampler(seed + r).
int XcdReplicas::Chat(const int32_t* prompts, const int32_t* prompt_len, int n_req, int stride, int max_new, int eos, int32_t* out, int32_t* out_len, long long* stats,
                      const int32_t* max_new_each) {
    const MODEL_CARD& c = hFish->config;
    if (!prompts || !prompt_len || !out || !out_len || n_req < 1 || stride < 1 || max_new < 1) return KF_INVALID_ARGS;
    if (max_new_each)
        for (int r = 0; r < n_req; r++)
            if (max_new_each[r] < 1 || max_new_each[r] > max_new) return KF_INVALID_ARGS;
    const bool sampled = !samp_params.greedy();
    auto draw = [&](int s) -> int {  // the slot's next id from its logits
        return samp_params.Draw(ctx, ToX(logits) + (size_t)s * c.vocab, c.vocab, d_rng + s, d_state + 4 * s, d_tokens_out + (size_t)s * c.n_ctx, d_forced + (size_t)s * c.n_ctx, c.n_ctx);
    };
    for (int r = 0; r < n_req; r++)
        if (prompt_len[r] < 1 || prompt_len[r] > stride || prompt_len[r] >= c.n_ctx) return KF_INVALID_ARGS;
    KF_TRY(Fresh());
    struct Slot { int req = -1, len = 0, want = 0, have = 0; };
    std::vector<Slot> slot(n_seq);
    std::vector<int32_t> row(c.n_ctx);
    long long st[4] = {0, 0, 0, 0};
    int next = 0, done = 0;
    for (int s = 0; s < n_seq; s++) KF_TRY(Park(s, true));
    auto finish = [&](int s, int n_ids) -> int {  // the slot's answer out, the slot parked
        Slot& q = slot[s];
        KF_TRY(kf_d2h(ctx, row.data(), d_tokens_out + (size_t)s * c.n_ctx, (size_t)(q.len - 1 + q.have) * 4));
        for (int i = 0; i < max_new; i++) out[(size_t)q.req * max_new + i] = i < n_ids ? row[q.len - 1 + i] : -1;
        out_len[q.req] = n_ids;
        st[3] += q.have - n_ids;
        q.req = -1, done++;
        return Park(s, true);
    };
    auto serve = [&]() -> int {
        while (done < n_req) {
            for (bool again = true; again && next < n_req;) { /* refill: the free slots take the next prompts -- together (PrefillBatch) when several are free and asked for */
                again = false;
                std::vector<int> fs;
                const int PC = hFish->prefill_chunk; /* rows of one token batch */
                int tmax = 0;
                for (int s = 0; s < n_seq && next + (int)fs.size() < n_req && (int)fs.size() < (prefill_batch > 1 ? prefill_batch : 1); s++) {
                    if (slot[s].req >= 0) continue;
                    const int len = prompt_len[next + (int)fs.size()], t2 = len > tmax ? len : tmax;
                    if (!fs.empty() && (long long)(fs.size() + 1) * t2 > PC) break; /* the batch's rows fit the token-batch buffers */
                    tmax = t2, fs.push_back(s);
                }
                if (fs.empty()) break;
                const int m = (int)fs.size(), r0 = next;
                for (int i = 0; i < m; i++) {
                    Slot& q = slot[fs[i]];
                    q.req = next++, q.len = prompt_len[q.req], q.have = 1;  // the prefill picks the answer's first id
                    const int room = c.n_ctx - q.len;                       // the ids the cache has rows for: the id behind row p needs row p
                    const int asked = max_new_each ? max_new_each[q.req] : max_new; /* a limit of its own per request, or the common one */
                    q.want = asked < room + 1 ? asked : room + 1;
                    KF_TRY(kf_memset32(ctx, d_forced + (size_t)fs[i] * c.n_ctx, -1, (size_t)c.n_ctx)); /* free running */
                }
                if (m > 1)
                    KF_TRY(PrefillBatch(fs.data(), prompts + (size_t)r0 * stride, prompt_len + r0, m, stride));
                else
                    KF_TRY(Prefill(fs[0], prompts + (size_t)r0 * stride, prompt_len[r0]));
                st[2] += m;
                for (int i = 0; i < m; i++) {
                    const int s = fs[i];
                    Slot& q = slot[s];
                    if (sampled) { /* the prefill left the last prompt token's logits in the slot's logits and picked greedily: draw the answer's first id instead */
                        const uint64_t seed = samp_params.seed + (uint64_t)q.req;
                        KF_TRY(kf_set_state(ctx, reinterpret_cast<int32_t*>(d_rng + s), (int)(uint32_t)seed, (int)(uint32_t)(seed >> 32))); /* two words on the stream */
                        KF_TRY(kf_set_state(ctx, d_state + 4 * s, prompts[(size_t)q.req * stride + q.len - 1], q.len - 1));
                        KF_TRY(draw(s));
                    }
                    if (eos >= 0) {
                        int32_t first;
                        KF_TRY(kf_d2h(ctx, &first, d_tokens_out + (size_t)s * c.n_ctx + (q.len - 1), 4));
                        if (first == eos) q.want = 1;
                    }
                    if (q.have >= q.want) { KF_TRY(finish(s, q.want)); continue; }  // a one-id answer: the slot takes another prompt at once
                    KF_TRY(Park(s, false));
                }
                again = true; /* more free slots may be waiting (the batch limit, the buffer's rows, a one-id answer) */
            }
            int k = sampled ? 1 : steps_per_launch, active = 0;
            for (int s = 0; s < n_seq; s++)
                if (slot[s].req >= 0) active++, k = slot[s].want - slot[s].have < k ? slot[s].want - slot[s].have : k;
            if (!active) continue;
            KF_TRY(kf_xengine_steps(ctx, engine.get(), ToX(x), d_state, k, sampled ? 0 : 1));
            if (sampled)
                for (int s = 0; s < n_seq; s++)
                    if (slot[s].req >= 0) KF_TRY(draw(s));
            st[0]++, st[1] += k, steps_run += k;
            for (int s = 0; s < n_seq; s++) {
                Slot& q = slot[s];
                if (q.req < 0) continue;
                const int had = q.have;
                q.have += k;
                int n_ids = q.have >= q.want ? q.want : -1;
                if (eos >= 0) {
                    KF_TRY(kf_d2h(ctx, row.data(), d_tokens_out + (size_t)s * c.n_ctx + (q.len - 1 + had), (size_t)k * 4));
                    for (int i = 0; i < k; i++)
                        if (row[i] == eos) { n_ids = had + i + 1; break; }
                }
                if (n_ids >= 0) KF_TRY(finish(s, n_ids));
            }
        }
        return KF_OK;
    };
    const int rc = serve();
    for (int s = 0; s < n_seq; s++) { /* whatever happened, the object leaves as it came: every slot free running */
        const int r2 = Park(s, false);
        if (rc == KF_OK && r2 != KF_OK) return r2;
    }
    if (stats) for (int i = 0; i < 4; i++) stats[i] = st[i];
    return rc != KF_OK ? rc : Check();
}

// ---- tensor parallel over the XCDs
int XcdTP::Build(Fish** fs, int world) {
    if (!fs || world < 1) return KF_INVALID_ARGS;
    for (int r = 0; r < world; r++)
        if (!fs[r]) return KF_INVALID_ARGS;
    ranks.assign(fs, fs + world);
    Fish* f0 = fs[0];
    ctx = f0->ctx;
    const MODEL_CARD& c = f0->config;
    const int kvd = c.n_head_kv * c.head_dim;
    const size_t rank_elems = (size_t)c.nLayer * c.n_ctx * kvd;
    vocab = 0;
    for (int r = 0; r < world; r++) vocab += fs[r]->config.vocab; /* the logits vector: the shards in rank order */
    KF_TRY(Commit<XcdSeqs>(*this, ctx, c, world, 1, vocab));
    std::vector<std::vector<kf_engine_layer>> Ls(world);
    std::vector<kf_engine_desc> ds(world);
    std::vector<const kf_engine_desc*> dp(world);
    std::vector<kf_weight> heads(world);
    std::vector<const kf_weight*> hp(world);
    std::vector<int32_t> row0(world);
    for (int r = 0, v0 = 0; r < world; v0 += fs[r++]->config.vocab) {
        Fish* f = fs[r];
        const MODEL_CARD& cr = f->config;
        if (cr.nLayer != c.nLayer || cr.n_ctx != c.n_ctx || cr.nEmbed != c.nEmbed || cr.n_head_kv * cr.head_dim != kvd) {
            why = "the ranks' cards disagree";
            return KF_INVALID_ARGS;
        }
        KF_TRY(f->EngineRefusal(why));
        KF_TRY(f->EngineTable(ToX(key) + r * rank_elems, ToX(val) + r * rank_elems, false, why, Ls[r], ds[r])); /* no hot-row masks: the TP form has no sparse FFN */
        ds[r].rope_table = f0->rope_table; /* every rank's descriptor: rank 0's table (n_layer, max_seq and kv_stride agree, checked above) */
        dp[r] = &ds[r];
        if (!f->embed.w || !f->head.proj.w || !f->final_norm.w) {
            why = "embedding / head / final norm missing";
            return KF_ENGINE_NOT_SERVED;
        }
        heads[r] = f->head.proj.w->desc(), hp[r] = &heads[r], row0[r] = v0;
    }
    KF_TRY(EnsureWorkspace(kf_xengine_workspace_bytes_tp(dp[0])));
    kf_xengine* e = nullptr;
    int rc = kf_xengine_create_tp(ctx, dp.data(), world, engine_ws, engine_ws.bytes(), &e);
    if (rc != KF_OK) {
        why = kf_last_error();
        return rc == KF_UNSUPPORTED_DATATYPE ? KF_ENGINE_NOT_SERVED : rc;
    }
    engine.reset(e);
    kf_weight we = f0->embed.w->desc();
    rc = kf_xengine_set_embedding(ctx, engine.get(), &we, d_forced, c.n_ctx);
    if (rc == KF_OK) rc = kf_xengine_set_head_tp(ctx, engine.get(), hp.data(), row0.data(), ToX(f0->final_norm.w), ToX(logits), d_tokens_out, c.n_ctx);
    if (rc != KF_OK) {
        why = kf_last_error();
        return rc == KF_UNSUPPORTED_DATATYPE ? KF_ENGINE_NOT_SERVED : rc;
    }
    built_gen.clear();
    for (int r = 0; r < world; r++) built_gen.push_back(fs[r]->weights_gen);
    return KF_OK;
}
int XcdTP::SetForced(const int32_t* ids, int n) {
    const int n_ctx = ranks[0]->config.n_ctx;
    if (n < 0 || n > n_ctx) return KF_INVALID_ARGS;
    std::vector<int32_t> row(n_ctx, -1);
    for (int i = 0; i < n; i++) row[i] = ids[i];
    return kf_h2d(ctx, d_forced, row.data(), row.size() * 4);
}
int XcdTP::SetState(int token, int pos) {
    if (pos < 0 || pos >= ranks[0]->config.n_ctx || token < 0 || token >= vocab) return KF_INVALID_ARGS;
    return kf_set_state(ctx, d_state, token, pos);
}
int XcdTP::RunSteps(int n) {
    if (!engine || n < 1) return KF_INVALID_ARGS;
    for (size_t r = 0; r < ranks.size(); r++)
        if (r >= built_gen.size() || ranks[r]->weights_gen != built_gen[r]) { /* never a step on stale shards (the engine's tables and its fused q | k | v copy are of the old weights) */
            why = "a rank's weights changed since this engine was built (kfh_weights_changed / a weight set again): destroy it and create it again";
            return KF_INVALID_ARGS;
        }
    return LaunchSteps(n);
}
// the C entry points' create: a built object, or NULL with its refusal in kfh_host_error
template <class T, class... A>
static void* xcd_create(int* rc_out, A... args) {
    T* t = new T();
    const int rc = t->Build(args...);
    if (rc_out) *rc_out = rc;
    if (rc != KF_OK) {
        g_host_err = t->why;
        delete t;
        return nullptr;
    }
    return t;
}

}  // namespace koifish

// ================================================================================================ C entry points
// Flat C surface over the classes above for ctypes (tests, bench.py) -- host-side convenience, not part of the
// kernel ABI.  Handles are koifish::Fish*.
using namespace koifish;
extern "C" {

void* kfh_create(int device, void* stream, int dim, int n_layer, int n_head, int n_kv, int head_dim, int ffn, int vocab, int n_ctx, float rms_eps, float qk_eps,
                 float theta, int* rc_out) {
    Fish* f = new Fish();
    MODEL_CARD c;
    c.nEmbed = dim, c.nLayer = n_layer, c.n_head = n_head, c.n_head_kv = n_kv, c.head_dim = head_dim, c.n_ff = ffn, c.vocab = vocab, c.n_ctx = n_ctx;
    c.rms_eps = rms_eps, c.qk_eps = qk_eps, c.rope_theta = theta;
    int rc = f->Build(c, device, stream);
    if (rc_out) *rc_out = rc;
    if (rc != KF_OK) {
        delete f;
        return nullptr;
    }
    return f;
}
void kfh_destroy(void* h) { delete reinterpret_cast<Fish*>(h); }
const char* kfh_host_error(void) { return g_host_err.c_str(); } /* why the last kfh_create failed */
void* kfh_ctx(void* h) { return reinterpret_cast<Fish*>(h)->ctx; }
int kfh_set_fuse_level(void* h, int lvl) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (lvl == 0) KF_TRY(f->Admit(MODE_FUSE0, "kfh_set_fuse_level", g_host_err));
    f->fuse_level = lvl;
    return KF_OK;
}
// sparse forward: h_hot[ffn] (1 = hot, CS_Picker::hot) for one layer's FFN, NULL = dense again.  The mask becomes a device row list here (load time).
int kfh_set_hot(void* h, int layer, const int32_t* h_hot, int n) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (layer < 0 || layer >= f->config.nLayer) return KF_INVALID_ARGS;
    FFN* m = f->ffn[layer].get();
    if (h_hot && n != f->config.n_ff) return KF_INVALID_ARGS; /* arguments first: a rejected call changes nothing */
    if (h_hot) KF_TRY(f->Admit(MODE_HOT_MASK, "kfh_set_hot", g_host_err)); /* clearing is never refused */
    f->ModeChanged(); /* the engine's layer table, the captured graphs and an XcdReplicas' table hold the masks: rebuilt at their next use; the resident bf16 copies and the
                         measured delays do not depend on them and stay */
    if (!h_hot) {
        if (m->n_hot >= 0) f->masked_layers--;
        m->n_hot = -1, m->hot_rows.reset(), m->hot_mask.reset();
        return KF_OK;
    }
    hGTensor mask = GT(f->ctx, "hot", typNUMBER::I32, n), rows = GT(f->ctx, "hot_rows", typNUMBER::I32, n + 4);
    if (!mask || !rows) return KF_OUTOF_GPUMEMORY;
    KF_TRY(kf_h2d(f->ctx, mask->data, h_hot, (size_t)n * 4));
    int32_t* d_count = reinterpret_cast<int32_t*>(rows->data) + n;
    KF_TRY(kf_hot_rows(f->ctx, reinterpret_cast<const int32_t*>(mask->data), n, reinterpret_cast<int32_t*>(rows->data), d_count));
    int32_t cnt = 0;
    KF_TRY(kf_d2h(f->ctx, &cnt, d_count, 4));
    if (m->n_hot < 0) f->masked_layers++;
    m->hot_rows = rows, m->hot_mask = mask, m->n_hot = cnt;
    return KF_OK;
}
int kfh_n_hot(void* h, int layer) {
    Fish* f = reinterpret_cast<Fish*>(h);
    return (layer < 0 || layer >= f->config.nLayer) ? KF_INVALID_ARGS : f->ffn[layer]->n_hot;
}
// the persistent decode engine: on (default) / off; captured step graphs are dropped so that the next step is captured the new way
int kfh_set_engine(void* h, int on) {
    Fish* f = reinterpret_cast<Fish*>(h);
    f->use_engine = on != 0;
    f->DropGraphs();
    return KF_OK;
}
// int8 activations for the ternary / 1-bit layer matrices: on / off (off: today's routes, bit for bit).  A refusal leaves the switch as it was; kfh_host_error says why.
int kfh_set_act_int8(void* h, int on) { return reinterpret_cast<Fish*>(h)->SetActInt8(false, on != 0, g_host_err); }
// the same for the 4-bit layer matrices (kf_linear_w4a8 / kf_linear_w4a8_tiles): a second switch, independent of kfh_set_act_int8
int kfh_set_act_int8_q4(void* h, int on) { return reinterpret_cast<Fish*>(h)->SetActInt8(true, on != 0, g_host_err); }
// the int8 KV cache: on / off (off: today's routes on the bf16 cache, bit for bit).  The two caches are independent -- switching converts nothing, the caller prefills again.
// A refusal leaves the switch as it was; kfh_host_error says why.  kfh_kv8_*: the int8 pair and its steps on the device (NULL before the first switch-on).
int kfh_set_kv_int8(void* h, int on) { return reinterpret_cast<Fish*>(h)->SetKVInt8(on != 0, g_host_err); }
int kfh_kv_int8(void* h) { return reinterpret_cast<Fish*>(h)->kv_int8 ? 1 : 0; }
// the int8 prompt attention, a sub-setting of the int8 KV cache: off by default, refused (with the reason) unless kfh_set_kv_int8 is on, switched off with it.  On: token
// batches run kf_attn_prefill_kv8 on the int8 rows; off: the dequantise route, bit for bit.
int kfh_set_kv_int8_prefill(void* h, int on) { return reinterpret_cast<Fish*>(h)->SetKVInt8Prefill(on != 0, g_host_err); }
int kfh_kv_int8_prefill(void* h) { return reinterpret_cast<Fish*>(h)->kv_int8_prefill ? 1 : 0; }
// (kf_attn_prefill_kv8 launches, dequantise-route launches) of the token batches since the last reset; reset != 0 zeroes them after the read
int kfh_kv8_route_counts(void* h, int64_t* out2, int reset) {
    if (!h || !out2) return KF_INVALID_ARGS;
    Fish* f = reinterpret_cast<Fish*>(h);
    out2[0] = f->kv8_count[0], out2[1] = f->kv8_count[1];
    if (reset) f->kv8_count[0] = f->kv8_count[1] = 0;
    return KF_OK;
}
void* kfh_kv8_codes(void* h, int val) {
    const KVCache& kc = reinterpret_cast<Fish*>(h)->cache;
    return kc.k8 ? (val ? kc.v8 : kc.k8)->data : nullptr;
}
void* kfh_kv8_steps(void* h, int val) {
    const KVCache& kc = reinterpret_cast<Fish*>(h)->cache;
    return kc.k8 ? (val ? kc.vs : kc.ks)->data : nullptr;
}
// a low-rank adapter beside layer matrix `slot` (0 q, 1 k, 2 v, 3 o, 4 gate, 5 up, 6 down): a [r, in], b [out, r] bf16 DEVICE pointers, no copy (the caller keeps them alive and
// may update them in place: every launch reads them); s multiplies both products, one rank and one s per model.  While any is attached decode, prefill, score and perplexity
// apply it (Fish::Group) on per-layer launches.  A refusal changes nothing; kfh_host_error says why.
int kfh_set_adapter(void* h, int layer, int slot, const void* a, const void* b, int r, float s) {
    return reinterpret_cast<Fish*>(h)->SetAdapter(layer, slot, reinterpret_cast<const floatX*>(a), reinterpret_cast<const floatX*>(b), r, s, g_host_err);
}
int kfh_clear_adapters(void* h) {
    reinterpret_cast<Fish*>(h)->ClearAdapters();
    return KF_OK;
}
int kfh_n_adapters(void* h) { return reinterpret_cast<Fish*>(h)->n_adapters; }
// the token count from which a token batch's ternary / 1-bit matrices take the int8 MFMA tiles (kf_linear_a8_tiles) instead of the mat-vec (kf_linear_a8): n >= 2 sets it,
// 1 is treated as 2 (a single token always takes the mat-vec), 0 restores the default (KF_A8_TILE_MIN), n < 0 = never.  Both routes give the same bits.
int kfh_set_a8_tile_min(void* h, int n) {
    reinterpret_cast<Fish*>(h)->a8_tile_min = n == 0 ? (int)KF_A8_TILE_MIN : n == 1 ? 2 : n < 0 ? -1 : n;
    return KF_OK;
}
// (tile launches, mat-vec launches) of both integer families since the last switch-on of kfh_set_act_int8 / kfh_set_act_int8_q4
int kfh_a8_route_counts(void* h, int64_t* out2) {
    if (!h || !out2) return KF_INVALID_ARGS;
    const Fish* f = reinterpret_cast<Fish*>(h);
    out2[0] = f->a8_count[0], out2[1] = f->a8_count[1];
    return KF_OK;
}
// summation order of the decode kernels (kf_set_canonical): 1 (default) the canonical order shared with the CPU oracle, 0 the v_dot2c forms; captured graphs are dropped
int kfh_set_canonical(void* h, int on) {
    Fish* f = reinterpret_cast<Fish*>(h);
    f->DropGraphs();
    return kf_set_canonical(f->ctx, on);
}
// steps enqueued (or captured) through the engine so far; -1: the engine does not serve this model
int kfh_engine_steps(void* h) {
    Fish* f = reinterpret_cast<Fish*>(h);
    return f->engine_state < 0 ? -1 : f->engine_steps;
}
// diagnostics (scratch/eng_stamps.py, scratch/eng_ab.py): per-phase stamps of one workgroup of the engine; the first-sweep delays of its hand-offs
extern "C" int kfdbg_engine_stamps(kf_engine* e, unsigned long long* h_out, int n_words);
extern "C" int kfdbg_engine_stamps_enable(kf_engine* e, int wg);
extern "C" int kfdbg_engine_set_delays(kf_engine* e, const int* d6);
int kfh_engine_stamps(void* h, unsigned long long* out, int n) {
    Fish* f = reinterpret_cast<Fish*>(h);
    return f->engine ? kfdbg_engine_stamps(f->engine.get(), out, n) : -1;
}
int kfh_engine_stamps_enable(void* h, int wg) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (f->engine_state == 0) f->EnsureEngine();
    f->DropGraphs(); /* captured launches hold the product instantiation */
    return f->engine ? kfdbg_engine_stamps_enable(f->engine.get(), wg) : -1;
}
int kfh_engine_set_delays(void* h, const int* d6) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (f->engine_state == 0) f->EnsureEngine();
    f->DropGraphs();
    return f->engine ? kfdbg_engine_set_delays(f->engine.get(), d6) : -1;
}
// why the engine does not serve this model ("" when it does; valid once a step has been tried or kfh_engine_stamps_enable / kfh_engine_only forced the build)
const char* kfh_engine_why(void* h) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (f->engine_state == 0) f->EnsureEngine();
    return f->engine_why.c_str();
}
// kf_engine_tune at the position the decode state holds; us[0] / us[1] = mean launch time before / after
int kfh_engine_tune(void* h, int passes, float* us2) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (f->engine_state == 0) f->EnsureEngine();
    if (f->engine_state <= 0 || !f->engine_embed) return KF_ENGINE_NOT_SERVED;
    int32_t st[4];
    KF_TRY(kf_d2h(f->ctx, st, f->d_state, 16));
    f->tok_pos = st[1];
    float b = 0.f, a = 0.f;
    const int rc = kf_engine_tune(f->ctx, f->engine.get(), ToX(f->x), f->d_state, f->pos_bound(), passes, &b, &a);
    if (us2) us2[0] = b, us2[1] = a;
    return rc;
}
// resident bf16 copies for long prompts: on (default) / off, and the byte budget above which a model goes without (0 keeps the current one); takes effect at the next Prefill
/* after an IN-PLACE change of weight data this Fish was given as device pointers: every derived copy (resident bf16 copies, the engine's tables, captured graphs) is dropped */
int kfh_weights_changed(void* h) {
    reinterpret_cast<Fish*>(h)->DropEngine();
    return KF_OK;
}
int kfh_set_prefill_resident(void* h, int on, size_t max_bytes) {
    Fish* f = reinterpret_cast<Fish*>(h);
    f->DropResident();
    if (!on) f->DropHeadScreen(); /* the promise is withdrawn: no derived copy of a weight stays */
    f->prefill_resident = on ? 1 : 0;
    if (max_bytes) f->resident_max_bytes = max_bytes;
    return KF_OK;
}
size_t kfh_resident_bytes(void* h) {
    Fish* f = reinterpret_cast<Fish*>(h);
    return f->deq_arena ? kf_dequant_arena_used(f->ctx) : 0;
}
int kfh_set_engine_autotune(void* h, int passes) {
    Fish* f = reinterpret_cast<Fish*>(h);
    f->engine_autotune = passes < 0 ? 0 : passes;
    return KF_OK;
}
// statistics of the engine's hand-offs at `pos` (kf_engine_statistics as 14 ints: sweeps[6], polls, delay[6], tuned)
int kfh_engine_stats(void* h, int pos, int32_t* out14) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (!f->engine) return KF_ENGINE_NOT_SERVED;
    kf_engine_statistics s;
    f->tok_pos = pos;
    KF_TRY(kf_engine_stats(f->ctx, f->engine.get(), f->pos_bound(), &s));
    for (int i = 0; i < 6; i++) out14[i] = s.sweeps[i], out14[7 + i] = s.delay[i];
    out14[6] = s.polls, out14[13] = s.tuned;
    return KF_OK;
}
// the head screen's counters since the engine was built or reset: {screened steps, rows re-ranked, workgroup fall-backs}; zeros without an engine
int kfh_engine_screen_stats(void* h, int64_t* out3) {
    Fish* f = reinterpret_cast<Fish*>(h);
    out3[0] = out3[1] = out3[2] = 0;
    if (!f->engine) return KF_OK;
    kf_engine_screen_statistics s;
    KF_TRY(kf_engine_screen_stats(f->ctx, f->engine.get(), &s));
    out3[0] = s.screened_steps, out3[1] = s.rows_reranked, out3[2] = s.wg_fallbacks;
    return KF_OK;
}
// n launches of the engine alone at the position d_state holds (bench.py times the kernel with events around this); the residual stream is
// re-read from the embedding each time so that the values stay those of a real step
int kfh_engine_only(void* h, int n) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (f->engine_state == 0) f->EnsureEngine();
    if (f->engine_state <= 0) return KF_ENGINE_NOT_SERVED;
    int32_t st[4];
    KF_TRY(kf_d2h(f->ctx, st, f->d_state, 16));
    f->tok_pos = st[1];
    f->graph_mode = true;
    int rc = KF_OK;
    for (int i = 0; i < n && rc == KF_OK; i++) rc = kf_engine_step(f->ctx, f->engine.get(), ToX(f->x), ToX(f->x), f->d_state, f->pos_bound());
    f->graph_mode = false;
    return rc;
}
// synchronises; KF_INTERNAL_ERR when one of the engine's hand-off polls has timed out
int kfh_engine_check(void* h) { return reinterpret_cast<Fish*>(h)->EngineCheck(); }

static SLP* slot_of(Fish* f, int layer, int slot) { return layer >= 0 ? f->LayerMatrix(layer, slot) : slot == 1 ? &f->head.proj : nullptr; }
// the mode table without a device (tests/test_host_modes_cpu.py): mode_refusal / engine_refusal / eager_only for any set of active modes
static int why_out(int rc, const std::string& why, char* out, size_t n) {
    if (out && n) std::snprintf(out, n, "%s", rc != KF_OK ? why.c_str() : "");
    return rc;
}
int kfhdbg_mode_refusal(unsigned active, int asked, char* why, size_t n) {
    if (asked < 0 || asked >= N_MODES) return why_out(KF_INVALID_ARGS, "kfhdbg: no such mode", why, n);
    std::string w;
    return why_out(mode_refusal(active, (Mode)asked, "kfhdbg", w), w, why, n);
}
int kfhdbg_engine_refusal(unsigned active, char* why, size_t n) {
    std::string w;
    return why_out(engine_refusal(active, w), w, why, n);
}
int kfhdbg_eager_only(unsigned active) { return eager_only(active) ? 1 : 0; }

// slot: 0 q,1 k,2 v,3 o,4 gate,5 up,6 down (layer >= 0); layer = -1: slot 0 embed_tokens, 1 lm_head.
// Either a host blob (`data||gama`, copied to a fresh device allocation) or an existing device pointer.
static int set_weight_impl(void* h, int layer, int slot, int type, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device, int lGroup,
                           int qMin, int qMax, int qBias, bool normal_float);
int kfh_set_weight(void* h, int layer, int slot, int type, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device, int lGroup,
                   int qMin, int qMax, int qBias) {
    return set_weight_impl(h, layer, slot, type, ne0, ne1, blob, blob_bytes, szData, is_device, lGroup, qMin, qMax, qBias, false);
}
// the same for a tensor whose quant card says isNormalFloat (QUANT_MODE::RTNf): Q4 nibble stream || gama with a 16-entry table per row
int kfh_set_weight_lut(void* h, int layer, int slot, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device) {
    return set_weight_impl(h, layer, slot, (int)typNUMBER::Q4, ne0, ne1, blob, blob_bytes, szData, is_device, 0, 0, 15, 0, true);
}
// ... at `bits` per weight: 4 as above; 3 (RT_NormalF with bits == 3: an 8-entry table per row) for layer matrices only -- TokenEmbed::cuInfer asserts on Q3 and the LM
// head forms do not unpack it.  A Fish holding such a matrix multiplies it from the packed stream: kf_set_row_unpack goes on for its own context (there is no earlier
// behaviour to keep: the fused decode entries refused the storage)
int kfh_set_weight_lut_bits(void* h, int layer, int slot, int bits, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device) {
    if (bits == 4) return kfh_set_weight_lut(h, layer, slot, ne0, ne1, blob, blob_bytes, szData, is_device);
    if (bits != 3) {
        g_host_err = "kfh_set_weight_lut_bits: normal-float row codebooks exist at 4 and 3 bits (RT_NormalF)";
        return KF_UNSUPPORTED_DATATYPE;
    }
    if (layer < 0) {
        g_host_err = "kfh_set_weight_lut_bits: the embedding and the LM head stay bf16 or 4-bit (TokenEmbed::cuInfer asserts on Q3; no 3-bit head mat-vec): NF3 is for layer matrices";
        return KF_UNSUPPORTED_DATATYPE;
    }
    if (ne1 % 128 != 0 || ne0 % 8 != 0) {
        g_host_err = "kfh_set_weight_lut_bits: a 3-bit layer matrix needs ne1 % 128 == 0 and ne0 % 8 == 0 (whole 32-weight units per lane, 16-byte aligned row tables)";
        return KF_BLAS_UNALIGN;
    }
    Fish* f = reinterpret_cast<Fish*>(h);
    const int rc = set_weight_impl(h, layer, slot, (int)typNUMBER::Q3, ne0, ne1, blob, blob_bytes, szData, is_device, 0, 0, 7, 0, true);
    return rc != KF_OK ? rc : kf_set_row_unpack(f->ctx, 1);
}
static int set_weight_impl(void* h, int layer, int slot, int type, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device, int lGroup,
                           int qMin, int qMax, int qBias, bool normal_float) {
    Fish* f = reinterpret_cast<Fish*>(h);
    auto t = std::make_shared<GTensor>();
    t->type = (typNUMBER)type, t->ne[0] = ne0, t->ne[1] = ne1;
    t->szData = szData, t->szGama = blob_bytes - szData;
    t->quant.T_group = lGroup, t->quant.qMin = qMin, t->quant.qMax = qMax, t->quant.qBias = qBias;
    t->quant.isNormalFloat = normal_float;
    KF_TRY(t->Take(f->ctx, blob, blob_bytes, is_device != 0));
    f->DropEngine(); /* the engine's device table (and every captured graph) holds the old tensors' addresses */
    if (layer < 0 && slot == 0) {
        f->embed.w = t;
        return KF_OK;
    }
    SLP* s = slot_of(f, layer, slot);
    if (!s) return KF_INVALID_ARGS;
    if (s->lora_a) { /* the pair beside it was checked against the old matrix's sides */
        g_host_err = "kfh_set_weight: the matrix carries a low-rank adapter: clear the adapters first";
        return KF_INVALID_ARGS;
    }
    s->w = t, s->nOut = ne0, s->nIn = ne1;
    return f->EnsureLinearScratch(t->desc(), f->prefill_chunk); /* load time: the launches themselves never allocate */
}
// tie_word_embeddings: lm_head shares embed_tokens' tensor (Neuron.cpp:349-356)
int kfh_tie_head(void* h) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (!f->embed.w) return KF_INVALID_ARGS;
    f->DropEngine();
    f->head.proj.w = f->embed.w, f->head.proj.nOut = f->embed.w->ne[0], f->head.proj.nIn = f->embed.w->ne[1];
    return KF_OK;
}
// slot: 0 input_layernorm, 1 post_attention_layernorm, 2 q_norm, 3 k_norm; layer = -1: final norm.  bf16 [n]
int kfh_set_norm(void* h, int layer, int slot, const void* w, int n, int is_device) {
    Fish* f = reinterpret_cast<Fish*>(h);
    auto t = std::make_shared<GTensor>();
    t->type = typNUMBER::BF16, t->ne[0] = n, t->szData = (size_t)n * 2;
    KF_TRY(t->Take(f->ctx, w, (size_t)n * 2, is_device != 0));
    f->DropEngine();
    if (layer < 0) {
        f->final_norm.w = t;
        return KF_OK;
    }
    if (layer >= f->config.nLayer) return KF_INVALID_ARGS;
    SelfAttention* a = f->attn[layer].get();
    switch (slot) {
        case 0: a->norm.w = t; break;
        case 1: f->ffn[layer]->norm.w = t; break;
        case 2: a->normQ.w = t; break;
        case 3: a->normK.w = t; break;
        default: return KF_INVALID_ARGS;
    }
    return KF_OK;
}

// one eager step; logits (bf16[vocab]) and hidden copied to host when non-null; returns the greedy id or < 0
int kfh_forward(void* h, int token, int pos, uint16_t* h_logits) {
    Fish* f = reinterpret_cast<Fish*>(h);
    int rc = f->ForwardOnRLS(token, pos);
    if (rc != KF_OK) return rc;
    int32_t st[4];
    rc = kf_d2h(f->ctx, st, f->d_state, 16);
    if (rc != KF_OK) return rc;
    if (h_logits) {
        rc = kf_d2h(f->ctx, h_logits, f->head.preLogits->data, (size_t)f->config.vocab * 2);
        if (rc != KF_OK) return rc;
    }
    return f->fuse_level == 0 ? st[2] : st[0];
}
// the verify pass (Fish::Verify): n = 1 .. 8 tokens at positions pos0 .., top1_out [n] int32, logits_out [n][vocab] bf16 or NULL.  A refusal: kfh_host_error says why
int kfh_verify(void* h, const int* tokens, int n, int pos0, int* top1_out, uint16_t* logits_out) {
    return reinterpret_cast<Fish*>(h)->Verify(tokens, n, pos0, top1_out, reinterpret_cast<floatX*>(logits_out), g_host_err);
}
// speculative decoding (koifish::SpecDecoder): handles are SpecDecoder*.  The drafter is the lookup drafter until one of the setters names another
void* kfh_spec_create(void* target, int k) {
    if (!target || k < 1 || k > KF_SPEC_MAX_K) {
        g_host_err = "kfh_spec_create: a target and k in 1 .. 7";
        return nullptr;
    }
    SpecDecoder* s = new SpecDecoder();
    s->target = reinterpret_cast<Fish*>(target), s->k = k;
    s->rows_shared = -s->target->verify_rows[0], s->rows_single = -s->target->verify_rows[1]; /* the target's counts when the decoder began */
    return s;
}
void kfh_spec_destroy(void* s) { delete reinterpret_cast<SpecDecoder*>(s); }
int kfh_spec_set_lookup(void* s, int ngram) {
    if (!s || ngram < 1) return KF_INVALID_ARGS;
    SpecDecoder* d = reinterpret_cast<SpecDecoder*>(s);
    d->kind = 0, d->ngram = ngram;
    return KF_OK;
}
int kfh_spec_set_draft_model(void* s, void* fish) {
    if (!s || !fish) return KF_INVALID_ARGS;
    SpecDecoder* d = reinterpret_cast<SpecDecoder*>(s);
    d->kind = 1, d->draft = reinterpret_cast<Fish*>(fish);
    return KF_OK;
}
int kfh_spec_set_callback(void* s, SpecDecoder::DraftFn fn, void* user) {
    if (!s || !fn) return KF_INVALID_ARGS;
    SpecDecoder* d = reinterpret_cast<SpecDecoder*>(s);
    d->kind = 2, d->fn = fn, d->user = user;
    return KF_OK;
}
int kfh_spec_generate(void* s, const int* prompt, int n_prompt, int n_new, int* out) {
    return s ? reinterpret_cast<SpecDecoder*>(s)->Generate(prompt, n_prompt, n_new, out, g_host_err) : KF_INVALID_ARGS;
}
// {rounds, ids proposed, ids accepted, activation rows of the verify passes served with the shared unpack, ... served row by row}, since the decoder exists
int kfh_spec_stats(void* s, int64_t* out5) {
    if (!s || !out5) return KF_INVALID_ARGS;
    const SpecDecoder* d = reinterpret_cast<SpecDecoder*>(s);
    out5[0] = d->rounds, out5[1] = d->proposed, out5[2] = d->accepted, out5[3] = d->rows_shared + d->target->verify_rows[0], out5[4] = d->rows_single + d->target->verify_rows[1];
    return KF_OK;
}
// the rules of kf_spec.hpp without a device (tests/test_spec_cpu.py)
int kfhdbg_spec_clip_k(int k, int n_left, int pos, int n_ctx) { return spec_clip_k(k, n_left, pos, n_ctx); }
int kfhdbg_spec_accept(const int* drafts, int k, const int* top1) { return spec_accept(drafts, k, top1); }
int kfhdbg_spec_lookup(const int* ids, int n, int ngram, int k, int* out) { return spec_lookup(ids, n, ngram, k, out); }
int kfhdbg_verify_refusal(unsigned active, int greedy, char* why, size_t n) {
    std::string w;
    return why_out(verify_refusal(active, greedy != 0, "kfhdbg", w), w, why, n);
}
int kfh_generate(void* h, const int* prompt, int n_prompt, int n_new, int* out, int use_graph) {
    return reinterpret_cast<Fish*>(h)->Generate(prompt, n_prompt, n_new, out, use_graph != 0);
}
int kfh_set_forced(void* h, const int32_t* forced, int n) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (n > f->config.n_ctx) return KF_INVALID_ARGS;
    return kf_h2d(f->ctx, f->d_forced, forced, (size_t)n * 4);
}
int kfh_prefill(void* h, const int* tokens, int n, int pos0) { return reinterpret_cast<Fish*>(h)->Prefill(tokens, n, pos0); }
// Fish_ppl / Fish::Eval_ppl as a batch (Fish::Score, Fish::EvalPPL): logprob_out [n - 1] fp32, top1_out [n - 1] int32 or NULL
int kfh_score(void* h, const int* tokens, int n, int pos0, float* logprob_out, int* top1_out) { return reinterpret_cast<Fish*>(h)->Score(tokens, n, pos0, logprob_out, top1_out); }
int kfh_eval_ppl(void* h, const int* tokens, long long n, int window, double* ppl, double* pplerr, long long* n_scored) {
    return reinterpret_cast<Fish*>(h)->EvalPPL(tokens, n, window, ppl, pplerr, n_scored);
}
int kfh_set_prefill_mode(void* h, int mode, int chunk) {
    Fish* f = reinterpret_cast<Fish*>(h);
    f->prefill_mode = mode;
    if (chunk > 0 && !f->gBUFF.bX) f->prefill_chunk = chunk;
    return KF_OK;
}
int kfh_set_sampler(void* h, float temperature, float top_p, int top_k, uint64_t seed) {
    return reinterpret_cast<Fish*>(h)->SetSampler(CHAT_SAMPLER::FromArgs(temperature, top_p, top_k, seed));
}
int kfh_set_state(void* h, int token, int pos) { return reinterpret_cast<Fish*>(h)->SetState(token, pos); }
int kfh_run_steps(void* h, int pos, int n, int use_graph) { return reinterpret_cast<Fish*>(h)->RunSteps(pos, n, use_graph != 0); }
int kfh_sync(void* h) { return kf_sync(reinterpret_cast<Fish*>(h)->ctx); }
// the ids of the steps run so far; KF_INTERNAL_ERR (once) when a hand-off of the persistent engine timed out since the last check: the ids behind the failure are not valid
int kfh_get_tokens(void* h, int32_t* out, int n) {
    Fish* f = reinterpret_cast<Fish*>(h);
    KF_TRY(f->EngineCheck());
    return kf_d2h(f->ctx, out, f->d_tokens_out, (size_t)n * 4);
}
void* kfh_kcache(void* h) { return reinterpret_cast<Fish*>(h)->cache.key->data; }
void* kfh_vcache(void* h) { return reinterpret_cast<Fish*>(h)->cache.val->data; }
void* kfh_logits(void* h) { return reinterpret_cast<Fish*>(h)->head.preLogits->data; }
void* kfh_hidden(void* h) { return reinterpret_cast<Fish*>(h)->x->data; }
// ---- tensor parallel
int kfh_tp_init(void* h, int rank, int world, int vocab_row0) { return reinterpret_cast<Fish*>(h)->TPInit(rank, world, vocab_row0); }
void* kfh_tp_area(void* h) { return reinterpret_cast<Fish*>(h)->tp.area.get(); }
int kfh_tp_set_peer(void* h, int r, void* area) { return reinterpret_cast<Fish*>(h)->TPSetPeer(r, area); }
int kfh_tp_export(void* h, unsigned char* handle64) {
    Fish* f = reinterpret_cast<Fish*>(h);
    return f->tp.area ? kf_tp_ipc_export(f->ctx, f->tp.area, handle64) : KF_INVALID_ARGS;
}
int kfh_tp_open_peer(void* h, int r, const unsigned char* handle64) {
    Fish* f = reinterpret_cast<Fish*>(h);
    void* p = nullptr;
    KF_TRY(kf_tp_ipc_open(f->ctx, handle64, &p));
    f->tp.opened.push_back(p);
    return f->TPSetPeer(r, p);
}
// synchronises; KF_INTERNAL_ERR when a poll of this rank ran out of spins (a peer never pushed)
int kfh_tp_check(void* h) {
    Fish* f = reinterpret_cast<Fish*>(h);
    if (f->tp.world < 2) return KF_OK;
    KF_TRY(kf_sync(f->ctx));
    int32_t e = 0;
    KF_TRY(kf_d2h(f->ctx, &e, f->tp.comm.d_err, 4));
    return e == 0 ? KF_OK : KF_INTERNAL_ERR;
}
// R ranks of this process (all on the stream of rank 0) run n decode steps from `pos` in lock-step; tokens / positions come from each rank's d_state
int kfh_tp_group_run(void** hs, int R, int pos, int n, int use_graph) {
    if (R < 2 || R > 8) return KF_INVALID_ARGS;
    Fish* fs[8];
    for (int r = 0; r < R; r++) {
        fs[r] = reinterpret_cast<Fish*>(hs[r]);
        if (fs[r]->tp.world != R || fs[r]->tp.rank != r) return KF_INVALID_ARGS;
    }
    if (pos < 0 || pos + n > fs[0]->config.n_ctx) return KF_INVALID_ARGS;
    for (int r = 0; r < R; r++) KF_TRY(fs[r]->TPCommit());
    auto& graphs = fs[0]->tp.group_graphs;
    for (int i = 0; i < n; i++) {
        for (int r = 0; r < R; r++) fs[r]->tok_pos = pos + i, fs[r]->graph_mode = true;
        int rc = KF_OK;
        if (use_graph) {
            const int b = bucket_of(pos + i);
            if ((int)graphs.size() <= b) graphs.resize(b + 1);
            if (!graphs[b]) rc = Capture(fs[0]->ctx, graphs[b], [&] { return tp_group_enqueue(fs, R); });
            if (rc == KF_OK) rc = kf_graph_launch(fs[0]->ctx, graphs[b].get());
        } else {
            rc = tp_group_enqueue(fs, R);
        }
        for (int r = 0; r < R; r++) fs[r]->graph_mode = false;
        KF_TRY(rc);
    }
    return KF_OK;
}

// ---- XCD engines: handles are koifish::XcdReplicas* / koifish::XcdTP*
void* kfh_xr_create(void* fish, int n_seq, int* rc_out) { return xcd_create<XcdReplicas>(rc_out, reinterpret_cast<Fish*>(fish), n_seq); }
void kfh_xr_destroy(void* h) { delete reinterpret_cast<XcdReplicas*>(h); }
int kfh_xr_set_forced(void* h, int seq, const int32_t* ids, int n) { return reinterpret_cast<XcdReplicas*>(h)->SetForced(seq, ids, n); }
int kfh_xr_set_state(void* h, int seq, int token, int pos) { return reinterpret_cast<XcdReplicas*>(h)->SetState(seq, token, pos); }
int kfh_xr_prefill(void* h, int seq, const int* tokens, int n) { return reinterpret_cast<XcdReplicas*>(h)->Prefill(seq, tokens, n); }
int kfh_xr_run_steps(void* h, int n) { return reinterpret_cast<XcdReplicas*>(h)->RunSteps(n); }
int kfh_xr_check(void* h) { return reinterpret_cast<XcdReplicas*>(h)->Check(); }
int kfh_xr_park(void* h, int seq, int on) { return reinterpret_cast<XcdReplicas*>(h)->Park(seq, on != 0); }
int kfh_xr_prefill_batch(void* h, const int* slots, const int32_t* tokens, const int* lens, int S, int stride) {
    return reinterpret_cast<XcdReplicas*>(h)->PrefillBatch(slots, tokens, lens, S, stride);
}
int kfh_xr_set_prefill_batch(void* h, int n) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    if (n < 1 || n > r->n_seq) return KF_INVALID_ARGS;
    r->prefill_batch = n;
    return KF_OK;
}
int kfh_xr_set_sampler(void* h, float temperature, float top_p, int top_k, uint64_t seed) {
    return reinterpret_cast<XcdReplicas*>(h)->SetSampler(CHAT_SAMPLER::FromArgs(temperature, top_p, top_k, seed));
}
int kfh_xr_chat(void* h, const int32_t* prompts, const int32_t* prompt_len, int n_req, int stride, int max_new, int eos, int32_t* out, int32_t* out_len, long long* stats) {
    return reinterpret_cast<XcdReplicas*>(h)->Chat(prompts, prompt_len, n_req, stride, max_new, eos, out, out_len, stats);
}
// max_new_each [n_req] (or NULL): request r's own limit, <= max_new (the width of out's rows)
int kfh_xr_chat_each(void* h, const int32_t* prompts, const int32_t* prompt_len, int n_req, int stride, int max_new, int eos, int32_t* out, int32_t* out_len, long long* stats,
                     const int32_t* max_new_each) {
    return reinterpret_cast<XcdReplicas*>(h)->Chat(prompts, prompt_len, n_req, stride, max_new, eos, out, out_len, stats, max_new_each);
}
int kfh_xr_status(void* h, int seq, int32_t* out4) { return reinterpret_cast<XcdReplicas*>(h)->Status(seq, out4); }
int kfh_xr_set_steps_per_launch(void* h, int n) { return reinterpret_cast<XcdReplicas*>(h)->SetStepsPerLaunch(n); }
int kfh_xr_get_tokens(void* h, int seq, int32_t* out, int n) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    if (seq < 0 || seq >= r->n_seq || n < 0 || n > r->hFish->config.n_ctx) return KF_INVALID_ARGS;
    return kf_d2h(r->ctx, out, r->d_tokens_out + (size_t)seq * r->hFish->config.n_ctx, (size_t)n * 4);
}
int kfh_xr_get_state(void* h, int seq, int32_t* out2) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    if (seq < 0 || seq >= r->n_seq) return KF_INVALID_ARGS;
    return kf_d2h(r->ctx, out2, r->d_state + 4 * seq, 8);
}
void* kfh_xr_logits(void* h, int seq) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    return ToX(r->logits) + (size_t)seq * r->hFish->config.vocab;
}
void* kfh_xr_hidden(void* h, int seq) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    return ToX(r->x) + (size_t)seq * r->hFish->config.nEmbed;
}
void* kfh_xr_kcache(void* h, int seq) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    return ToX(r->key) + (size_t)seq * r->kv_seq_elems();
}
void* kfh_xr_vcache(void* h, int seq) {
    XcdReplicas* r = reinterpret_cast<XcdReplicas*>(h);
    return ToX(r->val) + (size_t)seq * r->kv_seq_elems();
}
void* kfh_xtp_create(void** fishes, int world, int* rc_out) { return xcd_create<XcdTP>(rc_out, reinterpret_cast<Fish**>(fishes), world); }
void kfh_xtp_destroy(void* h) { delete reinterpret_cast<XcdTP*>(h); }
int kfh_xtp_set_forced(void* h, const int32_t* ids, int n) { return reinterpret_cast<XcdTP*>(h)->SetForced(ids, n); }
int kfh_xtp_set_state(void* h, int token, int pos) { return reinterpret_cast<XcdTP*>(h)->SetState(token, pos); }
int kfh_xtp_run_steps(void* h, int n) { return reinterpret_cast<XcdTP*>(h)->RunSteps(n); }
int kfh_xtp_check(void* h) { return reinterpret_cast<XcdTP*>(h)->Check(); }
int kfh_xtp_set_steps_per_launch(void* h, int n) { return reinterpret_cast<XcdTP*>(h)->SetStepsPerLaunch(n); }
int kfh_xtp_get_tokens(void* h, int32_t* out, int n) {
    XcdTP* t = reinterpret_cast<XcdTP*>(h);
    if (n < 0 || n > t->ranks[0]->config.n_ctx) return KF_INVALID_ARGS;
    return kf_d2h(t->ctx, out, t->d_tokens_out, (size_t)n * 4);
}
int kfh_xtp_vocab(void* h) { return reinterpret_cast<XcdTP*>(h)->vocab; }
void* kfh_xtp_logits(void* h) { return ToX(reinterpret_cast<XcdTP*>(h)->logits); }
void* kfh_xtp_hidden(void* h) { return ToX(reinterpret_cast<XcdTP*>(h)->x); }
void* kfh_xtp_kcache(void* h) { return ToX(reinterpret_cast<XcdTP*>(h)->key); }
void* kfh_xtp_vcache(void* h) { return ToX(reinterpret_cast<XcdTP*>(h)->val); }
extern "C" int kfdbg_xengine_variant(kf_xengine* e, int nwv, int depth);
extern "C" int kfdbg_xengine_stamps_enable(kf_xengine* e, int seq, int wg, int max_steps);
extern "C" int kfdbg_xengine_stamps(kf_xengine* e, unsigned long long* h_out, int n_words);
int kfh_xtp_stamps_enable(void* h, int rank, int wg, int max_steps) { return kfdbg_xengine_stamps_enable(reinterpret_cast<XcdTP*>(h)->engine.get(), rank, wg, max_steps); }
int kfh_xtp_stamps(void* h, unsigned long long* out, int n) { return kfdbg_xengine_stamps(reinterpret_cast<XcdTP*>(h)->engine.get(), out, n); }
int kfh_xr_variant(void* h, int nwv, int depth) { return kfdbg_xengine_variant(reinterpret_cast<XcdReplicas*>(h)->engine.get(), nwv, depth); }
int kfh_xr_stamps_enable(void* h, int seq, int wg, int max_steps) { return kfdbg_xengine_stamps_enable(reinterpret_cast<XcdReplicas*>(h)->engine.get(), seq, wg, max_steps); }
int kfh_xr_stamps(void* h, unsigned long long* out, int n) { return kfdbg_xengine_stamps(reinterpret_cast<XcdReplicas*>(h)->engine.get(), out, n); }

int kfh_num_graphs(void* h) {
    int n = 0;
    for (const auto& g : reinterpret_cast<Fish*>(h)->graphs) n += g != nullptr;
    return n;
}
}
