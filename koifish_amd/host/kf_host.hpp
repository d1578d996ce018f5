// kf_host.hpp -- host side of the decode path, ABOVE the C ABI (include/kf_abi.h): a C++ mirror of the
// reference's neuron / tensor interface for this path.  Class and method names, argument meaning and error
// behaviour follow gruai/koifish so that a maintainer can read one against the other:
//   GTensor            src/Tensor/GTensor.hpp:168-490        (data||gama blob, type, ne[], quant card)
//   KVCache            src/Utils/Cache.{hpp,cpp}:14-57       ([n_layer, max_seq, kv_dim] bf16 pair)
//   LayerNormal::cuFlow src/Manifold/Neuron.hpp:438-458, src/Device/CUDA/T.cu:561-573
//   SLP::Forw          src/Manifold/Neuron.hpp:397-430, src/Device/CUDA/NeuronFuse.cu:305-381
//   ROPE::cuInfer      src/Device/CUDA/kernel/rope.cu:645-672
//   SelfAttention::cuInfer / _devQKV   src/Device/CUDA/QKV.cu:617-702, src/Manifold/TGraph.cpp:198-207
//   FFN::cuInfer       src/Device/CUDA/NeuronFuse.cu:615-656
//   TokenEmbed::cuInfer src/Device/CUDA/NeuronFuse.cu:176-218
//   Head4Token::cuInfer_1 src/Device/CUDA/NeuronFuse.cu:842-862
//   Fish::ForwardOnRLS / Chat  src/Manifold/gLLM.cpp:722-787, src/Manifold/GoPT.cpp:1111-1235
// No HIP headers here: device memory and launches go through the kf_* C ABI only (plain g++ builds this file).
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kf_abi.h"
#include "kf_devbuf.hpp"
#include "kf_host_modes.hpp"
#include "kf_spec.hpp"

namespace koifish {

using floatX = kf_bf16;
enum class typNUMBER : uint8_t { F32 = 0, F64, F16, BF16, F8E5M2, F8E4M3, U8, I8, U16, I16, U32, I32, U64, I64, Q4, Q3, Q2, T_SIGN, T_SEQ, BOOL1, T_BINARY };

struct Fish;

// kf_graph / kf_engine / kf_xengine handles: destroyed by these deleters only.  A deleter does not synchronise: where an engine may still run, kf_sync stands at that site.
template <auto Destroy>
struct HandleDel {
    template <class H>
    void operator()(H* h) const { Destroy(h); }
};
using hGraph = std::unique_ptr<kf_graph, HandleDel<kf_graph_destroy>>;
using hEngine = std::unique_ptr<kf_engine, HandleDel<kf_engine_destroy>>;
using hXEngine = std::unique_ptr<kf_xengine, HandleDel<kf_xengine_destroy>>;

#define KF_TRY(expr)                 \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != KF_OK) return rc_; \
    } while (0)

// Quant card fields that cross the kernel seam (QUANT_CARD / GeQuant, GeQuant.cpp:107-124)
struct QuantCard {
    int bits = 16, T_group = 128, qMin = 0, qMax = 0, qBias = 0;
    bool isNormalFloat = false;  // QUANT_MODE::RTNf (GeQuant.cpp:853): row-codebook storage -> kf_weight.quant = KF_QUANT_ROW_LUT
};

// A device tensor: `data||gama` in one allocation, as huTensor::Alloc lays it out (GTensor.cpp:456-510).
struct GTensor {
    std::string name;
    DevBuf<> mem;          // the allocation, when this tensor owns one (Alloc / LoadBlob); empty for a caller's device pointer
    void* data = nullptr;  // the view the kernels read: mem's block, a caller's pointer, or -- for the length of XcdReplicas::Prefill -- a sequence's rows
    size_t szData = 0, szGama = 0;
    typNUMBER type = typNUMBER::BF16;
    int ne[4] = {1, 1, 1, 1};
    QuantCard quant;
    kf_ctx* ctx = nullptr;
    std::shared_ptr<GTensor> qZero, qScale;  // vendor AutoAWQ tensors (GeQuant.cpp:410): data = qweight [in, out/8]; ne = {out, in}

    size_t size() const { return (size_t)ne[0] * ne[1] * ne[2] * ne[3]; }
    int nGroup() const { return (szGama && quant.T_group > 0) ? (int)(size() / quant.T_group) : 0; }
    floatX* gama_T() const { return szGama ? reinterpret_cast<floatX*>(reinterpret_cast<uint8_t*>(data) + szData) : nullptr; }
    kf_weight desc() const;  // what TASKA_quant / TASKA_AxB hand to the kernels
    // SerialGamaData H2D (huTensor.cu:413-458): allocate and copy a host `data||gama` blob
    int LoadBlob(kf_ctx* c, const void* h_blob, size_t nbytes);
    int Alloc(kf_ctx* c, size_t nbytes);
    int Take(kf_ctx* c, const void* blob, size_t nbytes, bool is_device) {  // a caller's device pointer as the view (not owned), or LoadBlob of a host blob
        return is_device ? (ctx = c, data = const_cast<void*>(blob), KF_OK) : LoadBlob(c, blob, nbytes);
    }
};
using hGTensor = std::shared_ptr<GTensor>;
hGTensor GT(kf_ctx* c, const std::string& name, typNUMBER tp, int n0, int n1 = 1);  // zero-filled [n1][n0] of a whole-byte type; NULL when refused
inline floatX* ToX(const hGTensor& t) { return t ? reinterpret_cast<floatX*>(t->data) : nullptr; }

struct KVCache {
    enum CTYPE { KV_KEY = 0, KV_VAL };
    hGTensor key, val;
    int n_layer = 0, max_seq_len = 0, kv_dim = 0;
    int Init(kf_ctx* c, int n_layer, int max_seq, int kv_dim);
    void* Get(CTYPE type, int layer, int pos) const;  // Cache.cpp:42-57
    // the int8 pair (include/kf_abi.h "int8 KV cache"; the reference's DEBUG.T_kvcache_quant, QKV.cu:664): k8 / v8 int8 [n_layer, max_seq, kv_dim], ks / vs fp32
    // [n_layer, max_seq, n_kv], zero-filled; stage_k / stage_v bf16 [max_seq, kv_dim]: the rows a token batch attends to (its own rows, then every row dequantised).
    // Allocated by the first switch-on (Fish::SetKVInt8) and kept; the bf16 pair above stays allocated beside it (engine tables and captured graphs hold its addresses).
    hGTensor k8, v8, ks, vs, stage_k, stage_v;
    int n_kv = 0;
    int Init8(kf_ctx* c, int n_kv);
    int8_t* Codes(CTYPE type, int layer) const { return reinterpret_cast<int8_t*>((type == KV_KEY ? k8 : v8)->data) + (size_t)layer * max_seq_len * kv_dim; }
    float* Steps(CTYPE type, int layer) const { return reinterpret_cast<float*>((type == KV_KEY ? ks : vs)->data) + (size_t)layer * max_seq_len * n_kv; }
};

struct GeNeuron {
    std::string name;
    Fish* hFish = nullptr;
    int layid = 0;  // 1-based like the reference (hCache->Get(.., layid - 1, 0))
    virtual ~GeNeuron() {}
};

struct LayerNormal : GeNeuron {
    hGTensor w, out;
    float rms_eps = 1e-6f;
    int nHead = 0, ldTH = 0;
    hGTensor cuFlow(hGTensor inpDelta, int flag = 0);
};

struct Relu : GeNeuron {
    int Forw(hGTensor out, hGTensor gate, hGTensor inp, int flag = 0);  // CU_swiglu_v0
};

struct SLP : GeNeuron {
    hGTensor w, b, out;
    int nIn = 0, nOut = 0;
    const floatX *lora_a = nullptr, *lora_b = nullptr;  // a [r, nIn], b [nOut, r] of a low-rank adapter beside w (Fish::SetAdapter: the caller's device memory), or none
    bool Empty() const { return !w; }
    // rhs = W.lhs (+b);  returns 0 or -1 like the reference (NeuronFuse.cu:305-381)
    int Forw(hGTensor rhs, hGTensor lhs, hGTensor toGelu = nullptr, Relu* hRelu = nullptr, int flag = 0);
    int Forw(floatX* rhs, const floatX* lhs, uint32_t epilogue = 0, const floatX* residual = nullptr);
};

struct SelfAttention;
struct ROPE : GeNeuron {
    LayerNormal *hnQ = nullptr, *hnK = nullptr;
    int n_head = 0, n_head_kv = 0, head_dim = 0;
    float theta = 1e6f;
    hGTensor cuInfer(SelfAttention* hQKV, uint32_t seed, int pos, int flag = 0);
};

struct SelfAttention : GeNeuron {
    LayerNormal norm, normQ, normK;
    SLP Q, K, V, proj_cat;
    ROPE rope;
    KVCache* hCache = nullptr;
    hGTensor out;
    int n_head = 0, n_head_kv = 0, head_dim = 0, q_dim = 0, kv_dim = 0;
    bool isSeparateQKV = true;
    void _devQKV(int pos);  // K.out / V.out alias the KV-cache row (TGraph.cpp:198-207)
    hGTensor cuInfer(hGTensor inpL, int flag = 0);
    // n tokens at positions pos0.. in one pass (the forward of SelfAttention::cuFlow, NeuronFuse.cu:692-731, with the decode arithmetic)
    int cuFlow(floatX* bx, int pos0, int n);
};

struct FFN : GeNeuron {
    LayerNormal norm;
    SLP gate, up, down;
    Relu relu;
    hGTensor out;
    int latent = 0;
    // sparse forward (CS_Picker::hot, SparseNeuron.cpp:20-29): the hot rows of gate / up as a device list; n_hot < 0 = dense
    hGTensor hot_rows, hot_mask;  // hot_mask: CS_Picker's hot[ffn] itself on the device (the persistent engine reads the mask, the per-layer launches the list)
    int n_hot = -1;
    hGTensor cuInfer(hGTensor hIn, int flag = 0);
    int cuFlow(floatX* bx, int n);
};

struct TokenEmbed : GeNeuron {
    hGTensor w, out;
    hGTensor cuInfer(int token, int flag = 0);
};

struct Head4Token : GeNeuron {
    SLP proj;
    hGTensor preLogits;
    hGTensor cuInfer_1(hGTensor inp_, int flag = 0);
};

struct MODEL_CARD {  // the fields of CLI_params / MODEL_CARD this path reads (CLI_params.hpp, cases/qwen3/*.json)
    int nEmbed = 0, nLayer = 0, n_head = 0, n_head_kv = 0, head_dim = 0, n_ff = 0, vocab = 0, n_ctx = 0;
    float rms_eps = 1e-6f, qk_eps = 1e-6f, rope_theta = 1e6f;
    bool tie_word_embeddings = true;
};

// token-batch (prefill) activations, [rows, .], allocated by the first Prefill and grown by a larger batch (Fish::PrefillReady)
struct TokenBatch {
    hGTensor bX, bNorm, bQ, bAttn, bGate, bUp;
    DevBuf<int32_t> d_ptok;
    int rows = 0;
    int Alloc(kf_ctx* c, int n, int dim, int q_dim, int ffn);
};
// Fish::Score: a chunk's target ids, log-probs and greedy ids [score_rows], and kf_head_logprob's workspace; allocated by the first Score (ScoreReady)
struct ScoreBuffers {
    DevBuf<int32_t> d_stgt, d_stop1;
    DevBuf<float> d_slp;
    DevBuf<> score_ws;
    int score_rows = 0;
    int Alloc(kf_ctx* c, int n, size_t ws_bytes) {
        KF_TRY(d_stgt.Alloc(c, (size_t)n * 4));
        KF_TRY(d_slp.Alloc(c, (size_t)n * 4));
        KF_TRY(d_stop1.Alloc(c, (size_t)n * 4));
        KF_TRY(score_ws.Alloc(c, ws_bytes));
        return score_rows = n, KF_OK;
    }
};
// Shared scratch, named after GST_MemBuffer's gBUFF members (GST_MemBuffer.hpp:46-48).  The two sets above are bases: gBUFF.bX / gBUFF.d_stgt read as members, each set commits whole
struct MemBuffer : TokenBatch, ScoreBuffers {
    hGTensor tmpFF1;    // Q.out
    hGTensor kraw;      // new key before norm/rope (fused path)
    hGTensor vraw;      // new value row before it is quantised (int8 KV cache; allocated by the first switch-on)
    hGTensor scratch;   // proj_cat out / gate-act
    hGTensor delta;     // down out
    hGTensor upOut;     // up out (unfused path)
    hGTensor normed;    // norm.out
    hGTensor attn_ws;   // split-KV partials
    hGTensor head_ws;   // arg-max partials
    hGTensor residual;  // alias, not owned
};

// CHAT_SAMPLER (CLI_params.hpp:663-683): the fields GeneratOnPrompt::Sample reads.  temperature == 0 or top_k == 1 -> sample_argmax.
// (The reference defaults to temperature 0.6; this host defaults to greedy, the mode every parity test and the bench use.)
struct CHAT_SAMPLER {
    float temperature = 0.0f;
    float top_p = 0.95f;
    int top_k = 50;
    uint64_t seed = 42;
    bool true_topk = false;  // false: the candidate set the reference's TOPK_heap keeps (kf_sample); true: the k largest logits (kf_sample_topk)
    bool greedy() const { return temperature == 0.0f || top_k == 1; }
    bool Valid(int vocab) const;  // what kf_sample accepts (greedy: always)
    static CHAT_SAMPLER FromArgs(float temperature, float top_p, int top_k, uint64_t seed);  // the C arguments: bit 16 of top_k = true_topk
    // the next id drawn from `logits` with rng state `rng`: state {token, pos} -> {id, pos + 1}, ids [pos] = id (nothing drawn where forced [pos + 1] >= 0)
    int Draw(kf_ctx* c, const floatX* logits, int vocab, uint64_t* rng, int32_t* state, int32_t* ids, const int32_t* forced, int n_ctx) const;
};

// The decode buffers of n sequences, allocated and filled together (Fish: one sequence; XcdReplicas: n_seq; XcdTP: its one sequence)
struct SeqBuffers {
    DevBuf<int32_t> d_state;       // [n][4]: {token, pos, 0, 0} (XcdReplicas: {token, pos, parked, status})
    DevBuf<int32_t> d_forced;      // [n][n_ctx] teacher-forced ids, -1 = free running
    DevBuf<int32_t> d_tokens_out;  // [n][n_ctx] the id produced at each position
    int Alloc(kf_ctx* c, int n, int n_ctx, int tokens_fill) {  // tokens_fill: the byte d_tokens_out starts as
        KF_TRY(d_state.AllocFilled(c, (size_t)n * 16, 0));
        KF_TRY(d_forced.AllocFilled(c, (size_t)n * n_ctx * 4, 0xff));
        return d_tokens_out.AllocFilled(c, (size_t)n * n_ctx * 4, tokens_fill);
    }
};

// Tensor-parallel decode (no counterpart in the single-GPU reference, QKV.cu:503): this Fish holds ONE rank's shard -- the
// card carries the LOCAL head / ffn / vocab counts and the full nEmbed -- and exchanges fp32 partials through peer-mapped receive areas
// (kf_tp_* of the ABI).  q/k/v/gate/up are row shards, o_proj / down_proj column shards, the head a vocabulary shard, the embedding replicated.
struct TPState {
    int rank = 0, world = 1, vocab_row0 = 0;
    kf_tp_comm comm;
    DevBuf<uint8_t> area;               // uncached (kf_tp_alloc): the receive area, the generation and error words, the push descriptors
    bool committed = false;             // kf_tp_commit done for the current peer set
    std::vector<void*> opened;          // IPC mappings of other processes' areas (closed with the Fish)
    std::vector<hGraph> group_graphs;  // ranks of ONE process stepped in lock-step on one stream: rank 0 keeps the group's graphs, one per bucket
};

// the int8 activation rows (Fish::A8Ready): q [rows][max(q_dim, nEmbed, n_ff)], step [rows]
struct A8Rows {
    DevBuf<int8_t> q;
    DevBuf<float> step;
    int rows = 0;
    int Alloc(kf_ctx* c, int n, size_t wide) {
        KF_TRY(q.Alloc(c, wide * n));
        KF_TRY(step.Alloc(c, (size_t)n * 4));
        return rows = n, KF_OK;
    }
};
// [8][.] activation rows of the verify pass and its scratch, allocated by the first Verify
struct VerifyRows {
    hGTensor vX, vQ, vAttn, vGate, v_attn_ws, v_head_ws;
    DevBuf<int32_t> d_vtok;  // [8] the pass's ids, then [8] its greedy ids
    int Alloc(kf_ctx* c, const MODEL_CARD& card, const kf_weight& head);
};
// The context: the FIRST base of Fish, so it is destroyed LAST -- after every member and base that frees device memory through it.
struct CtxHolder {
    kf_ctx* ctx = nullptr;
    CtxHolder() = default;
    CtxHolder(const CtxHolder&) = delete;
    ~CtxHolder() { kf_destroy(ctx); }  // NULL (kf_init refused): nothing to do
};
struct Fish : CtxHolder, SeqBuffers {
    MODEL_CARD config;
    // The ways a layer can run (kf_host_modes.hpp: the one table of modes, of the pairs that do not combine and of what a refusal says).  Modes() is derived from the state
    // below, never stored; every entry that switches a mode ON asks Admit first (after its argument checks: a rejected call changes nothing), switching off is never
    // refused; ModeChanged() follows every switch that moved: the engine's table and the captured graphs belong to the other arithmetic, and XcdReplicas / XcdTP objects
    // built on this Fish re-check at their next use (weights_gen).
    unsigned Modes() const;
    // a refusal that names the int8 KV cache names its sub-setting too while that is on
    void Kv8Note(std::string& why) const {
        if (kv_int8 && kv_int8_prefill && why.find("int8 KV cache") != std::string::npos) why += " (its int8 prompt attention, kfh_set_kv_int8_prefill, is on too)";
    }
    int Admit(Mode asked, const char* entry, std::string& why) const {
        const int rc = mode_refusal(Modes(), asked, entry, why);
        if (rc != KF_OK) Kv8Note(why);
        return rc;
    }
    int EngineRefusal(std::string& why) const {  // engine_refusal for this Fish's modes
        const int rc = engine_refusal(Modes(), why);
        if (rc != KF_OK) Kv8Note(why);
        return rc;
    }
    bool EagerOnly() const { return eager_only(Modes()); }  // what the step sequencing asks: eager per-layer launches, position from the host, no engine, no graphs
    void ModeChanged();
    TPState tp;
    int TPInit(int rank, int world, int vocab_row0);  // allocates this rank's receive area; peers are set afterwards
    int TPSetPeer(int r, void* area);
    // One phase of a TP step: 0 embed | 1 attention half of `layer` up to the o_proj push | 2 its reduce | 3 FFN half up to the down_proj push |
    // 4 its reduce | 5 LM-head shard + arg-max push | 6 pick.  A rank that owns its GPU enqueues all of them in order (EnqueueStep); ranks that
    // share one stream are enqueued phase by phase across ranks (a reduce must not sit in the queue ahead of the pushes it waits for).
    int TPCommit();
    int TPPhase(int phase, int layer);
    int EnqueueStepTP();
    CHAT_SAMPLER samp_params;
    DevBuf<uint64_t> d_rng;  // LogitsInfo::rng_state on the device
    int SetSampler(const CHAT_SAMPLER& s);  // also (re)seeds the device rng state
    int HeadAndPick(const floatX* x_last);  // [final norm + LM head] then arg-max or Sample, and the decode-state update
    int fuse_level = 1;  // 0: one launch per reference kernel; 1: fused launches (5 per layer)
    // the layer loop of a decode step as one persistent launch (kf_engine_*): used by EnqueueStep when fuse_level >= 1, the model's shapes and
    // storage are served and the position bound is; otherwise the per-layer launches run.  Same arithmetic, bit for bit.
    DevBuf<> lin_scratch;  // kf_set_scratch: workspace of the dequantise-then-multiply storages (AutoAWQ, row forms), sized when weights are set
    DevBuf<> deq_arena;    // kf_set_dequant_arena: resident bf16 copies of the layers' quantised matrices for long prompts (EnsureResident)
    size_t resident_max_bytes = (size_t)16 << 30;
    // OFF by default: the copies are keyed by the blobs' addresses, so a caller that hands weights over as device pointers (kfh_set_weight is_device = 1) and later
    // re-quantises or updates them IN PLACE would prefill on stale bf16 copies while the decode reads the live data.  kfh_set_prefill_resident opts in and takes that promise
    // ("the quantised data does not change under me"); kfh_weights_changed drops the copies (and the engine's table) after an in-place update.
    int prefill_resident = 0;
    bool resident_tried = false;
    int EnsureResident(int PC);
    void DropResident();
    int GrowScratch(size_t need);  // the kf_set_scratch workspace grown to `need` bytes (synchronises first; never shrinks)
    int EnsureLinearScratch(const kf_weight& w, int nTok) { return GrowScratch(kf_linear_scratch_bytes(&w, nTok)); }
    bool use_engine = true;
    hEngine engine;      // points into engine_ws and head_screen: ~Fish drops it (and the graphs) before the members go
    DevBuf<> engine_ws;
    int engine_state = 0;  // 0 not tried, 1 built, -1 not served
    unsigned weights_gen = 0;  // counts DropEngine (a weight set again, kfh_weights_changed) and ModeChanged calls: engines other objects built on this Fish compare it with their own copy
    bool engine_embed = false;  // the engine reads the (bf16) embedding row itself
    bool engine_head = false;   // ... and runs the final norm, the (bf16) LM head and the greedy pick as trailing phases of its launch
    // The int8 screen of the in-launch head (kf_engine_set_head_screen): a derived copy of the head like the resident bf16 copies, so it is built only under the same promise
    // (prefill_resident: "the quantised data does not change under me"), counts against resident_max_bytes, and is dropped with the engine's table (kfh_weights_changed, a
    // weight set again) and when the promise is withdrawn.  The promise may arrive after the engine exists: RunSteps looks before every multi-step run.
    DevBuf<> head_screen;
    bool head_screen_tried = false;
    void EnsureHeadScreen();
    void DropHeadScreen();
    int masked_layers = 0;      // layers with a hot-row mask (kfh_set_hot): the engine walks dense FFNs only
    int EnsureEngine();
    // what the decode engines read of this model: one kf_engine_layer per layer -- the seven matrices (none with a bias), both norms, the q / k norms, the hot-row mask
    // (refused unless `masks`), K / V rows of layer l at kbase / vbase + l * n_ctx * kv_dim -- and the descriptor over them; KF_ENGINE_NOT_SERVED with `why` otherwise
    int EngineTable(floatX* kbase, floatX* vbase, bool masks, std::string& why, std::vector<kf_engine_layer>& L, kf_engine_desc& d) const;
    void DropEngineTable();     // the engine's device table and the captured graphs only (a hot-row mask changed)
    void DropEngine();          // weights / norms / caches changed: the engine's device table and the captured graphs hold stale pointers
    int EngineCheck();          // synchronises; a timed-out hand-off is reported ONCE (KF_INTERNAL_ERR), the engine reset so that later steps run again
    int engine_steps = 0;  // steps enqueued (or captured) through the engine
    std::string engine_why;  // why the engine does not serve this model (kf_engine_served), "" when it does
    int engine_autotune = 0;  // > 0: passes of kf_engine_tune run once per position bucket, at the first step inside it (kfh_set_engine_autotune; off in the library: ~0.2 s of
                              // host-blocking launches inside RunSteps -- bench.py opts in).  A failed tune is never fatal: the defaults stay, the engine is reset, the decode goes on.
    std::vector<unsigned char> bucket_tuned;
    KVCache cache;
    MemBuffer gBUFF;
    TokenEmbed embed;
    std::vector<std::unique_ptr<SelfAttention>> attn;
    std::vector<std::unique_ptr<FFN>> ffn;
    LayerNormal final_norm;
    Head4Token head;
    DevBuf<float> rope_table;     // device [n_ctx][hd/2][2]
    int tok_pos = 0;              // hBatch->tok_pos
    bool graph_mode = false;      // launches take position/token from d_state
    bool state_tokens = false;    // eager per-kernel steps (fuse_level 0, e.g. AutoAWQ weights): position from the host, token from d_state
    std::vector<hGraph> graphs;   // one per position bucket
    void DropGraphs() {           // every captured step graph (they hold the other arithmetic, pick, engine form or masks); the next step captures again
        for (auto& g : graphs) g.reset();
    }
    hGTensor x;                   // residual stream

    ~Fish();
    // the attention kernels are instantiated for query-group sizes 1, 2, 4, 8 and head_dim 64 / 128 (every Qwen3 size except the 14B's group of 5)
    static bool ShapeServed(const MODEL_CARD& card, std::string& why);
    int Build(const MODEL_CARD& card, int device, void* stream);
    int pos_bound() const;  // launch-geometry bound for the current bucket
    // one token through every neuron (Fish::ForwardOnRLS, gLLM.cpp:722-787)
    int ForwardOnRLS(int token, int pos);
    int EnqueueStep(int bound);  // the launch sequence of one step, positions/tokens from d_state
    kf_graph* GraphFor(int pos);
    int SetState(int token, int pos);
    // token-serial prefill then greedy decode (Fish::Chat, GoPT.cpp:1139-1159); ids of the new tokens to out
    int Generate(const int* prompt, int n_prompt, int n_new, int* out, bool use_graph);
    // replay n decode steps starting at `pos` with whatever d_forced holds (bench / long runs); no host sync
    bool OneLaunchStep(); /* the decode step is one kernel launch: launched directly, no graph */
    int RunSteps(int pos, int n, bool use_graph);
    // n prompt tokens at positions pos0.. through every layer as token batches (MFMA tile kernels), then the head on the last one:
    // afterwards the KV cache holds rows pos0..pos0+n-1, d_state = {greedy next token, pos0+n}, d_tokens_out[pos0+n-1] = that token.
    // The reference prefills token by token (Fish::Chat, GoPT.cpp:1139-1146); same arithmetic per token, fp32 sums in MFMA order.
    int Prefill(const int* tokens, int n, int pos0);
    // Fish_ppl / Fish::Eval_ppl (Evaluate.cpp:19-94) as a batch: the n tokens at positions pos0.. through every layer exactly as Prefill runs them (hot-row masks included),
    // then per chunk the final RMSNorm over the chunk's rows and kf_head_logprob against the NEXT token: logprob_out[i] = log P(tokens[i + 1] | tokens[0 .. i]) for
    // i < n - 1 -- the pair across a chunk boundary included -- and top1_out[i] (or NULL) the greedy id after token i.  K / V rows, d_state, d_tokens_out, logits and the
    // residual row are left exactly as Prefill(tokens, n, pos0) leaves them.  Argument checks and codes as Prefill's; n >= 2.
    int Score(const int* tokens, int n, int pos0, float* logprob_out, int* top1_out);
    int ScoreReady();  // PrefillReady + the scoring buffers, sized to the token-batch rows: allocated by the first Score, never inside a later one
    // the reference's perplexity loop: windows of at most `window` tokens (<= 0: n_ctx), each scored from position 0; sum, sum of squares and count of the log-probs in
    // fp64, ppl = exp(-sum / nz), pplerr = ppl * sqrt((ss - sum * sum / nz) / nz / nz) (Evaluate.cpp:64-80).  A trailing window of one token has no pair and is left out.
    int EvalPPL(const int* tokens, long long n, int window, double* ppl, double* pplerr, long long* n_scored);
    int PrefillReady(int min_rows = 0);  // the token-batch buffers ([rows >= min_rows]), scratch and resident copies: allocated by the first prefill, grown by a larger batch
    // rows per token batch (clamped to n_ctx).  Measured, Qwen3-0.6B 4-bit, prompt filling the context: 2047 tokens 20.9 / 15.5 / 9.8 ms at 512 / 1024 / 2048 rows,
    // 8191 tokens 92.3 / 53.9 / 42.7 / 36.6 ms at 1024 / 2048 / 4096 / 8192 (scratch/prefill_chunk.py): the tile kernels want many rows per launch.
    int prefill_chunk = 8192;
    int prefill_mode = 0;  // Generate: 0 token-serial prefill like the reference, 1 batched
    // ---- the modes.  Which of them combine, and every refusal's text: kf_host_modes.hpp.  Each setter keeps only the checks that are its mode's own.
    // int8 activations (kfh_set_act_int8; include/kf_abi.h "int8 activations"): every layer matrix stored ternary or 1-bit takes its input through kf_act_quant_i8 and
    // kf_linear_a8 -- q | k | v share one quantisation of the normed row (the norm prologue), gate | up one, o_proj and down_proj quantise their own inputs; matrices of
    // any other storage keep kf_rmsnorm + kf_linear; embedding, final norm and LM head are untouched.  Token-serial steps and token batches alike (an eager-only mode).
    // act_int8 is "either switch is on".  act_int8_t is kfh_set_act_int8's own state (ternary / 1-bit matrices -> kf_linear_a8), act_int8_q4 kfh_set_act_int8_q4's
    // (include/kf_abi.h "int8 activations for 4-bit layers": KF_Q4 group matrices that kf_linear_w4a8_status serves -> kf_linear_w4a8 / kf_linear_w4a8_tiles; their ZERO
    // need not be 0, the dequant arena is not consulted for them).
    bool act_int8 = false, act_int8_t = false, act_int8_q4 = false;
    A8Rows a8;
    // token batches of at least a8_tile_min rows send those matrices to kf_linear_a8_tiles (int8 MFMA tiles; the same bits), smaller ones and every single token to
    // kf_linear_a8; < 0: never.  kfh_set_a8_tile_min; the default is the tile plan's KF_A8_TILE_MIN.  a8_count: (tile, mat-vec) launches since the last switch-on.
    int a8_tile_min = KF_A8_TILE_MIN;
    int64_t a8_count[2] = {0, 0};
    // one switch per family; its own switch-on checks: a layer matrix of the family exists (q4: one kf_linear_w4a8 serves; otherwise: ternary / 1-bit, kf_linear_a8
    // accepts each, every ZERO section of those is zero)
    int SetActInt8(bool q4, bool on, std::string& why);
    int A8Route(const kf_weight& w, int n) const;  // 2 = kf_linear_w4a8(_tiles), 1 = kf_linear_a8(_tiles), 0 = kf_rmsnorm + kf_linear
    int A8Ready(int rows);
    // low-rank adapters at inference (kfh_set_adapter; include/kf_abi.h kf_lora_apply; the LORA branch of SLP::Forw): any subset of the layers' seven matrices carries a
    // trained pair a [r, in], b [out, r] -- device pointers of the caller's, no copy, read at every launch (a trainer's later step is seen) -- with ONE rank and ONE s for
    // the model (an eager-only mode).  Its own checks: s finite, one rank and one s, a rank and shape kf_lora_apply_status serves, 16-byte alignment.
    int n_adapters = 0, lora_r = 0;
    float lora_s = 0.0f;
    std::array<SLP*, 7> LayerMatrices(int layer) const;  // q k v o gate up down, the order of kf_engine_layer.w and of the C entries' slots
    bool HasRow3() const;  // a layer matrix is a 3-bit row codebook (NF3): per-layer launches with kf_set_row_unpack on; no engine, no XCD decoders, no Verify
    SLP* LayerMatrix(int layer, int slot) const;  // one of them, or NULL
    int SetAdapter(int layer, int slot, const floatX* a, const floatX* b, int r, float s, std::string& why);
    void ClearAdapters();
    // What the eager-only layer bodies run for the matrices s[0 .. n_w) on the rows x [n][ldx = dim] (normed by norm_w first when given): y[i] [n][ne0], with `residual`
    // (may alias y[0]; n_w == 1) the products' residual epilogue; normed: [n][dim] for the bf16 route.  One quantisation (kf_act_quant_i8) when a matrix takes an integer
    // route, one kf_rmsnorm when a matrix takes kf_linear, the product per matrix, then kf_lora_apply on the same y for the matrices that carry an adapter: one
    // vector-form launch for the group when n == 1, a tile-form launch per adapted matrix otherwise.
    int Group(const floatX* x, const floatX* norm_w, float eps, int n, int dim, floatX* normed, int n_w, SLP* const* s, floatX* const* y, const floatX* residual);
    // int8 KV cache (kfh_set_kv_int8; include/kf_abi.h "int8 KV cache"): K / V rows live as int8 codes with one fp32 step per row and kv-head; a decode step runs
    // kf_norm_linear (q, raw k, raw v into scratch rows) -> kf_attn_block_kv8 -> kf_linear per layer -- still 5 launches with the FFN's two, eager or on captured graphs
    // (d_pos, position buckets) like any model the engine does not serve; token batches quantise their rows into the cache and attend to the dequantised rows of the
    // staging pair (kf_kv8_quant_rows, kf_kv8_dequant_rows, then the existing kf_attn_prefill).  The two caches are independent: switching converts nothing, the caller
    // prefills again.  Its own check: kf_attn_block_kv8_status.
    bool kv_int8 = false;
    int SetKVInt8(bool on, std::string& why);
    // ... and its sub-setting (kfh_set_kv_int8_prefill; include/kf_abi.h "int8 KV cache, the prompt form"): token batches attend to the int8 rows themselves --
    // kf_qkv_rope_batch into the chunk's rows of the staging pair, kf_kv8_quant_rows, kf_attn_prefill_kv8: no kf_kv8_dequant_rows, no bf16 kf_attn_prefill, and the scores
    // of a prompt row are the decode kernel's.  A field beside kv_int8, not a mode: it is refused unless kv_int8 is on, excludes what MODE_KV_INT8 excludes through that
    // row, and is switched off with kv_int8.  Off by default.  Its own check: kf_attn_prefill_kv8_status.  kv8_count: (int8, dequantise-route) prompt-attention launches
    // since the last kfh_kv8_route_counts reset.
    bool kv_int8_prefill = false;
    int64_t kv8_count[2] = {0, 0};
    int SetKVInt8Prefill(bool on, std::string& why);
    // what Prefill and Score share: m tokens at positions pos.. as one token batch through the embedding and every layer (rows in gBUFF.bX); the ending -- the head on row
    // `last` of the batch buffer, the state update leaves {next token, pos + 1}
    int FlowChunk(const int* tokens, int m, int pos);
    int FlowEnd(int last, int token, int pos);
    int LayersAndHead(hGTensor cur);  // what EnqueueStep and ForwardOnRLS share: the embedded row through every layer's cuInfer, then the head
    // ---- the verify pass of speculative decoding (include/kf_abi.h "row siblings"): n = 1 .. 8 tokens at positions pos0 .. pos0 + n - 1 -- a token and its drafted
    // continuations -- through every layer with ONE pass over the weights: per layer [norm + q | k | v rows] -> q/k-norm + RoPE rows -> attention rows -> [o_proj +
    // residual rows] -> [norm + gate | up + SwiGLU rows] -> [down + residual rows], then [final norm + head + pick per row]: six launches per layer whatever n is.
    // top1[i] = the greedy id behind row i; logits_or_null [n][vocab].  Row i carries every bit (id, logits, K / V rows pos0 + i) of ForwardOnRLS(tokens[i], pos0 + i)
    // run one after the other on the fused per-layer launches (canonical order; in the v_dot2c order and for storages the row kernel does not take the entries run the
    // one-token launches row by row: still the plain step's bits).  Eager, the position from the host; K / V rows pos0 .. pos0 + n - 1 are (re)written, d_state, the
    // residual row x and the logits row of the plain step are not touched.  Not a mode: it reads Modes() and refuses while any is on, and a sampler that is not greedy
    // (verify_refusal, kf_spec.hpp).  One device-to-host read (the n ids; the logits when asked for).
    VerifyRows vrows;
    hGTensor vLogits;  // [8][vocab], allocated by the first Verify that asks for logits
    int Verify(const int* tokens, int n, int pos0, int* top1, floatX* logits_or_null, std::string& why);
    int64_t verify_rows[2] = {0, 0};  // activation rows of the Verify passes' mat-vec entries served with the shared unpack / row by row (kf_rows_route_counts deltas)
};

// Speculative decoding on a target Fish (greedy): rounds of "propose k ids, verify them in one pass, keep the longest agreed prefix" (kf_spec.hpp).  The ids it emits
// are Fish::Generate's, id for id: every kept id is the target's own greedy id behind a context of kept ids.
struct SpecDecoder {
    typedef int (*DraftFn)(const int* ids, int n, int k, int* out, void* user);  // a host drafter: the context ids [0, n) -> up to k proposals in out, their number back
    Fish* target = nullptr;    // not owned
    int k = 4;                 // drafts per round, 1 .. KF_SPEC_MAX_K
    int kind = 0;              // 0 lookup, 1 another Fish, 2 callback
    int ngram = 3;
    Fish* draft = nullptr;     // not owned; the same device, an equal vocabulary; its greedy steps run through RunSteps (whatever serves it, the engine included)
    int draft_rows = 0;        // the drafter's cache rows [0, draft_rows) belong to accepted tokens
    DraftFn fn = nullptr;
    void* user = nullptr;
    int64_t rounds = 0, proposed = 0, accepted = 0;
    int64_t rows_shared = 0, rows_single = 0;  // minus the target's verify_rows when the decoder began: kfh_spec_stats adds the target's current counts
    int Propose(const std::vector<int>& ids, int kk, int* out);  // up to kk proposals behind ids (the last of them the token not yet in the caches)
    // prompt [n_prompt] -> out [n_new], Generate's ids; leaves the target behind the last id: d_state = {last id, its position}, d_tokens_out as Generate leaves it
    int Generate(const int* prompt, int n_prompt, int n_new, int* out, std::string& why);
};

// What both XCD objects (XcdReplicas, XcdTP) own and do: the engine over the Fish's (ranks') weights and its workspace, the K / V rows, logits and residual streams of their
// sequences, the sequences' buffers, the launches in runs of steps_per_launch, the check and the teardown.
struct XcdSeqs : SeqBuffers {  // the K / V rows and per-sequence block of an XCD object: what XcdReplicas::MakeEngine(allocate) and XcdTP::Build make, all of it or none
    hGTensor key, val;      // [sequence or rank][n_layer][n_ctx][kv_dim] bf16
    hGTensor logits, x;     // [sequence][vocab], [sequence][nEmbed]
    int Alloc(kf_ctx* c, const MODEL_CARD& card, int n_kv, int n_seq, int vocab);
};
struct XcdEngine : XcdSeqs {
    kf_ctx* ctx = nullptr;  // the (first) Fish's, not owned; set by Build
    DevBuf<> engine_ws;     // declared ahead of the engine that points into it: destroyed after it
    hXEngine engine;
    std::string why;        // why the model is not served, "" when it is
    int steps_per_launch;
    explicit XcdEngine(int steps) : steps_per_launch(steps) {}
    ~XcdEngine() { if (ctx) kf_sync(ctx); }  // a launch may still be running; then the engine, its workspace and the sequences' buffers go with the members, in that order
    int EnsureWorkspace(size_t bytes) { return engine_ws && bytes <= engine_ws.bytes() ? KF_OK : engine_ws.Alloc(ctx, bytes); }  // kept when large enough; never while an engine points into it
    int LaunchSteps(int n);  // n greedy steps of every sequence, kf_xengine_steps in runs of at most steps_per_launch; no host sync
    int SetStepsPerLaunch(int n);
    int Check();          // synchronises; a timed-out hand-off is reported once (KF_INTERNAL_ERR) and the engine reset
};

// Eight independent decoders on ONE GPU, one per XCD, sharing a Fish's weights (kf_xengine_* of the ABI; round 5).  The reference decodes one sequence per process
// (Fish::Chat, GoPT.cpp:1139-1180) and scales a small model by running more processes; here the "processes" are the 32-workgroup halves of one launch: sequence s has its own
// KVCache (Cache.cpp:14-57, one per sequence), decode state, forced ids, ids out and logits -- everything the reference's per-process Fish owns except the weights.
// Every sequence's ids / logits / K / V rows are those Fish::RunSteps produces for it alone (canonical order), bit for bit.
struct XcdReplicas : XcdEngine {
    Fish* hFish = nullptr;  // the weights (not owned)
    int n_seq = 0;
    long long steps_run = 0;
    unsigned built_gen = 0;  // Fish::weights_gen the engine was built on
    XcdReplicas() : XcdEngine(32) {}
    int Build(Fish* f, int n_seq_);
    int MakeEngine(bool allocate);
    int Fresh();          // re-creates the engine when the Fish's weights changed since it was built (kfh_weights_changed, a weight set again)
    int Park(int seq, bool on);
    int Status(int seq, int32_t* out4);
    int SetForced(int seq, const int32_t* ids, int n);
    int SetState(int seq, int token, int pos);
    int Prefill(int seq, const int* tokens, int n);  // the sequence's prompt through Fish::Prefill (token batches on the tile kernels), its K / V rows into the sequence's cache; the sequence then stands behind the prompt
    int RunSteps(int n);  // n greedy steps of EVERY sequence from wherever each stands; no host sync
    // a queue of prompts answered through the slots (Fish::Chat's rounds over DEBUG.prompts, GoPT.cpp:1111-1180, n_seq at once); see kf_host.cpp
    int Chat(const int32_t* prompts, const int32_t* prompt_len, int n_req, int stride, int max_new, int eos, int32_t* out, int32_t* out_len, long long* stats,
             const int32_t* max_new_each = nullptr);  // max_new_each: a limit of its own per request (<= max_new)
    // S prompts at once (rows = S x T, T = the longest, shorter ones padded): ONE token batch through the tile kernels -- the rows of a prompt attend to that prompt only
    // (kf_attn_prefill_batch), positions restart per prompt (kf_qknorm_rope_train), every prompt's K / V rows scattered into its slot's cache (kf_copy_blocks), the head on
    // each prompt's last row.  What Fish::Chat's token-serial prefill loop (GoPT.cpp:1139-1146) does for one prompt, for S of them in the launches of one.
    int PrefillBatch(const int* slots, const int32_t* tokens, const int* lens, int S, int stride);
    int prefill_batch = 1;        // Chat: prompts prefilled together when several slots are free (1: one by one, the bits of Fish::Prefill)
    struct BatchRows {            // what PrefillBatch needs beside the Fish's token-batch buffers; regrown whole when a batch has more rows
        hGTensor bK, bV, bL;      // [rows, kv_dim] K / V rows of a prompt batch before they are scattered; [n_seq, vocab] the batch's logits
        DevBuf<void*> d_dst;      // [3][n_seq] device tables of the scatters' destinations (K, V, logits), then the batch's slots as int32
        int Alloc(kf_ctx* c, int kv_dim, int rows, int vocab, int n_seq);
    } pb;
    CHAT_SAMPLER samp_params;     // Chat's sampler (greedy by default); non-greedy: one launch per token, kf_sample per occupied slot
    DevBuf<uint64_t> d_rng;       // [n_seq] xorshift states, seeded per request (seed + request index)
    int SetSampler(const CHAT_SAMPLER& s);
    size_t kv_seq_elems() const;
};

// ONE sequence of a model split over eight tensor-parallel ranks, the ranks as the eight XCDs of ONE launch (kf_xengine_create_tp): the Fish of every rank holds its shards
// (koifish_amd/tp.py build_native_rank); this object owns the ranks' K / V rows, the sequence's state / forced ids / ids out, the full logits vector.
// key / val: [rank][n_layer][n_ctx][kv_dim of a rank]; logits: [vocab] (the shards in rank order); x: [nEmbed].
struct XcdTP : XcdEngine {
    std::vector<Fish*> ranks;  // not owned
    int vocab = 0;
    std::vector<unsigned> built_gen;  // the ranks' Fish::weights_gen at Build: a rank whose weights changed since makes RunSteps refuse (the engine holds a fused copy of q | k | v)
    XcdTP() : XcdEngine(16) {}
    int Build(Fish** fs, int world);
    int SetForced(const int32_t* ids, int n);
    int SetState(int token, int pos);
    int RunSteps(int n);
};

}  // namespace koifish
