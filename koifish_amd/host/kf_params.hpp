// kf_params.hpp -- which parameters the decoder has, stated once: name, kind, (layer, slot), shape, required or not.  Plain C++17, no device.  The loaders (Hugging Face,
// .kun), the .kun writer and the kfh_set_* entries walk or search this table; Fish::Resolve says where an entry lives.
#pragma once
#include <string>
#include <vector>

namespace koifish {

struct MODEL_CARD {  // the fields of CLI_params / MODEL_CARD this path reads (CLI_params.hpp, cases/qwen3/*.json)
    int nEmbed = 0, nLayer = 0, n_head = 0, n_head_kv = 0, head_dim = 0, n_ff = 0, vocab = 0, n_ctx = 0;
    float rms_eps = 1e-6f, qk_eps = 1e-6f, rope_theta = 1e6f;
    bool tie_word_embeddings = true;
};

enum ParamKind { P_EMBED = 0, P_HEAD, P_NORM, P_MATRIX };
// (layer, slot) in the numbering of the C entries.  Matrices (kfh_set_weight*): layer >= 0, slot 0 q, 1 k, 2 v, 3 o, 4 gate, 5 up, 6 down -- the order of
// kf_engine_layer.w; layer -1: slot 0 embed_tokens, 1 lm_head.  Norms (kfh_set_norm): layer >= 0, slot 0 input_layernorm, 1 post_attention_layernorm, 2 q_norm,
// 3 k_norm; layer -1, slot 0: the final norm.  Shapes are [ne0 = out][ne1 = in]; a norm is [ne0][1].
struct Param {
    std::string name;  // the Hugging Face name
    ParamKind kind;
    int layer, slot, ne0, ne1;
    bool required;  // q_norm / k_norm may be missing; so may lm_head (head_is_tied)
};

// The model's parameters in the order the neurons are built (embed, layers, final norm, head): a `.kun` file's tensor order and offsets follow it.
inline std::vector<Param> param_table(const MODEL_CARD& c) {
    const int C = c.nEmbed, qd = c.n_head * c.head_dim, kvd = c.n_head_kv * c.head_dim, hd = c.head_dim, F = c.n_ff;
    std::vector<Param> v;
    v.push_back({"model.embed_tokens.weight", P_EMBED, -1, 0, c.vocab, C, true});
    for (int l = 0; l < c.nLayer; l++) {
        const std::string p = "model.layers." + std::to_string(l) + ".";
        v.push_back({p + "input_layernorm.weight", P_NORM, l, 0, C, 1, true});
        v.push_back({p + "self_attn.q_proj.weight", P_MATRIX, l, 0, qd, C, true});
        v.push_back({p + "self_attn.k_proj.weight", P_MATRIX, l, 1, kvd, C, true});
        v.push_back({p + "self_attn.v_proj.weight", P_MATRIX, l, 2, kvd, C, true});
        v.push_back({p + "self_attn.q_norm.weight", P_NORM, l, 2, hd, 1, false});
        v.push_back({p + "self_attn.k_norm.weight", P_NORM, l, 3, hd, 1, false});
        v.push_back({p + "self_attn.o_proj.weight", P_MATRIX, l, 3, C, qd, true});
        v.push_back({p + "post_attention_layernorm.weight", P_NORM, l, 1, C, 1, true});
        v.push_back({p + "mlp.gate_proj.weight", P_MATRIX, l, 4, F, C, true});
        v.push_back({p + "mlp.up_proj.weight", P_MATRIX, l, 5, F, C, true});
        v.push_back({p + "mlp.down_proj.weight", P_MATRIX, l, 6, C, F, true});
    }
    v.push_back({"model.norm.weight", P_NORM, -1, 0, C, 1, true});
    v.push_back({"lm_head.weight", P_HEAD, -1, 1, c.vocab, C, false});
    return v;
}
// the entry a C setter names: a norm (kfh_set_norm) or a weight (kfh_set_weight*: embedding, head, layer matrix); NULL when there is none
inline const Param* find_param(const std::vector<Param>& table, bool norm, int layer, int slot) {
    for (const Param& p : table)
        if ((p.kind == P_NORM) == norm && p.layer == layer && p.slot == slot) return &p;
    return nullptr;
}
// tie_word_embeddings: lm_head shares embed_tokens' tensor when the card says so or the checkpoint holds no lm_head.weight (Neuron.cpp:349-356)
inline bool head_is_tied(const MODEL_CARD& c, bool has_lm_head) { return c.tie_word_embeddings || !has_lm_head; }

}  // namespace koifish
