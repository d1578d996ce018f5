/*
 * kf_host_abi.h -- C surface of libkf_host.so: one prototype per exported kfh_* / kfhdbg_* function.  The definitions (the four .cpp files of koifish_amd/host) carry the
 * documentation and include this header, so a definition that disagrees with its prototype does not compile; koifish_amd/lib.py reads the ctypes signatures
 * from this text (it does not preprocess: every entry is written out).  Handles are void*: koifish::Fish* (kfh_create, kfh_load_*), SpecDecoder*
 * (kfh_spec_create), XcdReplicas* (kfh_xr_create), XcdTP* (kfh_xtp_create), a trainer (kfh_gpt2_create / kfh_qwen3t_create), a safetensors file (kfh_st_open).
 * int returns are 0 (KF_OK) or a negative KF_* code of kf_abi.h unless the definition says otherwise.
 */
#ifndef KF_HOST_ABI_H
#define KF_HOST_ABI_H
#include <stddef.h>
#include <stdint.h>

#include "kf_abi.h" /* kf_ctx, kf_weight */

#ifdef __cplusplus
extern "C" {
#endif

/* a host drafter of kfh_spec_set_callback (koifish::SpecDecoder::DraftFn): the context ids [0, n) -> up to k proposals in out, their number back */
typedef int (*kfh_spec_draft_fn)(const int* ids, int n, int k, int* out, void* user);


/* ---- kf_host.cpp: the model (koifish::Fish), the decode engines, speculative decoding, tensor parallel, the XCD decoders ---- */
void* kfh_create(int device, void* stream, int dim, int n_layer, int n_head, int n_kv, int head_dim, int ffn, int vocab, int n_ctx, float rms_eps, float qk_eps,
                 float theta, int* rc_out);
void kfh_destroy(void* h);
const char* kfh_host_error(void);
void* kfh_ctx(void* h);
int kfh_set_fuse_level(void* h, int lvl);
int kfh_set_hot(void* h, int layer, const int32_t* h_hot, int n);
int kfh_n_hot(void* h, int layer);
int kfh_set_engine(void* h, int on);
int kfh_set_act_int8(void* h, int on);
int kfh_set_act_int8_q4(void* h, int on);
int kfh_set_kv_int8(void* h, int on);
int kfh_kv_int8(void* h);
int kfh_set_kv_int8_prefill(void* h, int on);
int kfh_kv_int8_prefill(void* h);
int kfh_kv8_route_counts(void* h, int64_t* out2, int reset);
void* kfh_kv8_codes(void* h, int val);
void* kfh_kv8_steps(void* h, int val);
int kfh_set_adapter(void* h, int layer, int slot, const void* a, const void* b, int r, float s);
int kfh_clear_adapters(void* h);
int kfh_n_adapters(void* h);
int kfh_set_a8_tile_min(void* h, int n);
int kfh_a8_route_counts(void* h, int64_t* out2);
int kfh_set_canonical(void* h, int on);
int kfh_engine_steps(void* h);
int kfh_engine_stamps(void* h, unsigned long long* out, int n);
int kfh_engine_stamps_enable(void* h, int wg);
int kfh_engine_set_delays(void* h, const int* d6);
const char* kfh_engine_why(void* h);
int kfh_engine_tune(void* h, int passes, float* us2);
int kfh_weights_changed(void* h);
int kfh_set_prefill_resident(void* h, int on, size_t max_bytes);
size_t kfh_resident_bytes(void* h);
int kfh_set_engine_autotune(void* h, int passes);
int kfh_engine_stats(void* h, int pos, int32_t* out14);
int kfh_engine_screen_stats(void* h, int64_t* out3);
int kfh_engine_only(void* h, int n);
int kfh_engine_check(void* h);
int kfhdbg_mode_refusal(unsigned active, int asked, char* why, size_t n);
int kfhdbg_engine_refusal(unsigned active, char* why, size_t n);
int kfhdbg_eager_only(unsigned active);
int kfh_set_weight(void* h, int layer, int slot, int type, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device, int lGroup,
                   int qMin, int qMax, int qBias);
int kfh_set_weight_lut(void* h, int layer, int slot, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device);
int kfh_set_weight_lut_bits(void* h, int layer, int slot, int bits, int ne0, int ne1, const void* blob, size_t blob_bytes, size_t szData, int is_device);
int kfh_tie_head(void* h);
int kfh_set_norm(void* h, int layer, int slot, const void* w, int n, int is_device);
int kfh_forward(void* h, int token, int pos, uint16_t* h_logits);
int kfh_verify(void* h, const int* tokens, int n, int pos0, int* top1_out, uint16_t* logits_out);
void* kfh_spec_create(void* target, int k);
void kfh_spec_destroy(void* s);
int kfh_spec_set_lookup(void* s, int ngram);
int kfh_spec_set_draft_model(void* s, void* fish);
int kfh_spec_set_callback(void* s, kfh_spec_draft_fn fn, void* user);
int kfh_spec_generate(void* s, const int* prompt, int n_prompt, int n_new, int* out);
int kfh_spec_stats(void* s, int64_t* out5);
int kfhdbg_spec_clip_k(int k, int n_left, int pos, int n_ctx);
int kfhdbg_spec_accept(const int* drafts, int k, const int* top1);
int kfhdbg_spec_lookup(const int* ids, int n, int ngram, int k, int* out);
int kfhdbg_verify_refusal(unsigned active, int greedy, char* why, size_t n);
int kfh_generate(void* h, const int* prompt, int n_prompt, int n_new, int* out, int use_graph);
int kfh_set_forced(void* h, const int32_t* forced, int n);
int kfh_prefill(void* h, const int* tokens, int n, int pos0);
int kfh_score(void* h, const int* tokens, int n, int pos0, float* logprob_out, int* top1_out);
int kfh_eval_ppl(void* h, const int* tokens, long long n, int window, double* ppl, double* pplerr, long long* n_scored);
int kfh_set_prefill_mode(void* h, int mode, int chunk);
int kfh_set_sampler(void* h, float temperature, float top_p, int top_k, uint64_t seed);
int kfh_set_state(void* h, int token, int pos);
int kfh_run_steps(void* h, int pos, int n, int use_graph);
int kfh_sync(void* h);
int kfh_get_tokens(void* h, int32_t* out, int n);
void* kfh_kcache(void* h);
void* kfh_vcache(void* h);
void* kfh_logits(void* h);
void* kfh_hidden(void* h);
int kfh_tp_init(void* h, int rank, int world, int vocab_row0);
void* kfh_tp_area(void* h);
int kfh_tp_set_peer(void* h, int r, void* area);
int kfh_tp_export(void* h, unsigned char* handle64);
int kfh_tp_open_peer(void* h, int r, const unsigned char* handle64);
int kfh_tp_check(void* h);
int kfh_tp_group_run(void** hs, int R, int pos, int n, int use_graph);
void* kfh_xr_create(void* fish, int n_seq, int* rc_out);
void kfh_xr_destroy(void* h);
int kfh_xr_set_forced(void* h, int seq, const int32_t* ids, int n);
int kfh_xr_set_state(void* h, int seq, int token, int pos);
int kfh_xr_prefill(void* h, int seq, const int* tokens, int n);
int kfh_xr_run_steps(void* h, int n);
int kfh_xr_check(void* h);
int kfh_xr_park(void* h, int seq, int on);
int kfh_xr_prefill_batch(void* h, const int* slots, const int32_t* tokens, const int* lens, int S, int stride);
int kfh_xr_set_prefill_batch(void* h, int n);
int kfh_xr_set_sampler(void* h, float temperature, float top_p, int top_k, uint64_t seed);
int kfh_xr_chat(void* h, const int32_t* prompts, const int32_t* prompt_len, int n_req, int stride, int max_new, int eos, int32_t* out, int32_t* out_len,
                long long* stats);
int kfh_xr_chat_each(void* h, const int32_t* prompts, const int32_t* prompt_len, int n_req, int stride, int max_new, int eos, int32_t* out, int32_t* out_len,
                     long long* stats, const int32_t* max_new_each);
int kfh_xr_status(void* h, int seq, int32_t* out4);
int kfh_xr_set_steps_per_launch(void* h, int n);
int kfh_xr_get_tokens(void* h, int seq, int32_t* out, int n);
int kfh_xr_get_state(void* h, int seq, int32_t* out2);
void* kfh_xr_logits(void* h, int seq);
void* kfh_xr_hidden(void* h, int seq);
void* kfh_xr_kcache(void* h, int seq);
void* kfh_xr_vcache(void* h, int seq);
void* kfh_xtp_create(void** fishes, int world, int* rc_out);
void kfh_xtp_destroy(void* h);
int kfh_xtp_set_forced(void* h, const int32_t* ids, int n);
int kfh_xtp_set_state(void* h, int token, int pos);
int kfh_xtp_run_steps(void* h, int n);
int kfh_xtp_check(void* h);
int kfh_xtp_set_steps_per_launch(void* h, int n);
int kfh_xtp_get_tokens(void* h, int32_t* out, int n);
int kfh_xtp_vocab(void* h);
void* kfh_xtp_logits(void* h);
void* kfh_xtp_hidden(void* h);
void* kfh_xtp_kcache(void* h);
void* kfh_xtp_vcache(void* h);
int kfh_xtp_stamps_enable(void* h, int rank, int wg, int max_steps);
int kfh_xtp_stamps(void* h, unsigned long long* out, int n);
int kfh_xr_variant(void* h, int nwv, int depth);
int kfh_xr_stamps_enable(void* h, int seq, int wg, int max_steps);
int kfh_xr_stamps(void* h, unsigned long long* out, int n);
int kfh_num_graphs(void* h);

/* ---- kf_safetensors.cpp: checkpoints: safetensors, HF directories, .kun files, JSON / msgpack ---- */
const char* kfh_last_error(void);
void* kfh_st_open(const char* path_or_dir, int is_dir);
void kfh_st_close(void* h);
int kfh_st_count(void* h);
int kfh_st_info(void* h, int i, char* name, int name_cap, char* dtype, int dtype_cap, int64_t* shape4, int* ndim, uint64_t* begin, uint64_t* end);
int kfh_st_read(void* h, const char* name, void* out, uint64_t nbytes);
void* kfh_load_hf(const char* dir, int device, void* stream, int layer_type, int head_type, int lGroup, int max_seq, int* rc);
int kfh_save_kun(void* h, const char* path);
void* kfh_load_kun(const char* path, int device, void* stream, int max_seq, int* rc);
int kfh_kun_write(const char* path, int n, const char* const* names, const char* const* dtypes, const int64_t* shape4, const uint64_t* szData,
                  const uint64_t* szGama, const void* const* blobs, const char* config_json);
int64_t kfh_st_config_json(void* h, char* out, int64_t cap);
int kfh_st_blob_sizes(void* h, int i, uint64_t* szData, uint64_t* szGama);
int64_t kfh_json_to_msgpack(const char* text, uint8_t* out, int64_t cap);
int64_t kfh_msgpack_to_json(const uint8_t* pack, int64_t n, char* out, int64_t cap);
int kfh_get_config(void* h, int* out10, float* out2);

/* ---- kf_train.cpp: koifish::GPT2Trainer (handles are its TrainerCore) ---- */
void* kfh_gpt2_create(kf_ctx* ctx, int C, int H, int NL, int V, int Vp, int B, int T);
void kfh_gpt2_destroy(void* h);
int kfh_gpt2_n_params(void* h);
int kfh_gpt2_set_param(void* h, int index, void* p, void* g, void* m, void* v, long long n, int decay, const kf_weight* blob, int requant);
int kfh_gpt2_set_param_gama(void* h, int index, void* g, void* m, void* v, const kf_weight* blob);
int kfh_gpt2_set_gama_scratch(void* h, void* scratch, size_t bytes);
int kfh_gpt2_set_block_acts(void* h, int layer, void* const* ptrs);
int kfh_gpt2_set_buffers(void* h, void* const* ptrs);
int kfh_gpt2_forward(void* h, const int32_t* d_ids, const int32_t* d_tgt);
int kfh_gpt2_backward(void* h);
int kfh_gpt2_update(void* h, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed);
int kfh_gpt2_step(void* h, const int32_t* d_ids, const int32_t* d_tgt, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed);
int kfh_gpt2_set_optimizer(void* h, int method, float lr_scale, float mui, float eps_muon, int tp_decay, void* scratch, size_t scratch_bytes);
long long kfh_gpt2_steps_taken(void* h);
int kfh_gpt2_set_branches(void* h, int layers_in_branch);
int kfh_gpt2_n_branches(void* h);
int kfh_gpt2_set_active_branch(void* h, int b);
int kfh_gpt2_active_branch(void* h);
int kfh_gpt2_evolve(void* h, int head_branch, int algorithm, float alpha, float social, float t_cross, uint32_t seed);
int kfh_gpt2_eval(void* h, const int32_t* d_ids, const int32_t* d_tgt, int mode, int branch, float* d_loss_out);
int kfh_gpt2_set_grad_clip(void* h, int mode, float gclip, void* scratch, size_t scratch_bytes);
size_t kfh_gpt2_grad_clip_scratch_bytes(void* h);
int kfh_gpt2_grad_norms(void* h, float* h_out, int n);
int kfh_gpt2_set_distill(void* h, const void* teacher_logits, int64_t teacher_ld, float ce_weight, float kd_weight, float temperature, void* kd_rows);
int kfh_gpt2_forward_logits(void* h, const int32_t* d_ids);
const char* kfh_gpt2_last_error(void);

/* ---- kf_train_qwen3.cpp: koifish::Qwen3Trainer (handles are its TrainerCore); the entries it shares with kfh_gpt2_* have the same signatures ---- */
void* kfh_qwen3t_create(kf_ctx* ctx, int dim, int n_layer, int n_head, int n_kv, int head_dim, int ffn, int V, int Vp, int B, int T, float rms_eps, int tied);
void kfh_qwen3t_destroy(void* h);
int kfh_qwen3t_n_params(void* h);
int kfh_qwen3t_set_param(void* h, int index, void* p, void* g, void* m, void* v, long long n, int decay, const kf_weight* blob, int requant);
int kfh_qwen3t_set_param_gama(void* h, int index, void* g, void* m, void* v, const kf_weight* blob);
int kfh_qwen3t_set_gama_scratch(void* h, void* scratch, size_t bytes);
int kfh_qwen3t_set_param_lora(void* h, int index, void* p, void* g, void* m, void* v, int rank, float s, void* ax, const kf_weight* blob);
int kfh_qwen3t_set_lora_scratch(void* h, void* scratch, size_t bytes);
int kfh_qwen3t_set_layer_acts(void* h, int layer, void* const* ptrs);
int kfh_qwen3t_set_buffers(void* h, void* const* ptrs);
int kfh_qwen3t_forward(void* h, const int32_t* d_ids, const int32_t* d_tgt);
int kfh_qwen3t_backward(void* h);
int kfh_qwen3t_update(void* h, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed);
int kfh_qwen3t_step(void* h, const int32_t* d_ids, const int32_t* d_tgt, float lr, double beta1, double beta2, float eps, float wd, uint32_t seed);
int kfh_qwen3t_set_optimizer(void* h, int method, float lr_scale, float mui, float eps_muon, int tp_decay, void* scratch, size_t scratch_bytes);
long long kfh_qwen3t_steps_taken(void* h);
int kfh_qwen3t_set_grad_clip(void* h, int mode, float gclip, void* scratch, size_t scratch_bytes);
size_t kfh_qwen3t_grad_clip_scratch_bytes(void* h);
int kfh_qwen3t_grad_norms(void* h, float* h_out, int n);
int kfh_qwen3t_set_distill(void* h, const void* teacher_logits, int64_t teacher_ld, float ce_weight, float kd_weight, float temperature, void* kd_rows);
int kfh_qwen3t_forward_logits(void* h, const int32_t* d_ids);
int kfh_qwen3t_set_documents(void* h, const void* h_header, const void* d_table, const int32_t* d_pos, const int32_t* d_mask, int n_valid);
const char* kfh_qwen3t_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
