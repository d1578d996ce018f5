"""ctypes loader for libkf_hip.so / libkf_host.so (built in-tree by koifish_amd/build.py)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# KF_LIB_DIR (development only: scratch/build_variant.py): a directory holding an A/B build of the two libraries
LIB_HIP = os.path.join(os.environ.get("KF_LIB_DIR", HERE), "libkf_hip.so")
LIB_HOST = os.path.join(os.environ.get("KF_LIB_DIR", HERE), "libkf_host.so")

# typNUMBER (src/g_float.hpp:84-117)
F32, F64, F16, BF16, F8E5M2, F8E4M3, U8, I8, U16, I16, U32, I32, U64, I64, Q4, Q3, Q2, T_SIGN, T_SEQ, BOOL1, T_BINARY, T_BINARY_3, T_BINARY_TILE = range(23)
BITS = {BF16: 16, F8E5M2: 8, Q4: 4, T_SIGN: 2, BOOL1: 1, T_BINARY: 1}
KF_EPI_RESIDUAL = 1
EVO_PSO, EVO_MIX, EVO_PSO_GA = 1, 2, 4   # enum kf_evo_algorithm = the live members of Fuyou_params::ALGORITHM
EVO_ALGORITHMS = {"pso": EVO_PSO, "mix": EVO_MIX, "pso_ga": EVO_PSO_GA}   # Fuyou_params::Algo2Name
ENSEMBLE_AGGREGATION, ENSEMBLE_BRANCH = 0, 1   # kfh_gpt2_eval's mode
QUANT_GROUP, QUANT_ROW_LUT, QUANT_ROW_RTN = 0, 1, 2  # kf_weight.quant
CLIP_OFF, CLIP_REPORT, CLIP_TENSOR, CLIP_GLOBAL = 0, 1, 2, 3   # enum kf_clip_mode (0: the trainers' "off"; kf_grad_norms itself has no such mode)
CLIP_MODES = {None: CLIP_OFF, "report": CLIP_REPORT, "tensor": CLIP_TENSOR, "global": CLIP_GLOBAL}
MODES = ("TP", "ACT_INT8", "ADAPTERS", "KV_INT8", "HOT_MASK", "FUSE0")  # enum koifish::Mode (host/kf_host_modes.hpp), in precedence order
NF4 = 1000  # not a typNUMBER: "Q4 with the normal-float quant card" (QUANT_MODE::RTNf) for the helpers that take a storage type
NF3 = 1001  # the same card at 3 bits (RT_NormalF with bits == 3): layer matrices only, multiplied from the packed stream with kf_set_row_unpack
FMT_Q3R, FMT_Q2R, FMT_Q2N = 9, 10, 11   # kf_kernels.h: the kernel formats of the 3- / 2-bit row forms (kfdbg_rowq_standin)

# every symbol include/kf_abi.h declares (tests/test_abi_symbols.py checks the header against this list and the .so)
ABI_SYMBOLS = [
    "kf_init", "kf_destroy", "kf_sync", "kf_last_error", "kf_version", "kf_malloc", "kf_free", "kf_memset", "kf_memset32", "kf_h2d", "kf_d2h", "kf_d2d",
    "kf_graph_begin", "kf_graph_end", "kf_graph_launch", "kf_graph_destroy", "kf_event_create", "kf_event_record", "kf_event_elapsed_ms",
    "kf_event_destroy", "kf_dequant", "kf_quantize", "kf_linear", "kf_rmsnorm", "kf_qknorm_rope", "kf_rope_table_host", "kf_attn_decode",
    "kf_attn_scratch_bytes", "kf_linear_f32", "kf_tp_reduce", "kf_swiglu", "kf_add", "kf_embed", "kf_lm_head", "kf_head_scratch_bytes", "kf_norm_linear",
    "kf_norm_gateup_swiglu", "kf_attn_block", "kf_norm_lm_head", "kf_set_state", "kf_embed_state", "kf_embed_batch", "kf_qknorm_rope_batch", "kf_attn_prefill", "kf_sample", "kf_linear_multi", "kf_linear_multi_scratch_bytes", "kf_gateup_swiglu_batch", "kf_adamw", "kf_layernorm", "kf_gelu", "kf_sample_topk", "kf_fused_classifier", "kf_gelu_backward", "kf_swiglu_backward", "kf_rope_backward", "kf_norm_backward", "kf_norm_backward_scratch_bytes", "kf_linear_backward", "kf_linear_backward_scratch_bytes", "kf_embed_backward", "kf_attn_backward", "kf_attn_backward_scratch_bytes", "kf_attn_prefill_batch", "kf_attn_prefill_batch_strided", "kf_embed_pos", "kf_memset2d", "kf_copy_blocks", "kf_argmax_rows_state", "kf_qknorm_rope_train",
    "kf_hot_rows", "kf_linear_masked", "kf_zero_cold_columns", "kf_norm_gateup_swiglu_masked", "kf_linear_scratch_bytes", "kf_set_scratch", "kf_engine_workspace_bytes", "kf_engine_create", "kf_engine_step", "kf_engine_check", "kf_engine_destroy", "kf_engine_set_embedding", "kf_engine_set_head", "kf_engine_step_head", "kf_engine_steps_head", "kf_engine_reset", "kf_set_canonical", "kf_get_canonical", "kf_set_row_unpack", "kf_get_row_unpack", "kf_engine_served", "kf_engine_tune", "kf_engine_stats", "kf_engine_head_screen_bytes", "kf_engine_set_head_screen", "kf_engine_screen_stats", "kf_qkv_rope_batch", "kf_qkv_rope_seqs", "kf_set_dequant_arena", "kf_dequant_arena_used", "kf_resident_scratch_bytes",
    "kf_xengine_workspace_bytes", "kf_xengine_create", "kf_xengine_served", "kf_xengine_set_embedding", "kf_xengine_set_head", "kf_xengine_steps", "kf_xengine_check", "kf_xengine_reset", "kf_xengine_destroy", "kf_xengine_workspace_bytes_tp", "kf_xengine_create_tp", "kf_xengine_set_head_tp",
    "kf_tp_recv_bytes", "kf_tp_push_bytes", "kf_tp_commit", "kf_tp_alloc", "kf_tp_ipc_export", "kf_tp_ipc_open", "kf_tp_ipc_close", "kf_linear_f32_push", "kf_tp_reduce_recv", "kf_tp_lm_head", "kf_tp_pick",
    "kf_head_logprob", "kf_head_logprob_scratch_bytes",
    "kf_act_quant_i8", "kf_linear_a8", "kf_linear_a8_status", "kf_linear_a8_tiles", "kf_linear_a8_tiles_status",
    "kf_linear_w4a8", "kf_linear_w4a8_status", "kf_linear_w4a8_tiles", "kf_linear_w4a8_tiles_status",
    "kf_attn_block_kv8", "kf_attn_block_kv8_status", "kf_kv8_quant_rows", "kf_kv8_dequant_rows", "kf_attn_prefill_kv8", "kf_attn_prefill_kv8_status",
    "kf_muon_scratch_bytes", "kf_muon_momentum", "kf_newton_schulz", "kf_muon_apply", "kf_muon",
    "kf_gama_backward", "kf_gama_backward_scratch_bytes", "kf_dequant_arena_bytes",
    "kf_lora_forward", "kf_lora_backward", "kf_lora_backward_scratch_bytes", "kf_lora_apply", "kf_lora_apply_status",
    "kf_evolve", "kf_loss_mean", "kf_distill_classifier",
    "kf_qknorm_rope_backward", "kf_qknorm_rope_backward_scratch_bytes", "kf_d2d_rows",
    "kf_linear_rows", "kf_norm_linear_rows", "kf_norm_gateup_swiglu_rows", "kf_norm_lm_head_rows", "kf_head_rows_scratch_bytes", "kf_rows_route_counts", "kf_attn_decode_rows", "kf_attn_rows_scratch_bytes",
    "kf_adamw_scaled", "kf_grad_norms_scratch_bytes", "kf_grad_norms_plan", "kf_grad_norms", "kf_grad_norms_forget",
    "kf_attn_docs_table_bytes", "kf_attn_docs_plan", "kf_attn_prefill_docs", "kf_attn_backward_docs", "kf_attn_backward_docs_scratch_bytes", "kf_qknorm_rope_train_pos",
    "kf_qknorm_rope_backward_pos", "kf_zero_ignored_rows",
]


class KFError(RuntimeError):
    pass


class Weight(C.Structure):
    """struct kf_weight (include/kf_abi.h)"""
    _fields_ = [("data", C.c_void_p), ("gama", C.c_void_p), ("type", C.c_int32), ("ne0", C.c_int32), ("ne1", C.c_int32), ("nGroup", C.c_int32),
                ("lGroup", C.c_int32), ("qMin", C.c_int32), ("qMax", C.c_int32), ("qBias", C.c_int32), ("qzeros", C.c_void_p), ("qscales", C.c_void_p), ("quant", C.c_int32), ("reserved_", C.c_int32)]


class AttnDocsHeader(C.Structure):
    """struct kf_attn_docs_header (include/kf_abi.h): the first 64 bytes of a table kf_attn_docs_plan wrote; off / n: the forward, dQ and dK/dV tables in entries"""
    _fields_ = ([(f, C.c_int32) for f in ("magic", "n_rows", "n_head", "n_kv", "head_dim", "n_doc", "max_len")] + [("off", C.c_int32 * 3), ("n", C.c_int32 * 3)]
                + [(f, C.c_int32) for f in ("doc_rows", "gap_rows", "reserved_")])


ATTN_DOCS_MAGIC = 0x53434F44
F_IGNORE_LOSS = 0x10000   # MASK_FLAG::F_IGNORE_LOSS: the mask word of a row whose target does not count


class LoraPlan(C.Structure):
    """struct kf::LoraPlan (csrc/kf_lora_plan.h), as kfdbg_lora_plan fills it"""
    _fields_ = ([(f, C.c_int) for f in ("status", "tm", "rows_gx", "rows_block", "rows_lds", "tr_gx", "SA", "SB", "tilesA", "tilesB", "w_gx", "w_block", "w_lds", "fin_gx")]
                + [(f, C.c_longlong) for f in ("off_adelta", "off_aT", "off_bT", "off_partA", "off_partB", "scratch")])


class GradNormPlan(C.Structure):
    """struct kf::GradNormPlan (csrc/kf_gradnorm_plan.h), as kfdbg_gradnorm_plan fills it"""
    _fields_ = [("status", C.c_int), ("bad", C.c_int), ("n_tensors", C.c_int), ("total_wg", C.c_int), ("off_table", C.c_size_t), ("off_part", C.c_size_t), ("bytes", C.c_size_t), ("stamp", C.c_ulonglong)]


# the entries of libkf_host.so that kfh_gpt2_* and kfh_qwen3t_* have with one signature: (name, argtypes, restype)
_TRAINER_ENTRIES = [
    ("destroy", [C.c_void_p], None),
    ("n_params", [C.c_void_p], C.c_int),
    ("set_param", [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int], C.c_int),
    ("set_param_gama", [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("set_gama_scratch", [C.c_void_p, C.c_void_p, C.c_size_t], C.c_int),
    ("set_buffers", [C.c_void_p, C.c_void_p], C.c_int),
    ("forward", [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("backward", [C.c_void_p], C.c_int),
    ("update", [C.c_void_p, C.c_float, C.c_double, C.c_double, C.c_float, C.c_float, C.c_uint32], C.c_int),
    ("step", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_double, C.c_double, C.c_float, C.c_float, C.c_uint32], C.c_int),
    ("set_optimizer", [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_size_t], C.c_int),
    ("steps_taken", [C.c_void_p], C.c_longlong),
    ("set_grad_clip", [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_size_t], C.c_int),
    ("grad_clip_scratch_bytes", [C.c_void_p], C.c_size_t),
    ("grad_norms", [C.c_void_p, C.c_void_p, C.c_int], C.c_int),
    ("set_distill", [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_void_p], C.c_int),
    ("forward_logits", [C.c_void_p, C.c_void_p], C.c_int),
]
# a host drafter of generate_speculative: (ids, n, k, out, user) -> the number of ids proposed (koifish::SpecDecoder::DraftFn)
SPEC_DRAFT_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p)
_libs = None


def load():
    """Returns (hip, host) CDLLs.  No fallback: a missing library is an error the caller must see."""
    global _libs
    if _libs is None:
        for p in (LIB_HIP, LIB_HOST):
            if not os.path.exists(p):
                raise KFError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                              "koifish_amd has no CPU fallback." % p)
        hip = C.CDLL(LIB_HIP, mode=C.RTLD_GLOBAL)
        host = C.CDLL(os.environ.get("KF_HOST_LIB", LIB_HOST))   # KF_HOST_LIB: the sanitizer build of the host library (tests/test_host_asan_cpu.py)
        hip.kf_last_error.restype = C.c_char_p
        hip.kf_version.restype = C.c_char_p
        hip.kf_attn_scratch_bytes.restype = C.c_size_t
        hip.kf_head_scratch_bytes.restype = C.c_size_t
        hip.kf_linear.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_void_p]
        hip.kf_linear_f32.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p]
        hip.kf_tp_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        hip.kf_rmsnorm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
        hip.kf_qknorm_rope.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]
        hip.kf_rope_table_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
        hip.kf_attn_decode.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        hip.kf_attn_block.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
        hip.kf_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_linear_multi.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_linear_multi_scratch_bytes.argtypes, hip.kf_linear_multi_scratch_bytes.restype = [C.c_int, C.c_void_p, C.c_int], C.c_size_t
        hip.kf_gateup_swiglu_batch.argtypes = [C.c_void_p, C.POINTER(Weight), C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_adamw.argtypes = [C.c_void_p] * 5 + [C.c_size_t, C.c_int] + [C.c_float] * 8 + [C.c_uint32, C.c_void_p]
        hip.kf_adamw_scaled.argtypes = [C.c_void_p] * 5 + [C.c_size_t, C.c_int] + [C.c_float] * 7 + [C.c_void_p, C.c_uint32, C.c_void_p]
        hip.kf_grad_norms_scratch_bytes.argtypes, hip.kf_grad_norms_scratch_bytes.restype = [C.c_int, C.c_void_p], C.c_size_t
        hip.kf_grad_norms_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        hip.kf_grad_norms.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        hip.kf_grad_norms_forget.argtypes = [C.c_void_p, C.c_void_p]
        hip.kfdbg_gradnorm_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        hip.kf_muon_scratch_bytes.argtypes, hip.kf_muon_scratch_bytes.restype = [C.c_int, C.c_int], C.c_size_t
        hip.kf_muon_momentum.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_float, C.c_uint32, C.c_void_p]
        hip.kf_newton_schulz.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_size_t]
        hip.kf_muon_apply.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_float, C.c_float, C.c_uint32, C.c_void_p]
        hip.kf_muon.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        hip.kf_evolve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32]
        hip.kf_loss_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
        hip.kf_sample_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_layernorm.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        hip.kf_qknorm_rope_train.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        hip.kf_attn_prefill_batch.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        hip.kf_attn_backward.argtypes = [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        hip.kf_attn_backward_scratch_bytes.argtypes, hip.kf_attn_backward_scratch_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_size_t
        hip.kf_attn_prefill_batch_strided.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        # packed documents: the host plan, its three launches, the row-position forms of the q/k-norm + RoPE entries
        docs_layout = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        hip.kf_attn_docs_table_bytes.argtypes, hip.kf_attn_docs_table_bytes.restype = docs_layout, C.c_size_t
        hip.kf_attn_docs_plan.argtypes = docs_layout + [C.c_void_p, C.c_size_t]
        hip.kf_attn_prefill_docs.argtypes = [C.c_void_p] * 7 + [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
        hip.kf_attn_backward_docs_scratch_bytes.argtypes, hip.kf_attn_backward_docs_scratch_bytes.restype = [C.c_int, C.c_int], C.c_size_t
        hip.kf_attn_backward_docs.argtypes = [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        hip.kf_qknorm_rope_train_pos.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        hip.kf_qknorm_rope_backward_pos.argtypes = ([C.c_void_p] * 4 + [C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
                                                    + [C.c_int] * 3 + [C.c_void_p] * 6)
        hip.kf_zero_ignored_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        hip.kf_embed_pos.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        hip.kf_argmax_rows_state.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_memset32.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t]
        hip.kf_copy_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        hip.kf_memset2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t]
        hip.kf_embed_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        hip.kf_linear_backward.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p]
        hip.kf_linear_backward_scratch_bytes.argtypes, hip.kf_linear_backward_scratch_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_size_t
        hip.kf_gama_backward.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        hip.kf_gama_backward_scratch_bytes.argtypes, hip.kf_gama_backward_scratch_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_size_t
        hip.kf_lora_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        hip.kf_lora_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_float, C.c_void_p]
        hip.kf_lora_backward_scratch_bytes.argtypes, hip.kf_lora_backward_scratch_bytes.restype = [C.c_int] * 4, C.c_size_t
        hip.kfdbg_lora_plan.argtypes = [C.c_int] * 4 + [C.POINTER(LoraPlan)]
        hip.kf_lora_apply_status.argtypes = [C.c_int] * 5
        hip.kf_lora_apply.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        hip.kf_norm_backward.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p]
        hip.kf_norm_backward_scratch_bytes.argtypes, hip.kf_norm_backward_scratch_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_size_t
        hip.kf_rope_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int]
        hip.kf_qknorm_rope_backward.argtypes = [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong] + [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p] * 6
        hip.kf_qknorm_rope_backward_scratch_bytes.argtypes, hip.kf_qknorm_rope_backward_scratch_bytes.restype = [C.c_int] * 4, C.c_size_t
        hip.kf_d2d_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]
        hip.kf_gelu_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        hip.kf_swiglu_backward.argtypes = [C.c_void_p] * 5 + [C.c_size_t]
        hip.kf_fused_classifier.argtypes = [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        hip.kf_distill_classifier.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]
        hip.kf_gelu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        hip.kf_embed_batch.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_int, C.c_void_p]
        hip.kf_qknorm_rope_batch.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float]
        hip.kf_qkv_rope_batch.argtypes = [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
        hip.kf_qkv_rope_seqs.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
        hip.kf_attn_prefill.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
        hip.kf_norm_linear.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        hip.kf_norm_gateup_swiglu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(Weight), C.POINTER(Weight), C.c_void_p]
        hip.kf_norm_lm_head.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # the row siblings (R = 1 .. 8 activation rows over one weight pass)
        hip.kf_linear_rows.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_void_p, C.c_int64]
        hip.kf_norm_linear_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        hip.kf_norm_gateup_swiglu_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.POINTER(Weight), C.POINTER(Weight), C.c_void_p, C.c_int64, C.c_int]
        hip.kf_norm_lm_head_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.POINTER(Weight), C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        hip.kf_head_rows_scratch_bytes.argtypes, hip.kf_head_rows_scratch_bytes.restype = [C.POINTER(Weight)], C.c_size_t
        hip.kf_rows_route_counts.argtypes = [C.c_void_p, C.c_void_p]
        hip.kf_attn_decode_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
        hip.kf_attn_rows_scratch_bytes.argtypes, hip.kf_attn_rows_scratch_bytes.restype = [C.c_int] * 3, C.c_size_t
        hip.kfdbg_gemv_rows_plan.argtypes = [C.c_void_p, C.c_void_p]
        hip.kf_lm_head.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        hip.kf_head_logprob.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        hip.kf_head_logprob_scratch_bytes.argtypes, hip.kf_head_logprob_scratch_bytes.restype = [C.POINTER(Weight), C.c_int], C.c_size_t
        hip.kf_act_quant_i8.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        for f in ("kf_linear_a8", "kf_linear_a8_tiles", "kf_linear_w4a8", "kf_linear_w4a8_tiles"):
            getattr(hip, f + "_status").argtypes = [C.POINTER(Weight), C.c_int]
            getattr(hip, f).argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_attn_block_kv8_status.argtypes = [C.c_int, C.c_int, C.c_int]
        hip.kf_attn_block_kv8.argtypes = [C.c_void_p] * 12 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
        hip.kf_kv8_quant_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int]
        hip.kf_kv8_dequant_rows.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        hip.kfdbg_kv8_plan.argtypes = [C.c_int] * 5 + [C.c_void_p]
        hip.kf_attn_prefill_kv8_status.argtypes = [C.c_int] * 4
        hip.kf_attn_prefill_kv8.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
        hip.kf_embed.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_int, C.c_void_p, C.c_void_p]
        hip.kf_swiglu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_dequant.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p]
        hip.kf_quantize.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_int]
        hip.kf_init.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        hip.kf_destroy.argtypes = [C.c_void_p]
        hip.kf_sync.argtypes = [C.c_void_p]
        hip.kf_event_create.argtypes = [C.POINTER(C.c_void_p)]
        hip.kf_event_record.argtypes = [C.c_void_p, C.c_void_p]
        hip.kf_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        hip.kf_event_destroy.argtypes = [C.c_void_p]
        host.kfh_create.restype = C.c_void_p
        host.kfh_create.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 8 + [C.c_float] * 3 + [C.POINTER(C.c_int)]
        host.kfh_destroy.argtypes = [C.c_void_p]
        host.kfh_ctx.restype = C.c_void_p
        host.kfh_ctx.argtypes = [C.c_void_p]
        host.kfh_set_fuse_level.argtypes = [C.c_void_p, C.c_int]
        host.kfh_set_weight.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int]
        host.kfh_set_weight_lut.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        host.kfh_set_weight_lut_bits.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        host.kfh_tie_head.argtypes = [C.c_void_p]
        host.kfh_set_norm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        host.kfh_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        host.kfh_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        host.kfh_set_forced.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        # speculative decoding: the verify pass, the decoder, and its pure rules (host/kf_spec.hpp) without a device
        host.kfh_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        host.kfh_spec_create.restype = C.c_void_p
        host.kfh_spec_create.argtypes = [C.c_void_p, C.c_int]
        host.kfh_spec_destroy.argtypes, host.kfh_spec_destroy.restype = [C.c_void_p], None
        host.kfh_spec_set_lookup.argtypes = [C.c_void_p, C.c_int]
        host.kfh_spec_set_draft_model.argtypes = [C.c_void_p, C.c_void_p]
        host.kfh_spec_set_callback.argtypes = [C.c_void_p, SPEC_DRAFT_FN, C.c_void_p]
        host.kfh_spec_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        host.kfh_spec_stats.argtypes = [C.c_void_p, C.c_void_p]
        host.kfhdbg_spec_clip_k.argtypes = [C.c_int] * 4
        host.kfhdbg_spec_accept.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        host.kfhdbg_spec_lookup.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        host.kfhdbg_verify_refusal.argtypes = [C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
        host.kfh_set_state.argtypes = [C.c_void_p, C.c_int, C.c_int]
        host.kfh_last_error.restype = C.c_char_p
        host.kfh_host_error.restype = C.c_char_p
        host.kfh_st_open.restype = C.c_void_p
        host.kfh_st_open.argtypes = [C.c_char_p, C.c_int]
        host.kfh_st_close.argtypes = [C.c_void_p]
        host.kfh_st_count.argtypes = [C.c_void_p]
        host.kfh_st_info.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        host.kfh_st_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        host.kfh_load_hf.restype = C.c_void_p
        host.kfh_load_hf.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        host.kfh_get_config.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        host.kfh_tp_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        host.kfh_tp_area.restype = C.c_void_p
        host.kfh_tp_area.argtypes = [C.c_void_p]
        host.kfh_tp_set_peer.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        host.kfh_tp_export.argtypes = [C.c_void_p, C.c_void_p]
        host.kfh_tp_open_peer.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        host.kfh_tp_check.argtypes = [C.c_void_p]
        host.kfh_tp_group_run.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]
        host.kfh_save_kun.argtypes = [C.c_void_p, C.c_char_p]
        host.kfh_load_kun.restype = C.c_void_p
        host.kfh_load_kun.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        host.kfh_kun_write.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                       C.c_char_p]
        host.kfh_st_config_json.restype = C.c_int64
        host.kfh_st_config_json.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        host.kfh_st_blob_sizes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        host.kfh_json_to_msgpack.restype = C.c_int64
        host.kfh_json_to_msgpack.argtypes = [C.c_char_p, C.c_void_p, C.c_int64]
        host.kfh_msgpack_to_json.restype = C.c_int64
        host.kfh_msgpack_to_json.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]
        host.kfh_set_sampler.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_uint64]
        host.kfh_prefill.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        host.kfh_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        host.kfh_eval_ppl.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        host.kfh_set_prefill_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
        host.kfh_run_steps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        host.kfh_sync.argtypes = [C.c_void_p]
        host.kfh_get_tokens.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        for f in ("kfh_kcache", "kfh_vcache", "kfh_logits", "kfh_hidden"):
            getattr(host, f).restype = C.c_void_p
            getattr(host, f).argtypes = [C.c_void_p]
        host.kfh_num_graphs.argtypes = [C.c_void_p]
        host.kfh_set_engine.argtypes = [C.c_void_p, C.c_int]
        host.kfh_set_act_int8.argtypes = [C.c_void_p, C.c_int]
        host.kfh_set_act_int8_q4.argtypes = [C.c_void_p, C.c_int]
        host.kfh_set_kv_int8.argtypes = [C.c_void_p, C.c_int]
        host.kfh_kv_int8.argtypes = [C.c_void_p]
        host.kfh_set_kv_int8_prefill.argtypes = [C.c_void_p, C.c_int]
        host.kfh_kv_int8_prefill.argtypes = [C.c_void_p]
        host.kfh_kv8_route_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        for f in ("kfh_kv8_codes", "kfh_kv8_steps"):
            getattr(host, f).restype = C.c_void_p
            getattr(host, f).argtypes = [C.c_void_p, C.c_int]
        # the mode table (host/kf_host_modes.hpp) without a device: bit m of `active` = mode m of MODES is on
        host.kfhdbg_mode_refusal.argtypes = [C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
        host.kfhdbg_engine_refusal.argtypes = [C.c_uint, C.c_char_p, C.c_size_t]
        host.kfhdbg_eager_only.argtypes = [C.c_uint]
        host.kfh_set_adapter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        host.kfh_clear_adapters.argtypes = [C.c_void_p]
        host.kfh_n_adapters.argtypes = [C.c_void_p]
        host.kfh_set_a8_tile_min.argtypes = [C.c_void_p, C.c_int]
        host.kfh_a8_route_counts.argtypes = [C.c_void_p, C.c_void_p]
        host.kfh_engine_steps.argtypes = [C.c_void_p]
        host.kfh_engine_check.argtypes = [C.c_void_p]
        host.kfh_set_hot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        host.kfh_n_hot.argtypes = [C.c_void_p, C.c_int]
        host.kfh_engine_only.argtypes = [C.c_void_p, C.c_int]
        hip.kf_hot_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        hip.kf_linear_masked.argtypes = [C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_zero_cold_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        hip.kf_norm_gateup_swiglu_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(Weight), C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_linear_scratch_bytes.argtypes, hip.kf_linear_scratch_bytes.restype = [C.POINTER(Weight), C.c_int], C.c_size_t
        hip.kf_set_scratch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        hip.kf_set_dequant_arena.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        hip.kf_dequant_arena_used.argtypes, hip.kf_dequant_arena_used.restype = [C.c_void_p], C.c_size_t
        hip.kf_dequant_arena_bytes.argtypes, hip.kf_dequant_arena_bytes.restype = [C.c_void_p], C.c_size_t
        hip.kf_resident_scratch_bytes.argtypes, hip.kf_resident_scratch_bytes.restype = [], C.c_size_t
        host.kfh_set_prefill_resident.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        host.kfh_weights_changed.argtypes = [C.c_void_p]
        host.kfh_resident_bytes.argtypes, host.kfh_resident_bytes.restype = [C.c_void_p], C.c_size_t
        hip.kf_engine_workspace_bytes.argtypes, hip.kf_engine_workspace_bytes.restype = [C.c_void_p], C.c_size_t
        hip.kf_engine_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        hip.kf_engine_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        hip.kf_engine_check.argtypes = [C.c_void_p, C.c_void_p]
        hip.kf_engine_set_head.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Weight), C.c_void_p, C.c_void_p, C.c_void_p]
        hip.kf_engine_step_head.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        hip.kf_engine_reset.argtypes = [C.c_void_p, C.c_void_p]
        hip.kf_engine_head_screen_bytes.argtypes, hip.kf_engine_head_screen_bytes.restype = [C.c_int, C.c_int], C.c_size_t
        hip.kf_engine_set_head_screen.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        hip.kf_engine_screen_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]   # kf_engine_screen_statistics: three int64
        host.kfh_engine_screen_stats.argtypes = [C.c_void_p, C.c_void_p]
        hip.kf_set_canonical.argtypes = [C.c_void_p, C.c_int]
        hip.kf_get_canonical.argtypes = [C.c_void_p]
        hip.kf_set_row_unpack.argtypes = [C.c_void_p, C.c_int]
        hip.kf_get_row_unpack.argtypes = [C.c_void_p]
        hip.kf_engine_destroy.argtypes = [C.c_void_p]
        # the training steps' sequencers: koifish::GPT2Trainer (host/kf_train.cpp, kfh_gpt2_*) and koifish::Qwen3Trainer (host/kf_train_qwen3.cpp, kfh_qwen3t_*), the
        # entries both families have from one table (_TRAINER_ENTRIES); getattr raises on a name the library lacks
        for fam, acts in (("gpt2", "set_block_acts"), ("qwen3t", "set_layer_acts")):
            for name, argtypes, restype in _TRAINER_ENTRIES + [(acts, [C.c_void_p, C.c_int, C.c_void_p], C.c_int)]:
                f = getattr(host, "kfh_%s_%s" % (fam, name))
                f.argtypes, f.restype = argtypes, restype
        host.kfh_gpt2_create.restype = C.c_void_p
        host.kfh_gpt2_create.argtypes = [C.c_void_p] + [C.c_int] * 7
        host.kfh_gpt2_last_error.restype = C.c_char_p
        host.kfh_qwen3t_create.restype = C.c_void_p
        host.kfh_qwen3t_create.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.c_float, C.c_int]
        host.kfh_qwen3t_last_error.restype = C.c_char_p
        # a low-rank adapter beside a frozen layer matrix: the Qwen3 trainer only
        host.kfh_qwen3t_set_param_lora.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        host.kfh_qwen3t_set_lora_scratch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        # packed documents: (header on the host, table / positions / mask words on the device, n_valid); the Qwen3 trainer only
        host.kfh_qwen3t_set_documents.argtypes = [C.c_void_p] * 5 + [C.c_int]
        # EOE: layer-section branches, the evolve step over the swarm, the ensemble evaluation
        host.kfh_gpt2_set_branches.argtypes = [C.c_void_p, C.c_int]
        host.kfh_gpt2_n_branches.argtypes = [C.c_void_p]
        host.kfh_gpt2_set_active_branch.argtypes = [C.c_void_p, C.c_int]
        host.kfh_gpt2_active_branch.argtypes = [C.c_void_p]
        host.kfh_gpt2_evolve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32]
        host.kfh_gpt2_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        # eight decoders, one per XCD (kf_xengine_*): handles are koifish::XcdReplicas* of the host library
        host.kfh_xr_create.restype = C.c_void_p
        host.kfh_xr_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        host.kfh_xr_destroy.argtypes = [C.c_void_p]
        host.kfh_xr_set_forced.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        host.kfh_xr_set_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        host.kfh_xr_prefill.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        host.kfh_xr_run_steps.argtypes = [C.c_void_p, C.c_int]
        host.kfh_xr_check.argtypes = [C.c_void_p]
        host.kfh_xr_park.argtypes = [C.c_void_p, C.c_int, C.c_int]
        host.kfh_xr_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        host.kfh_xr_prefill_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        host.kfh_xr_set_prefill_batch.argtypes = [C.c_void_p, C.c_int]
        host.kfh_xr_set_sampler.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_uint64]
        host.kfh_xr_chat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        host.kfh_xr_chat_each.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        host.kfh_xr_set_steps_per_launch.argtypes = [C.c_void_p, C.c_int]
        host.kfh_xr_get_tokens.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        host.kfh_xr_get_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in ("kfh_xr_logits", "kfh_xr_hidden", "kfh_xr_kcache", "kfh_xr_vcache"):
            getattr(host, f).restype = C.c_void_p
            getattr(host, f).argtypes = [C.c_void_p, C.c_int]
        host.kfh_xr_variant.argtypes = [C.c_void_p, C.c_int, C.c_int]
        host.kfh_xr_stamps_enable.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        host.kfh_xr_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        # one sequence over eight tensor-parallel ranks = the eight XCDs of one launch (kf_xengine_create_tp): handles are koifish::XcdTP*
        host.kfh_xtp_create.restype = C.c_void_p
        host.kfh_xtp_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        host.kfh_xtp_destroy.argtypes = [C.c_void_p]
        host.kfh_xtp_set_forced.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        host.kfh_xtp_set_state.argtypes = [C.c_void_p, C.c_int, C.c_int]
        host.kfh_xtp_run_steps.argtypes = [C.c_void_p, C.c_int]
        host.kfh_xtp_check.argtypes = [C.c_void_p]
        host.kfh_xtp_set_steps_per_launch.argtypes = [C.c_void_p, C.c_int]
        host.kfh_xtp_get_tokens.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        host.kfh_xtp_vocab.argtypes = [C.c_void_p]
        host.kfh_xtp_stamps_enable.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        host.kfh_xtp_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        for f in ("kfh_xtp_logits", "kfh_xtp_hidden", "kfh_xtp_kcache", "kfh_xtp_vcache"):
            getattr(host, f).restype = C.c_void_p
            getattr(host, f).argtypes = [C.c_void_p]
        _libs = (hip, host)
    return _libs


def check(rc, what=""):
    if rc != 0:
        hip, _ = load()
        raise KFError("%s failed: code %d: %s" % (what, rc, hip.kf_last_error().decode()))
    return rc
