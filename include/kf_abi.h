/*
 * kf_abi.h -- C ABI of libkf_hip.so: the MI355X (gfx950) implementation of Koifish's quantized
 * transformer forward path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 * its name starts with h_.  All functions return 0 (KF_OK) or a negative KOIFISH_* code
 * (src/g_def_x.hpp:21-83) and never exit(); kf_last_error() returns the text.
 *
 * Each entry point replaces one seam of the reference; the seam is cited as
 * file:line into gruai/koifish.  A kf_ctx is single-threaded by contract (the reference drives one
 * stream from one host thread, NeuronFuse.cu:29); kernels never allocate (GTensor owns memory).
 * bf16 is carried as uint16_t bit patterns (floatX = floatGama = __nv_bfloat16, g_float.hpp:246-262).
 */
#ifndef KF_ABI_H
#define KF_ABI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t kf_bf16;
typedef struct kf_ctx kf_ctx;
typedef struct kf_graph kf_graph;

/* error codes: values of src/g_def_x.hpp:21-83 that this path can raise */
#define KF_OK 0
#define KF_INTERNAL_ERR (-11)          /* KOIFISH_INTERNAL_ERR */
#define KF_INVALID_ARGS (-20)          /* KOIFISH_INVALID_ARGS */
#define KF_OUTOF_GPUMEMORY (-100)      /* KOIFISH_OUTOF_GPUMEMORY */
#define KF_QUANT_ERR (-701)            /* KOIFISH_QUANT_ERR */
#define KF_UNSUPPORTED_DATATYPE (-1000) /* KOIFISH_UNSUPPORTED_DATATYPE */
#define KF_HIP_CHECK (-1400)           /* KOIFISH_CUDA_CHECK */
#define KF_ADAMW_MV (-5100)            /* KOIFISH_ADAMW_MV: a non-finite parameter or step met by kf_adamw (written to *d_status) */
#define KF_BLAS_UNALIGN (-2000)        /* KOIFISH_BLAS_UNALIGN: a pointer is not 16-byte aligned (gemm.cu:119-122) */
#define KF_RMS_PARAMS (-2100)          /* KOIFISH_RMS_PARAMS */

/* typNUMBER (src/g_float.hpp:84-117), same numeric values */
enum kf_dtype {
    KF_F32 = 0, KF_F64, KF_F16, KF_BF16, KF_F8E5M2, KF_F8E4M3, KF_U8, KF_I8, KF_U16, KF_I16, KF_U32, KF_I32, KF_U64, KF_I64,
    KF_Q4, KF_Q3, KF_Q2, KF_T_SIGN, KF_T_SEQ, KF_BOOL1, KF_T_BINARY, KF_T_BINARY_3, KF_T_BINARY_TILE
};

/*
 * A weight as GTensor + its quant card hand it to a kernel (GTensor.hpp:168-490, TASKA_quant
 * GeQuant.cpp:1297-1350).  `data` is the start of the `data||gama` allocation: packed Packed128 stream
 * (PackedQ.hpp:28-60; W[ne0,ne1] row-major flattened, groups of lGroup consecutive elements) or plain
 * bf16 / f8e5m2 elements.  `gama` = gama_T(GAMA) = data + szData: bf16 [R_SCALE ne0][C_SCALE ne1]
 * [ZERO nGroup][STEP nGroup] (GTensor.cpp:456-510); NULL for unquantised types.
 */
typedef struct kf_weight {
    const void* data;
    const kf_bf16* gama;
    int32_t type;   /* kf_dtype: KF_BF16, KF_F8E5M2, KF_Q4, KF_T_SIGN, KF_BOOL1, KF_T_BINARY */
    int32_t ne0;    /* rows  = out features (OC) */
    int32_t ne1;    /* cols  = in features  (IC) */
    int32_t nGroup; /* ne0*ne1/lGroup */
    int32_t lGroup; /* T_group, 128 */
    int32_t qMin, qMax, qBias;
    /* Vendor AutoAWQ tensors (GTensor::qZero / qScale, GeQuant.cpp:410; CU_Q42X_awq quantizer.cu:131-156).  Both non-NULL select the
     * AWQ GEMM layout: type = KF_Q4, data = qweight int32 [ne1, ne0/8] (TRANSPOSED: input rows), qzeros int32 [ne1/128, ne0/8],
     * qscales fp16 [ne1/128, ne0]; gama is unused.  Served by kf_linear and kf_dequant (which then writes [ne1, ne0], TransA = 0). */
    const void* qzeros;
    const void* qscales;
    /* Quant card mode (QUANT_MODE, GeQuant.hpp).  0 = KF_QUANT_GROUP: everything above.  KF_QUANT_ROW_LUT: the row-codebook 4-bit storage of
     * GeQuant::RT_NormalF / _row_lut (GeQuant.cpp:696-755; QUANT_MODE::RTNf "NF4" and the generic LUT mode share it): type = KF_Q4,
     * data = the nibble stream BIT_SET_k writes (CLI_params.cpp:2177-2190: element i of the row-major matrix in byte i/2, even i in the HIGH nibble),
     * gama = bf16 [R_SCALE ne0][C_SCALE ne1][LUT ne0 x 16] (GTensor.cpp:456-510 with the LUT at +ne0+ne1); a weight is lut[row][nibble]
     * (CU_Q42X_NF4 / CU_Q42X_lut, quantizer.cu:583-652, rc_normal = 0 as LowBit_worker's only sweep entry leaves it, GeQuant.cpp:844).
     * lGroup / nGroup / qMin / qMax / qBias are not used.  ne1 must be a multiple of 32.
     * The same mode with type = KF_Q3 / KF_Q2 is the 8- / 4-entry form (CU_Q32X_NF3 / CU_Q32X_ / CU_Q22X_, quantizer.cu:690-792): a 3- / 2-bit stream,
     * most significant bit first, 8 weights per 3 / 2 bytes, [LUT ne0 x 8] / [LUT ne0 x 4]; ne1 a multiple of 8.  KF_QUANT_ROW_RTN (type = KF_Q2) is
     * CU_Q22X_RTN (quantizer.cu:655-688): gama = [R][C][(zero, step) x ne0], weight = bf16(zero + bf16(step * id)).  By default these three are served the
     * way the reference serves them -- kf_dequant (GetDataX), and kf_linear as dequant + the bf16 product; kf_quantize builds the 3-bit normal-float form
     * (RT_NormalF asserts bits == 4 || 3).  CU_Q32X_RTN is not restated: it reads every row from row 0's stream (quantizer.cu:802, no row offset).
     * With kf_set_row_unpack they are multiplied from the packed stream (below): STORAGE UNITS -- a row is cut into units of 32 weights, 12 bytes at 3 bits and
     * 8 bytes at 2; with V = the unit's bytes read as one big-endian integer, weight i (0 .. 31) has id (V >> (93 - 3 i)) & 7, resp. (V >> (62 - 2 i)) & 3
     * (BIT_SET_k order, no un-biasing), and the value lut[row][id], resp. bf16(zero + bf16(step * id)) formed once per row into a 4-entry table. */
    int32_t quant;
    int32_t reserved_;
} kf_weight;
#define KF_QUANT_GROUP 0
#define KF_QUANT_ROW_LUT 1
#define KF_QUANT_ROW_RTN 2

/* kf_linear epilogue flags */
#define KF_EPI_NONE 0u
#define KF_EPI_RESIDUAL 1u /* y = bf16(residual + bf16(W.x))   (CU_add3 after proj_cat/down: QKV.cu:687, NeuronFuse.cu:642) */

/* ---- lifetime: InitCUDA / CUDA_cleanup / SYNC_STREAM (QKV.cu:501-571,600-615; E_GPU.cpp:152-175) ---- */
int kf_init(int device, void* hip_stream_or_null, kf_ctx** out);
int kf_destroy(kf_ctx* ctx);
int kf_sync(kf_ctx* ctx);
const char* kf_last_error(void);
const char* kf_version(void);
/* device memory (huTensor::Alloc / SerialGamaData: huTensor.cu:385-458) -- thin wrappers so that host code
 * above this ABI needs no HIP headers */
int kf_malloc(kf_ctx* ctx, size_t bytes, void** out);
int kf_free(kf_ctx* ctx, void* p);
int kf_memset(kf_ctx* ctx, void* p, int value, size_t bytes);
/* `count` 32-bit words of `value`, on the context's stream, no host sync (kf_h2d synchronises: a flag or a seed set between launches goes through this) */
int kf_memset32(kf_ctx* ctx, void* p, int32_t value, size_t count);
int kf_h2d(kf_ctx* ctx, void* dst, const void* h_src, size_t bytes);
int kf_d2h(kf_ctx* ctx, void* h_dst, const void* src, size_t bytes);
int kf_d2d(kf_ctx* ctx, void* dst, const void* src, size_t bytes);
/* `rows` rows of `width` bytes between two pitched device buffers, on the context's stream (a dense [rows, width] block into / out of a column block of wider rows) */
int kf_d2d_rows(kf_ctx* ctx, void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows);
/* hipGraph capture of whatever is launched between begin/end on the ctx stream; replay with kf_graph_launch */
int kf_graph_begin(kf_ctx* ctx);
int kf_graph_end(kf_ctx* ctx, kf_graph** out);
int kf_graph_launch(kf_ctx* ctx, kf_graph* g);
int kf_graph_destroy(kf_graph* g);
/* HIP events on the ctx stream (bench.py times kernels with these) */
int kf_event_create(void** ev);
int kf_event_record(kf_ctx* ctx, void* ev);
int kf_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* synchronises on ev_stop */
int kf_event_destroy(void* ev);

/* ---- position / token source.  Every decode kernel takes `pos` by value AND an optional device
 * pointer d_pos: when d_pos != NULL the kernel reads *d_pos instead (so one captured graph serves many
 * positions) and `pos` only bounds the launch geometry (it must be >= *d_pos). ---- */

/* GTensor::GetDataX (GTensor.hpp:399, quantizer.cu:249-392): bf16 view of any weight into `out` [ne0*ne1] */
int kf_dequant(kf_ctx* ctx, const kf_weight* w, kf_bf16* out);

/* device quantiser, GeQuant::RTN_x / YinYang (GeQuant.cpp:428-628; device twin CU_XtoQ128_ T.cu:105-175):
 * src bf16 [ne0*ne1] -> w->data (packed) and w->gama zero/step.  `w` must be fully described. symmetric: RTN only.
 * KF_F8E5M2: the storage conversion of Float2T<f8e5> (g_float.hpp:433-443): float -> half (RNE) -> high byte. */
int kf_quantize(kf_ctx* ctx, const kf_weight* w, const kf_bf16* src, int symmetric);

/* SLP::Forw -> TASKA_AxB::blasLt -> CU_mm_blasLt (Neuron.hpp:418, NeuronFuse.cu:305-381, GTensor.hpp:703-741,
 * gemm.cu:93-214): y[nTok, ne0] = alpha * x[nTok, ne1] . W^T (+ beta*y) (+ bias), fp32 accumulate, bf16 out,
 * computed straight from the packed stream (no GetDataX round trip).  x [nTok, ne1], y [nTok, ne0] row-major; from 8 token rows up
 * the product runs on MFMA tiles fed by in-register unpack (kf_gemm.hip), below that (or for K not a multiple of 128) one mat-vec per row:
 * the same values up to fp32 summation order.
 * epilogue KF_EPI_RESIDUAL adds `residual` [nTok, ne0]; `residual` MAY alias `y` (the in-place form of SelfAttention / FFN::cuFlow): every path reads a
 * residual element before it stores that element.  x must not alias y.
 * Kernels never allocate: the three storages served by "dequantise, then multiply" (the reference's own order) -- AutoAWQ tensors, the 3- / 2-bit row
 * forms, and the 4-bit row codebook for token batches the tile kernels do not cover -- use a caller-owned workspace: kf_linear_scratch_bytes says how
 * much a weight needs (0 for every PackedQ / bf16 / f8 weight), kf_set_scratch hands the context a buffer (device memory, 16-byte aligned, the caller's
 * to free after the last call that used it; not while capturing, since captured launches hold the pointer).  Too small or missing: KF_INVALID_ARGS. */
/* Summation order of the decode kernels (mat-vecs, LM head, decode attention, the persistent engine's mat-vec phases).
 *   1 (the default since round 4): the CANONICAL order kernels and the CPU oracle share (oracle/kf_oracle.c sections 4c and 6 "CANON"): every lane keeps two fused
 *     multiply-add chains (even / odd elements: one v_pk_fma_f32 per weight pair) joined by a balanced tree, the softmax works on exact power-of-two scalings with
 *     fp64 sums -- logits, greedy ids and KV rows equal the oracle's BIT FOR BIT (tests/test_gpu_canonical.py, bench.py cpu_baseline parity pass).  It is the order
 *     bench.py times.  (The persistent engine follows the switch in every phase: mat-vecs, attention slice, head.)
 *   0: products by v_dot2c_f32_bf16, the softmax in fp32 -- <= 1 bf16 ulp per output from the oracle (its order is not reproducible on a host: the instruction's
 *     internal rounding has no bit-exact model); the fewest vector instructions per weight: a few per cent faster on the latency-bound 0.6B step, ~25 % on the
 *     VALU-bound mat-vecs of a 32B model.  Greedy ids may differ from the oracle's at near-ties of the two best logits.
 * The reference's own order is cuBLASLt's and unspecified (gemm.cu:126).  Not while capturing. */
int kf_set_canonical(kf_ctx* ctx, int on);
int kf_get_canonical(kf_ctx* ctx);
/* The 3- / 2-bit row forms (KF_QUANT_ROW_LUT with KF_Q3 / KF_Q2, KF_QUANT_ROW_RTN with KF_Q2) unpacked in registers.  0 (the default): every entry treats them as
 * before -- kf_linear dequantises into the scratch and multiplies the bf16 copy, the fused decode entries refuse them.  1: kf_linear (one token and token batches,
 * every epilogue), kf_norm_linear (1-3 matrices of one form), kf_norm_gateup_swiglu, kf_linear_multi, kf_qkv_rope_batch / _seqs and kf_gateup_swiglu_batch read
 * the packed stream once: a lane owns units of 32 weights (kf_weight.quant above), looks four ids up with one v_perm_b32 per byte plane of the row's table, and
 * sums EXACTLY as it would over the 4-bit row codebook holding the same values (the same ids as nibbles, a 16-entry table whose first 8 / 4 entries are the
 * row's own): that "4-bit twin" gives the same bits through every one of these entries, in both summation orders, and it is how the launch is planned.
 * Shape rule: ne1 a multiple of 128, the row tables aligned to their own size (16 / 8 / 4 bytes).  Where it fails kf_linear keeps the dequantise route and the
 * fused entries refuse with KF_BLAS_UNALIGN.  Not served in either setting: kf_lm_head / kf_norm_lm_head, kf_embed* (TokenEmbed::cuInfer asserts on Q3), the
 * masked (hot-row) forms, the *_rows entries, the engines.  kf_linear_scratch_bytes does not change.  Not while capturing. */
int kf_set_row_unpack(kf_ctx* ctx, int on);
int kf_get_row_unpack(kf_ctx* ctx);
size_t kf_linear_scratch_bytes(const kf_weight* w, int nTok);
int kf_set_scratch(kf_ctx* ctx, void* scratch, size_t bytes);
/* RESIDENT dequantised copies for token batches (prompt prefill).  The reference dequantises a quantised weight in front of EVERY token-batch product
 * (GTensor::GetDataX -> cuBLASLt, SLP::Forw); with 288 GB of HBM the bf16 form of an inference model's matrices can simply stay: the routes of kf_linear,
 * kf_linear_multi, kf_qkv_rope_batch and kf_gateup_swiglu_batch that dequantise into the scratch (>= 1024 token rows; with an arena from 320) put the copy into `arena` instead the first
 * time they meet a weight (or a stacked Q | K | V / interleaved gate | up set) and find it there afterwards -- same values, same tile kernels, no dequantise
 * launches, and kf_linear takes the bf16 tile kernels from 320 rows (o_proj / down_proj of a prompt: 64 x 128 / 64 x 64 tiles of kf_gemm3.hip, in k-pieces when a
 * kf_set_scratch workspace of kf_resident_scratch_bytes() is lent).
 * Copies are keyed by the weights' data pointers: the caller promises the weights do not change while the arena holds them (inference; after a weight update
 * call kf_set_dequant_arena again -- it forgets every copy).  arena: device memory, 16-byte aligned, the caller's; NULL switches the feature off; when it is
 * full, further weights go through the scratch as before.  kf_dequant_arena_used: bytes filled so far.  Not while capturing. */
int kf_set_dequant_arena(kf_ctx* ctx, void* arena, size_t bytes);
size_t kf_dequant_arena_used(kf_ctx* ctx);
size_t kf_dequant_arena_bytes(kf_ctx* ctx); /* the size of the arena set, 0: none -- a trainer that changes quantised weights in place asks before it multiplies them */
size_t kf_resident_scratch_bytes(void); /* a kf_set_scratch workspace of at least this size lets kf_linear's resident-copy route cut short token batches into k-pieces */
int kf_linear(kf_ctx* ctx, const kf_weight* w, const kf_bf16* x, kf_bf16* y, const kf_bf16* bias, int nTok, float alpha, float beta,
              uint32_t epilogue, const kf_bf16* residual);

/* ---- tensor parallel (no counterpart in the reference, which is single-GPU: QKV.cu:503) ----
 * column-split projections (o_proj, down_proj) give un-rounded fp32 partial row dots per rank ... */
int kf_linear_f32(kf_ctx* ctx, const kf_weight* w_shard, const kf_bf16* x_shard, float* y_partial);
/* ... that are combined in rank order after an all-gather: out = bf16(residual + bf16(sum_r partials[r][:])) */
int kf_tp_reduce(kf_ctx* ctx, const float* partials, int n_ranks, int n, const kf_bf16* residual_or_null, kf_bf16* out);

/* The exchange itself without a collective library: every rank owns a receive area that every other rank can address (xGMI peer-to-peer mapping
 * of kf_tp_alloc memory, exported / opened with the kf_tp_ipc_* calls; ranks of one process just pass pointers).  kf_linear_f32_push is kf_linear_f32
 * whose epilogue stores each fp32 row dot, tagged, into this rank's slot of EVERY rank's area (one 8-byte system-scope store per rank and row);
 * kf_tp_reduce_recv waits for the tags of all ranks' slots and forms out = bf16(residual + bf16(sum_r partial_r)) in rank order -- the bits of
 * kf_tp_reduce.  kf_tp_lm_head runs the LM head on this rank's vocabulary rows and pushes its first maximum (value, GLOBAL row) to every rank;
 * kf_tp_pick takes the first maximum over the ranks, updates the decode state {token, pos + 1} like kf_norm_lm_head does, and advances the
 * generation word.  All of it is plain kernel launches on the context's stream: the TP step captures into a hipGraph.
 * Area layout (8-byte granules): [2 exchange buffers][world][n_max] vector slots, then [world][2] pick slots; kf_tp_recv_bytes gives the size;
 * the area must be zero before the first step (kf_tp_alloc zeroes it).  `index` numbers the exchanges of one step (0 .. per_step - 2; the
 * pick uses per_step - 1); exchanges with even index use buffer 0, odd ones buffer 1.  A poll that outlasts ~2^24 re-reads sets *d_err
 * (1 + rank waited for) instead of hanging. */
typedef struct kf_tp_comm {
    int32_t rank, world; /* world <= 8 */
    int32_t n_max;       /* rows of a vector slot */
    uint32_t per_step;   /* exchanges per token including the pick */
    void* recv;          /* this rank's receive area */
    void* peer[8];       /* peer[r]: rank r's receive area as addressable from this process (peer[rank] == recv) */
    uint32_t* d_step;    /* device word, zero at start: generation */
    int32_t* d_err;      /* device word, zero at start */
    void* d_push;        /* kf_tp_push_bytes(per_step) bytes of device memory: the push descriptors, written by kf_tp_commit */
} kf_tp_comm;
size_t kf_tp_recv_bytes(int world, int n_max);
size_t kf_tp_push_bytes(uint32_t per_step);
int kf_tp_commit(kf_ctx* ctx, const kf_tp_comm* comm); /* once every peer[] is set, before the first kf_linear_f32_push (not while capturing) */
int kf_tp_alloc(kf_ctx* ctx, size_t bytes, void** out);              /* device memory other processes / devices may map; zeroed */
int kf_tp_ipc_export(kf_ctx* ctx, void* p, unsigned char handle[64]); /* hipIpcGetMemHandle */
int kf_tp_ipc_open(kf_ctx* ctx, const unsigned char handle[64], void** out);
int kf_tp_ipc_close(kf_ctx* ctx, void* p);
int kf_linear_f32_push(kf_ctx* ctx, const kf_weight* w_shard, const kf_bf16* x_shard, const kf_tp_comm* comm, uint32_t index);
int kf_tp_reduce_recv(kf_ctx* ctx, const kf_tp_comm* comm, uint32_t index, int n, const kf_bf16* residual_or_null, kf_bf16* out);
int kf_tp_lm_head(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* norm_w, float eps, const kf_weight* w_shard, kf_bf16* logits_shard, int row0,
                  const kf_tp_comm* comm, void* head_scratch);
int kf_tp_pick(kf_ctx* ctx, const kf_tp_comm* comm, int32_t* d_state, int32_t* d_tokens_out);

/* ---- sparse ("EOE" / hot-neuron) forward: D_matmul_sparse (src/Utils/GST_float.cpp:306-318) with the hot[] array of CS_Picker
 * (src/Manifold/SparseNeuron.cpp:20-29; Neuron.hpp:265-285: one int per FFN row, 1 = hot):  y[i] = (hot[i] == 1 ? W[i,:].x : 0) (+ bias[i]).
 * The mask is turned into a list of hot rows once (kf_hot_rows: ascending indices, their number to *d_count) and the products walk that list, so
 * cold rows cost no HBM traffic: algorithmic bytes = n_hot / ne0 of the dense product's.  Hot rows carry every bit of kf_linear's rows.
 * kf_norm_gateup_swiglu_masked is the FFN form (FFN::cuInfer with the mask on the gate / up rows): cold rows of `act` are SwiGLU(0, 0) = 0.
 * kf_zero_cold_columns is the token-batch form (FFN::cuFlow, after kf_gateup_swiglu_batch): y[r][i] = 0 for every row r < rows where d_hot[i] != 1, the
 * hot columns untouched -- so they keep every bit of the dense batched product. */
int kf_hot_rows(kf_ctx* ctx, const int32_t* d_hot, int n, int32_t* d_rows, int32_t* d_count);
int kf_linear_masked(kf_ctx* ctx, const kf_weight* w, const kf_bf16* x, kf_bf16* y, const kf_bf16* bias_or_null, const int32_t* d_rows, int n_hot);
int kf_zero_cold_columns(kf_ctx* ctx, kf_bf16* y, const int32_t* d_hot, int rows, int cols);
int kf_norm_gateup_swiglu_masked(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* norm_w_or_null, float eps, const kf_weight* gate, const kf_weight* up,
                                 kf_bf16* act, const int32_t* d_rows, int n_hot);

/* LayerNormal::cuFlow -> CU_rms_infer (Neuron.hpp:453, T.cu:561-573, layernorm.cuh:800-859) */
int kf_rmsnorm(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* w, kf_bf16* y, int rows, int dim, float eps, float* rstd_or_null);

/* ROPE::cuInfer (Neuron.hpp:364, rope.cu:645-672): per-head RMSNorm (CU_rms_forward_v2) then rotate-half RoPE
 * (CU_rope2_v0) on q [n_head*hd] and on the new key row k [n_kv*hd], in place.  wq_norm/wk_norm may be NULL.
 * rope_table: fp32 [max_pos][hd/2][2] = (cos, sin) built by kf_rope_table_host. */
int kf_qknorm_rope(kf_ctx* ctx, kf_bf16* q, kf_bf16* k, const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rope_table, int pos,
                   const int32_t* d_pos, int n_head, int n_kv, int hd, float eps);
/* host: fills h_table [n_pos][hd/2][2] with cosf/sinf(pos / powf(theta, 2j/hd)) (operator.cuh:734-772) */
int kf_rope_table_host(float* h_table, int n_pos, int hd, float theta);

/* attention triple of SelfAttention::cuInfer (QKV.cu:669-673; operator.cuh:572-632,251-277,649-668), fused,
 * full causal length.  q bf16 [n_head*hd] (already normed+roped), kcache/vcache: layer base, row t at
 * t*kv_stride elements; out bf16 [n_head*hd]; scratch: kf_attn_scratch_bytes(), zero-filled ONCE by the caller (the
 * kernel keeps its arrival counters at zero between launches). */
int kf_attn_decode(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* kcache, const kf_bf16* vcache, kf_bf16* out, int pos, const int32_t* d_pos,
                   int n_head, int n_kv, int hd, int kv_stride, void* scratch);
size_t kf_attn_scratch_bytes(int n_head, int hd);

/* Relu::Forw -> CU_swiglu_v0 (Neuron.hpp:384, Activation.cu:85-93) */
int kf_swiglu(kf_ctx* ctx, const kf_bf16* gate, const kf_bf16* up, kf_bf16* out, int n);
/* T1p1(CU_add3) (QKV.cu:687, packedN.cuh:866-875) */
int kf_add(kf_ctx* ctx, const kf_bf16* a, const kf_bf16* b, kf_bf16* out, int n);
/* TokenEmbed::cuInfer/OnEmbed (NeuronFuse.cu:176-218, embed.cuh:54-132).  token by value, or *d_token */
int kf_embed(kf_ctx* ctx, const kf_weight* w, int token, const int32_t* d_token, kf_bf16* out);
/* Head4Token::cuInfer_1 + sample_argmax (NeuronFuse.cu:842-862, GoPT.cpp:602-612): logits bf16 [ne0] (required) and
 * the greedy id (first maximum) to d_argmax_out (device int32; NULL: logits only, no pick).  scratch: kf_head_scratch_bytes(). */
int kf_lm_head(kf_ctx* ctx, const kf_weight* w, const kf_bf16* x, kf_bf16* logits, int32_t* d_argmax_out, void* scratch_or_null);
size_t kf_head_scratch_bytes(void);
/* The LM head scored against target ids: what Fish_ppl / Fish::Eval_ppl compute token by token as log(P_softmax(tokens[i + 1], logits, nVocab))
 * (Evaluate.cpp:19-94, CLI_params.cpp:1692-1705), for n_rows rows at once and without the [n_rows x ne0] logit matrix being written.
 * x [n_rows][ldx] bf16 is the hidden state AFTER the final RMSNorm (kf_rmsnorm over the rows), 16-byte aligned, ldx >= ne1 a multiple of 8.  Per row t:
 *   logit[v]   = bf16(fp32 dot(x[t], W[v])), rounded exactly as kf_lm_head / kf_linear store it (token-batch products sum in MFMA order);
 *   logprob[t] = (logit[target] - m) - log(sum_v exp(logit[v] - m)), m the row maximum, fp32, the fixed exp / log of kf_fused_classifier.  The same number as
 *                log(P_softmax(..)) of the reference WITHOUT its underflow to log(0) = -inf for a token the model finds unlikely;
 *   lse[t]     = m + log(sum);   top1[t] = the FIRST maximum of the bf16 logits (sample_argmax, GoPT.cpp:602-612), ties to the lower id.
 * d_targets[t] < 0: the row is not scored, logprob[t] = 0, lse / top1 are still written.  d_targets[t] >= ne0 (ids the host never saw) gives NaN and reads nothing;
 * callers with host-side ids refuse them with KF_INVALID_ARGS (kfh_score).  Every storage type is served: a bf16 head with ne1 % 64 == 0 by MFMA tiles whose epilogue
 * keeps three numbers per row and vocabulary tile, the rest through kf_linear on panels of rows (its kf_set_scratch workspace as for kf_linear).
 * scratch: kf_head_logprob_scratch_bytes(head, n_rows) bytes, 16-byte aligned -- for a bf16 head at most 1/16 of the logit matrix's bytes. */
size_t kf_head_logprob_scratch_bytes(const kf_weight* head, int n_rows);
int kf_head_logprob(kf_ctx* ctx, const kf_weight* head, const kf_bf16* x, int64_t ldx, int n_rows, const int32_t* d_targets, float* d_logprob,
                    float* d_lse_or_null, int32_t* d_top1_or_null, void* scratch);

/* ---- fused forms used by the decode step (same arithmetic as the calls above, fewer launches) ---- */
/* [RMSNorm(x, norm_w)] -> up to 3 projections sharing the normed input.  y[i] rows go to y[i], or, when
 * y_pos_stride[i] != 0, to y[i] + pos*y_pos_stride[i] (K.out/V.out alias the KV-cache row: TGraph.cpp:198-207) */
int kf_norm_linear(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* norm_w_or_null, float eps, int n_w, const kf_weight* const* w,
                   kf_bf16* const* y, const int64_t* y_pos_stride, int pos, const int32_t* d_pos);
/* [RMSNorm] -> gate & up -> SwiGLU -> act [ffn]   (FFN::cuInfer NeuronFuse.cu:615-637) */
int kf_norm_gateup_swiglu(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* norm_w_or_null, float eps, const kf_weight* gate, const kf_weight* up,
                          kf_bf16* act);
/* q/k-norm + RoPE + attention in one pass: q raw [n_head*hd], k_raw [n_kv*hd] (the new key before norm/rope,
 * written normed+roped into kcache row pos), v row must already sit in vcache row pos.
 * Requirement on the caches (also kf_attn_decode, kf_engine_step): with d_pos the launch is laid out for positions up to `pos` (the bound) and loads K / V rows
 * up to that bound before the device position is known; rows past the real position are masked by a zero probability, not by a select, so they must hold
 * FINITE values (allocate the caches zero-filled, as KVCache::Init does: 0 * NaN would poison the output). */
int kf_attn_block(kf_ctx* ctx, const kf_bf16* q_raw, const kf_bf16* k_raw, kf_bf16* kcache, const kf_bf16* vcache, kf_bf16* out,
                  const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rope_table, int pos, const int32_t* d_pos, int n_head, int n_kv,
                  int hd, int kv_stride, float eps, void* scratch);
/* [final RMSNorm] + LM head + greedy pick; then state update for graph replay: d_state[0] = next token,
 * d_state[1] += 1 (position), d_tokens_out[old pos] = next token (when non-NULL).  d_state == NULL: logits only (kf_sample follows). */
int kf_norm_lm_head(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* norm_w_or_null, float eps, const kf_weight* w, kf_bf16* logits,
                    int32_t* d_state, int32_t* d_tokens_out, void* scratch);
/* writes the decode state {token, pos} (a one-thread kernel: capturable, no host staging buffer) */
int kf_set_state(kf_ctx* ctx, int32_t* d_state, int token, int pos);
/* embed lookup driven by device state: token = (d_forced && d_forced[pos] >= 0) ? d_forced[pos] : d_state[0] */
int kf_embed_state(kf_ctx* ctx, const kf_weight* w, const int32_t* d_state, const int32_t* d_forced, kf_bf16* out);

/* ---- row siblings of the fused mat-vec entries: n_rows = 1 .. 8 activation rows against ONE pass over the weights (no counterpart in the reference).  The use is
 * the verify pass of speculative decoding: a token and up to seven drafted continuations of one sequence, whose rows are consecutive positions pos0 .. pos0 +
 * n_rows - 1.  Row r is x + r * x_stride (elements; a multiple of 8); the pass is eager and the host knows the position, so there is no d_pos form.
 * In the canonical order (kf_set_canonical 1, the default) row r carries EVERY BIT of the one-token entry called on row r at position pos0 + r -- kf_linear
 * with nTok = 1, kf_norm_linear, kf_norm_gateup_swiglu, kf_norm_lm_head: the lanes per weight row come from the same rule with the same arguments, and with them
 * the per-lane chains, the lane tree, the RMSNorm sums and the epilogue arithmetic.
 * Sharing: for 4-bit group weights (PackedQ, qBias 0 or 8) and bf16 weights in the canonical order, from two rows up, every 16-byte weight block is loaded and
 * dequantised once and multiplied into one accumulator pair per row; rows whose activations do not fit 80 KiB of LDS together are cut into panels of equal size, one
 * weight pass per panel.  Everything else -- the v_dot2c order, f8 / 2-bit / 1-bit / row-codebook weights, one row, rows longer than 40 832 elements -- runs the
 * one-token launch row by row inside the same entry: the same results, no sharing.  kf_rows_route_counts says how many rows took which route since kf_init.
 * AutoAWQ-layout weights, sparse forms, bias, alpha / beta: not served (KF_UNSUPPORTED_DATATYPE for AWQ as the one-token entries; the others have no argument).
 * Refusals are the one-token entries' own, plus KF_INVALID_ARGS for n_rows outside 1 .. 8 and KF_BLAS_UNALIGN for an x_stride that is not a multiple of 8. */
/* y[r] = W . x[r] (+ residual[r]); row r of y / residual at r * y_stride / r * residual_stride elements; `residual` MAY alias `y` (with equal strides) */
int kf_linear_rows(kf_ctx* ctx, const kf_weight* w, const kf_bf16* x, int64_t x_stride, kf_bf16* y, int64_t y_stride, int n_rows, uint32_t epilogue,
                   const kf_bf16* residual, int64_t residual_stride);
/* [RMSNorm per row] -> up to 3 projections; row r of projection i goes to y[i] + r * y_row_stride[i] + (pos0 + r) * y_pos_stride[i]: K.out / V.out land in the
 * cache rows pos0 .. pos0 + n_rows - 1 with y_row_stride 0 and y_pos_stride = the cache's row stride (y_pos_stride NULL: all zero) */
int kf_norm_linear_rows(kf_ctx* ctx, const kf_bf16* x, int64_t x_stride, const kf_bf16* norm_w_or_null, float eps, int n_w, const kf_weight* const* w,
                        kf_bf16* const* y, const int64_t* y_row_stride, const int64_t* y_pos_stride_or_null, int pos0, int n_rows);
/* [RMSNorm per row] -> gate & up -> SwiGLU -> act[r] at r * act_stride */
int kf_norm_gateup_swiglu_rows(kf_ctx* ctx, const kf_bf16* x, int64_t x_stride, const kf_bf16* norm_w_or_null, float eps, const kf_weight* gate, const kf_weight* up,
                               kf_bf16* act, int64_t act_stride, int n_rows);
/* [final RMSNorm per row] + LM head + greedy pick per row: d_top1[r] = the first maximum of row r's bf16 logits (ties to the lower id), always; the logits
 * themselves to logits + r * logits_stride when logits != NULL.  No decode-state update.  scratch: kf_head_rows_scratch_bytes(w) bytes, 16-byte aligned. */
int kf_norm_lm_head_rows(kf_ctx* ctx, const kf_bf16* x, int64_t x_stride, const kf_bf16* norm_w_or_null, float eps, const kf_weight* w, kf_bf16* logits_or_null,
                         int64_t logits_stride, int32_t* d_top1, int n_rows, void* scratch);
size_t kf_head_rows_scratch_bytes(const kf_weight* w);
/* kf_attn_decode for n_rows = 1 .. 8 consecutive queries of one sequence in ONE launch: query r (prepared: normed + roped, at q + r * row_stride) sits at position
 * pos0 + r and attends to keys 0 .. pos0 + r; out row r at out + r * row_stride.  The K / V rows of the whole batch, positions pos0 .. pos0 + n_rows - 1, must be in
 * the cache before the call (kf_norm_linear_rows into the cache rows, then kf_qknorm_rope_batch on the K rows in place): query r reads the keys of rows 0 .. r.
 * Canonical order: each row equals kf_attn_decode at its position bit for bit -- every query cuts its keys into kf_attn_decode's slices at its own position and owns
 * its arrival counters and partials.  The v_dot2c order: the one-token launch per row.  scratch: kf_attn_rows_scratch_bytes(n_head, hd, n_rows) bytes, 16-byte
 * aligned, zero-filled ONCE by the caller (the counters return to zero). */
int kf_attn_decode_rows(kf_ctx* ctx, const kf_bf16* q, int64_t row_stride, const kf_bf16* kcache, const kf_bf16* vcache, kf_bf16* out, int pos0, int n_rows,
                        int n_head, int n_kv, int hd, int kv_stride, void* scratch);
size_t kf_attn_rows_scratch_bytes(int n_head, int hd, int n_rows);
/* out2[0]: activation rows served with the shared unpack, out2[1]: rows served by one-token launches, by the four entries above since kf_init */
int kf_rows_route_counts(kf_ctx* ctx, int64_t* out2);

/* GeneratOnPrompt::Sample, non-greedy branch (GoPT.cpp:614-630; LogitsInfo::TopK / UpdateLogits / TopP / Qu_FlipCoin, GoPT.cpp:632-790):
 * picks the next token from bf16 logits[n] on the device -- candidate set exactly as TOPK_heap::Select builds it (indices
 * 0..k-2 plus the first maximum over i >= k-1), softmax with temperature, top-p cut, xorshift64* coin.  d_rng_state: one uint64 in device
 * memory (LogitsInfo::rng_state, seeded with config.common.seed), advanced once per call.  Writes *d_token (when non-NULL) and, when
 * d_state is non-NULL, the decode-state update of kf_norm_lm_head.  temperature == 0 or top_k == 1 is the greedy path: use kf_lm_head.
 * d_forced (optional, n_forced entries, -1 = free): when the token of the NEXT position is teacher-forced (prompt prefill through the
 * decode path) nothing is drawn and the rng state is left alone, as the reference's prefill loop never samples (GoPT.cpp:1139-1146).
 * KF_INVALID_ARGS unless 2 <= top_k < n/2 (the reference asserts it), top_k <= 1024, temperature > 0, top_p > 0. */
int kf_sample(kf_ctx* ctx, const kf_bf16* logits, int n, int top_k, float temperature, float top_p, uint64_t* d_rng_state, int32_t* d_token,
              int32_t* d_state, int32_t* d_tokens_out, const int32_t* d_forced, int n_forced);

/* kf_sample with the candidate set the reference's TopK is evidently meant to keep: the top_k LARGEST logits (ties at the k-th value towards the
 * lower token index; candidates ordered by logit, equal logits by index).  Not what the reference computes (its heap keeps indices 0..k-2, see
 * kf_sample); offered beside it.  Everything else -- softmax with temperature, top-p cut, xorshift coin, state update -- is identical. */
int kf_sample_topk(kf_ctx* ctx, const kf_bf16* logits, int n, int top_k, float temperature, float top_p, uint64_t* d_rng_state, int32_t* d_token,
                   int32_t* d_state, int32_t* d_tokens_out, const int32_t* d_forced, int n_forced);

/* ---- GPT-2 family forward pieces (BASELINE config 3) */
/* LayerNorm forward with affine weight and bias (LayerNormal::cuFlow for the GPT-2 family -> CU_lm_forward, layernorm.cuh:226-300):
 * y = bf16((x - mean) * rstd * w + b), rstd = 1/sqrtf(var + eps); bias may be NULL; mean / rstd [rows] fp32 are optional outputs. */
int kf_layernorm(kf_ctx* ctx, const kf_bf16* x, const kf_bf16* w, const kf_bf16* bias_or_null, kf_bf16* y, int rows, int dim, float eps, float* mean_or_null,
                 float* rstd_or_null);
/* GELU, tanh form (Relu::Forw GELU -> gelu_forward_kernel2, Activation.cu:23-40) */
int kf_gelu(kf_ctx* ctx, const kf_bf16* x, kf_bf16* y, size_t n);

/* kf_qknorm_rope_batch for a training batch: n_tok rows = sequences of seq_len tokens back to back, positions 0 .. seq_len - 1 in each; the per-head
 * 1/rms of the q / k norms (fp32, before the bf16 rounding the forward applies to it) go to rstd_q [n_tok * n_head] / rstd_k [n_tok * n_kv] when given:
 * what kf_norm_backward needs for the q/k-norm backward. */
int kf_qknorm_rope_train(kf_ctx* ctx, kf_bf16* q, kf_bf16* k, const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rope_table, int n_tok, int seq_len, int64_t q_stride,
                         int64_t k_stride, int n_head, int n_kv, int head_dim, float eps, float* rstd_q_or_null, float* rstd_k_or_null);

/* kf_attn_prefill for n_seq independent sequences of n_tok tokens each (a training batch), positions 0 .. n_tok - 1, in ONE launch: sequence s owns rows
 * s * n_tok .. (s + 1) * n_tok - 1 of q / out (row stride q_stride) and of k / v (row stride kv_stride; e.g. the column blocks of a fused [B*T, 3C] buffer).
 * Same arithmetic as kf_attn_prefill (the MFMA tile kernel).  head_dim 64 or 128. */
int kf_attn_prefill_batch(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, kf_bf16* out, int n_tok, int64_t q_stride, int n_head, int n_kv, int head_dim,
                          int kv_stride, int n_seq);

/* the same with a row stride of its own for out: a training step reads q out of the fused [rows, 3C] buffer (q_stride 3C) and writes a dense [rows, C] out (out_stride C),
 * which saves the copy of the q columns (GPT-2's c_attn output: QKV.cu's fused qkv, /root/reference/src/Device/CUDA/QKV.cu) */
int kf_attn_prefill_batch_strided(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, kf_bf16* out, int n_tok, int64_t q_stride, int64_t out_stride, int n_head,
                                  int n_kv, int head_dim, int kv_stride, int n_seq);

/* Causal attention backward for n_seq sequences of T tokens each, stored back to back in every tensor (the training path's SDPA backward:
 * cudnn-frontend in the reference, QKV.cu:130-315, 427-447).  q: rows of n_head * head_dim, k / v: rows of n_kv * head_dim (GQA: n_head a multiple of
 * n_kv), all with row stride ld_qkv (e.g. the column blocks of a fused q|k|v buffer); o (the forward output) and dO: n_head * head_dim with stride ld_o;
 * dq (n_head heads) and dk, dv (n_kv heads, summed over the query heads of a group) with stride ld_d.  scale 1/sqrt(head_dim), fp32 softmax recomputed
 * from q and k, bf16 stores.  head_dim 64 or 128 (KF_UNSUPPORTED_DATATYPE otherwise).
 * scratch: kf_attn_backward_scratch_bytes(T, n_head, n_seq) bytes (the rows' log-sum-exp and dO.O). */
size_t kf_attn_backward_scratch_bytes(int T, int n_head, int n_seq);
int kf_attn_backward(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, long long ld_qkv, const kf_bf16* o, const kf_bf16* dO, long long ld_o, kf_bf16* dq,
                     kf_bf16* dk, kf_bf16* dv, long long ld_d, int T, int n_head, int n_kv, int head_dim, int n_seq, void* scratch);

/* Embedding forward of a training batch (encoder_forward -> encoder_forward_kernel3, kernel/embed.cuh:20-45,372-376): out[bt][c] = bf16(wte[tokens[bt]][c] + wpe[bt % T][c]), fp32 sum, round to nearest.
 * wte rows ldw apart; an id outside [0, V) reads row 0. */
int kf_embed_pos(kf_ctx* ctx, const kf_bf16* wte, long long ldw, const kf_bf16* wpe, const int32_t* tokens, int B, int T, int C, int V, kf_bf16* out);
/* The greedy pick (sample_argmax, GoPT.cpp:602-612: first maximum over float(logits)) of n_rows rows of bf16 logits [n] (rows ld apart) at once, each followed by the
 * decode-state update of kf_norm_lm_head for sequence d_seq[row] of a [n_seq][4] state array {token, pos, ..}: d_tokens_out[seq * tokens_stride + pos] = id (when non-NULL),
 * state = {id, pos + 1}.  The head of a batch of prompts: ONE product over the rows' hidden states (kf_linear), one pick launch. */
int kf_argmax_rows_state(kf_ctx* ctx, const kf_bf16* logits, long long ld, int n, int n_rows, const int32_t* d_seq, int32_t* d_states, int32_t* d_tokens_out, int tokens_stride);
/* block b (b < n_blocks) of src, blocks src_stride bytes apart, copied to d_dst_table[b] + dst_offset -- d_dst_table is a DEVICE array of device pointers (16-byte aligned
 * destinations); sizes, strides and the offset multiples of 16 bytes.  One launch scatters the K / V rows of a batch of prompts into the prompts' own caches
 * (the reference re-aims K.out / V.out at the cache rows of ONE sequence, TGraph.cpp:198-207). */
int kf_copy_blocks(kf_ctx* ctx, void* const* d_dst_table, size_t dst_offset, const void* src, size_t src_stride, size_t block_bytes, int n_blocks);
/* value into `width` bytes of each of `rows` rows `pitch` bytes apart, on the context's stream (the padded logit columns of a step) */
int kf_memset2d(kf_ctx* ctx, void* p, size_t pitch, int value, size_t width, size_t rows);

/* Embedding backward (encoder_backward, kernel/embed.cuh:380-470): dout [B*T, C] is the gradient of  wte[tokens[bt]] + wpe[t].
 *   dwpe [T, C]        += sum over the batch                         (NULL: no position table, e.g. a RoPE model)
 *   dwte [V, ldw >= C] += the rows of every position holding that token, in ascending position order   (NULL: skipped)
 * fp32 sums, bf16(sum + old) stores; tokens outside [0, V) are skipped.  Deterministic (no atomics), all on the device. */
int kf_embed_backward(kf_ctx* ctx, kf_bf16* dwte_or_null, long long ldw, kf_bf16* dwpe_or_null, const kf_bf16* dout, const int32_t* tokens, int B, int T, int C, int V);

/* Linear layer backward (SLP::Back, NeuronFuse.cu:495-547; matmul_backward, kernel/gemm.cu:326-370).  w [OC, IC] in any PackedQ / f8 / bf16 storage,
 * dequantised to bf16 first exactly as the reference's GetDataX does; deltaIn [n, OC] is the gradient of the layer's output, inp [n, IC] its input:
 *   delta [n, IC]  = (accumulate_delta ? delta : 0) + deltaIn . W        (NULL: skipped)
 *   gW    [OC, IC] += deltaIn^T . inp                                     (NULL: skipped -- isFixWeight; the bf16 gradient of a quantised weight's master copy)
 *   gBias [OC]     += column sums of deltaIn                              (NULL: no bias)
 * fp32 accumulation, bf16 stores (beta = 1 adds the stored bf16 value).  OC a multiple of 64 and >= 128 (so is n when gW is wanted), IC a multiple of 8.
 * scratch: kf_linear_backward_scratch_bytes(OC, IC, n) bytes of device memory, 256-byte aligned (the dequantised weight; the fp32 partial tiles of the split-K weight-gradient
 * launch, >= 64 MiB, or the transposed copies of shapes too small for the 256 x 256 tile kernel; the bias column-sum slabs).  Contents need not be initialised and
 * are not kept between calls; results do not depend on them (the split-K partial sums are added in a fixed order). */
size_t kf_linear_backward_scratch_bytes(int OC, int IC, int n);
int kf_linear_backward(kf_ctx* ctx, const kf_weight* w, const kf_bf16* deltaIn, const kf_bf16* inp_or_null, kf_bf16* delta_or_null, kf_bf16* gW_or_null,
                       kf_bf16* gBias_or_null, int n, int accumulate_delta, void* scratch);

/* The other way to train a quantised layer, "train_target": "gama" (SLP::Back with w->gama_param, NeuronFuse.cu:538-549 -> GamaBack_v0 -> CU_GamaBack_2,
 * kernel/quantizer.cu:66-94; GTensor::InitGamaParam, GTensor.cpp:903-945): the packed integers stay frozen and each group's (zero, step) pair is the parameter.
 * With w = step (q - qBias) - zero and dW = deltaIn^T . inp (the gW of kf_linear_backward, never written here), per 128-column group g of row r:
 *   gGama[g]          = bf16(gGama[g]          + scale * (- sum_{c in g} dW[r, c]))                      (zero)
 *   gGama[nGroup + g] = bf16(gGama[nGroup + g] + scale * (+ sum_{c in g} dW[r, c] (q[r, c] - qBias)))     (step)
 * -- the order of the blob's [ZERO nGroup][STEP nGroup] and of the reference's gW[idG], gW[idG + nG].  q - qBias is the integer read from the Packed128 stream; the
 * weight is never dequantised.  Sums in fp32 (MFMA accumulation over the n token rows, then the 128 columns), accumulating into gGama as gW / gBias do (kf_adamw zeroes
 * what it consumed).  scale: CU_GamaBack_2 divides by nSample (SLP::Back passes B, not B * T); 1.0f is the chain rule's value and what this project's trainer passes.
 * Deterministic: no atomics; a cut over n leaves fp32 partials in the scratch that a second launch adds in slab order; results do not depend on the scratch's contents.
 * Served: KF_QUANT_GROUP storage with lGroup 128 of KF_Q4 (qBias 0 or 8), KF_T_SIGN, KF_BOOL1.  Refusals launch nothing: IC % 128, OC % 64, OC < 128 or n % 64 violated,
 * a null pointer or a missing scratch: KF_INVALID_ARGS; AutoAWQ layout, row-LUT / row-RTN modes, any other type: KF_UNSUPPORTED_DATATYPE; deltaIn / inp / gGama not
 * 16-byte aligned or scratch not 256-byte aligned: KF_BLAS_UNALIGN.  scratch: kf_gama_backward_scratch_bytes(OC, IC, n) bytes (0 for a refused shape); the entry is not
 * told its size -- the caller sizes it with that function.  The input gradient stays with kf_linear_backward(..., gW = NULL). */
size_t kf_gama_backward_scratch_bytes(int OC, int IC, int n);
int kf_gama_backward(kf_ctx* ctx, const kf_weight* w, const kf_bf16* deltaIn, const kf_bf16* inp, kf_bf16* gGama, int n, float scale, void* scratch);

/* The third way: the matrix W [OC, IC] stays frozen in whatever storage it has and a low-rank pair trains beside it -- the LORA branch of SLP::Forw / SLP::Back
 * (NeuronFuse.cu:286-302, 343-358, 384-423, 453-468: HIERARCH_LorAB::Forw / Back; construction SparseNeuron.cpp:210-264).  a [r, IC], b [OC, r] bf16 row-major,
 * x [n, IC], y [n, OC].  s is the reference's sAB and multiplies BOTH products of a direction, as there: the adapter's effective weight is s^2 b a -- on purpose, a
 * caller who wants the usual alpha / r passes s = sqrt(alpha / r).
 *   kf_lora_forward    ax [n, r]     = bf16(s x a^T)                     kept for the backward (the reference's Ax)
 *                      y  [n, OC]    = bf16(y + s ax b^T)                in place, after the base product (kf_linear, epilogue included) has written y
 *   kf_lora_backward   adelta [n, r] = bf16(s deltaIn b)                 at offset 0 of the scratch (the reference's Adelta)
 *                      delta [n, IC] = bf16(delta + s adelta a)          ALWAYS on top of what kf_linear_backward(..., gW = NULL) of the base left there
 *                      gB [OC, r]    = bf16(gB + s deltaIn^T ax)         g = [gA (r IC) | gB (OC r)], one vector
 *                      gA [r, IC]    = bf16(gA + s adelta^T inp)
 * Sums in fp32 (MFMA accumulation), bf16 roundings to nearest even exactly where written.  The gradients ACCUMULATE into g as gW and gGama do (kf_adamw zeroes what it
 * consumed); the reference writes them with beta = 0, the same on a zeroed buffer.  Deterministic: no atomics; the weight side cuts n into slabs whose fp32 partials a
 * finish launch adds in slab order; results do not depend on the scratch's contents.  Launches: forward one; backward four (transposed copies of a and b, the row side,
 * both gradients' slabs, the finish) -- csrc/kf_lora_plan.h.
 * Served: r 16, 32 or 64; OC and IC multiples of 64 and >= 128; n a multiple of 64 and >= 64.  Refusals launch nothing: no context, another shape or a null pointer:
 * KF_INVALID_ARGS; an operand not 16-byte aligned or the scratch not 256-byte aligned: KF_BLAS_UNALIGN.  scratch: kf_lora_backward_scratch_bytes(r, OC, IC, n) bytes
 * (0 for a refused shape), sized by the caller. */
size_t kf_lora_backward_scratch_bytes(int r, int OC, int IC, int n);
int kf_lora_forward(kf_ctx* ctx, const kf_bf16* a, const kf_bf16* b, int r, int OC, int IC, const kf_bf16* x, kf_bf16* y, kf_bf16* ax, int n, float s);
int kf_lora_backward(kf_ctx* ctx, const kf_bf16* a, const kf_bf16* b, int r, int OC, int IC, const kf_bf16* deltaIn, const kf_bf16* inp, const kf_bf16* ax, kf_bf16* delta,
                     kf_bf16* g, int n, float s, void* scratch);

/* The same pair applied at inference: the reference runs its LORA branch inside SLP::Forw on every forward (NeuronFuse.cu:286-302), decode, prompt and scoring alike.
 * Per row the arithmetic is kf_lora_forward's, unchanged:   ax [r] = bf16(s x a^T),   y [OC] = bf16(y + s ax b^T)   in place, after the base product (kf_linear,
 * epilogue included) has written y.  Any n >= 1; the form follows from n alone (csrc/kf_lora_plan.h, kf::lora_apply_plan):
 *   n >= 2   the tile form: kf_lora_forward's kernel with a row bound.  Rows >= n of the last 32-row tile load as zero and store nothing (neither y nor ax): every row
 *            < n has the bits kf_lora_forward gives it on the input zero-padded to a multiple of 64 rows.  n_w must be 1.  ax [n, r] is written when given; NULL: not kept.
 *   n == 1   the vector form: n_w <= 3 adapters that share the input row x (q | k | v, gate | up) in ONE launch; h_a / h_b / h_OC / h_y are HOST arrays of n_w entries
 *            (device pointers a [r, IC], b [OC_i, r], y_i [OC_i]; the y_i are separate -- a V row lies inside the KV cache); r, IC, x and s are shared.  ax is ignored.
 *            No workgroup waits for another: each recomputes the r dot products and owns 64 output rows of one adapter.  The order of every sum is FIXED:
 *              ax_j   lane l (of 64) adds the products of the 8-element chunks l, l + 64, l + 128, ... of the contraction to one fp32 accumulator, chunks ascending,
 *                     k ascending inside a chunk (fma; the product of two bf16 is exact in fp32, so fma and multiply-add agree); a lane without a chunk holds 0.  The 64
 *                     lane sums p_l meet in a butterfly, six steps m = 32, 16, 8, 4, 2, 1, each p_l <- p_l + p_(l xor m) on all lanes at once.  ax_j = bf16(s p_0).
 *              y_m    one fp32 chain over j = 0 .. r - 1 ascending of ax_j b [m, j] (fma), then bf16(y_m + s sum): the multiply by s and the addition round to fp32 each.
 *            tests/lora_apply_restate.py restates this in numpy, bit for bit.  The two forms sum in different orders: equal on exact operands, within rounding otherwise.
 * Deterministic, no atomics, no scratch.  Served: r 16, 32 or 64; OC_i and IC multiples of 64 and >= 128; n >= 1; 1 <= n_w <= 3, n_w > 1 only with n == 1 --
 * kf_lora_apply_status(r, OC, IC, n, n_w) answers KF_OK or the refusal for ONE adapter of such a group without a device (a pure host function).  Refusals launch nothing:
 * no context, another shape, a null pointer (ax excepted): KF_INVALID_ARGS; a, b, x, y or ax not 16-byte aligned: KF_BLAS_UNALIGN. */
int kf_lora_apply_status(int r, int OC, int IC, int n, int n_w);
int kf_lora_apply(kf_ctx* ctx, int n_w, const kf_bf16* const* h_a, const kf_bf16* const* h_b, int r, const int* h_OC, int IC, const kf_bf16* x, kf_bf16* const* h_y,
                  kf_bf16* ax_or_null, int n, float s);

/* LayerNorm / RMSNorm backward (LayerNormal::cuFlow, backward branch, T.cu:605-646: layernorm_backward -> layernorm_backward_kernel10, layernorm.cuh:311-503;
 * RMS: CU_rms_back_llmc, layernorm.cuh:863-1051).  mean == NULL selects RMSNorm.  dinp (the residual-path gradient on entry) becomes
 * bf16(dinp + dL/dinp); dweight (and dbias, LayerNorm with a bias) accumulate the sums over the rows: bf16(sum + old).  rstd (and mean) are the forward's
 * per-row outputs.  scratch: kf_norm_backward_scratch_bytes(rows, dim, mean != NULL) bytes of device memory, 8-byte aligned. */
size_t kf_norm_backward_scratch_bytes(int rows, int dim, int is_layernorm);
int kf_norm_backward(kf_ctx* ctx, kf_bf16* dinp, kf_bf16* dweight, kf_bf16* dbias_or_null, const kf_bf16* dout, const kf_bf16* inp, const kf_bf16* weight,
                     const float* mean_or_null, const float* rstd, int rows, int dim, void* scratch);

/* RoPE backward (the transpose of the rotate-half rotation of kf_qknorm_rope), in place on a gradient d [n_tok rows of n_head * head_dim, row stride
 * `stride`]: row t belongs to position pos0 + t % seq_len (seq_len = n_tok for one sequence; a batch of equal-length sequences stored back to back
 * passes its sequence length).  The q/k-norm that precedes RoPE in the forward is an RMSNorm over head_dim: its backward is kf_norm_backward with
 * rows = n_tok * n_head and dim = head_dim. */
int kf_rope_backward(kf_ctx* ctx, kf_bf16* d, const float* rope_table, int pos0, int n_tok, int seq_len, long long stride, int n_head, int head_dim);

/* The backward of kf_qknorm_rope_train in ONE entry (the backward branches of ROPE::cuFlow, kernel/rope.cu, and of LayerNormal::cuFlow, T.cu:605-646, over
 * n_tok * n_head rows of head_dim), fed by kf_attn_backward's dq | dk | dv -- column blocks of fused rows with the common row stride ld_d:
 *   per head row: g = R^T d  (the transpose of the rotate-half rotation, as kf_rope_backward; row t at position t % seq_len), kept in fp32;
 *   then kf_norm_backward's RMS branch with the forward's rstd: d_raw = bf16((w g - norm (sum_i w_i g_i raw_i / head_dim) rstd) rstd), norm = raw rstd.
 * One bf16 rounding fewer than kf_rope_backward + kf_norm_backward.  q_raw / k_raw: the PRE-norm q and k of the forward, row strides ld_qraw / ld_kraw; rstd_q
 * [n_tok * n_head] / rstd_k [n_tok * n_kv]: what kf_qknorm_rope_train wrote.  Outputs, all dense: dq_raw [n_tok, n_head * head_dim], dk_raw [n_tok, n_kv * head_dim]
 * (written, not accumulated: they feed kf_linear_backward as they are), dv_out [n_tok, n_kv * head_dim] = a plain copy of dv (dv and dv_out both NULL: skipped);
 * dwq / dwk [head_dim] ACCUMULATE bf16(sum over the rows + old), as kf_norm_backward's dweight.  Deterministic: no atomics, the row sums go through the scratch in a
 * fixed order, and nothing depends on the scratch's contents.  Served: head_dim 64 or 128 (otherwise KF_UNSUPPORTED_DATATYPE), n_head a multiple of n_kv, any
 * n_tok >= 1 a multiple of seq_len, strides multiples of 8 no smaller than their rows.  Refusals launch nothing: a null pointer (one of dv / dv_out alone included), a
 * bad shape or stride: KF_INVALID_ARGS; a tensor or the table not 16-byte aligned, the scratch not 8-byte aligned: KF_BLAS_UNALIGN.
 * scratch: kf_qknorm_rope_backward_scratch_bytes(n_tok, n_head, n_kv, head_dim) bytes (0 for a refused shape). */
size_t kf_qknorm_rope_backward_scratch_bytes(int n_tok, int n_head, int n_kv, int head_dim);
int kf_qknorm_rope_backward(kf_ctx* ctx, const kf_bf16* dq, const kf_bf16* dk, const kf_bf16* dv_or_null, long long ld_d, const kf_bf16* q_raw, long long ld_qraw,
                            const kf_bf16* k_raw, long long ld_kraw, const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rstd_q, const float* rstd_k,
                            const float* rope_table, int n_tok, int seq_len, int n_head, int n_kv, int head_dim, kf_bf16* dq_raw, kf_bf16* dk_raw, kf_bf16* dv_out_or_null,
                            kf_bf16* dwq, kf_bf16* dwk, void* scratch);

/* ---- Packed documents (supervised fine-tuning: the reference's P_SFT phase -- BATCH_INPUT::UpdatePadMask, TokenSet/DataLoader.cpp:1560-1630, and SelfAttention
 * with isVarLen, Manifold/TGraph.cpp:97 -- which pads one sample per batch row; here any number of documents share the rows of a batch).
 * THE LAYOUT: a batch is n_rows rows.  Document d owns rows [row0[d], row0[d] + len[d]); documents are ascending and do not overlap; 1 <= len[d] <= max_len (the
 * rope table's length); a document may start at any row.  A row in no document is a GAP ROW.  Row r of document d stands at position r - row0[d] and attends
 * causally to its own document's rows only; a gap row stands at position 0, attends to nothing and receives nothing: the forward writes zeros to its output row,
 * the backward zeros to its dq | dk | dv rows -- with launches whose writes for gap rows are proportional to their number.
 * kf_attn_docs_plan (host only, no device or context needed) writes the workgroup tables of the launches below to h_table: a kf_attn_docs_header, then three
 * tables of kf_attn_docs_entry, one entry per tile of a document (forward: ATTN_TILE_COLS / (n_head / n_kv) = 128 / GQ tokens; the two backward launches: 128
 * rows), longest key range first, then the gap rows as entries with gap = 1.  The caller copies the whole table to the device once and hands both to the
 * launches: the header on the host (read at the call), the copy on the device (16-byte aligned).  kf_attn_docs_table_bytes: the table's size, 0 for a layout
 * the plan refuses.  Refusals (KF_INVALID_ARGS, nothing written): a null pointer, n_doc < 1, a length outside [1, max_len], overlapping or descending
 * documents, a document past n_rows, a head geometry kf_attn_prefill_batch or kf_attn_backward refuse, table_bytes too small. */
#define KF_ATTN_DOCS_MAGIC 0x53434F44
typedef struct kf_attn_docs_header {
    int32_t magic, n_rows, n_head, n_kv, head_dim, n_doc, max_len;
    int32_t off[3], n[3]; /* forward, dQ launch, dK/dV launch: first entry (in 16-byte units from the table's start) and entry count */
    int32_t doc_rows, gap_rows, reserved_;
} kf_attn_docs_header;
typedef struct kf_attn_docs_entry {
    int32_t row0, len, tile, gap; /* the document's first row and length (gap = 1: a run of gap rows), this entry's tile inside it */
} kf_attn_docs_entry;
size_t kf_attn_docs_table_bytes(const int32_t* row0, const int32_t* len, int n_doc, int n_rows, int max_len, int n_head, int n_kv, int head_dim);
int kf_attn_docs_plan(const int32_t* row0, const int32_t* len, int n_doc, int n_rows, int max_len, int n_head, int n_kv, int head_dim, void* h_table, size_t table_bytes);
/* kf_attn_prefill_batch_strided on a table: the tile kernel in its one-key-half form for every document length (never the paired form); the output rows of a
 * document are bit for bit what kf_attn_prefill_batch_strided writes for that document alone (n_seq = 1, n_tok = len) on its tile route; gap rows of out are
 * written as zero.  Refusals launch nothing: a null pointer or a header that is not this geometry's: KF_INVALID_ARGS; misaligned rows or table: KF_BLAS_UNALIGN. */
int kf_attn_prefill_docs(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, kf_bf16* out, const kf_attn_docs_header* h_header, const void* d_table,
                         int64_t q_stride, int64_t out_stride, int n_head, int n_kv, int head_dim, int kv_stride);
/* kf_attn_backward on a table: dq, dk, dv rows of a document are bit for bit kf_attn_backward on that document alone (n_seq = 1, T = len); gap rows of dq | dk | dv
 * are written as zero.  scratch: kf_attn_backward_docs_scratch_bytes(n_rows, n_head) bytes (log-sum-exp and dO.O, indexed by global row). */
size_t kf_attn_backward_docs_scratch_bytes(int n_rows, int n_head);
int kf_attn_backward_docs(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, long long ld_qkv, const kf_bf16* o, const kf_bf16* dO, long long ld_o, kf_bf16* dq,
                          kf_bf16* dk, kf_bf16* dv, long long ld_d, const kf_attn_docs_header* h_header, const void* d_table, int n_head, int n_kv, int head_dim, void* scratch);
/* kf_qknorm_rope_train / kf_qknorm_rope_backward with the position of every row given: pos [n_tok] int32 on the device, each in [0, the rope table's length),
 * in place of t % seq_len.  The bits are the plain entries' at equal positions (dwq / dwk: the same fixed summation order over the n_tok rows). */
int kf_qknorm_rope_train_pos(kf_ctx* ctx, kf_bf16* q, kf_bf16* k, const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rope_table, int n_tok, const int32_t* pos,
                             int64_t q_stride, int64_t k_stride, int n_head, int n_kv, int head_dim, float eps, float* rstd_q_or_null, float* rstd_k_or_null);
int kf_qknorm_rope_backward_pos(kf_ctx* ctx, const kf_bf16* dq, const kf_bf16* dk, const kf_bf16* dv_or_null, long long ld_d, const kf_bf16* q_raw, long long ld_qraw,
                                const kf_bf16* k_raw, long long ld_kraw, const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rstd_q, const float* rstd_k,
                                const float* rope_table, int n_tok, const int32_t* pos, int n_head, int n_kv, int head_dim, kf_bf16* dq_raw, kf_bf16* dk_raw,
                                kf_bf16* dv_out_or_null, kf_bf16* dwq, kf_bf16* dwk, void* scratch);
/* After kf_fused_classifier with a mask: the rows it skipped (mask word has 0x10000, F_IGNORE_LOSS) still hold raw logits where every other row holds a gradient.
 * This writes zeros to exactly those rows of buf [n_rows, P] (P a multiple of 8, 16-byte aligned) and touches no other row. */
int kf_zero_ignored_rows(kf_ctx* ctx, kf_bf16* buf, int n_rows, int P, const int32_t* mask);

/* Activation backward (Relu::Back, Activation.cu:283-320).  GELU, in place on the incoming gradient (Activation_backward_inplace ->
 * gelu_backward_inplace_kernel, Activation.cu:42-78): d = bf16(gelu'(x) * d) with x the pre-activation.  SwiGLU (CU_swiglu_back_v0,
 * Activation.cu:245-260): delta_gate = bf16(delta * up * sig * (1 + gate * (1 - sig))), delta_in_out = bf16(delta * gate * sig), sig = sigmoid(gate). */
int kf_gelu_backward(kf_ctx* ctx, kf_bf16* d_in_out, const kf_bf16* x, size_t n);
int kf_swiglu_backward(kf_ctx* ctx, kf_bf16* delta_in_out, kf_bf16* delta_gate, const kf_bf16* gate, const kf_bf16* up, size_t n);

/* Fused classifier of the GPT-2 / training forward (fused_classifier, src/Device/CUDA/kernel/fused_classifier.cuh:68-140, launched by Head4Token at
 * NeuronFuse.cu:923 as <<<dB*T, 1024>>>(logits, losses, nullptr, rLoss, targets, dB, T, V, Vp, devMask, write_dlogits)): for every row of
 * logits [B*T, P] (V valid entries, P the padded row length, a multiple of 8):  losses[row] -= log(softmax(row)[target])  (accumulates, as the
 * reference does), then -- write_dlogits != 0 -- the row is overwritten by bf16((prob - onehot(target)) * dloss), and probs (may be NULL) gets
 * bf16(prob).  Rows whose mask word (may be NULL) has bit 0x10000 (MASK_FLAG::F_IGNORE_LOSS, DataLoader.hpp:78) are skipped entirely.
 * Same thread decomposition and reduction order as the reference; exp / log are this library's fixed fp32 recipes. */
int kf_fused_classifier(kf_ctx* ctx, kf_bf16* logits, float* losses, kf_bf16* probs_or_null, float dloss, const int32_t* targets, int B, int T, int V, int P,
                        const int32_t* mask_or_null, int write_dlogits);

/* Distilling classifier: the fused classifier with a teacher's logits beside the hard labels (logit distillation as BitNet-style training of low-bit students
 * uses it).  The reference states the intent only (src/Fuzi/Distillation.hpp is a stub, src/Device/CUDA/Distill.cu an attention-relation loss, not built here),
 * so the contract is this comment.  Per row of logits [B*T, P] (z: V valid bf16 entries) and of teacher [B*T, teacher_ld] (u), tau = temperature,
 * it = 1 / tau (fp32), a = ce_weight, b = kd_weight, m_z / m_u the row maxima:
 *     p_i  = exp(z_i - m_z) / S1            S1 = sum exp(z_i - m_z)
 *     pt_i = exp((z_i - m_z) it) / St       St = sum exp((z_i - m_z) it)
 *     qt_i = exp((u_i - m_u) it) / Ut       Ut = sum exp((u_i - m_u) it)
 *     A    = sum exp((u_i - m_u) it) ((u_i - m_u) - (z_i - m_z)) it
 *     KL   = A / Ut - log Ut + log St       = KL(qt || pt), not clamped
 *     CE   = -log p[target]
 *     losses[row] += a CE + b tau^2 KL      (accumulates, as the fused classifier's)
 *     kd[row]      = KL                     (kd may be NULL; written, not accumulated; only when b != 0)
 *     dlogit_i     = bf16((a (p_i - [i == target]) + b tau (pt_i - qt_i)) dloss)   over the logits, when write_dlogits != 0
 * Rows whose mask word has bit 0x10000 are skipped entirely; the columns [V, P) and [V, teacher_ld) are never read or written; the teacher is never written.
 * With a == 0 the targets are not read (NULL is accepted), with b == 0 neither teacher nor kd is (NULL is accepted).
 *
 * Order of operations (fp32; exp / log the fixed recipes of the fused classifier; no fma except where one is named; tests/distill_restate.py is this in numpy).
 * One workgroup of 1024 threads per row.  Thread t owns the 8-element vectors i = ceil(V/8) + t - 1024, i - 1024, ... >= 0 and visits them in that order, highest
 * first, the elements of a vector ascending.  "Block max / sum" is the fused classifier's reduction: an xor butterfly (offsets 16, 8, 4, 2, 1) inside each group
 * of 32 consecutive threads, then the same butterfly over the 32 group results.
 *   1. As the fused classifier: per thread a running (max, sum) over its z -- on a new maximum sum *= exp(old - new), then sum += exp(z - max) --; m_z = block max;
 *      sum_t *= exp(max_t - m_z); S1 = block sum; r1 = 1 / S1.  In the same sweep, b != 0: the thread's maximum of u; m_u = block max.
 *   2. b != 0.  Per thread, from 0, over its elements in the visiting order:  dz = z - m_z;  du = u - m_u;  st = st + exp(dz it);  eu = exp(du it);  ut = ut + eu;
 *      at = fma(eu, (du - dz) it, at).  St, Ut, A = the block sums of st, ut, at.  KL = (A / Ut - log Ut) + log St;  rt = 1 / St;  ru = 1 / Ut.
 *      The z and the u sums run through one chain and one tree, so u == z gives Ut == St bit for bit, A == 0 and KL == 0.0 at any temperature.
 *   3. c = a (-log(exp(z[target] - m_z) r1)) when a != 0;  w = (b tau) tau;  c = fma(w, KL, c) when both weights are set, c = w KL when a == 0;  losses[row] += c.
 *   4. write_dlogits: per element  g = a (exp(dz) r1 - [i == target]) when a != 0, else 0;  b != 0:  g = fma(b tau, exp(dz it) rt - exp(du it) ru, g);
 *      dlogit = bf16(g dloss).
 * a = 1, b = 0 is the fused classifier bit for bit (1 x is exact); u == z adds exactly nothing to a gradient.
 * KF_INVALID_ARGS, nothing launched: NULL logits or losses; NULL teacher with b != 0; NULL targets with a != 0; a weight negative or not finite, or both zero;
 * a temperature not finite or <= 0; P < V or teacher_ld < V; teacher rows that overlap the logits' rows.  KF_BLAS_UNALIGN: P or teacher_ld no multiple of 8,
 * logits or teacher not 16-byte aligned. */
int kf_distill_classifier(kf_ctx* ctx, kf_bf16* logits, const kf_bf16* teacher_or_null, int64_t teacher_ld, float* losses, float* kd_or_null, float dloss,
                          const int32_t* targets_or_null, int B, int T, int V, int P, const int32_t* mask_or_null, float ce_weight, float kd_weight, float temperature,
                          int write_dlogits);

/* ---- training kernel path (BASELINE config 3), first piece: the AdamW parameter update CU_adamw_p (src/Device/CUDA/Optimizer.cu:393-442)
 * as PIPE_Adamw::Update launches it (Optimizer.cu:630-646; TASKA_1p1, packedN.cuh:612-643: 512 threads x 8 bf16 per thread).
 * params / grads bf16 [n] (grads are zeroed), gm / gv: first and second moments, mv_type KF_BF16 (floatMV = bf16) or KF_F32.
 * g = grad_scale*grad; m = sAtB(g, m, beta1); v = sAtB(g*g, v, beta2); step = (m/beta1_correction) / (sqrtf(v/beta2_correction) + eps);
 * p -= lr*weight_decay*p + lr*step.  bf16 stores use the reference's seeded stochastic rounding (CU_Float2T<bf16>, packedN.cuh:62-72;
 * SquirrelNoise5 keyed on the launch geometry, which this entry reproduces), so results are bit-identical to the restatement in oracle/.
 * n must be a multiple of 8.  A thread that meets a non-finite parameter or step stores nothing and writes KF_ADAMW_MV to *d_status
 * (device int32, optional). */
int kf_adamw(kf_ctx* ctx, kf_bf16* params, kf_bf16* grads, void* gm, void* gv, size_t n, int mv_type, float learning_rate, float beta1, float beta2,
             float beta1_correction, float beta2_correction, float eps, float weight_decay, float grad_scale, uint32_t seed, int32_t* d_status);
/* kf_adamw with grad_scale read on the device: *d_grad_scale (one float, 4-byte aligned; loaded once per thread) in place of the by-value float -- there is no
 * product of two scales.  Bit for bit kf_adamw with the same float.  The clip factors of kf_grad_norms are what it is made for: d_scale + i. */
int kf_adamw_scaled(kf_ctx* ctx, kf_bf16* params, kf_bf16* grads, void* gm, void* gv, size_t n, int mv_type, float learning_rate, float beta1, float beta2,
                    float beta1_correction, float beta2_correction, float eps, float weight_decay, const float* d_grad_scale, uint32_t seed, int32_t* d_status);

/* ---- gradient norms: the sum of squares of EVERY gradient tensor of a step in one launch, |g| and the clip factors left on the device (kf_gradnorm.hip,
 * kf_gradnorm_plan.h).  The reference: GTensor::Length per tensor (huTensor.cu:665-704: memset, atomicAdd kernel, blocking read-back), grad_scale = gnorm > gclip ?
 * gclip / gnorm : 1 formed on the host (Optimizer.cu:756-774), Optimizer::gClip over the whole gradient (Optimizer.cpp:276-308), g_step = sqrt(sum gnorm^2) printed
 * with the loss.  Here nothing is read back and no sum depends on scheduling.
 *
 * The table: n_tensors pairs (grads[i], n[i]); n[i] a positive multiple of 8, grads[i] 16-byte aligned.  Tensor i is cut into ceil(n[i] / 4096) chunks of 4096
 * elements (512 threads x 8 bf16, kf_adamw's geometry); it owns the workgroups [wg0[i], wg0[i + 1]), wg0[0] = 0.  kf_grad_norms_plan writes {pointer, n, wg0,
 * no_clip} once into the caller's scratch (device memory, 256-byte aligned, kf_grad_norms_scratch_bytes long: the table, then one fp64 partial per chunk) with one
 * blocking copy -- outside the step -- and the context remembers the layout under the scratch's address; kf_grad_norms refuses a scratch it has not planned.  The
 * gradient tensors and the scratch must stay where they are, and the table untouched, while the plan is in use; kf_grad_norms rewrites the partials inside the
 * scratch.  Each plan carries a stamp, in the table and on the host: a scratch whose memory was given back and handed out again since (same address, other contents)
 * makes kf_grad_norms a no-op that reports NaN sums and norms and unit scales -- the pointers of a table that is not the planned one are never followed.
 *
 * The summation order, complete (every addition fp64; the product of two bf16 values is exact in fp64, so only the additions round):
 *   1. thread t of chunk k holds elements 4096 k + 8 t .. + 7 of the tensor: ss = 0; ss = fma(x, x, ss) for the 8 elements in element order (elements at or past n
 *      are not loaded: such a thread holds 0);
 *   2. the 64 lanes of a wave: six pairwise levels, level j adding the sums of adjacent blocks of 2^j lanes ((l0 + l1) + (l2 + l3) ...); the 8 waves of the
 *      workgroup: 0 + w0 + w1 + ... + w7 in wave order.  One partial per chunk;
 *   3. a tensor's np partials: per = ceil(np / 256); run r = partials [r per, min((r + 1) per, np)) added in order from 0; then the 256 runs in order from 0;
 *   4. the total: the per-tensor sums in tensor order from 0.
 * Outputs, all on the device: d_sumsq fp64 [n_tensors + 1] (the last entry: the total), d_gnorm float [n_tensors + 1] = (float)sqrt(sumsq) (the root in fp64,
 * narrowed once), d_scale float [n_tensors]; with c = gclip and the division in fp32:
 *   KF_CLIP_REPORT  every scale 1.0f
 *   KF_CLIP_TENSOR  scale[i] = gnorm[i] > c ? c / gnorm[i] : 1.0f
 *   KF_CLIP_GLOBAL  scale[i] = gnorm[n_tensors] > c ? c / gnorm[n_tensors] : 1.0f
 * and 1.0f in every mode for a tensor whose no_clip byte was set at plan time (it still counts in the total).  A non-finite sum needs no special case: a NaN
 * norm compares false and gives 1.0f, +inf gives 0.0f, and kf_adamw's own non-finite guard does the rest.
 * kf_grad_norms_forget drops what the context remembers of a scratch (before the scratch is freed: its address may be handed out again); unknown: KF_OK.
 * n_tensors is at most 4096: the total is one thread's serial chain over the per-tensor sums (measured at 580 tensors; microseconds at the cap).
 * Refusals are KF_INVALID_ARGS, launch nothing, and kf_last_error names the cause: a null pointer; n_tensors < 1 or above 4096; an n that is not a positive multiple of 8; a
 * misaligned pointer; a scratch that is missing, not 256-byte aligned, too short, or (kf_grad_norms) not planned for n_tensors on this context; an unknown mode;
 * gclip not finite or <= 0 in a clipping mode.  kf_grad_norms_scratch_bytes is 0 for a list the entries refuse. */
enum kf_clip_mode { KF_CLIP_REPORT = 1, KF_CLIP_TENSOR = 2, KF_CLIP_GLOBAL = 3 };
size_t kf_grad_norms_scratch_bytes(int n_tensors, const long long* n);
int kf_grad_norms_plan(kf_ctx* ctx, int n_tensors, const kf_bf16* const* grads, const long long* n, const uint8_t* no_clip_or_null, void* scratch, size_t scratch_bytes);
int kf_grad_norms(kf_ctx* ctx, const void* scratch, int n_tensors, int mode, float gclip, double* d_sumsq, float* d_gnorm, float* d_scale);
int kf_grad_norms_forget(kf_ctx* ctx, const void* scratch);

/* ---- Muon, the reference's default optimiser (CLI_params.hpp:627), for a hidden matrix W [ne0 = out][ne1 = in] with ne0 >= ne1: PIPE_Muon::CU_core
 * (src/Device/CUDA/Optimizer.cu:498-583; set up by PIPE_Muon::Update, src/Device/Pipe.cpp:16-57).  The reference's column-major X (m = ne1, n = ne0) is W^T, its
 * A = X X^T is W^T W [ne1, ne1]; isTrans is forced off there and is not built here.  grad_scale is NOT applied on this path, as in the reference (CU_muon_mG reads
 * grads0 as they are).  No entry allocates or synchronises with the host: the sums of squares stay on the device (the reference's D2e read-backs are not restated).
 * Sums of squares are deterministic: one fp64 partial per workgroup, added in workgroup order by a one-workgroup follow-up launch (the reference: atomicAdd).
 * Refusals are KF_INVALID_ARGS and launch nothing: ne0 < ne1, a dimension that is no multiple of 64, n_iter outside [0, 16], a tensor that is not 16-byte aligned,
 * a scratch that is missing, not 256-byte aligned or shorter than kf_muon_scratch_bytes(ne0, ne1) (0 for a shape the entries refuse).
 *
 * scratch layout (every offset a multiple of 256; up = round up to 256):  A [ne1][ne1] bf16 at 0;  B [ne1][ne1] bf16 at up(2 ne1^2);  X [ne0][ne1] bf16 at
 * 2 up(2 ne1^2) (kf_muon: the momentum kernel's output, orthogonalised in place);  X' (the ping-pong buffer) at + up(2 ne0 ne1);  ceil(ne0 ne1 / 4096) fp64 partial
 * sums;  two doubles: sum X^2, and kf_muon's wnorm^2 when the caller passes no destination.  Contents need not be initialised; after a call A and B hold the last
 * iteration's matrices. */
size_t kf_muon_scratch_bytes(int ne0, int ne1);
/* CU_muon_mG (Optimizer.cu:93-109) in TASKA_1p1 geometry (512 threads x 8 bf16, as kf_adamw):  mG <- sr(mG + (1 - mui)(g - mG)), then X <- sr(g + mui (mG' - g)) with
 * mG' the bf16 value just stored; sr = the seeded stochastic bf16 store of kf_adamw, one threshold per thread.  *d_sumsq (device) = sum of X^2 over the stored X.
 * n a multiple of 8, at most 2^28. */
int kf_muon_momentum(kf_ctx* ctx, kf_bf16* mG, const kf_bf16* grads, kf_bf16* X, size_t n, float mui, uint32_t seed, double* d_sumsq);
/* The orthogonalisation of CU_core (Optimizer.cu:522-570), X [ne0, ne1] in place:  alpha = 1 / (sqrt(sum X^2) + eps_muon) in fp64 on the device, narrowed to float;
 * X <- bf16(X + (alpha - 1) X);  n_iter times:  A = bf16(X^T X),  B = bf16(b A + bf16(c A A)),  X <- bf16(a X + bf16(X B))  (the bf16 stores of cublasGemmEx and
 * cublasAxpyEx; fp32 accumulation);  X <- bf16(X + beta X), beta = sqrt(max(1, ne1 / ne0)) - 1, which is 0 for every shape this entry takes.  A, A A and B are
 * computed on and above the diagonal only and mirrored: symmetric bit for bit.  d_sumsq NULL: the entry sums X itself. */
int kf_newton_schulz(kf_ctx* ctx, kf_bf16* X, int ne0, int ne1, const double* d_sumsq_or_null, float eps_muon, int n_iter, float a, float b, float c, void* scratch,
                     size_t scratch_bytes);
/* CU_muon_update (Optimizer.cu:111-131), same geometry and threshold rule:  p <- sr((1 - lr weight_decay) p + (-lr) X);  grads are zeroed;  *d_wnormsq (device,
 * optional) = sum of the stored p^2, the reference's wnorm^2. */
int kf_muon_apply(kf_ctx* ctx, kf_bf16* params, kf_bf16* grads, const kf_bf16* X, size_t n, float lr, float weight_decay, uint32_t seed, double* d_wnormsq_or_null);
/* The three in order, as CU_core runs them, with a / b / c = 3.4445 / -4.7750 / 2.0315 (Pipe.hpp:131) and one seed for both elementwise kernels (task_11.config.seed). */
int kf_muon(kf_ctx* ctx, kf_bf16* params, kf_bf16* grads, kf_bf16* mG, int ne0, int ne1, float lr, float weight_decay, float mui, float eps_muon, int n_iter,
            uint32_t seed, void* scratch, size_t scratch_bytes, double* d_wnormsq_or_null);

/* ---- EOE, "Evolutionary Optimization of Experts": Fuyou::Exploitation (src/Device/CUDA/Optimizer.cu:439-484) of ONE follower matrix towards the head's, one pass.
 * x [ne0, ne1] bf16: the follower's master, updated in place; head [ne0, ne1] bf16: read only.  n = ne0 ne1.  The algorithms carry the values of the three live
 * members of Fuyou_params::ALGORITHM (CLI_params.hpp:194-204; GENE_MUTATION is commented out in the reference and not built).
 * The draw is this project's own (the reference's per-row curand XORWOW streams cannot be restated): counter-based, one hash per element, for flat row-major index i
 *     h = SquirrelNoise5(i, seed) (the noise of kf_adamw);  b0 .. b3 = the bytes of h, low to high;  r = float(b0 + b1 + b2) * (1.0f / 765.0f)
 * r stands for the reference's clip((N(0,1) + 3) / 6, 0, 1]: support [0, 1], mean 0.5, standard deviation 0.1673 (there: 1/6).  r == 0 leaves x[i] as it is.
 *   KF_EVO_PSO     (CU_PSO_2D)   xf = f32(x[i]), gf = f32(head[i]);  t = social * r;  d = gf - xf;  x[i] = bf16(xf + t * d) -- every operation rounded on its own, no
 *                                fma.  The reference passes alpha to CU_PSO_2D and never reads it: alpha is ignored here.
 *   KF_EVO_PSO_GA  (+ CU_crossover_, the same pass)  the PSO value, then where b3 < thr the 16 bits of head[i] verbatim;  thr = clamp(floor(t_cross * 256 + 0.5), 0, 256),
 *                                computed on the host (t_cross = 0: exactly KF_EVO_PSO; t_cross = 1: x == head bit for bit).
 *   KF_EVO_MIX     (CU_mix_)     x[i] = bf16(alpha * xf + beta * gf),  beta = (float)(1.0 - (double)alpha): two rounded products, one add.  No draw.
 * Stores round to nearest even (the reference's (T) cast), not the optimiser's stochastic store.  The bits do not depend on the launch geometry.
 * Refusals are KF_INVALID_ARGS, launch nothing, and kf_last_error says which: a null pointer; x == head or overlapping ranges; ne0 or ne1 < 1, n < 8, n % 8 != 0 or
 * n >= 2^32; a pointer that is not 16-byte aligned; an unknown algorithm; social, alpha or t_cross not finite. */
enum kf_evo_algorithm { KF_EVO_PSO = 1, KF_EVO_MIX = 2, KF_EVO_PSO_GA = 4 };
int kf_evolve(kf_ctx* ctx, kf_bf16* x, const kf_bf16* head, int ne0, int ne1, int algorithm, float alpha, float social, float t_cross, uint32_t seed);
/* The ensemble mean of per-row losses (Fish::ForwardOnRLS, gLLM.cpp:722-787: tmpLoss[i] / curB), one member at a time -- the trainer's one losses buffer is
 * overwritten by the next member's forward:  index 0: acc[i] = losses[i];  0 < index: acc[i] = acc[i] + losses[i];  and at index == count - 1 also acc[i] = acc[i] / count.
 * fp32, in index order; acc and losses fp32 [n] on the device, acc != losses.  KF_INVALID_ARGS: a null pointer, acc == losses, n = 0 or n >= 2^31, count < 1, index
 * outside [0, count). */
int kf_loss_mean(kf_ctx* ctx, float* acc, const float* losses, size_t n, int index, int count);

/* ---- token batch (prompt prefill).  The reference feeds the prompt one token at a time through the decode path (Fish::Chat,
 * GoPT.cpp:1139-1146); its batched forward exists only on the training side (SelfAttention::cuFlow / ROPE::cuFlow,
 * NeuronFuse.cu:692-731, rope.cu).  These entries run the same per-token arithmetic for n_tok consecutive positions at once;
 * kf_linear / kf_rmsnorm / kf_swiglu already take row batches. */
/* n_w <= 3 matrices that share the input rows x [nTok, ne1] (Q, K, V): y[i] [nTok, w[i]->ne0].  One launch when a tile kernel
 * covers the shape, otherwise kf_linear per matrix.  Batches of >= 1024 rows (>= 320 with resident copies, kf_set_dequant_arena) of group-quantised matrices whose row counts are multiples of
 * 256 are dequantised back to back into the kf_set_scratch workspace (kf_linear_multi_scratch_bytes says how large; 0 = route not taken)
 * and multiplied by ONE launch of the 256 x 256 bf16 tile kernel -- the reference's own order (GetDataX, then the GEMM); its fp32 summation
 * order differs from the in-register-unpack kernels of smaller batches, as kf_linear's own large-batch path does. */
size_t kf_linear_multi_scratch_bytes(int n_w, const kf_weight* const* w, int nTok);
int kf_linear_multi(kf_ctx* ctx, int n_w, const kf_weight* const* w, const kf_bf16* x, kf_bf16* const* y, int nTok);
/* act [nTok, ne0] = silu(x . gate^T) * (x . up^T) for nTok rows (FFN::cuFlow: gate.Forw, up.Forw, Relu::Forw SWIG,
 * NeuronFuse.cu:615-656 with a batch): one launch, bit-identical to kf_linear x 2 + kf_swiglu; up_scratch [nTok, ne0] is used by
 * the unfused fallback and by the large-batch route (>= 1024 rows, >= 320 with resident copies: gate | up interleaved, SwiGLU in the tile GEMM's epilogue; or stacked as in kf_linear_multi, then kf_swiglu). */
int kf_gateup_swiglu_batch(kf_ctx* ctx, const kf_weight* gate, const kf_weight* up, const kf_bf16* x, kf_bf16* act, kf_bf16* up_scratch, int nTok);
/* out[t] = row d_tokens[t] of the table, t < n_tok (TokenEmbed::OnEmbed for a batch, NeuronFuse.cu:176-207) */
int kf_embed_batch(kf_ctx* ctx, const kf_weight* w, const int32_t* d_tokens, int n_tok, kf_bf16* out);
/* kf_qknorm_rope for tokens t < n_tok at positions pos0 + t: q + t*q_stride, k + t*k_stride (k may be cache rows: k_stride = kv_stride) */
int kf_qknorm_rope_batch(kf_ctx* ctx, kf_bf16* q, kf_bf16* k, const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rope_table, int pos0, int n_tok,
                         int64_t q_stride, int64_t k_stride, int n_head, int n_kv, int hd, float eps);
/* SelfAttention::cuFlow's projection step for a token batch in one call: Q | K | V of the same x (K / V rows may be the cache rows themselves, TGraph.cpp:198-207) followed by
 * ROPE::cuInfer on q and k (kf_qknorm_rope_batch).  For >= 1024 tokens (>= 320 with resident copies) and head_dim 128 both happen in ONE launch -- the stacked tile GEMM with the q/k-norm and the rotation in
 * its epilogue (a 128-row tile is one head) -- otherwise kf_linear_multi + kf_qknorm_rope_batch.  Same arithmetic either way (token batches: MFMA summation order, tolerances). */
int kf_qkv_rope_batch(kf_ctx* ctx, const kf_weight* wq, const kf_weight* wk, const kf_weight* wv, const kf_bf16* x, kf_bf16* q, kf_bf16* k, kf_bf16* v, int nTok,
                      const kf_bf16* wq_norm_or_null, const kf_bf16* wk_norm_or_null, const float* rope_table_or_null, int pos0, int n_head, int n_kv, int head_dim, float eps);
/* the same for nTok rows that are SEQUENCES of seq_len tokens back to back (a batch of prompts; a training batch): positions 0 .. seq_len - 1 in each (pos0 must be 0, nTok a
 * multiple of seq_len; seq_len 0 = kf_qkv_rope_batch).  Unfused route: kf_linear_multi + kf_qknorm_rope_train. */
int kf_qkv_rope_seqs(kf_ctx* ctx, const kf_weight* wq, const kf_weight* wk, const kf_weight* wv, const kf_bf16* x, kf_bf16* q, kf_bf16* k, kf_bf16* v, int nTok, int seq_len,
                     const kf_bf16* wq_norm_or_null, const kf_bf16* wk_norm_or_null, const float* rope_table_or_null, int pos0, int n_head, int n_kv, int head_dim, float eps);
/* causal attention of tokens t < n_tok (position pos0 + t attends to cache rows 0 .. pos0 + t, which must already hold the prepared
 * keys / values of the batch); q and out rows are q_stride elements apart; same arithmetic as kf_attn_decode, one workgroup per
 * (kv-head, token), no scratch. */
int kf_attn_prefill(kf_ctx* ctx, const kf_bf16* q, const kf_bf16* kcache, const kf_bf16* vcache, kf_bf16* out, int pos0, int n_tok, int64_t q_stride,
                    int n_head, int n_kv, int hd, int kv_stride);

/* ---- the decode step's layer loop as ONE persistent launch (kf_engine.hip).  Replaces, for all layers of one token, the neuron walk of
 * Fish::ForwardOnRLS (gLLM.cpp:755-771) over SelfAttention::cuInfer (QKV.cu:617-702) and FFN::cuInfer (NeuronFuse.cu:615-656): the same
 * arithmetic as kf_norm_linear -> kf_attn_block -> kf_linear -> kf_norm_gateup_swiglu -> kf_linear per layer (every output bit equal), with the
 * five launches per layer turned into phases of one resident kernel that hand their vectors over through tagged granules in `workspace`.
 * One workgroup per CU; the launch must have the GPU's CUs to itself (every poll is bounded: a launch that cannot become fully resident sets the
 * engine's error word instead of hanging; kf_engine_check reads it).  w[7] = q k v o gate up down; all layers the same shapes and storage.
 * kf_engine_step returns KF_ENGINE_NOT_SERVED (1) when the position bound needs an attention slicing the engine does not restate: the caller
 * then issues the per-layer calls.  x_in / x_out: plain bf16 [dim] (the embedding row in, the residual stream after the last layer out; they may
 * alias).  pos_bound bounds the position as in the other decode entries (graph replay); the position itself is d_state[1]. */
typedef struct kf_engine kf_engine;
typedef struct kf_engine_layer {
    kf_weight w[7];
    const kf_bf16 *norm_in, *norm_post, *q_norm, *k_norm; /* q_norm / k_norm may be NULL */
    kf_bf16 *kcache, *vcache;                            /* layer base; row t at t*kv_stride elements */
    const int32_t* hot_ffn; /* sparse forward (D_matmul_sparse, GST_float.cpp:306-318): CS_Picker's hot[ffn] on the DEVICE, 1 = the gate / up row is computed, anything else = 0
                               (SwiGLU(0, 0) = 0: that element of the FFN's hidden vector is zero); cold rows are never read.  NULL: dense.  Read once per launch. */
} kf_engine_layer;
typedef struct kf_engine_desc {
    int32_t n_layer, dim, n_head, n_kv, head_dim, ffn, kv_stride;
    int32_t max_seq; /* rows of every layer's K / V cache (> 0): a launch whose positions reach past it is refused (KF_INVALID_ARGS from the bound, error word bit 64 from the state) */
    float rms_eps, qk_eps;
    const float* rope_table;
    const kf_engine_layer* layers; /* HOST array [n_layer] of device pointers */
} kf_engine_desc;
#define KF_ENGINE_NOT_SERVED 1
size_t kf_engine_workspace_bytes(const kf_engine_desc* desc);
/* workspace: device memory, 256-byte aligned, kf_engine_workspace_bytes(desc) bytes, owned by the caller, initialised here.
 * KF_UNSUPPORTED_DATATYPE: shapes / storage outside what the engine serves (the per-layer calls remain). */
int kf_engine_create(kf_ctx* ctx, const kf_engine_desc* desc, void* workspace, size_t workspace_bytes, kf_engine** out);
int kf_engine_step(kf_ctx* ctx, kf_engine* e, const kf_bf16* x_in, kf_bf16* x_out, const int32_t* d_state, int pos_bound);
/* TokenEmbed::cuInfer inside the launch: with a bf16 embedding table set, kf_engine_step may be given x_in == NULL and reads the row of the state's token
 * (or of d_forced[pos] when that is >= 0, as kf_embed_state does) itself.  NULL table: back to x_in.  KF_UNSUPPORTED_DATATYPE for other storages. */
int kf_engine_set_embedding(kf_ctx* ctx, kf_engine* e, const kf_weight* embed_bf16_or_null, const int32_t* d_forced_or_null);
/* Head4Token::cuInfer_1 (NeuronFuse.cu:842-862) + sample_argmax (GoPT.cpp:602-612) as trailing phases of the same launch: with a bf16 head [vocab, dim] and
 * the final RMSNorm weight set, kf_engine_step_head runs the layers, the final norm, the LM-head mat-vec (logits [vocab] bf16, every bit equal to
 * kf_norm_lm_head's) and -- pick != 0 -- the greedy first-maximum pick with the decode-state update of kf_norm_lm_head (d_tokens_out[pos] = id,
 * d_state = {id, pos + 1}): one launch per token instead of three.  A launch whose error word is set never advances the state.  NULL head: removed.
 * KF_UNSUPPORTED_DATATYPE for other head storages (the caller keeps kf_norm_lm_head). */
int kf_engine_set_head(kf_ctx* ctx, kf_engine* e, const kf_weight* head_bf16_or_null, const kf_bf16* final_norm_w, kf_bf16* logits, int32_t* d_tokens_out_or_null);
int kf_engine_step_head(kf_ctx* ctx, kf_engine* e, const kf_bf16* x_in, kf_bf16* x_out, int32_t* d_state, int pos_bound, int pick);
/* The int8 screen of the in-launch head.  In a kf_engine_steps_head launch only the LAST step's logits can be observed; on the steps before it the pick alone matters.  With a
 * screen set those steps stream an int8 copy of the head (one scale per row, half the bytes), bound every row's logit by a rigorous per-row error bound, and re-compute from
 * the bf16 head -- by the arithmetic of the full stream -- only the rows that can still be the first maximum: the picked ids are bit for bit what they are without a screen,
 * those steps write no logits, and the last step of every launch (every single-step call) runs the full head unchanged.  buf: device memory, 256-byte aligned,
 * kf_engine_head_screen_bytes(vocab, dim) bytes, owned by the caller, filled here (one launch on the context's stream) from the head that is set; it must stay valid, and the
 * head's data unchanged, until the screen is switched off (buf == NULL), the head is set again (which drops the screen) or the engine is destroyed. */
size_t kf_engine_head_screen_bytes(int vocab, int dim);
int kf_engine_set_head_screen(kf_ctx* ctx, kf_engine* e, void* buf, size_t bytes);
typedef struct kf_engine_screen_statistics { /* since creation / kf_engine_reset */
    int64_t screened_steps; /* decode steps whose head phase streamed the screen */
    int64_t rows_reranked;  /* rows re-computed from the bf16 head on those steps, all workgroups */
    int64_t wg_fallbacks;   /* workgroup-steps whose candidate list overflowed: that workgroup streamed its bf16 rows instead */
} kf_engine_screen_statistics;
int kf_engine_screen_stats(kf_ctx* ctx, kf_engine* e, kf_engine_screen_statistics* out);
/* n_steps consecutive greedy decode steps in ONE launch (Fish::ForwardOnRLS + Head4Token::cuInfer_1 + sample_argmax, n_steps times: GoPT.cpp:1155-1180): the step of
 * kf_engine_step_head(x_in = NULL, pick = 1) repeated inside the kernel -- the id a step picks reaches the next step's embedding read as a tagged granule instead of
 * through a launch boundary (~8 us per step).  Every position d_state[1] .. d_state[1] + n_steps - 1 must lie under pos_bound (the bound fixes the attention slicing of
 * the launch); d_tokens_out, d_forced and d_state are read and written per step as by the single step; logits / x_out hold the last step's.  Same bits as n_steps launches. */
int kf_engine_steps_head(kf_ctx* ctx, kf_engine* e, kf_bf16* x_out, int32_t* d_state, int pos_bound, int n_steps);
/* Why a model is (not) served: KF_OK, or KF_ENGINE_NOT_SERVED with the reason in `why` (shape not instantiated, storage, device too small, ...): validation only, nothing is
 * allocated (desc->layers as for kf_engine_create).  Fish::EnsureEngine logs it once. */
int kf_engine_served(kf_ctx* ctx, const kf_engine_desc* desc, char* why, size_t why_bytes);
/* First-sweep delays of the hand-offs, measured on THIS device.  A consumer's first sweep of a hand-off vector is issued a fixed delay behind the moment its own workgroup
 * published its rows of the feeding phase; too early costs a second sweep, too late its lateness.  kf_engine_tune times the layers-only launch at the position d_state holds
 * (reads the state's token, rewrites that position's K / V rows with the values the real step is about to write; the state does not advance) and walks the six delays by
 * coordinate descent (`passes` <= 3 rounds of 8, 4, 2 sleep units; ~100 launches per round), for the attention slice count of `pos_bound`.  Results never depend on the
 * delays.  Needs the embedding table (kf_engine_set_embedding).  us_before / us_after (optional): mean launch time with the old and the chosen delays. */
int kf_engine_tune(kf_ctx* ctx, kf_engine* e, kf_bf16* x_out, const int32_t* d_state, int pos_bound, int passes, float* us_before, float* us_after);
typedef struct kf_engine_statistics {
    int32_t sweeps[6]; /* sweeps the poller of workgroup 0 issued since creation / reset, per hand-off: x (P1), q|k|v (P2), slice partials (P3), ao (P4), xB (P5), act (P6) */
    int32_t polls;     /* polls per hand-off in the same span (= layers stepped): sweeps[i] / polls = sweeps per poll, 1.0 when every first sweep came back complete */
    int32_t delay[6];  /* the delays in use at pos_bound's slice count (s_sleep units) */
    int32_t tuned;     /* 1: measured by kf_engine_tune on this device, 0: the built-in defaults */
} kf_engine_statistics;
int kf_engine_stats(kf_ctx* ctx, kf_engine* e, int pos_bound, kf_engine_statistics* out);
int kf_engine_check(kf_ctx* ctx, kf_engine* e); /* synchronises; KF_INTERNAL_ERR when a hand-off poll has timed out since creation or the last kf_engine_reset, or (error word bit 128, canonical order) an attention score left the engine's fixed-exponent range: |round(s log2 e)| > 448 -- the per-layer launches serve such a model */
/* After KF_INTERNAL_ERR from kf_engine_check: the error word latches and every later launch of the engine returns at once without output.  kf_engine_reset
 * synchronises, puts the hand-off state back to its initial one and clears the word; the steps since the failure have to be redone. */
int kf_engine_reset(kf_ctx* ctx, kf_engine* e);
int kf_engine_destroy(kf_engine* e);

/* ---- EIGHT decoders per GPU, one per XCD, for up to 32 independent sequences (kf_xengine.hip; rounds 5 - 6).  The reference decodes ONE sequence per process (Fish::Chat, GoPT.cpp:1139-1180) and
 * scales a small model by running more processes; on this part a single sequence cannot keep the HBM busy (its step is a chain of hand-offs), so the replicas move
 * INSIDE the package: the 32 workgroups of XCD s are the decoder of sequence s, every hand-off stays in that XCD's L2, and the chip streams eight sequences' bytes at
 * once.  The sequences share the weights (the kf_engine_desc's layer table, the embedding, the head) and nothing else; per sequence: a K/V cache (sequence s at
 * layers[].kcache + s * kv_seq_stride elements), a decode state {token, pos, -, -} (d_state + 4 s), forced ids (d_forced + s * forced_stride), ids out, logits
 * (logits + s * vocab), the residual stream out (x_out + s * dim).  Each sequence's ids, logits and K/V rows are bit for bit those kf_engine_steps_head, the per-layer
 * calls and the oracle give for that sequence alone (canonical order only: kf_set_canonical(ctx, 0) is refused).  One workgroup per CU, 32 per XCD: the launch must have
 * the GPU to itself (bounded polls, error word, kf_xengine_check / _reset as for kf_engine).  Sequences may stand at different positions.
 * n_seq <= 8: sequence s on XCD s, one workgroup per CU.  More (round 6): still ONE decoder per XCD, each decoding 2 (n_seq <= 16) or 4 (n_seq <= 32) sequences -- XCD x takes
 * sequences x, x + 8, x + 16, x + 24.  Every 4-bit block a decoder streams is unpacked ONCE (the exact bf16-stepwise dequantisation, T.cu:274, is what bounds these engines) and
 * multiplied against the activations of all its sequences; each sequence keeps its own canonical chains, attention, K / V cache and state, so its bits do not change.
 * Served: 4-bit PackedQ (RTN, groups of 128) layers of the Qwen3-0.6B, 1.7B, 4B and 8B shapes (and two small test shapes), bf16 embedding / head; more than 8
 * sequences for the 0.6B / 1.7B shapes (1.7B: at most 16), more than 16 for the 0.6B shape.  Round 6: 1-bit and 2-bit PackedQ (YinYang) layers for the 0.6B shape and the 256-wide
 * test shape (1-bit: BASELINE config 5's storage), and FFNs with a hot-row mask (kf_engine_layer::hot_ffn: a cold gate / up row publishes a zero, D_matmul_sparse).  Weights are read in place and must not
 * change while an engine built on them lives; for the GQA-4 shapes (and the TP form below) the engine keeps a fused COPY of every layer's q | k | v rows in its workspace, made at
 * create time: after a weight update destroy the engine and create it again.
 * d_state [n_seq][4] = {token, pos, parked, status}.  parked != 0: the launch skips the sequence (the other sequences of its decoder go on).  A launch one of whose positions
 * would lie beyond a sequence's cache rows (pos + n_steps > max_seq) skips THAT sequence and sets bit 64 of its status word -- the others decode on; nothing is shared but
 * the weights, so one finished sequence never stops the rest (the caller clears the word when it re-aims the sequence). */
typedef struct kf_xengine kf_xengine;
#define KF_XENGINE_MAX_SEQ 32
size_t kf_xengine_workspace_bytes(const kf_engine_desc* desc);
int kf_xengine_create(kf_ctx* ctx, const kf_engine_desc* desc, int n_seq, int64_t kv_seq_stride, void* workspace, size_t workspace_bytes, kf_xengine** out);
int kf_xengine_served(kf_ctx* ctx, const kf_engine_desc* desc, char* why, size_t why_bytes); /* KF_OK or KF_ENGINE_NOT_SERVED + the reason */
/* TokenEmbed::cuInfer inside the launch (bf16 table, required); d_forced [n_seq][forced_stride] or NULL */
int kf_xengine_set_embedding(kf_ctx* ctx, kf_xengine* e, const kf_weight* embed_bf16, const int32_t* d_forced_or_null, int forced_stride);
/* Head4Token::cuInfer_1 + sample_argmax inside the launch: logits [n_seq][vocab] bf16, d_tokens_out [n_seq][tokens_stride] or NULL */
int kf_xengine_set_head(kf_ctx* ctx, kf_xengine* e, const kf_weight* head_bf16_or_null, const kf_bf16* final_norm_w, kf_bf16* logits, int32_t* d_tokens_out_or_null, int tokens_stride);
/* n_steps greedy decode steps of EVERY sequence in one launch (Fish::ForwardOnRLS + Head4Token::cuInfer_1 + sample_argmax per sequence and step): d_state [n_seq][4] is
 * read and advanced per step, x_out [n_seq][dim] holds the last step's residual stream.  pick = 0 (n_steps = 1 only): logits without the pick, the state stays. */
int kf_xengine_steps(kf_ctx* ctx, kf_xengine* e, kf_bf16* x_out, int32_t* d_state, int n_steps, int pick); /* (launched directly: refused inside kf_graph_begin / _end) */
int kf_xengine_check(kf_ctx* ctx, kf_xengine* e); /* synchronises; KF_INTERNAL_ERR when a hand-off poll has timed out since creation or the last kf_xengine_reset */
int kf_xengine_reset(kf_ctx* ctx, kf_xengine* e);
int kf_xengine_destroy(kf_xengine* e);
/* Tensor parallel over the XCDs (round 5): ONE sequence of a model whose TP = 8 ranks (koifish_amd/tp.py TPPlan; the partitioning of SURVEY 8e) run as the eight XCDs of one
 * launch -- rank r's 32 workgroups stream rank r's shards; q | k | v, the attention of the rank's kv-head and gate | up stay inside the XCD; the column shards (o_proj, down_proj)
 * leave as fp32 partials into every rank's receive area (the {value | generation} protocol of kf_tp_*, inside the launch), summed in rank order: the bits of kf_tp_reduce_recv.
 * Served: the ranks of Qwen3-32B (per rank: dim 5120, 8 / 1 heads of 128, ffn 3200), 4-bit PackedQ layers, bf16 embedding (replicated) and head (vocabulary shards).
 * rank_descs[r]: rank r's layers (its shards, its kv-head's cache rows: kv_stride = 128).  kf_xengine_set_embedding / _steps / _check / _reset / _destroy as above with
 * n_seq = 1 (d_state [4], x_out [dim]); logits: the FULL vector, the shards' rows in rank order.  No reference counterpart (QKV.cu:503 is single-GPU). */
size_t kf_xengine_workspace_bytes_tp(const kf_engine_desc* rank0_desc);
int kf_xengine_create_tp(kf_ctx* ctx, const kf_engine_desc* const* rank_descs, int world, void* workspace, size_t workspace_bytes, kf_xengine** out);
int kf_xengine_set_head_tp(kf_ctx* ctx, kf_xengine* e, const kf_weight* const* head_shards, const int32_t* row0, const kf_bf16* final_norm_w, kf_bf16* logits, int32_t* d_tokens_out_or_null, int tokens_stride);

/* ---- int8 activations for 1-bit and ternary layers: W1.58 . A8 as the reference runs its BitNet family (Bitnet::Bitnet sets DEBUG.tpActi = I8, QWen.cpp:146-153;
 * SelfAttention::cuInfer calls inpQ->Quant4A(DEBUG.tpActi) in front of Q / K / V, QKV.cu:647; huTensor::Quant4A -> CU_X2A8_, T.cu:24-102).  Off unless called.
 * THE DEFINITION (DESIGN.md "Int8 activations"; restated in numpy by tests/test_a8_cpu.py and tests/test_gpu_a8.py):
 *   quantiser, per token row x[dim] (bf16 read as fp32; with norm_w first normed and rounded to bf16 exactly as kf_rmsnorm stores it):
 *     amax = max_i |x_i|;  step_x = amax / 127.0f  (correctly rounded fp32 division);
 *     q_i = clamp(round_half_away(x_i / step_x), -127, 127)  (correctly rounded fp32 division, std::round as T.cu:60);  amax == 0: step_x = 0 and every q_i = 0.
 *     DEVIATION from CU_X2A8_: it takes the SIGNED row maximum (step = wMax / qMax, T.cu:41-43) and asserts step > 0 -- a row whose largest element is negative trips
 *     the assert, a row with |min| > max clips.  Here: the absolute maximum, as BitNet b1.58 defines it.
 *   product, per output row r and token t, groups g of 128 consecutive weights:
 *     I_g = sum_{c in g} (code[c] - qBias) * q[t][c]  as int32 (ternary KF_T_SIGN: {-1, 0, 1}; KF_BOOL1 / KF_T_BINARY: {0, 1}); |I_g| <= 128 * 127 = 16256;
 *     acc = 0;  acc = acc + fp32(step_w[g]) * fp32(I_g)  for g = 0, 1, .. K/128 - 1: ONE ascending fp32 chain; every product is exact (8 + 14 significant bits).
 *     The order depends on K and g only -- never on lanes per row, grid, plan form or nTok;
 *     y = bf16_rn(step_x[t] * acc);  with bias: bf16_rn(step_x[t] * acc + bias[r]);  with residual: y = bf16(residual + bf16(..)), kf_linear's epilogue.
 *   The group ZERO is not part of this arithmetic: YinYang and the symmetric quantiser write zero = 0 (GeQuant.cpp:536-628); callers check it (Fish, at switch-on).
 * kf_act_quant_i8: x rows of dim bf16, ldx elements apart (ldx >= dim) -> q int8 [rows][dim], step fp32 [rows].
 * kf_linear_a8: y [nTok][ne0] as kf_linear writes it; residual [nTok][ne0] may alias y.  Refusals (kf::a8_plan, csrc/kf_a8.h): any storage other than KF_T_SIGN /
 * KF_BOOL1 / KF_T_BINARY in KF_QUANT_GROUP form KF_UNSUPPORTED_DATATYPE; lGroup != 128 or no gama KF_QUANT_ERR; ne1 % 128 != 0, ne0 < 1, nTok < 1 KF_INVALID_ARGS; data not
 * 16-byte aligned KF_BLAS_UNALIGN.  nTok > 1 runs the same kernel on tiles of token rows: the bits of nTok = 1.
 * With norm_w the prologue refuses what kf_rmsnorm refuses (an odd dim: KF_RMS_PARAMS).
 * kf_linear_a8_status: what kf_linear_a8 would answer for this weight and nTok -- KF_OK or the refusal -- without a launch: THE served-storage rule for callers that route
 * matrices (Fish asks it per layer matrix: KF_UNSUPPORTED_DATATYPE = "keep the bf16-activation route"). */
int kf_linear_a8_status(const kf_weight* w, int nTok);
int kf_act_quant_i8(kf_ctx* ctx, const kf_bf16* x, int64_t ldx, const kf_bf16* norm_w_or_null, float eps, int rows, int dim, int8_t* q, float* step);
int kf_linear_a8(kf_ctx* ctx, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias_or_null, const kf_bf16* residual_or_null, int nTok);
/* kf_linear_a8_tiles: kf_linear_a8's contract and kf_linear_a8's bits on the int8 MFMA (v_mfma_i32_16x16x64_i8), for token batches: q int8 [nTok][ne1] and step fp32
 * [nTok] as kf_act_quant_i8 writes them, y bf16 [nTok][ne0], y = bf16(step_x * acc [+ bias]) then bf16(residual + bf16(y)); residual [nTok][ne0] may alias y (every
 * output element is read and written by one lane).  Any nTok >= 1 is served; token and row tails are masked.  Per 128-weight group an int32 accumulator starts from
 * zero and takes exactly that group (two MFMA steps); the lane that holds an output element folds I_g into its fp32 chain in ascending g: the definition above, so the
 * result equals kf_linear_a8's bit for bit whatever the tile, the grid or nTok.  The launch is the tile route of kf::a8_plan (csrc/kf_a8.h); its refusals are
 * the mat-vec route's, the ones listed above.
 * kf_linear_a8_tiles_status: what kf_linear_a8_tiles would answer for this weight and nTok, without a launch.
 * KF_A8_TILE_MIN: the token count from which callers that route (Fish::A8Group) send a batch to the tiles by default; below it, and for nTok = 1 always, kf_linear_a8. */
enum { KF_A8_TILE_MIN = 32 };
int kf_linear_a8_tiles_status(const kf_weight* w, int nTok);
int kf_linear_a8_tiles(kf_ctx* ctx, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias_or_null, const kf_bf16* residual_or_null, int nTok);

/* ---- int8 activations for 4-bit layers: W4 . A8, the integer form of KF_Q4 group storage.  Off unless called; the entries above keep refusing KF_Q4.
 * THE DEFINITION (restated in numpy by tests/w4a8_restate.py):
 *   activations: kf_act_quant_i8 above, unchanged -- q int8 [nTok][K], step_x fp32 [nTok].
 *   product, per output row r and token t, groups g of 128 consecutive weights; code = the 4-bit value of the Packed128 stream (0 .. 15), qBias (0 or 8), ZERO[g], STEP[g]
 *   from the blob (gama_T):
 *     I_g = sum_{c in g} (code[c] - qBias) * q[t][c]  as int32;  |I_g| <= 128 * 15 * 127 = 243 840 < 2^24, so fp32(I_g) is exact;
 *     S_g = sum_{c in g} q[t][c]                      as int32;  |S_g| <= 16 256;
 *     p = fp32(STEP[g]) * fp32(I_g)   ONE IEEE fp32 multiply, one rounding: unlike the ternary case the product (8 + 18 significant bits) is NOT exact;
 *     z = fp32(ZERO[g]) * fp32(S_g)   exact (8 + 14 significant bits);
 *     c = p - z                       one fp32 subtract;
 *     acc = 0;  acc = acc + c         for g = 0, 1, .. K/128 - 1: ONE ascending fp32 chain, one add per group.
 *     The multiply, the subtract and the add are three separate roundings: no fused multiply-add stands in for any pair of them.  The order depends on K and g only --
 *     never on lanes per row, tile, grid, chunk or nTok;
 *     y = bf16_rn(step_x[t] * acc);  with bias: bf16_rn(step_x[t] * acc + bias[r]);  with residual: y = bf16(residual + bf16(..)), exactly as kf_linear_a8 writes it.
 *   DEVIATIONS: (1) the weight is the affine STEP * (code - qBias) - ZERO WITHOUT the per-weight bf16 roundings of CU_Q128toX_ (bf16(bf16(step * (q - qBias)) - zero),
 *   T.cu:274): the result differs from the bf16-activation route by more than the activation quantisation.  (2) the activation quantiser's deviation is the one stated
 *   above (the absolute row maximum).
 * kf_linear_w4a8: the mat-vec on v_dot4c_i32_i8; y [nTok][ne0], residual [nTok][ne0] may alias y.  Refusals (kf::a8_plan, csrc/kf_a8.h), in kf_linear_a8's order and
 * with its codes: any storage other than KF_Q4 in KF_QUANT_GROUP form (AutoAWQ included) KF_UNSUPPORTED_DATATYPE; lGroup != 128, no gama, or a qBias other than 0 / 8
 * KF_QUANT_ERR; ne1 % 128 != 0, ne0 < 1, nTok < 1 KF_INVALID_ARGS; data not 16-byte aligned KF_BLAS_UNALIGN.
 * kf_linear_w4a8_tiles: the same contract and the same bits on v_mfma_i32_16x16x64_i8, for token batches (any nTok >= 1 is served; token and row tails masked); the launch
 * is the tile route of kf::a8_plan, its refusals are the mat-vec route's.  q need not be 16-byte aligned.
 * kf_linear_w4a8_status / kf_linear_w4a8_tiles_status: what the entry would answer for this weight and nTok, without a launch: the served-storage rule for callers that
 * route (Fish asks it per layer matrix while kfh_set_act_int8_q4 is on).  KF_A8_TILE_MIN is the default threshold of this family too. */
int kf_linear_w4a8_status(const kf_weight* w, int nTok);
int kf_linear_w4a8(kf_ctx* ctx, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias_or_null, const kf_bf16* residual_or_null, int nTok);
int kf_linear_w4a8_tiles_status(const kf_weight* w, int nTok);
int kf_linear_w4a8_tiles(kf_ctx* ctx, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias_or_null, const kf_bf16* residual_or_null, int nTok);

/* ---- int8 KV cache: quantised K / V rows and a decode attention whose scores are exact integer dots (the reference's switch DEBUG.T_kvcache_quant, QKV.cu:664, has a
 * stub behind it).  Off unless called; the bf16 entries above are untouched.
 * THE DEFINITION (restated in numpy by tests/kv8_restate.py):
 *   storage, per layer: K8, V8 int8 [n_ctx][kv_stride] (kv_stride >= n_kv * hd bytes, a multiple of 16); KS, VS fp32 [n_ctx][n_kv]: one step per row and kv-head.  The
 *     caller zero-fills all four at allocation: rows past the position are then finite, which is what the d_pos contract (kf_attn_block) asks of the bf16 cache too.
 *   row quantiser, per token and kv-head over its hd elements: kf_act_quant_i8's arithmetic, unchanged -- amax = max_i |x_i|; step = amax / 127.0f (correctly rounded fp32
 *     division); q_i = clamp(round_half_away(x_i / step), -127, 127); amax == 0: step = 0 and every q_i = 0.  K rows are quantised after q/k-norm + RoPE and their rounding
 *     to bf16; V rows as the projection stores them (bf16).
 *   decode attention, for query head h of kv-head kvh at position pos, keys t = 0 .. pos:
 *     query    (q8, sq) = the row quantiser on the normed, roped bf16 query head;
 *     integer  I_t = sum_i q8_i * k8[t][i] as int32;  |I_t| <= 128 * 127^2 < 2^24, so fp32(I_t) is exact;
 *     score    c = sq * KS[t][kvh];  d = fp32(I_t) * c;  s_t = bf16_rn(d * rden), rden = 1.0f / sqrtf(hd) as the bf16 kernel's score multiplies by it: THREE separate fp32
 *              multiplies, none fused with another;
 *     weight   (f_t, n_t) = kf_exp2_parts(s_t * log2 e), p_t = f_t * 2^(n_t - m), m ANY integer >= every n it meets -- the canonical order of kf_attn_block;
 *     value    g_t = f_t * VS[t][kvh]: ONE fp32 multiply, taken before the power-of-two scaling, so that it does not depend on m;
 *     sums     fp64: L = sum_t p_t;  O[d] = sum_t ldexp((double)g_t * (double)v8[t][d], n_t - m): every term is exact (24 + 7 significant bits);
 *     out      bf16_rn((float)(O[d] / L)).
 *     The new row is quantised FIRST and attended in its quantised form like every other key.  There is ONE arithmetic: kf_set_canonical 0 and 1 give the same bits.
 *   dequantised row (token batches): bf16_rn(fp32(q8) * step): one fp32 multiply, one rounding.
 * kf_attn_block_kv8: kf_attn_block's contract on this cache in one launch -- q/k-norm + RoPE of the raw q [n_head * hd] and raw new key [n_kv * hd], the new K row and the
 * raw new V row [n_kv * hd] quantised and written with their steps at the position, then the attention over keys 0 .. position; pos is the launch bound, d_pos (or NULL)
 * the device word that holds the position (<= pos); scratch: kf_attn_scratch_bytes(), zero-filled once, shared with kf_attn_block (the counters return to zero).  The
 * launch is the ATTN_DECODE_KV8 entry of kf::attn_plan (csrc/kf_attn_plan.h).  Refusals: a null pointer KF_INVALID_ARGS; query heads per kv-head other than 1, 2, 4, 8 or
 * hd other than 64, 128 KF_INVALID_ARGS; K8 / V8 not 16-byte aligned or kv_stride % 16 != 0 KF_BLAS_UNALIGN.
 * kf_attn_block_kv8_status: what the entry would answer for a shape, without a launch.
 * kf_kv8_quant_rows: n bf16 K rows and n bf16 V rows [n_kv * hd], ld elements apart -> rows pos0 .. pos0 + n - 1 of K8 / V8 / KS / VS.
 * kf_kv8_dequant_rows: rows 0 .. n - 1 of K8 / V8 -> bf16 kout / vout [n][n_kv * hd], ld_out elements apart. */
int kf_attn_block_kv8_status(int n_head, int n_kv, int hd);
int kf_attn_block_kv8(kf_ctx* ctx, const kf_bf16* q_raw, const kf_bf16* k_raw, const kf_bf16* v_raw, int8_t* k8, int8_t* v8, float* ks, float* vs, kf_bf16* out,
                      const kf_bf16* wq_norm_or_null, const kf_bf16* wk_norm_or_null, const float* rope_table, int pos, const int32_t* d_pos_or_null, int n_head, int n_kv,
                      int hd, int kv_stride, float eps, void* scratch);
int kf_kv8_quant_rows(kf_ctx* ctx, const kf_bf16* k, const kf_bf16* v, int64_t ld, int n, int n_kv, int hd, int8_t* k8, int8_t* v8, float* ks, float* vs, int pos0,
                      int kv_stride);
int kf_kv8_dequant_rows(kf_ctx* ctx, const int8_t* k8, const int8_t* v8, const float* ks, const float* vs, int n, int n_kv, int hd, int kv_stride, kf_bf16* kout,
                        kf_bf16* vout, int64_t ld_out);
/* ---- int8 KV cache, the prompt form: attention of a token batch on the int8 rows themselves (restated in numpy by tests/kv8_prefill_restate.py).
 * THE DEFINITION, for row r of the batch at position p = pos0 + r, query head h of kv-head kvh, keys t = 0 .. p.  Up to the weight it IS the decode definition above, bit
 * for bit: (q8, sq) the row quantiser on the prepared bf16 query head; I_t the exact int32 dot (here on v_mfma_i32_16x16x64_i8); c = sq * KS[t][kvh], d = fp32(I_t) * c,
 * s_t = bf16_rn(d * rden): three separate fp32 multiplies; (f_t, n_t) = kf_exp2_parts(s_t * log2 e); p_t = f_t * 2^(n_t - m), m any integer >= every n met so far (moving
 * m multiplies by a power of two: exact); g_t = f_t * VS[t][kvh], one fp32 multiply.  So a prompt row's scores and weights are the ones kf_attn_block_kv8 computes there.
 *   The tail is this form's own:
 *     operand  gb_t = bf16_rn(g_t); the P.V product runs on bf16 MFMA, its V operand is bf16(v8[t][d]) (exact);
 *     sums     fp32: O[d] = sum_t (gb_t * 2^(n_t - m)) * v8[t][d], L = sum_t p_t.  Every product is exact (8 + 7 significant bits); the additions round, and their order
 *              inside an MFMA accumulator is the hardware's, not ours to state.  (A product scaled below the fp32 normal range, n_t - m < about -120, may be flushed: it is
 *              below 2^-120 of the largest weight.)
 *     out      bf16_rn(fl32(O[d] / L)): ONE correctly rounded fp32 division per element (not a reciprocal and a multiply), then the bf16 store.
 *   Hence the tail is held to a DERIVED bound, not to bit equality.  With N = p + 1 keys, unit roundoff u = 2^-23 (which covers an accumulator that truncates as well as
 *   one that rounds to nearest), A[d] = sum_t |gb_t * v8[t][d]| * 2^(n_t - M) and O, L the exact sums against one M: any-order fp32 summation gives |O~ - O| <= N u A and
 *   |L~ - L| <= N u L to first order, so |out - O / L| <= 2^-8 |O / L| (the bf16 store) + 2^-24 |O / L| (the division) + 2 N u (A + |O|) / L.  With ONE key nothing is
 *   summed and out is exact: bf16_rn(fl32(gb_0 * v8[0][d] / f_0)).
 *   EXACT, whatever the launch: a row's output bits depend only on its position, its q row and the cache -- not on pos0, n_tok, the rows beside it or the grid.  (Key tiles
 *   are anchored at key 0, a key's place in the walk is a function of its index, a column's m after a tile is the largest n among its keys so far; there is no split
 *   over keys and no merge.)  There is ONE arithmetic: kf_set_canonical 0 and 1 give the same bits.
 *   Against the decode form at the same position the result differs by the gb rounding (<= 2^-8 A / L) and the fp32 sums; the two are NOT bit-equal.
 * kf_attn_prefill_kv8: kf_attn_prefill's contract on the int8 cache -- q the prepared bf16 queries [n_tok][q_stride] as kf_qkv_rope_batch leaves them, rows
 * pos0 .. pos0 + n_tok - 1 of K8 / V8 / KS / VS already written by kf_kv8_quant_rows; out [n_tok][q_stride].  No scratch.  The launch is the ATTN_PROMPT_KV8 entry of
 * kf::attn_plan: one form for any n_tok >= 1 and pos0 >= 0.  Refusals, as kf_attn_block_kv8: a null pointer KF_INVALID_ARGS; query heads per kv-head other than 1, 2, 4, 8,
 * hd other than 64, 128, pos0 < 0, n_tok < 1, or a row stride shorter than the row KF_INVALID_ARGS; K8 / V8 or q not 16-byte aligned, out not 8-byte aligned,
 * kv_stride % 16 != 0 or q_stride % 8 != 0 KF_BLAS_UNALIGN.
 * kf_attn_prefill_kv8_status: what the entry would answer for a shape and n_tok, without a launch. */
int kf_attn_prefill_kv8_status(int n_head, int n_kv, int hd, int n_tok);
int kf_attn_prefill_kv8(kf_ctx* ctx, const kf_bf16* q, const int8_t* k8, const int8_t* v8, const float* ks, const float* vs, kf_bf16* out, int pos0, int n_tok,
                        int64_t q_stride, int n_head, int n_kv, int hd, int kv_stride);

#ifdef __cplusplus
}
#endif
#endif
