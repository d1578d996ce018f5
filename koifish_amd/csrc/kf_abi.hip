// kf_abi.hip -- extern "C" boundary of libkf_hip.so (include/kf_abi.h).  Argument checks, stream plumbing and
// hipGraph capture live here; the kernels are in kf_gemv.hip / kf_attn.hip / kf_ops.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>


#include <atomic>
#include <mutex>
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "kf_a8.h"
#include "kf_attn_plan.h"
#include "kf_attn_docs_plan.h"
#include "kf_gemm_plan.h"
#include "kf_gemv_plan.h"
#include "kf_gemv_rows_plan.h"
#include "kf_score_plan.h"
#include "kf_gama_plan.h"
#include "kf_lora_plan.h"
#include "kf_gradnorm_plan.h"
#include "kf_rowq.h"
#include "kf_engine_host.h"

struct kf_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    bool capturing;
    float* amax_val; /* per-workgroup partial maxima for kf_lm_head when the caller passes no scratch */
    int* amax_idx;
    double* muon_part; /* per-workgroup partial sums of squares of kf_muon_momentum / kf_muon_apply (those entries take no scratch) */
    int canonical;    /* 1: the decode kernels sum in the canonical order of oracle/kf_oracle.c sections 4c / 6 (bit-exact against the oracle; the default); 0: v_dot2c / fp32 forms */
    int row_unpack;   /* kf_set_row_unpack: 1: the 3- / 2-bit row forms unpack in registers where their 4-bit stand-in (kf_rowq.h) is served; 0 (the default): dequant + bf16 product */
    long long rows_shared, rows_single; /* activation rows the kf_*_rows entries served with the shared unpack / with one-token launches (kf_rows_route_counts) */
    void* scratch;    /* caller-owned workspace of kf_linear (kf_set_scratch): AWQ slice partials, or a weight dequantised to bf16 */
    size_t scratch_bytes;
    // resident GetDataX copies for token batches (kf_set_dequant_arena): caller-owned memory, filled on first use, keyed by the data pointers of the matrices a route
    // multiplies in one launch and the form they are laid out in (DEQ_STACK: back to back; DEQ_ILV: gate | up interleaved in blocks of 16 rows)
    struct DeqCopy {
        const void* key[3];
        int form;
        size_t off;
    };
    void* arena;
    size_t arena_bytes, arena_used;
    std::vector<DeqCopy> copies;
    // the tables kf_grad_norms_plan has written, by the address of the scratch that holds them: kf_grad_norms launches what is remembered here and nothing else
    struct GradNormSlot {
        const void* scratch;
        kf::GradNormPlan plan;
    };
    std::vector<GradNormSlot> gn_plans;
};
struct kf_graph {
    hipGraph_t graph;
    hipGraphExec_t exec;
};

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(KF_HIP_CHECK, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define CHKCTX(c) \
    if (!(c)) return fail(KF_INVALID_ARGS, "%s: null kf_ctx", __func__)
#define RET(code) \
    do {          \
        int c_ = (code); \
        if (c_ != KF_OK) return fail(c_, "%s failed with %d", __func__, c_); \
        return KF_OK;    \
    } while (0)

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" {

const char* kf_last_error(void) { return g_err; }
const char* kf_version(void) { return "koifish_amd 0.1 (gfx950)"; }

int kf_init(int device, void* stream, kf_ctx** out) {
    if (!out) return fail(KF_INVALID_ARGS, "kf_init: out is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(KF_HIP_CHECK, "kf_init: no HIP device (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(KF_INVALID_ARGS, "kf_init: device %d of %d", device, n);
    HIPCHK(hipSetDevice(device));
    kf_ctx* c = new kf_ctx();
    c->device = device;
    c->capturing = false;
    if (stream) {
        c->stream = (hipStream_t)stream, c->own_stream = false;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    HIPCHK(hipMalloc(&c->amax_val, sizeof(float) * kf::KF_MAX_ARGMAX_PARTIALS));
    HIPCHK(hipMalloc(&c->amax_idx, sizeof(int) * kf::KF_MAX_ARGMAX_PARTIALS));
    HIPCHK(hipMalloc(&c->muon_part, sizeof(double) * kf::KF_MUON_MAX_PARTIALS));
    c->scratch = nullptr, c->scratch_bytes = 0;
    c->arena = nullptr, c->arena_bytes = c->arena_used = 0;
    c->canonical = 1;
    c->row_unpack = 0;
    *out = c;
    return KF_OK;
}
static size_t up256z(size_t v) { return (v + 255) & ~(size_t)255; }
// the resident copy of n_w matrices in `form` (kf_set_dequant_arena), or NULL: a lookup, nothing is launched or filled
static const uint16_t* arena_find(const kf_ctx* c, int n_w, const kf_weight* const* w, int form) {
    if (!c->arena) return nullptr;
    for (const kf_ctx::DeqCopy& e : c->copies) {
        bool same = e.form == form;
        for (int i = 0; i < 3; i++) same = same && e.key[i] == (i < n_w ? w[i]->data : nullptr);
        if (same) return (const uint16_t*)((const char*)c->arena + e.off);
    }
    return nullptr;
}
// The bf16 copies of a plan (p.deq, p.deq_form): resident in the arena, dequantised into it and kept, or dequantised into the scratch for this call.  KF_OK: *out holds
// them; < 0 error.
static int deq_copies(kf_ctx* c, const kf::GemmPlan& p, int n_w, const kf_weight* const* w, const uint16_t** out) {
    if (p.deq == kf::DQ_RESIDENT) {
        *out = arena_find(c, n_w, w, p.deq_form);
        return KF_OK;
    }
    char* dst = p.deq == kf::DQ_ARENA ? (char*)c->arena + c->arena_used : (char*)c->scratch;
    size_t off = 0;
    for (int i = 0; i < n_w; i++) {
        const int r = p.deq_form == kf::DEQ_ILV ? kf::dequant_launch(c->stream, w[i], (uint16_t*)dst, n_w, i) : kf::dequant_launch(c->stream, w[i], (uint16_t*)(dst + off));
        if (r != KF_OK) return r < 0 ? r : KF_HIP_CHECK;
        off += up256z((size_t)w[i]->ne0 * w[i]->ne1 * 2);
    }
    if (p.deq == kf::DQ_ARENA) {
        kf_ctx::DeqCopy e;
        for (int i = 0; i < 3; i++) e.key[i] = i < n_w ? w[i]->data : nullptr;
        e.form = p.deq_form, e.off = c->arena_used;
        c->copies.push_back(e);
        c->arena_used += p.deq_bytes;
    }
    *out = (const uint16_t*)dst;
    return KF_OK;
}
// what a token-batch entry knows before it launches anything (kf_gemm_plan.h)
static kf::GemmProblem problem_of(const kf_ctx* c, int entry, int n_w, const kf_weight* const* w, int n, const void* x) {
    kf::GemmProblem P;
    memset(&P, 0, sizeof(P));
    P.entry = entry, P.n_w = n_w, P.n = n, P.x_al = al16(x);
    for (int i = 0; i < n_w; i++) P.w[i] = kf::mat_of(w[i]);
    // kf_set_row_unpack: matrices of one 3- / 2-bit row form, every one of them runnable in registers, are planned as the 4-bit row codebooks of their shapes;
    // otherwise as they are stored (kf_linear's dequantise route, the shared entries' one kf_linear per matrix)
    if (c->row_unpack) (void)kf::rowq_standins(n_w, w, P.w, true);
    P.scratch = c->scratch ? (long long)c->scratch_bytes : 0;
    P.arena = c->arena != nullptr, P.capturing = c->capturing, P.arena_free = (long long)(c->arena_bytes - c->arena_used);
    for (int f = kf::DEQ_STACK; f <= kf::DEQ_ILV; f++)
        if (arena_find(c, n_w, w, f)) P.arena_hit |= 1 << f;
    return P;
}

int kf_destroy(kf_ctx* c) {
    if (!c) return KF_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->amax_val), (void)hipFree(c->amax_idx), (void)hipFree(c->muon_part);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return KF_OK;
}
int kf_sync(kf_ctx* c) {
    CHKCTX(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    return KF_OK;
}
// blocks handed out by kf_malloc / kf_tp_alloc and not yet given back to kf_free (kfdbg_live_allocations: tests/test_gpu_host_lifetimes.py); nothing on a launch path reads it
static std::atomic<long long> g_live_allocations{0};
long long kfdbg_live_allocations(void) { return g_live_allocations.load(); }
int kf_malloc(kf_ctx* c, size_t bytes, void** out) {
    CHKCTX(c);
    if (!out) return fail(KF_INVALID_ARGS, "kf_malloc: out is null");
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(KF_OUTOF_GPUMEMORY, "kf_malloc(%zu): %s", bytes, hipGetErrorString(e));
    g_live_allocations++;
    return KF_OK;
}
int kf_free(kf_ctx* c, void* p) {
    CHKCTX(c);
    if (p) {
        HIPCHK(hipFree(p));
        g_live_allocations--;
    }
    return KF_OK;
}
int kf_memset(kf_ctx* c, void* p, int v, size_t bytes) {
    CHKCTX(c);
    HIPCHK(hipMemsetAsync(p, v, bytes, c->stream));
    return KF_OK;
}
int kf_memset32(kf_ctx* c, void* p, int32_t v, size_t count) {
    CHKCTX(c);
    if (!p || ((uintptr_t)p & 3)) return fail(KF_INVALID_ARGS, "kf_memset32: null or unaligned pointer");
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)p, v, count, c->stream));
    return KF_OK;
}
int kf_h2d(kf_ctx* c, void* dst, const void* src, size_t bytes) {
    CHKCTX(c);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KF_OK;
}
int kf_d2h(kf_ctx* c, void* dst, const void* src, size_t bytes) {
    CHKCTX(c);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KF_OK;
}
int kf_d2d(kf_ctx* c, void* dst, const void* src, size_t bytes) {
    CHKCTX(c);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return KF_OK;
}
int kf_d2d_rows(kf_ctx* c, void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows) {
    CHKCTX(c);
    if (!dst || !src || width > dst_pitch || width > src_pitch) return fail(KF_INVALID_ARGS, "kf_d2d_rows: null pointer or width above a pitch");
    if (!width || !rows) return KF_OK;
    HIPCHK(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width, rows, hipMemcpyDeviceToDevice, c->stream));
    return KF_OK;
}

int kf_graph_begin(kf_ctx* c) {
    CHKCTX(c);
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_graph_begin: already capturing");
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    return KF_OK;
}
int kf_graph_end(kf_ctx* c, kf_graph** out) {
    CHKCTX(c);
    if (!c->capturing || !out) return fail(KF_INVALID_ARGS, "kf_graph_end: not capturing");
    c->capturing = false;
    kf_graph* g = new kf_graph();
    hipError_t e = hipStreamEndCapture(c->stream, &g->graph);
    if (e != hipSuccess) {
        delete g;
        return fail(KF_HIP_CHECK, "hipStreamEndCapture: %s", hipGetErrorString(e));
    }
    e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g->graph);
        delete g;
        return fail(KF_HIP_CHECK, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    *out = g;
    return KF_OK;
}
int kf_graph_launch(kf_ctx* c, kf_graph* g) {
    CHKCTX(c);
    if (!g) return fail(KF_INVALID_ARGS, "kf_graph_launch: null graph");
    HIPCHK(hipGraphLaunch(g->exec, c->stream));
    return KF_OK;
}
int kf_graph_destroy(kf_graph* g) {
    if (!g) return KF_OK;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return KF_OK;
}

int kf_event_create(void** ev) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    *ev = (void*)e;
    return KF_OK;
}
int kf_event_record(kf_ctx* c, void* ev) {
    CHKCTX(c);
    HIPCHK(hipEventRecord((hipEvent_t)ev, c->stream));
    return KF_OK;
}
int kf_event_elapsed_ms(void* a, void* b, float* ms) {
    HIPCHK(hipEventSynchronize((hipEvent_t)b));
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return KF_OK;
}
int kf_event_destroy(void* ev) {
    if (ev) HIPCHK(hipEventDestroy((hipEvent_t)ev));
    return KF_OK;
}

// ------------------------------------------------------------------------------------------------ operators
static int check_weight(const kf_weight* w, const char* who) {
    if (!w || !w->data) return fail(KF_INVALID_ARGS, "%s: null weight", who);
    if (w->ne0 <= 0 || w->ne1 <= 0) return fail(KF_INVALID_ARGS, "%s: bad shape %d x %d", who, w->ne0, w->ne1);
    if (!al16(w->data)) return fail(KF_BLAS_UNALIGN, "%s: weight data not 16-byte aligned", who);
    if (w->qzeros || w->qscales) { /* AutoAWQ layout */
        if (!w->qzeros || !w->qscales || w->type != KF_Q4 || w->lGroup != 128 || (w->ne0 % 8) || (w->ne1 % 128) || !al16(w->qscales))
            return fail(KF_QUANT_ERR, "%s: malformed AWQ weight (%d x %d, group %d)", who, w->ne0, w->ne1, w->lGroup);
        return KF_OK;
    }
    if ((w->quant == KF_QUANT_ROW_LUT && (w->type == KF_Q3 || w->type == KF_Q2)) || (w->quant == KF_QUANT_ROW_RTN && w->type == KF_Q2)) {
        /* 3- / 2-bit row forms: kf_dequant, kf_quantize for NF3, kf_linear through the dequantised copy -- or, with kf_set_row_unpack, unpacked in registers by kf_linear,
           kf_norm_linear, kf_norm_gateup_swiglu and the token-batch entries (kf_rowq.h) */
        if (!w->gama) return fail(KF_QUANT_ERR, "%s: row-quantised weight without gama", who);
        if (w->ne1 % 8) return fail(KF_BLAS_UNALIGN, "%s: rows of %d weights are not whole 8-weight units", who, w->ne1);
        return KF_OK;
    }
    if (w->quant == KF_QUANT_ROW_RTN) return fail(KF_QUANT_ERR, "%s: row-RTN storage exists for KF_Q2 only (type %d)", who, w->type);
    if (w->quant == KF_QUANT_ROW_LUT) { /* row-codebook 4-bit storage (GeQuant::RT_NormalF): nibble stream + 16 table entries per row */
        if (w->type != KF_Q4 || !w->gama) return fail(KF_QUANT_ERR, "%s: malformed row-LUT weight (type %d)", who, w->type);
        if (w->ne1 % 32) return fail(KF_BLAS_UNALIGN, "%s: row-LUT rows of %d weights are not 16-byte aligned", who, w->ne1);
        if (!al16(w->gama + w->ne0 + w->ne1)) return fail(KF_BLAS_UNALIGN, "%s: row-LUT tables not 16-byte aligned (ne0 = %d must be a multiple of 8)", who, w->ne0);
        return KF_OK;
    }
    if (w->quant != KF_QUANT_GROUP) return fail(KF_UNSUPPORTED_DATATYPE, "%s: unknown quant mode %d", who, w->quant);
    switch (w->type) {
        case KF_BF16: case KF_F8E5M2: break;
        case KF_Q4: case KF_T_SIGN: case KF_BOOL1: case KF_T_BINARY:
            if (!w->gama) return fail(KF_QUANT_ERR, "%s: quantised weight without gama", who);
            if (w->lGroup <= 0 || ((long long)w->ne0 * w->ne1) % w->lGroup) return fail(KF_QUANT_ERR, "%s: bad group size %d", who, w->lGroup);
            break;
        default: return fail(KF_UNSUPPORTED_DATATYPE, "%s: unsupported weight type %d", who, w->type);
    }
    return KF_OK;
}

int kf_dequant(kf_ctx* c, const kf_weight* w, kf_bf16* out) {
    CHKCTX(c);
    int r = check_weight(w, "kf_dequant");
    if (r) return r;
    if (!out || !al16(out)) return fail(KF_BLAS_UNALIGN, "kf_dequant: out null/unaligned");
    if (w->qzeros) RET(kf::awq_dequant_launch(c->stream, w, out));
    RET(kf::dequant_launch(c->stream, w, out));
}
int kf_quantize(kf_ctx* c, const kf_weight* w, const kf_bf16* src, int symmetric) {
    CHKCTX(c);
    int r = check_weight(w, "kf_quantize");
    if (r) return r;
    if (!src) return fail(KF_INVALID_ARGS, "kf_quantize: null src");
    RET(kf::quantize_launch(c->stream, w, src, symmetric));
}

static void init_args(kf_ctx* c, kf::GemvLaunch& L) { memset(&L, 0, sizeof(L)); L.args.alpha = 1.0f; L.canon = c->canonical; }

// Fish sizes its scratch from this answer, and the resident route lends that scratch to the split-K slots (kf_gemm_plan.h gemm_plan_linear): a smaller answer could
// change a route and with it the bits.  So it stays what it always was -- the row forms' GetDataX copy (the 4-bit row codebook's too), and the large-batch dequantise
// route's shape even where that route's tile-count test then declines.
size_t kf_linear_scratch_bytes(const kf_weight* w, int nTok) {
    if (!w || nTok < 1) return 0;
    if (w->qzeros) return kf::awq_scratch_bytes(w);
    const kf::GemmMat m = kf::mat_of(w);
    return m.quant != KF_QUANT_GROUP || kf::deq_tile_shape(m, nTok) ? (size_t)w->ne0 * w->ne1 * 2 : 0;
}
int kf_set_canonical(kf_ctx* c, int on) {
    CHKCTX(c);
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_set_canonical: not while capturing");
    c->canonical = on ? 1 : 0;
    return KF_OK;
}
int kf_get_canonical(kf_ctx* c) { return c ? c->canonical : 0; }
int kf_set_row_unpack(kf_ctx* c, int on) {
    CHKCTX(c);
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_set_row_unpack: not while capturing");
    c->row_unpack = on ? 1 : 0;
    return KF_OK;
}
int kf_get_row_unpack(kf_ctx* c) { return c ? c->row_unpack : 0; }
int kf_set_dequant_arena(kf_ctx* c, void* arena, size_t bytes) {
    CHKCTX(c);
    if (arena && !al16(arena)) return fail(KF_BLAS_UNALIGN, "kf_set_dequant_arena: unaligned");
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_set_dequant_arena: not while capturing");
    c->arena = arena, c->arena_bytes = arena ? bytes : 0, c->arena_used = 0;
    c->copies.clear();
    return KF_OK;
}
size_t kf_dequant_arena_used(kf_ctx* c) { return c ? c->arena_used : 0; }
size_t kf_dequant_arena_bytes(kf_ctx* c) { return c && c->arena ? c->arena_bytes : 0; }
size_t kf_resident_scratch_bytes(void) { return kf::gemm3_sk_ws_bytes(); }
int kf_set_scratch(kf_ctx* c, void* scratch, size_t bytes) {
    CHKCTX(c);
    if (scratch && !al16(scratch)) return fail(KF_BLAS_UNALIGN, "kf_set_scratch: unaligned");
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_set_scratch: not while capturing (captured launches hold the old pointer)");
    c->scratch = scratch, c->scratch_bytes = scratch ? bytes : 0;
    return KF_OK;
}

// one mat-vec launch per token row, all of one plan
static int linear_rows(kf_ctx* c, const kf_weight* w, const kf_bf16* x, kf_bf16* y, const kf_bf16* bias, int nTok, float alpha, float beta, const kf_bf16* residual) {
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 1, L.w[0] = w, L.mode = kf::GEMV_PLAIN, L.row_unpack = c->row_unpack;
    L.args.bias = bias, L.args.alpha = alpha, L.args.beta = beta;
    const kf::GemvPlan p = kf::gemv_plan(kf::gemv_problem(L));
    for (int t = 0; t < nTok; t++) {
        L.args.x = x + (size_t)t * w->ne1, L.args.job[0].y = y + (size_t)t * w->ne0;
        L.args.residual = residual ? residual + (size_t)t * w->ne0 : nullptr;
        int rc = kf::gemv_launch(c->stream, L, p);
        if (rc != KF_OK) return fail(rc, "kf_linear failed with %d", rc);
    }
    return KF_OK;
}
int kf_linear(kf_ctx* c, const kf_weight* w, const kf_bf16* x, kf_bf16* y, const kf_bf16* bias, int nTok, float alpha, float beta, uint32_t epilogue,
              const kf_bf16* residual) {
    CHKCTX(c);
    int r = check_weight(w, "kf_linear");
    if (r) return r;
    if (nTok < 1) return fail(KF_INVALID_ARGS, "kf_linear: nTok=%d", nTok);
    if (!x || !y || !al16(x)) return fail(KF_BLAS_UNALIGN, "kf_linear: x/y null or x unaligned");
    if ((epilogue & KF_EPI_RESIDUAL) && !residual) return fail(KF_INVALID_ARGS, "kf_linear: residual epilogue without residual");
    if (nTok > 1 && ((w->ne1 * 2) % 16 != 0)) return fail(KF_BLAS_UNALIGN, "kf_linear: token rows of x are not 16-byte aligned");
    // nTok > 1 (SLP::Forw with a batch of tokens: x [nTok, ne1] row-major, y [nTok, ne0]): the MFMA tile kernels from kf::GEMM_MIN rows up when the shape is covered,
    // otherwise one mat-vec launch per token row; which kernel, on which operand, is kf::gemm_plan's choice
    const kf_bf16* res = (epilogue & KF_EPI_RESIDUAL) ? residual : nullptr;
    const kf::GemmPlan p = kf::gemm_plan(problem_of(c, kf::GE_LINEAR, 1, &w, nTok, x));
    if (p.route == kf::GR_AWQ) { /* AutoAWQ layout: its own transposed mat-vec */
        const size_t need = kf::awq_scratch_bytes(w);
        if (need > c->scratch_bytes || !c->scratch)
            return fail(KF_INVALID_ARGS, "kf_linear: the AWQ mat-vec needs %zu bytes of scratch (kf_linear_scratch_bytes), kf_set_scratch gave %zu", need, c->scratch_bytes);
        for (int t = 0; t < nTok; t++) {
            int rc = kf::awq_linear_launch(c->stream, w, x + (size_t)t * w->ne1, y + (size_t)t * w->ne0, bias, alpha, beta, res ? res + (size_t)t * w->ne0 : nullptr,
                                           (float*)c->scratch);
            if (rc != KF_OK) return fail(rc, "kf_linear (AWQ) failed with %d", rc);
        }
        return KF_OK;
    }
    if (p.route == kf::GR_MATVEC) return linear_rows(c, w, x, y, bias, nTok, alpha, beta, res);
    if (p.route == kf::GR_TILE) {
        const kf::GemmKern k = kf::rowq_kern(p.k, c->row_unpack ? kf::rowq_fmt(w) : -1); /* a row form planned as its 4-bit stand-in: the weight's own unpack */
        const int rc = p.status ? p.status : kf::gemm_launch(c->stream, k, kf::gm_operand(w, k), x, w->ne1, nTok, y, w->ne0, bias, alpha, beta, res, w->ne0);
        return rc ? fail(rc, "kf_linear (token-batch GEMM) failed with %d", rc) : KF_OK;
    }
    // on a bf16 copy: a row form's GetDataX into the scratch, the resident copy (kf_set_dequant_arena), a large batch's dequantise into the scratch
    const bool row = p.route == kf::GR_ROWFORM, lut = row && w->type == KF_Q4, resident = p.route == kf::GR_RESIDENT;
    const char* what = lut ? "row-LUT dequant" : row ? "row-form dequant" : (resident ? "resident dequantised copy" : "dequantise for the large-batch tile kernel");
    if (row && (!c->scratch || (size_t)p.deq_bytes > c->scratch_bytes)) return fail(KF_INVALID_ARGS, "kf_linear (%s) failed with %d", what, KF_INVALID_ARGS);
    const uint16_t* W = nullptr;
    r = deq_copies(c, p, 1, &w, &W);
    if (r != KF_OK) return fail(r, "kf_linear (%s) failed with %d", what, r);
    if (!p.k.fam) { /* a row form below kf::GEMM_MIN rows, or a shape no tile kernel takes: the mat-vec on the copy */
        kf_weight wb;
        memset(&wb, 0, sizeof(wb));
        wb.data = W, wb.type = KF_BF16, wb.ne0 = w->ne0, wb.ne1 = w->ne1;
        return linear_rows(c, &wb, x, y, bias, nTok, alpha, beta, res);
    }
    const int rc = kf::gemm_launch(c->stream, p.k, kf::gm_bf16(W, w->ne0, w->ne1), x, w->ne1, nTok, y, w->ne0, bias, alpha, beta, res, w->ne0, p.ws_bytes ? c->scratch : nullptr);
    if (rc) return fail(rc, "kf_linear (%s) failed with %d", lut ? "row-LUT token-batch GEMM" : row ? "token-batch GEMM" : (resident ? "bf16 tile GEMM on the resident copy" : "large-batch bf16 tile GEMM"), rc);
    return KF_OK;
}

// ---- the LM head scored against target ids (kf_head_score.hip; the route: kf_score_plan.h)
static kf::ScoreProblem score_problem(const kf_weight* head, int n_rows, bool x_al) {
    kf::ScoreProblem P = {};
    P.w = kf::mat_of(head), P.n = n_rows, P.x_al = x_al, P.force = kf::g_knobs.score_route, P.form = kf::g_knobs.score_form;
    return P;
}
size_t kf_head_logprob_scratch_bytes(const kf_weight* head, int n_rows) {
    if (!head || n_rows < 1) return 0;
    return (size_t)kf::score_plan(score_problem(head, n_rows, true)).scratch; /* kf_head_logprob refuses an x that is not aligned: the plan is the call's */
}
int kf_head_logprob(kf_ctx* c, const kf_weight* head, const kf_bf16* x, int64_t ldx, int n_rows, const int32_t* d_targets, float* d_logprob, float* d_lse_or_null,
                    int32_t* d_top1_or_null, void* scratch) {
    CHKCTX(c);
    int r = check_weight(head, "kf_head_logprob");
    if (r) return r;
    if (n_rows < 1 || !d_targets || !d_logprob || !scratch) return fail(KF_INVALID_ARGS, "kf_head_logprob: n_rows=%d, or targets / logprob / scratch null", n_rows);
    if (ldx < head->ne1) return fail(KF_INVALID_ARGS, "kf_head_logprob: ldx=%lld below dim=%d", (long long)ldx, head->ne1);
    if (!x || !al16(x) || (ldx & 7) || !al16(scratch)) return fail(KF_BLAS_UNALIGN, "kf_head_logprob: x / scratch null or not 16-byte aligned, or ldx not a multiple of 8");
    const kf::ScorePlan p = kf::score_plan(score_problem(head, n_rows, true));
    if (p.status) return fail(p.status, "kf_head_logprob: bad shape");
    const int V = head->ne0, K = head->ne1;
    if (p.route == kf::SR_FUSED) {
        const int rc = kf::score_fused_launch(c->stream, p, (const uint16_t*)head->data, V, K, x, ldx, n_rows, d_targets, d_logprob, d_lse_or_null, d_top1_or_null, scratch);
        return rc ? fail(rc, "kf_head_logprob (fused tiles) failed with %d", rc) : KF_OK;
    }
    kf_bf16* logits = (kf_bf16*)scratch; /* [panel_rows][V] */
    for (int r0 = 0; r0 < n_rows; r0 += p.panel_rows) {
        const int m = n_rows - r0 < p.panel_rows ? n_rows - r0 : p.panel_rows;
        if (ldx == K) {
            r = kf_linear(c, head, x + (size_t)r0 * ldx, logits, nullptr, m, 1.0f, 0.0f, 0, nullptr);
            if (r) return r;
        } else { /* padded rows: kf_linear's batch form wants them dense */
            for (int t = 0; t < m; t++) {
                r = kf_linear(c, head, x + (size_t)(r0 + t) * ldx, logits + (size_t)t * V, nullptr, 1, 1.0f, 0.0f, 0, nullptr);
                if (r) return r;
            }
        }
        const int rc = kf::score_rows_launch(c->stream, logits, V, V, m, d_targets + r0, d_logprob + r0, d_lse_or_null ? d_lse_or_null + r0 : nullptr,
                                             d_top1_or_null ? d_top1_or_null + r0 : nullptr);
        if (rc) return fail(rc, "kf_head_logprob (panel fold) failed with %d", rc);
    }
    return KF_OK;
}

int kf_linear_f32(kf_ctx* c, const kf_weight* w, const kf_bf16* x, float* y) {
    CHKCTX(c);
    int r = check_weight(w, "kf_linear_f32");
    if (r) return r;
    if (!x || !y || !al16(x)) return fail(KF_BLAS_UNALIGN, "kf_linear_f32: x/y null or x unaligned");
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 1, L.w[0] = w, L.mode = kf::GEMV_PLAIN;
    L.args.x = x, L.args.yf = y, L.args.job[0].y = nullptr;
    RET(kf::gemv_launch(c->stream, L));
}
int kf_tp_reduce(kf_ctx* c, const float* partials, int n_ranks, int n, const kf_bf16* residual, kf_bf16* out) {
    CHKCTX(c);
    if (!partials || !out || n_ranks < 1 || n < 1) return fail(KF_INVALID_ARGS, "kf_tp_reduce: bad args");
    RET(kf::tp_reduce_launch(c->stream, partials, n_ranks, n, residual, out));
}

// ---- tensor-parallel exchange over peer-mapped receive areas (kf_tp.hip)
static int tp_check(const kf_tp_comm* t, const char* who) {
    if (!t || t->world < 1 || t->world > 8 || t->rank < 0 || t->rank >= t->world || t->n_max < 1 || t->per_step < 1 || !t->recv || !t->d_step || !t->d_err)
        return fail(KF_INVALID_ARGS, "%s: bad kf_tp_comm", who);
    for (int r = 0; r < t->world; r++)
        if (!t->peer[r]) return fail(KF_INVALID_ARGS, "%s: peer %d not set", who, r);
    return KF_OK;
}
static unsigned long long* tp_vec_slot(void* area, const kf_tp_comm* t, uint32_t index, int rank) {
    return (unsigned long long*)area + ((size_t)(index & 1u) * t->world + rank) * t->n_max;
}
size_t kf_tp_push_bytes(uint32_t per_step) { return (size_t)per_step * sizeof(kf::TpPushDev); }
int kf_tp_commit(kf_ctx* c, const kf_tp_comm* t) {
    CHKCTX(c);
    int r = tp_check(t, "kf_tp_commit");
    if (r) return r;
    if (!t->d_push) return fail(KF_INVALID_ARGS, "kf_tp_commit: d_push is null (kf_tp_push_bytes(per_step) bytes of device memory)");
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_tp_commit: not while capturing");
    std::vector<kf::TpPushDev> tab(t->per_step);
    for (uint32_t i = 0; i < t->per_step; i++) {
        kf::TpPushDev& d = tab[i];
        memset(&d, 0, sizeof(d));
        for (int p = 0; p < t->world; p++) d.peer[p] = tp_vec_slot(t->peer[p], t, i, t->rank);
        d.step = t->d_step, d.per_step = t->per_step, d.index = i, d.world = t->world;
    }
    HIPCHK(hipMemcpyAsync(t->d_push, tab.data(), tab.size() * sizeof(kf::TpPushDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KF_OK;
}
size_t kf_tp_recv_bytes(int world, int n_max) { return world < 1 || n_max < 1 ? 0 : ((size_t)2 * world * n_max + (size_t)2 * world) * 8; }
int kf_tp_alloc(kf_ctx* c, size_t bytes, void** out) {
    CHKCTX(c);
    if (!out || !bytes) return fail(KF_INVALID_ARGS, "kf_tp_alloc: bad args");
    // uncached (fine-grained) device memory: remote writes become visible to this device's polling loads inside a running kernel
    // No fallback to cached (coarse-grained) memory: a peer's stores into it are not guaranteed to reach a running kernel's polls, and every exchange would end in
    // a 2^24-spin timeout with no hint of the cause.
    hipError_t e = hipExtMallocWithFlags(out, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return fail(KF_OUTOF_GPUMEMORY, "kf_tp_alloc(%zu): uncached device memory refused (%s); a cached allocation cannot serve as a receive area", bytes, hipGetErrorString(e));
    }
    HIPCHK(hipMemset(*out, 0, bytes));
    g_live_allocations++;
    return KF_OK;
}
int kf_tp_ipc_export(kf_ctx* c, void* p, unsigned char handle[64]) {
    CHKCTX(c);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, p));
    memcpy(handle, &h, 64);
    return KF_OK;
}
int kf_tp_ipc_open(kf_ctx* c, const unsigned char handle[64], void** out) {
    CHKCTX(c);
    hipIpcMemHandle_t h;
    memcpy(&h, handle, 64);
    HIPCHK(hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess));
    return KF_OK;
}
int kf_tp_ipc_close(kf_ctx* c, void* p) {
    CHKCTX(c);
    HIPCHK(hipIpcCloseMemHandle(p));
    return KF_OK;
}
int kf_linear_f32_push(kf_ctx* c, const kf_weight* w, const kf_bf16* x, const kf_tp_comm* t, uint32_t index) {
    CHKCTX(c);
    int r = check_weight(w, "kf_linear_f32_push");
    if (r) return r;
    if ((r = tp_check(t, "kf_linear_f32_push"))) return r;
    if (!x || !al16(x)) return fail(KF_BLAS_UNALIGN, "kf_linear_f32_push: x null or unaligned");
    if (w->ne0 > t->n_max || index + 1 >= t->per_step) return fail(KF_INVALID_ARGS, "kf_linear_f32_push: %d rows / index %u do not fit the comm", w->ne0, index);
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 1, L.w[0] = w, L.mode = kf::GEMV_PLAIN;
    L.args.x = x, L.args.job[0].y = nullptr;
    if (!t->d_push) return fail(KF_INVALID_ARGS, "kf_linear_f32_push: kf_tp_commit has not been called");
    L.args.tp = reinterpret_cast<const kf::TpPushDev*>(t->d_push) + index;
    RET(kf::gemv_launch(c->stream, L));
}
int kf_tp_reduce_recv(kf_ctx* c, const kf_tp_comm* t, uint32_t index, int n, const kf_bf16* residual, kf_bf16* out) {
    CHKCTX(c);
    int r = tp_check(t, "kf_tp_reduce_recv");
    if (r) return r;
    if (!out || n < 1 || n > t->n_max || index + 1 >= t->per_step) return fail(KF_INVALID_ARGS, "kf_tp_reduce_recv: bad args");
    RET(kf::tp_reduce_recv_launch(c->stream, tp_vec_slot(t->recv, t, index, 0), t->world, t->n_max, n, t->d_step, t->per_step, index, residual, out, t->d_err));
}
int kf_tp_lm_head(kf_ctx* c, const kf_bf16* x, const kf_bf16* norm_w, float eps, const kf_weight* w, kf_bf16* logits, int row0, const kf_tp_comm* t, void* scratch) {
    CHKCTX(c);
    int r = tp_check(t, "kf_tp_lm_head");
    if (r) return r;
    if ((r = check_weight(w, "kf_tp_lm_head"))) return r;
    if (!x || !al16(x) || !logits) return fail(KF_BLAS_UNALIGN, "kf_tp_lm_head: x null/unaligned or no logits buffer");
    float* av = scratch ? (float*)scratch : c->amax_val;
    int* ai = scratch ? (int*)((float*)scratch + kf::KF_MAX_ARGMAX_PARTIALS) : c->amax_idx;
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 1, L.w[0] = w, L.mode = kf::GEMV_ARGMAX;
    L.args.x = x, L.args.norm_w = norm_w, L.args.eps = eps, L.args.job[0].y = logits;
    L.args.amax_val = av, L.args.amax_idx = ai;
    r = kf::gemv_launch(c->stream, L);
    if (r) return fail(r, "kf_tp_lm_head: gemv failed with %d", r);
    unsigned long long* peers[8];
    for (int p = 0; p < t->world; p++) peers[p] = (unsigned long long*)t->peer[p] + (size_t)2 * t->world * t->n_max + 2 * t->rank;
    RET(kf::tp_argmax_push_launch(c->stream, av, ai, L.blocks, row0, peers, t->world, t->d_step, t->per_step, t->per_step - 1));
}
int kf_tp_pick(kf_ctx* c, const kf_tp_comm* t, int32_t* d_state, int32_t* d_tokens_out) {
    CHKCTX(c);
    int r = tp_check(t, "kf_tp_pick");
    if (r) return r;
    if (!d_state) return fail(KF_INVALID_ARGS, "kf_tp_pick: d_state is null");
    RET(kf::tp_pick_launch(c->stream, (const unsigned long long*)t->recv + (size_t)2 * t->world * t->n_max, t->world, t->d_step, t->per_step, t->per_step - 1, d_state,
                           d_tokens_out, t->d_err, 0x7fffffff));
}

int kf_norm_linear(kf_ctx* c, const kf_bf16* x, const kf_bf16* norm_w, float eps, int n_w, const kf_weight* const* w, kf_bf16* const* y,
                   const int64_t* y_pos_stride, int pos, const int32_t* d_pos) {
    CHKCTX(c);
    if (n_w < 1 || n_w > 3 || !w || !y) return fail(KF_INVALID_ARGS, "kf_norm_linear: n_w=%d", n_w);
    if (!x || !al16(x) || (norm_w && !al16(norm_w))) return fail(KF_BLAS_UNALIGN, "kf_norm_linear: x/norm_w null or unaligned");
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = n_w, L.mode = kf::GEMV_PLAIN, L.row_unpack = c->row_unpack;
    for (int i = 0; i < n_w; i++) {
        int r = check_weight(w[i], "kf_norm_linear");
        if (r) return r;
        if (!y[i]) return fail(KF_INVALID_ARGS, "kf_norm_linear: y[%d] null", i);
        L.w[i] = w[i];
        L.args.job[i].y = y[i];
        L.args.job[i].y_pos_stride = y_pos_stride ? y_pos_stride[i] : 0;
    }
    L.args.x = x, L.args.norm_w = norm_w, L.args.eps = eps, L.args.pos = pos, L.args.d_pos = d_pos;
    RET(kf::gemv_launch(c->stream, L));
}

int kf_norm_gateup_swiglu(kf_ctx* c, const kf_bf16* x, const kf_bf16* norm_w, float eps, const kf_weight* gate, const kf_weight* up, kf_bf16* act) {
    CHKCTX(c);
    int r = check_weight(gate, "kf_norm_gateup_swiglu");
    if (r) return r;
    r = check_weight(up, "kf_norm_gateup_swiglu");
    if (r) return r;
    if (!x || !act || !al16(x)) return fail(KF_BLAS_UNALIGN, "kf_norm_gateup_swiglu: x/act");
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 2, L.w[0] = gate, L.w[1] = up, L.mode = kf::GEMV_PAIRED, L.row_unpack = c->row_unpack;
    L.args.x = x, L.args.norm_w = norm_w, L.args.eps = eps, L.args.job[0].y = act;
    RET(kf::gemv_launch(c->stream, L));
}

// ---- the row siblings of the fused decode entries: R = 1 .. 8 activation rows against one pass over the weights (kf_gemv_rows_plan.h decides; kf_gemv_rows.hip).
// A plan that does not share (the v_dot2c order, another storage, one row) is carried out here as the one-token launch row by row: the same bits either way
struct RowsCall {
    int n_w, mode, n_rows;
    const kf_weight* w[3];
    kf_bf16* y[3];
    int64_t y_row_stride[3], y_pos_stride[3];
    const kf_bf16 *x, *norm_w, *residual;
    int64_t x_stride, res_stride;
    float eps;
    int pos0;
    float* amax_val; /* GEMV_ARGMAX: [n_rows][KF_MAX_ARGMAX_PARTIALS] */
    int* amax_idx;
    int32_t* d_top1;
    kf_bf16* logits_row; /* GEMV_ARGMAX row by row without a logits matrix: one row to write them to */
};
static kf::GemvRowsLaunch rows_launch_of(const RowsCall& q) {
    kf::GemvRowsLaunch L;
    memset(&L, 0, sizeof(L));
    L.n = q.n_w, L.mode = q.mode, L.n_rows = q.n_rows;
    for (int j = 0; j < q.n_w; j++) L.w[j] = q.w[j], L.args.job[j].y = q.y[j], L.args.job[j].y_pos_stride = q.y_pos_stride[j], L.args.y_row_stride[j] = q.y_row_stride[j];
    L.args.x = q.x, L.args.x_stride = q.x_stride, L.args.norm_w = q.norm_w, L.args.eps = q.eps;
    L.args.residual = q.residual, L.args.res_stride = q.res_stride, L.args.pos0 = q.pos0;
    L.args.amax_val = q.amax_val, L.args.amax_idx = q.amax_idx;
    return L;
}
static int rows_run(kf_ctx* c, const RowsCall& q, const char* who) {
    if (q.n_rows < 1 || q.n_rows > kf::GEMV_ROWS_MAX) return fail(KF_INVALID_ARGS, "%s: n_rows=%d outside 1 .. %d", who, q.n_rows, kf::GEMV_ROWS_MAX);
    if (!q.x || !al16(q.x) || (q.x_stride & 7) || (q.norm_w && !al16(q.norm_w))) return fail(KF_BLAS_UNALIGN, "%s: x / norm_w null or not 16-byte aligned, or x_stride not a multiple of 8", who);
    for (int j = 0; j < q.n_w; j++) {
        const int r = check_weight(q.w[j], who);
        if (r) return r;
    }
    kf::GemvRowsLaunch L = rows_launch_of(q);
    const kf::GemvRowsPlan p = kf::gemv_rows_plan(kf::gemv_rows_problem(L, c->canonical));
    if (p.status) return fail(p.status, "%s: refused with %d", who, p.status);
    c->rows_shared += p.shared ? q.n_rows : 0, c->rows_single += p.shared ? 0 : q.n_rows;
    if (p.shared) {
        int rc = kf::gemv_rows_launch(c->stream, L, p);
        if (rc == KF_OK && q.mode == kf::GEMV_ARGMAX) {
            kf::argmax_rows_finish_launch(c->stream, q.amax_val, q.amax_idx, p.grid, q.n_rows, q.d_top1);
            rc = hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
        }
        return rc ? fail(rc, "%s: launch failed with %d", who, rc) : KF_OK;
    }
    kf::GemvLaunch G;
    init_args(c, G);
    G.n = q.n_w, G.mode = q.mode;
    for (int j = 0; j < q.n_w; j++) G.w[j] = q.w[j];
    G.args.norm_w = q.norm_w, G.args.eps = q.eps;
    const kf::GemvPlan g = kf::gemv_plan(kf::gemv_problem(G));
    for (int r = 0; r < q.n_rows; r++) {
        G.args.x = q.x + (size_t)r * q.x_stride, G.args.pos = q.pos0 + r;
        G.args.residual = q.residual ? q.residual + (size_t)r * q.res_stride : nullptr;
        for (int j = 0; j < q.n_w; j++) G.args.job[j].y = q.y[j] ? q.y[j] + (size_t)r * q.y_row_stride[j] : q.logits_row, G.args.job[j].y_pos_stride = q.y_pos_stride[j];
        G.args.amax_val = q.amax_val, G.args.amax_idx = q.amax_idx;
        int rc = kf::gemv_launch(c->stream, G, g);
        if (rc == KF_OK && q.mode == kf::GEMV_ARGMAX) {
            kf::argmax_finish_launch(c->stream, q.amax_val, q.amax_idx, G.blocks, q.d_top1 + r, nullptr, nullptr);
            rc = hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
        }
        if (rc != KF_OK) return fail(rc, "%s: row %d failed with %d", who, r, rc);
    }
    return KF_OK;
}
int kf_linear_rows(kf_ctx* c, const kf_weight* w, const kf_bf16* x, int64_t x_stride, kf_bf16* y, int64_t y_stride, int n_rows, uint32_t epilogue,
                   const kf_bf16* residual, int64_t residual_stride) {
    CHKCTX(c);
    if (!y) return fail(KF_INVALID_ARGS, "kf_linear_rows: y null");
    if ((epilogue & KF_EPI_RESIDUAL) && !residual) return fail(KF_INVALID_ARGS, "kf_linear_rows: residual epilogue without residual");
    RowsCall q = {};
    q.n_w = 1, q.mode = kf::GEMV_PLAIN, q.n_rows = n_rows, q.w[0] = w, q.y[0] = y, q.y_row_stride[0] = y_stride;
    q.x = x, q.x_stride = x_stride;
    if (epilogue & KF_EPI_RESIDUAL) q.residual = residual, q.res_stride = residual_stride;
    return rows_run(c, q, "kf_linear_rows");
}
int kf_norm_linear_rows(kf_ctx* c, const kf_bf16* x, int64_t x_stride, const kf_bf16* norm_w, float eps, int n_w, const kf_weight* const* w, kf_bf16* const* y,
                        const int64_t* y_row_stride, const int64_t* y_pos_stride, int pos0, int n_rows) {
    CHKCTX(c);
    if (n_w < 1 || n_w > 3 || !w || !y || !y_row_stride || pos0 < 0) return fail(KF_INVALID_ARGS, "kf_norm_linear_rows: n_w=%d, pos0=%d, or w / y / y_row_stride null", n_w, pos0);
    RowsCall q = {};
    q.n_w = n_w, q.mode = kf::GEMV_PLAIN, q.n_rows = n_rows;
    for (int i = 0; i < n_w; i++) {
        if (!y[i]) return fail(KF_INVALID_ARGS, "kf_norm_linear_rows: y[%d] null", i);
        q.w[i] = w[i], q.y[i] = y[i], q.y_row_stride[i] = y_row_stride[i], q.y_pos_stride[i] = y_pos_stride ? y_pos_stride[i] : 0;
    }
    q.x = x, q.x_stride = x_stride, q.norm_w = norm_w, q.eps = eps, q.pos0 = pos0;
    return rows_run(c, q, "kf_norm_linear_rows");
}
int kf_norm_gateup_swiglu_rows(kf_ctx* c, const kf_bf16* x, int64_t x_stride, const kf_bf16* norm_w, float eps, const kf_weight* gate, const kf_weight* up, kf_bf16* act,
                               int64_t act_stride, int n_rows) {
    CHKCTX(c);
    if (!act) return fail(KF_INVALID_ARGS, "kf_norm_gateup_swiglu_rows: act null");
    RowsCall q = {};
    q.n_w = 2, q.mode = kf::GEMV_PAIRED, q.n_rows = n_rows, q.w[0] = gate, q.w[1] = up, q.y[0] = act, q.y_row_stride[0] = act_stride;
    q.x = x, q.x_stride = x_stride, q.norm_w = norm_w, q.eps = eps;
    return rows_run(c, q, "kf_norm_gateup_swiglu_rows");
}
size_t kf_head_rows_scratch_bytes(const kf_weight* w) {
    return w ? (size_t)kf::GEMV_ROWS_MAX * kf_head_scratch_bytes() + (((size_t)w->ne0 * 2 + 15) & ~(size_t)15) : 0;
}
int kf_norm_lm_head_rows(kf_ctx* c, const kf_bf16* x, int64_t x_stride, const kf_bf16* norm_w, float eps, const kf_weight* w, kf_bf16* logits, int64_t logits_stride,
                         int32_t* d_top1, int n_rows, void* scratch) {
    CHKCTX(c);
    if (!d_top1 || !scratch || !al16(scratch)) return fail(KF_INVALID_ARGS, "kf_norm_lm_head_rows: top1 / scratch null, or scratch not 16-byte aligned");
    RowsCall q = {};
    q.n_w = 1, q.mode = kf::GEMV_ARGMAX, q.n_rows = n_rows, q.w[0] = w, q.y[0] = logits, q.y_row_stride[0] = logits_stride;
    q.x = x, q.x_stride = x_stride, q.norm_w = norm_w, q.eps = eps;
    const size_t parts = (size_t)kf::GEMV_ROWS_MAX * kf::KF_MAX_ARGMAX_PARTIALS;
    q.amax_val = (float*)scratch, q.amax_idx = (int*)(q.amax_val + parts), q.logits_row = (kf_bf16*)(q.amax_idx + parts), q.d_top1 = d_top1;
    return rows_run(c, q, "kf_norm_lm_head_rows");
}
int kf_rows_route_counts(kf_ctx* c, int64_t* out2) {
    CHKCTX(c);
    if (!out2) return fail(KF_INVALID_ARGS, "kf_rows_route_counts: out null");
    out2[0] = c->rows_shared, out2[1] = c->rows_single;
    return KF_OK;
}

// ---- sparse forward (hot rows)
int kf_hot_rows(kf_ctx* c, const int32_t* d_hot, int n, int32_t* d_rows, int32_t* d_count) {
    CHKCTX(c);
    if (!d_hot || !d_rows || !d_count || n < 1) return fail(KF_INVALID_ARGS, "kf_hot_rows: null pointer or n < 1");
    RET(kf::hot_rows_launch(c->stream, d_hot, n, d_rows, d_count));
}
int kf_zero_cold_columns(kf_ctx* c, kf_bf16* y, const int32_t* d_hot, int rows, int cols) {
    CHKCTX(c);
    if (!y || !d_hot || rows < 1 || cols < 1) return fail(KF_INVALID_ARGS, "kf_zero_cold_columns: null pointer or rows / cols < 1");
    RET(kf::cold_cols_launch(c->stream, y, d_hot, rows, cols));
}
int kf_linear_masked(kf_ctx* c, const kf_weight* w, const kf_bf16* x, kf_bf16* y, const kf_bf16* bias, const int32_t* d_rows, int n_hot) {
    CHKCTX(c);
    int r = check_weight(w, "kf_linear_masked");
    if (r) return r;
    if (!x || !y || !al16(x) || !d_rows || n_hot < 0 || n_hot > w->ne0) return fail(KF_INVALID_ARGS, "kf_linear_masked: null / unaligned pointer or n_hot outside [0, ne0]");
    if (w->qzeros) return fail(KF_UNSUPPORTED_DATATYPE, "kf_linear_masked: AutoAWQ-layout weights are served by kf_linear only");
    r = kf::cold_fill_launch(c->stream, y, bias, w->ne0); /* cold rows: 0 (+ bias); the hot rows are overwritten below */
    if (r != KF_OK || n_hot == 0) RET(r);
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 1, L.w[0] = w, L.mode = kf::GEMV_PLAIN, L.n_hot = n_hot;
    L.args.x = x, L.args.job[0].y = y, L.args.bias = bias, L.args.row_map = d_rows;
    RET(kf::gemv_launch(c->stream, L));
}
int kf_norm_gateup_swiglu_masked(kf_ctx* c, const kf_bf16* x, const kf_bf16* norm_w, float eps, const kf_weight* gate, const kf_weight* up, kf_bf16* act,
                                 const int32_t* d_rows, int n_hot) {
    CHKCTX(c);
    int r = check_weight(gate, "kf_norm_gateup_swiglu_masked");
    if (r) return r;
    r = check_weight(up, "kf_norm_gateup_swiglu_masked");
    if (r) return r;
    if (!x || !act || !al16(x) || !d_rows || n_hot < 0 || n_hot > gate->ne0) return fail(KF_INVALID_ARGS, "kf_norm_gateup_swiglu_masked: bad pointer or n_hot");
    r = kf::cold_fill_launch(c->stream, act, nullptr, gate->ne0); /* SwiGLU of two zero projections is zero */
    if (r != KF_OK || n_hot == 0) RET(r);
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 2, L.w[0] = gate, L.w[1] = up, L.mode = kf::GEMV_PAIRED, L.n_hot = n_hot;
    L.args.x = x, L.args.norm_w = norm_w, L.args.eps = eps, L.args.job[0].y = act, L.args.row_map = d_rows;
    RET(kf::gemv_launch(c->stream, L));
}

int kf_rmsnorm(kf_ctx* c, const kf_bf16* x, const kf_bf16* w, kf_bf16* y, int rows, int dim, float eps, float* rstd) {
    CHKCTX(c);
    if (!x || !w || !y) return fail(KF_INVALID_ARGS, "kf_rmsnorm: null pointer");
    if (dim % 2 != 0) return fail(KF_RMS_PARAMS, "rmsnorm dim %d is not divisible by 2", dim);
    RET(kf::rmsnorm_launch(c->stream, x, w, y, rows, dim, eps, rstd));
}

int kf_rope_table_host(float* t, int n_pos, int hd, float theta) {
    if (!t || n_pos <= 0 || hd <= 0 || (hd & 1)) return fail(KF_INVALID_ARGS, "kf_rope_table_host: bad args");
    for (int p = 0; p < n_pos; p++)
        for (int j = 0; j < hd / 2; j++) {
            const float inv_freq = 1.0f / powf(theta, (float)(j * 2) / (float)hd);
            const float angle = (float)p * inv_freq;
            t[((size_t)p * (hd / 2) + j) * 2] = cosf(angle);
            t[((size_t)p * (hd / 2) + j) * 2 + 1] = sinf(angle);
        }
    return KF_OK;
}

int kf_qknorm_rope(kf_ctx* c, kf_bf16* q, kf_bf16* k, const kf_bf16* wq, const kf_bf16* wk, const float* table, int pos, const int32_t* d_pos, int n_head,
                   int n_kv, int hd, float eps) {
    CHKCTX(c);
    if (!q) return fail(KF_INVALID_ARGS, "kf_qknorm_rope: null q");
    RET(kf::qknorm_rope_launch(c->stream, q, k, wq, wk, table, pos, d_pos, n_head, n_kv, hd, eps));
}

size_t kf_attn_scratch_bytes(int n_head, int hd) { return kf::attn_decode_scratch_bytes(n_head, hd); }
// q 16-byte and out 8-byte aligned: the tile kernels' rows
static int attn_al(const void* q, const void* out) { return (al16(q) ? kf::ATTN_Q_AL : 0) | (((uintptr_t)out & 7) == 0 ? kf::ATTN_OUT_AL : 0); }
static kf::AttnProblem attn_problem(int entry, kf_ctx* c, int n_head, int n_kv, int hd, int pos, int n_tok, int n_seq, const void* q, const void* out, long long q_stride,
                                    long long out_stride, long long kv_stride) {
    return kf::AttnProblem{entry, n_head, n_kv, hd, pos, n_tok, n_seq, c->canonical, attn_al(q, out), q_stride, out_stride, kv_stride};
}
// the decode kernel's arguments of kf_attn_decode, kf_attn_block and kf_attn_prefill's per-token route: what is not named stays 0 (no new key, q prepared, no scratch)
static kf::AttnArgs attn_args(kf_ctx* c, const kf_bf16* q, kf_bf16* kc, const kf_bf16* vc, kf_bf16* out, int pos, const int32_t* d_pos, int n_head, int n_kv, int hd,
                              int kv_stride, void* scratch) {
    kf::AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.canon = c->canonical, a.q = q, a.kcache = kc, a.vcache = vc, a.out = out;
    a.pos = pos, a.d_pos = d_pos, a.n_head = n_head, a.n_kv = n_kv, a.hd = hd, a.kv_stride = kv_stride;
    if (scratch) /* the first KF_ATTN_CNT_BYTES: arrival counters (fixed place whatever the shape); the partials behind them */
        a.counters = (int*)scratch, a.part = (float*)((char*)scratch + kf::KF_ATTN_CNT_BYTES);
    return a;
}

int kf_attn_decode(kf_ctx* c, const kf_bf16* q, const kf_bf16* kc, const kf_bf16* vc, kf_bf16* out, int pos, const int32_t* d_pos, int n_head, int n_kv, int hd,
                   int kv_stride, void* scratch) {
    CHKCTX(c);
    if (!q || !kc || !vc || !out || !scratch) return fail(KF_INVALID_ARGS, "kf_attn_decode: null pointer");
    if (!al16(kc) || !al16(vc) || (kv_stride % 8)) return fail(KF_BLAS_UNALIGN, "kf_attn_decode: cache not 16-byte aligned");
    kf::AttnArgs a = attn_args(c, q, const_cast<kf_bf16*>(kc), vc, out, pos, d_pos, n_head, n_kv, hd, kv_stride, scratch);
    RET(kf::attn_launch(c->stream, a, kf::attn_plan(attn_problem(kf::ATTN_DECODE, c, n_head, n_kv, hd, pos, 1, 1, q, out, 0, 0, 0))));
}

// R consecutive queries of one sequence in one launch (the ATTN_VERIFY entry of kf::attn_plan); the v_dot2c order: the one-token launch per row on row 0's scratch
size_t kf_attn_rows_scratch_bytes(int n_head, int hd, int n_rows) { return n_rows < 1 ? 0 : (size_t)n_rows * kf::attn_decode_scratch_bytes(n_head, hd); }
int kf_attn_decode_rows(kf_ctx* c, const kf_bf16* q, int64_t row_stride, const kf_bf16* kc, const kf_bf16* vc, kf_bf16* out, int pos0, int n_rows, int n_head, int n_kv,
                        int hd, int kv_stride, void* scratch) {
    CHKCTX(c);
    if (!q || !kc || !vc || !out || !scratch || pos0 < 0) return fail(KF_INVALID_ARGS, "kf_attn_decode_rows: null pointer or pos0 < 0");
    if (n_rows < 1 || n_rows > kf::ATTN_VERIFY_MAX) return fail(KF_INVALID_ARGS, "kf_attn_decode_rows: n_rows=%d outside 1 .. %d", n_rows, kf::ATTN_VERIFY_MAX);
    if (!al16(kc) || !al16(vc) || (kv_stride % 8) || !al16(scratch)) return fail(KF_BLAS_UNALIGN, "kf_attn_decode_rows: cache / scratch not 16-byte aligned");
    if (row_stride < (int64_t)n_head * hd) return fail(KF_INVALID_ARGS, "kf_attn_decode_rows: row_stride below n_head * hd");
    if (!c->canonical) {
        for (int r = 0; r < n_rows; r++) {
            kf::AttnArgs a = attn_args(c, q + (size_t)r * row_stride, const_cast<kf_bf16*>(kc), vc, out + (size_t)r * row_stride, pos0 + r, nullptr, n_head, n_kv, hd, kv_stride, scratch);
            const int rc = kf::attn_launch(c->stream, a, kf::attn_plan(attn_problem(kf::ATTN_DECODE, c, n_head, n_kv, hd, pos0 + r, 1, 1, q, out, 0, 0, 0)));
            if (rc != KF_OK) return fail(rc, "kf_attn_decode_rows: row %d failed with %d", r, rc);
        }
        return KF_OK;
    }
    kf::AttnArgs a = attn_args(c, q, const_cast<kf_bf16*>(kc), vc, out, pos0, nullptr, n_head, n_kv, hd, kv_stride, scratch);
    a.q_stride = row_stride;
    RET(kf::attn_launch(c->stream, a, kf::attn_plan(attn_problem(kf::ATTN_VERIFY, c, n_head, n_kv, hd, pos0, n_rows, 1, q, out, row_stride, 0, kv_stride)), true));
}

int kf_attn_block(kf_ctx* c, const kf_bf16* q_raw, const kf_bf16* k_raw, kf_bf16* kc, const kf_bf16* vc, kf_bf16* out, const kf_bf16* wq, const kf_bf16* wk,
                  const float* table, int pos, const int32_t* d_pos, int n_head, int n_kv, int hd, int kv_stride, float eps, void* scratch) {
    CHKCTX(c);
    if (!q_raw || !k_raw || !kc || !vc || !out || !scratch || !table) return fail(KF_INVALID_ARGS, "kf_attn_block: null pointer");
    if (!al16(kc) || !al16(vc) || (kv_stride % 8)) return fail(KF_BLAS_UNALIGN, "kf_attn_block: cache not 16-byte aligned");
    kf::AttnArgs a = attn_args(c, q_raw, kc, vc, out, pos, d_pos, n_head, n_kv, hd, kv_stride, scratch);
    a.k_raw = k_raw, a.wq_norm = wq, a.wk_norm = wk, a.rope_table = table, a.eps = eps;
    RET(kf::attn_launch(c->stream, a, kf::attn_plan(attn_problem(kf::ATTN_DECODE, c, n_head, n_kv, hd, pos, 1, 1, q_raw, out, 0, 0, 0))));
}

// ---- int8 KV cache (include/kf_abi.h): every launch decision is kf::attn_plan's ATTN_DECODE_KV8 entry
static kf::AttnProblem kv8_problem(int n_head, int n_kv, int hd, int pos, long long kv_stride) {
    return kf::AttnProblem{kf::ATTN_DECODE_KV8, n_head, n_kv, hd, pos, 1, 1, 1, 0, 0, 0, kv_stride};
}
int kf_attn_block_kv8_status(int n_head, int n_kv, int hd) { return kf::attn_plan(kv8_problem(n_head, n_kv, hd, 0, 0)).status; }
int kf_attn_block_kv8(kf_ctx* c, const kf_bf16* q_raw, const kf_bf16* k_raw, const kf_bf16* v_raw, int8_t* k8, int8_t* v8, float* ks, float* vs, kf_bf16* out,
                      const kf_bf16* wq, const kf_bf16* wk, const float* table, int pos, const int32_t* d_pos, int n_head, int n_kv, int hd, int kv_stride, float eps,
                      void* scratch) {
    CHKCTX(c);
    if (!q_raw || !k_raw || !v_raw || !k8 || !v8 || !ks || !vs || !out || !scratch || !table) return fail(KF_INVALID_ARGS, "kf_attn_block_kv8: null pointer");
    if (!al16(k8) || !al16(v8)) return fail(KF_BLAS_UNALIGN, "kf_attn_block_kv8: cache not 16-byte aligned");
    const kf::AttnPlan p = kf::attn_plan(kv8_problem(n_head, n_kv, hd, pos, kv_stride));
    if (p.status == KF_BLAS_UNALIGN) return fail(p.status, "kf_attn_block_kv8: kv_stride %d is not a multiple of 16", kv_stride);
    if (p.status != KF_OK || kv_stride < n_kv * hd)
        return fail(KF_INVALID_ARGS, "kf_attn_block_kv8: %d / %d heads x %d, pos %d, kv_stride %d: query heads per kv-head 1, 2, 4 or 8, head_dim 64 or 128, pos >= 0", n_head, n_kv,
                    hd, pos, kv_stride);
    kf::AttnKv8Args a;
    memset(&a, 0, sizeof(a));
    a.q = q_raw, a.k_raw = k_raw, a.v_raw = v_raw, a.k8 = k8, a.v8 = v8, a.ks = ks, a.vs = vs, a.out = out;
    a.wq_norm = wq, a.wk_norm = wk, a.rope_table = table, a.eps = eps;
    a.pos = pos, a.d_pos = d_pos, a.n_kv = n_kv, a.kv_stride = kv_stride;
    a.counters = (int*)scratch, a.part = (double*)((char*)scratch + kf::KF_ATTN_CNT_BYTES);
    RET(kf::attn_kv8_launch(c->stream, a, p));
}
static int kv8_rows_check(const char* entry, int n, int n_kv, int hd, int kv_stride) {
    if (n < 1 || n_kv < 1 || (hd != 64 && hd != 128) || kv_stride < n_kv * hd) return fail(KF_INVALID_ARGS, "%s: n=%d n_kv=%d hd=%d kv_stride=%d", entry, n, n_kv, hd, kv_stride);
    return KF_OK;
}
int kf_kv8_quant_rows(kf_ctx* c, const kf_bf16* k, const kf_bf16* v, int64_t ld, int n, int n_kv, int hd, int8_t* k8, int8_t* v8, float* ks, float* vs, int pos0, int kv_stride) {
    CHKCTX(c);
    if (!k || !v || !k8 || !v8 || !ks || !vs) return fail(KF_INVALID_ARGS, "kf_kv8_quant_rows: null pointer");
    if (const int r = kv8_rows_check("kf_kv8_quant_rows", n, n_kv, hd, kv_stride)) return r;
    if (pos0 < 0 || ld < (int64_t)n_kv * hd) return fail(KF_INVALID_ARGS, "kf_kv8_quant_rows: pos0=%d ld=%lld", pos0, (long long)ld);
    RET(kf::kv8_quant_rows_launch(c->stream, k, v, ld, n, n_kv, hd, k8, v8, ks, vs, pos0, kv_stride));
}
int kf_kv8_dequant_rows(kf_ctx* c, const int8_t* k8, const int8_t* v8, const float* ks, const float* vs, int n, int n_kv, int hd, int kv_stride, kf_bf16* kout, kf_bf16* vout,
                        int64_t ld_out) {
    CHKCTX(c);
    if (!k8 || !v8 || !ks || !vs || !kout || !vout) return fail(KF_INVALID_ARGS, "kf_kv8_dequant_rows: null pointer");
    if (const int r = kv8_rows_check("kf_kv8_dequant_rows", n, n_kv, hd, kv_stride)) return r;
    if (ld_out < (int64_t)n_kv * hd) return fail(KF_INVALID_ARGS, "kf_kv8_dequant_rows: ld_out=%lld", (long long)ld_out);
    RET(kf::kv8_dequant_rows_launch(c->stream, k8, v8, ks, vs, n, n_kv, hd, kv_stride, kout, vout, ld_out));
}
// the prompt form: every launch decision is kf::attn_plan's ATTN_PROMPT_KV8 entry
static kf::AttnProblem kv8_prefill_problem(int n_head, int n_kv, int hd, int pos0, int n_tok, int al, long long q_stride, long long kv_stride) {
    return kf::AttnProblem{kf::ATTN_PROMPT_KV8, n_head, n_kv, hd, pos0, n_tok, 1, 1, al, q_stride, 0, kv_stride};
}
int kf_attn_prefill_kv8_status(int n_head, int n_kv, int hd, int n_tok) {
    return kf::attn_plan(kv8_prefill_problem(n_head, n_kv, hd, 0, n_tok, kf::ATTN_Q_AL | kf::ATTN_OUT_AL, 0, 0)).status;
}
int kf_attn_prefill_kv8(kf_ctx* c, const kf_bf16* q, const int8_t* k8, const int8_t* v8, const float* ks, const float* vs, kf_bf16* out, int pos0, int n_tok, int64_t q_stride,
                        int n_head, int n_kv, int hd, int kv_stride) {
    CHKCTX(c);
    if (!q || !k8 || !v8 || !ks || !vs || !out) return fail(KF_INVALID_ARGS, "kf_attn_prefill_kv8: null pointer");
    if (!al16(k8) || !al16(v8)) return fail(KF_BLAS_UNALIGN, "kf_attn_prefill_kv8: cache not 16-byte aligned");
    const kf::AttnPlan p = kf::attn_plan(kv8_prefill_problem(n_head, n_kv, hd, pos0, n_tok, attn_al(q, out), q_stride, kv_stride));
    if (p.status == KF_BLAS_UNALIGN)
        return fail(p.status, "kf_attn_prefill_kv8: kv_stride %d is not a multiple of 16, q_stride %lld not a multiple of 8, q not 16-byte or out not 8-byte aligned", kv_stride,
                    (long long)q_stride);
    if (p.status != KF_OK)
        return fail(KF_INVALID_ARGS, "kf_attn_prefill_kv8: %d / %d heads x %d, pos0 %d, n_tok %d: query heads per kv-head 1, 2, 4 or 8, head_dim 64 or 128, pos0 >= 0, n_tok >= 1",
                    n_head, n_kv, hd, pos0, n_tok);
    if (q_stride < (int64_t)n_head * hd || kv_stride < n_kv * hd) return fail(KF_INVALID_ARGS, "kf_attn_prefill_kv8: q_stride=%lld kv_stride=%d", (long long)q_stride, kv_stride);
    kf::AttnPrefillKv8Args a;
    a.q = q, a.k8 = k8, a.v8 = v8, a.ks = ks, a.vs = vs, a.out = out, a.pos0 = pos0, a.n_tok = n_tok, a.n_kv = n_kv, a.kv_stride = kv_stride, a.q_stride = q_stride, a.rden = 0.0f;
    RET(kf::attn_prefill_kv8_launch(c->stream, a, p));
}

int kf_swiglu(kf_ctx* c, const kf_bf16* gate, const kf_bf16* up, kf_bf16* out, int n) {
    CHKCTX(c);
    if (!gate || !up || !out || n <= 0) return fail(KF_INVALID_ARGS, "kf_swiglu: bad args");
    RET(kf::swiglu_launch(c->stream, gate, up, out, n));
}
int kf_add(kf_ctx* c, const kf_bf16* a, const kf_bf16* b, kf_bf16* out, int n) {
    CHKCTX(c);
    if (!a || !b || !out || n <= 0) return fail(KF_INVALID_ARGS, "kf_add: bad args");
    RET(kf::add_launch(c->stream, a, b, out, n));
}
int kf_embed(kf_ctx* c, const kf_weight* w, int token, const int32_t* d_token, kf_bf16* out) {
    CHKCTX(c);
    int r = check_weight(w, "kf_embed");
    if (r) return r;
    if (!out || !al16(out)) return fail(KF_BLAS_UNALIGN, "kf_embed: out null/unaligned");
    if (!d_token && (token < 0 || token >= w->ne0)) return fail(KF_INVALID_ARGS, "kf_embed: token %d outside [0,%d)", token, w->ne0);
    RET(kf::embed_launch(c->stream, w, token, d_token, nullptr, nullptr, out));
}
int kf_embed_state(kf_ctx* c, const kf_weight* w, const int32_t* d_state, const int32_t* d_forced, kf_bf16* out) {
    CHKCTX(c);
    int r = check_weight(w, "kf_embed_state");
    if (r) return r;
    if (!out || !al16(out) || !d_state) return fail(KF_INVALID_ARGS, "kf_embed_state: bad args");
    RET(kf::embed_launch(c->stream, w, 0, nullptr, d_state, d_forced, out));
}

// ---- token batch (prefill)
int kf_embed_batch(kf_ctx* c, const kf_weight* w, const int32_t* d_tokens, int n_tok, kf_bf16* out) {
    CHKCTX(c);
    int r = check_weight(w, "kf_embed_batch");
    if (r) return r;
    if (!out || !al16(out) || !d_tokens || n_tok < 1) return fail(KF_INVALID_ARGS, "kf_embed_batch: bad args");
    RET(kf::embed_launch(c->stream, w, 0, d_tokens, nullptr, nullptr, out, n_tok));
}
// Large token batches of matrices that share their input (Q | K | V, gate | up): GetDataX of each into the caller's scratch, back to back, then ONE launch of the
// 256 x 256 bf16 tile kernel over the stacked rows (each matrix a multiple of 256 rows; its rows go to its own output).  A 1024-row K or V projection alone is 4 x 8
// tiles at 2048 tokens -- an eighth of the chip -- and took 32 us on the in-register-unpack kernels; stacked with Q it is 128 tiles.
size_t kf_linear_multi_scratch_bytes(int n_w, const kf_weight* const* w, int nTok) {
    if (!w || n_w < 2 || n_w > 3) return 0;
    kf::GemmProblem P;
    memset(&P, 0, sizeof(P));
    P.n_w = n_w, P.n = nTok;
    for (int i = 0; i < n_w; i++) {
        if (!w[i]) return 0;
        P.w[i] = kf::mat_of(w[i]);
    }
    long long bytes = 0;
    return kf::stack_shape(P, &bytes) ? (size_t)bytes : 0; /* the stacked route's copy without an arena */
}
// GR_STACKED / GR_ROPE: the plan's copies back to back, one kf_gemm3.hip launch over the stacked rows
static int stacked_launch(kf_ctx* c, const kf::GemmPlan& p, int n_w, const kf_weight* const* w, const kf_bf16* x, kf_bf16* const* y, int nTok, const kf::G3Rope* rope = nullptr) {
    int M[3] = {0, 0, 0};
    for (int i = 0; i < n_w; i++) M[i] = w[i]->ne0;
    const uint16_t* W = nullptr;
    const int r = deq_copies(c, p, n_w, w, &W);
    if (r != KF_OK) return r;
    return kf::gemm3_multi_launch(c->stream, p.k, n_w, W, M, w[0]->ne1, x, w[0]->ne1, nTok, y, rope);
}
// GR_FUSED: the direct kernel over the matrices as they are stored
static int fused_launch(kf_ctx* c, const kf::GemmPlan& p, int n_w, const kf_weight* const* w, const kf_bf16* x, int nTok, kf_bf16* const* y) {
    if (p.status) return p.status;
    const kf::GemmKern k = kf::rowq_kern(p.k, c->row_unpack ? kf::rowq_fmt(w[0]) : -1); /* row forms planned as their 4-bit stand-ins (problem_of): all of one format */
    kf::GmWeight g[3];
    for (int i = 0; i < n_w; i++) g[i] = kf::gm_operand(w[i], k);
    return kf::gemm_multi_launch(c->stream, k, n_w, g, x, w[0]->ne1, nTok, y);
}
int kf_qkv_rope_batch(kf_ctx* c, const kf_weight* wq, const kf_weight* wk, const kf_weight* wv, const kf_bf16* x, kf_bf16* q, kf_bf16* k, kf_bf16* v, int nTok, const kf_bf16* wq_norm,
                      const kf_bf16* wk_norm, const float* rope_table, int pos0, int n_head, int n_kv, int hd, float eps) {
    return kf_qkv_rope_seqs(c, wq, wk, wv, x, q, k, v, nTok, 0, wq_norm, wk_norm, rope_table, pos0, n_head, n_kv, hd, eps);
}
int kf_qkv_rope_seqs(kf_ctx* c, const kf_weight* wq, const kf_weight* wk, const kf_weight* wv, const kf_bf16* x, kf_bf16* q, kf_bf16* k, kf_bf16* v, int nTok, int seq_len,
                     const kf_bf16* wq_norm, const kf_bf16* wk_norm, const float* rope_table, int pos0, int n_head, int n_kv, int hd, float eps) {
    CHKCTX(c);
    if (!wq || !wk || !wv || !x || !q || !k || !v || nTok < 1 || pos0 < 0 || seq_len < 0 || (seq_len > 0 && (pos0 != 0 || nTok % seq_len)))
        return fail(KF_INVALID_ARGS, "kf_qkv_rope_batch / _seqs: bad args");
    const kf_weight* ws[3] = {wq, wk, wv};
    kf_bf16* ys[3] = {q, k, v};
    kf::GemmProblem P = problem_of(c, kf::GE_QKV_ROPE, 3, ws, nTok, x);
    P.rope_ok = hd == 128 && wq->ne0 == n_head * hd && wk->ne0 == n_kv * hd;
    P.y_al = (((uintptr_t)q | (uintptr_t)k) & 7) == 0;
    if (P.rope_ok && nTok >= kf::stack_min(P.arena)) {
        for (int i = 0; i < 3; i++) {
            const int r = check_weight(ws[i], "kf_qkv_rope_batch");
            if (r) return r;
        }
    }
    const kf::GemmPlan p = kf::gemm_plan(P);
    if (p.route == kf::GR_ROPE) { /* one launch: the stacked tile GEMM with q/k-norm + RoPE in its epilogue */
        const kf::G3Rope rp = {wq_norm, wk_norm, rope_table, pos0, eps, seq_len};
        const int rc = stacked_launch(c, p, 3, ws, x, ys, nTok, &rp);
        if (rc) return fail(rc, "kf_qkv_rope_batch (stacked tile GEMM + RoPE epilogue) failed with %d", rc);
        return KF_OK;
    }
    const int r = kf_linear_multi(c, 3, ws, x, ys, nTok);
    if (r) return r;
    if (seq_len > 0) return kf_qknorm_rope_train(c, q, k, wq_norm, wk_norm, rope_table, nTok, seq_len, wq->ne0, wk->ne0, n_head, n_kv, hd, eps, nullptr, nullptr);
    return kf_qknorm_rope_batch(c, q, k, wq_norm, wk_norm, rope_table, pos0, nTok, wq->ne0, wk->ne0, n_head, n_kv, hd, eps);
}
int kf_linear_multi(kf_ctx* c, int n_w, const kf_weight* const* w, const kf_bf16* x, kf_bf16* const* y, int nTok) {
    CHKCTX(c);
    if (n_w < 1 || n_w > 3 || !w || !y || !x || nTok < 1) return fail(KF_INVALID_ARGS, "kf_linear_multi: bad args (n_w=%d nTok=%d)", n_w, nTok);
    for (int i = 0; i < n_w; i++) {
        int r = check_weight(w[i], "kf_linear_multi");
        if (r) return r;
        if (!y[i]) return fail(KF_INVALID_ARGS, "kf_linear_multi: y[%d] null", i);
        if (w[i]->ne1 != w[0]->ne1) return fail(KF_INVALID_ARGS, "kf_linear_multi: the matrices do not share the input width");
    }
    const kf::GemmPlan p = kf::gemm_plan(problem_of(c, kf::GE_MULTI, n_w, w, nTok, x));
    if (p.route == kf::GR_STACKED) {
        const int rc = stacked_launch(c, p, n_w, w, x, y, nTok);
        return rc ? fail(rc, "kf_linear_multi (dequantise + stacked tile GEMM) failed with %d", rc) : KF_OK;
    }
    if (p.route == kf::GR_FUSED) {
        const int rc = fused_launch(c, p, n_w, w, x, nTok, y);
        return rc ? fail(rc, "kf_linear_multi failed with %d", rc) : KF_OK;
    }
    for (int i = 0; i < n_w; i++) {
        int r = kf_linear(c, w[i], x, y[i], nullptr, nTok, 1.0f, 0.0f, KF_EPI_NONE, nullptr);
        if (r) return r;
    }
    return KF_OK;
}
int kf_gateup_swiglu_batch(kf_ctx* c, const kf_weight* gate, const kf_weight* up, const kf_bf16* x, kf_bf16* act, kf_bf16* up_scratch, int nTok) {
    CHKCTX(c);
    int r = check_weight(gate, "kf_gateup_swiglu_batch");
    if (r) return r;
    r = check_weight(up, "kf_gateup_swiglu_batch");
    if (r) return r;
    if (!x || !act || !up_scratch || nTok < 1) return fail(KF_INVALID_ARGS, "kf_gateup_swiglu_batch: bad args");
    if (gate->ne0 != up->ne0 || gate->ne1 != up->ne1) return fail(KF_INVALID_ARGS, "kf_gateup_swiglu_batch: gate and up shapes differ");
    const kf_weight* ws[2] = {gate, up};
    kf_bf16* ys[2] = {act, up_scratch};
    kf::GemmProblem P = problem_of(c, kf::GE_GATEUP, 2, ws, nTok, x);
    P.y_al = ((uintptr_t)act & 7) == 0;
    const kf::GemmPlan p = kf::gemm_plan(P);
    if (p.route == kf::GR_SWIGLU) { /* gate | up dequantised interleaved, ONE tile-GEMM launch with the SwiGLU expression in its epilogue (on the two bf16-rounded
                                       projections, as the paired kernel and swiglu_kernel form it) */
        const uint16_t* W = nullptr;
        int rc = deq_copies(c, p, 2, ws, &W);
        if (rc == KF_OK) rc = kf::gemm3_swiglu_launch(c->stream, p.k, W, gate->ne0, gate->ne1, x, gate->ne1, nTok, act);
        return rc ? fail(rc, "kf_gateup_swiglu_batch (interleaved dequantise + tile GEMM with SwiGLU epilogue) failed with %d", rc) : KF_OK;
    }
    if (p.route == kf::GR_STACKED) {
        const int rc = stacked_launch(c, p, 2, ws, x, ys, nTok);
        if (rc) return fail(rc, "kf_gateup_swiglu_batch (dequantise + stacked tile GEMM) failed with %d", rc);
        return kf_swiglu(c, act, up_scratch, act, (size_t)nTok * gate->ne0);
    }
    if (p.route == kf::GR_FUSED) { /* the paired direct kernel */
        const int rc = fused_launch(c, p, 2, ws, x, nTok, ys);
        return rc ? fail(rc, "kf_gateup_swiglu_batch failed with %d", rc) : KF_OK;
    }
    r = kf_linear(c, gate, x, act, nullptr, nTok, 1.0f, 0.0f, KF_EPI_NONE, nullptr);
    if (r) return r;
    r = kf_linear(c, up, x, up_scratch, nullptr, nTok, 1.0f, 0.0f, KF_EPI_NONE, nullptr);
    if (r) return r;
    return kf_swiglu(c, act, up_scratch, act, nTok * gate->ne0);
}
int kf_qknorm_rope_batch(kf_ctx* c, kf_bf16* q, kf_bf16* k, const kf_bf16* wq, const kf_bf16* wk, const float* table, int pos0, int n_tok, int64_t q_stride,
                         int64_t k_stride, int n_head, int n_kv, int hd, float eps) {
    CHKCTX(c);
    if (!q || n_tok < 1 || pos0 < 0) return fail(KF_INVALID_ARGS, "kf_qknorm_rope_batch: bad args");
    if (hd % 2) return fail(KF_RMS_PARAMS, "head_dim %d is not divisible by 2", hd);
    RET(kf::qknorm_rope_launch(c->stream, q, k, wq, wk, table, pos0, nullptr, n_head, n_kv, hd, eps, n_tok, q_stride, k_stride));
}
int kf_qknorm_rope_train(kf_ctx* c, kf_bf16* q, kf_bf16* k, const kf_bf16* wq, const kf_bf16* wk, const float* table, int n_tok, int seq_len, int64_t q_stride,
                         int64_t k_stride, int n_head, int n_kv, int hd, float eps, float* rstd_q, float* rstd_k) {
    CHKCTX(c);
    if (!q || n_tok < 1 || seq_len < 1) return fail(KF_INVALID_ARGS, "kf_qknorm_rope_train: bad args");
    if (hd % 2) return fail(KF_RMS_PARAMS, "head_dim %d is not divisible by 2", hd);
    RET(kf::qknorm_rope_launch(c->stream, q, k, wq, wk, table, 0, nullptr, n_head, n_kv, hd, eps, n_tok, q_stride, k_stride, seq_len, rstd_q, rstd_k));
}
int kf_attn_prefill(kf_ctx* c, const kf_bf16* q, const kf_bf16* kc, const kf_bf16* vc, kf_bf16* out, int pos0, int n_tok, int64_t q_stride, int n_head, int n_kv,
                    int hd, int kv_stride) {
    CHKCTX(c);
    if (!q || !kc || !vc || !out || n_tok < 1 || pos0 < 0) return fail(KF_INVALID_ARGS, "kf_attn_prefill: bad args");
    if (!al16(kc) || !al16(vc) || (kv_stride % 8)) return fail(KF_BLAS_UNALIGN, "kf_attn_prefill: cache not 16-byte aligned");
    const kf::AttnPlan p = kf::attn_plan(attn_problem(kf::ATTN_PROMPT, c, n_head, n_kv, hd, pos0, n_tok, 1, q, out, q_stride, 0, kv_stride));
    if (p.route != kf::ATTN_PER_TOKEN) {
        const int rc = kf::attn_prefill_mfma_launch(c->stream, p, q, kc, vc, out, pos0, n_tok, q_stride, n_kv, kv_stride, 1, 0);
        if (rc != KF_OK) return fail(rc, "kf_attn_prefill: launch failed (%d)", rc);
        return KF_OK;
    }
    kf::AttnArgs a = attn_args(c, q, const_cast<kf_bf16*>(kc), vc, out, pos0, nullptr, n_head, n_kv, hd, kv_stride, nullptr);
    a.q_stride = q_stride, a.one_slice = 1;
    RET(kf::attn_launch(c->stream, a, p));
}

int kf_attn_prefill_batch(kf_ctx* c, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, kf_bf16* out, int n_tok, int64_t q_stride, int n_head, int n_kv, int hd,
                          int kv_stride, int n_seq) {
    CHKCTX(c);
    if (!q || !k || !v || !out || n_tok < 1 || n_seq < 1) return fail(KF_INVALID_ARGS, "kf_attn_prefill_batch: bad args");
    if (!al16(k) || !al16(v) || (kv_stride % 8)) return fail(KF_BLAS_UNALIGN, "kf_attn_prefill_batch: k / v rows not 16-byte aligned");
    const kf::AttnPlan p = kf::attn_plan(attn_problem(kf::ATTN_BATCH, c, n_head, n_kv, hd, 0, n_tok, n_seq, q, out, q_stride, 0, kv_stride));
    if (p.status != KF_OK) return fail(KF_INVALID_ARGS, "kf_attn_prefill_batch: shape not covered by the tile kernel (head_dim 64 / 128, n_head / n_kv in 1, 2, 4, 8, 16-byte aligned rows)");
    RET(kf::attn_prefill_mfma_launch(c->stream, p, q, k, v, out, 0, n_tok, q_stride, n_kv, kv_stride, n_seq, 0));
}
int kf_attn_prefill_batch_strided(kf_ctx* c, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, kf_bf16* out, int n_tok, int64_t q_stride, int64_t out_stride, int n_head,
                                  int n_kv, int hd, int kv_stride, int n_seq) {
    CHKCTX(c);
    if (!q || !k || !v || !out || n_tok < 1 || n_seq < 1 || out_stride < (int64_t)n_head * hd) return fail(KF_INVALID_ARGS, "kf_attn_prefill_batch_strided: bad args");
    if (!al16(k) || !al16(v) || (kv_stride % 8)) return fail(KF_BLAS_UNALIGN, "kf_attn_prefill_batch_strided: k / v rows not 16-byte aligned");
    const kf::AttnPlan p = kf::attn_plan(attn_problem(kf::ATTN_BATCH, c, n_head, n_kv, hd, 0, n_tok, n_seq, q, out, q_stride, out_stride, kv_stride));
    if (p.status != KF_OK) return fail(KF_INVALID_ARGS, "kf_attn_prefill_batch_strided: shape not covered by the tile kernel (head_dim 64 / 128, n_head / n_kv in 1, 2, 4, 8, 16-byte aligned rows)");
    RET(kf::attn_prefill_mfma_launch(c->stream, p, q, k, v, out, 0, n_tok, q_stride, n_kv, kv_stride, n_seq, out_stride));
}

int kf_set_state(kf_ctx* c, int32_t* d_state, int token, int pos) {
    CHKCTX(c);
    if (!d_state) return fail(KF_INVALID_ARGS, "kf_set_state: null state");
    RET(kf::set_state_launch(c->stream, d_state, token, pos));
}

size_t kf_head_scratch_bytes(void) { return (sizeof(float) + sizeof(int)) * (size_t)kf::KF_MAX_ARGMAX_PARTIALS; }

static int head_impl(kf_ctx* c, const kf_bf16* x, const kf_bf16* norm_w, float eps, const kf_weight* w, kf_bf16* logits, int32_t* d_argmax, int32_t* d_state,
                     int32_t* d_tokens_out, void* scratch, const char* who) {
    int r = check_weight(w, who);
    if (r) return r;
    if (!x || !al16(x)) return fail(KF_BLAS_UNALIGN, "%s: x null/unaligned", who);
    float* av = scratch ? (float*)scratch : c->amax_val;
    int* ai = scratch ? (int*)((float*)scratch + kf::KF_MAX_ARGMAX_PARTIALS) : c->amax_idx;
    kf_bf16* lg = logits;
    if (!lg) return fail(KF_INVALID_ARGS, "%s: logits buffer required (vocab*2 bytes)", who);
    kf::GemvLaunch L;
    init_args(c, L);
    L.n = 1, L.w[0] = w, L.mode = kf::GEMV_ARGMAX;
    L.args.x = x, L.args.norm_w = norm_w, L.args.eps = eps, L.args.job[0].y = lg;
    L.args.amax_val = av, L.args.amax_idx = ai;
    r = kf::gemv_launch(c->stream, L);
    if (r) return fail(r, "%s: gemv failed with %d", who, r);
    // (the pick stays its own 4-us launch: folded into this kernel behind an arrival ticket -- write-through partial stores, drained, one atomic per workgroup -- it
    // measured 2-5 us SLOWER per step than the separate launch, and with a release fence per workgroup 170 us slower)
    if (d_argmax || d_state) kf::argmax_finish_launch(c->stream, av, ai, L.blocks, d_argmax, d_state, d_tokens_out); /* both NULL: logits only */
    return hipGetLastError() == hipSuccess ? KF_OK : fail(KF_HIP_CHECK, "%s: launch failed", who);
}
int kf_lm_head(kf_ctx* c, const kf_weight* w, const kf_bf16* x, kf_bf16* logits, int32_t* d_argmax_out, void* scratch) {
    CHKCTX(c);
    return head_impl(c, x, nullptr, 0.f, w, logits, d_argmax_out, nullptr, nullptr, scratch, "kf_lm_head");
}
int kf_norm_lm_head(kf_ctx* c, const kf_bf16* x, const kf_bf16* norm_w, float eps, const kf_weight* w, kf_bf16* logits, int32_t* d_state, int32_t* d_tokens_out,
                    void* scratch) {
    CHKCTX(c);
    return head_impl(c, x, norm_w, eps, w, logits, nullptr, d_state, d_tokens_out, scratch, "kf_norm_lm_head");
}

int kf_sample(kf_ctx* c, const kf_bf16* logits, int n, int top_k, float temperature, float top_p, uint64_t* d_rng_state, int32_t* d_token, int32_t* d_state,
              int32_t* d_tokens_out, const int32_t* d_forced, int n_forced) {
    CHKCTX(c);
    if (!logits || !d_rng_state || (!d_token && !d_state)) return fail(KF_INVALID_ARGS, "kf_sample: null pointer");
    int r = kf::sample_launch(c->stream, logits, n, top_k, temperature, top_p, (unsigned long long*)d_rng_state, d_token, d_state, d_tokens_out, d_forced, n_forced);
    if (r == KF_INVALID_ARGS)
        return fail(r, "kf_sample: needs 2 <= top_k < n/2 (TOPK_heap::Select asserts it), top_k <= 1024, temperature > 0, top_p > 0 (got k=%d n=%d T=%g p=%g)",
                    top_k, n, temperature, top_p);
    RET(r);
}

int kf_sample_topk(kf_ctx* c, const kf_bf16* logits, int n, int top_k, float temperature, float top_p, uint64_t* d_rng_state, int32_t* d_token, int32_t* d_state,
                   int32_t* d_tokens_out, const int32_t* d_forced, int n_forced) {
    CHKCTX(c);
    if (!logits || !d_rng_state || (!d_token && !d_state)) return fail(KF_INVALID_ARGS, "kf_sample_topk: null pointer");
    int r = kf::sample_launch(c->stream, logits, n, top_k, temperature, top_p, (unsigned long long*)d_rng_state, d_token, d_state, d_tokens_out, d_forced, n_forced, 1);
    if (r == KF_INVALID_ARGS) return fail(r, "kf_sample_topk: needs 2 <= top_k < n/2, top_k <= 1024, temperature > 0, top_p > 0 (got k=%d n=%d T=%g p=%g)", top_k, n, temperature, top_p);
    RET(r);
}
int kf_layernorm(kf_ctx* c, const kf_bf16* x, const kf_bf16* w, const kf_bf16* bias, kf_bf16* y, int rows, int dim, float eps, float* mean, float* rstd) {
    CHKCTX(c);
    if (!x || !w || !y || rows < 1 || dim < 1) return fail(KF_INVALID_ARGS, "kf_layernorm: bad args");
    RET(kf::layernorm_launch(c->stream, x, w, bias, y, rows, dim, eps, mean, rstd));
}
int kf_gelu(kf_ctx* c, const kf_bf16* x, kf_bf16* y, size_t n) {
    CHKCTX(c);
    if (!x || !y || n == 0) return fail(KF_INVALID_ARGS, "kf_gelu: bad args");
    RET(kf::gelu_launch(c->stream, x, y, n));
}
// scratch layout of kf_linear_backward: [W bf16 OC*IC][middle][bias slabs fp64 ceil(n/256)*OC], each 256-B aligned; the middle region is either the transposed copies
// [W^T bf16 IC*OC][deltaIn^T bf16 OC*n][inp^T bf16 IC*n] of the small-shape path or the partial-tile slots of the large tile kernel's stream-K form (kf_gemm3.hip)
static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t lbw_mid_bytes(int OC, int IC, int n) {
    const size_t t = up256((size_t)OC * IC * 2) + up256((size_t)OC * n * 2) + up256((size_t)IC * n * 2), k = up256(kf::gemm3_sk_ws_bytes());
    return t > k ? t : k;
}
size_t kf_linear_backward_scratch_bytes(int OC, int IC, int n) {
    if (OC < 1 || IC < 1 || n < 1) return 0;
    return up256((size_t)OC * IC * 2) + lbw_mid_bytes(OC, IC, n) + up256((size_t)((n + 255) / 256) * OC * 8);
}
int kf_linear_backward(kf_ctx* c, const kf_weight* w, const kf_bf16* deltaIn, const kf_bf16* inp, kf_bf16* delta, kf_bf16* gW, kf_bf16* gBias, int n, int accumulate_delta,
                       void* scratch) {
    CHKCTX(c);
    int r = check_weight(w, "kf_linear_backward");
    if (r) return r;
    if (w->qzeros) return fail(KF_UNSUPPORTED_DATATYPE, "kf_linear_backward: AutoAWQ-layout weights are inference-only");
    if (!deltaIn || !scratch || n < 1) return fail(KF_INVALID_ARGS, "kf_linear_backward: null deltaIn / scratch or n < 1");
    if ((gW && !inp) || (!delta && !gW && !gBias)) return fail(KF_INVALID_ARGS, "kf_linear_backward: gW needs inp; nothing to compute");
    const int OC = w->ne0, IC = w->ne1;
    // the MFMA kernels contract over multiples of 64 and want 16-byte aligned rows
    if ((OC % 64) || OC < 128 || (IC % 8) || (gW && ((n % 64) || n < 128)))
        return fail(KF_INVALID_ARGS, "kf_linear_backward: OC (and n, for the weight gradient) must be multiples of 64 and >= 128, IC a multiple of 8 (got %d %d %d)", OC, IC, n);
    if (!al16(deltaIn) || (inp && !al16(inp)) || (delta && !al16(delta)) || (gW && !al16(gW)) || ((uintptr_t)scratch & 255))
        return fail(KF_BLAS_UNALIGN, "kf_linear_backward: tensors must be 16-byte aligned, scratch 256-byte aligned");
    char* p = (char*)scratch;
    uint16_t* Wd = (uint16_t*)p;    p += up256((size_t)OC * IC * 2);
    uint16_t* WdT = (uint16_t*)p;   p += up256((size_t)OC * IC * 2);
    uint16_t* dInT = (uint16_t*)p;  p += up256((size_t)OC * n * 2);
    uint16_t* inpT = (uint16_t*)p;
    double* slabs = (double*)((char*)scratch + up256((size_t)OC * IC * 2) + lbw_mid_bytes(OC, IC, n));
    void* const sk_ws = WdT; /* the middle region: stream-K slots when the large tile kernel takes the shape, the transposed copies otherwise */
    const size_t sk_bytes = lbw_mid_bytes(OC, IC, n);
    if (gBias) {
        r = kf::colsum_add_launch(c->stream, deltaIn, gBias, n, OC, slabs);
        if (r != KF_OK) return fail(r, "kf_linear_backward: bias column sums failed with %d", r);
    }
    kf::GemmProblem P; /* the two products' plans (kf_gemm_plan.h gemm_plan_backward): the middle region lends the split-K slots */
    memset(&P, 0, sizeof(P));
    P.n_w = 1, P.w[0] = kf::mat_of(w), P.n = n, P.x_al = 1, P.scratch = (long long)sk_bytes;
    if (delta) { /* delta [n, IC] (+)= deltaIn [n, OC] . W [OC, IC]: rows of W^T are contiguous in the contraction index OC */
        P.entry = kf::GE_BWD_DX;
        const kf::GemmPlan p = kf::gemm_plan(P);
        const uint16_t* Wsrc = (const uint16_t*)w->data;
        r = KF_OK;
        if (w->type != KF_BF16) r = kf::dequant_launch(c->stream, w, Wd), Wsrc = Wd;
        if (r != KF_OK) return fail(r, "kf_linear_backward: dequantise of the weight failed with %d", r);
        if (p.route == kf::GR_KMAJOR) { /* large shapes: the tile kernel reads W as the K-MAJOR operand it already is (contraction over its OC rows): no transpose */
            r = kf::gemm3_km_launch(c->stream, p.k, Wsrc, IC, deltaIn, OC, n, IC, OC, delta, IC, 1.0f, accumulate_delta ? 1.0f : 0.0f, sk_ws);
            if (r) return fail(r, "kf_linear_backward: input-gradient GEMM failed with %d", r);
        } else {
            r = w->type == KF_BF16 ? kf::dequant_launch(c->stream, w, Wd) : KF_OK;
            if (r == KF_OK) r = kf::transpose_bf16_launch(c->stream, Wd, WdT, OC, IC);
            if (r != KF_OK) return fail(r, "kf_linear_backward: dequantise / transpose of the weight failed with %d", r);
            r = p.k.fam ? kf::gemm_launch(c->stream, p.k, kf::gm_bf16(WdT, IC, OC), deltaIn, OC, n, delta, IC, nullptr, 1.0f, accumulate_delta ? 1.0f : 0.0f, nullptr, IC) : 1;
            if (r != KF_OK) return fail(r < 0 ? r : KF_INVALID_ARGS, "kf_linear_backward: input-gradient GEMM not covered (%d)", r);
        }
    }
    if (gW) { /* both operands are k-major for the contraction over the n token rows: inp [n][IC] is the "weight" side, deltaIn [n][OC] the "token" side */
        P.entry = kf::GE_BWD_DW;
        const kf::GemmPlan p = kf::gemm_plan(P);
        if (p.route == kf::GR_KMAJOR) {
            r = kf::gemm3_km_launch(c->stream, p.k, inp, IC, deltaIn, OC, OC, IC, n, gW, IC, 1.0f, 1.0f, sk_ws);
            if (r) return fail(r, "kf_linear_backward: weight-gradient GEMM failed with %d", r);
        } else { /* gW [OC, IC] += deltaIn^T [OC, n] . inp [n, IC]: "weight" = inp^T [IC, n], "tokens" = the OC rows of deltaIn^T, contraction over n */
            r = kf::transpose_bf16_launch(c->stream, deltaIn, dInT, n, OC);
            if (r == KF_OK) r = kf::transpose_bf16_launch(c->stream, inp, inpT, n, IC);
            if (r != KF_OK) return fail(r, "kf_linear_backward: operand transposes failed with %d", r);
            r = p.k.fam ? kf::gemm_launch(c->stream, p.k, kf::gm_bf16(inpT, IC, n), dInT, n, OC, gW, IC, nullptr, 1.0f, 1.0f, nullptr, IC) : 1;
            if (r != KF_OK) return fail(r < 0 ? r : KF_INVALID_ARGS, "kf_linear_backward: weight-gradient GEMM not covered (%d)", r);
        }
    }
    return KF_OK;
}
// ---- "train_target": "gama" (SLP::Back's gama branch -> CU_GamaBack_2): the (zero, step) gradients of a group-quantised weight (kf_gama_bwd.hip; the launch: kf_gama_plan.h)
size_t kf_gama_backward_scratch_bytes(int OC, int IC, int n) {
    const kf::GamaPlan p = kf::gama_plan(OC, IC, n);
    return p.status == KF_OK ? (size_t)p.scratch : 0;
}
int kf_gama_backward(kf_ctx* c, const kf_weight* w, const kf_bf16* deltaIn, const kf_bf16* inp, kf_bf16* gGama, int n, float scale, void* scratch) {
    CHKCTX(c);
    int r = check_weight(w, "kf_gama_backward");
    if (r) return r;
    if (w->qzeros || w->qscales) return fail(KF_UNSUPPORTED_DATATYPE, "kf_gama_backward: AutoAWQ-layout weights are inference-only");
    if (w->quant != KF_QUANT_GROUP) return fail(KF_UNSUPPORTED_DATATYPE, "kf_gama_backward: row-quantised storage (quant mode %d) has no (zero, step) per group", w->quant);
    int fmt;
    switch (w->type) {
        case KF_Q4: fmt = kf::FMT_Q4; break;
        case KF_T_SIGN: fmt = kf::FMT_Q2; break;
        case KF_BOOL1: fmt = kf::FMT_Q1; break;
        default: return fail(KF_UNSUPPORTED_DATATYPE, "kf_gama_backward: type %d is not a PackedQ group storage (KF_Q4, KF_T_SIGN, KF_BOOL1)", w->type);
    }
    if (!deltaIn || !inp || !gGama || !scratch) return fail(KF_INVALID_ARGS, "kf_gama_backward: null deltaIn / inp / gGama / scratch");
    const int OC = w->ne0, IC = w->ne1;
    const kf::GamaPlan p = kf::gama_plan(OC, IC, n);
    if (p.status != KF_OK || w->lGroup != kf::GAMA_GROUP || (long long)w->nGroup * kf::GAMA_GROUP != (long long)OC * IC)
        return fail(KF_INVALID_ARGS, "kf_gama_backward: needs groups of 128, IC a multiple of 128, OC and n multiples of 64, OC >= 128 (got %d x %d, n %d, group %d)", OC, IC, n, w->lGroup);
    if (!al16(deltaIn) || !al16(inp) || !al16(gGama) || ((uintptr_t)scratch & 255))
        return fail(KF_BLAS_UNALIGN, "kf_gama_backward: tensors must be 16-byte aligned, scratch 256-byte aligned");
    r = kf::gama_backward_launch(c->stream, p, (const unsigned char*)w->data, fmt, w->qBias, OC, IC, deltaIn, inp, n, gGama, scale, (float*)scratch);
    RET(r);
}
// ---- low-rank adapters beside a frozen matrix (SLP::Forw / SLP::Back, LORA branch -> HIERARCH_LorAB::Forw / Back): kf_lora.hip; the launches: kf_lora_plan.h
size_t kf_lora_backward_scratch_bytes(int r, int OC, int IC, int n) {
    const kf::LoraPlan p = kf::lora_plan(r, OC, IC, n);
    return p.status == KF_OK ? (size_t)p.scratch : 0;
}
int kf_lora_forward(kf_ctx* c, const kf_bf16* a, const kf_bf16* b, int r, int OC, int IC, const kf_bf16* x, kf_bf16* y, kf_bf16* ax, int n, float s) {
    CHKCTX(c);
    if (!a || !b || !x || !y || !ax) return fail(KF_INVALID_ARGS, "kf_lora_forward: null a / b / x / y / ax");
    const kf::LoraPlan p = kf::lora_plan(r, OC, IC, n);
    if (p.status != KF_OK)
        return fail(KF_INVALID_ARGS, "kf_lora_forward: needs rank 16, 32 or 64, OC and IC multiples of 64 and >= 128, n a multiple of 64 and >= 64 (got rank %d, %d x %d, n %d)", r, OC, IC, n);
    if (!al16(a) || !al16(b) || !al16(x) || !al16(y) || !al16(ax)) return fail(KF_BLAS_UNALIGN, "kf_lora_forward: tensors must be 16-byte aligned");
    RET(kf::lora_forward_launch(c->stream, p, a, b, r, OC, IC, x, y, ax, n, s));
}
int kf_lora_backward(kf_ctx* c, const kf_bf16* a, const kf_bf16* b, int r, int OC, int IC, const kf_bf16* deltaIn, const kf_bf16* inp, const kf_bf16* ax, kf_bf16* delta, kf_bf16* g,
                     int n, float s, void* scratch) {
    CHKCTX(c);
    if (!a || !b || !deltaIn || !inp || !ax || !delta || !g || !scratch) return fail(KF_INVALID_ARGS, "kf_lora_backward: null a / b / deltaIn / inp / ax / delta / g / scratch");
    const kf::LoraPlan p = kf::lora_plan(r, OC, IC, n);
    if (p.status != KF_OK)
        return fail(KF_INVALID_ARGS, "kf_lora_backward: needs rank 16, 32 or 64, OC and IC multiples of 64 and >= 128, n a multiple of 64 and >= 64 (got rank %d, %d x %d, n %d)", r, OC, IC, n);
    if (!al16(a) || !al16(b) || !al16(deltaIn) || !al16(inp) || !al16(ax) || !al16(delta) || !al16(g) || ((uintptr_t)scratch & 255))
        return fail(KF_BLAS_UNALIGN, "kf_lora_backward: tensors must be 16-byte aligned, scratch 256-byte aligned");
    RET(kf::lora_backward_launch(c->stream, p, a, b, r, OC, IC, deltaIn, inp, ax, delta, g, n, s, (unsigned char*)scratch));
}
// ---- the same pair at inference (kf_lora_apply.hip): the form and the geometry are kf::lora_apply_plan's
int kf_lora_apply_status(int r, int OC, int IC, int n, int n_w) { return kf::lora_apply_plan(r, OC, IC, n, n_w).status; }
int kf_lora_apply(kf_ctx* c, int n_w, const kf_bf16* const* h_a, const kf_bf16* const* h_b, int r, const int* h_OC, int IC, const kf_bf16* x, kf_bf16* const* h_y, kf_bf16* ax,
                  int n, float s) {
    CHKCTX(c);
    if (!h_a || !h_b || !h_OC || !h_y || !x || n_w < 1 || n_w > kf::LORA_APPLY_MAX) return fail(KF_INVALID_ARGS, "kf_lora_apply: null h_a / h_b / h_OC / h_y / x, or n_w %d outside 1 .. 3", n_w);
    kf::LoraApplyPlan p[kf::LORA_APPLY_MAX];
    for (int i = 0; i < n_w; i++) {
        if (!h_a[i] || !h_b[i] || !h_y[i]) return fail(KF_INVALID_ARGS, "kf_lora_apply: null a / b / y of adapter %d", i);
        p[i] = kf::lora_apply_plan(r, h_OC[i], IC, n, n_w);
        if (p[i].status != KF_OK)
            return fail(KF_INVALID_ARGS, "kf_lora_apply: needs rank 16, 32 or 64, OC and IC multiples of 64 and >= 128, n >= 1, and n == 1 for more than one adapter (got rank %d, %d x %d, n %d, %d adapters)",
                        r, h_OC[i], IC, n, n_w);
        if (!al16(h_a[i]) || !al16(h_b[i]) || !al16(h_y[i])) return fail(KF_BLAS_UNALIGN, "kf_lora_apply: tensors must be 16-byte aligned");
    }
    if (!al16(x) || !al16(ax)) return fail(KF_BLAS_UNALIGN, "kf_lora_apply: tensors must be 16-byte aligned");
    RET(kf::lora_apply_launch(c->stream, p, n_w, h_a, h_b, r, h_OC, IC, x, h_y, ax, n, s));
}
size_t kf_attn_backward_scratch_bytes(int T, int n_head, int n_seq) { return kf::attn_backward_scratch_bytes(T, n_head, n_seq); }
int kf_attn_backward(kf_ctx* c, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, long long ld_qkv, const kf_bf16* o, const kf_bf16* dO, long long ld_o, kf_bf16* dq,
                     kf_bf16* dk, kf_bf16* dv, long long ld_d, int T, int n_head, int n_kv, int hd, int n_seq, void* scratch) {
    CHKCTX(c);
    if (!q || !k || !v || !o || !dO || !dq || !dk || !dv || !scratch || n_seq < 1 || n_kv < 1 || n_head % n_kv) return fail(KF_INVALID_ARGS, "kf_attn_backward: null pointer, n_seq < 1 or n_head not a multiple of n_kv");
    if (!al16(q) || !al16(k) || !al16(v) || !al16(o) || !al16(dO) || !al16(dq) || !al16(dk) || !al16(dv) || (ld_qkv % 8) || (ld_o % 8) || (ld_d % 8) || ((uintptr_t)scratch & 3))
        return fail(KF_BLAS_UNALIGN, "kf_attn_backward: rows must be 16-byte aligned");
    if (ld_qkv < (long long)n_head * hd || ld_o < (long long)n_head * hd || ld_d < (long long)n_head * hd) return fail(KF_INVALID_ARGS, "kf_attn_backward: row stride below n_head * head_dim");
    if (T < 1 || n_head < 1) return fail(KF_INVALID_ARGS, "kf_attn_backward: T / n_head < 1");
    const kf::AttnPlan p = kf::attn_plan(attn_problem(kf::ATTN_BACKWARD, c, n_head, n_kv, hd, 0, T, n_seq, q, dq, 0, 0, 0));
    if (p.status != KF_OK) return fail(p.status, "kf_attn_backward: head_dim %d not covered (64, 128)", hd);
    RET(kf::attn_backward_mfma_launch(c->stream, p, q, k, v, ld_qkv, o, dO, ld_o, dq, dk, dv, ld_d, T, (float*)scratch, ld_qkv, ld_d));
}
// ---- packed documents (kf_attn_docs_plan.h): the plan on the host, the three launches and the row-position forms of the q/k-norm + RoPE entries
size_t kf_attn_docs_table_bytes(const int32_t* row0, const int32_t* len, int n_doc, int n_rows, int max_len, int n_head, int n_kv, int hd) {
    const kf::AttnDocsPlan p = kf::attn_docs_plan(row0, len, n_doc, n_rows, max_len, n_head, n_kv, hd);
    return p.status == KF_OK ? p.bytes() : 0;
}
int kf_attn_docs_plan(const int32_t* row0, const int32_t* len, int n_doc, int n_rows, int max_len, int n_head, int n_kv, int hd, void* h_table, size_t table_bytes) {
    if (!h_table) return fail(KF_INVALID_ARGS, "kf_attn_docs_plan: null table");
    const kf::AttnDocsPlan p = kf::attn_docs_plan(row0, len, n_doc, n_rows, max_len, n_head, n_kv, hd);
    if (p.status != KF_OK)
        return fail(KF_INVALID_ARGS, "kf_attn_docs_plan: needs n_doc >= 1 ascending, non-overlapping documents of 1 .. max_len rows inside n_rows, and a head geometry the "
                                     "attention entries take (head_dim 64 / 128, n_head / n_kv in 1, 2, 4, 8)");
    if (table_bytes < p.bytes()) return fail(KF_INVALID_ARGS, "kf_attn_docs_plan: the table needs %zu bytes (kf_attn_docs_table_bytes), got %zu", p.bytes(), table_bytes);
    memcpy(h_table, &p.hdr, sizeof(p.hdr));
    memcpy((char*)h_table + sizeof(p.hdr), p.entries.data(), p.entries.size() * sizeof(kf_attn_docs_entry));
    return KF_OK;
}
int kf_attn_prefill_docs(kf_ctx* c, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, kf_bf16* out, const kf_attn_docs_header* h, const void* d_table, int64_t q_stride,
                         int64_t out_stride, int n_head, int n_kv, int hd, int kv_stride) {
    CHKCTX(c);
    if (!q || !k || !v || !out || !h || !d_table || out_stride < (int64_t)n_head * hd) return fail(KF_INVALID_ARGS, "kf_attn_prefill_docs: null pointer or out_stride below n_head * head_dim");
    if (!al16(k) || !al16(v) || (kv_stride % 8) || !al16(d_table)) return fail(KF_BLAS_UNALIGN, "kf_attn_prefill_docs: k / v rows and the table must be 16-byte aligned");
    const kf::AttnPlan p = kf::attn_plan(attn_problem(kf::ATTN_BATCH, c, n_head, n_kv, hd, 0, 1, 1, q, out, q_stride, out_stride, kv_stride));
    if (p.status != KF_OK) { /* as kf_attn_prefill_batch_strided; a q or out the tile kernel cannot read is an alignment refusal here */
        const bool unal = (((uintptr_t)q) & 15) || (((uintptr_t)out) & 7) || (q_stride & 7) || (out_stride & 3);
        return fail(unal ? KF_BLAS_UNALIGN : KF_INVALID_ARGS, "kf_attn_prefill_docs: shape not covered by the tile kernel (head_dim 64 / 128, n_head / n_kv in 1, 2, 4, 8, 16-byte aligned rows)");
    }
    if (!kf::attn_docs_header_ok(h, n_head, n_kv, hd)) return fail(KF_INVALID_ARGS, "kf_attn_prefill_docs: the table's header is not kf_attn_docs_plan's for %d / %d heads of %d", n_head, n_kv, hd);
    RET(kf::attn_prefill_docs_launch(c->stream, p, *h, d_table, q, k, v, out, q_stride, n_kv, kv_stride, out_stride));
}
size_t kf_attn_backward_docs_scratch_bytes(int n_rows, int n_head) { return kf::attn_backward_docs_scratch_bytes(n_rows, n_head); }
int kf_attn_backward_docs(kf_ctx* c, const kf_bf16* q, const kf_bf16* k, const kf_bf16* v, long long ld_qkv, const kf_bf16* o, const kf_bf16* dO, long long ld_o, kf_bf16* dq,
                          kf_bf16* dk, kf_bf16* dv, long long ld_d, const kf_attn_docs_header* h, const void* d_table, int n_head, int n_kv, int hd, void* scratch) {
    CHKCTX(c);
    if (!q || !k || !v || !o || !dO || !dq || !dk || !dv || !scratch || !h || !d_table || n_kv < 1 || n_head < 1 || n_head % n_kv)
        return fail(KF_INVALID_ARGS, "kf_attn_backward_docs: null pointer or n_head not a multiple of n_kv");
    if (!al16(q) || !al16(k) || !al16(v) || !al16(o) || !al16(dO) || !al16(dq) || !al16(dk) || !al16(dv) || (ld_qkv % 8) || (ld_o % 8) || (ld_d % 8) || ((uintptr_t)scratch & 3) ||
        !al16(d_table))
        return fail(KF_BLAS_UNALIGN, "kf_attn_backward_docs: rows and the table must be 16-byte aligned");
    if (ld_qkv < (long long)n_head * hd || ld_o < (long long)n_head * hd || ld_d < (long long)n_head * hd) return fail(KF_INVALID_ARGS, "kf_attn_backward_docs: row stride below n_head * head_dim");
    const kf::AttnPlan p = kf::attn_plan(attn_problem(kf::ATTN_BACKWARD, c, n_head, n_kv, hd, 0, 1, 1, q, dq, 0, 0, 0));
    if (p.status != KF_OK) return fail(p.status, "kf_attn_backward_docs: head_dim %d not covered (64, 128)", hd);
    if (!kf::attn_docs_header_ok(h, n_head, n_kv, hd)) return fail(KF_INVALID_ARGS, "kf_attn_backward_docs: the table's header is not kf_attn_docs_plan's for %d / %d heads of %d", n_head, n_kv, hd);
    RET(kf::attn_backward_docs_launch(c->stream, p, *h, d_table, q, k, v, ld_qkv, o, dO, ld_o, dq, dk, dv, ld_d, (float*)scratch));
}
int kf_qknorm_rope_train_pos(kf_ctx* c, kf_bf16* q, kf_bf16* k, const kf_bf16* wq, const kf_bf16* wk, const float* table, int n_tok, const int32_t* pos, int64_t q_stride,
                             int64_t k_stride, int n_head, int n_kv, int hd, float eps, float* rstd_q, float* rstd_k) {
    CHKCTX(c);
    if (!q || n_tok < 1 || !pos) return fail(KF_INVALID_ARGS, "kf_qknorm_rope_train_pos: bad args");
    if (hd % 2) return fail(KF_RMS_PARAMS, "head_dim %d is not divisible by 2", hd);
    RET(kf::qknorm_rope_pos_launch(c->stream, q, k, wq, wk, table, pos, n_head, n_kv, hd, eps, n_tok, q_stride, k_stride, rstd_q, rstd_k));
}
int kf_zero_ignored_rows(kf_ctx* c, kf_bf16* buf, int n_rows, int P, const int32_t* mask) {
    CHKCTX(c);
    if (!buf || !mask || n_rows < 1 || P < 8) return fail(KF_INVALID_ARGS, "kf_zero_ignored_rows: null pointer, n_rows < 1 or P < 8");
    if ((P % 8) != 0 || !al16(buf)) return fail(KF_BLAS_UNALIGN, "kf_zero_ignored_rows: rows must be 16-byte aligned (P = %d a multiple of 8)", P);
    RET(kf::zero_ignored_rows_launch(c->stream, buf, n_rows, P, mask));
}
int kf_embed_pos(kf_ctx* c, const kf_bf16* wte, long long ldw, const kf_bf16* wpe, const int32_t* tokens, int B, int T, int C, int V, kf_bf16* out) {
    CHKCTX(c);
    if (!wte || !wpe || !tokens || !out) return fail(KF_INVALID_ARGS, "kf_embed_pos: null pointer");
    if (!al16(wte) || !al16(wpe) || !al16(out)) return fail(KF_BLAS_UNALIGN, "kf_embed_pos: tensors must be 16-byte aligned");
    const int r = kf::embed_pos_launch(c->stream, wte, ldw, wpe, tokens, B, T, C, V, out);
    if (r == KF_INVALID_ARGS) return fail(r, "kf_embed_pos: needs B, T, V >= 1, C a multiple of 8, ldw >= C a multiple of 8 (got %d %d %d %d %lld)", B, T, C, V, ldw);
    RET(r);
}
int kf_argmax_rows_state(kf_ctx* c, const kf_bf16* logits, long long ld, int n, int n_rows, const int32_t* d_seq, int32_t* d_states, int32_t* d_tokens_out, int tokens_stride) {
    CHKCTX(c);
    if (!logits || !d_seq || !d_states) return fail(KF_INVALID_ARGS, "kf_argmax_rows_state: null pointer");
    const int r = kf::argmax_rows_state_launch(c->stream, logits, ld, n, n_rows, d_seq, d_states, d_tokens_out, tokens_stride);
    if (r == KF_INVALID_ARGS) return fail(r, "kf_argmax_rows_state: needs n, n_rows >= 1 and ld >= n");
    RET(r);
}
int kf_copy_blocks(kf_ctx* c, void* const* d_dst_table, size_t dst_offset, const void* src, size_t src_stride, size_t block_bytes, int n_blocks) {
    CHKCTX(c);
    if (!d_dst_table || !src) return fail(KF_INVALID_ARGS, "kf_copy_blocks: null pointer");
    if (!al16(src)) return fail(KF_BLAS_UNALIGN, "kf_copy_blocks: src must be 16-byte aligned");
    const int r = kf::copy_blocks_launch(c->stream, d_dst_table, dst_offset, src, src_stride, block_bytes, n_blocks);
    if (r == KF_INVALID_ARGS) return fail(r, "kf_copy_blocks: 1 .. 65535 blocks, sizes / strides / offset multiples of 16 bytes");
    RET(r);
}
int kf_memset2d(kf_ctx* c, void* p, size_t pitch, int value, size_t width, size_t rows) {
    CHKCTX(c);
    if (!p || width > pitch) return fail(KF_INVALID_ARGS, "kf_memset2d: null pointer or width > pitch");
    if (!width || !rows) return KF_OK;
    RET(hipMemset2DAsync(p, pitch, value, width, rows, c->stream) == hipSuccess ? KF_OK : KF_HIP_CHECK);
}
int kf_embed_backward(kf_ctx* c, kf_bf16* dwte, long long ldw, kf_bf16* dwpe, const kf_bf16* dout, const int32_t* tokens, int B, int T, int C, int V) {
    CHKCTX(c);
    if (!dout || !tokens || (!dwte && !dwpe)) return fail(KF_INVALID_ARGS, "kf_embed_backward: null pointer");
    if (!al16(dout) || (dwte && !al16(dwte)) || (dwpe && !al16(dwpe))) return fail(KF_BLAS_UNALIGN, "kf_embed_backward: tensors must be 16-byte aligned");
    const int r = kf::embed_backward_launch(c->stream, dwte, ldw, dwpe, dout, tokens, B, T, C, V);
    if (r == KF_INVALID_ARGS) return fail(r, "kf_embed_backward: needs B, T, V >= 1, C a multiple of 8 up to 8192, ldw >= C a multiple of 8 (got %d %d %d %d %lld)", B, T, C, V, ldw);
    RET(r);
}
size_t kf_norm_backward_scratch_bytes(int rows, int dim, int is_layernorm) {
    return sizeof(double) * (size_t)kf::norm_backward_groups(rows < 1 ? 1 : rows) * (is_layernorm ? 2 : 1) * (size_t)(dim < 0 ? 0 : dim);
}
int kf_norm_backward(kf_ctx* c, kf_bf16* dinp, kf_bf16* dweight, kf_bf16* dbias, const kf_bf16* dout, const kf_bf16* inp, const kf_bf16* weight, const float* mean,
                     const float* rstd, int rows, int dim, void* scratch) {
    CHKCTX(c);
    if (!dinp || !dweight || !dout || !inp || !weight || !rstd || !scratch) return fail(KF_INVALID_ARGS, "kf_norm_backward: null pointer");
    if (rows < 1 || dim < 8 || (dim % 8) != 0 || dim > 8192) return fail(KF_INVALID_ARGS, "kf_norm_backward: needs rows >= 1 and dim a multiple of 8 up to 8192 (got %d x %d)", rows, dim);
    if (!al16(dinp) || !al16(dout) || !al16(inp) || !al16(weight) || ((uintptr_t)scratch & 7)) return fail(KF_BLAS_UNALIGN, "kf_norm_backward: tensors must be 16-byte aligned");
    RET(kf::norm_backward_launch(c->stream, dinp, dweight, dbias, dout, inp, weight, mean, rstd, rows, dim, (double*)scratch));
}
int kf_rope_backward(kf_ctx* c, kf_bf16* d, const float* rope_table, int pos0, int n_tok, int seq_len, long long stride, int n_head, int hd) {
    CHKCTX(c);
    if (!d || !rope_table || pos0 < 0) return fail(KF_INVALID_ARGS, "kf_rope_backward: bad args");
    RET(kf::rope_backward_launch(c->stream, d, rope_table, pos0, n_tok, seq_len, stride, n_head, hd));
}
size_t kf_qknorm_rope_backward_scratch_bytes(int n_tok, int n_head, int n_kv, int hd) { return kf::qknorm_rope_backward_scratch_bytes(n_tok, n_head, n_kv, hd); }
// kf_qknorm_rope_backward (pos NULL: row t at t % seq_len) and kf_qknorm_rope_backward_pos (row t at pos[t]; seq_len is passed as 1): one set of refusals
static int qknorm_rope_backward_impl(kf_ctx* c, const kf_bf16* dq, const kf_bf16* dk, const kf_bf16* dv, long long ld_d, const kf_bf16* q_raw, long long ld_qraw, const kf_bf16* k_raw,
                                     long long ld_kraw, const kf_bf16* wq, const kf_bf16* wk, const float* rstd_q, const float* rstd_k, const float* table, int n_tok, int seq_len,
                                     const int32_t* pos, int n_head, int n_kv, int hd, kf_bf16* dq_raw, kf_bf16* dk_raw, kf_bf16* dv_out, kf_bf16* dwq, kf_bf16* dwk, void* scratch) {
    if (!dq || !dk || !q_raw || !k_raw || !wq || !wk || !rstd_q || !rstd_k || !table || !dq_raw || !dk_raw || !dwq || !dwk || !scratch || (!dv) != (!dv_out))
        return fail(KF_INVALID_ARGS, "kf_qknorm_rope_backward: null pointer (dv and dv_out go together)");
    if (n_tok < 1 || seq_len < 1 || n_tok % seq_len || n_head < 1 || n_kv < 1 || n_head % n_kv)
        return fail(KF_INVALID_ARGS, "kf_qknorm_rope_backward: needs n_tok >= 1 a multiple of seq_len and n_head a multiple of n_kv (got %d, %d, %d, %d)", n_tok, seq_len, n_head, n_kv);
    if (hd != 64 && hd != 128) return fail(KF_UNSUPPORTED_DATATYPE, "kf_qknorm_rope_backward: head_dim %d not covered (64, 128)", hd);
    if (ld_d < (long long)n_head * hd || ld_qraw < (long long)n_head * hd || ld_kraw < (long long)n_kv * hd || (ld_d % 8) || (ld_qraw % 8) || (ld_kraw % 8))
        return fail(KF_INVALID_ARGS, "kf_qknorm_rope_backward: a row stride is below its row or no multiple of 8 (%lld, %lld, %lld)", ld_d, ld_qraw, ld_kraw);
    if (!al16(dq) || !al16(dk) || (dv && !al16(dv)) || !al16(q_raw) || !al16(k_raw) || !al16(wq) || !al16(wk) || !al16(table) || !al16(dq_raw) || !al16(dk_raw) ||
        (dv_out && !al16(dv_out)) || ((uintptr_t)rstd_q & 3) || ((uintptr_t)rstd_k & 3) || ((uintptr_t)dwq & 1) || ((uintptr_t)dwk & 1) || ((uintptr_t)scratch & 7))
        return fail(KF_BLAS_UNALIGN, "kf_qknorm_rope_backward: tensors and the table must be 16-byte aligned, the scratch 8-byte aligned");
    RET(kf::qknorm_rope_backward_launch(c->stream, dq, dk, dv, ld_d, q_raw, ld_qraw, k_raw, ld_kraw, wq, wk, rstd_q, rstd_k, table, n_tok, seq_len, n_head, n_kv, hd, dq_raw, dk_raw,
                                        dv_out, dwq, dwk, (double*)scratch, pos));
}
int kf_qknorm_rope_backward(kf_ctx* c, const kf_bf16* dq, const kf_bf16* dk, const kf_bf16* dv, long long ld_d, const kf_bf16* q_raw, long long ld_qraw, const kf_bf16* k_raw,
                            long long ld_kraw, const kf_bf16* wq, const kf_bf16* wk, const float* rstd_q, const float* rstd_k, const float* table, int n_tok, int seq_len,
                            int n_head, int n_kv, int hd, kf_bf16* dq_raw, kf_bf16* dk_raw, kf_bf16* dv_out, kf_bf16* dwq, kf_bf16* dwk, void* scratch) {
    CHKCTX(c);
    return qknorm_rope_backward_impl(c, dq, dk, dv, ld_d, q_raw, ld_qraw, k_raw, ld_kraw, wq, wk, rstd_q, rstd_k, table, n_tok, seq_len, nullptr, n_head, n_kv, hd, dq_raw, dk_raw,
                                     dv_out, dwq, dwk, scratch);
}
int kf_qknorm_rope_backward_pos(kf_ctx* c, const kf_bf16* dq, const kf_bf16* dk, const kf_bf16* dv, long long ld_d, const kf_bf16* q_raw, long long ld_qraw, const kf_bf16* k_raw,
                                long long ld_kraw, const kf_bf16* wq, const kf_bf16* wk, const float* rstd_q, const float* rstd_k, const float* table, int n_tok,
                                const int32_t* pos, int n_head, int n_kv, int hd, kf_bf16* dq_raw, kf_bf16* dk_raw, kf_bf16* dv_out, kf_bf16* dwq, kf_bf16* dwk, void* scratch) {
    CHKCTX(c);
    if (!pos || ((uintptr_t)pos & 3)) return fail(KF_INVALID_ARGS, "kf_qknorm_rope_backward_pos: pos is null or not 4-byte aligned");
    return qknorm_rope_backward_impl(c, dq, dk, dv, ld_d, q_raw, ld_qraw, k_raw, ld_kraw, wq, wk, rstd_q, rstd_k, table, n_tok, 1, pos, n_head, n_kv, hd, dq_raw, dk_raw, dv_out,
                                     dwq, dwk, scratch);
}
int kf_gelu_backward(kf_ctx* c, kf_bf16* d_in_out, const kf_bf16* x, size_t n) {
    CHKCTX(c);
    if (!d_in_out || !x || n == 0) return fail(KF_INVALID_ARGS, "kf_gelu_backward: bad args");
    RET(kf::gelu_backward_launch(c->stream, d_in_out, x, n));
}
int kf_swiglu_backward(kf_ctx* c, kf_bf16* delta_in_out, kf_bf16* delta_gate, const kf_bf16* gate, const kf_bf16* up, size_t n) {
    CHKCTX(c);
    if (!delta_in_out || !delta_gate || !gate || !up || n == 0) return fail(KF_INVALID_ARGS, "kf_swiglu_backward: bad args");
    RET(kf::swiglu_backward_launch(c->stream, delta_in_out, delta_gate, gate, up, n));
}
int kf_fused_classifier(kf_ctx* c, kf_bf16* logits, float* losses, kf_bf16* probs, float dloss, const int32_t* targets, int B, int T, int V, int P,
                        const int32_t* mask, int write_dlogits) {
    CHKCTX(c);
    if (!logits || !losses || !targets) return fail(KF_INVALID_ARGS, "kf_fused_classifier: null pointer");
    if (B < 1 || T < 1 || V < 1 || P < V) return fail(KF_INVALID_ARGS, "kf_fused_classifier: needs B, T, V >= 1 and P >= V (got %d %d %d %d)", B, T, V, P);
    if ((P % 8) != 0 || !al16(logits) || (probs && !al16(probs)))
        return fail(KF_BLAS_UNALIGN, "kf_fused_classifier: rows must be 16-byte aligned (P = %d a multiple of 8, like the reference's padded vocabulary)", P);
    RET(kf::fused_classifier_launch(c->stream, logits, losses, probs, dloss, targets, (long)B * T, V, P, mask, write_dlogits));
}
int kf_distill_classifier(kf_ctx* c, kf_bf16* logits, const kf_bf16* teacher, int64_t teacher_ld, float* losses, float* kd, float dloss, const int32_t* targets, int B, int T,
                          int V, int P, const int32_t* mask, float ce_weight, float kd_weight, float temperature, int write_dlogits) {
    CHKCTX(c);
    if (!logits || !losses) return fail(KF_INVALID_ARGS, "kf_distill_classifier: null logits or losses");
    if (!isfinite(ce_weight) || !isfinite(kd_weight) || ce_weight < 0.0f || kd_weight < 0.0f || (ce_weight == 0.0f && kd_weight == 0.0f))
        return fail(KF_INVALID_ARGS, "kf_distill_classifier: ce_weight and kd_weight must be finite and >= 0, and not both zero (got %g, %g)", (double)ce_weight, (double)kd_weight);
    if (!isfinite(temperature) || !(temperature > 0.0f)) return fail(KF_INVALID_ARGS, "kf_distill_classifier: the temperature must be finite and > 0 (got %g)", (double)temperature);
    if (kd_weight != 0.0f && !teacher) return fail(KF_INVALID_ARGS, "kf_distill_classifier: kd_weight != 0 needs a teacher");
    if (ce_weight != 0.0f && !targets) return fail(KF_INVALID_ARGS, "kf_distill_classifier: ce_weight != 0 needs targets");
    if (B < 1 || T < 1 || V < 1 || P < V) return fail(KF_INVALID_ARGS, "kf_distill_classifier: needs B, T, V >= 1 and P >= V (got %d %d %d %d)", B, T, V, P);
    if (teacher && teacher_ld < V) return fail(KF_INVALID_ARGS, "kf_distill_classifier: teacher_ld %lld is below V = %d", (long long)teacher_ld, V);
    if ((P % 8) != 0 || !al16(logits) || (teacher && ((teacher_ld % 8) != 0 || !al16(teacher))))
        return fail(KF_BLAS_UNALIGN, "kf_distill_classifier: rows must be 16-byte aligned (P = %d and teacher_ld = %lld multiples of 8)", P, (long long)teacher_ld);
    if (teacher) { /* the rows' own extents: the last row ends at its V-th element */
        const long long rows = (long long)B * T;
        const uintptr_t z0 = (uintptr_t)logits, z1 = z0 + (size_t)((rows - 1) * P + V) * 2, u0 = (uintptr_t)teacher, u1 = u0 + (size_t)((rows - 1) * teacher_ld + V) * 2;
        if (z0 < u1 && u0 < z1) return fail(KF_INVALID_ARGS, "kf_distill_classifier: the teacher's rows overlap the logits");
    }
    RET(kf::distill_classifier_launch(c->stream, logits, teacher, (long)teacher_ld, losses, kd, dloss, targets, (long)B * T, V, P, mask, ce_weight, kd_weight, temperature,
                                      write_dlogits));
}
int kf_adamw(kf_ctx* c, kf_bf16* params, kf_bf16* grads, void* gm, void* gv, size_t n, int mv_type, float learning_rate, float beta1, float beta2,
             float beta1_correction, float beta2_correction, float eps, float weight_decay, float grad_scale, uint32_t seed, int32_t* d_status) {
    CHKCTX(c);
    if (!params || !grads || !gm || !gv) return fail(KF_INVALID_ARGS, "kf_adamw: null pointer");
    if (mv_type != KF_BF16 && mv_type != KF_F32) return fail(KF_UNSUPPORTED_DATATYPE, "kf_adamw: moments must be bf16 or f32 (got %d)", mv_type);
    if (n == 0 || n % 8) return fail(KF_INVALID_ARGS, "kf_adamw: n = %zu is not a positive multiple of 8 (TASKA_1p1 asserts N %% typ128::size == 0)", n);
    if (!al16(params) || !al16(grads) || !al16(gm) || !al16(gv)) return fail(KF_BLAS_UNALIGN, "kf_adamw: tensors must be 16-byte aligned");
    RET(kf::adamw_launch(c->stream, params, grads, gm, gv, n, mv_type == KF_BF16, learning_rate, beta1, beta2, beta1_correction, beta2_correction, eps,
                         weight_decay, grad_scale, seed, d_status));
}
int kf_adamw_scaled(kf_ctx* c, kf_bf16* params, kf_bf16* grads, void* gm, void* gv, size_t n, int mv_type, float learning_rate, float beta1, float beta2,
                    float beta1_correction, float beta2_correction, float eps, float weight_decay, const float* d_grad_scale, uint32_t seed, int32_t* d_status) {
    CHKCTX(c);
    if (!params || !grads || !gm || !gv || !d_grad_scale) return fail(KF_INVALID_ARGS, "kf_adamw_scaled: null pointer");
    if (mv_type != KF_BF16 && mv_type != KF_F32) return fail(KF_UNSUPPORTED_DATATYPE, "kf_adamw_scaled: moments must be bf16 or f32 (got %d)", mv_type);
    if (n == 0 || n % 8) return fail(KF_INVALID_ARGS, "kf_adamw_scaled: n = %zu is not a positive multiple of 8", n);
    if (!al16(params) || !al16(grads) || !al16(gm) || !al16(gv) || (((uintptr_t)d_grad_scale) & 3)) return fail(KF_BLAS_UNALIGN, "kf_adamw_scaled: tensors must be 16-byte aligned, the scale 4-byte");
    RET(kf::adamw_launch(c->stream, params, grads, gm, gv, n, mv_type == KF_BF16, learning_rate, beta1, beta2, beta1_correction, beta2_correction, eps,
                         weight_decay, 1.0f, seed, d_status, d_grad_scale));
}

// ---- gradient norms (kf_gradnorm.hip): every launch figure is kf::gradnorm_plan's
size_t kf_grad_norms_scratch_bytes(int n_tensors, const long long* n) {
    const kf::GradNormPlan p = kf::gradnorm_plan(n_tensors, n);
    return p.status == KF_OK ? p.bytes : 0;
}
int kf_grad_norms_plan(kf_ctx* c, int n_tensors, const kf_bf16* const* grads, const long long* n, const uint8_t* no_clip, void* scratch, size_t scratch_bytes) {
    CHKCTX(c);
    if (n_tensors < 1 || n_tensors > kf::GN_MAX_TENSORS) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: n_tensors = %d outside [1, %d]", n_tensors, kf::GN_MAX_TENSORS);
    if (!grads || !n) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: null pointer");
    kf::GradNormPlan p = kf::gradnorm_plan(n_tensors, n);
    if (p.status != KF_OK) {
        if (p.bad >= 0 && (n[p.bad] < 8 || (n[p.bad] & 7))) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: n[%d] = %lld is not a positive multiple of 8", p.bad, n[p.bad]);
        return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: the list is too long (tensor %d: more than 2^40 elements, or more than 2^31 - 1 chunks in all)", p.bad);
    }
    for (int i = 0; i < n_tensors; i++) {
        if (!grads[i]) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: grads[%d] is null", i);
        if (!al16(grads[i])) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: grads[%d] is not 16-byte aligned", i);
    }
    if (!scratch || (((uintptr_t)scratch) & 255)) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: scratch is missing or not 256-byte aligned");
    if (scratch_bytes < p.bytes) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: scratch of %zu bytes, kf_grad_norms_scratch_bytes = %zu", scratch_bytes, p.bytes);
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_grad_norms_plan: not inside a graph capture (it copies the table with a blocking copy)");
    std::vector<kf::GradNormEntry> tab((size_t)n_tensors + 1);
    std::vector<int> wg0((size_t)n_tensors + 1);
    kf::gradnorm_wg0(n_tensors, n, wg0.data());
    for (int i = 0; i <= n_tensors; i++) {
        kf::GradNormEntry& e = tab[i];
        memset(&e, 0, sizeof(e));
        e.wg0 = wg0[i];
        if (i < n_tensors) e.g = (const uint16_t*)grads[i], e.n = n[i], e.no_clip = no_clip && no_clip[i];
    }
    static std::mutex mu;
    static unsigned long long counter = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        p.stamp = kf::GN_STAMP0 + ++counter;
    }
    tab[n_tensors].n = (long long)p.stamp;
    // every remembered layout whose bytes this scratch overlaps is forgotten first (the same scratch planned again, or memory that was freed and handed out anew),
    // so that a failed copy leaves no stale layout behind
    for (size_t k = c->gn_plans.size(); k-- > 0;) {
        const char *a0 = (const char*)c->gn_plans[k].scratch, *a1 = a0 + c->gn_plans[k].plan.bytes, *b0 = (const char*)scratch, *b1 = b0 + p.bytes;
        if (a0 < b1 && b0 < a1) c->gn_plans.erase(c->gn_plans.begin() + k);
    }
    HIPCHK(hipMemcpyAsync((char*)scratch + p.off_table, tab.data(), sizeof(kf::GradNormEntry) * tab.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->gn_plans.push_back(kf_ctx::GradNormSlot{scratch, p});
    return KF_OK;
}
int kf_grad_norms_forget(kf_ctx* c, const void* scratch) {
    CHKCTX(c);
    for (size_t k = c->gn_plans.size(); k-- > 0;)
        if (c->gn_plans[k].scratch == scratch) c->gn_plans.erase(c->gn_plans.begin() + k);
    return KF_OK;
}
int kf_grad_norms(kf_ctx* c, const void* scratch, int n_tensors, int mode, float gclip, double* d_sumsq, float* d_gnorm, float* d_scale) {
    CHKCTX(c);
    if (!scratch || !d_sumsq || !d_gnorm || !d_scale) return fail(KF_INVALID_ARGS, "kf_grad_norms: null pointer");
    if (n_tensors < 1) return fail(KF_INVALID_ARGS, "kf_grad_norms: n_tensors = %d", n_tensors);
    if (((uintptr_t)scratch) & 255) return fail(KF_INVALID_ARGS, "kf_grad_norms: scratch is not 256-byte aligned");
    if ((((uintptr_t)d_sumsq) & 7) || (((uintptr_t)d_gnorm) & 3) || (((uintptr_t)d_scale) & 3)) return fail(KF_INVALID_ARGS, "kf_grad_norms: a misaligned output (fp64 sums 8-byte, floats 4-byte)");
    if (mode != KF_CLIP_REPORT && mode != KF_CLIP_TENSOR && mode != KF_CLIP_GLOBAL) return fail(KF_INVALID_ARGS, "kf_grad_norms: unknown mode %d", mode);
    if (mode != KF_CLIP_REPORT && !(isfinite(gclip) && gclip > 0.0f)) return fail(KF_INVALID_ARGS, "kf_grad_norms: gclip = %g must be finite and > 0 in a clipping mode", (double)gclip);
    const kf::GradNormPlan* p = nullptr;
    for (const kf_ctx::GradNormSlot& s : c->gn_plans)
        if (s.scratch == scratch) p = &s.plan;
    if (!p) return fail(KF_INVALID_ARGS, "kf_grad_norms: this scratch holds no table of this context (kf_grad_norms_plan first)");
    if (p->n_tensors != n_tensors) return fail(KF_INVALID_ARGS, "kf_grad_norms: n_tensors = %d, the scratch was planned for %d", n_tensors, p->n_tensors);
    RET(kf::grad_norms_launch(c->stream, scratch, *p, mode, gclip, d_sumsq, d_gnorm, d_scale));
}

// ---- Muon (PIPE_Muon::CU_core, Optimizer.cu:498-583): kf_muon.hip
static bool muon_dims_ok(int ne0, int ne1) { return ne1 >= 64 && ne0 >= ne1 && !(ne0 % 64) && !(ne1 % 64); }
static int muon_scratch_ok(const char* who, int ne0, int ne1, const void* scratch, size_t scratch_bytes) {
    if (!scratch || (((uintptr_t)scratch) & 255)) return fail(KF_INVALID_ARGS, "%s: scratch is missing or not 256-byte aligned", who);
    const size_t need = kf::muon_layout(ne0, ne1).bytes;
    if (scratch_bytes < need) return fail(KF_INVALID_ARGS, "%s: scratch of %zu bytes, kf_muon_scratch_bytes(%d, %d) = %zu", who, scratch_bytes, ne0, ne1, need);
    return KF_OK;
}
size_t kf_muon_scratch_bytes(int ne0, int ne1) { return muon_dims_ok(ne0, ne1) ? kf::muon_layout(ne0, ne1).bytes : 0; }
int kf_muon_momentum(kf_ctx* c, kf_bf16* mG, const kf_bf16* grads, kf_bf16* X, size_t n, float mui, uint32_t seed, double* d_sumsq) {
    CHKCTX(c);
    if (!mG || !grads || !X || !d_sumsq) return fail(KF_INVALID_ARGS, "kf_muon_momentum: null pointer");
    if (n == 0 || n % 8 || n > (size_t)kf::KF_MUON_MAX_PARTIALS * 4096) return fail(KF_INVALID_ARGS, "kf_muon_momentum: n = %zu is not a multiple of 8 in (0, 2^28]", n);
    if (!al16(mG) || !al16(grads) || !al16(X) || (((uintptr_t)d_sumsq) & 7)) return fail(KF_INVALID_ARGS, "kf_muon_momentum: tensors must be 16-byte aligned");
    RET(kf::muon_momentum_launch(c->stream, mG, grads, X, n, mui, seed, c->muon_part, d_sumsq));
}
int kf_muon_apply(kf_ctx* c, kf_bf16* params, kf_bf16* grads, const kf_bf16* X, size_t n, float lr, float weight_decay, uint32_t seed, double* d_wnormsq) {
    CHKCTX(c);
    if (!params || !grads || !X) return fail(KF_INVALID_ARGS, "kf_muon_apply: null pointer");
    if (n == 0 || n % 8 || n > (size_t)kf::KF_MUON_MAX_PARTIALS * 4096) return fail(KF_INVALID_ARGS, "kf_muon_apply: n = %zu is not a multiple of 8 in (0, 2^28]", n);
    if (!al16(params) || !al16(grads) || !al16(X) || (((uintptr_t)d_wnormsq) & 7)) return fail(KF_INVALID_ARGS, "kf_muon_apply: tensors must be 16-byte aligned");
    RET(kf::muon_apply_launch(c->stream, params, grads, X, n, lr, weight_decay, seed, c->muon_part, d_wnormsq));
}
int kf_newton_schulz(kf_ctx* c, kf_bf16* X, int ne0, int ne1, const double* d_sumsq, float eps_muon, int n_iter, float a, float b, float cc, void* scratch, size_t scratch_bytes) {
    CHKCTX(c);
    if (!X || !al16(X) || (((uintptr_t)d_sumsq) & 7)) return fail(KF_INVALID_ARGS, "kf_newton_schulz: X is null or not 16-byte aligned");
    if (!muon_dims_ok(ne0, ne1)) return fail(KF_INVALID_ARGS, "kf_newton_schulz: needs ne0 >= ne1, both multiples of 64 (got %d x %d)", ne0, ne1);
    if (n_iter < 0 || n_iter > 16) return fail(KF_INVALID_ARGS, "kf_newton_schulz: n_iter = %d outside [0, 16]", n_iter);
    const int r = muon_scratch_ok("kf_newton_schulz", ne0, ne1, scratch, scratch_bytes);
    if (r) return r;
    RET(kf::newton_schulz_launch(c->stream, X, ne0, ne1, d_sumsq, eps_muon, n_iter, a, b, cc, scratch));
}
int kf_muon(kf_ctx* c, kf_bf16* params, kf_bf16* grads, kf_bf16* mG, int ne0, int ne1, float lr, float weight_decay, float mui, float eps_muon, int n_iter, uint32_t seed,
            void* scratch, size_t scratch_bytes, double* d_wnormsq) {
    CHKCTX(c);
    if (!params || !grads || !mG || !al16(params) || !al16(grads) || !al16(mG) || (((uintptr_t)d_wnormsq) & 7)) return fail(KF_INVALID_ARGS, "kf_muon: a tensor is null or not 16-byte aligned");
    if (!muon_dims_ok(ne0, ne1)) return fail(KF_INVALID_ARGS, "kf_muon: needs ne0 >= ne1, both multiples of 64 (got %d x %d)", ne0, ne1);
    if (n_iter < 0 || n_iter > 16) return fail(KF_INVALID_ARGS, "kf_muon: n_iter = %d outside [0, 16]", n_iter);
    int r = muon_scratch_ok("kf_muon", ne0, ne1, scratch, scratch_bytes);
    if (r) return r;
    const kf::MuonLayout L = kf::muon_layout(ne0, ne1);
    char* const sc = (char*)scratch;
    uint16_t* const X = (uint16_t*)(sc + L.X0);
    double *const part = (double*)(sc + L.part), *const dbl = (double*)(sc + L.dbl);
    const size_t n = (size_t)ne0 * ne1;
    if ((r = kf::muon_momentum_launch(c->stream, mG, grads, X, n, mui, seed, part, dbl)) != KF_OK) return fail(r, "kf_muon: momentum failed with %d", r);
    if ((r = kf::newton_schulz_launch(c->stream, X, ne0, ne1, dbl, eps_muon, n_iter, 3.4445f, -4.7750f, 2.0315f, scratch)) != KF_OK) return fail(r, "kf_muon: Newton-Schulz failed with %d", r);
    RET(kf::muon_apply_launch(c->stream, params, grads, X, n, lr, weight_decay, seed, part, d_wnormsq ? d_wnormsq : dbl + 1));
}

// ---- EOE (Fuyou::Exploitation, Optimizer.cu:439-484): kf_evo.hip
int kf_evolve(kf_ctx* c, kf_bf16* x, const kf_bf16* head, int ne0, int ne1, int algorithm, float alpha, float social, float t_cross, uint32_t seed) {
    CHKCTX(c);
    if (!x || !head) return fail(KF_INVALID_ARGS, "kf_evolve: null pointer");
    if (ne0 < 1 || ne1 < 1) return fail(KF_INVALID_ARGS, "kf_evolve: shape %d x %d", ne0, ne1);
    const unsigned long long n = (unsigned long long)ne0 * (unsigned long long)ne1;
    if (n < 8 || n % 8 || n >= (1ull << 32)) return fail(KF_INVALID_ARGS, "kf_evolve: n = %llu is not a multiple of 8 in [8, 2^32)", n);
    const uintptr_t xa = (uintptr_t)x, ha = (uintptr_t)head;
    if (xa < ha + 2 * n && ha < xa + 2 * n) return fail(KF_INVALID_ARGS, "kf_evolve: x and head %s", xa == ha ? "are the same tensor" : "overlap");
    if (!al16(x) || !al16(head)) return fail(KF_INVALID_ARGS, "kf_evolve: tensors must be 16-byte aligned");
    if (algorithm != KF_EVO_PSO && algorithm != KF_EVO_PSO_GA && algorithm != KF_EVO_MIX)
        return fail(KF_INVALID_ARGS, "kf_evolve: unknown algorithm %d (KF_EVO_PSO = 1, KF_EVO_MIX = 2, KF_EVO_PSO_GA = 4)", algorithm);
    if (!isfinite(social) || !isfinite(alpha) || !isfinite(t_cross)) return fail(KF_INVALID_ARGS, "kf_evolve: social, alpha or t_cross is not finite");
    const double th = floor((double)t_cross * 256.0 + 0.5);
    const unsigned thr = th < 0.0 ? 0u : (th > 256.0 ? 256u : (unsigned)th);
    RET(kf::evolve_launch(c->stream, x, head, (size_t)n, algorithm, alpha, (float)(1.0 - (double)alpha), social, thr, seed));
}
int kf_loss_mean(kf_ctx* c, float* acc, const float* losses, size_t n, int index, int count) {
    CHKCTX(c);
    if (!acc || !losses || acc == losses) return fail(KF_INVALID_ARGS, "kf_loss_mean: acc / losses null or the same buffer");
    if (n == 0 || n >= ((size_t)1 << 31) || count < 1 || index < 0 || index >= count) return fail(KF_INVALID_ARGS, "kf_loss_mean: n = %zu, index %d of %d", n, index, count);
    RET(kf::loss_mean_launch(c->stream, acc, losses, n, index, count));
}

// ---- the decode engines (kf_engine_*, kf_xengine_*, kfdbg_*engine*).  What the entries share, stated once.  The opening: the context, then the handles the entry cannot do
// without (`what` names them: "engine" / "argument"), then, where the entry changes what a captured launch holds, ENG_NOT_CAPTURING.  The tails: ENG_HIP for a call that
// can only fail in HIP, ok_or for one fixed refusal text, ENG_WRAP for a create (the refusal, or the host object h wrapped into *out), eng_served for the *_served answers.
#define ENG_ENTER(c, ok, what) \
    CHKCTX(c);                 \
    if (!(ok)) return fail(KF_INVALID_ARGS, "%s: null " what, __func__)
#define ENG_NOT_CAPTURING(c) \
    if ((c)->capturing) return fail(KF_INVALID_ARGS, "%s: not while capturing", __func__)
#define ENG_HIP(expr) \
    if (const int rc_ = (expr)) return fail(rc_, "%s: HIP failure", __func__)
#define ENG_WRAP(E, rc, why, h, out) ((rc) != KF_OK ? fail(rc, "%s: %s", __func__, why) : (*(out) = new E{h}, KF_OK))
static int ok_or(int rc, const char* refusal) { return rc == KF_OK ? KF_OK : fail(rc, "%s", refusal); }
struct kf_engine {
    kf::EngineHost* h;
};
struct kf_xengine {
    kf::XEngineHost* h;
};
static int eng_served(int rc, const char* fn, const char* w, char* why, size_t why_bytes) {
    if (why && why_bytes > 0) snprintf(why, why_bytes, "%s", w);
    if (rc == KF_OK) return KF_OK;
    return rc == KF_UNSUPPORTED_DATATYPE ? KF_ENGINE_NOT_SERVED : fail(rc, "%s: %s", fn, w);
}

// ---- persistent decode engine
size_t kf_engine_workspace_bytes(const kf_engine_desc* d) { return d ? kf::engine_ws_bytes(d) : 0; }
int kf_engine_create(kf_ctx* c, const kf_engine_desc* d, void* ws, size_t ws_bytes, kf_engine** out) {
    ENG_ENTER(c, d && ws && out, "argument");
    ENG_NOT_CAPTURING(c);
    kf::EngineHost* h = nullptr;
    const char* why = "";
    const int rc = kf::engine_build(d, ws, ws_bytes, c->stream, &h, &why);
    return ENG_WRAP(kf_engine, rc, why, h, out);
}
int kf_engine_step(kf_ctx* c, kf_engine* e, const kf_bf16* x_in, kf_bf16* x_out, const int32_t* d_state, int pos_bound) {
    ENG_ENTER(c, e && e->h, "engine");
    kf::engine_set_canonical(e->h, c->canonical);
    const int rc = kf::engine_step(e->h, c->stream, x_in, x_out, d_state, pos_bound);
    return rc < 0 ? fail(rc, "kf_engine_step failed with %d", rc) : rc;
}
int kf_engine_step_head(kf_ctx* c, kf_engine* e, const kf_bf16* x_in, kf_bf16* x_out, int32_t* d_state, int pos_bound, int pick) {
    ENG_ENTER(c, e && e->h, "engine");
    kf::engine_set_canonical(e->h, c->canonical);
    const int rc = kf::engine_step(e->h, c->stream, x_in, x_out, d_state, pos_bound, pick ? 2 : 1);
    return rc < 0 ? fail(rc, "kf_engine_step_head failed with %d (no head set?)", rc) : rc;
}
int kf_engine_steps_head(kf_ctx* c, kf_engine* e, kf_bf16* x_out, int32_t* d_state, int pos_bound, int n_steps) {
    ENG_ENTER(c, e && e->h, "engine");
    if (n_steps < 1) return fail(KF_INVALID_ARGS, "kf_engine_steps_head: n_steps %d", n_steps);
    kf::engine_set_canonical(e->h, c->canonical);
    const int rc = kf::engine_step(e->h, c->stream, nullptr, x_out, d_state, pos_bound, 2, n_steps);
    return rc < 0 ? fail(rc, "kf_engine_steps_head failed with %d (no head / embedding set?)", rc) : rc;
}
int kf_engine_set_head(kf_ctx* c, kf_engine* e, const kf_weight* head_or_null, const kf_bf16* final_norm_w, kf_bf16* logits, int32_t* d_tokens_out) {
    ENG_ENTER(c, e && e->h, "engine");
    ENG_NOT_CAPTURING(c);
    return ok_or(kf::engine_set_head(e->h, head_or_null, final_norm_w, logits, d_tokens_out),
                 "kf_engine_set_head: the in-launch head takes a bf16 [vocab, dim] matrix of the engine's width, a norm weight and a logits buffer");
}
size_t kf_engine_head_screen_bytes(int vocab, int dim) { return kf::head_screen_bytes(vocab, dim); }
int kf_engine_set_head_screen(kf_ctx* c, kf_engine* e, void* buf, size_t bytes) {
    ENG_ENTER(c, e && e->h, "engine");
    ENG_NOT_CAPTURING(c);
    return ok_or(kf::engine_set_head_screen(e->h, buf, bytes, c->stream),
                 "kf_engine_set_head_screen: needs a head set by kf_engine_set_head and a 256-byte aligned buffer of kf_engine_head_screen_bytes(vocab, dim) bytes");
}
int kf_engine_screen_stats(kf_ctx* c, kf_engine* e, kf_engine_screen_statistics* out) {
    ENG_ENTER(c, e && e->h && out, "argument");
    long long w[3];
    ENG_HIP(kf::engine_screen_stats(e->h, c->stream, w));
    out->screened_steps = w[0], out->rows_reranked = w[1], out->wg_fallbacks = w[2];
    return KF_OK;
}
int kf_engine_reset(kf_ctx* c, kf_engine* e) {
    ENG_ENTER(c, e && e->h, "engine");
    ENG_NOT_CAPTURING(c);
    ENG_HIP(kf::eng_then_sync(KF_OK, c->stream));
    ENG_HIP(kf::engine_reset(e->h, c->stream));
    return KF_OK;
}
int kf_engine_set_embedding(kf_ctx* c, kf_engine* e, const kf_weight* embed_or_null, const int32_t* d_forced) {
    ENG_ENTER(c, e && e->h, "engine");
    ENG_NOT_CAPTURING(c);
    return ok_or(kf::engine_set_embedding(e->h, embed_or_null, d_forced),
                 "kf_engine_set_embedding: the fused row read takes a bf16 table of the engine's width (other storages keep kf_embed_state)");
}
int kf_engine_served(kf_ctx* c, const kf_engine_desc* d, char* why, size_t why_bytes) {
    CHKCTX(c);
    const char* w = "";
    const int rc = kf::engine_build(d, nullptr, 0, c->stream, nullptr, &w, kf::ENG_DRY);
    return eng_served(rc, __func__, w, why, why_bytes);
}
int kf_engine_tune(kf_ctx* c, kf_engine* e, kf_bf16* x_out, const int32_t* d_state, int pos_bound, int passes, float* us_before, float* us_after) {
    ENG_ENTER(c, e && e->h, "engine");
    ENG_NOT_CAPTURING(c);
    kf::engine_set_canonical(e->h, c->canonical);
    const int rc = kf::engine_tune(e->h, c->stream, x_out, d_state, pos_bound, passes, us_before, us_after);
    return rc < 0 ? fail(rc, "kf_engine_tune failed with %d (no embedding table set, or a poll timed out)", rc) : rc;
}
int kf_engine_stats(kf_ctx* c, kf_engine* e, int pos_bound, kf_engine_statistics* out) {
    ENG_ENTER(c, e && e->h && out, "argument");
    int w[14];
    ENG_HIP(kf::engine_stats(e->h, c->stream, pos_bound, w));
    for (int i = 0; i < 6; i++) out->sweeps[i] = w[i], out->delay[i] = w[7 + i];
    out->polls = w[6], out->tuned = w[13];
    return KF_OK;
}
int kf_engine_check(kf_ctx* c, kf_engine* e) {
    ENG_ENTER(c, e && e->h, "engine");
    int err = 0;
    ENG_HIP(kf::engine_error_word(e->h, c->stream, &err));
    if (err & 128) /* kf_attn_common.h, KF_CANON_FIX_LIM: an arithmetic flag of the canonical attention, no hand-off failed */
        return fail(KF_INTERNAL_ERR, "kf_engine: attention scores outside the engine's fixed-exponent range (error word 0x%x): the per-layer launches serve such a model (set_engine(False))", err);
    if (err) return fail(KF_INTERNAL_ERR, "kf_engine: a hand-off poll timed out (error word 0x%x): the launch was not fully resident", err);
    return KF_OK;
}
// ---- XCD-confined decode engines (kf_xengine.hip)
size_t kf_xengine_workspace_bytes(const kf_engine_desc* d) { return d ? kf::xengine_ws_bytes(d) : 0; }
int kf_xengine_create(kf_ctx* c, const kf_engine_desc* d, int n_seq, int64_t kv_seq_stride, void* ws, size_t ws_bytes, kf_xengine** out) {
    ENG_ENTER(c, d && ws && out, "argument");
    ENG_NOT_CAPTURING(c);
    if (n_seq < 1 || n_seq > KF_XENGINE_MAX_SEQ) return fail(KF_INVALID_ARGS, "kf_xengine_create: n_seq %d outside 1 .. %d (up to four sequences per XCD)", n_seq, KF_XENGINE_MAX_SEQ);
    kf::XEngineHost* h = nullptr;
    const char* why = "";
    const int rc = kf::xengine_build(d, n_seq, (long long)kv_seq_stride, ws, ws_bytes, c->stream, &h, &why);
    return ENG_WRAP(kf_xengine, rc, why, h, out);
}
size_t kf_xengine_workspace_bytes_tp(const kf_engine_desc* d) { return d ? kf::xengine_ws_bytes_tp(d) : 0; }
int kf_xengine_create_tp(kf_ctx* c, const kf_engine_desc* const* ds, int world, void* ws, size_t ws_bytes, kf_xengine** out) {
    ENG_ENTER(c, ds && ws && out, "argument");
    ENG_NOT_CAPTURING(c);
    kf::XEngineHost* h = nullptr;
    const char* why = "";
    const int rc = kf::xengine_build_tp(ds, world, ws, ws_bytes, c->stream, &h, &why);
    return ENG_WRAP(kf_xengine, rc, why, h, out);
}
int kf_xengine_set_head_tp(kf_ctx* c, kf_xengine* e, const kf_weight* const* shards, const int32_t* row0, const kf_bf16* final_norm_w, kf_bf16* logits, int32_t* d_tokens_out, int tokens_stride) {
    ENG_ENTER(c, e && e->h, "engine");
    return ok_or(kf::xengine_set_head_tp(e->h, shards, row0, final_norm_w, logits, d_tokens_out, tokens_stride),
                 "kf_xengine_set_head_tp: eight bf16 [rows, dim] vocabulary shards in rank order (row0 = the rows before), a norm weight and a logits buffer");
}
int kf_xengine_served(kf_ctx* c, const kf_engine_desc* d, char* why, size_t why_bytes) {
    CHKCTX(c);
    if (!d) return fail(KF_INVALID_ARGS, "kf_xengine_served: null descriptor");
    const char* w = "";
    const int rc = kf::xengine_build(d, 1, 0, nullptr, 0, c->stream, nullptr, &w, kf::ENG_DRY);
    return eng_served(rc, __func__, w, why, why_bytes);
}
int kf_xengine_set_embedding(kf_ctx* c, kf_xengine* e, const kf_weight* embed, const int32_t* d_forced, int forced_stride) {
    ENG_ENTER(c, e && e->h && embed, "argument");
    if (d_forced && forced_stride < 1) return fail(KF_INVALID_ARGS, "kf_xengine_set_embedding: forced_stride %d", forced_stride);
    return ok_or(kf::xengine_set_embedding(e->h, embed, d_forced, forced_stride), "kf_xengine_set_embedding: the row read inside the launch takes a bf16 table of the engine's width");
}
int kf_xengine_set_head(kf_ctx* c, kf_xengine* e, const kf_weight* head_or_null, const kf_bf16* final_norm_w, kf_bf16* logits, int32_t* d_tokens_out, int tokens_stride) {
    ENG_ENTER(c, e && e->h, "engine");
    return ok_or(kf::xengine_set_head(e->h, head_or_null, final_norm_w, logits, d_tokens_out, tokens_stride),
                 "kf_xengine_set_head: the in-launch head takes a bf16 [vocab, dim] matrix of the engine's width, a norm weight and a logits buffer");
}
int kf_xengine_steps(kf_ctx* c, kf_xengine* e, kf_bf16* x_out, int32_t* d_state, int n_steps, int pick) {
    ENG_ENTER(c, e && e->h, "engine");
    if (!c->canonical) return fail(KF_UNSUPPORTED_DATATYPE, "kf_xengine_steps: the XCD-confined engines run the canonical summation order only (kf_set_canonical(ctx, 1))");
    if (n_steps < 1 || (n_steps > 1 && !pick)) return fail(KF_INVALID_ARGS, "kf_xengine_steps: n_steps %d (several steps per launch need the pick inside)", n_steps);
    if (c->capturing) return fail(KF_INVALID_ARGS, "kf_xengine_steps: not while capturing (the launch's generation is a kernel argument the host counts: a replayed launch would repeat it)");
    const int rc = kf::xengine_steps(e->h, c->stream, d_state, x_out, pick ? 2 : 1, n_steps);
    if (rc == KF_UNSUPPORTED_DATATYPE) return fail(rc, "kf_xengine_steps: the form for this many sequences does not fit the LDS at this depth");
    return rc == KF_OK ? KF_OK : fail(rc, "kf_xengine_steps failed with %d (no embedding / head set?)", rc);
}
int kf_xengine_check(kf_ctx* c, kf_xengine* e) {
    ENG_ENTER(c, e && e->h, "engine");
    int err = 0;
    ENG_HIP(kf::xengine_error_word(e->h, c->stream, &err));
    if (err) return fail(KF_INTERNAL_ERR, "kf_xengine: error word 0x%x (8: an XCD did not get 32 workgroups; 64: a position beyond the cache rows (TP form); others: a hand-off poll timed out -- the launch was not fully resident)", err);
    return KF_OK;
}
int kf_xengine_reset(kf_ctx* c, kf_xengine* e) {
    ENG_ENTER(c, e && e->h, "engine");
    ENG_NOT_CAPTURING(c);
    ENG_HIP(kf::eng_then_sync(KF_OK, c->stream));
    ENG_HIP(kf::xengine_reset(e->h, c->stream));
    return KF_OK;
}
int kf_xengine_destroy(kf_xengine* e) {
    if (e) kf::xengine_free(e->h);
    delete e;
    return KF_OK;
}
// ---- diagnostics (NOT part of the ABI header; tests and scratch/ only): -1 = no engine / refused
#define ENG_DBG(e, call) ((e) && (e)->h ? (call) : -1)
int kfdbg_xengine_variant(kf_xengine* e, int nwv, int depth) { return ENG_DBG(e, kf::xengine_set_variant(e->h, nwv, depth)); }
// the form the engines pick (kf::xengine_form, no HIP call) for a shape class (1 Qwen3-0.6B, 2 the 256-wide test shape, 3 1.7B, 4 4B, 5 8B, 6 the 8-on-1 test shape, 7 / 8 / 9
// the TP ranks of 32B / 8B / 4B), a storage (kf::FMT_Q4P / FMT_Q1T / FMT_Q2T) and the hooks: out[5] = waves, ring depth, decoders per XCD, sequences per decoder, stamps;
// -1: refused
int kfdbg_xengine_form(int shape_class, int fmt, int n_seq, int n_layer, int stamps, int two_wpc, int* out) {
    const kf::XForm* f = kf::xengine_form(shape_class, fmt, n_seq, n_layer, stamps != 0, two_wpc != 0);
    if (!f || !out) return -1;
    out[0] = f->nwv, out[1] = f->depth, out[2] = f->wpc, out[3] = f->nb, out[4] = f->dbg;
    return 0;
}
// the form the persistent engine picks (kf::engine_form, no HIP call) for a shape class (1 Qwen3-0.6B, 2 the 256-wide test shape, 3 1.7B), a storage (kf::FMT_Q4P /
// FMT_Q1T / FMT_Q2T), an order and the stamps: out[5] = shape class, storage, canonical, stamps, launch LDS in bytes; -1: refused
int kfdbg_engine_form(int shape_class, int fmt, int canon, int stamps, int n_layer, int* out) {
    const kf::EngForm* f = kf::engine_form(shape_class, fmt, canon != 0, stamps != 0, n_layer);
    if (!f || !out) return -1;
    out[0] = f->shape_class, out[1] = f->fmt, out[2] = f->canon, out[3] = f->dbg, out[4] = (int)f->smem(n_layer);
    return 0;
}
// what a build answers for a descriptor, and why, without a device (kf::ENG_DRY_NO_DEVICE: every check of create but the CU count, in create's order; no device pointer is
// dereferenced).  family: 0 the persistent engine, 1 the XCD-confined engines with n_seq sequences
int kfdbg_engine_desc_refusal(int family, const kf_engine_desc* d, int n_seq, char* why, size_t n) {
    const char* w = "";
    const int rc = family == 0 ? kf::engine_build(d, nullptr, 0, nullptr, nullptr, &w, kf::ENG_DRY_NO_DEVICE)
                               : kf::xengine_build(d, n_seq, 0, nullptr, 0, nullptr, nullptr, &w, kf::ENG_DRY_NO_DEVICE);
    if (why && n > 0) snprintf(why, n, "%s", w);
    return rc;
}
// what the setters answer for an operand of an engine `dim` wide (kf_engine_host.h): kind 0 the in-launch head (has_norm_and_logits: both given), 1 the embedding table
int kfdbg_engine_operand_rule(int kind, const kf_weight* w, int dim, int has_norm_and_logits) {
    const void* given = has_norm_and_logits ? (const void*)w : nullptr;
    return kind == 0 ? kf::eng_head_rule(w, dim, given, given) : kf::eng_embed_rule(w, dim);
}
int kfdbg_xengine_stamps_enable(kf_xengine* e, int seq, int wg, int max_steps) { return ENG_DBG(e, kf::xengine_debug_enable(e->h, seq, wg, max_steps)); }
int kfdbg_xengine_stamps(kf_xengine* e, unsigned long long* h_out, int n_words) { return ENG_DBG(e, kf::xengine_debug_read(e->h, h_out, n_words)); }
// the per-phase stamps of one workgroup of the engine: enable (the diagnostic instantiation of the kernel serves the next launches), read
int kfdbg_engine_stamps_enable(kf_engine* e, int wg) { return ENG_DBG(e, kf::engine_debug_enable(e->h, wg)); }
int kfdbg_engine_stamps(kf_engine* e, unsigned long long* h_out, int n_words) { return ENG_DBG(e, kf::engine_debug_read(e->h, h_out, n_words)); }
int kfdbg_engine_set_delays(kf_engine* e, const int* d6) { return ENG_DBG(e, d6 ? (kf::engine_set_delays(e->h, d6), 0) : -1); }
// ---- int8 activations (include/kf_abi.h "int8 activations", "int8 activations for 4-bit layers"): the quantiser, then the products
int kf_act_quant_i8(kf_ctx* c, const kf_bf16* x, int64_t ldx, const kf_bf16* norm_w, float eps, int rows, int dim, int8_t* q, float* step) {
    CHKCTX(c);
    if (!x || !q || !step) return fail(KF_INVALID_ARGS, "kf_act_quant_i8: null pointer");
    if (rows < 1 || dim < 1 || ldx < dim) return fail(KF_INVALID_ARGS, "kf_act_quant_i8: rows=%d dim=%d ldx=%lld", rows, dim, (long long)ldx);
    if (norm_w && dim % 2 != 0) return fail(KF_RMS_PARAMS, "kf_act_quant_i8: rmsnorm dim %d is not divisible by 2", dim); /* what kf_rmsnorm refuses, the prologue refuses */
    RET(kf::act_quant_launch(c->stream, x, ldx, norm_w, eps, rows, dim, q, step));
}
// the products of the two families (1-bit / ternary: kf_linear_a8*, 4-bit: kf_linear_w4a8*) on the two routes: every launch decision is kf::a8_plan's (kf_a8.h).  An entry
// serves its own family: the other family's storage has no form there, whatever else is wrong with it
static kf::A8Plan a8_family_plan(int family, const kf::A8Problem& P) {
    kf::A8Plan p = kf::a8_plan(P);
    if (p.family != family) p = kf::A8Plan{}, p.status = KF_UNSUPPORTED_DATATYPE;
    return p;
}
static kf::A8Plan a8_entry_plan(int family, int route, const kf_weight* w, int nTok) { return a8_family_plan(family, kf::A8Problem{kf::mat_of(w), nTok, w->qBias, route}); }
static int a8_status(int family, int route, const kf_weight* w, int nTok) { return (w && w->data) ? a8_entry_plan(family, route, w, nTok).status : KF_INVALID_ARGS; }
static int a8_refusal(const char* entry, int family, int status, const kf_weight* w, int nTok) {
    const bool q4 = family == kf::A8_Q4;
    const char* awq = (w->qzeros || w->qscales) ? ", AutoAWQ" : "";
    if (status == KF_UNSUPPORTED_DATATYPE && q4)
        return fail(status, "%s: weight type %d (quant mode %d%s) has no W4.A8 form: served is KF_Q4 (%d) in group storage", entry, w->type, w->quant, awq, KF_Q4);
    if (status == KF_UNSUPPORTED_DATATYPE)
        return fail(status, "%s: weight type %d (quant mode %d%s) has no integer form: served are KF_T_SIGN (%d), KF_BOOL1 (%d), KF_T_BINARY (%d) in group storage", entry, w->type,
                    w->quant, awq, KF_T_SIGN, KF_BOOL1, KF_T_BINARY);
    if (status == KF_QUANT_ERR && q4) return fail(status, "%s: group size %d (must be 128), gama missing, or qBias %d (must be 0 or 8)", entry, w->lGroup, w->qBias);
    if (status == KF_QUANT_ERR) return fail(status, "%s: group size %d (must be 128) or gama missing", entry, w->lGroup);
    if (status == KF_BLAS_UNALIGN) return fail(status, "%s: weight data not 16-byte aligned", entry);
    return fail(status, "%s: %d x %d, nTok=%d: rows of whole 128-weight groups, at least one row and one token", entry, w->ne0, w->ne1, nTok);
}
static int a8_entry(const char* entry, int family, int route, kf_ctx* c, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias,
                    const kf_bf16* residual, int nTok) {
    CHKCTX(c);
    if (!w || !w->data) return fail(KF_INVALID_ARGS, "%s: null weight", entry);
    if (!q || !step || !y) return fail(KF_INVALID_ARGS, "%s: null pointer", entry);
    const kf::A8Plan p = a8_entry_plan(family, route, w, nTok);
    if (p.status != KF_OK) return a8_refusal(entry, family, p.status, w, nTok);
    RET(kf::a8_launch(c->stream, p, w, q, step, y, bias, residual, nTok));
}
int kf_linear_a8_status(const kf_weight* w, int nTok) { return a8_status(kf::A8_LOWBIT, kf::A8_MATVEC, w, nTok); }
int kf_linear_a8(kf_ctx* c, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias, const kf_bf16* residual, int nTok) {
    return a8_entry("kf_linear_a8", kf::A8_LOWBIT, kf::A8_MATVEC, c, w, q, step, y, bias, residual, nTok);
}
int kf_linear_a8_tiles_status(const kf_weight* w, int nTok) { return a8_status(kf::A8_LOWBIT, kf::A8_TILES, w, nTok); }
int kf_linear_a8_tiles(kf_ctx* c, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias, const kf_bf16* residual, int nTok) {
    return a8_entry("kf_linear_a8_tiles", kf::A8_LOWBIT, kf::A8_TILES, c, w, q, step, y, bias, residual, nTok);
}
int kf_linear_w4a8_status(const kf_weight* w, int nTok) { return a8_status(kf::A8_Q4, kf::A8_MATVEC, w, nTok); }
int kf_linear_w4a8(kf_ctx* c, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias, const kf_bf16* residual, int nTok) {
    return a8_entry("kf_linear_w4a8", kf::A8_Q4, kf::A8_MATVEC, c, w, q, step, y, bias, residual, nTok);
}
int kf_linear_w4a8_tiles_status(const kf_weight* w, int nTok) { return a8_status(kf::A8_Q4, kf::A8_TILES, w, nTok); }
int kf_linear_w4a8_tiles(kf_ctx* c, const kf_weight* w, const int8_t* q, const float* step, kf_bf16* y, const kf_bf16* bias, const kf_bf16* residual, int nTok) {
    return a8_entry("kf_linear_w4a8_tiles", kf::A8_Q4, kf::A8_TILES, c, w, q, step, y, bias, residual, nTok);
}
// the plan kf::a8_plan makes for a problem, either family, either route (no HIP call): tests/a8_plan_mirror.py
int kfdbg_a8_route_plan(const kf::A8Problem* P, kf::A8Plan* out) {
    if (!P || !out) return -1;
    *out = kf::a8_plan(*P);
    return 0;
}
// the four per-entry exports of earlier versions keep their names and layouts for callers built against them (tests/a8_plan_mirror.py check_views).  Each is a view of
// the one plan for an entry's problem: a route's figures only; the second word is `bits` for the low-bit family and `qbias` for q4, whose problem carries it
struct A8DbgProblem {
    kf::GemmMat w;
    int nTok;
};
struct W4A8DbgProblem {
    kf::GemmMat w;
    int nTok, qbias;
};
struct A8DbgMatvec {
    int status, bits_or_qbias, order, n_groups, lpr_log2, iters, rows_per_wave, rows_per_wg, tok_tile, tok_tiles, grid_x, grid_y, block, lds;
};
struct A8DbgTiles {
    int status, bits_or_qbias, order, n_groups, row_tile, tok_tile, waves, mfma_tok, chunk, grid_x, grid_y, block, lds, min_tok;
};
static int a8_dbg_matvec(int family, const kf::GemmMat& w, int nTok, int qbias, A8DbgMatvec* out) {
    const kf::A8Plan p = a8_family_plan(family, kf::A8Problem{w, nTok, qbias, kf::A8_MATVEC});
    *out = {p.status, family == kf::A8_Q4 ? p.qbias : p.bits, p.order, p.n_groups, p.lpr_log2, p.iters, p.rows_per_wave, p.rows_per_wg,
            p.tok_tile, p.tok_tiles, p.grid_x, p.grid_y, p.block, p.lds};
    return 0;
}
static int a8_dbg_tiles(int family, const kf::GemmMat& w, int nTok, int qbias, A8DbgTiles* out) {
    const kf::A8Plan p = a8_family_plan(family, kf::A8Problem{w, nTok, qbias, kf::A8_TILES});
    *out = {p.status, family == kf::A8_Q4 ? p.qbias : p.bits, p.order, p.n_groups, p.row_tile, p.tok_tile, p.waves, p.mfma_tok, p.chunk,
            p.grid_x, p.grid_y, p.block, p.lds, kf::A8T_MIN_TOK};
    return 0;
}
int kfdbg_a8_plan(const A8DbgProblem* P, A8DbgMatvec* out) { return (P && out) ? a8_dbg_matvec(kf::A8_LOWBIT, P->w, P->nTok, 0, out) : -1; }
int kfdbg_a8_tile_plan(const A8DbgProblem* P, A8DbgTiles* out) { return (P && out) ? a8_dbg_tiles(kf::A8_LOWBIT, P->w, P->nTok, 0, out) : -1; }
int kfdbg_w4a8_plan(const W4A8DbgProblem* P, A8DbgMatvec* out) { return (P && out) ? a8_dbg_matvec(kf::A8_Q4, P->w, P->nTok, P->qbias, out) : -1; }
int kfdbg_w4a8_tile_plan(const W4A8DbgProblem* P, A8DbgTiles* out) { return (P && out) ? a8_dbg_tiles(kf::A8_Q4, P->w, P->nTok, P->qbias, out) : -1; }

// the plan kf::gemm_plan makes for a problem (no HIP call): tests/test_gemm_plan_cpu.py
int kfdbg_gemm_plan(const kf::GemmProblem* P, kf::GemmPlan* out) {
    if (!P || !out) return -1;
    *out = kf::gemm_plan(*P);
    return 0;
}
// the 4-bit stand-in kf::rowq_standin plans a 3- / 2-bit row form as (no HIP call): out[8] = status, real format, then the stand-in's type, quant, M, K, gama, al;
// tests/test_rowq_cpu.py
int kfdbg_rowq_standin(const kf_weight* w, int* out) {
    if (!w || !out) return -1;
    kf::GemmMat m = {};
    int fmt = -1;
    out[0] = kf::rowq_standin(w, &m, &fmt), out[1] = fmt;
    out[2] = m.type, out[3] = m.quant, out[4] = m.M, out[5] = m.K, out[6] = m.gama, out[7] = m.al;
    return 0;
}
// the plan kf::gemv_plan makes for a one-token mat-vec problem (no HIP call): tests/test_gemv_plan_cpu.py
int kfdbg_gemv_plan(const kf::GemvProblem* P, kf::GemvPlan* out) {
    if (!P || !out) return -1;
    *out = kf::gemv_plan(*P);
    return 0;
}
// the plan kf::gemv_rows_plan makes for R activation rows over one weight pass (no HIP call): tests/test_gemv_rows_plan_cpu.py
int kfdbg_gemv_rows_plan(const kf::GemvRowsProblem* P, kf::GemvRowsPlan* out) {
    if (!P || !out) return -1;
    *out = kf::gemv_rows_plan(*P);
    return 0;
}
// the plan kf::attn_plan makes for an attention problem (no HIP call): tests/test_attn_plan_cpu.py
int kfdbg_attn_plan(const kf::AttnProblem* P, kf::AttnPlan* out) {
    if (!P || !out) return -1;
    *out = kf::attn_plan(*P);
    return 0;
}
// the plan of kf_attn_block_kv8 (the ATTN_DECODE_KV8 entry of kf::attn_plan; no HIP call): tests/test_kv8_cpu.py
int kfdbg_kv8_plan(int n_head, int n_kv, int hd, int pos, int kv_stride, kf::AttnPlan* out) {
    if (!out) return -1;
    *out = kf::attn_plan(kv8_problem(n_head, n_kv, hd, pos, kv_stride));
    return 0;
}
// the table kf::gradnorm_plan lays out for a list of tensor lengths (no HIP call): wg0_out [n_tensors + 1], and for every workgroup the tensor gradnorm_find gives it
// (owner_out [total_wg], may be NULL): tests/test_gradnorm_cpu.py
int kfdbg_gradnorm_plan(int n_tensors, const long long* n, kf::GradNormPlan* out, int* wg0_out, int* owner_out) {
    if (!out) return -1;
    *out = kf::gradnorm_plan(n_tensors, n);
    if (out->status != KF_OK || !wg0_out) return 0;
    kf::gradnorm_wg0(n_tensors, n, wg0_out);
    if (owner_out) {
        std::vector<kf::GradNormEntry> tab((size_t)n_tensors + 1);
        for (int i = 0; i <= n_tensors; i++) tab[i].wg0 = wg0_out[i];
        for (int wg = 0; wg < out->total_wg; wg++) owner_out[wg] = kf::gradnorm_find(tab.data(), n_tensors, wg);
    }
    return 0;
}
// the plan kf::lora_plan makes for an adapter (no HIP call): tests/test_lora_cpu.py
int kfdbg_lora_plan(int r, int OC, int IC, int n, kf::LoraPlan* out) {
    if (!out) return -1;
    *out = kf::lora_plan(r, OC, IC, n);
    return 0;
}
// the plan kf::score_plan makes for a scoring problem (no HIP call): tests/test_score_cpu.py
int kfdbg_score_plan(const kf::ScoreProblem* P, kf::ScorePlan* out) {
    if (!P || !out) return -1;
    *out = kf::score_plan(*P);
    return 0;
}
// development knobs (kf::Knobs): a kernel form against the form it replaces, inside one process (the token-batch routes have none: kf_gemm_plan.h; the mat-vec's
// slots per wave and load form none either: kf_gemv_plan.h; nor the attention routes and forms: kf_attn_plan.h)
int kfdbg_set_knob(const char* name, long value) {
    if (!name) return -1;
    kf::Knobs& k = kf::g_knobs;
    if (!strcmp(name, "q4_perm")) k.q4_perm = (int)value;
    else if (!strcmp(name, "q2_tab")) k.q2_tab = (int)value;
    else if (!strcmp(name, "q1_tab")) k.q1_tab = (int)value;
    else if (!strcmp(name, "gemv_xf2")) k.gemv_xf2 = (int)value;
    else if (!strcmp(name, "score_route")) k.score_route = (int)value;
    else if (!strcmp(name, "score_form")) k.score_form = (int)value;
    else return -1;
    return 0;
}
int kf_engine_destroy(kf_engine* e) {
    if (e) kf::engine_free(e->h);
    delete e;
    return KF_OK;
}

}  // extern "C"
