// kf_engine_host.h -- the host rules the two decode-engine families share (kf_engine.hip: one sequence on every CU; kf_xengine.hip: decoders confined to an XCD).  Host code
// only, free functions and one plain struct: which model shapes, descriptors, heads and embedding tables an engine takes (these decide whether a model is served and in
// which summation order it runs), the layer table out of a descriptor, and the few HIP calls both build, check, reset and first-launch paths make.
#pragma once
#include <vector>

#include "kf_engine_common.h"

namespace kf {

// ---- a model's dimensions: what a shape-table row is compared by and what the host object of an engine keeps
struct EngDims {
    int hd, dim, q_dim, kv_dim, ffn, n_head, n_kv;
};
inline EngDims eng_dims_of(const kf_engine_desc* d) { return EngDims{d->head_dim, d->dim, d->n_head * d->head_dim, d->n_kv * d->head_dim, d->ffn, d->n_head, d->n_kv}; }
template <class C> /* the row of a kernel form (EngCfg / XCfg) */
constexpr EngDims eng_dims_c() {
    return EngDims{C::HD, C::DIM, C::QD, C::KVD, C::FFN, C::QD / C::HD, C::KVD / C::HD};
}
inline bool eng_dims_match(const EngDims& row, const EngDims& d) { return d.hd == row.hd && d.dim == row.dim && d.q_dim == row.q_dim && d.kv_dim == row.kv_dim && d.ffn == row.ffn; }

// ---- the descriptor prologue of every build (each caller words its own refusal and keeps its own place in the order of checks)
inline bool eng_desc_heads_ok(const kf_engine_desc* d) { return (d->head_dim == 64 || d->head_dim == 128) && d->n_kv > 0 && d->n_head % d->n_kv == 0; }
inline bool eng_desc_cache_ok(const kf_engine_desc* d) { return d->rope_table && (d->kv_stride % 8) == 0 && d->max_seq >= 1; }
// the CUs of the current device; what the count must be is the family's premise and stays with it
inline int eng_device_cus(int* n_cu) {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

// ---- operands of the in-launch phases.  A head: bf16 [vocab >= 64, dim] in group form, 16-byte aligned, with its norm weight and logits buffer, and the compile-time geometry
// of the head phases must be the mat-vec launcher's for this matrix (same lanes per row: same summation order).  An embedding table: bf16 [rows, dim] in group form.
inline int eng_embed_rule(const kf_weight* w, int dim) {
    return w && w->type == KF_BF16 && w->quant == KF_QUANT_GROUP && !w->qzeros && w->ne1 == dim && w->data ? KF_OK : KF_UNSUPPORTED_DATATYPE;
}
inline int eng_head_rule(const kf_weight* w, int dim, const void* norm_w, const void* logits) {
    if (eng_embed_rule(w, dim) != KF_OK || ((uintptr_t)w->data & 15) != 0 || !norm_w || !logits || w->ne0 < 64) return KF_UNSUPPORTED_DATATYPE;
    return gemv_lpr_log2(8, dim, w->ne0) == gemv_lpr_log2(8, dim, 1L << 20) ? KF_OK : KF_UNSUPPORTED_DATATYPE;
}

// one model's (one TP rank's) layer table out of its descriptor, validated for both engine families; qbias: the seven matrices' zero points of layer 0 (every layer, every
// rank: the same).  *fmt_io: the storage every matrix of the model carries (0 on entry = not known yet): FMT_Q4P, FMT_Q1T or FMT_Q2T; NULL: 4-bit only.  Reads descriptor
// fields and forms addresses; no device pointer is dereferenced.
inline int eng_fill_layers(const kf_engine_desc* d, EngLayer* tab, float* qbias, bool qbias_set, bool& q4p_ok, int* fmt_io = nullptr, bool allow_hot = false) {
    const int hd = d->head_dim, q_dim = d->n_head * hd, kv_dim = d->n_kv * hd;
    const int Ks[7] = {d->dim, d->dim, d->dim, q_dim, d->dim, d->dim, d->ffn}, Ms[7] = {q_dim, kv_dim, kv_dim, d->dim, d->ffn, d->ffn, d->dim};
    for (int l = 0; l < d->n_layer; l++) {
        const kf_engine_layer& Ly = d->layers[l];
        if (Ly.hot_ffn && !allow_hot) return KF_UNSUPPORTED_DATATYPE;
        if (!Ly.norm_in || !Ly.norm_post || !Ly.kcache || !Ly.vcache || (((uintptr_t)Ly.kcache | (uintptr_t)Ly.vcache) & 15) != 0) return KF_UNSUPPORTED_DATATYPE;
        for (int j = 0; j < 7; j++) {
            const kf_weight& w = Ly.w[j];
            const int wf = gemv_fmt(mat_of(&w)), ef = wf == FMT_Q4 ? FMT_Q4P : (wf == FMT_Q1 ? FMT_Q1T : (wf == FMT_Q2 ? FMT_Q2T : -1));
            if (ef < 0 || (!fmt_io && ef != FMT_Q4P) || (fmt_io && *fmt_io != 0 && *fmt_io != ef)) return KF_UNSUPPORTED_DATATYPE;
            if (fmt_io) *fmt_io = ef;
            if (w.ne0 != Ms[j] || w.ne1 != Ks[j] || w.qzeros || w.qscales || !w.gama || w.lGroup != 128 || (Ks[j] % 128) != 0 || ((uintptr_t)w.data & 15) != 0)
                return KF_UNSUPPORTED_DATATYPE;
            const long rows = j < 3 ? (long)q_dim + 2 * kv_dim : (j == 4 || j == 5 ? (long)d->ffn : (long)Ms[j]);
            if (gemv_lpr_log2(32, Ks[j], rows) < 2) q4p_ok = false; /* the register-table form needs a group's four blocks in one aligned lane quad (1-bit: the four dwords of a block in one) */
            tab[l].m[j].w = (g_u32x4)(uintptr_t)w.data;
            tab[l].m[j].zero = (g_u16)(uintptr_t)(w.gama + w.ne0 + w.ne1);
            tab[l].m[j].step = (g_u16)(uintptr_t)(w.gama + w.ne0 + w.ne1 + (size_t)w.ne0 * w.ne1 / w.lGroup);
            if (l == 0 && !qbias_set) qbias[j] = (float)w.qBias;
            else if (qbias[j] != (float)w.qBias) return KF_UNSUPPORTED_DATATYPE;
        }
        tab[l].norm_in = (g_u16)(uintptr_t)Ly.norm_in, tab[l].norm_post = (g_u16)(uintptr_t)Ly.norm_post;
        tab[l].norm_q = (g_u16)(uintptr_t)Ly.q_norm, tab[l].norm_k = (g_u16)(uintptr_t)Ly.k_norm;
        tab[l].kcache = (g_u16w)(uintptr_t)Ly.kcache, tab[l].vcache = (g_u16w)(uintptr_t)Ly.vcache;
        tab[l].hot = (g_i32)(uintptr_t)Ly.hot_ffn; /* sparse forward: CS_Picker's hot[ffn] on the device (kf_abi.h kf_engine_layer::hot_ffn); NULL: dense */
    }
    return KF_OK;
}

// ---- the HIP calls both families make
inline int eng_then_sync(int rc, hipStream_t st) { return rc != KF_OK ? rc : (hipStreamSynchronize(st) == hipSuccess ? KF_OK : KF_HIP_CHECK); } /* a reset: the family's init state, then this */
// the build tail behind the family's init state (init_rc): the layer table uploaded, the stream drained; the caller releases its engine when this fails
inline int eng_upload_layers(int init_rc, const EngLayer* dst, const std::vector<EngLayer>& tab, hipStream_t st, const char** why) {
    *why = "HIP failure while initialising the workspace";
    if (init_rc != KF_OK || hipMemcpyAsync(const_cast<EngLayer*>(dst), tab.data(), tab.size() * sizeof(EngLayer), hipMemcpyHostToDevice, st) != hipSuccess) return KF_HIP_CHECK;
    if (hipStreamSynchronize(st) != hipSuccess) return KF_HIP_CHECK;
    *why = "";
    return KF_OK;
}
inline int eng_read_error_word(const int* ws, hipStream_t st, int* h_err) { /* ws[0] the epoch, ws[1] the error word */
    int v[2] = {0, 0};
    if (hipMemcpyAsync(v, ws, sizeof(v), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return KF_HIP_CHECK;
    *h_err = v[1];
    return KF_OK;
}
// the per-phase stamps of a diagnostic form (each family sizes its own buffer): allocated where absent and zeroed; n_words of them read (0: stamps are off, -1: HIP failure)
inline int eng_stamps_zeroed(unsigned long long** dbg, size_t bytes) {
    if (!*dbg && hipMalloc(dbg, bytes) != hipSuccess) {
        *dbg = nullptr;
        return KF_HIP_CHECK;
    }
    (void)hipMemset(*dbg, 0, bytes);
    return KF_OK;
}
inline int eng_stamps_read(const unsigned long long* dbg, unsigned long long* h_out, int n_words) {
    if (!dbg) return 0;
    return hipMemcpy(h_out, dbg, (size_t)n_words * 8, hipMemcpyDeviceToHost) == hipSuccess ? n_words : -1;
}
// the 160 KB ceiling of a kernel's dynamic LDS, raised before its first launch on each device: the attribute is per device, so one bit per device.  C, the
// kernel's configuration type, keys the word: every form of a family has the same function type K.
template <class C, class K>
int eng_raise_lds(K kernel) {
    static unsigned long long ready = 0; /* bit d: the attribute is set on device d */
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return KF_HIP_CHECK;
    if (dev < 0 || dev >= 64 || !((ready >> dev) & 1ull)) {
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return KF_HIP_CHECK;
        if (dev >= 0 && dev < 64) ready |= 1ull << dev;
    }
    return KF_OK;
}

}  // namespace kf
