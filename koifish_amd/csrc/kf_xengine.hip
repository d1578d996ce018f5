// kf_xengine.hip -- host side of the XCD-confined decode engines (the kernel: kf_xengine_kernel.h): the table of shapes, workspaces, the layer tables, the table of forms
// (the 4-bit instantiations) and the one rule that picks a form at create and at every launch.  (kf_xengine_q1.hip: the 1-bit / 2-bit forms.)
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kf_xengine_kernel.h"

namespace kf {

// ------------------------------------------------------------------------------------------------ host side

template <int NWV, int DEPTH, bool DBG, int WPC, int AU = 2, int NB = 1>
using XC1 = XCfg<FMT_Q4P, 2, 128, NWV, 1024, 2048, 1024, 3072, DEPTH, DBG, WPC, AU, false, NB>; /* Qwen3-0.6B (BASELINE config 2) */
template <int NWV, int DEPTH, bool DBG, int WPC, int AU = 2, int NB = 1>
using XC2 = XCfg<FMT_Q4P, 2, 64, NWV, 256, 256, 128, 512, DEPTH, DBG, WPC, AU, false, NB>; /* the small parity-test shape */
template <int NWV, int DEPTH, bool DBG, int WPC, int AU = 2, int NB = 1>
using XC3 = XCfg<FMT_Q4P, 2, 128, NWV, 2048, 2048, 1024, 6144, DEPTH, DBG, WPC, AU, false, NB>; /* Qwen3-1.7B: the streaming phases do not care how many blocks a lane walks */
// the GQA-4 shapes (Qwen3-4B / 8B: 32 / 8 heads; cases/tutorial/history.md:4-6): one decoder per XCD, 11 compute waves at 168 registers: the attention loop spills, the mat-vec
// phases (nine tenths of the bytes) have the waves
using XC4W = XCfg<FMT_Q4P, 4, 128, 12, 2560, 4096, 1024, 9728, 6, false, 1, 1>;
using XC5W = XCfg<FMT_Q4P, 4, 128, 12, 4096, 4096, 1024, 12288, 6, false, 1, 1>;
using XC6 = XCfg<FMT_Q4P, 8, 64, 12, 256, 512, 64, 512, 6, false, 1, 2>; /* parity-test shape: 8 query heads on ONE kv-head (two head groups), 20 workgroups with q | k | v rows */
// ---- tensor parallel over the XCDs: ONE sequence of a model too wide for one XCD's share to be a decoder of its own -- eight ranks = eight XCDs (XCfg::TP)
// a rank of Qwen3-32B under TP = 8: 8 query heads on 1 kv-head, q_dim 1024, ffn 3200 (koifish_amd/tp.py TPPlan)
using XC7 = XCfg<FMT_Q4P, 8, 128, 12, 5120, 1024, 128, 3200, 6, false, 1, 1, true>;
using XC7D = XCfg<FMT_Q4P, 8, 128, 12, 5120, 1024, 128, 3200, 6, true, 1, 1, true>; /* + the per-phase stamps of one workgroup of one rank */
// a rank of Qwen3-8B under TP = 8 (round 6: ONE sequence of a GQA-4 model on the eight XCDs): 4 query heads on 1 kv-head, q_dim 512, ffn 1536 (12 groups of 128)
using XC8 = XCfg<FMT_Q4P, 4, 128, 12, 4096, 512, 128, 1536, 6, false, 1, 1, true>;
// a rank of Qwen3-4B under TP = 8: ffn 9728 = 76 groups of 128 does not split into eight whole-group column shards -- the model is run with its FFN padded to 80 groups (512
// zero rows of gate / up, 512 zero columns of down_proj: exact zeros in every sum), 1280 per rank
using XC9 = XCfg<FMT_Q4P, 4, 128, 12, 2560, 512, 128, 1280, 2, false, 1, 1, true>; /* (ring depth, ms per token at 2 k keys: 6 2.33, 4 2.25, 2 2.22; 8 waves 2.42 - 2.48, 16 waves 2.87) */
static_assert(XC7::FUSED && XC8::FUSED && XC9::FUSED, "the TP forms multiply q | k | v as one fused matrix");

// ---- the table of shapes: one row per shape class, read off a form of the shape (the dimensions, TP, the fused q | k | v copy and the exchange area are the same in every form)
struct XShape {
    int sc;
    EngDims dm;
    bool tp, fused;
    int loc_dw;  /* a decoder's XCD-local exchange area (dwords) */
    int max_seq; /* the most sequences served */
    bool lowbit; /* 1-bit / 2-bit layers served (kf_xengine_q1.hip) */
};
template <class C>
constexpr XShape xe_shape(int sc, int max_seq, bool lowbit) {
    return XShape{sc, eng_dims_c<C>(), C::TP, C::FUSED, C::loc_dw, max_seq, lowbit};
}
// more than 8 sequences: two or four per decoder (XCfg::NB) for the 16 / 8-head shapes; the GQA-4 / GQA-8 shapes would need two workgroups per CU, 2 x 78 KB (2 x 98 KB) of
// activations in LDS
static const XShape xe_shapes[] = {xe_shape<XC1<12, 2, false, 1>>(1, XE_MAXSEQ, true), xe_shape<XC2<12, 2, false, 1>>(2, XE_MAXSEQ, true), xe_shape<XC3<12, 6, false, 1>>(3, 2 * XE_NXCD, false),
                                   xe_shape<XC4W>(4, XE_NXCD, false), xe_shape<XC5W>(5, XE_NXCD, false), xe_shape<XC6>(6, XE_NXCD, false),
                                   xe_shape<XC7>(7, XE_NXCD, false), xe_shape<XC8>(8, XE_NXCD, false), xe_shape<XC9>(9, XE_NXCD, false)};
static const XShape* xe_shape_of(const kf_engine_desc* d, bool tp) { /* nullptr: not instantiated */
    for (const XShape& s : xe_shapes)
        if (s.tp == tp && eng_dims_match(s.dm, eng_dims_of(d))) return &s;
    return nullptr;
}

// ---- the table of forms: every instantiation the engines launch, in the rule's order of preference (xengine_form)
// classes 1 and 2.  n_seq <= 8: one sequence per decoder, 12 waves (11 compute waves + the poller, 168 registers) at ring depth 2 (8 sequences: depth 6 4370, 4 4570, 2 4630
// tokens/s).  More: the BATCHED form (round 6) -- still one decoder per XCD, every unpacked block multiplied against the activations of 2 (n_seq <= 16; depth 6 5990, 4 6250,
// 2 6200) or 4 (n_seq <= 32) sequences.  Four: 8 compute waves + the four sequences' pollers at ring depth 2 (measured, 32 sequences at 2 k keys, tokens/s: depth 8 5320 --
// spills --, 6 6970, 4 7360, 2 7815: with four sequences' chain pairs and activation chunks live, every register the ring does not hold is worth more than a deeper queue) where
// the four sequences' activations + the layer table fit the LDS, else 4 + 4 waves.  The round-5 form of 9 .. 16 sequences (two decoders per XCD, two workgroups of 8 waves per
// CU, 128 registers) stays behind XEngineHost::two_wpc as the A/B reference.  Then the stamped twins.
#define XE_SMALL_FORMS(XC, sc)                                                                                                                                         \
    xe_form<XC<12, 2, false, 1, 2, 1>>(sc), xe_form<XC<12, 4, false, 1, 2, 2>>(sc), xe_form<XC<12, 2, false, 1, 2, 4>>(sc), xe_form<XC<8, 8, false, 1, 2, 4>>(sc), \
        xe_form<XC<8, 4, false, 2, 1, 1>>(sc), xe_form<XC<12, 2, true, 1, 2, 1>>(sc), xe_form<XC<12, 4, true, 1, 2, 2>>(sc), xe_form<XC<12, 2, true, 1, 2, 4>>(sc),      \
        xe_form<XC<8, 4, true, 2, 1, 1>>(sc)
static const XForm xe_forms[] = {
    XE_SMALL_FORMS(XC1, 1), XE_SMALL_FORMS(XC2, 2),
    // the 1.7B shape: one sequence per decoder at 12 waves (eight sequences: 1940 tokens/s); two: 6 compute waves + 2 pollers at 256 registers, ring depth 8 (16 sequences at
    // 2 k keys, ring depth 4 / 6 / 8: 2180 / 2230 / 2240 tokens/s; 12 waves at 168 registers spill in the streaming loops: 1650 - 1690; round 5's two decoders per XCD 1600)
    xe_form<XC3<12, 6, false, 1>>(3), xe_form<XC3<8, 8, false, 1, 2, 2>>(3), xe_form<XC3<8, 4, false, 2, 1>>(3),
    xe_form<XC4W>(4), xe_form<XC5W>(5), xe_form<XC6>(6), xe_form<XC7>(7), xe_form<XC7D>(7), xe_form<XC8>(8), xe_form<XC9>(9)};
#undef XE_SMALL_FORMS
const XForm* xe_forms_lowbit(int* n); /* kf_xengine_q1.hip: the 1-bit / 2-bit entries of the table */
template <class Match>
static const XForm* xe_find(Match match) {
    for (const XForm& f : xe_forms)
        if (match(f)) return &f;
    int n = 0;
    const XForm* lowbit = xe_forms_lowbit(&n);
    for (int i = 0; i < n; i++)
        if (match(lowbit[i])) return &lowbit[i];
    return nullptr;
}
// one, two or four sequences per decoder (n_seq <= 8 / 16 / 32); the two hooks where the shape and storage have a form for them: two decoders per XCD instead of two sequences
// per decoder, the stamps; then the first form of that kind whose LDS fits
const XForm* xengine_form(int sc, int fmt, int n_seq, int n_layer, bool stamps, bool two_wpc) {
    int nb = n_seq <= XE_NXCD ? 1 : (n_seq <= 2 * XE_NXCD ? 2 : 4), wpc = 1;
    auto kind = [sc, fmt](int nb, int wpc, bool dbg) { return [=](const XForm& f) { return f.shape_class == sc && f.fmt == fmt && f.nb == nb && f.wpc == wpc && f.dbg == dbg; }; };
    if (two_wpc && nb == 2 && xe_find(kind(1, 2, false))) nb = 1, wpc = 2;
    const auto want = kind(nb, wpc, stamps && xe_find(kind(nb, wpc, true)));
    return xe_find([&](const XForm& f) { return want(f) && f.smem(n_layer) * f.wpc <= 160 * 1024; });
}

// FUSED shapes (XCfg::FUSED): q | k | v of a layer as ONE matrix -- blocks, then the zero words, then the step words of the QD + 2 KVD rows -- copied once into the workspace
static size_t xe_fused_layer_bytes(const kf_engine_desc* d) {
    const size_t rows = (size_t)(d->n_head + 2 * d->n_kv) * d->head_dim, nblk = d->dim / 32, grp = d->dim / 128;
    return ((rows * nblk * 16 + 255) & ~(size_t)255) + 2 * ((rows * grp * 2 + 255) & ~(size_t)255);
}
static int xe_fuse_qkv(const kf_engine_desc* d, EngLayer* tab, const float* qbias, char*& p, hipStream_t st) {
    if (qbias[0] != qbias[1] || qbias[0] != qbias[2]) return KF_UNSUPPORTED_DATATYPE; /* one zero point for the fused rows */
    const size_t nblk = d->dim / 32, grp = d->dim / 128;
    const size_t rows_all = (size_t)(d->n_head + 2 * d->n_kv) * d->head_dim;
    for (int l = 0; l < d->n_layer; l++) {
        char* wdst = p;
        char* zdst = wdst + ((rows_all * nblk * 16 + 255) & ~(size_t)255);
        char* sdst = zdst + ((rows_all * grp * 2 + 255) & ~(size_t)255);
        size_t r0 = 0;
        for (int j = 0; j < 3; j++) {
            const kf_weight& w = d->layers[l].w[j];
            const size_t rows = (size_t)w.ne0;
            const uint16_t* zero = w.gama + w.ne0 + w.ne1;
            const uint16_t* step = zero + rows * grp;
            if (hipMemcpyAsync(wdst + r0 * nblk * 16, w.data, rows * nblk * 16, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                hipMemcpyAsync(zdst + r0 * grp * 2, zero, rows * grp * 2, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                hipMemcpyAsync(sdst + r0 * grp * 2, step, rows * grp * 2, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return KF_HIP_CHECK;
            r0 += rows;
        }
        tab[l].m[0].w = (g_u32x4)(uintptr_t)wdst, tab[l].m[0].zero = (g_u16)(uintptr_t)zdst, tab[l].m[0].step = (g_u16)(uintptr_t)sdst;
        p += xe_fused_layer_bytes(d);
    }
    return KF_OK;
}

size_t xengine_ws_bytes(const kf_engine_desc* d) {
    const XShape* sh = xe_shape_of(d, false);
    size_t b = 4096 + (((size_t)d->n_layer * sizeof(EngLayer) + 255) & ~(size_t)255);
    b += (size_t)XE_MAXSEQ * xe_loc_stride(sh ? sh->loc_dw : 0) + 4096;
    if (sh && sh->fused) b += (size_t)d->n_layer * xe_fused_layer_bytes(d) + 256;
    return b;
}
static size_t xe_tp_recv_granules(int dim) { return (size_t)XE_NXCD * 2 * XE_NXCD * dim; }
size_t xengine_ws_bytes_tp(const kf_engine_desc* d0) {
    const XShape* sh = xe_shape_of(d0, true);
    size_t b = 4096 + (((size_t)XE_NXCD * d0->n_layer * sizeof(EngLayer) + 255) & ~(size_t)255);
    b += (size_t)XE_NXCD * xe_loc_stride(sh ? sh->loc_dw : 0) + 4096;
    b += xe_tp_recv_granules(d0->dim) * 8 + (size_t)XE_NXCD * XE_NXCD * 8 + 4096;
    b += (size_t)XE_NXCD * d0->n_layer * xe_fused_layer_bytes(d0) + 256;
    return b;
}
static int xengine_init_state(XEngineHost* E, hipStream_t st) {
    XArgs& a = E->args;
    if (hipMemsetAsync(a.loc, 0xff, (size_t)(E->tp_bytes ? XE_NXCD : XE_MAXSEQ) * E->loc_stride, st) != hipSuccess) return KF_HIP_CHECK;
    if (E->tp_bytes && hipMemsetAsync(a.tp_recv, 0xff, E->tp_bytes, st) != hipSuccess) return KF_HIP_CHECK;
    static int init[16 + 32 * XE_NXCD];
    memset(init, 0, sizeof(init));
    init[0] = 1; /* no error, tickets zero */
    if (hipMemcpyAsync(a.ws, init, sizeof(init), hipMemcpyHostToDevice, st) != hipSuccess) return KF_HIP_CHECK;
    E->epoch = 1;
    return KF_OK;
}
void xengine_free(XEngineHost* E) {
    if (!E) return;
    if (E->args.dbg) (void)hipFree(E->args.dbg);
    delete E;
}
// the engine over its validated, filled layer table (TP: the eight ranks' tables one after the other, ds[r] rank r's descriptor): the workspace carved, the fused q | k | v
// copies made, the state initialised
static int xe_make(const kf_engine_desc* const* ds, const XShape* sh, int fmt, int n_seq, long long kv_seq_stride, std::vector<EngLayer>& tab, const float* qbias, void* ws,
                   size_t ws_bytes, hipStream_t st, XEngineHost** out, const char** why) {
    const kf_engine_desc* d = ds[0];
    XEngineHost* E = new XEngineHost();
    memset(E, 0, sizeof(*E));
    XArgs& a = E->args;
    E->shape_class = sh->sc, E->fmt = fmt, E->dm = eng_dims_of(d);
    a.n_layer = d->n_layer, a.n_seq = n_seq, a.kv_seq_stride = kv_seq_stride, a.kv_stride = d->kv_stride, a.max_seq = d->max_seq;
    a.eps = d->rms_eps, a.qk_eps = d->qk_eps, a.rope_table = d->rope_table;
    for (int j = 0; j < 7; j++) a.qbias[j] = qbias[j];
    char* p = reinterpret_cast<char*>(ws);
    E->ws = ws, E->ws_bytes = ws_bytes;
    a.ws = reinterpret_cast<int*>(p), p += 4096;
    a.layers = reinterpret_cast<const EngLayer*>(p), p += (tab.size() * sizeof(EngLayer) + 255) & ~(size_t)255;
    p = reinterpret_cast<char*>(((uintptr_t)p + 4095) & ~(uintptr_t)4095);
    E->loc_stride = xe_loc_stride(sh->loc_dw);
    a.loc = p, a.loc_stride = E->loc_stride, p += (size_t)(sh->tp ? XE_NXCD : XE_MAXSEQ) * E->loc_stride;
    if (sh->tp) {
        a.tp_recv = reinterpret_cast<unsigned long long*>(p), p += xe_tp_recv_granules(d->dim) * 8;
        a.tp_best = reinterpret_cast<unsigned long long*>(p), p += (size_t)XE_NXCD * XE_NXCD * 8;
        E->tp_bytes = xe_tp_recv_granules(d->dim) * 8 + (size_t)XE_NXCD * XE_NXCD * 8;
    }
    if (sh->fused) {
        char* fp = reinterpret_cast<char*>(((uintptr_t)p + 255) & ~(uintptr_t)255);
        for (int r = 0; r < (sh->tp ? XE_NXCD : 1); r++) {
            const int frc = xe_fuse_qkv(ds[r], tab.data() + (size_t)r * d->n_layer, qbias, fp, st);
            if (frc != KF_OK) {
                xengine_free(E);
                *why = "q / k / v carry different zero points (the fused copy of the three takes one), or a HIP failure while copying";
                return frc;
            }
        }
    }
    if (eng_upload_layers(xengine_init_state(E, st), a.layers, tab, st, why) != KF_OK) {
        xengine_free(E);
        return KF_HIP_CHECK;
    }
    *out = E;
    return KF_OK;
}
int xengine_build(const kf_engine_desc* d, int n_seq, long long kv_seq_stride, void* ws, size_t ws_bytes, hipStream_t st, XEngineHost** out, const char** why, int mode) {
    const bool dry = mode != ENG_BUILD; /* ENG_DRY: validation only, nothing allocated, ws may be NULL; ENG_DRY_NO_DEVICE: the same without the question to the device */
    *why = "bad arguments";
    if (!d || (!dry && (!ws || !out)) || d->n_layer < 1 || !d->layers || n_seq < 1 || n_seq > XE_MAXSEQ || kv_seq_stride < 0) return KF_INVALID_ARGS;
    *why = "head_dim must be 64 or 128 and n_head a multiple of n_kv";
    if (!eng_desc_heads_ok(d)) return KF_UNSUPPORTED_DATATYPE;
    const XShape* sh = xe_shape_of(d, false);
    *why = "model shape not instantiated for the XCD-confined engine: built for Qwen3-0.6B (dim 1024, 16/8 heads of 128, ffn 3072), Qwen3-1.7B (dim 2048, same heads, ffn 6144), Qwen3-4B "
           "(dim 2560, 32/8 heads, ffn 9728), Qwen3-8B (dim 4096, 32/8 heads, ffn 12288) and the 256-wide test shape";
    if (!sh) return KF_UNSUPPORTED_DATATYPE;
    *why = sh->max_seq == XE_NXCD ? "the GQA-4 / GQA-8 shapes (Qwen3-4B / 8B, the 8-on-1 test shape) run one decoder per XCD: at most 8 sequences (two workgroups per CU would need 2 x 78 KB (2 x 98 KB) of activations in LDS)"
                                  : "more than 16 sequences (four per decoder) are served for the Qwen3-0.6B shape and the 256-wide test shape only";
    if (n_seq > sh->max_seq) return KF_UNSUPPORTED_DATATYPE;
    if (!dry && (ws_bytes < xengine_ws_bytes(d) || ((uintptr_t)ws & 255) != 0)) {
        *why = "workspace too small or not 256-byte aligned";
        return KF_INVALID_ARGS;
    }
    int n_cu = XE_GRID;
    *why = "HIP failure";
    if (mode != ENG_DRY_NO_DEVICE && eng_device_cus(&n_cu) != KF_OK) return KF_HIP_CHECK;
    *why = "the device does not show 256 compute units (8 XCDs of 32): one resident workgroup per CU, 32 per XCD, is the premise";
    if (n_cu != XE_GRID) return KF_UNSUPPORTED_DATATYPE;
    *why = "rope_table missing, kv_stride not a multiple of 8, or max_seq < 1";
    if (!eng_desc_cache_ok(d)) return KF_INVALID_ARGS;
    *why = "layer storage not served: 4-bit (RTN), 2-bit or 1-bit (YinYang) PackedQ layers in groups of 128 with 16-byte aligned blocks, every matrix the same storage, every layer the same shapes (FFN dense or with a hot-row mask)";
    std::vector<EngLayer> tab(d->n_layer);
    float qbias[7] = {0};
    bool q4p_ok = true;
    int fmt = 0;
    if (eng_fill_layers(d, tab.data(), qbias, false, q4p_ok, &fmt, true) != KF_OK || !q4p_ok) return KF_UNSUPPORTED_DATATYPE;
    *why = "1-bit / 2-bit PackedQ layers are served for the Qwen3-0.6B shape and the 256-wide test shape";
    if (fmt != FMT_Q4P && !sh->lowbit) return KF_UNSUPPORTED_DATATYPE;
    *why = sh->sc == 3 && n_seq > XE_NXCD ? "two decoders per XCD (more than 8 sequences) do not fit this shape and depth: two workgroups per CU need 2 x the activations + the layer table in 160 KB of LDS"
                                          : "the model is too deep for this many sequences: the workgroup's activations of every sequence of a decoder + the layer table must fit 160 KB of LDS";
    if (!xengine_form(sh->sc, fmt, n_seq, d->n_layer, false, false)) return KF_UNSUPPORTED_DATATYPE;
    if (dry) {
        *why = "";
        return KF_OK;
    }
    return xe_make(&d, sh, fmt, n_seq, kv_seq_stride, tab, qbias, ws, ws_bytes, st, out, why);
}
int xengine_build_tp(const kf_engine_desc* const* ds, int world, void* ws, size_t ws_bytes, hipStream_t st, XEngineHost** out, const char** why) {
    *why = "bad arguments";
    if (!ds || !ws || !out || world < 1) return KF_INVALID_ARGS;
    *why = "tensor parallel over the XCDs: exactly 8 ranks (one per XCD)";
    if (world != XE_NXCD) return KF_UNSUPPORTED_DATATYPE;
    for (int r = 0; r < world; r++)
        if (!ds[r] || !ds[r]->layers || ds[r]->n_layer < 1 || ds[r]->n_layer != ds[0]->n_layer) return KF_INVALID_ARGS;
    *why = "rank shape not instantiated: built for the TP = 8 ranks of Qwen3-32B (dim 5120, 8 / 1 heads of 128, ffn 3200 per rank), Qwen3-8B (dim 4096, 4 / 1 heads, ffn 1536) and Qwen3-4B with "
           "its FFN padded to 10240 (dim 2560, 4 / 1 heads, ffn 1280)";
    const XShape* sh = xe_shape_of(ds[0], true);
    for (int r = 0; r < world; r++)
        if (!sh || xe_shape_of(ds[r], true) != sh) return KF_UNSUPPORTED_DATATYPE;
    const kf_engine_desc* d = ds[0];
    if (ws_bytes < xengine_ws_bytes_tp(d) || ((uintptr_t)ws & 255) != 0) {
        *why = "workspace too small or not 256-byte aligned";
        return KF_INVALID_ARGS;
    }
    int n_cu = 0;
    *why = "HIP failure";
    if (eng_device_cus(&n_cu) != KF_OK) return KF_HIP_CHECK;
    *why = "the device does not show 256 compute units (8 XCDs of 32): one resident workgroup per CU, 32 per XCD, is the premise";
    if (n_cu != XE_GRID) return KF_UNSUPPORTED_DATATYPE;
    *why = "rope_table missing, kv_stride not a multiple of 8, max_seq < 1, or the ranks disagree";
    for (int r = 0; r < world; r++)
        if (!eng_desc_cache_ok(ds[r]) || ds[r]->max_seq != d->max_seq || ds[r]->kv_stride != d->kv_stride || ds[r]->rms_eps != d->rms_eps ||
            ds[r]->qk_eps != d->qk_eps)
            return KF_INVALID_ARGS;
    *why = "layer storage not served: 4-bit PackedQ (RTN) layers in groups of 128 with 16-byte aligned blocks, dense FFN, every layer and rank the same shapes";
    std::vector<EngLayer> tab((size_t)world * d->n_layer);
    float qbias[7] = {0};
    bool q4p_ok = true;
    for (int r = 0; r < world; r++)
        if (eng_fill_layers(ds[r], tab.data() + (size_t)r * d->n_layer, qbias, r > 0, q4p_ok) != KF_OK) return KF_UNSUPPORTED_DATATYPE;
    if (!q4p_ok) return KF_UNSUPPORTED_DATATYPE;
    return xe_make(ds, sh, FMT_Q4P, XE_NXCD /* decoders = ranks */, 0, tab, qbias, ws, ws_bytes, st, out, why);
}
// the head in vocabulary shards (rank r: rows row0[r] .. of the full matrix), logits: the full vector, the shards in rank order
int xengine_set_head_tp(XEngineHost* E, const kf_weight* const* ws, const int* row0, const uint16_t* norm_w, uint16_t* logits, int32_t* d_tokens_out, int tokens_stride) {
    XArgs& a = E->args;
    if (!E->tp_bytes || !ws || !row0 || !norm_w || !logits) return KF_INVALID_ARGS;
    long at = 0;
    for (int r = 0; r < XE_NXCD; r++) {
        const kf_weight* w = ws[r];
        if (eng_head_rule(w, E->dm.dim, norm_w, logits) != KF_OK || row0[r] != at) return KF_UNSUPPORTED_DATATYPE;
        a.head_w_r[r] = (g_u32x4)(uintptr_t)w->data, a.logits_r[r] = logits + at, a.vocab_r[r] = w->ne0, a.row0_r[r] = row0[r];
        at += w->ne0;
    }
    a.head_w = a.head_w_r[0], a.vocab = a.vocab_r[0], a.logits = logits; /* (head_w: "a head is set") */
    a.head_norm = (g_u16)(uintptr_t)norm_w, a.d_tokens_out = d_tokens_out, a.tokens_stride = tokens_stride;
    return KF_OK;
}
// n_steps decode steps of every sequence in ONE launch; with_head: 0 layers only (x_out), 1 + logits, 2 + greedy pick and state update (needed for n_steps > 1)
int xengine_steps(XEngineHost* E, hipStream_t st, int32_t* d_state, uint16_t* x_out, int with_head, int n_steps) {
    XArgs& a = E->args;
    if (!a.emb || !d_state || !x_out || n_steps < 1 || (n_steps > 1 && with_head != 2)) return KF_INVALID_ARGS;
    if (with_head && !a.head_w) return KF_INVALID_ARGS;
    const XForm* f = xengine_form(E->shape_class, E->fmt, a.n_seq, a.n_layer, a.dbg != nullptr, E->two_wpc != 0);
    if (!f) return KF_UNSUPPORTED_DATATYPE;
    XArgs save = a;
    a.d_state = d_state, a.x_out = x_out, a.n_steps = n_steps, a.pick = with_head == 2 ? 1 : 0;
    a.epoch0 = E->epoch, E->epoch += n_steps; /* generations never repeat between resets (a 31-bit count of steps) */
    if (!with_head) a.head_w = nullptr;
    const int rc = f->go(E, st);
    a.head_w = save.head_w;
    return rc;
}
int xengine_set_embedding(XEngineHost* E, const kf_weight* w, const int32_t* d_forced, int forced_stride) {
    if (eng_embed_rule(w, E->dm.dim) != KF_OK) return KF_UNSUPPORTED_DATATYPE;
    E->args.emb = reinterpret_cast<const uint16_t*>(w->data), E->args.emb_rows = w->ne0, E->args.d_forced = d_forced, E->args.forced_stride = forced_stride;
    return KF_OK;
}
int xengine_set_head(XEngineHost* E, const kf_weight* w, const uint16_t* norm_w, uint16_t* logits, int32_t* d_tokens_out, int tokens_stride) {
    XArgs& a = E->args;
    if (E->tp_bytes) return KF_INVALID_ARGS; /* a TP engine takes its head in vocabulary shards: kf_xengine_set_head_tp */
    if (!w) { /* no head: kf_xengine_steps then refuses (every step of the ABI ends in the head); kept so that a head can be taken away before its weight is freed */
        a.head_w = nullptr, a.head_norm = nullptr, a.logits = nullptr, a.d_tokens_out = nullptr, a.vocab = 0;
        return KF_OK;
    }
    if (eng_head_rule(w, E->dm.dim, norm_w, logits) != KF_OK) return KF_UNSUPPORTED_DATATYPE;
    a.head_w = (g_u32x4)(uintptr_t)w->data, a.head_norm = (g_u16)(uintptr_t)norm_w, a.logits = logits, a.d_tokens_out = d_tokens_out, a.tokens_stride = tokens_stride, a.vocab = w->ne0;
    return KF_OK;
}
int xengine_error_word(XEngineHost* E, hipStream_t st, int* h_err) { return eng_read_error_word(E->args.ws, st, h_err); }
int xengine_reset(XEngineHost* E, hipStream_t st) { return eng_then_sync(xengine_init_state(E, st), st); }
int xengine_set_variant(XEngineHost* E, int nwv, int depth) {
    if (nwv != -2) return -1;
    E->two_wpc = depth != 0; /* A/B hook: depth != 0 = 9 .. 16 sequences through the round-5 form (two decoders per XCD) instead of the batched one */
    return 0;
}
int xengine_debug_enable(XEngineHost* E, int seq, int wg, int max_steps) {
    XArgs& a = E->args;
    const size_t bytes = (size_t)max_steps * a.n_layer * 64 * 8;
    if (a.dbg) (void)hipFree(a.dbg), a.dbg = nullptr;
    if (seq < 0) return KF_OK;
    if (eng_stamps_zeroed(&a.dbg, bytes) != KF_OK) return KF_HIP_CHECK;
    a.dbg_seq = seq, a.dbg_wg = wg, a.dbg_steps = max_steps;
    return KF_OK;
}
int xengine_debug_read(XEngineHost* E, unsigned long long* h_out, int n_words) { return eng_stamps_read(E->args.dbg, h_out, n_words); }

}  // namespace kf
