// kf_storage.hpp -- how a stored weight is laid out, stated once: the quant card of a type, the shape conditions of the row forms, the bytes of `data||gama`, and the one
// factory that fills a tensor's type / ne / quant / szData / szGama.  Plain C++17: no HIP, no Fish, no kf_ctx (tests/storage_main.cpp builds it alone); kf_abi.h gives
// the status codes only.  Every loader (Hugging Face, .kun, the kfh_set_* entries) and Python (kfh_weight_layout / kfh_quant_card) ask here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>

#include "../../include/kf_abi.h"
#include "../csrc/kf_f8b_plan.h" /* the e4m3 block-scaled form's shape rule, stated there (plain C++) */

namespace koifish {

enum class typNUMBER : uint8_t { F32 = 0, F64, F16, BF16, F8E5M2, F8E4M3, U8, I8, U16, I16, U32, I32, U64, I64, Q4, Q3, Q2, T_SIGN, T_SEQ, BOOL1, T_BINARY };

// Quant card fields that cross the kernel seam (QUANT_CARD / GeQuant, GeQuant.cpp:107-124)
struct QuantCard {
    int bits = 16, T_group = 128, qMin = 0, qMax = 0, qBias = 0;
    bool isNormalFloat = false;  // QUANT_MODE::RTNf (GeQuant.cpp:853): row-codebook storage -> kf_weight.quant = KF_QUANT_ROW_LUT
    bool isRowRTN = false;       // KF_QUANT_ROW_RTN: (zero, step) per row in place of the codebook (2-bit, operator-level storage; implies isNormalFloat's row layout)
};

inline bool is_quant_type(typNUMBER t) { return t == typNUMBER::Q4 || t == typNUMBER::Q3 || t == typNUMBER::Q2 || t == typNUMBER::T_SIGN || t == typNUMBER::T_BINARY || t == typNUMBER::BOOL1; }

// ---- the card (GeQuant ctor, GeQuant.cpp:107-124).  normal_float: the row forms of Q4 / Q3 / Q2 (RT_NormalF), which have no groups
inline QuantCard card_of(typNUMBER t, bool symmetric, bool normal_float, int lGroup) {
    QuantCard q;
    q.isNormalFloat = normal_float, q.T_group = normal_float ? 0 : lGroup;
    switch (t) {
        case typNUMBER::Q4: q.bits = 4; if (symmetric) q.qMin = -8, q.qMax = 7, q.qBias = 8; else q.qMax = 15; break;
        case typNUMBER::Q3: q.bits = 3, q.qMax = 7; break; /* the normal-float row form only (RT_NormalF with bits == 3) */
        case typNUMBER::Q2: q.bits = 2, q.qMax = 3; break;
        case typNUMBER::T_SIGN: q.bits = 2, q.qMin = -1, q.qMax = 1, q.qBias = 1; break;
        case typNUMBER::BOOL1: case typNUMBER::T_BINARY: q.bits = 1, q.qMax = 1; break;
        case typNUMBER::F8E5M2: case typNUMBER::F8E4M3: q.bits = 8; break;
        default: break;
    }
    return q;
}

// ---- the shape conditions of the row forms the decode path multiplies: [ne0 = out][ne1 = in]
inline bool nf4_shape_ok(int64_t ne0, int64_t ne1) { return ne1 % 32 == 0 && ne0 % 8 == 0; }
inline bool nf3_shape_ok(int64_t ne0, int64_t ne1) { return ne1 % 128 == 0 && ne0 % 8 == 0; } /* whole 32-weight units per lane, 16-byte aligned row tables */
inline const char* row_shape_rule(int bits) {
    return bits == 3 ? "the 3-bit normal-float row form needs in % 128 == 0 and out % 8 == 0 (whole 32-weight units, aligned row tables)"
                     : "the normal-float row form needs in % 32 == 0 and out % 8 == 0";
}
inline size_t group_count(const QuantCard& q, size_t n) { return !q.isNormalFloat && q.T_group > 0 ? n / (size_t)q.T_group : 0; }

// ---- the layout.  status: KF_OK, or KF_QUANT_ERR (the group), KF_UNSUPPORTED_DATATYPE (a type or form the decode path does not serve), KF_INVALID_ARGS (a size that is
// not positive or overflows), and for a row form whose shape condition fails KF_BLAS_UNALIGN with row_shape set: a site that answers that refusal with a code of its own
// asks code(its code).  The sizes of a row_shape refusal are filled all the same: operators outside the decode path take such a stream.
struct Layout {
    size_t szData = 0, szGama = 0, nGroup = 0;
    int status = KF_OK;
    bool row_shape = false;
    std::string why;
    size_t bytes() const { return szData + szGama; }
    bool fits(size_t data, size_t blob) const { return data == szData && blob == bytes(); } /* a caller's szData / blob_bytes: compared, never subtracted */
    int code(int row_shape_code) const { return row_shape ? row_shape_code : status; }
};

inline Layout layout_of(typNUMBER type, const QuantCard& q, int64_t ne0, int64_t ne1) {
    Layout L;
    auto refuse = [&](int st, const std::string& why) {
        L.status = st, L.why = why;
        if (!L.row_shape) L.szData = L.szGama = L.nGroup = 0;
        return L;
    };
    bool ok = ne0 > 0 && ne1 > 0;
    auto mul = [&](size_t a, size_t b) { size_t r = 0; ok = ok && !__builtin_mul_overflow(a, b, &r); return r; };
    auto add = [&](size_t a, size_t b) { size_t r = 0; ok = ok && !__builtin_add_overflow(a, b, &r); return r; };
    if (!ok) return refuse(KF_INVALID_ARGS, "shape " + std::to_string(ne0) + " x " + std::to_string(ne1));
    const size_t r = (size_t)ne0, c = (size_t)ne1, n = mul(r, c), rc = add(r, c);
    if (type == typNUMBER::BF16 || type == typNUMBER::F8E5M2) {
        L.szData = type == typNUMBER::BF16 ? mul(n, 2) : n;
    } else if (type == typNUMBER::F8E4M3) { /* a byte per weight || fp32 [ceil(ne0 / 128)][ne1 / 128] block scales (kf_weight.qscales); nGroup: their number */
        if (!kf::f8b_shape_ok(ne0, ne1)) return refuse(KF_BLAS_UNALIGN, kf::f8b_shape_rule());
        L.szData = n, L.nGroup = (size_t)kf::f8b_scale_count(ne0, ne1), L.szGama = mul(L.nGroup, 4);
    } else if (!is_quant_type(type) || (type == typNUMBER::Q3 && !q.isNormalFloat)) {
        return refuse(KF_UNSUPPORTED_DATATYPE, type == typNUMBER::Q3 ? "Q<3> is served as the normal-float row form only" : "type " + std::to_string((int)type) + " is not served by the decode path");
    } else if (q.isNormalFloat) { /* `bits`-wide stream || [R_SCALE ne0][C_SCALE ne1][LUT ne0 x 2^bits], or (zero, step) per row */
        if (type != typNUMBER::Q4 && type != typNUMBER::Q3 && type != typNUMBER::Q2) return refuse(KF_UNSUPPORTED_DATATYPE, "row codebooks exist at 4, 3 and 2 bits");
        if (q.isRowRTN && q.bits != 2) return refuse(KF_UNSUPPORTED_DATATYPE, "(zero, step) per row exists at 2 bits");
        L.szData = mul(n, (size_t)q.bits) / 8;
        L.szGama = mul(add(rc, mul(r, q.isRowRTN ? 2 : (size_t)1 << q.bits)), 2);
        L.row_shape = ok && ((q.bits == 4 && !nf4_shape_ok(ne0, ne1)) || (q.bits == 3 && !nf3_shape_ok(ne0, ne1)));
    } else { /* packed groups || [R_SCALE ne0][C_SCALE ne1][ZERO nGroup][STEP nGroup] */
        if (q.T_group <= 0) return refuse(KF_QUANT_ERR, "group size " + std::to_string(q.T_group));
        if (ok && n % (size_t)q.T_group) return refuse(KF_QUANT_ERR, "size is not a multiple of the group size " + std::to_string(q.T_group));
        L.nGroup = group_count(q, n);
        L.szData = mul(n, (size_t)q.bits) / 8;
        L.szGama = mul(add(rc, mul(2, L.nGroup)), 2);
    }
    add(L.szData, L.szGama);
    if (!ok) return L.row_shape = false, refuse(KF_INVALID_ARGS, "the size of " + std::to_string(ne0) + " x " + std::to_string(ne1) + " overflows");
    if (L.row_shape) return refuse(KF_BLAS_UNALIGN, row_shape_rule(q.bits));
    return L;
}

// ---- the factory: the one place that assigns a weight tensor's type, ne, quant, szData and szGama (Tensor: GTensor, or a test's stand-in).  NULL when the layout refuses
template <class Tensor>
std::shared_ptr<Tensor> make_tensor(const std::string& name, typNUMBER type, const QuantCard& card, int ne0, int ne1, Layout& lay) {
    lay = layout_of(type, card, ne0, ne1);
    if (lay.status != KF_OK) return nullptr;
    auto t = std::make_shared<Tensor>();
    t->name = name, t->type = type, t->ne[0] = ne0, t->ne[1] = ne1;
    t->quant = card, t->szData = lay.szData, t->szGama = lay.szGama;
    return t;
}

}  // namespace koifish
