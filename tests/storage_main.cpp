// storage_main.cpp -- koifish_amd/host/kf_storage.hpp and kf_params.hpp alone, as a program (tests/test_storage_cpu.py builds it with AddressSanitizer + UBSan and runs
// it: nothing preloaded).  layout_of over every served form at the smallest shapes where its rule can go wrong, every refusal, sizes at the edge of size_t, the
// comparison a setter makes with a caller's szData / blob_bytes, the factory, and the parameter table's lookups.
#include <climits>
#include <cstdio>

#include "../koifish_amd/host/kf_params.hpp"
#include "../koifish_amd/host/kf_storage.hpp"

using namespace koifish;
static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        n_checks++;                                                  \
        if (!(cond)) n_failed++, printf("FAILED line %d: %s\n", __LINE__, #cond); \
    } while (0)

struct Stand {  // what make_tensor fills
    std::string name;
    typNUMBER type = typNUMBER::BF16;
    int ne[4] = {1, 1, 1, 1};
    QuantCard quant;
    size_t szData = 0, szGama = 0;
};

static Layout lay(typNUMBER t, int64_t ne0, int64_t ne1, int group = 128, bool nf = false, bool rtn = false) {
    QuantCard q = card_of(t, false, nf, group);
    q.isRowRTN = rtn;
    return layout_of(t, q, ne0, ne1);
}
static bool is(const Layout& L, size_t d, size_t g, size_t ng) { return L.status == KF_OK && L.szData == d && L.szGama == g && L.nGroup == ng && L.why.empty(); }
static bool refused(const Layout& L, int st) { return L.status == st && !L.why.empty() && (L.row_shape || L.bytes() == 0); }

int main() {
    CHECK(is(lay(typNUMBER::BF16, 8, 32), 512, 0, 0));
    CHECK(is(lay(typNUMBER::F8E5M2, 8, 32), 256, 0, 0));
    CHECK(is(lay(typNUMBER::Q4, 8, 128), 512, 304, 8));
    CHECK(is(lay(typNUMBER::Q4, 16, 256), 2048, 672, 32));
    CHECK(is(lay(typNUMBER::Q2, 8, 128), 256, 304, 8));
    CHECK(is(lay(typNUMBER::T_SIGN, 8, 128), 256, 304, 8));
    CHECK(is(lay(typNUMBER::T_BINARY, 8, 128), 128, 304, 8));
    CHECK(is(lay(typNUMBER::BOOL1, 8, 128), 128, 304, 8));
    CHECK(is(lay(typNUMBER::Q4, 8, 32, 0, true), 128, 336, 0));
    CHECK(is(lay(typNUMBER::Q3, 8, 128, 0, true), 384, 400, 0));
    CHECK(is(lay(typNUMBER::Q2, 8, 128, 0, true), 256, 336, 0));
    CHECK(is(lay(typNUMBER::Q2, 8, 128, 0, true, true), 256, 304, 0));
    // refusals
    CHECK(refused(lay(typNUMBER::Q4, 8, 128, 0), KF_QUANT_ERR));
    CHECK(refused(lay(typNUMBER::T_SIGN, 8, 128, -4), KF_QUANT_ERR));
    CHECK(refused(lay(typNUMBER::Q4, 8, 40), KF_QUANT_ERR));
    CHECK(refused(lay(typNUMBER::Q4, 8, 96, 512), KF_QUANT_ERR));
    CHECK(refused(lay(typNUMBER::Q3, 8, 128), KF_UNSUPPORTED_DATATYPE)); /* Q3 in groups */
    CHECK(refused(lay(typNUMBER::F32, 8, 32), KF_UNSUPPORTED_DATATYPE));
    CHECK(refused(lay(typNUMBER::T_SIGN, 8, 128, 0, true), KF_UNSUPPORTED_DATATYPE));
    CHECK(refused(lay(typNUMBER::Q4, 8, 32, 0, true, true), KF_UNSUPPORTED_DATATYPE));
    for (const Layout& L : {lay(typNUMBER::Q4, 8, 48, 0, true), lay(typNUMBER::Q4, 12, 32, 0, true), lay(typNUMBER::Q3, 8, 64, 0, true), lay(typNUMBER::Q3, 12, 128, 0, true)}) {
        CHECK(refused(L, KF_BLAS_UNALIGN) && L.row_shape && L.bytes() > 0);
        CHECK(L.code(KF_QUANT_ERR) == KF_QUANT_ERR && L.code(KF_UNSUPPORTED_DATATYPE) == KF_UNSUPPORTED_DATATYPE);
    }
    CHECK(lay(typNUMBER::Q4, 8, 48, 0, true).szData == 192 && lay(typNUMBER::Q4, 8, 48, 0, true).szGama == 368);
    CHECK(lay(typNUMBER::Q4, 8, 40).code(KF_BLAS_UNALIGN) == KF_QUANT_ERR); /* only the row-shape refusal takes the site's code */
    CHECK(nf4_shape_ok(8, 32) && !nf4_shape_ok(8, 48) && !nf4_shape_ok(12, 32) && nf3_shape_ok(8, 128) && !nf3_shape_ok(8, 64) && !nf3_shape_ok(12, 128));
    // extreme shapes: refused, never wrapped
    const int64_t big = (int64_t)1 << 40, i31 = INT_MAX;
    CHECK(refused(lay(typNUMBER::BF16, 0, 32), KF_INVALID_ARGS) && refused(lay(typNUMBER::BF16, 8, -1), KF_INVALID_ARGS));
    CHECK(refused(lay(typNUMBER::BF16, big, big), KF_INVALID_ARGS));
    CHECK(refused(lay(typNUMBER::Q4, (int64_t)1 << 31, (int64_t)1 << 31), KF_INVALID_ARGS));          /* n = 2^62: n * bits wraps */
    CHECK(refused(lay(typNUMBER::BF16, (int64_t)1 << 32, (int64_t)1 << 31), KF_INVALID_ARGS));        /* n * 2 = 2^64 */
    CHECK(refused(lay(typNUMBER::Q4, LLONG_MAX, 1, 1), KF_INVALID_ARGS) && refused(lay(typNUMBER::Q4, LLONG_MAX, LLONG_MAX, 0, true), KF_INVALID_ARGS));
    CHECK(is(lay(typNUMBER::F8E5M2, i31, i31), (size_t)i31 * i31, 0, 0));
    CHECK(lay(typNUMBER::Q4, i31, 128).status == KF_OK && lay(typNUMBER::Q4, i31, 128).szData == (size_t)i31 * 64);
    // a caller's sizes against the layout: compared, never subtracted
    const Layout q4 = lay(typNUMBER::Q4, 8, 128);
    CHECK(q4.fits(512, 816) && !q4.fits(512, 816 - 4) && !q4.fits(512, 100) /* blob_bytes < szData */ && !q4.fits(900, 816) && !q4.fits(0, 0) && !q4.fits(816, 512));
    // the card
    auto card = [](typNUMBER t, bool sym, bool nf, int b, int lo, int hi, int bias) {
        const QuantCard q = card_of(t, sym, nf, 128);
        return q.bits == b && q.qMin == lo && q.qMax == hi && q.qBias == bias && q.isNormalFloat == nf && q.T_group == (nf ? 0 : 128);
    };
    CHECK(card(typNUMBER::BF16, false, false, 16, 0, 0, 0) && card(typNUMBER::F8E5M2, false, false, 8, 0, 0, 0) && card(typNUMBER::Q4, false, false, 4, 0, 15, 0));
    CHECK(card(typNUMBER::Q4, true, false, 4, -8, 7, 8) && card(typNUMBER::Q4, false, true, 4, 0, 15, 0) && card(typNUMBER::Q3, false, true, 3, 0, 7, 0));
    CHECK(card(typNUMBER::Q2, false, true, 2, 0, 3, 0) && card(typNUMBER::T_SIGN, false, false, 2, -1, 1, 1) && card(typNUMBER::BOOL1, false, false, 1, 0, 1, 0));
    CHECK(card(typNUMBER::T_BINARY, false, false, 1, 0, 1, 0));
    // the factory
    Layout L;
    auto t = make_tensor<Stand>("w", typNUMBER::Q4, card_of(typNUMBER::Q4, true, false, 128), 16, 256, L);
    CHECK(t && t->name == "w" && t->type == typNUMBER::Q4 && t->ne[0] == 16 && t->ne[1] == 256 && t->szData == 2048 && t->szGama == 672 && t->quant.qBias == 8);
    CHECK(!make_tensor<Stand>("w", typNUMBER::Q4, card_of(typNUMBER::Q4, false, false, 0), 16, 256, L) && L.status == KF_QUANT_ERR);
    // the table
    MODEL_CARD c;
    c.nEmbed = 256, c.nLayer = 2, c.n_head = 4, c.n_head_kv = 2, c.head_dim = 64, c.n_ff = 512, c.vocab = 512;
    const std::vector<Param> tab = param_table(c);
    CHECK(tab.size() == 25 && tab.front().kind == P_EMBED && tab.back().kind == P_HEAD && !tab.back().required);
    const Param* p = find_param(tab, false, 1, 3);
    CHECK(p && p->name == "model.layers.1.self_attn.o_proj.weight" && p->ne0 == 256 && p->ne1 == 256);
    p = find_param(tab, true, 1, 3);
    CHECK(p && p->name == "model.layers.1.self_attn.k_norm.weight" && p->ne0 == 64 && p->ne1 == 1 && !p->required);
    CHECK(find_param(tab, false, -1, 0) == &tab.front() && find_param(tab, false, -1, 1) == &tab.back() && find_param(tab, true, -1, 0)->name == "model.norm.weight");
    CHECK(!find_param(tab, false, 0, 7) && !find_param(tab, false, -1, 2) && !find_param(tab, true, 0, 4) && !find_param(tab, false, 2, 0) && !find_param(tab, true, -1, 1) &&
          !find_param(tab, false, -2, 0));
    c.tie_word_embeddings = false;
    CHECK(head_is_tied(c, false) && !head_is_tied(c, true));
    c.tie_word_embeddings = true;
    CHECK(head_is_tied(c, true));
    printf("storage_main: %d checks, %d failed\n", n_checks, n_failed);
    return n_failed ? 1 : 0;
}
