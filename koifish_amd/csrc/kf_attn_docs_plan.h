// kf_attn_docs_plan.h -- packed documents: kf::attn_docs_plan, one pure host function, turns a document layout (include/kf_abi.h: document d owns rows
// [row0[d], row0[d] + len[d]) of a batch of n_rows rows, ascending and disjoint, every other row a gap row) into the workgroup tables of the three launches that
// read it: kf_attn_prefill_docs (tiles of ATTN_TILE_COLS / GQ tokens) and the two launches of kf_attn_backward_docs (tiles of ATTN_TILE_COLS = 128 rows).  One
// entry per tile {row0, len, tile index in the document, gap}: a workgroup reads its sequence origin, its sequence length and its block from the entry where
// the batch kernels read blockIdx.  Entries are ordered longest key range first -- the rule the kernels follow inside one sequence --; the gap rows come last, as
// entries with gap = 1 over the same tile sizes: the workgroup that draws one writes zeros to its rows and ends, so what is written for gap rows is
// proportional to their number.  kf_attn_docs_plan (the ABI entry) and the launchers both go through here; the launchers check a table's header, never plan.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "kf_attn_plan.h"

namespace kf {

enum { ATTN_DOCS_FWD = 0, ATTN_DOCS_DQ = 1, ATTN_DOCS_DKV = 2 };
static_assert(sizeof(kf_attn_docs_header) == 64 && sizeof(kf_attn_docs_entry) == 16, "table layout");

// rows per tile of the three tables
constexpr int attn_docs_tile(int which, int gq) { return which == ATTN_DOCS_FWD ? ATTN_TILE_COLS / gq : ATTN_TILE_COLS; }
// keys a document tile's workgroup walks: the forward and the dQ launch read keys 0 .. the tile's last row, the dK/dV launch the queries from its first row on
constexpr int attn_docs_walk(int which, int len, int tile, int rows) {
    const int end = (tile + 1) * rows < len ? (tile + 1) * rows : len;
    return which == ATTN_DOCS_DKV ? len - tile * rows : end;
}

struct AttnDocsPlan {
    int status;
    kf_attn_docs_header hdr;
    std::vector<kf_attn_docs_entry> entries; /* the three tables back to back, hdr.off / hdr.n in entries */
    size_t bytes() const { return sizeof(kf_attn_docs_header) + entries.size() * sizeof(kf_attn_docs_entry); }
};

inline AttnDocsPlan attn_docs_plan(const int32_t* row0, const int32_t* len, int n_doc, int n_rows, int max_len, int n_head, int n_kv, int hd) {
    AttnDocsPlan p = {};
    p.status = KF_INVALID_ARGS;
    if (!row0 || !len || n_doc < 1 || n_rows < 1 || max_len < 1) return p;
    AttnProblem P = {};
    P.entry = ATTN_BATCH, P.n_head = n_head, P.n_kv = n_kv, P.hd = hd, P.n_tok = 1, P.n_seq = 1, P.al = ATTN_Q_AL | ATTN_OUT_AL, P.q_stride = P.out_stride = P.kv_stride = 8;
    const AttnPlan fw = attn_plan(P);
    P.entry = ATTN_BACKWARD;
    if (fw.status != KF_OK || attn_plan(P).status != KF_OK) return p;
    long long next = 0, doc_rows = 0; /* the first row the next document may start at */
    for (int d = 0; d < n_doc; d++) {
        if (len[d] < 1 || len[d] > max_len || row0[d] < next || (long long)row0[d] + len[d] > n_rows) return p;
        next = (long long)row0[d] + len[d], doc_rows += len[d];
    }
    const int gq = n_head / n_kv;
    kf_attn_docs_header& h = p.hdr;
    h.magic = KF_ATTN_DOCS_MAGIC, h.n_rows = n_rows, h.n_head = n_head, h.n_kv = n_kv, h.head_dim = hd, h.n_doc = n_doc, h.max_len = max_len;
    h.doc_rows = (int32_t)doc_rows, h.gap_rows = (int32_t)(n_rows - doc_rows);
    for (int which = 0; which < 3; which++) {
        const int rows = attn_docs_tile(which, gq);
        std::vector<kf_attn_docs_entry> e;
        for (int d = 0; d < n_doc; d++)
            for (int t = 0; t * rows < len[d]; t++) e.push_back(kf_attn_docs_entry{row0[d], len[d], t, 0});
        std::stable_sort(e.begin(), e.end(), [&](const kf_attn_docs_entry& a, const kf_attn_docs_entry& b) {
            return attn_docs_walk(which, a.len, a.tile, rows) > attn_docs_walk(which, b.len, b.tile, rows);
        });
        int at = 0; /* the gaps: before every document, and behind the last */
        for (int d = 0; d <= n_doc; d++) {
            const int end = d < n_doc ? row0[d] : n_rows;
            for (int t = 0; t * rows < end - at; t++) e.push_back(kf_attn_docs_entry{at, end - at, t, 1});
            if (d < n_doc) at = row0[d] + len[d];
        }
        h.off[which] = (int32_t)(sizeof(kf_attn_docs_header) / sizeof(kf_attn_docs_entry) + p.entries.size()), h.n[which] = (int32_t)e.size();
        p.entries.insert(p.entries.end(), e.begin(), e.end());
    }
    p.status = KF_OK;
    return p;
}

// what a launcher asks of a table before it launches: a header this rule wrote, for this geometry and this batch
inline bool attn_docs_header_ok(const kf_attn_docs_header* h, int n_head, int n_kv, int hd) {
    if (!h || h->magic != KF_ATTN_DOCS_MAGIC || h->n_head != n_head || h->n_kv != n_kv || h->head_dim != hd || h->n_rows < 1 || h->n_doc < 1) return false;
    for (int w = 0; w < 3; w++)
        if (h->n[w] < 1 || h->off[w] < (int)(sizeof(kf_attn_docs_header) / sizeof(kf_attn_docs_entry))) return false;
    return h->doc_rows + h->gap_rows == h->n_rows;
}
constexpr size_t attn_backward_docs_scratch_bytes(int n_rows, int n_head) { return (n_rows < 1 || n_head < 1) ? 0 : sizeof(float) * 2 * (size_t)n_rows * n_head; }

// the launchers (kf_attn_prefill.hip, kf_attn_bwd_mfma.hip): d_table is the device copy of the whole table, h its header on the host
int attn_prefill_docs_launch(hipStream_t st, const AttnPlan& p, const kf_attn_docs_header& h, const void* d_table, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                             uint16_t* out, long long q_stride, int n_kv, int kv_stride, long long out_stride);
int attn_backward_docs_launch(hipStream_t st, const AttnPlan& p, const kf_attn_docs_header& h, const void* d_table, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                              long long ld_qkv, const uint16_t* o, const uint16_t* dO, long long ld_o, uint16_t* dq, uint16_t* dk, uint16_t* dv, long long ld_d, float* scratch);

}  // namespace kf
