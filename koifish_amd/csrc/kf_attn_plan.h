// kf_attn_plan.h -- how attention is launched: kf::attn_plan, one pure host function, picks the route, kernel form, slices, grid, threads, LDS and scratch of every
// attention launch (kf_attn_decode / kf_attn_block, kf_attn_block_kv8, kf_attn_prefill, kf_attn_prefill_kv8, kf_attn_prefill_batch(_strided), kf_attn_backward); the launchers (kf_attn.hip,
// kf_attn_kv8.hip, kf_attn_prefill.hip, kf_attn_prefill_kv8.hip, kf_attn_bwd_mfma.hip) carry out what it returns and decide nothing.  attn_slices is the one slice rule: the decode engine reads it too.
// The Attn*Lds layouts are the ONE statement of every attention kernel's dynamic LDS: the plan's size and the kernels' pointers both come from them.
#pragma once
#include "kf_kernels.h"

namespace kf {

// ---- the thresholds
// ~64 keys per slice: short contexts in ONE slice per kv-head (no cross-workgroup hand-off), long ones cut so that the chip is covered, at most 512 / n_kv and
// KF_ATTN_MAX_SPLITS (the scratch layout) slices (the round-1 sweeps)
constexpr int ATTN_SLICE_KEYS = 64, ATTN_ONE_SLICE_KEYS = 192, ATTN_SLICE_WGS = 512;
// one 64-key batch per 4-wave workgroup (one wave per SIMD: the kernel is bound by VALU issue inside a latency chain, so spreading the keys over more CUs beats more
// waves per CU); 8 waves once the slices of a kv-head with at most ATTN_NW8_GQ query heads grow past ATTN_NW8_KEYS keys
constexpr int ATTN_NW8_KEYS = 128, ATTN_NW8_GQ = 2;
// the canonical order deals the query heads of GQA-4 / GQA-8 to workgroups of two: 8 heads in one workgroup need 411 registers (one wave per SIMD), 2 need 224
constexpr int ATTN_CANON_GQ_WG = 2;
constexpr int ATTN_VERIFY_MAX = 8; /* queries of one verify launch (kf_attn_decode_rows): the rows of kf_gemv_rows_plan.h */
// arrival counters at the head of the decode scratch, at most 64 ints apart: the counters of two (kv-head, part) on different cache lines (atomics on one line serialise)
constexpr int KF_ATTN_CNT_BYTES = 16384, ATTN_CNT_STRIDE_MAX = 64;
// prompts: the MFMA tile kernel (128 (token, query head) columns per workgroup, as in the backward) from 8 tokens; fewer: one slice of the decode kernel per token
constexpr int ATTN_TILE_MIN_TOK = 8, ATTN_TILE_COLS = 128;
// the paired form (two key halves per workgroup) at about one workgroup per CU or fewer: the launch lasts as long as its last query block (2047 tokens, 16 / 8 heads
// x 128: 81 -> 67 us); with more workgroups the halves only compete for the CU (8 x 1024 x 25 x 64: 130 vs 143 us); short prompts take a few us either way
constexpr long ATTN_PAIR_MAX_WGS = 320;
constexpr int ATTN_PAIR_MIN_TOK = 256;
constexpr int AP_KT = 32, AP_KT_LONG = 64; /* keys per staged tile: tile kernel, paired form */
constexpr int AP_KPAD = 8, AP_VPAD = 32;   /* K and V row padding, elements (16 B; 64 B: rows 4 apart in a transposing read land on distinct 16-bank groups) */
// the int8 cache (kf_attn_kv8.hip): a lane holds 16 elements of a key, so a key takes hd / 16 lanes and a wave step twice the keys of the bf16 kernel; the slices are
// attn_slices' (one rule), 4 waves always, ATTN_KV8_U tiles in flight per wave: one 64-key slice of hd = 128 is one batch of the workgroup (4 waves x 8 keys x 2 tiles)
constexpr int ATTN_KV8_NW = 4, ATTN_KV8_U = 2;
// prompts on the int8 cache (kf_attn_prefill_kv8.hip): 64 (token, query head) columns per workgroup, 16 per wave (the N of v_mfma_i32_16x16x64_i8); key tiles of 64
// anchored at key 0; K8 rows 16 bytes apart from a multiple of 128 (the 16 rows of an A read on distinct banks), bf16 V rows 32 bytes (the 8 rows of a transposing pass)
constexpr int APK8_COLS = 64, APK8_KT = 64, APK8_KPAD = 16, APK8_VPAD = 16;

// ---- the slice rule: slices, keys per slice and waves of the decode kernel for keys 0 .. pos_bound (one_slice: the per-token form)
struct AttnSlices {
    int n_splits, chunk, nw;
};
constexpr AttnSlices attn_slices(int pos_bound, int n_kv, int gq, bool one_slice = false) {
    const int len = pos_bound + 1, cap = ATTN_SLICE_WGS / n_kv;
    int nsp = 1;
    if (!one_slice && len > ATTN_ONE_SLICE_KEYS) {
        nsp = (len + ATTN_SLICE_KEYS - 1) / ATTN_SLICE_KEYS;
        if (nsp > cap) nsp = cap < 1 ? 1 : cap;
        if (nsp > KF_ATTN_MAX_SPLITS) nsp = KF_ATTN_MAX_SPLITS;
    }
    const int chunk = (len + nsp - 1) / nsp;
    return AttnSlices{nsp, chunk, gq <= ATTN_NW8_GQ && chunk > ATTN_NW8_KEYS ? 8 : 4};
}
// scratch: the decode kernel's {O[hd], L, m} fp64 partials per (head, slice) behind the counters; the backward's L and D per (sequence, head, row)
constexpr size_t attn_decode_scratch_bytes(int n_head, int hd) { return sizeof(double) * (size_t)n_head * KF_ATTN_MAX_SPLITS * (hd + 2) + KF_ATTN_CNT_BYTES; }
constexpr size_t attn_backward_scratch_bytes(int T, int n_head, int n_seq) { return (T < 1 || n_head < 1 || n_seq < 1) ? 0 : sizeof(float) * 2 * (size_t)T * n_head * n_seq; }

// ---- the LDS layouts, ONE statement per kernel: every buffer's byte offset in the dynamic LDS and the total.  attn_plan takes p.lds from `bytes`, the kernel its
// pointers from the offsets and asserts fits() for the form it is.  take() hands out the buffers back to back in the order of the members and notes whether each starts
// on its alignment: 8 for the fp64 partials (and the rows stored as float2), 4 for floats and ints, 16 for the rows read or written with 128-bit LDS accesses.
constexpr int ATTN_LDS_MAX = 64 * 1024, ATTN_TILE_LDS_MAX = 160 * 1024; /* what a launcher can ask for; attn_prefill_mfma_launch raises the tile kernel to the second */
struct AttnLds {
    int bytes = 0;
    bool sound = true; /* every buffer aligned, every alias inside what it lies over */
    constexpr int take(int n, int align) { return sound = sound && bytes % align == 0, bytes += n, bytes - n; }
    constexpr bool fits(int max = ATTN_LDS_MAX) const { return sound && bytes <= max; }
};
struct AttnCanonLds : AttnLds { /* attn_kernel<gq, nw, hd> */
    int comb, qb, knew, flag;   /* [nw][gq][hd + 2] the waves' {O[hd], L, m} doubles; [gq][hd] prepared q heads and [hd] the new key, bf16 bits; the merge flag */
    constexpr AttnCanonLds(int gq, int nw, int hd) : comb(take(8 * nw * gq * (hd + 2), 8)), qb(take(2 * gq * hd, 16)), knew(take(2 * hd, 16)), flag(take(16, 4)) {}
};
struct AttnFastLds : AttnLds { /* attn_fast_kernel<gq, nw, hd> */
    int qb, knew, wmax, flag, comb; /* q heads and new key as above; [nw][gq] the waves' batch maxima; the flag; [nw][gq][hd + 4] floats {acc[hd], m, l, pad, pad} */
    constexpr AttnFastLds(int gq, int nw, int hd)
        : qb(take(2 * gq * hd, 16)), knew(take(2 * hd, 16)), wmax(take(4 * nw * gq, 4)), flag(take(16, 4)), comb(take(4 * nw * gq * (hd + 4), 8)) {}
};
struct AttnKv8Lds : AttnLds { /* attn_kv8_kernel<gq, hd>, ATTN_KV8_NW waves */
    int comb, qb, knew;              /* as attn_kernel's */
    int q8, k8n, v8n, stp, flag;     /* [gq][hd] the q heads' codes, [hd] the new K row's, [hd] the new V row's; [gq] q steps, then the new K and V rows'; the merge flag */
    constexpr AttnKv8Lds(int gq, int hd)
        : comb(take(8 * ATTN_KV8_NW * gq * (hd + 2), 8)), qb(take(2 * gq * hd, 16)), knew(take(2 * hd, 16)), q8(take(gq * hd, 16)), k8n(take(hd, 16)), v8n(take(hd, 16)),
          stp(take(4 * (gq + 2), 4)), flag(take(16, 4)) {}
};
struct AttnTileLds : AttnLds { /* attn_prefill_kernel<hd, gq, kh, kt> */
    int ks, vt, half; /* 2 x [kt][hd + AP_KPAD] K tiles and 2 x [kt][hd + AP_VPAD] V tiles of key half 0, bf16; key half 1: the same, `half` bytes on */
    int ex, ex_rows;  /* kh = 2, after the key walk: the odd half's (O, M, l), ex_rows rows of 256 floats, OVER the tiles from the start of the buffer */
    constexpr AttnTileLds(int hd, int kh, int kt) : ks(take(2 * 2 * kt * (hd + AP_KPAD), 16)), vt(take(2 * 2 * kt * (hd + AP_VPAD), 16)), half(bytes), ex(0), ex_rows(hd / 2 + 2) {
        bytes = kh * half;
        sound = sound && half % 16 == 0 && (kh == 1 || ex + 4 * ex_rows * 256 <= bytes);
    }
};
struct AttnTileKv8Lds : AttnLds { /* attn_prefill_kv8_kernel<hd, gq> */
    int kt8, vt, kst, vst; /* [KT][hd + KPAD] the K8 tile; [KT][hd + VPAD] the V tile, bf16 bits; [KT] K steps and, right behind them (one store fills both), [KT] V steps */
    int q8, sqs, qb;       /* [COLS][hd] query codes, [COLS] query steps; prologue only: [COLS][hd] bf16 query heads IN the V tile, which is not staged yet */
    constexpr AttnTileKv8Lds(int hd)
        : kt8(take(APK8_KT * (hd + APK8_KPAD), 16)), vt(take(2 * APK8_KT * (hd + APK8_VPAD), 16)), kst(take(4 * APK8_KT, 16)), vst(take(4 * APK8_KT, 16)),
          q8(take(APK8_COLS * hd, 16)), sqs(take(4 * APK8_COLS, 4)), qb(vt) {
        sound = sound && qb + 2 * APK8_COLS * hd <= kst;
    }
};

// ---- the problem
enum { ATTN_DECODE = 0, ATTN_PROMPT = 1, ATTN_BATCH = 2, ATTN_BACKWARD = 3, ATTN_DECODE_KV8 = 4, ATTN_PROMPT_KV8 = 5, ATTN_VERIFY = 6 };
enum { ATTN_Q_AL = 1, ATTN_OUT_AL = 2 }; /* q 16-byte aligned, out 8-byte aligned */
struct AttnProblem {
    int entry, n_head, n_kv, hd;
    int pos;                                   /* ATTN_DECODE: the position bound; ATTN_PROMPT: the first token's */
    int n_tok, n_seq, canon, al;               /* tokens per sequence (the backward's T), sequences, the canonical order, ATTN_Q_AL | ATTN_OUT_AL */
    long long q_stride, out_stride, kv_stride; /* elements between rows; out_stride 0: q_stride */
};
// ---- the plan, by route:
//   ATTN_SLICED     attn_kernel (canon) / attn_fast_kernel <gq, nw, hd> on (n_splits, n_kv * gq_split, 1); the last workgroup of a (kv-head, part) merges the slices
//                   (ATTN_VERIFY: the canonical kernel's ROWS form on (n_splits of the last query, n_kv * gq_split, n_tok), scratch per query)
//   ATTN_PER_TOKEN  the same kernels on (1, n_kv * gq_split, n_tok), no scratch
//   ATTN_TILE / ATTN_PAIRED  attn_prefill_kernel<hd, gq, kh, kt> on (blocks, n_kv, n_seq); kh = 2: a block from the front and one from the back per workgroup
//   ATTN_BWD        attn_bwd_dq_mfma_kernel<hd> on grid, then attn_bwd_dkv_mfma_kernel<hd> on grid_kv
//   ATTN_SLICED_KV8 attn_kv8_kernel<gq, hd> on (n_splits, n_kv * gq_split, 1), ATTN_KV8_NW waves; slices, counters and scratch as ATTN_SLICED in the canonical order
//   ATTN_TILE_KV8   attn_prefill_kv8_kernel<hd, gq> on (blocks of 64 / gq tokens, n_kv, 1), four waves, no scratch; gq = the query heads of a kv-head, any n_tok >= 1
enum { ATTN_SLICED = 0, ATTN_PER_TOKEN = 1, ATTN_TILE = 2, ATTN_PAIRED = 3, ATTN_BWD = 4, ATTN_SLICED_KV8 = 5, ATTN_TILE_KV8 = 6 };
struct AttnPlan {
    int status, route;             /* KF_OK or the refusal; the route (of a refusal: the one that refused) */
    int canon, gq, nw, hd, kh, kt; /* the kernel form; gq = query heads per workgroup */
    int gq_split, n_splits, chunk, cnt_stride;
    int grid[3], grid_kv[3], threads, lds;
    long long scratch; /* bytes the route needs */
};

inline AttnPlan attn_plan(const AttnProblem& P) {
    AttnPlan p = {};
    auto refuse = [&p](int status) { return p.status = status, p; };
    const bool kv_ok = P.n_kv > 0 && P.n_head % P.n_kv == 0, hd_ok = P.hd == 64 || P.hd == 128;
    const int GQ = kv_ok ? P.n_head / P.n_kv : 0;
    const bool gq_ok = GQ == 1 || GQ == 2 || GQ == 4 || GQ == 8;
    p.hd = P.hd, p.gq = GQ;
    // the sliced geometry of the decode kernels (s: the slices, nw waves, n_tok tokens on grid z): the canonical order's query heads dealt to workgroups of
    // ATTN_CANON_GQ_WG, the counter stride (refused below 1), grid, threads, and the hand-off's scratch; false: refused
    auto sliced = [&](bool canon, const AttnSlices& s, int nw, int n_tok, bool hand_off) {
        p.canon = canon, p.gq_split = canon && GQ > ATTN_CANON_GQ_WG ? GQ / ATTN_CANON_GQ_WG : 1;
        p.cnt_stride = KF_ATTN_CNT_BYTES / 4 / (P.n_kv * p.gq_split);
        if (p.cnt_stride > ATTN_CNT_STRIDE_MAX) p.cnt_stride = ATTN_CNT_STRIDE_MAX;
        if (p.cnt_stride < 1) return refuse(KF_INVALID_ARGS), false;
        p.gq = GQ / p.gq_split, p.nw = nw, p.n_splits = s.n_splits, p.chunk = s.chunk, p.threads = 64 * nw;
        p.grid[0] = s.n_splits, p.grid[1] = P.n_kv * p.gq_split, p.grid[2] = n_tok;
        p.scratch = hand_off ? (long long)attn_decode_scratch_bytes(P.n_head, P.hd) : 0;
        return true;
    };
    if (P.entry == ATTN_BACKWARD) {
        p.route = ATTN_BWD;
        if (!hd_ok || !kv_ok) return refuse(KF_UNSUPPORTED_DATATYPE);
        p.grid[0] = p.grid_kv[0] = (P.n_tok + ATTN_TILE_COLS - 1) / ATTN_TILE_COLS, p.grid[1] = P.n_head, p.grid_kv[1] = P.n_kv, p.grid[2] = p.grid_kv[2] = P.n_seq;
        p.threads = 256, p.scratch = (long long)attn_backward_scratch_bytes(P.n_tok, P.n_head, P.n_seq);
        return p;
    }
    if (P.entry == ATTN_DECODE_KV8) { /* one token against the int8 cache: ONE arithmetic (P.canon is not read), the canonical order's two query heads per workgroup */
        p.route = ATTN_SLICED_KV8;
        if (!hd_ok || !kv_ok || !gq_ok || P.pos < 0) return refuse(KF_INVALID_ARGS);
        if (P.kv_stride & 15) return refuse(KF_BLAS_UNALIGN);
        if (!sliced(true, attn_slices(P.pos, P.n_kv, GQ), ATTN_KV8_NW, 1, true)) return p;
        p.lds = AttnKv8Lds(p.gq, P.hd).bytes;
        return p;
    }
    if (P.entry == ATTN_PROMPT_KV8) { /* a token batch against the int8 cache: ONE arithmetic and ONE form for every n_tok >= 1 (P.canon is not read) */
        p.route = ATTN_TILE_KV8;
        if (!hd_ok || !kv_ok || !gq_ok || P.pos < 0 || P.n_tok < 1) return refuse(KF_INVALID_ARGS);
        if ((P.kv_stride & 15) || (P.q_stride & 7) || !(P.al & ATTN_Q_AL) || !(P.al & ATTN_OUT_AL)) return refuse(KF_BLAS_UNALIGN); /* 16-byte q and K8 / V8 rows, 8-byte out rows */
        const int TQ = APK8_COLS / GQ;
        p.canon = 1, p.kh = 1, p.kt = APK8_KT, p.threads = 256;
        p.grid[0] = (P.n_tok + TQ - 1) / TQ, p.grid[1] = P.n_kv, p.grid[2] = 1;
        p.lds = AttnTileKv8Lds(P.hd).bytes;
        return p;
    }
    if (P.entry == ATTN_VERIFY) { /* n_tok consecutive queries of one sequence, query r at pos + r against keys 0 .. pos + r: the sliced decode kernel with the query on
                                     grid z.  Canonical order only: every z takes attn_slices at its own position inside the kernel, the grid's x and the waves are
                                     the last row's (the slice count never falls as the position grows), the hand-off scratch is one decode scratch per row */
        p.route = ATTN_SLICED;
        if (!hd_ok || !kv_ok || !gq_ok || P.pos < 0 || P.n_tok < 1 || P.n_tok > ATTN_VERIFY_MAX || !P.canon) return refuse(KF_INVALID_ARGS);
        const AttnSlices s = attn_slices(P.pos + P.n_tok - 1, P.n_kv, GQ);
        if (!sliced(true, s, s.nw, P.n_tok, true)) return p;
        p.scratch *= P.n_tok;
        p.lds = AttnCanonLds(p.gq, p.nw, P.hd).bytes;
        return p;
    }
    // the tile kernel: 16-byte q and K / V rows, 8-byte out rows
    const long long out_stride = P.out_stride > 0 ? P.out_stride : P.q_stride;
    const bool tile_ok = !(out_stride & 3) && hd_ok && kv_ok && !(P.q_stride & 7) && !(P.kv_stride & 7) && (P.al & ATTN_Q_AL) && (P.al & ATTN_OUT_AL) && gq_ok;
    if (P.entry == ATTN_BATCH || (P.entry == ATTN_PROMPT && P.n_tok >= ATTN_TILE_MIN_TOK && tile_ok)) {
        p.route = ATTN_TILE;
        if (!tile_ok) return refuse(KF_INVALID_ARGS);
        const int TQ = ATTN_TILE_COLS / GQ; /* tokens per workgroup */
        p.grid[0] = (P.n_tok + TQ - 1) / TQ, p.grid[1] = P.n_kv, p.grid[2] = P.n_seq;
        if ((long)p.grid[0] * P.n_kv * P.n_seq <= ATTN_PAIR_MAX_WGS && P.n_tok >= ATTN_PAIR_MIN_TOK)
            p.route = ATTN_PAIRED, p.grid[0] = ((P.n_tok + TQ / 2 - 1) / (TQ / 2) + 1) / 2; /* half blocks of TQ / 2 tokens, two per workgroup */
        p.kh = p.route == ATTN_PAIRED ? 2 : 1, p.kt = p.kh == 2 ? AP_KT_LONG : AP_KT, p.threads = 256 * p.kh;
        p.lds = AttnTileLds(P.hd, p.kh, p.kt).bytes;
        return p;
    }
    // the decode kernel: sliced (one token), or one slice per token (a prompt the tile kernel does not take)
    const bool per_token = P.entry == ATTN_PROMPT;
    p.route = per_token ? ATTN_PER_TOKEN : ATTN_SLICED;
    if (!hd_ok || !kv_ok || !gq_ok) return refuse(KF_INVALID_ARGS);
    const int n_tok = per_token ? P.n_tok : 1;
    const AttnSlices s = attn_slices(P.pos + n_tok - 1, P.n_kv, GQ, per_token);
    if (!sliced(P.canon != 0, s, s.nw, n_tok, !per_token)) return p;
    p.lds = p.canon ? AttnCanonLds(p.gq, p.nw, P.hd).bytes : AttnFastLds(p.gq, p.nw, P.hd).bytes;
    return p;
}

// ---- the launchers carry out a plan with status KF_OK: KF_OK, KF_INTERNAL_ERR (a form the plan never names) or KF_HIP_CHECK
int attn_launch(hipStream_t st, AttnArgs& a, const AttnPlan& p, bool rows = false); /* kf_attn.hip, ATTN_SLICED / ATTN_PER_TOKEN (returns p.status when not KF_OK); a's geometry from p; rows: an ATTN_VERIFY plan */
int attn_prefill_mfma_launch(hipStream_t st, const AttnPlan& p, const uint16_t* q, const uint16_t* kc, const uint16_t* vc, uint16_t* out, int pos0, int n_tok,
                             long long q_stride, int n_kv, int kv_stride, int n_seq, long long out_stride); /* kf_attn_prefill.hip, ATTN_TILE / ATTN_PAIRED */
int attn_backward_mfma_launch(hipStream_t st, const AttnPlan& p, const uint16_t* q, const uint16_t* k, const uint16_t* v, long long ld_qkv, const uint16_t* o,
                              const uint16_t* dO, long long ld_o, uint16_t* dq, uint16_t* dk, uint16_t* dv, long long ld_d, int T, float* scratch, long long ld_kv,
                              long long ld_dkv); /* kf_attn_bwd_mfma.hip, ATTN_BWD */
// the int8 cache (kf_attn_kv8.hip): ATTN_SLICED_KV8, and the two row kernels (no plan: one wave per (row, kv-head), one workgroup per row)
struct AttnKv8Args {
    const uint16_t* q;     /* raw q [n_head * hd] */
    const uint16_t* k_raw; /* raw new key [n_kv * hd] */
    const uint16_t* v_raw; /* new value row [n_kv * hd] */
    int8_t* k8;
    int8_t* v8;
    float* ks;
    float* vs;
    const uint16_t* wq_norm;
    const uint16_t* wk_norm;
    const float* rope_table;
    double* part;  /* [n_head][n_splits][hd + 2] fp64 partials {O, L, m} */
    int* counters; /* per (kv-head, part), zero between launches */
    uint16_t* out;
    const int* d_pos;
    int pos, n_kv, kv_stride, n_splits, chunk, cnt_stride, gq_split;
    float eps, inv_sqrt_hd_den;
};
int attn_kv8_launch(hipStream_t st, AttnKv8Args& a, const AttnPlan& p);
struct AttnPrefillKv8Args { /* kf_attn_prefill_kv8.hip, ATTN_TILE_KV8 */
    const uint16_t* q; /* prepared bf16 query rows */
    const int8_t* k8;
    const int8_t* v8;
    const float* ks;
    const float* vs;
    uint16_t* out;
    int pos0, n_tok, n_kv, kv_stride;
    long long q_stride; /* of q and of out */
    float rden;
};
int attn_prefill_kv8_launch(hipStream_t st, AttnPrefillKv8Args& a, const AttnPlan& p);
int kv8_quant_rows_launch(hipStream_t st, const uint16_t* k, const uint16_t* v, long long ld, int n, int n_kv, int hd, int8_t* k8, int8_t* v8, float* ks, float* vs, int pos0,
                          int kv_stride);
int kv8_dequant_rows_launch(hipStream_t st, const int8_t* k8, const int8_t* v8, const float* ks, const float* vs, int n, int n_kv, int hd, int kv_stride, uint16_t* kout,
                            uint16_t* vout, long long ld_out);

}  // namespace kf
