// kf_gemm_plan.h -- how a batch of tokens is multiplied: kf::gemm_plan, one pure host function, picks the route (which operand, dequantised where), the kernel family
// and its form, the split-K cut, grid and LDS for every token-batch entry of kf_abi.hip; the launchers of kf_gemm*.hip execute what it returns and decide nothing.
// Each route sums in its own fp32 order, so the choice decides the bits: every threshold that picks a route is a constant of this file.
#pragma once
#include "kf_kernels.h"

namespace kf {

// ---- the tile shapes the rule sizes grids and LDS with (the kernels of kf_gemm.hip, kf_gemm2.hip, kf_gemm3.hip use the same constants)
constexpr int GM_TOK = 128;      /* kf_gemm.hip staged kernel: tokens per workgroup tile (4 MFMA column blocks) */
constexpr int GM_KT = 128;       /* k per staged x tile */
constexpr int GM_XS = GM_KT + 8; /* padded LDS row in bf16 elements: 272 B, ds_read_b128 of 32 rows is conflict-free */
constexpr int GD_NW = 8, GD_UPG = 2; /* direct kernel: 8 waves, groups of two 64-element units, 32-token tiles */
constexpr int GM_EPB[7] = {8, 16, 32, 64, 128, 32, 32}; /* elements per 16-byte block, by FMT_* */
constexpr int G2_BM = 128, G2_BN = 256, G2_BK = 64; /* kf_gemm2.hip producer / consumer tile */
constexpr int G2_LS = G2_BK + 8;                    /* LDS row, bf16 elements */
constexpr size_t G2_STAGE = (size_t)(G2_BM + G2_BN) * G2_LS * sizeof(uint16_t);
constexpr int G3_BM = 256, G3_BN = 256, G3_BK = 64;
// kf_gemm3.hip: the workgroup tile BM rows x BN tokens, NW waves as 2 (rows) x NW / 2 (tokens).  Big = 256 x 256 (8 waves, 128 KiB of LDS: one workgroup per CU); Small =
// 128 x 128 on 4 waves (64 KiB: two per CU) for products with too few 256 x 256 tiles to fill the chip.  K-contiguous operands only.
template <int BM_, int BN_, int NW_>
struct G3Cfg {
    static constexpr int BM = BM_, BN = BN_, NW = NW_, WN = NW_ / 2, MT = BM_ / 32, NT = BN_ / (16 * (NW_ / 2));
    static constexpr int NIA = BM_ / (8 * NW_), NIB = BN_ / (8 * NW_); /* global_load_lds instructions per wave, operand and k-step (8 rows of 128 bytes each) */
    static constexpr int STAGE = (BM_ + BN_) * G3_BK * 2, NTH = 64 * NW_, WGS_PER_CU = (160 * 1024) / (2 * STAGE);
};
using G3Big = G3Cfg<256, 256, 8>;
using G3Small = G3Cfg<128, 128, 4>;
// products whose 128 x 128 tiles do not fill the chip either (M = 1024 at 1-2 k tokens: 64-128 of them; split-K S = 4 measured 37.8 us against 27 plain: three
// 64 KiB partials per tile through memory) get MORE, SMALLER tiles instead of k-pieces: 64 x 128 (48 KiB of LDS: three workgroups per CU) and 64 x 64 (32 KiB: five)
using G3Mid = G3Cfg<64, 128, 4>;
using G3Tiny = G3Cfg<64, 64, 4>;
// 192 x 256: a product whose 256 x 256 tiles number 160-255 (gate | up of a 0.6B model at 2047 tokens: 24 x 8 = 192 tiles on 256 CUs) becomes 32 x 8 = 256 tiles of 3/4 the work
using G3Wide = G3Cfg<192, 256, 8>;
enum { G3_BIG = 0, G3_SMALL = 1, G3_MID = 2, G3_TINY = 3, G3_WIDE = 4 };
struct G3Form {
    int bm, bn, nth, lds, wgs;
};
template <class C>
constexpr G3Form g3_form() { return {C::BM, C::BN, C::NTH, 2 * C::STAGE, C::WGS_PER_CU}; }
constexpr G3Form G3_FORMS[5] = {g3_form<G3Big>(), g3_form<G3Small>(), g3_form<G3Mid>(), g3_form<G3Tiny>(), g3_form<G3Wide>()};
constexpr size_t G3_SK_FLAG_BYTES = 8192; /* up to 2048 resident workgroups (64 x 64 tiles, eight per CU) */
/* the split-K workspace: 256 partial 256 x 256 fp32 tiles + the flags in its last 8 KiB */
constexpr size_t gemm3_sk_ws_bytes() { return (size_t)256 * G3_BM * G3_BN * 4 + G3_SK_FLAG_BYTES; }

// ---- the route thresholds (token rows unless said otherwise)
constexpr int GEMM_MIN = 8;             /* the MFMA tile kernels replace the per-token mat-vec loop */
constexpr int G3_FIRST = 256;           /* bf16 operands try the kf_gemm3.hip tiles before the 32 x 32 direct kernel (the direct kernel took 64 us for bf16 1024 x 2048 at 1024 rows) */
constexpr int RESIDENT_MIN = 320;       /* with a dequant arena: the resident bf16 copies + the kf_gemm3.hip tiles (the 1024-row o_proj / down_proj of a long prompt) */
constexpr int STACK_MIN = 1024;         /* without an arena: the stacked route, a dequantise per call */
constexpr int DEQ_TILE_MIN = 2048;      /* a quantised weight is dequantised into the scratch once for the bf16 tiles (a few % of the product at these sizes) */
// prompt-sized batches on small matrices: the wave-independent direct kernel while its 32 x 32 workgroups fit ~2-3 rounds of the chip (measured crossover against
// the staged tiles, scratch/ub_gemm.py: 1024 rows up to n ~ 1024, 2048 up to ~ 600, 3072 up to ~ 400)
constexpr long DIRECT_MAX = 1280;       /* 32 x 32 workgroups */
constexpr long GD_FUSED_MAX = 2048;     /* workgroups up to which the fused direct launches (Q | K | V, gate | up) beat separate (staged) ones */
constexpr long G2_MIN_WG = 128;         /* fewer producer / consumer workgroups than this: the staged / direct tiles fill the chip better */
constexpr long G3_BIG_MIN = 160;        /* 256 x 256 tiles from this many; fewer: four times as many 128 x 128 ones (M 1024 x K 3072 at 8192 rows: 83 -> 57 us) */
constexpr long G3_MID_MIN = 192;        /* 64 x 128 tiles from this many of them, 64 x 64 below */

enum { DEQ_STACK = 0, DEQ_ILV = 1 }; /* dequantised copies: back to back, or gate | up interleaved in blocks of 16 rows (dequant_launch ilv_n = 2) */

// ---- the problem: what an entry knows before it launches anything
enum GemmEntry { GE_LINEAR = 0, GE_MULTI = 1, GE_GATEUP = 2, GE_QKV_ROPE = 3, GE_BWD_DX = 4, GE_BWD_DW = 5 };
struct GemmProblem {
    int entry;              /* GemmEntry */
    int n_w;                /* matrices: 1 (linear, backward), 2-3 (multi), 2 (gate | up), 3 (Q | K | V) */
    GemmMat w[3];
    int n;                  /* token rows */
    int x_al;               /* x 16-byte aligned (its row stride is K) */
    int y_al;               /* GE_GATEUP: act, GE_QKV_ROPE: q and k 8-byte aligned */
    int rope_ok;            /* GE_QKV_ROPE: head_dim 128, wq / wk n_head / n_kv heads */
    int arena, capturing;   /* a dequant arena is set; the stream is being captured */
    int arena_hit;          /* bit (1 << form): the copy of these matrices in that form is resident */
    long long arena_free;   /* arena bytes not used yet */
    long long scratch;      /* bytes lent: kf_set_scratch's (16-byte aligned), the backward's middle region; 0 none */
};

// ---- the plan: what the entry does
enum GemmRoute {
    GR_MATVEC = 0,   /* one mat-vec launch per token row */
    GR_AWQ,          /* the AutoAWQ mat-vec per token row */
    GR_ROWFORM,      /* row forms: GetDataX into the scratch, then k on the copy (3- / 2-bit at any batch, k.fam == GK_NONE: the mat-vec loop on it; 4-bit row-LUT when
                        only the copy is tile-eligible) */
    GR_RESIDENT,     /* k on the weight's resident bf16 copy (kf_set_dequant_arena) */
    GR_DEQ_TILE,     /* k on the weight dequantised into the scratch */
    GR_TILE,         /* k on the weight as it is stored */
    GR_STACKED,      /* the matrices dequantised back to back, one kf_gemm3.hip launch over the stacked rows (+ kf_swiglu for gate | up) */
    GR_SWIGLU,       /* gate | up dequantised interleaved, SwiGLU in the kf_gemm3.hip epilogue */
    GR_ROPE,         /* Q | K | V stacked, q/k-norm + RoPE in the kf_gemm3.hip epilogue */
    GR_FUSED,        /* the direct kernel over 2-3 matrices sharing x (Q | K | V; paired gate | up + SwiGLU) */
    GR_SEPARATE,     /* one kf_linear per matrix (+ kf_swiglu / q/k-norm + RoPE launches) */
    GR_KMAJOR,       /* backward: kf_gemm3.hip on the k-major operands as they lie */
    GR_TRANSPOSE     /* backward: the operands transposed into the scratch, then k */
};
enum GemmFamily { GK_NONE = 0, GK_DIRECT, GK_PAIRED, GK_STAGED, GK_G2, GK_G3 };
enum { DQ_NONE = 0, DQ_SCRATCH, DQ_ARENA, DQ_RESIDENT }; /* the copy: none, into the scratch, into the arena (kept), already in the arena */
struct GemmKern {
    int fam;            /* GemmFamily; GK_NONE: no tile kernel takes the shape */
    int fmt;            /* FMT_* of the operand the kernel reads */
    int gshift;         /* log2(16-byte blocks per quantisation group) */
    int form;           /* GK_DIRECT: 32- / 64-token tiles; GK_STAGED: KS 1 / 2; GK_G3: G3_BIG .. G3_WIDE */
    int akm, bkm;       /* GK_G3: k-major A (weight) / B (token) operand */
    int gx, gy, block, lds;
    int sk;             /* GK_G3: the split-K form (gemm3_sk_kernel) with P tiles, S pieces, kp owner steps, R helper steps */
    int P, S, kp, R;
};
struct GemmPlan {
    int route;            /* GemmRoute */
    int status;           /* KF_OK, or the error the route meets (a malformed quantisation group: KF_QUANT_ERR) */
    int deq, deq_form;    /* DQ_*, DEQ_STACK / DEQ_ILV */
    long long deq_bytes;  /* bytes of the copy */
    long long ws_bytes;   /* scratch lent to k's split-K slots; 0 none */
    GemmKern k;
};

// ---- the rule
inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline long long up256(long long v) { return (v + 255) & ~255LL; }

// g3's launch over nwg tiles of form f: split-K when the tiles are fewer than 4/5 of the resident workgroups, the caller lent the workspace and the pieces stay
// >= 512 deep in k (kf_gemm3.hip gemm3_sk_kernel); otherwise one workgroup per tile when there are at least min_plain of them
inline GemmKern g3_kern(int f, bool akm, bool bkm, long nwg, int K, long long ws, long min_plain) {
    const G3Form& c = G3_FORMS[f];
    GemmKern k = {};
    k.fam = GK_G3, k.fmt = FMT_BF16, k.form = f, k.akm = akm, k.bkm = bkm, k.gy = 1, k.block = c.nth, k.lds = c.lds;
    const int G = 256 * c.wgs, nkt = K / G3_BK, min_steps = 512 / G3_BK;
    if (ws >= (long long)gemm3_sk_ws_bytes() && 5 * nwg < 4 * G) {
        int P = (int)nwg, S = G / P, kp = 0, R = 1, nlaunch;
        if (S >= 2) {
            while (S > 1 && nkt / S < min_steps) S--;
            nlaunch = P * S;
        } else {
            kp = (int)(((long long)nkt * P + G / 2) / G);
            nlaunch = G;
            const long long T = (long long)P * (nkt - kp);
            R = (int)((T + (G - P) - 1) / (G - P));
            if (nkt - kp < 1 || nkt < 4 * min_steps || T * 2 >= (1LL << 31)) S = 0;
        }
        if (S >= 1 && (S >= 2 || kp > 0)) {
            k.sk = 1, k.P = P, k.S = S, k.kp = kp, k.R = R, k.gx = nlaunch;
            return k;
        }
    }
    if (nwg < min_plain) return GemmKern{};
    k.gx = (int)nwg;
    return k;
}
// kf_gemm3.hip on one bf16 operand W[M][K] (16-byte aligned) x x[n][K]: ws lends the 64-row tiles their split-K slots
inline GemmKern g3_plain(int M, int K, int n, bool x_al, long long ws) {
    if (K % G3_BK != 0 || K < G3_BK || !x_al) return GemmKern{};
    if (n >= G3_BN && M >= G3_BM) {
        const long nwg = cdiv(M, G3_BM) * cdiv(n, G3_BN);
        if (nwg >= G3_BIG_MIN) return g3_kern(G3_BIG, false, false, nwg, K, 0, 64);
    }
    // 128 x 128 tiles, two workgroups per CU: bf16 products of 1-4 k rows whose M is 1024-3072 (M 1024 x K 2048 at 2048 rows: 36.9 -> 27.4 us, 3072 x 1024: 35.6 -> 23.9)
    if (n < 128 || M < 128) return GemmKern{};
    const long nwg = cdiv(M, 128) * cdiv(n, 128), ntiny = cdiv(M, 64) * cdiv(n, 64);
    if (nwg < 32 && ntiny < 64) return GemmKern{};
    if (nwg < 256) { /* fewer 128 x 128 tiles than CUs: twice or four times as many smaller ones, in k-pieces with the workspace when even those leave CUs idle */
        const long nmid = cdiv(M, 64) * cdiv(n, 128);
        return nmid >= G3_MID_MIN ? g3_kern(G3_MID, false, false, nmid, K, ws, 64) : g3_kern(G3_TINY, false, false, ntiny, K, ws, 64);
    }
    return g3_kern(G3_SMALL, false, false, nwg, K, 0, 128);
}

// the in-register-unpack tile kernels' view of a matrix (kf_gemm.hip): 0 eligible (fmt, gshift set), 1 not, KF_QUANT_ERR a malformed group
inline int gm_eligible(const GemmMat& m, int& fmt, int& gshift) {
    switch (m.type) {
        case KF_BF16: fmt = FMT_BF16; break;
        case KF_F8E5M2: fmt = FMT_F8; break;
        case KF_Q4: fmt = FMT_Q4; break;
        case KF_T_SIGN: fmt = FMT_Q2; break;
        case KF_BOOL1: case KF_T_BINARY: fmt = FMT_Q1; break;
        default: fmt = -1;
    }
    if (m.quant != KF_QUANT_GROUP) { /* 4-bit row codebooks unpack in registers like the Packed128 form; the 3- / 2-bit row forms are dequantised by the caller */
        if (m.type != KF_Q4 || m.quant != KF_QUANT_ROW_LUT) return 1;
        fmt = FMT_Q4R;
    }
    gshift = 0;
    if (fmt < 0 || m.awq) return 1;
    // K a multiple of 128 for every kernel; a multiple of 64 is enough for the direct kernel on the formats whose 64-element unit is made of whole blocks (bf16, f8,
    // 4-bit) -- GPT-2's n_embd = 1600
    if (m.K % 64 != 0 || m.K < GM_KT || m.M < 1 || !(m.al & GM_DATA_AL)) return 1;
    if (m.K % GM_KT != 0 && fmt > FMT_Q4 && fmt != FMT_Q4R) return 1;
    if ((unsigned long long)m.M * (unsigned long long)(m.K / GM_EPB[fmt]) >= (1ull << 32)) return 1;
    if (fmt == FMT_Q4R) {
        if (!m.gama) return KF_QUANT_ERR;
        if (!(m.al & GM_TAB_AL)) return 1;
    } else if (fmt >= FMT_Q4) {
        if (!m.gama || m.lgroup <= 0 || (m.lgroup % GM_EPB[fmt]) != 0 || ((long)m.M * m.K) % m.lgroup != 0) return KF_QUANT_ERR;
        const int bpg = m.lgroup / GM_EPB[fmt];
        if (bpg < 1 || (bpg & (bpg - 1)) != 0) return KF_QUANT_ERR;
        gshift = __builtin_ctz(bpg);
    }
    return 0;
}
inline GemmMat bf16_mat(int M, int K) { return GemmMat{KF_BF16, KF_QUANT_GROUP, 0, M, K, 0, 0, GM_DATA_AL}; } /* a dequantised / transposed copy */

// one matrix x a batch of n token rows (x row stride K): 0 with k set, 1 no tile kernel takes it, < 0 error
inline int tile_plan(const GemmMat& m, int n, bool x_al, long long ws, GemmKern& k) {
    k = GemmKern{};
    int fmt, gshift;
    const int rc = gm_eligible(m, fmt, gshift);
    if (rc) return rc;
    if (!x_al || m.K % 8) return 1;
    const int M = m.M;
    const bool direct = cdiv(M, 32) * cdiv(n, 32) <= DIRECT_MAX;
    if (fmt == FMT_BF16 && (n >= G3_FIRST || !direct)) { /* bf16 operands: the global_load_lds tiles first from G3_FIRST rows, past the direct kernel's size below */
        k = g3_plain(M, m.K, n, x_al, n >= G3_FIRST ? ws : 0);
        if (k.fam) return 0;
    }
    k.fmt = fmt, k.gshift = gshift;
    if (direct) {
        k.fam = GK_DIRECT, k.form = 32, k.gx = (int)cdiv(M, 32), k.gy = (int)cdiv(n, 32), k.block = GD_NW * 64, k.lds = GD_NW * 16 * 64 * 4;
        return 0;
    }
    if ((fmt == FMT_Q4 || fmt == FMT_BF16 || fmt == FMT_F8) && m.K % G2_BK == 0 && n >= G2_BN && cdiv(M, G2_BM) * cdiv(n, G2_BN) >= G2_MIN_WG) {
        k.fam = GK_G2, k.gx = (int)cdiv(M, G2_BM), k.gy = (int)cdiv(n, G2_BN), k.block = 512, k.lds = (int)(2 * G2_STAGE);
        return 0;
    }
    const long ttiles = cdiv(n, GM_TOK);
    k.fam = GK_STAGED, k.form = cdiv(M, 128) * ttiles < 512 ? 2 : 1;
    k.gx = (int)cdiv(M, 32 * (4 / k.form)), k.gy = (int)ttiles, k.block = 256, k.lds = 2 * GM_TOK * GM_XS * 2;
    return 0;
}

inline int stack_min(bool arena) { return arena ? RESIDENT_MIN : STACK_MIN; } /* token rows from which the stacked routes are taken */
// the stacked route's shape: 2-3 group-quantised (or bf16) matrices of one input width, each a multiple of 256 rows, enough tiles for kf_gemm3.hip; its bytes
inline bool stack_shape(const GemmProblem& P, long long* bytes) {
    long rows = 0;
    long long tot = 0;
    if (P.n_w < 2 || P.n_w > 3 || P.n < stack_min(P.arena)) return false;
    for (int i = 0; i < P.n_w; i++) {
        const GemmMat& m = P.w[i];
        if (m.awq || m.quant != KF_QUANT_GROUP || m.M < 256 || m.M % 256 != 0 || m.K % 64 != 0 || m.K != P.w[0].K) return false;
        tot += up256((long long)m.M * m.K * 2), rows += m.M; /* up256: a no-op on these sizes, the stacked rows are contiguous */
    }
    if ((rows / 256) * cdiv(P.n, 256) < 64 && (rows / 128) * cdiv(P.n, 128) < 64) return false; /* fewer tiles than that: the in-register-unpack kernels */
    *bytes = tot;
    return true;
}
// where the copy of the problem's matrices in `form` comes from: resident, kept in the arena (not while capturing: a replay would refill it), or the scratch
inline int copy_target(const GemmProblem& P, int form, long long bytes, bool arena_only) {
    if (P.arena && (P.arena_hit >> form & 1)) return DQ_RESIDENT;
    if (P.arena && !P.capturing && bytes <= P.arena_free) return DQ_ARENA;
    return !arena_only && P.scratch >= bytes ? DQ_SCRATCH : DQ_NONE;
}
// the large-batch dequantise + tile route's shape (kf_linear; also what kf_linear_scratch_bytes asks for)
inline bool deq_tile_shape(const GemmMat& m, int n) { return m.type != KF_BF16 && m.quant == KF_QUANT_GROUP && n >= DEQ_TILE_MIN && m.M >= 256 && m.K % 64 == 0; }

inline GemmPlan plan_of(int route, GemmKern k = GemmKern{}, int deq = DQ_NONE, long long deq_bytes = 0, int status = 0) {
    GemmPlan p = {};
    p.route = route, p.k = k, p.deq = deq, p.deq_bytes = deq_bytes, p.status = status;
    return p;
}

inline GemmPlan gemm_plan_linear(const GemmProblem& P) {
    const GemmMat& m = P.w[0];
    const long long bytes = (long long)m.M * m.K * 2;
    GemmKern k;
    if (m.awq) return plan_of(GR_AWQ);
    if (m.quant != KF_QUANT_GROUP && m.type != KF_Q4) { /* 3- / 2-bit row forms: GetDataX into the scratch whatever the batch (the reference's own order) */
        if (P.n < GEMM_MIN || tile_plan(bf16_mat(m.M, m.K), P.n, P.x_al, 0, k) != 0) k = GemmKern{};
        return plan_of(GR_ROWFORM, k, DQ_SCRATCH, bytes);
    }
    if (P.arena && P.n >= RESIDENT_MIN && m.type != KF_BF16 && m.quant == KF_QUANT_GROUP && m.M >= 128 && m.K % 64 == 0) {
        const int dq = copy_target(P, DEQ_STACK, up256(bytes), true);
        const long long ws = P.scratch >= (long long)gemm3_sk_ws_bytes() ? P.scratch : 0; /* the scratch holds no copy on this route: split-K slots */
        if (dq && tile_plan(bf16_mat(m.M, m.K), P.n, P.x_al, ws, k) == 0) {
            GemmPlan p = plan_of(GR_RESIDENT, k, dq, up256(bytes));
            p.ws_bytes = ws;
            return p;
        }
    }
    if (deq_tile_shape(m, P.n) && P.scratch >= bytes &&
        (cdiv(m.M, 256) * cdiv(P.n, 256) >= 128 || cdiv(m.M, 128) * cdiv(P.n, 128) >= 256 /* the 128 x 128 form: M 1024 from 4096 rows */) &&
        tile_plan(bf16_mat(m.M, m.K), P.n, P.x_al, 0, k) == 0)
        return plan_of(GR_DEQ_TILE, k, DQ_SCRATCH, bytes);
    if (P.n >= GEMM_MIN) {
        const int rc = tile_plan(m, P.n, P.x_al, 0, k);
        if (rc <= 0) return plan_of(GR_TILE, k, DQ_NONE, 0, rc);
        // a 4-bit row codebook the nibble form does not take but its bf16 copy does -- row tables not 16-byte aligned, which kf_linear's argument check refuses first:
        // GetDataX into the scratch, then the bf16 tiles on the copy
        if (m.quant == KF_QUANT_ROW_LUT && P.scratch >= bytes && tile_plan(bf16_mat(m.M, m.K), P.n, P.x_al, 0, k) == 0) return plan_of(GR_ROWFORM, k, DQ_SCRATCH, bytes);
    }
    return plan_of(GR_MATVEC);
}

// the direct kernel over the problem's matrices sharing x: Q | K | V (GR_FUSED, 32- or 64-token tiles) or gate | up + SwiGLU (paired); 0, 1 not eligible, < 0 error
inline int fused_plan(const GemmProblem& P, bool paired, GemmKern& k) {
    k = GemmKern{};
    if (!P.x_al || P.w[0].K % 8) return 1;
    int fmt0 = 0, g0 = 0;
    long rbs = 0;
    for (int i = 0; i < P.n_w; i++) {
        int fmt, gshift;
        const int rc = gm_eligible(P.w[i], fmt, gshift);
        if (rc) return rc;
        if (i == 0) fmt0 = fmt, g0 = gshift;
        if (fmt != fmt0 || P.w[i].K != P.w[0].K || gshift != g0 || (paired && P.w[i].M != P.w[0].M)) return 1;
        rbs += cdiv(P.w[i].M, 32);
    }
    if (paired) rbs = cdiv(P.w[0].M, 32);
    if (rbs * cdiv(P.n, 32) > GD_FUSED_MAX) return 1;
    k.fam = paired ? GK_PAIRED : GK_DIRECT, k.fmt = fmt0, k.gshift = g0, k.form = 32, k.gx = (int)rbs, k.gy = (int)cdiv(P.n, 32), k.block = GD_NW * 64;
    k.lds = GD_NW * (paired ? 2 : 1) * 16 * 64 * 4;
    if (!paired && P.n >= 64 && rbs * cdiv(P.n, 64) >= 256) /* 64-token tiles: every weight block is unpacked for two token blocks */
        k.form = 64, k.gy = (int)cdiv(P.n, 64), k.lds = GD_NW * 2 * 16 * 64 * 4;
    return 0;
}
// one kf_gemm3.hip launch over the stacked rows (tot of them, multiples of 256): fewer than 160 big tiles (Q | K | V of a 0.6B model at 2047 tokens: 128) go on four
// times as many 128 x 128 ones (2047-token prompt 8.20 -> 7.84 ms); the RoPE epilogue always on the head-sized 128 x 128 tile
inline GemmKern stacked_kern(long tot, int K, int n, bool rope) {
    const long nwg = (tot / G3_BM) * cdiv(n, G3_BN), nsmall = (tot / 128) * cdiv(n, 128);
    if (rope || nwg < G3_BIG_MIN) return g3_kern(G3_SMALL, false, false, nsmall, K, 0, 1);
    return g3_kern(G3_BIG, false, false, nwg, K, 0, 64);
}
// gate | up interleaved (M = 2 ffn rows) with the SwiGLU epilogue: fewer than 160 big tiles go on 128 x 128 ones -- unless those spill into a second round of the 512
// resident workgroups and 192 x 256 ones make one round
inline GemmKern swiglu_kern(int M, int K, int n) {
    const long nwg = (M / G3_BM) * cdiv(n, G3_BN), nws = (M / 128) * cdiv(n, 128), nww = (M / 192) * cdiv(n, G3_BN);
    const bool wide_ok = M % 192 == 0 && nww <= 256;
    if (nwg < G3_BIG_MIN && !(wide_ok && nws > 512 && nww >= G3_BIG_MIN)) return g3_kern(G3_SMALL, false, false, nws, K, 0, 1);
    if (wide_ok && nwg < 256) return g3_kern(G3_WIDE, false, false, nww, K, 0, 1);
    return g3_kern(G3_BIG, false, false, nwg, K, 0, 64);
}

inline GemmPlan gemm_plan_shared(const GemmProblem& P) { /* GE_MULTI, GE_GATEUP, GE_QKV_ROPE */
    long long bytes = 0;
    const GemmMat& m = P.w[0];
    if (stack_shape(P, &bytes) && P.x_al) {
        long tot = 0;
        for (int i = 0; i < P.n_w; i++) tot += P.w[i].M;
        if (P.entry == GE_QKV_ROPE) {
            const int dq = P.rope_ok && P.y_al ? copy_target(P, DEQ_STACK, bytes, false) : DQ_NONE;
            if (dq) return plan_of(GR_ROPE, stacked_kern(tot, m.K, P.n, true), dq, bytes);
            return plan_of(GR_SEPARATE); /* kf_linear_multi: the stacked route without the epilogue */
        }
        if (P.entry == GE_GATEUP && m.M % 128 == 0 && P.y_al) {
            const int dq = copy_target(P, DEQ_ILV, bytes, false);
            if (dq) {
                GemmPlan p = plan_of(GR_SWIGLU, swiglu_kern(2 * m.M, m.K, P.n), dq, bytes);
                p.deq_form = DEQ_ILV;
                return p;
            }
        }
        const int dq = copy_target(P, DEQ_STACK, bytes, false);
        if (dq) return plan_of(GR_STACKED, stacked_kern(tot, m.K, P.n, false), dq, bytes);
    }
    if (P.entry == GE_QKV_ROPE) return plan_of(GR_SEPARATE);
    // bf16 storage from G3_FIRST rows: one kf_linear per matrix (the kf_gemm3.hip tiles) -- the fused in-register launch would be another summation order
    if (P.n_w > 1 && P.n >= GEMM_MIN && !(m.type == KF_BF16 && P.n >= G3_FIRST)) {
        GemmKern k;
        const int rc = fused_plan(P, P.entry == GE_GATEUP, k);
        if (rc <= 0) return plan_of(GR_FUSED, k, DQ_NONE, 0, rc);
    }
    return plan_of(GR_SEPARATE);
}

// backward (kf_linear_backward, W [OC = w[0].M][IC = w[0].K], n token rows): dX [n, IC] = dY [n, OC] . W, or dW [OC, IC] += dY^T . X -- kf_gemm3.hip on the k-major
// operands as they lie (the scratch lends the split-K slots), else the transposed copies on the token-batch tiles.  IC % 8 == 0 and OC, n % 64 == 0 (the entry's checks)
// keep every row stride a multiple of 8 elements.
inline GemmPlan gemm_plan_backward(const GemmProblem& P) {
    const int OC = P.w[0].M, IC = P.w[0].K;
    const bool dx = P.entry == GE_BWD_DX;
    const int M = IC, K = dx ? OC : P.n, n = dx ? P.n : OC; /* y [n, M] = sum over K */
    GemmKern k = {};
    if (K % G3_BK == 0 && K >= G3_BK && n >= G3_BN && M >= G3_BM && !(M & 7) && !(n & 7)) {
        // big tiles that fill less than 4/5 of the CUs: 128 x 128 tiles instead when they make (nearly) whole rounds of the 512 resident workgroups, or -- with the
        // workspace -- their split-K form (partials of 64 KiB instead of 256 KiB, twice the workgroups).  (Qwen3-0.6B training step 99.3 -> 95.7 ms with the first rule
        // alone, -> 87.2 ms with both; GPT2-1558M 166.0 -> 163.7 -> 161.2 ms)
        const long nwg = cdiv(M, G3_BM) * cdiv(n, G3_BN), nws = cdiv(M, 128) * cdiv(n, 128), rounds = cdiv(nws, 512);
        const bool small = 5 * nwg < 4 * 256 && (20 * nws >= 17 * rounds * 512 || (P.scratch >= (long long)gemm3_sk_ws_bytes() && 5 * nws < 4 * 512));
        k = small ? g3_kern(G3_SMALL, true, !dx, nws, K, P.scratch, 1) : g3_kern(G3_BIG, true, !dx, nwg, K, P.scratch, 64);
        if (k.fam) {
            GemmPlan p = plan_of(GR_KMAJOR, k);
            p.ws_bytes = P.scratch;
            return p;
        }
    }
    if (tile_plan(bf16_mat(M, K), n, true, 0, k) != 0) k = GemmKern{}; /* GK_NONE: not covered */
    return plan_of(GR_TRANSPOSE, k);
}

inline GemmPlan gemm_plan(const GemmProblem& P) {
    switch (P.entry) {
        case GE_LINEAR: return gemm_plan_linear(P);
        case GE_BWD_DX: case GE_BWD_DW: return gemm_plan_backward(P);
        default: return gemm_plan_shared(P);
    }
}

// ---- the launchers (kf_gemm.hip, kf_gemm3.hip): each executes a plan's k, nothing else; KF_OK or KF_HIP_CHECK
struct GmWeight { /* an operand in the form k reads: the stream, its group tables (or the row codebooks), M x K */
    const unsigned char* w;
    const uint16_t *zero, *step;
    float qBias;
    int M, K;
};
GmWeight gm_operand(const kf_weight* w, const GemmKern& k);                                  /* the weight as it is stored */
inline GmWeight gm_bf16(const void* data, int M, int K) { return GmWeight{(const unsigned char*)data, nullptr, nullptr, 0.f, M, K}; } /* a bf16 copy */
int gemm_launch(hipStream_t st, const GemmKern& k, const GmWeight& g, const uint16_t* x, long long ldx, int n, uint16_t* y, long long ldy, const uint16_t* bias, float alpha,
                float beta, const uint16_t* residual, long long ldr, void* ws = nullptr);
// GR_FUSED: matrix j of g (sharing x and K) into y[j] (row stride its M); GK_PAIRED: act = y[0] = silu(x . g[0]^T) * (x . g[1]^T)
int gemm_multi_launch(hipStream_t st, const GemmKern& k, int n_w, const GmWeight* g, const uint16_t* x, long long ldx, int n, uint16_t* const* y);
struct G3Rope { /* ROPE::cuInfer folded into the stacked Q | K | V launch's epilogue (kf_gemm3.hip g3_epilogue_qkrope) */
    const uint16_t *wq, *wk; /* q / k norm weights [128] or NULL */
    const float* table;      /* RoPE (cos, sin) table or NULL */
    int pos0;
    float eps;
    int seq_len; /* > 0: rows are sequences of seq_len tokens back to back, positions pos0 .. pos0 + seq_len - 1 in each */
};
// GR_STACKED / GR_ROPE: bf16 matrices stacked along M in one buffer (each a multiple of 256 rows), matrix j's rows into y[j] (row stride M[j]); rope: its epilogue
int gemm3_multi_launch(hipStream_t st, const GemmKern& k, int n_w, const uint16_t* Wcat, const int* M, int K, const uint16_t* x, long long ldx, int n, uint16_t* const* y,
                       const G3Rope* rope = nullptr);
// GR_SWIGLU: gate | up interleaved in blocks of 16 rows, act[n, ffn] = SwiGLU in the epilogue
int gemm3_swiglu_launch(hipStream_t st, const GemmKern& k, const uint16_t* Wilv, int ffn, int K, const uint16_t* x, long long ldx, int n, uint16_t* act);
// GR_KMAJOR: y[n, M] = alpha * sum_k B(k, tok) A(k, m) + beta * y, A = w[K][lda] k-major, B = x[K][ldb] (k.bkm) or x[n][ldb]; ws lends the split-K slots
int gemm3_km_launch(hipStream_t st, const GemmKern& k, const uint16_t* A, long long lda, const uint16_t* B, long long ldb, int n, int M, int K, uint16_t* y, long long ldy,
                    float alpha, float beta, void* ws);

}  // namespace kf
