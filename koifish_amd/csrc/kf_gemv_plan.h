// kf_gemv_plan.h -- how one token's mat-vec is launched: kf::gemv_plan, one pure host function, picks the storage form, the lanes per row, the slots per wave, the
// kernel form, grid and LDS of every gemv_launch; the launcher (kf_gemv.hip) carries out what it returns and decides nothing.  The lanes per row fix the canonical
// summation order (oracle/kf_oracle.c section 4c), so the choice decides the bits: every threshold is a constant of this file, and gemv_lpr_log2 is the one
// lanes-per-row rule of the library -- the persistent engines' compile-time plans (kf_engine_common.h c_plan) are built from it.
#pragma once
#include "kf_kernels.h"

namespace kf {

constexpr int GEMV_EPB[9] = {8, 16, 32, 64, 128, 32, 32, 128, 64}; /* elements per 16-byte block, by FMT_* */

// ---- the lanes-per-row rule
// LPR: the largest power of two <= 64 dividing nBlk when that is >= 16 (no idle lanes), else the largest power of two <= min(64, nBlk) with the row tail masked.
// Short launches (fewer waves than the chip has SIMDs) are bound by the per-step dequant arithmetic of the longest wave, not by lanes: a row gets more lanes, even
// with the tail of the last step masked, while that shortens the step count (down_proj of the 0.6B model, 1024 x 3072: 512 waves x 3 steps -> 1024 waves x 2 steps).
// `rows` = the rows of every job of the launch.  1- and 2-bit rows (epb 128 / 64) take the rule's figure for K / 32 "virtual" blocks -- the dwords (dword pairs) of a
// block are what neighbouring lanes of the persistent engines multiply side by side (canonical order: a chain pair per 32-element sub-block) -- divided by the
// sub-blocks per block: logical lanes, one whole block each, in the mat-vec kernel.  The engines call it with their own 32-weight pieces (eng_vepb) or bf16 blocks.
constexpr int gemv_lpr_log2(int epb, int K, long rows) {
    if (epb == 128 || epb == 64) {
        const int l = gemv_lpr_log2(32, K, rows) - (epb == 128 ? 2 : 1);
        return l > 0 ? l : 0;
    }
    const int nBlk = K / epb;
    int l = 6;
    while (l > 0 && (nBlk % (1 << l)) != 0) l--;
    if ((1 << l) < 16) {
        l = 6;
        while ((1 << l) > nBlk) l--;
    }
    while (l < 6 && nBlk > (1 << l) && (rows << l) / 64 < 1024 && (nBlk + (2 << l) - 1) / (2 << l) < (nBlk + (1 << l) - 1) / (1 << l)) l++;
    return l;
}

// ---- the thresholds
// one wave per spw slots: small problems one slot per wave (latency-bound, as many waves as slots); large ones several rounds of resident waves so that memory waits
// of one wave are covered by the dequant arithmetic of the others (measured: 25600 x 5120 q4 41 -> 33 us; the Qwen3-32B q/k/v and o_proj launches, 22-28 MB each,
// 21.8 -> 19.1 and 16.1 -> 13.2 us; the 0.6B launches stay below the threshold)
constexpr long GEMV_WAVES = 4096;           /* waves a launch aims for (16 per CU) ... */
constexpr long GEMV_BIG_BLOCKS = 1L << 19;  /* ... and from this many 16-byte blocks (rows of every slot) */
constexpr long GEMV_BIG_WAVES = 16384;
// the largest launches (the 25600-row FFN matrices of Qwen3-32B): two slots per wave through the buffer-load form, half the workgroups to start and half the x staging
// (25600 x 5120: 27.6 -> 26.4 us, A/B in one run; smaller launches lose more from the coarser tail than they gain).  Not the sparse or row-codebook launches.
constexpr long GEMV_HUGE_BLOCKS = 4000000L;
constexpr long GEMV_HUGE_WAVES = 8192;
constexpr int GEMV_G_PAIRED_MAX = 2;        /* slots in flight per wave of a paired launch: two weight streams per slot, keep register pressure down */
constexpr unsigned long long GEMV_BLOCKS_MAX = 1ull << 32;   /* 16-byte blocks per matrix: the kernel's 32-bit block index (64 GiB) */
constexpr unsigned long long GEMV_STREAM_REACH = 1ull << 31; /* the buffer-load form: every byte offset a wave can form */
constexpr size_t GEMV_LDS_MAX = 160 * 1024;
constexpr size_t GEMV_RED_BYTES = 256;      /* the reduction scratch behind x in LDS */
constexpr size_t GEMV_Q2T_BYTES = 2048, GEMV_Q1T_BYTES = 4096; /* the v_perm selector tables of the 2- / 1-bit table forms */
constexpr int GEMV_Q4P_GROUP = 128;         /* the 4-bit register-table form: a 128-weight group is one aligned quad of lanes */
// the canonical 4-bit forms take x as fp32 in LDS while 4 K + 256 bytes stay inside 48 KiB (K <= 12224: every matrix of the 0.6B model, Q | K | V, o_proj and gate | up
// of Qwen3-32B and all of its TP = 8 shards; not its 25600-wide down_proj, where 100 KiB per workgroup would halve the resident waves) ...
constexpr size_t GEMV_XF_LDS_MAX = 48 * 1024;
// ... longer rows, one row slot per wave and no norm in front, half the block columns at a time (XF2) within three workgroups per CU
constexpr size_t GEMV_XF2_LDS_MAX = 54 * 1024;
constexpr int GEMV_XF2_RING = 4;            /* = gemv_kernel's ring of steps in flight: the first window holds whole rounds of it */

// ---- the problem: what a launch knows before it launches (a weight as GemmMat, kf_kernels.h)
struct GemvProblem {
    int mode;          /* GEMV_PLAIN, GEMV_PAIRED (w[0] gate, w[1] up), GEMV_ARGMAX */
    int n_w;           /* matrices (jobs), 1-3 */
    GemmMat w[3];
    int sparse, n_hot; /* the sparse forward: slots for n_hot hot rows of each matrix */
    int norm;          /* RMSNorm prologue */
    int canon;         /* the canonical summation order (kf_set_canonical) */
    int q4_perm, q2_tab, q1_tab, xf2; /* the A/B switches of kf::Knobs: 0 = the arithmetic reference form, resp. no XF2 */
};

// ---- the plan: gemv_kernel<fmt, G, mode, sparse, onejob, canon, xf, xf2> on grid x 256 threads with lds bytes, and the geometry the launcher copies into GemvArgs
struct GemvPlan {
    int status; /* KF_OK, or the refusal */
    int fmt, G, mode, sparse, onejob, canon, xf, xf2;
    int K, nBlk, lpr_log2, iters, lgroup, gshift;
    int njobs, M[3], slot0[3], spw, total_slots, stream_ok;
    int grid, lds;
};

inline int gemv_fmt(const GemmMat& m) { /* FMT_* of a stored weight before the table forms; < 0: not served by the mat-vec kernel */
    if (m.quant != KF_QUANT_GROUP) return (m.type == KF_Q4 && m.quant == KF_QUANT_ROW_LUT) ? FMT_Q4R : -1;
    switch (m.type) {
        case KF_BF16: return FMT_BF16;
        case KF_F8E5M2: return FMT_F8;
        case KF_Q4: return FMT_Q4;
        case KF_T_SIGN: return FMT_Q2;
        case KF_BOOL1: case KF_T_BINARY: return FMT_Q1;
        default: return -1;
    }
}

// ---- the rule
inline GemvPlan gemv_plan(const GemvProblem& P) {
    GemvPlan p = {};
    auto refuse = [&p](int status) {
        p.status = status;
        return p;
    };
    const int fmt = gemv_fmt(P.w[0]);
    if (fmt < 0) return refuse(KF_UNSUPPORTED_DATATYPE);
    const int K = P.w[0].K, epb = GEMV_EPB[fmt];
    if (K % epb != 0) return refuse(KF_INVALID_ARGS);
    const bool paired = P.mode == GEMV_PAIRED;
    long rows_all = 0;
    for (int j = 0; j < P.n_w; j++)
        if (!(paired && j == 1)) rows_all += P.w[j].M;
    const int nBlk = K / epb, lpr_log2 = gemv_lpr_log2(epb, K, rows_all), RPS = 64 >> lpr_log2;
    p.K = K, p.nBlk = nBlk, p.lpr_log2 = lpr_log2, p.iters = (nBlk + (1 << lpr_log2) - 1) >> lpr_log2;
    long rows_slots[3] = {0, 0, 0}, raw_slots = 0;
    for (int j = 0; j < P.n_w; j++) {
        const GemmMat& w = P.w[j];
        if (gemv_fmt(w) != fmt || w.K != K) return refuse(KF_INVALID_ARGS);
        if (w.awq) return refuse(KF_UNSUPPORTED_DATATYPE); /* AutoAWQ layout: kf_linear only */
        if (!(w.al & GM_DATA_AL)) return refuse(KF_BLAS_UNALIGN);
        if ((unsigned long long)w.M * (unsigned long long)nBlk >= GEMV_BLOCKS_MAX) return refuse(KF_INVALID_ARGS);
        if (fmt == FMT_Q4R) {
            if (!w.gama) return refuse(KF_QUANT_ERR);
            if (!(w.al & GM_TAB_AL)) return refuse(KF_BLAS_UNALIGN);
        } else if (fmt >= FMT_Q4) {
            if (!w.gama || w.lgroup <= 0 || (w.lgroup % epb) != 0 || ((long)w.M * w.K) % w.lgroup != 0) return refuse(KF_QUANT_ERR);
            const int bpg = w.lgroup / epb; /* blocks per group: a power of two (128-element groups always are) */
            if ((bpg & (bpg - 1)) != 0) return refuse(KF_QUANT_ERR);
            p.lgroup = w.lgroup, p.gshift = __builtin_ctz(bpg);
        }
        p.M[j] = P.sparse ? P.n_hot : w.M; /* sparse forward: only the hot rows get slots */
        if (paired && j == 1) {
            if (w.M != P.w[0].M) return refuse(KF_INVALID_ARGS);
            continue; /* job 1 rides on job 0's slots */
        }
        rows_slots[j] = (p.M[j] + RPS - 1) / RPS;
        raw_slots += rows_slots[j];
    }
    p.njobs = paired ? 1 : P.n_w;
    const long blocks_all = raw_slots * (long)nBlk * RPS;
    long target_waves = blocks_all >= GEMV_BIG_BLOCKS ? GEMV_BIG_WAVES : GEMV_WAVES;
    if (blocks_all >= GEMV_HUGE_BLOCKS && !P.sparse && fmt != FMT_Q4R) target_waves = GEMV_HUGE_WAVES;
    long spw = (raw_slots + target_waves - 1) / target_waves;
    if (spw < 1) spw = 1;
    int G = spw >= 4 ? 4 : (spw >= 2 ? 2 : 1);
    if (paired && G > GEMV_G_PAIRED_MAX) G = GEMV_G_PAIRED_MAX;
    spw = (spw + G - 1) / G * G;
    p.G = G, p.spw = (int)spw;
    // every job starts on a wave boundary, so a wave never straddles two jobs
    long slots = 0;
    for (int j = 0; j < 3; j++) {
        p.slot0[j] = j < p.njobs ? (int)slots : 0x7fffffff;
        if (j < p.njobs) slots += (rows_slots[j] + spw - 1) / spw * spw;
    }
    p.total_slots = (int)slots;
    // buffer-load form of the long launches (gemv_kernel, STREAM): every byte offset a wave can form -- rows of the padded slot range included -- inside the reach, and
    // groups that never straddle two rows (then the G rows of a batch are a constant number of groups apart)
    if (G > 1 && !P.sparse && fmt != FMT_Q4R) {
        long max_rows = 0;
        for (int j = 0; j < P.n_w; j++) max_rows = p.M[j] > max_rows ? p.M[j] : max_rows;
        const unsigned long long reach = ((unsigned long long)max_rows + (unsigned long long)(spw + G) * RPS) * nBlk * 16ull;
        p.stream_ok = reach < GEMV_STREAM_REACH && (fmt < FMT_Q4 || (K % p.lgroup) == 0);
    }
    p.grid = (int)(((slots + spw - 1) / spw + 3) / 4); /* four waves per workgroup */
    if (P.mode == GEMV_ARGMAX && p.grid > KF_MAX_ARGMAX_PARTIALS) return refuse(KF_INTERNAL_ERR);
    size_t lds = (size_t)K * 2 + GEMV_RED_BYTES;
    if (lds > GEMV_LDS_MAX) return refuse(KF_INVALID_ARGS);
    // the storage form: the table forms are bit-identical to the arithmetic ones (same weights, same pairing, same summation order).  4-bit: the register table whenever
    // a 128-weight group is exactly one aligned quad of lanes (20 % fewer VALU instructions per weight); 2- and 1-bit: the LDS selector tables while they fit
    p.fmt = fmt;
    if (fmt == FMT_Q4 && P.q4_perm && p.lgroup == GEMV_Q4P_GROUP && K % GEMV_Q4P_GROUP == 0 && lpr_log2 >= 2) p.fmt = FMT_Q4P;
    if (fmt == FMT_Q2 && P.q2_tab && lds + GEMV_Q2T_BYTES <= GEMV_LDS_MAX) p.fmt = FMT_Q2T, lds += GEMV_Q2T_BYTES;
    if (fmt == FMT_Q1 && P.q1_tab && lds + GEMV_Q1T_BYTES <= GEMV_LDS_MAX) p.fmt = FMT_Q1T, lds += GEMV_Q1T_BYTES;
    // the kernel form: the sparse forms are plain or paired; a launch of one matrix never reads the descriptors of jobs 1 and 2 (ONEJOB), a paired one reads job 1 by name
    p.mode = P.sparse && !paired ? GEMV_PLAIN : P.mode;
    p.sparse = P.sparse != 0, p.canon = P.canon != 0;
    p.onejob = !paired && (P.mode == GEMV_ARGMAX || P.sparse || p.njobs == 1);
    if (p.canon && fmt == FMT_Q4) { /* x as fp32 in LDS (XF), or half the block columns of it at a time (XF2) */
        const int it_half = (p.iters >> 1) / GEMV_XF2_RING * GEMV_XF2_RING; /* = the kernel's: whole rounds of its ring against the first window */
        const size_t lds_2 = (size_t)((p.iters - it_half) << lpr_log2) * 128 + GEMV_RED_BYTES;
        if (lds + (size_t)K * 2 <= GEMV_XF_LDS_MAX)
            p.xf = 1, lds += (size_t)K * 2;
        else if (p.mode == GEMV_PLAIN && !p.sparse && p.onejob && G == 1 && spw == 1 && !P.norm && it_half >= GEMV_XF2_RING && lds_2 <= GEMV_XF2_LDS_MAX && P.xf2)
            p.xf = p.xf2 = 1, lds = lds_2;
    }
    p.lds = (int)lds;
    return p;
}

// ---- the launcher (kf_gemv.hip): carries out a plan, nothing else
struct GemvLaunch {
    GemvArgs args;
    const kf_weight* w[3];
    int n;
    int mode;
    int n_hot;  /* args.row_map != NULL: number of entries */
    int canon;  /* the canonical summation order (one v_pk_fma_f32 per weight pair: an even and an odd chain per lane; oracle/kf_oracle.c section 4c) instead of v_dot2c_f32_bf16 */
    int row_unpack; /* kf_set_row_unpack: 3- / 2-bit row forms are planned as their 4-bit stand-in (kf_rowq.h) and run in registers; 0: refused as ever */
    int blocks; /* out */
};
GemvProblem gemv_problem(const GemvLaunch& L); /* what L asks for, with the process's knobs */
// p = gemv_plan(gemv_problem(L)) for L's weights and mode: its geometry, job descriptors and kernel form into L.args, then the launch.  KF_OK, p.status or KF_HIP_CHECK
int gemv_launch(hipStream_t st, GemvLaunch& L, const GemvPlan& p);
inline int gemv_launch(hipStream_t st, GemvLaunch& L) { return gemv_launch(st, L, gemv_plan(gemv_problem(L))); }
int gemv_dispatch_dot2(const GemvPlan& p, const GemvArgs& a, hipStream_t st);  /* kf_gemv.hip */
int gemv_dispatch_canon(const GemvPlan& p, const GemvArgs& a, hipStream_t st); /* kf_gemv_canon.hip: the canonical instantiations */

}  // namespace kf
