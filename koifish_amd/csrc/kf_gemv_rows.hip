// kf_gemv_rows.hip -- the canonical mat-vec of up to eight activation rows against ONE pass over the packed weights (the verify pass of speculative decoding: a
// token and its drafted continuations), gfx950 / wave64.  The sibling of gemv_kernel (kf_gemv_kernel.h) with the same data mapping; what makes activation row r carry
// every bit of the one-token launch on that row is shared by construction: the plan's figures (kf_gemv_rows_plan.h takes them from the one-token plan), the job
// selection, the two-chunk sum of squares, the block dots and the lane tree (kf_gemv_blocks.h), the epilogue rules and the pick (kf_device.h), the job fill on the host.
// Its own: a 16-byte block is loaded once and dequantised once into its 16 bf16 pair words (BlockPrep), then multiplied into one accumulator pair per activation row.
// LDS: the rows' activations, row after row, each laid out as the one-token kernel lays out its one | 256 B reduction scratch.
#include "kf_gemv_blocks.h"
#include "kf_gemv_rows_plan.h"

namespace kf {

template <bool PAIRED>
struct RowsBlk {
    u32x4 w, w2;
    uint16_t st, ze, st2, ze2;
};

// the 16-byte block as bf16 pair words in element order: 16 for a 4-bit block (BlockPrep), the block itself for bf16 storage
template <int FMT>
__device__ __forceinline__ void rows_prep(u32x4 w, float st, float ze, float nb, uint32_t (&P)[16]) {
    if constexpr (FMT == FMT_BF16) {
        P[0] = w.x, P[1] = w.y, P[2] = w.z, P[3] = w.w;
    } else {
        BlockPrep<FMT>::prep(w, st, ze, nb, (int)threadIdx.x, P);
    }
}
// one activation row's products of a block, in the order of BlockDot<FMT, true> (bf16 chunks) / BlockDotF<FMT> (fp32 chunks)
template <int FMT, bool XF>
__device__ __forceinline__ f32x2_t rows_dot(const uint32_t (&P)[16], const u32x4* xr, int col, int nBlk, f32x2_t acc) {
    if constexpr (FMT == FMT_BF16) {
        const u32x4 X = xr[col];
        acc = dotp<true>(P[0], X.x, acc);
        acc = dotp<true>(P[1], X.y, acc);
        acc = dotp<true>(P[2], X.z, acc);
        acc = dotp<true>(P[3], X.w, acc);
    } else if constexpr (XF) {
        acc = pairs_dot<true>(P, xr, col, nBlk, acc);
    } else {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const u32x4 X = xr[d * nBlk + col];
            acc = dotp<true>(P[4 * d], X.x, acc);
            acc = dotp<true>(P[4 * d + 1], X.y, acc);
            acc = dotp<true>(P[4 * d + 2], X.z, acc);
            acc = dotp<true>(P[4 * d + 3], X.w, acc);
        }
    }
    return acc;
}

template <int FMT, int NR, int MODE, bool XF_>
__global__ void __launch_bounds__(256) gemv_rows_kernel(const GemvRowsArgs a) {
    constexpr bool PAIRED = (MODE == GEMV_PAIRED), Q = (FMT != FMT_BF16), XF = XF_ && Q;
    constexpr int XCH = Q ? 4 : 1; /* bf16 chunks of 8 per block */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem_raw);
    const int nr = a.nr, nBlk = a.nBlk, iters = a.iters, nch = a.K >> 3;
    const int row_chunks = nch * (XF ? 2 : 1); /* 16-byte words of one activation row in LDS */
    double* red = reinterpret_cast<double*>(smem_raw + (size_t)nr * row_chunks * 16);
    const int tid = threadIdx.x, lane = tid & 63, wave_in_blk = tid >> 6;
    const int LPR = 1 << a.lpr_log2, RPS = 64 >> a.lpr_log2;
    const int sub = lane >> a.lpr_log2, ll = lane & (LPR - 1);
    const long gwave = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(wave_in_blk);
    const long s_begin = gwave * a.spw;
    long s_end = s_begin + a.spw;
    if (s_end > a.total_slots) s_end = a.total_slots;
    const int nsteps = s_end > s_begin ? (int)(s_end - s_begin) * iters : 0;

    const GemvJobSel js = gemv_job_sel<false>(a, s_begin); /* the wave's job, scalar for the whole loop */
    const u32x4* const jw = js.w;
    const u32x4* const jw2 = reinterpret_cast<const u32x4*>(a.job[1].w);
    const uint16_t* const jstep = js.step;
    const uint16_t* const jzero = js.zero;
    uint16_t* const jy = js.y;
    const long long jystride = js.y_pos_stride;
    const long long jyrow = js.jx == 0 ? a.y_row_stride[0] : (js.jx == 1 ? a.y_row_stride[1] : a.y_row_stride[2]);
    const int jM = js.M, jslot0 = js.slot0;
    const float jqb = js.qb, jqb2 = (float)a.job[1].qBias;
    const int gshift = a.gshift;

    // unconditional loads from a clamped (row, column): a lane outside the matrix re-reads a valid block and is masked when the block is multiplied (gemv_kernel, LAT)
    auto load = [&](long s, int it, RowsBlk<PAIRED>& b) {
        int row = (int)(s - jslot0) * RPS + sub, col = it * LPR + ll;
        row = row < jM ? row : jM - 1;
        row = row > 0 ? row : 0;
        col = col < nBlk ? col : nBlk - 1;
        const uint32_t bidx = (uint32_t)row * (uint32_t)nBlk + (uint32_t)col;
        b.w = ld_nt(jw + bidx);
        if constexpr (PAIRED) b.w2 = ld_nt(jw2 + bidx);
        if constexpr (Q) {
            const uint32_t gi = bidx >> gshift;
            b.st = jstep[gi], b.ze = jzero[gi];
            if constexpr (PAIRED) b.st2 = a.job[1].step[gi], b.ze2 = a.job[1].zero[gi];
        }
    };
    RowsBlk<PAIRED> cur, nxt;
    load(s_begin, 0, cur); /* before the prologue: the weights' HBM latency overlaps the staging (a wave without work re-reads a valid block) */

    // ---- prologue: every row's activations into LDS, behind its RMSNorm when there is one.  The sum of squares of a row is formed as the one-token kernel forms it
    // on that row: from two chunks per thread (norm_regs), or in the strided element pass of block_sumsq_bf16
    const bool has_norm = a.norm_w != nullptr;
    if (has_norm) {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            if (r >= nr) break;
            const uint16_t* xr = a.x + (size_t)r * a.x_stride;
            double ss;
            if (a.norm_regs) {
                const bool h0 = tid < nch, h1 = tid + 256 < nch;
                const u32x4 r0 = *reinterpret_cast<const u32x4*>(xr + (size_t)(h0 ? tid : 0) * 8), r1 = *reinterpret_cast<const u32x4*>(xr + (size_t)(h1 ? tid + 256 : 0) * 8);
                ss = sumsq_2chunks(r0, r1, h0, h1);
            } else {
                ss = 0.0;
                for (int i = tid; i < a.K; i += 256) {
                    const double v = (double)bf2f(xr[i]);
                    ss = fma(v, v, ss);
                }
            }
            ss = wave_sum_f64_fast(ss);
            if (lane == 0) red[r * 4 + wave_in_blk] = ss;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < nr * nch; idx += 256) {
        const int r = idx / nch, e8 = idx - r * nch;
        const u32x4 raw = *reinterpret_cast<const u32x4*>(a.x + (size_t)r * a.x_stride + (size_t)e8 * 8);
        u32x4 o = raw;
        if (has_norm) {
            const double* rr = red + r * 4;
            const double tot = a.norm_regs ? (rr[0] + rr[1]) + (rr[2] + rr[3]) : (((0.0 + rr[0]) + rr[1]) + rr[2]) + rr[3];
            const float mul = rms_scale((float)tot, a.inv_dim, a.eps);
            const u32x4 nw = *reinterpret_cast<const u32x4*>(a.norm_w + (size_t)e8 * 8);
            const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, ww[4] = {nw.x, nw.y, nw.z, nw.w};
            uint32_t ow[4];
#pragma unroll
            for (int k = 0; k < 4; k++) ow[k] = rms_pair(rw[k], ww[k], mul);
            o = u32x4{ow[0], ow[1], ow[2], ow[3]};
        }
        // element e of block column c, chunk j (e = c * EPB + j * 8 + i) -> the row's LDS chunk j * nBlk + c (XF: the two fp32 chunks 2 j, 2 j + 1)
        const int c = e8 / XCH, j = e8 - c * XCH;
        u32x4* xr = xs + (size_t)r * row_chunks;
        if constexpr (XF) {
            xr[(2 * j) * nBlk + c] = widen_bf16x4(o.x, o.y);
            xr[(2 * j + 1) * nBlk + c] = widen_bf16x4(o.z, o.w);
        } else {
            xr[j * nBlk + c] = o;
        }
    }
    __syncthreads();

    // ---- main: one (slot, iteration) step at a time, the next step's block in flight
    f32x2_t acc[NR], acc2[PAIRED ? NR : 1];
    float best_v[MODE == GEMV_ARGMAX ? NR : 1];
    int best_i[MODE == GEMV_ARGMAX ? NR : 1];
    if constexpr (MODE == GEMV_ARGMAX) {
#pragma unroll
        for (int r = 0; r < NR; r++) best_v[r] = FIRST_MAX_NONE_V, best_i[r] = FIRST_MAX_NONE_I;
    }
    int bi = 0, it = 0, nbi = 0, nit = 0;
    for (int k = 0; k < nsteps; k++) {
        if (k + 1 < nsteps) {
            if (++nit == iters) nit = 0, nbi++;
            load(s_begin + nbi, nit, nxt);
        }
        if (it == 0) {
#pragma unroll
            for (int r = 0; r < NR; r++) {
                acc[r] = f32x2_t{0.0f, 0.0f};
                if constexpr (PAIRED) acc2[r] = f32x2_t{0.0f, 0.0f};
            }
        }
        const int row = (int)(s_begin + bi - jslot0) * RPS + sub;
        int col = it * LPR + ll;
        const bool ok = row < jM && col < nBlk;
        if (col >= nBlk) col = nBlk - 1; /* keep the LDS reads in range */
        {
            uint32_t P[16];
            const float st = Q ? bf2f(cur.st) : 0.0f;
            rows_prep<FMT>(cur.w, st, Q ? bf2f(cur.ze) : 0.0f, -(jqb * st), P);
#pragma unroll
            for (int r = 0; r < NR; r++)
                if (r < nr) acc[r] = acc_pick(ok, rows_dot<FMT, XF>(P, xs + (size_t)r * row_chunks, col, nBlk, acc[r]), acc[r]);
        }
        if constexpr (PAIRED) {
            uint32_t P[16];
            const float st2 = Q ? bf2f(cur.st2) : 0.0f;
            rows_prep<FMT>(cur.w2, st2, Q ? bf2f(cur.ze2) : 0.0f, -(jqb2 * st2), P);
#pragma unroll
            for (int r = 0; r < NR; r++)
                if (r < nr) acc2[r] = acc_pick(ok, rows_dot<FMT, XF>(P, xs + (size_t)r * row_chunks, col, nBlk, acc2[r]), acc2[r]);
        }
        if (it == iters - 1) {
#pragma unroll
            for (int r = 0; r < NR; r++) {
                if (r >= nr) break;
                const float v = group_sum(acc_join(acc[r]), a.lpr_log2);
                float v2 = 0.0f;
                if constexpr (PAIRED) v2 = group_sum(acc_join(acc2[r]), a.lpr_log2);
                if (ll == 0 && row < jM) {
                    uint16_t* y = jy ? jy + (size_t)r * jyrow + (size_t)(a.pos0 + r) * jystride : nullptr;
                    if constexpr (PAIRED) {
                        y[row] = swiglu_bf16(round_bf16(v), round_bf16(v2));
                    } else {
                        /* alpha = 1, beta = 0, no bias; the residual is read before the store: it may alias y */
                        const uint16_t o = linear_out_bf16(v, 1.0f, 0.0f, nullptr, 0, nullptr, 0, a.residual, (size_t)r * a.res_stride + row);
                        if (y) y[row] = o;
                        if constexpr (MODE == GEMV_ARGMAX) first_max(best_v[r], best_i[r], bf2f(o), row);
                    }
                }
            }
        }
        if (++it == iters) it = 0, bi++;
        cur = nxt;
    }

    if constexpr (MODE == GEMV_ARGMAX) { /* per row: the first maximum over this workgroup's weight rows (gemv_kernel) */
        float* rv = reinterpret_cast<float*>(red);
        int* ri = reinterpret_cast<int*>(rv + 32);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; r++) {
            if (r >= nr) break;
            float bv = best_v[r];
            int bx = best_i[r];
            wave_first_max(bv, bx);
            if (lane == 0) rv[r * 4 + wave_in_blk] = bv, ri[r * 4 + wave_in_blk] = bx;
        }
        __syncthreads();
        if (tid < nr) { /* thread r folds row r's four waves in order */
            float bv = rv[tid * 4];
            int bx = ri[tid * 4];
            waves_first_max(bv, bx, rv + tid * 4, ri + tid * 4, 1, 4);
            a.amax_val[(size_t)tid * gridDim.x + blockIdx.x] = bv;
            a.amax_idx[(size_t)tid * gridDim.x + blockIdx.x] = bx;
        }
    }
}

// the pick over a row's per-workgroup partial maxima: workgroup r takes row r (first maximum, ties to the lower id)
__global__ void __launch_bounds__(256) argmax_rows_finish_kernel(const float* val, const int* idx, int n, int32_t* d_top1) {
    const float* v = val + (size_t)blockIdx.x * n;
    const int* ix = idx + (size_t)blockIdx.x * n;
    float bv = FIRST_MAX_NONE_V;
    int bi = FIRST_MAX_NONE_I;
    for (int i = threadIdx.x; i < n; i += 256) first_max(bv, bi, v + i, ix + i);
    block_first_max_256(bv, bi);
    if (threadIdx.x == 0) d_top1[blockIdx.x] = bi;
}
void argmax_rows_finish_launch(hipStream_t st, const float* val, const int* idx, int n, int n_rows, int32_t* d_top1) {
    hipLaunchKernelGGL(argmax_rows_finish_kernel, dim3(n_rows), dim3(256), 0, st, val, idx, n, d_top1);
}

// ---- the forms a plan can name: storage (bf16, 4-bit arithmetic, 4-bit register table) x NR 4 / 8 x mode x XF (4-bit only)
using GemvRowsKernel = void (*)(GemvRowsArgs);
template <int FMT, int NR, int MODE>
static GemvRowsKernel rows_form_xf(bool xf) {
    if constexpr (FMT == FMT_BF16) return gemv_rows_kernel<FMT, NR, MODE, false>;
    else return xf ? gemv_rows_kernel<FMT, NR, MODE, true> : gemv_rows_kernel<FMT, NR, MODE, false>;
}
template <int FMT, int NR>
static GemvRowsKernel rows_form_mode(int mode, bool xf) {
    return mode == GEMV_PAIRED ? rows_form_xf<FMT, NR, GEMV_PAIRED>(xf) : mode == GEMV_ARGMAX ? rows_form_xf<FMT, NR, GEMV_ARGMAX>(xf) : rows_form_xf<FMT, NR, GEMV_PLAIN>(xf);
}
template <int FMT>
static GemvRowsKernel rows_form_nr(int NR, int mode, bool xf) {
    return NR == GEMV_ROWS_NR_SMALL ? rows_form_mode<FMT, GEMV_ROWS_NR_SMALL>(mode, xf) : NR == GEMV_ROWS_MAX ? rows_form_mode<FMT, GEMV_ROWS_MAX>(mode, xf) : nullptr;
}
static GemvRowsKernel rows_form(const GemvRowsPlan& p) {
    return p.fmt == FMT_BF16 ? rows_form_nr<FMT_BF16>(p.NR, p.mode, false) : p.fmt == FMT_Q4 ? rows_form_nr<FMT_Q4>(p.NR, p.mode, p.xf) : p.fmt == FMT_Q4P ? rows_form_nr<FMT_Q4P>(p.NR, p.mode, p.xf) : nullptr;
}

GemvRowsProblem gemv_rows_problem(const GemvRowsLaunch& L, int canon) {
    GemvLaunch one = {};
    one.n = L.n, one.mode = L.mode, one.canon = canon;
    for (int j = 0; j < L.n; j++) one.w[j] = L.w[j];
    one.args.norm_w = L.args.norm_w;
    GemvRowsProblem P = {};
    P.one = gemv_problem(one), P.n_rows = L.n_rows;
    return P;
}

int gemv_rows_launch(hipStream_t st, GemvRowsLaunch& L, const GemvRowsPlan& p) {
    if (p.status) return p.status;
    const GemvRowsKernel k = p.shared ? rows_form(p) : nullptr;
    if (!k) return KF_INTERNAL_ERR; /* a form gemv_rows_plan never names */
    GemvRowsArgs a = L.args;
    a.njobs = p.njobs, a.K = p.K, a.nBlk = p.nBlk, a.lpr_log2 = p.lpr_log2, a.iters = p.iters, a.gshift = p.gshift;
    a.spw = p.spw, a.total_slots = p.total_slots, a.norm_regs = p.norm_regs;
    a.inv_dim = 1.0f / (float)p.K;
    gemv_fill_jobs(a.job, p.slot0, p.M, L.w, L.n, p.fmt);
    if (p.lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds) != hipSuccess) return KF_HIP_CHECK;
    for (int r0 = 0; r0 < L.n_rows; r0 += p.panel_rows) {
        GemvRowsArgs b = a;
        b.nr = L.n_rows - r0 < p.panel_rows ? L.n_rows - r0 : p.panel_rows;
        b.x = a.x + (size_t)r0 * a.x_stride, b.pos0 = a.pos0 + r0;
        if (a.residual) b.residual = a.residual + (size_t)r0 * a.res_stride;
        for (int j = 0; j < 3; j++)
            if (b.job[j].y) b.job[j].y += (size_t)r0 * a.y_row_stride[j];
        if (a.amax_val) b.amax_val = a.amax_val + (size_t)r0 * p.grid, b.amax_idx = a.amax_idx + (size_t)r0 * p.grid;
        void* args[] = {&b};
        (void)hipLaunchKernel(reinterpret_cast<const void*>(k), dim3(p.grid), dim3(256), args, (size_t)p.lds, st);
        if (hipGetLastError() != hipSuccess) return KF_HIP_CHECK;
    }
    return KF_OK;
}

}  // namespace kf
