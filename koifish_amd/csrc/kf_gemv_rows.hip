// kf_gemv_rows.hip -- the canonical mat-vec of up to eight activation rows against ONE pass over the packed weights (the verify pass of speculative decoding: a
// token and its drafted continuations), gfx950 / wave64.  A sibling of gemv_kernel (kf_gemv_kernel.h): the same data mapping -- LPR lanes walk a weight row, 64 / LPR
// weight rows side by side per wave slot, ITERS loads per row, the lanes per row from kf::gemv_lpr_log2 -- the same even / odd chain pair per lane, the same lane tree
// and the same epilogue arithmetic, so activation row r of a launch carries every bit of the one-token launch on that row (kf_gemv_rows_plan.h takes those figures
// from the one-token plan).  What is shared is the weight side: a 16-byte block is loaded once and dequantised once into its 16 bf16 pair words (BlockPrep, the
// persistent engine's "dequantise ahead" form, kf_gemv_blocks.h), then multiplied into one accumulator pair per activation row.
// LDS: the rows' activations, row after row, each laid out as the one-token kernel lays out its one ([chunk j of block][block column], bf16 chunks of 8 or, XF, fp32
// chunks of 4) | 256 B reduction scratch.
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

    // a wave works inside one job (the plan pads each job's slot range to whole waves): its fields are picked once and stay scalar (gemv_kernel)
    int jx = 0;
    if (a.njobs > 1 && s_begin >= a.job[1].slot0) jx = 1;
    if (a.njobs > 2 && s_begin >= a.job[2].slot0) jx = 2;
    jx = __builtin_amdgcn_readfirstlane(jx);
#define JF(f) (jx == 0 ? a.job[0].f : (jx == 1 ? a.job[1].f : a.job[2].f))
    const u32x4* const jw = reinterpret_cast<const u32x4*>(JF(w));
    const u32x4* const jw2 = reinterpret_cast<const u32x4*>(a.job[1].w);
    const uint16_t* const jstep = JF(step);
    const uint16_t* const jzero = JF(zero);
    uint16_t* const jy = JF(y);
    const long long jystride = JF(y_pos_stride);
    const long long jyrow = jx == 0 ? a.y_row_stride[0] : (jx == 1 ? a.y_row_stride[1] : a.y_row_stride[2]);
    const int jM = JF(M), jslot0 = JF(slot0);
    const float jqb = (float)JF(qBias), jqb2 = (float)a.job[1].qBias;
#undef JF
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
                const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                double ss0 = 0.0, ss1 = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double lo = (double)bf_lo(rw[k]), hi = (double)bf_hi(rw[k]), lo1 = (double)bf_lo(rw[4 + k]), hi1 = (double)bf_hi(rw[4 + k]);
                    ss0 = fma(lo, lo, ss0), ss0 = fma(hi, hi, ss0);
                    ss1 = fma(lo1, lo1, ss1), ss1 = fma(hi1, hi1, ss1);
                }
                ss = (h0 ? ss0 : 0.0) + (h1 ? ss1 : 0.0);
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
            const float mul = 1.0f / sqrtf(fmaf((float)tot, a.inv_dim, a.eps));
            const u32x4 nw = *reinterpret_cast<const u32x4*>(a.norm_w + (size_t)e8 * 8);
            const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, ww[4] = {nw.x, nw.y, nw.z, nw.w};
            uint32_t ow[4];
#pragma unroll
            for (int k = 0; k < 4; k++) ow[k] = pack_bf16x2((bf_lo(rw[k]) * mul) * bf_lo(ww[k]), (bf_hi(rw[k]) * mul) * bf_hi(ww[k]));
            o = u32x4{ow[0], ow[1], ow[2], ow[3]};
        }
        // element e of block column c, chunk j (e = c * EPB + j * 8 + i) -> the row's LDS chunk j * nBlk + c (XF: the two fp32 chunks 2 j, 2 j + 1)
        const int c = e8 / XCH, j = e8 - c * XCH;
        u32x4* xr = xs + (size_t)r * row_chunks;
        if constexpr (XF) {
            xr[(2 * j) * nBlk + c] = u32x4{o.x << 16, o.x & 0xffff0000u, o.y << 16, o.y & 0xffff0000u};
            xr[(2 * j + 1) * nBlk + c] = u32x4{o.z << 16, o.z & 0xffff0000u, o.w << 16, o.w & 0xffff0000u};
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
        for (int r = 0; r < NR; r++) best_v[r] = -__builtin_inff(), best_i[r] = 0x7fffffff;
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
                    if constexpr (PAIRED) { /* SwiGLU of the two bf16-rounded projections (gemv_kernel) */
                        const float gt = round_bf16(v), up = round_bf16(v2);
                        y[row] = f2bf((gt * up) / (1.0f + kf_expf(-gt)));
                    } else {
                        uint16_t o = f2bf(v);
                        if (a.residual) o = f2bf(bf2f(a.residual[(size_t)r * a.res_stride + row]) + bf2f(o)); /* read before the store: residual may alias y */
                        if (y) y[row] = o;
                        if constexpr (MODE == GEMV_ARGMAX) {
                            const float fv = bf2f(o);
                            if (fv > best_v[r] || (fv == best_v[r] && row < best_i[r])) best_v[r] = fv, best_i[r] = row;
                        }
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
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                const float ov = __shfl_xor(bv, m, 64);
                const int oi = __shfl_xor(bx, m, 64);
                if (ov > bv || (ov == bv && oi < bx)) bv = ov, bx = oi;
            }
            if (lane == 0) rv[r * 4 + wave_in_blk] = bv, ri[r * 4 + wave_in_blk] = bx;
        }
        __syncthreads();
        if (tid < nr) {
            float bv = rv[tid * 4];
            int bx = ri[tid * 4];
            for (int w = 1; w < 4; w++)
                if (rv[tid * 4 + w] > bv || (rv[tid * 4 + w] == bv && ri[tid * 4 + w] < bx)) bv = rv[tid * 4 + w], bx = ri[tid * 4 + w];
            a.amax_val[(size_t)tid * gridDim.x + blockIdx.x] = bv;
            a.amax_idx[(size_t)tid * gridDim.x + blockIdx.x] = bx;
        }
    }
}

// the pick over a row's per-workgroup partial maxima: workgroup r takes row r (first maximum, ties to the lower id)
__global__ void __launch_bounds__(256) argmax_rows_finish_kernel(const float* val, const int* idx, int n, int32_t* d_top1) {
    const float* v = val + (size_t)blockIdx.x * n;
    const int* ix = idx + (size_t)blockIdx.x * n;
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256)
        if (v[i] > bv || (v[i] == bv && ix[i] < bi)) bv = v[i], bi = ix[i];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float ov = __shfl_xor(bv, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    __shared__ float sv[4];
    __shared__ int si[4];
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) bv = sv[w], bi = si[w];
        d_top1[blockIdx.x] = bi;
    }
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
    for (int j = 0; j < 3; j++) {
        GemvJob& jb = a.job[j];
        jb.slot0 = p.slot0[j];
        if (j >= L.n) continue;
        const kf_weight* w = L.w[j];
        jb.w = w->data, jb.M = p.M[j], jb.qBias = w->qBias;
        jb.zero = jb.step = nullptr;
        if (p.fmt != FMT_BF16) jb.zero = w->gama + w->ne0 + w->ne1, jb.step = jb.zero + (size_t)w->ne0 * w->ne1 / w->lGroup; /* gemv_launch */
    }
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
