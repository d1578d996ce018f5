// kf_gemv_kernel.h -- fused PackedQ unpack + mat-vec for decode (nTok = 1), gfx950 / wave64.
//
// Replaces GTensor::GetDataX (dequantise the whole weight to bf16 in gBUFF->tmpTernary, quantizer.cu:249-392)
// followed by cuBLASLt (gemm.cu:93-214): the packed stream is read ONCE, 16 bytes per lane, fully coalesced,
// dequantised in registers with the reference's bf16-stepwise arithmetic (T.cu:274) and contracted against the
// activation held in LDS.  HBM-bound: algorithmic bytes = packed data + zero/step (+ x, y).
//
// Data mapping.  W[M,K] row-major flattened is a stream of 16-byte blocks (one Packed128 for 4/2/1-bit; 8 bf16;
// 16 f8).  EPB = elements per block; a row has nBlk = K/EPB blocks.  LPR lanes (a power of two <= 64) walk one
// row, RPS = 64/LPR rows are processed side by side by one wave ("slot"), ITERS = ceil(nBlk/LPR) loads per row.
// Each wave owns SPW consecutive slots and keeps G of them in flight.  x sits in LDS as 16-byte chunks laid
// out [chunk j of block][block column] so that consecutive lanes read consecutive 16-byte words (no bank
// conflicts for ds_read_b128).
// Two translation units instantiate it: kf_gemv.hip (the v_dot2c_f32_bf16 forms) and kf_gemv_canon.hip (CANON: the canonical order of oracle/kf_oracle.c section 4c,
// two v_fma_f32 per weight pair, every output bit reproducible with fmaf on the host).  Same kernels, same geometry; gemv_launch picks by the plan's canon.
#pragma once
#include <stdlib.h>

#include <array>
#include <utility>

#include "kf_gemv_blocks.h"
#include "kf_gemv_plan.h"

namespace kf {

template <int G, bool PAIRED, bool LUT, bool LUT16 = LUT>
struct Batch {
    u32x4 w[G];
    u32x4 w2[PAIRED ? G : 1];
    u32x4 ta[LUT ? G : 1], tb[LUT16 ? G : 1];                     /* row codebook (FMT_Q4R: 16 entries in ta | tb; the 3- / 2-bit row forms: ta alone) */
    u32x4 ta2[LUT && PAIRED ? G : 1], tb2[LUT16 && PAIRED ? G : 1];
    // zero / step stay raw bf16 bits until the block is multiplied: converted when loaded, the shift makes the wave wait for the loads it has
    // just issued (s_waitcnt vmcnt right behind the prefetch) instead of overlapping them with the current batch's arithmetic
    uint16_t st[G], ze[G];
    uint16_t st2[PAIRED ? G : 1], ze2[PAIRED ? G : 1];
};

// LDS: x as u32x4 chunks [XCH][nBlk] (K*2 bytes) | 256 B reduction scratch.
// Each wave keeps two batches of G blocks in flight: the first batch is issued BEFORE the x prologue so that the
// weight stream's HBM latency overlaps the (dependent) activation load + norm.
// ONEJOB: a launch with a single matrix (o_proj, down_proj, LM head, sparse rows) never reads the descriptors of jobs 1 and 2: kernel arguments are fetched ahead of the
// first load, and every one a launch touches is on its critical path
// XF (canonical 4-bit forms only, chosen by the plan, kf_gemv_plan.h, when K * 4 bytes of LDS leave the occupancy alone): x is staged as fp32 chunks [8][nBlk] and multiplied through
// BlockDotF (the engine's form): a product is two conversions of the weight pair + one v_pk_fma_f32 instead of four conversions + one -- same chains, same bits
// XF2 (XF of a row too long for that: the 25600-wide down_proj of Qwen3-32B, one row slot per wave): the fp32 chunks of HALF the block columns at a time -- the iterations
// of the first half run against the first window, then the workgroup restages and the same chains go on over the second (weights stay in flight across the two barriers)
template <int FMT, int G, int MODE, bool SPARSE, bool ONEJOB, bool CANON, bool XF_ = false, bool XF2_ = false>
__global__ void __launch_bounds__(256) gemv_kernel(const GemvArgs a) {
    using BD = BlockDot<FMT, CANON>;
    constexpr bool PAIRED = (MODE == GEMV_PAIRED), ROWQ = fmt_rowq(FMT), LUT16 = (FMT == FMT_Q4R), LUT = LUT16 || ROWQ, XF = XF_ && CANON && (FMT == FMT_Q4 || FMT == FMT_Q4P);
    using BatchT = Batch<G, PAIRED, LUT, LUT16>;
    constexpr bool XF2 = XF2_ && XF && G == 1 && !PAIRED && !SPARSE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem_raw);
    constexpr int RD = 4; /* XF2: a ring of four steps in flight per wave (25 steps per row behind ONE step of prefetch left the launch latency-bound: 1.7 TB/s) */
    const int it_half = XF2 ? (a.iters >> 1) / RD * RD : a.iters;        /* iterations against the first window: whole ring rounds */
    const int wcols = XF2 ? (a.iters - it_half) << a.lpr_log2 : a.nBlk;   /* block columns of the (larger, second) window = the chunk stride of the staged activations */
    const int wcol0 = it_half << a.lpr_log2;                              /* first block column of the second window */
    double* red = reinterpret_cast<double*>(smem_raw + (XF2 ? (size_t)wcols * 128 : (size_t)a.K * (XF ? 4 : 2)));

    const int tid = threadIdx.x, lane = tid & 63, wave_in_blk = tid >> 6;
    const int nBlk = a.nBlk, iters = a.iters;
    if constexpr (FMT == FMT_Q2T) { /* selector table: entry B, dword p = bytes {2q, 2q+1, 2q', 2q'+1}, q / q' = the levels of elements 2p, 2p+1 of byte B */
        uint32_t e[2];
#pragma unroll
        for (int p = 0; p < 2; p++) e[p] = 0x01000100u + 0x0202u * ((tid >> (6 - 4 * p)) & 3u) + 0x02020000u * ((tid >> (4 - 4 * p)) & 3u);
        reinterpret_cast<u32x2*>(xs + nBlk * 8 + 16)[tid] = u32x2{e[0], e[1]};
    }
    if constexpr (FMT == FMT_Q1T) { /* selector table: entry B, dword p = bytes {2a, 2a+1, 2b, 2b+1}, a / b = bits 7-2p / 6-2p of B (elements 2p, 2p+1) */
        uint32_t e[4];
#pragma unroll
        for (int p = 0; p < 4; p++) e[p] = 0x01000100u + 0x0202u * ((tid >> (7 - 2 * p)) & 1u) + 0x02020000u * ((tid >> (6 - 2 * p)) & 1u);
        (xs + nBlk * 16 + 16)[tid] = u32x4{e[0], e[1], e[2], e[3]}; /* 256 threads, 256 entries; visible after the prologue's barrier */
    }
    const int LPR = 1 << a.lpr_log2, RPS = 64 >> a.lpr_log2;
    const int sub = lane >> a.lpr_log2, ll = lane & (LPR - 1);
    const long gwave = (long)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(wave_in_blk); /* wave-uniform: the slot range and step count stay scalar */
    const long s_begin = gwave * a.spw;
    long s_end = s_begin + a.spw;
    if (s_end > a.total_slots) s_end = a.total_slots;
    const int nbatch = s_end > s_begin ? (int)((s_end - s_begin + G - 1) / G) : 0;
    const int nsteps = nbatch * iters;

    const GemvJobSel js = gemv_job_sel<ONEJOB>(a, s_begin); /* the wave's job, scalar for the whole loop (kf_gemv_blocks.h) */
    const u32x4* const jw = js.w;
    const u32x4* const jw2 = reinterpret_cast<const u32x4*>(a.job[1].w);
    const uint16_t* const jstep = js.step;
    const uint16_t* const jzero = js.zero;
    uint16_t* const jy = js.y;
    const long long jystride = js.y_pos_stride;
    const int jM = js.M, jslot0 = js.slot0;
    const float jqb = js.qb, jqb2 = (float)a.job[1].qBias;
    const int gshift = a.gshift;
    auto slot = [&](long s, int& row) -> bool {
        row = (int)(s - jslot0) * RPS + sub;
        return (s < s_end) && (row < jM);
    };
    // Two load policies.  LAT (one slot per wave: the short, latency-bound launches of decode): unconditional loads from clamped
    // (row, column) -- a lane outside the matrix re-reads a valid block and is masked when the block is multiplied -- because loads under
    // a lane condition make the number of loads in flight path-dependent and every wait behind them a drain (vmcnt(0)), including the
    // wait for x, which is requested FIRST so that its staging overlaps the weights' HBM latency.  Long launches (G > 1) are bound by
    // the dequant arithmetic and hide latency with resident waves: they keep the masked loads (no per-step mask arithmetic).
    constexpr bool LAT = (G == 1);
    auto load = [&](int bi, int it, BatchT& b) {
        const long s0 = s_begin + (long)bi * G;
        int col = it * LPR + ll;
        const bool col_ok = col < nBlk;
        col = col_ok ? col : nBlk - 1;
#pragma unroll
        for (int g = 0; g < G; g++) {
            int row;
            const bool ok = slot(s0 + g, row) && col_ok;
            if constexpr (LAT) {
                row = row < jM ? row : jM - 1;
                row = row > 0 ? row : 0;
            } else {
                b.w[g] = u32x4{0, 0, 0, 0};
                b.st[g] = b.ze[g] = 0;
                if (PAIRED) b.w2[g] = u32x4{0, 0, 0, 0}, b.st2[g] = b.ze2[g] = 0;
                if constexpr (LUT) {
                    b.ta[g] = u32x4{0, 0, 0, 0};
                    if constexpr (PAIRED) b.ta2[g] = u32x4{0, 0, 0, 0};
                }
                if constexpr (LUT16) {
                    b.tb[g] = u32x4{0, 0, 0, 0};
                    if constexpr (PAIRED) b.tb2[g] = u32x4{0, 0, 0, 0};
                }
            }
            if (LAT || ok) {
                if constexpr (SPARSE) row = a.row_map[row]; /* sparse forward: the slot's row is the row-th hot row (one dependent, wave-uniform-per-group load).  A template
                                                              parameter: as a run-time branch its join carried an s_waitcnt vmcnt(0) that drained the weight stream of every launch */
                const uint32_t bidx = (uint32_t)row * (uint32_t)nBlk + (uint32_t)col; /* < 2^32 blocks = 64 GiB per tensor */
                if constexpr (ROWQ) { /* a unit of 12 / 8 bytes; consecutive lanes read consecutive units (rows start 16-byte aligned: K a multiple of 128) */
                    constexpr int UB = rowq_unit_bytes(FMT);
                    b.w[g] = ld_unit<UB>(reinterpret_cast<const unsigned char*>(jw) + (size_t)bidx * UB);
                    if constexpr (PAIRED) b.w2[g] = ld_unit<UB>(reinterpret_cast<const unsigned char*>(jw2) + (size_t)bidx * UB);
                } else {
                    b.w[g] = ld_nt(jw + bidx);
                    if (PAIRED) b.w2[g] = ld_nt(jw2 + bidx);
                }
                if (BD::HAS_GAMA) {
                    const uint32_t gi = bidx >> gshift; /* group = element / lGroup, lGroup / EPB a power of two */
                    b.st[g] = jstep[gi], b.ze[g] = jzero[gi];
                    if (PAIRED) b.st2[g] = a.job[1].step[gi], b.ze2[g] = a.job[1].zero[gi];
                }
                if constexpr (ROWQ) { /* job.zero carries the table base: 8 / 4 / 2 bf16 per row, aligned to their size */
                    auto tab = [&](const uint16_t* base) -> u32x4 {
                        if constexpr (FMT == FMT_Q3R) return reinterpret_cast<const u32x4*>(base)[row];
                        else if constexpr (FMT == FMT_Q2R) {
                            const u32x2 v = reinterpret_cast<const u32x2*>(base)[row];
                            return u32x4{v.x, v.y, 0u, 0u};
                        } else return u32x4{reinterpret_cast<const uint32_t*>(base)[row], 0u, 0u, 0u};
                    };
                    b.ta[g] = tab(jzero);
                    if constexpr (PAIRED) b.ta2[g] = tab(a.job[1].zero);
                }
                if constexpr (LUT16) { /* job.zero carries the table base: 16 bf16 per row */
                    const u32x4* lt = reinterpret_cast<const u32x4*>(jzero) + 2 * (size_t)row;
                    b.ta[g] = lt[0], b.tb[g] = lt[1];
                    if constexpr (PAIRED) {
                        const u32x4* lt2 = reinterpret_cast<const u32x4*>(a.job[1].zero) + 2 * (size_t)row;
                        b.ta2[g] = lt2[0], b.tb2[g] = lt2[1];
                    }
                }
            }
        }
    };

    // STREAM (long dense launches, G > 1): the same blocks through buffer loads.  The G rows of a batch lie a constant number of bytes apart, so
    // ONE lane offset serves all of them (the row stride rides in the instruction's scalar offset), rows past the matrix and columns past the row
    // fall outside the buffer and read as zero (no lane branches, no zero fill), and the zero / step words come the same way.  The launcher
    // sets stream_ok when every offset fits 31 bits and a group never straddles two rows.
    constexpr bool STREAM = !LAT && !SPARSE && !LUT;
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rs_w, rs_w2, rs_st, rs_ze, rs_st2, rs_ze2;
    [[maybe_unused]] uint32_t wbytes = 0, gbytes = 0, gstride_w = 0, gstride_g = 0;
    if constexpr (STREAM) {
        wbytes = (uint32_t)jM * (uint32_t)nBlk * 16u, gbytes = ((uint32_t)jM * (uint32_t)nBlk >> gshift) * 2u;
        gstride_w = (uint32_t)RPS * (uint32_t)nBlk * 16u, gstride_g = ((uint32_t)RPS * (uint32_t)nBlk >> gshift) * 2u;
        rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(jw), 0, (int)wbytes, 0x00020000);
        if constexpr (PAIRED) rs_w2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(jw2), 0, (int)wbytes, 0x00020000);
        if constexpr (BD::HAS_GAMA) {
            rs_st = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(jstep), 0, (int)gbytes, 0x00020000);
            rs_ze = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(jzero), 0, (int)gbytes, 0x00020000);
            if constexpr (PAIRED) {
                rs_st2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.job[1].step), 0, (int)gbytes, 0x00020000);
                rs_ze2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.job[1].zero), 0, (int)gbytes, 0x00020000);
            }
        }
    }
    auto sload = [&](int bi, int it, BatchT& b) {
        if constexpr (STREAM) {
            const int col = it * LPR + ll;
            const uint32_t row0 = (uint32_t)((int)(s_begin - jslot0) + bi * G) * (uint32_t)RPS + (uint32_t)sub;
            const uint32_t bidx = row0 * (uint32_t)nBlk + (uint32_t)col;
            const bool col_ok = col < nBlk;
            const uint32_t vo = col_ok ? bidx * 16u : wbytes, go = col_ok ? (bidx >> gshift) * 2u : gbytes;
#pragma unroll
            for (int g = 0; g < G; g++) {
                b.w[g] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo, g * gstride_w, 2 /* nt */));
                if constexpr (PAIRED) b.w2[g] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w2, vo, g * gstride_w, 2));
                if constexpr (BD::HAS_GAMA) {
                    b.st[g] = __builtin_amdgcn_raw_buffer_load_b16(rs_st, go, g * gstride_g, 0), b.ze[g] = __builtin_amdgcn_raw_buffer_load_b16(rs_ze, go, g * gstride_g, 0);
                    if constexpr (PAIRED)
                        b.st2[g] = __builtin_amdgcn_raw_buffer_load_b16(rs_st2, go, g * gstride_g, 0), b.ze2[g] = __builtin_amdgcn_raw_buffer_load_b16(rs_ze2, go, g * gstride_g, 0);
                }
            }
        }
    };
    const bool stream = STREAM && a.stream_ok;

    // x (and the norm weight) of vectors up to 4096 elements: <= 2 chunks of 8 per thread, requested before the weights
    const int nch = a.K >> 3;
    const bool xreg = LAT && nch <= 512, has_norm = a.norm_w != nullptr;
    const bool h0 = tid < nch, h1 = tid + 256 < nch;
    u32x4 r0 = u32x4{0, 0, 0, 0}, r1 = r0, n0 = r0, n1 = r0;
    if (xreg) {
        const size_t c0 = h0 ? tid : 0, c1 = h1 ? tid + 256 : 0;
        r0 = *reinterpret_cast<const u32x4*>(a.x + c0 * 8), r1 = *reinterpret_cast<const u32x4*>(a.x + c1 * 8);
        if (has_norm) n0 = *reinterpret_cast<const u32x4*>(a.norm_w + c0 * 8), n1 = *reinterpret_cast<const u32x4*>(a.norm_w + c1 * 8);
    }

    BatchT cur, nxt;
    [[maybe_unused]] BatchT ring[XF2 ? RD : 1];
    if constexpr (XF2) {
#pragma unroll
        for (int d = 0; d < RD; d++) load(0, d < iters ? d : iters - 1, ring[d]);
    } else if (stream) {
        if (nsteps > 0) sload(0, 0, cur);
    } else if (LAT || nsteps > 0) {
        load(0, 0, cur); /* LAT: waves without work re-read row 0 */
    }
    const int pos = a.d_pos ? *a.d_pos : a.pos;

    // ---- prologue: stage x into LDS as packed bf16 chunks (XF: the same elements widened to fp32, two chunks of four)
    {
        constexpr int XCH = BD::XCH;
        auto put = [&](int c, int j, u32x4 o) {
            if constexpr (XF) {
                xs[(2 * j) * wcols + c] = widen_bf16x4(o.x, o.y);
                xs[(2 * j + 1) * wcols + c] = widen_bf16x4(o.z, o.w);
            } else {
                xs[j * nBlk + c] = o;
            }
        };
        if (xreg) {
            // RMSNorm prologue, one pass (rms_norm_kernel, layernorm.cuh:800-847): fp64 sum of squares over the workgroup, then the
            // normalised chunks go to LDS; without a norm weight the chunks go to LDS as they are.
            const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            uint32_t ow[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            if (has_norm) {
                const uint32_t ww[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
                const double ss = wave_sum_f64_fast(sumsq_2chunks(r0, r1, h0, h1));
                if (lane == 0) red[wave_in_blk] = ss;
                __syncthreads();
                const double tot = (red[0] + red[1]) + (red[2] + red[3]);
                const float mul = rms_scale((float)tot, a.inv_dim, a.eps);
#pragma unroll
                for (int k = 0; k < 8; k++) ow[k] = rms_pair(rw[k], ww[k], mul);
            }
            if (h0) {
                const int c = tid / XCH, j = tid - c * XCH;
                put(c, j, u32x4{ow[0], ow[1], ow[2], ow[3]});
            }
            if (h1) {
                const int e8 = tid + 256, c = e8 / XCH, j = e8 - c * XCH;
                put(c, j, u32x4{ow[4], ow[5], ow[6], ow[7]});
            }
        } else {
            float mul = 1.0f;
            if (a.norm_w) { /* large K: two passes */
                mul = rms_scale((float)block_sumsq_bf16(a.x, a.K, red), a.inv_dim, a.eps);
            }
            // element e of block column c, chunk j (e = c*EPB + j*8 + i)  ->  LDS chunk (j*nBlk + c)
            const int nch_w = XF2 ? wcol0 * XCH : nch; /* XF2: the first window (the launcher takes this form only without a norm) */
            for (int e8 = tid; e8 < nch_w; e8 += blockDim.x) {
                const int c = e8 / XCH, j = e8 - c * XCH;
                const u32x4 raw = *reinterpret_cast<const u32x4*>(a.x + (size_t)e8 * 8);
                u32x4 o = raw;
                if (a.norm_w) {
                    const u32x4 nw = *reinterpret_cast<const u32x4*>(a.norm_w + (size_t)e8 * 8);
                    const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, ww[4] = {nw.x, nw.y, nw.z, nw.w};
                    uint32_t ow[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) ow[k] = rms_pair(rw[k], ww[k], mul);
                    o.x = ow[0], o.y = ow[1], o.z = ow[2], o.w = ow[3];
                }
                put(c, j, o);
            }
        }
        __syncthreads();
    }

    // ---- main: pipelined over (batch, iteration) steps
    float best_v = FIRST_MAX_NONE_V;
    int best_i = FIRST_MAX_NONE_I;
    using Acc = typename BD::Acc;
    Acc acc[G], acc2[PAIRED ? G : 1]; /* per-lane chains (canonical: an even and an odd one; four such pairs for 1-bit blocks) */
    float sum[G], sum2[PAIRED ? G : 1];
    int bi = 0, it = 0;       // the step being computed
    int nbi = 0, nit = 0;     // the step being loaded
    auto compute = [&](const BatchT& bt) {
        if (it == 0) {
#pragma unroll
            for (int g = 0; g < G; g++) {
                acc[g] = Acc{};
                if (PAIRED) acc2[g] = Acc{};
            }
        }
        {
            int col = it * LPR + ll;
            const bool col_ok = col < nBlk;
            if (!col_ok) col = nBlk - 1; /* keep the LDS reads in range */
#pragma unroll
            for (int g = 0; g < G; g++) {
                int row;
                const bool ok = !LAT || (slot(s_begin + (long)bi * G + g, row) && col_ok); /* masked loads carry zero weights */
                if constexpr (LUT) {
                    const Acc r = BD::run_lut(bt.w[g], xs, col, nBlk, bt.ta[g], bt.tb[LUT16 ? g : 0], acc[g]);
                    acc[g] = acc_pick(ok, r, acc[g]);
                    if constexpr (PAIRED) {
                        const Acc r2 = BD::run_lut(bt.w2[g], xs, col, nBlk, bt.ta2[g], bt.tb2[LUT16 ? g : 0], acc2[g]);
                        acc2[g] = acc_pick(ok, r2, acc2[g]);
                    }
                } else {
                    const float st = bf2f(bt.st[g]);
                    Acc r;
                    if constexpr (XF2) r = BlockDotF<FMT>::run(bt.w[g], reinterpret_cast<const f32x4*>(xs), it >= it_half ? col - wcol0 : col, wcols, st, bf2f(bt.ze[g]), -(jqb * st), acc[g]);
                    else if constexpr (XF) r = BlockDotF<FMT>::run(bt.w[g], reinterpret_cast<const f32x4*>(xs), col, nBlk, st, bf2f(bt.ze[g]), -(jqb * st), acc[g]);
                    else r = BD::run(bt.w[g], xs, col, nBlk, st, bf2f(bt.ze[g]), -(jqb * st), acc[g]);
                    acc[g] = acc_pick(ok, r, acc[g]);
                    if (PAIRED) {
                        const float st2 = bf2f(bt.st2[g]);
                        Acc r2;
                        if constexpr (XF) r2 = BlockDotF<FMT>::run(bt.w2[g], reinterpret_cast<const f32x4*>(xs), col, nBlk, st2, bf2f(bt.ze2[g]), -(jqb2 * st2), acc2[g]);
                        else r2 = BD::run(bt.w2[g], xs, col, nBlk, st2, bf2f(bt.ze2[g]), -(jqb2 * st2), acc2[g]);
                        acc2[g] = acc_pick(ok, r2, acc2[g]);
                    }
                }
            }
        }
        if (it == iters - 1) {
#pragma unroll
            for (int g = 0; g < G; g++) {
                sum[g] = group_sum(acc_join(acc[g]), a.lpr_log2);
                if (PAIRED) sum2[g] = group_sum(acc_join(acc2[g]), a.lpr_log2);
            }
            if (ll == 0) {
#pragma unroll
                for (int g = 0; g < G; g++) {
                    int r;
                    if (!slot(s_begin + (long)bi * G + g, r)) continue;
                    if constexpr (SPARSE) r = a.row_map[r];
                    uint16_t* y = jy + (size_t)pos * jystride;
                    float v = sum[g];
                    if (PAIRED) {
                        y[r] = swiglu_bf16(round_bf16(v), round_bf16(sum2[g])); /* of the two bf16-rounded projections */
                        continue;
                    }
                    if (a.tp) { /* tensor-parallel push: one 8-byte {value | tag} granule into this rank's slot of every rank's receive area (kf_tp.hip) */
                        const TpPushDev& t = *a.tp;
                        const unsigned long long gr = ((unsigned long long)(*t.step * t.per_step + t.index + 1u) << 32) | __float_as_uint(v);
                        for (int p = 0; p < t.world; p++) __hip_atomic_store(t.peer[p] + r, gr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        continue;
                    }
                    if (a.yf) { /* un-rounded fp32 row dots: tensor-parallel partial sums (column-split o_proj / down_proj) */
                        a.yf[r] = v;
                        continue;
                    }
                    /* linear_out_bf16 (kf_device.h), written out: through the helper the compiler forms y's address once in front of the branches */
                    if (a.alpha != 1.0f) v = a.alpha * v;
                    if (a.beta != 0.0f) v = v + a.beta * bf2f(y[r]);
                    if (a.bias) v = v + bf2f(a.bias[r]);
                    uint16_t o = f2bf(v);
                    if (a.residual) o = add_bf16(a.residual[r], o);
                    y[r] = o;
                    if (MODE == GEMV_ARGMAX) {
                        first_max(best_v, best_i, bf2f(o), r);
                    }
                }
            }
        }
        if (++it == iters) it = 0, bi++;
    };
    if (stream) { /* two batches ping-pong: no register copies between steps */
        for (int k = 0; k < nsteps; k += 2) {
            if (k + 1 < nsteps) {
                if (++nit == iters) nit = 0, nbi++;
                sload(nbi, nit, nxt);
            }
            compute(cur);
            if (k + 1 >= nsteps) break;
            if (k + 2 < nsteps) {
                if (++nit == iters) nit = 0, nbi++;
                sload(nbi, nit, cur);
            }
            compute(nxt);
        }
    } else if constexpr (XF2) { /* one row slot per wave (nsteps = iters, or 0 for a wave past the last slot: it still meets the two barriers) */
        auto run = [&](int k0, int k1) { /* k0: a multiple of RD */
            for (int k = k0; k < k1; k += RD) {
#pragma unroll
                for (int d = 0; d < RD; d++) {
                    if (k + d < k1) compute(ring[d]);
                    load(0, k + d + RD < iters ? k + d + RD : iters - 1, ring[d]); /* unconditional (a request behind a branch turns the waits into drains); past the row: its last step again */
                }
            }
        };
        run(0, nsteps < it_half ? nsteps : it_half);
        __syncthreads(); /* every wave has read the first window for the last time */
        {
            constexpr int XCH = BD::XCH;
            for (int e8 = wcol0 * XCH + tid; e8 < nch; e8 += blockDim.x) {
                const int c = e8 / XCH - wcol0, j = e8 % XCH;
                const u32x4 o = *reinterpret_cast<const u32x4*>(a.x + (size_t)e8 * 8);
                xs[(2 * j) * wcols + c] = widen_bf16x4(o.x, o.y);
                xs[(2 * j + 1) * wcols + c] = widen_bf16x4(o.z, o.w);
            }
        }
        __syncthreads();
        run(it_half, nsteps);
    } else {
        for (int k = 0; k < nsteps; k++) {
            if (k + 1 < nsteps) {
                if (++nit == iters) nit = 0, nbi++;
                load(nbi, nit, nxt);
            }
            compute(cur);
            cur = nxt;
        }
    }

    if (MODE == GEMV_ARGMAX) {
        // the first maximum over this workgroup's rows (first_max, kf_device.h)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) { /* wave_first_max spelled out: through the helper the compiler schedules this kernel differently ("rules stated once") */
            const float ov = __shfl_xor(best_v, m, 64);
            const int oi = __shfl_xor(best_i, m, 64);
            first_max(best_v, best_i, ov, oi);
        }
        float* rv = reinterpret_cast<float*>(red);
        int* ri = reinterpret_cast<int*>(rv + 16);
        __syncthreads();
        if (lane == 0) rv[wave_in_blk] = best_v, ri[wave_in_blk] = best_i;
        __syncthreads();
        if (tid == 0) { /* waves_first_max spelled out, for the same reason */
            for (int w = 1; w < (int)(blockDim.x >> 6); w++) first_max(best_v, best_i, rv + w, ri + w);
            a.amax_val[blockIdx.x] = best_v;
            a.amax_idx[blockIdx.x] = best_i;
        }
    }
}

// ---- the instantiations a plan can name, as one table per summation order: every storage form x G 1 / 2 / 4 x the launch forms (plain with one or more matrices, paired,
// arg-max, the sparse plain and paired forms); XF for the canonical 4-bit forms, XF2 for their plain one-matrix G = 1 launches
constexpr bool gemv_form_exists(bool canon, int fmt, int G, int mode, bool sparse, bool onejob, bool xf, bool xf2) {
    if (sparse && mode == GEMV_ARGMAX) return false;
    if (fmt_rowq(fmt) && (sparse || mode == GEMV_ARGMAX || xf)) return false; /* the 3- / 2-bit row forms: plain (1-3 matrices) and paired launches only */
    if (mode == GEMV_PAIRED ? onejob : (!onejob && (mode == GEMV_ARGMAX || sparse))) return false; /* paired: job 1 by name; arg-max and sparse: one matrix */
    if (xf && !(canon && (fmt == FMT_Q4 || fmt == FMT_Q4P))) return false;
    return !xf2 || (xf && mode == GEMV_PLAIN && !sparse && onejob && G == 1);
}
// the table index: one digit per template parameter, its stride named below -- fmt (12 FMT_*) x G (1 / 2 / 4 as 0 / 1 / 2) x mode (3) x sparse x onejob x xf x xf2;
// gemv_form_index composes an index from a plan, gemv_form's defaults take one apart with the same strides
constexpr int GF_XF2 = 1, GF_XF = 2, GF_ONEJOB = 4, GF_SPARSE = 8, GF_MODE = 16, GF_G = 3 * GF_MODE, GF_FMT = 3 * GF_G, GEMV_FORMS = 12 * GF_FMT;
constexpr int gemv_form_index(int fmt, int G, int mode, bool sparse, bool onejob, bool xf, bool xf2) {
    return fmt * GF_FMT + (G >> 1) * GF_G + mode * GF_MODE + sparse * GF_SPARSE + onejob * GF_ONEJOB + xf * GF_XF + xf2 * GF_XF2;
}
using GemvKernel = void (*)(GemvArgs);
template <bool CANON, int I, int FMT = I / GF_FMT, int G = 1 << (I / GF_G % 3), int MODE = I / GF_MODE % 3, bool SPARSE = I / GF_SPARSE % 2, bool ONEJOB = I / GF_ONEJOB % 2,
          bool XF = I / GF_XF % 2, bool XF2 = I / GF_XF2 % 2>
constexpr GemvKernel gemv_form() {
    static_assert(gemv_form_index(FMT, G, MODE, SPARSE, ONEJOB, XF, XF2) == I, "gemv_form_index");
    if constexpr (gemv_form_exists(CANON, FMT, G, MODE, SPARSE, ONEJOB, XF, XF2)) return gemv_kernel<FMT, G, MODE, SPARSE, ONEJOB, CANON, XF, XF2>;
    else return nullptr;
}
template <bool CANON, int... I>
constexpr std::array<GemvKernel, GEMV_FORMS> gemv_forms(std::integer_sequence<int, I...>) {
    return {{gemv_form<CANON, I>()...}};
}
template <bool CANON>
int gemv_dispatch(const GemvPlan& p, const GemvArgs& a, hipStream_t st) {
    static constexpr std::array<GemvKernel, GEMV_FORMS> forms = gemv_forms<CANON>(std::make_integer_sequence<int, GEMV_FORMS>());
    const GemvKernel k = forms[gemv_form_index(p.fmt, p.G, p.mode, p.sparse, p.onejob, p.xf, p.xf2)];
    if (!k) return KF_INTERNAL_ERR; /* a form gemv_plan never names */
    void* args[] = {const_cast<GemvArgs*>(&a)};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(k), dim3(p.grid), dim3(256), args, (size_t)p.lds, st);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
