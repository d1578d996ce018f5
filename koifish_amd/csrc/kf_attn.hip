// kf_attn.hip -- decode attention for one new token (GQA, full causal length), gfx950 / wave64.
//
// Replaces the reference's three launches attention_qk_kernel / CU_softmax_multihead / attention_v_kernel
// (QKV.cu:669-673; operator.cuh:572-632, 251-277, 649-668 -- one thread per key capped at 1024 keys, one
// THREAD per head for the softmax) by ONE launch: grid = slices x kv-heads; every workgroup streams its slice
// of K and V once (16-byte loads issued before anything else), keeps a softmax for the query heads of its GQA
// group against a workgroup-wide running maximum, and publishes {acc[hd], m, l}; the workgroup that arrives
// last for a kv-head merges the slices and writes the bf16 output (no separate merge launch).
// The q/k RMSNorm + RoPE of ROPE::cuInfer (rope.cu:645-672 -> CU_rms_forward_v2 layernorm.cuh:129-167,
// CU_rope2_v0 operator.cuh:734-772) is folded into the prologue; the workgroup whose slice holds the new
// position writes the normed+roped key into the cache row.  HBM-bound: bytes = 2 * (pos+1) * kv_dim * 2.
//
// Arithmetic (= oracle/kf_oracle.c kfo_attn_decode mode CANON, bit for bit; kf_attn_common.h states it): score = bf16(dot * (1 / sqrtf(hd))) -- the same
// bf16 store the reference makes (qk_v is floatX) -- with the dot as per-lane chains of v_fma_f32 + a tree; softmax weights as f * 2^(n - m) from a fixed
// polynomial with exact power-of-two rescales between lanes, waves and slices; fp64 sums; one bf16 store of out = (float)(O / L).
//
// Cross-workgroup hand-off (MI355X_MICROARCH.md "Valid forms", table row 1): partials are written with
// agent-scope relaxed atomic stores (write-through `sc1`), every storing wave drains vmcnt, the workgroup
// barriers, ONE lane adds to the kv-head's arrival counter (agent-scope atomic); the workgroup whose add returned
// nsp-1 reads every partial with agent-scope relaxed atomic loads (`sc1`) after a barrier, and re-zeroes the counter.
#include <stdlib.h>

#include <array>
#include <utility>

#include "kf_attn_common.h"
#include "kf_attn_plan.h"

namespace kf {

// ROWS (kf_attn_decode_rows: the verify pass of speculative decoding, R consecutive queries of one sequence on grid z): query z sits at position a.pos + z and
// attends to keys 0 .. a.pos + z.  Every z cuts its keys by attn_slices at its OWN position -- the slices kf_attn_decode would take there; the grid's x is the last
// row's count, workgroups past a row's own count leave at once -- and owns its arrival counters and partials: row z's scratch lies z * attn_decode_scratch_bytes
// behind row 0's.  The waves per workgroup are the launch's (the last row's): the canonical order does not depend on them.
template <int GQ, int NW, int HD, bool ROWS = false>
__global__ void __launch_bounds__(NW * 64) attn_kernel(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Slice = AttnSlice<GQ, NW, HD, 8>; /* the shell (kf_attn_common.h): 8 dims of a key per lane */
    constexpr int hd = HD, LPK = Slice::LPK, KPW = Slice::KPW, lpk_log2 = Slice::lpk_log2, tstride = Slice::tstride, NQ = Slice::NQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int PS = hd + 2; /* {O[hd], L, m} as doubles */
    constexpr AttnCanonLds lds(GQ, NW, HD);
    static_assert(lds.fits(), "LDS");
    double* comb = reinterpret_cast<double*>(smem_raw + lds.comb);
    uint16_t* qb = reinterpret_cast<uint16_t*>(smem_raw + lds.qb);
    uint16_t* knew = reinterpret_cast<uint16_t*>(smem_raw + lds.knew);
    int* flag = reinterpret_cast<int*>(smem_raw + lds.flag);

    // token batch (prefill): blockIdx.z = token, one slice per kv-head, position pos0 + token, q / out rows q_stride apart
    const int pos_l = a.pos + (int)blockIdx.z;
    int nsp = a.n_splits, chunk = a.chunk;
    if constexpr (ROWS) {
        const AttnSlices s = attn_slices(pos_l, a.n_kv, GQ * a.gq_split);
        nsp = s.n_splits, chunk = s.chunk;
        if ((int)blockIdx.x >= nsp) return; /* workgroup-uniform */
    }
    const Slice sl(a.gq_split, chunk);
    const uint16_t* const qsrc = a.q + (size_t)blockIdx.z * a.q_stride;
    uint16_t* const odst = a.out + (size_t)blockIdx.z * a.q_stride;
    const int h0 = sl.h0(), grp = lane >> lpk_log2, d0 = (lane & (LPK - 1)) * 8, tstart = sl.tstart(wave, grp);
    const bool has_new = a.k_raw != nullptr;

    // ---- issue the first K/V tiles before anything else: they depend neither on the position (read from device memory in
    // graph replay) nor on the previous kernel's q.  Rows up to the launch bound exist in the cache; rows past the real position
    // are masked later, and the row AT the position is replaced by the freshly normed+roped key.
    u32x4 kk[ATTN_U], vv[ATTN_U];
    auto issue = [&](int tb, int tend) {
#pragma unroll
        for (int u = 0; u < ATTN_U; u++) {
            const int t = tb + u * tstride;
            kk[u] = u32x4{0, 0, 0, 0}, vv[u] = u32x4{0, 0, 0, 0};
            if (t < tend) {
                const size_t off = (size_t)t * a.kv_stride + (size_t)sl.kvh * hd + d0;
                kk[u] = *reinterpret_cast<const u32x4*>(a.kcache + off);
                vv[u] = *reinterpret_cast<const u32x4*>(a.vcache + off);
            }
        }
    };
    issue(tstart, sl.end(pos_l)); /* a.pos is the launch bound here */
    // ... and the q heads (+ the raw new key) this wave will prepare: they do not depend on the position either
    const bool qnorm = a.rope_table && a.wq_norm;
    HeadRaw qraw[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const int hq = wave + i * NW;
        qraw[i] = load_head(qsrc + (size_t)(h0 + (hq < GQ ? hq : 0)) * hd, qnorm ? a.wq_norm : nullptr, hd);
    }
    const HeadRaw kraw = load_head(has_new ? a.k_raw + (size_t)sl.kvh * hd : qsrc, a.wk_norm, hd);

    const auto [pos, t1, empty] = sl.at(a.d_pos, pos_l);
    const size_t row_scratch = ROWS ? (size_t)blockIdx.z * attn_decode_scratch_bytes(a.n_head, HD) : 0; /* bytes from row 0's counters / partials to this row's */
    double* const part = reinterpret_cast<double*>(a.part) + row_scratch / sizeof(double); /* [n_head][n_splits][PS] doubles */

    if (!empty) {
        // ---- prologue: q heads of this group, and the new key when it lies in this slice
        const float* tab_pos = a.rope_table ? a.rope_table + (size_t)pos * hd : nullptr;
#pragma unroll
        for (int i = 0; i < NQ; i++)
            if (wave + i * NW < GQ) prep_head(qraw[i], qnorm, tab_pos, hd, a.eps, qb + (wave + i * NW) * hd);
        const bool own_new = has_new && sl.holds(pos, t1);
        if (own_new && wave == (GQ % NW)) prep_head(kraw, a.wk_norm != nullptr, tab_pos, hd, a.eps, knew);
        __syncthreads();
        if (own_new && sl.gpart == 0) { /* every part of the kv-head holds the same row: one writes it */
            uint16_t* krow = a.kcache + (size_t)pos * a.kv_stride + (size_t)sl.kvh * hd;
            for (int i = tid; i < hd; i += blockDim.x) krow[i] = knew[i];
        }
        float qf[GQ][8]; /* this lane's 8 dims of every q head */
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const u32x4 qv = *reinterpret_cast<const u32x4*>(qb + hq * hd + d0);
            const uint32_t q4[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int i = 0; i < 4; i++) qf[hq][2 * i] = bf_lo(q4[i]), qf[hq][2 * i + 1] = bf_hi(q4[i]);
        }
        CanonAcc<GQ> A;
        A.init();
        const float rden = 1.0f / a.inv_sqrt_hd_den; /* score /= sqrtf(head_dim) (operator.cuh:630), as a multiply by the rounded reciprocal */
        for (int tb = tstart; tb - grp - wave * KPW < t1; tb += ATTN_U * tstride) { /* workgroup-uniform trip count */
            u32x4 ck[ATTN_U], cv[ATTN_U];
            bool valid[ATTN_U];
#pragma unroll
            for (int u = 0; u < ATTN_U; u++) {
                const int t = tb + u * tstride;
                ck[u] = kk[u], cv[u] = vv[u], valid[u] = t < t1;
                if (has_new && valid[u] && t == pos) ck[u] = *reinterpret_cast<const u32x4*>(knew + d0);
            }
            if (tb - grp - wave * KPW + ATTN_U * tstride < t1) issue(tb + ATTN_U * tstride, t1);
            canon_batch<GQ, LPK>(A, qf, ck, cv, valid, lpk_log2, rden);
        }
        // ---- the wave's key groups summed (reduce-scatter by row swaps), the waves through LDS: exact rescales to the slice's maximum exponent
        canon_wave_to_lds<GQ, LPK>(A, comb + (size_t)wave * GQ * PS, hd, lane, d0);
        __syncthreads();
        canon_slice_publish<GQ, NW, HD>(comb, part, odst, h0, nsp, sl.split);
    } else if (nsp > 1) { /* empty slice: neutral partial, but it still arrives */
        canon_slice_publish_empty<GQ, HD>(part, h0, nsp, sl.split);
    }
    if (nsp == 1) return;
    // ---- arrival; the last workgroup of this kv-head merges (kf_attn_common.h)
    canon_arrive_and_merge<GQ, NW, HD>(part, a.counters + row_scratch / sizeof(int) + (int)blockIdx.y * a.cnt_stride, flag, odst, h0, nsp); /* per (kv-head, part): its slices' workgroups meet here */
}

// ---- the fp32 form of rounds 1-2 (kf_set_canonical(ctx, 0), the default): scores by v_dot2c_f32_bf16, exp by v_exp_f32(x * log2 e), a workgroup-wide running
// maximum, fp32 sums, slices merged with fp32 exponentials.  <= 1 bf16 ulp / 2^-10 of the scale from the oracle's FUSED mode; about half the vector work of the
// canonical form above (no fp64).  Partials: [n_head][n_splits][hd + 4] floats in the same scratch.
template <int GQ, int NW, int HD>
__global__ void __launch_bounds__(NW * 64) attn_fast_kernel(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Slice = AttnSlice<GQ, NW, HD, 8>;
    constexpr int hd = HD, hd_log2 = Slice::hd_log2, LPK = Slice::LPK, KPW = Slice::KPW, lpk_log2 = Slice::lpk_log2, tstride = Slice::tstride, NQ = Slice::NQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int PS = hd + 4; /* {acc[hd], m, l, pad, pad} */
    constexpr AttnFastLds lds(GQ, NW, HD);
    static_assert(lds.fits(), "LDS");
    uint16_t* qb = reinterpret_cast<uint16_t*>(smem_raw + lds.qb);
    uint16_t* knew = reinterpret_cast<uint16_t*>(smem_raw + lds.knew);
    float* wmax = reinterpret_cast<float*>(smem_raw + lds.wmax);
    int* flag = reinterpret_cast<int*>(smem_raw + lds.flag);
    float* comb = reinterpret_cast<float*>(smem_raw + lds.comb);

    // the shell, as in attn_kernel
    const Slice sl(a.gq_split, a.chunk);
    const int pos_l = a.pos + (int)blockIdx.z, nsp = a.n_splits;
    const uint16_t* const qsrc = a.q + (size_t)blockIdx.z * a.q_stride;
    uint16_t* const odst = a.out + (size_t)blockIdx.z * a.q_stride;
    const int h0 = sl.h0(), grp = lane >> lpk_log2, d0 = (lane & (LPK - 1)) * 8, tstart = sl.tstart(wave, grp);
    const bool has_new = a.k_raw != nullptr;

    u32x4 kk[ATTN_U], vv[ATTN_U];
    auto issue = [&](int tb, int tend) {
#pragma unroll
        for (int u = 0; u < ATTN_U; u++) {
            const int t = tb + u * tstride;
            kk[u] = u32x4{0, 0, 0, 0}, vv[u] = u32x4{0, 0, 0, 0};
            if (t < tend) {
                const size_t off = (size_t)t * a.kv_stride + (size_t)sl.kvh * hd + d0;
                kk[u] = *reinterpret_cast<const u32x4*>(a.kcache + off);
                vv[u] = *reinterpret_cast<const u32x4*>(a.vcache + off);
            }
        }
    };
    issue(tstart, sl.end(pos_l));
    const bool qnorm = a.rope_table && a.wq_norm;
    HeadRaw qraw[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const int hq = wave + i * NW;
        qraw[i] = load_head(qsrc + (size_t)(h0 + (hq < GQ ? hq : 0)) * hd, qnorm ? a.wq_norm : nullptr, hd);
    }
    const HeadRaw kraw = load_head(has_new ? a.k_raw + (size_t)sl.kvh * hd : qsrc, a.wk_norm, hd);

    const auto [pos, t1, empty] = sl.at(a.d_pos, pos_l);

    if (!empty) {
        const float* tab_pos = a.rope_table ? a.rope_table + (size_t)pos * hd : nullptr;
#pragma unroll
        for (int i = 0; i < NQ; i++)
            if (wave + i * NW < GQ) prep_head(qraw[i], qnorm, tab_pos, hd, a.eps, qb + (wave + i * NW) * hd);
        const bool own_new = has_new && sl.holds(pos, t1);
        if (own_new && wave == (GQ % NW)) prep_head(kraw, a.wk_norm != nullptr, tab_pos, hd, a.eps, knew);
        __syncthreads();
        if (own_new && sl.gpart == 0) { /* every part of the kv-head holds the same row: one writes it */
            uint16_t* krow = a.kcache + (size_t)pos * a.kv_stride + (size_t)sl.kvh * hd;
            for (int i = tid; i < hd; i += blockDim.x) krow[i] = knew[i];
        }
        u32x4 qreg[GQ]; /* this lane's 8 dims of every q head, packed bf16 */
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) qreg[hq] = *reinterpret_cast<const u32x4*>(qb + hq * hd + d0);

        float M[GQ], l[GQ], acc[GQ][8];
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            M[hq] = -__builtin_inff(), l[hq] = 0.f;
#pragma unroll
            for (int i = 0; i < 8; i++) acc[hq][i] = 0.f;
        }
        const float rden = 1.0f / a.inv_sqrt_hd_den; /* score /= sqrtf(head_dim) (operator.cuh:630), as a multiply by the rounded reciprocal */
        for (int tb = tstart; tb - grp - wave * KPW < t1; tb += ATTN_U * tstride) { /* workgroup-uniform trip count */
            u32x4 ck[ATTN_U], cv[ATTN_U];
#pragma unroll
            for (int u = 0; u < ATTN_U; u++) ck[u] = kk[u], cv[u] = vv[u];
            if (tb - grp - wave * KPW + ATTN_U * tstride < t1) issue(tb + ATTN_U * tstride, t1);
            // scores of this batch
            float s[ATTN_U][GQ], bm[GQ];
#pragma unroll
            for (int hq = 0; hq < GQ; hq++) bm[hq] = -__builtin_inff();
#pragma unroll
            for (int u = 0; u < ATTN_U; u++) {
                const int t = tb + u * tstride;
                const bool valid = t < t1;
                u32x4 kw = ck[u];
                if (has_new && valid && t == pos) kw = *reinterpret_cast<const u32x4*>(knew + d0);
#pragma unroll
                for (int hq = 0; hq < GQ; hq++) {
                    float d = dot2_bf16(qreg[hq].x, kw.x, 0.f);
                    d = dot2_bf16(qreg[hq].y, kw.y, d);
                    d = dot2_bf16(qreg[hq].z, kw.z, d);
                    d = dot2_bf16(qreg[hq].w, kw.w, d);
                    d = group_sum16(d, lpk_log2);
                    d = round_bf16(d * rden);
                    s[u][hq] = valid ? d : -__builtin_inff();
                    bm[hq] = fmaxf(bm[hq], s[u][hq]);
                }
            }
            // workgroup-wide maximum of the batch -> one running maximum shared by every lane
#pragma unroll
            for (int hq = 0; hq < GQ; hq++) {
                bm[hq] = xmax32(xmax16(bm[hq]));
                if (LPK < 16) bm[hq] = fmaxf(bm[hq], dpp_f<0x128>(bm[hq]));
            }
            __syncthreads(); /* previous batch's readers of wmax are done */
            if (lane == 0) {
#pragma unroll
                for (int hq = 0; hq < GQ; hq++) wmax[wave * GQ + hq] = bm[hq];
            }
            __syncthreads();
#pragma unroll
            for (int hq = 0; hq < GQ; hq++) {
                float Mb = wmax[hq];
#pragma unroll
                for (int w2 = 1; w2 < NW; w2++) Mb = fmaxf(Mb, wmax[w2 * GQ + hq]);
                if (Mb > M[hq]) {
                    const float sc = fast_exp(M[hq] - Mb);
                    l[hq] *= sc;
#pragma unroll
                    for (int i = 0; i < 8; i++) acc[hq][i] *= sc;
                    M[hq] = Mb;
                }
            }
#pragma unroll
            for (int u = 0; u < ATTN_U; u++) {
                float vf_[8];
                const uint32_t vw[4] = {cv[u].x, cv[u].y, cv[u].z, cv[u].w};
#pragma unroll
                for (int i = 0; i < 4; i++) vf_[2 * i] = bf_lo(vw[i]), vf_[2 * i + 1] = bf_hi(vw[i]);
#pragma unroll
                for (int hq = 0; hq < GQ; hq++) {
                    const float p = fast_exp(s[u][hq] - M[hq]); /* -inf (masked key) -> 0 */
                    l[hq] += p;
#pragma unroll
                    for (int i = 0; i < 8; i++) acc[hq][i] = fmaf(p, vf_[i], acc[hq][i]);
                }
            }
        }

        // ---- sum the key groups (same reference maximum everywhere: plain sums).  Inside the wave a reduce-scatter by row swaps:
        // swapping the halves of (acc[i], acc[i+4]) and adding leaves dims i in lanes 0-31 and i+4 in lanes 32-63, the same on 16-lane
        // rows leaves row R with the totals of dims 2R and 2R+1 -- 6 swaps + 6 adds per head instead of 8 butterflies
        const int row = lane >> 4;
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            float s1[4], r2[2];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[hq][i]), __float_as_uint(acc[hq][i + 4]), false, false);
                s1[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(s1[i]), __float_as_uint(s1[i + 2]), false, false);
                r2[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
                if (LPK < 16) r2[i] += dpp_f<0x128>(r2[i]); /* two key groups per row: row_ror:8 */
            }
            float lt = xsum16(xsum32(l[hq]));
            if (LPK < 16) lt += dpp_f<0x128>(lt);
            float* c = comb + ((size_t)wave * GQ + hq) * PS;
            if (LPK == 16 || (lane & 8) == 0) *reinterpret_cast<float2*>(c + d0 + 2 * row) = float2{r2[0], r2[1]};
            if (lane == 0) c[hd] = lt;
        }
        __syncthreads();
        for (int i = tid; i < GQ * hd; i += blockDim.x) {
            const int hq = i >> hd_log2, d = i & (hd - 1);
            float o = 0.f, L = 0.f;
#pragma unroll
            for (int sl = 0; sl < NW; sl++) {
                const float* c = comb + ((size_t)sl * GQ + hq) * PS;
                o += c[d];
                L += c[hd];
            }
            if (nsp == 1) {
                odst[(size_t)(h0 + hq) * hd + d] = f2bf(o * (1.0f / L));
            } else {
                float Mh = M[0];
#pragma unroll
                for (int q2 = 1; q2 < GQ; q2++) Mh = (hq == q2) ? M[q2] : Mh;
                float* dst = a.part + ((size_t)(h0 + hq) * nsp + sl.split) * PS;
                st_sc1(dst + d, o);
                if (d == 0) st_sc1(dst + hd, Mh), st_sc1(dst + hd + 1, L);
            }
        }
    } else if (nsp > 1) { /* empty slice: neutral partial, but it still arrives */
        for (int i = tid; i < GQ * hd; i += blockDim.x) {
            const int hq = i >> hd_log2, d = i & (hd - 1);
            float* dst = a.part + ((size_t)(h0 + hq) * nsp + sl.split) * PS;
            st_sc1(dst + d, 0.f);
            if (d == 0) st_sc1(dst + hd, -__builtin_inff()), st_sc1(dst + hd + 1, 0.f);
        }
    }
    if (nsp == 1) return;

    // ---- arrival; the last workgroup of this kv-head merges
    int* const counter = a.counters + (int)blockIdx.y * a.cnt_stride; /* per (kv-head, part): its slices' workgroups meet here */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag[0] = (old == nsp - 1);
    }
    __syncthreads();
    if (!flag[0]) return;

    // Every thread fetches its output element from all slices in one round of loads; the head is the same for the whole wave
    // (64 | hd), so lane sp of the wave fetches (m, l) of slice sp and the scales are made in registers: no LDS, no barrier.
    constexpr int NT = NW * 64;
    constexpr int NV = (GQ * 128 + NT - 1) / NT; /* output elements per thread (hd <= 128) */
    float v[NV][KF_ATTN_MAX_SPLITS], ms[NV], ls[NV];
#pragma unroll
    for (int e = 0; e < NV; e++) {
        const int i = tid + e * NT;
        const bool in = i < GQ * hd;
        const int hq = in ? (i >> hd_log2) : 0, d = i & (hd - 1);
        const float* p = a.part + (size_t)(h0 + hq) * nsp * PS;
        const bool mine = in && lane < nsp;
        ms[e] = mine ? ld_sc1(p + (size_t)lane * PS + hd) : -__builtin_inff();
        ls[e] = mine ? ld_sc1(p + (size_t)lane * PS + hd + 1) : 0.f;
#pragma unroll
        for (int sp = 0; sp < KF_ATTN_MAX_SPLITS; sp++) v[e][sp] = (in && sp < nsp) ? ld_sc1(p + (size_t)sp * PS + d) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < NV; e++) {
        const int i = tid + e * NT;
        const float Mx = wave_max(ms[e]);
        const float sc = (ms[e] == -__builtin_inff()) ? 0.f : fast_exp(ms[e] - Mx);
        const float L = wave_sum(ls[e] * sc);
        float o = 0.f;
#pragma unroll
        for (int sp = 0; sp < KF_ATTN_MAX_SPLITS; sp++)
            o = fmaf(v[e][sp], __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(sc), sp)), o);
        if (i < GQ * hd) odst[(size_t)(h0 + (i >> hd_log2)) * hd + (i & (hd - 1))] = f2bf(o * (1.0f / L));
    }
    if (tid == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// standalone ROPE::cuInfer: grid = n_head + n_kv, one wave each.  ROWPOS: d_pos is an array, one position per token (packed documents)
template <bool ROWPOS>
__global__ void __launch_bounds__(64) qknorm_rope_kernel(uint16_t* q, uint16_t* k, const uint16_t* wq, const uint16_t* wk, const float* table, int pos_,
                                                         const int* d_pos, int n_head, int n_kv, int hd, float eps, long long q_stride, long long k_stride, int seq_len, float* rstd_q,
                                                         float* rstd_k) {
    __shared__ uint16_t buf[256];
    /* blockIdx.y = token of a batch; seq_len > 0: sequences of seq_len tokens back to back, positions restart at pos_ in each */
    const int pos = ROWPOS ? d_pos[blockIdx.y] : (d_pos ? *d_pos : pos_) + (seq_len > 0 ? (int)blockIdx.y % seq_len : (int)blockIdx.y);
    const int b = blockIdx.x;
    uint16_t* src = b < n_head ? q + (size_t)blockIdx.y * q_stride + (size_t)b * hd : k + (size_t)blockIdx.y * k_stride + (size_t)(b - n_head) * hd;
    const uint16_t* wn = b < n_head ? wq : wk;
    float* ro = b < n_head ? (rstd_q ? rstd_q + (size_t)blockIdx.y * n_head + b : nullptr) : (rstd_k ? rstd_k + (size_t)blockIdx.y * n_kv + (b - n_head) : nullptr);
    prep_head(load_head(src, wn, hd), wn != nullptr, table ? table + (size_t)pos * hd : nullptr, hd, eps, buf, ro);
    __syncthreads();
    for (int i = threadIdx.x; i < hd; i += 64) src[i] = buf[i];
}

// the instantiations attn_plan can name, by (order, query heads per workgroup, waves, hd): 8 waves only at ATTN_NW8_GQ heads or fewer, the canonical order only with
// its ATTN_CANON_GQ_WG heads per workgroup or fewer
constexpr int AF_HD = 1, AF_NW = 2, AF_GQ = 4, AF_CANON = 16, ATTN_FORMS = 2 * AF_CANON;
constexpr int attn_form_index(bool canon, int gq, int nw, int hd) { return canon * AF_CANON + __builtin_ctz(gq) * AF_GQ + (nw == 8) * AF_NW + (hd == 128) * AF_HD; }
using AttnKernel = void (*)(AttnArgs);
template <int I, bool CANON = I / AF_CANON, int GQ = 1 << (I / AF_GQ % 4), int NW = I / AF_NW % 2 ? 8 : 4, int HD = I % 2 ? 128 : 64>
constexpr AttnKernel attn_form() {
    static_assert(attn_form_index(CANON, GQ, NW, HD) == I, "attn_form_index");
    if constexpr ((NW == 8 && GQ > ATTN_NW8_GQ) || (CANON && GQ > ATTN_CANON_GQ_WG)) return nullptr;
    else if constexpr (CANON) return attn_kernel<GQ, NW, HD>;
    else return attn_fast_kernel<GQ, NW, HD>;
}
template <int... I>
constexpr std::array<AttnKernel, ATTN_FORMS> attn_forms(std::integer_sequence<int, I...>) {
    return {{attn_form<I>()...}};
}

// the ROWS instantiations of the canonical kernel, by the same index (its canonical half)
template <int I, int GQ = 1 << (I / AF_GQ % 4), int NW = I / AF_NW % 2 ? 8 : 4, int HD = I % 2 ? 128 : 64>
constexpr AttnKernel attn_rows_form() {
    if constexpr ((NW == 8 && GQ > ATTN_NW8_GQ) || GQ > ATTN_CANON_GQ_WG) return nullptr;
    else return attn_kernel<GQ, NW, HD, true>;
}
template <int... I>
constexpr std::array<AttnKernel, AF_CANON> attn_rows_forms(std::integer_sequence<int, I...>) {
    return {{attn_rows_form<I>()...}};
}

int attn_launch(hipStream_t st, AttnArgs& a, const AttnPlan& p, bool rows) {
    static constexpr std::array<AttnKernel, ATTN_FORMS> forms = attn_forms(std::make_integer_sequence<int, ATTN_FORMS>());
    static constexpr std::array<AttnKernel, AF_CANON> rows_forms = attn_rows_forms(std::make_integer_sequence<int, AF_CANON>());
    if (p.status != KF_OK) return p.status;
    if (rows && !p.canon) return KF_INTERNAL_ERR;
    const AttnKernel k = rows ? rows_forms[attn_form_index(false, p.gq, p.nw, p.hd)] : forms[attn_form_index(p.canon, p.gq, p.nw, p.hd)];
    if (!k) return KF_INTERNAL_ERR; /* a form attn_plan never names */
    a.n_tok = p.grid[2], a.n_splits = p.n_splits, a.chunk = p.chunk, a.gq_split = p.gq_split, a.cnt_stride = p.cnt_stride;
    a.inv_sqrt_hd_den = sqrtf((float)p.hd);
    void* args[] = {&a};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(k), dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(p.threads), args, (size_t)p.lds, st);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

int qknorm_rope_launch(hipStream_t st, uint16_t* q, uint16_t* k, const uint16_t* wq, const uint16_t* wk, const float* table, int pos,
                       const int* d_pos, int n_head, int n_kv, int hd, float eps, int n_tok, long long q_stride, long long k_stride, int seq_len, float* rstd_q, float* rstd_k) {
    if (hd < 64 || hd > 128 || (hd & (hd - 1)) != 0 || n_tok < 1) return KF_INVALID_ARGS;
    hipLaunchKernelGGL(qknorm_rope_kernel<false>, dim3(n_head + (k ? n_kv : 0), n_tok), dim3(64), 0, st, q, k, wq, wk, table, pos, d_pos, n_head, n_kv, hd, eps,
                       q_stride, k_stride, seq_len, rstd_q, rstd_k);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}
// the same with row_pos [n_tok]: token t at position row_pos[t]
int qknorm_rope_pos_launch(hipStream_t st, uint16_t* q, uint16_t* k, const uint16_t* wq, const uint16_t* wk, const float* table, const int* row_pos, int n_head, int n_kv, int hd,
                           float eps, int n_tok, long long q_stride, long long k_stride, float* rstd_q, float* rstd_k) {
    if (hd < 64 || hd > 128 || (hd & (hd - 1)) != 0 || n_tok < 1 || !row_pos) return KF_INVALID_ARGS;
    hipLaunchKernelGGL(qknorm_rope_kernel<true>, dim3(n_head + (k ? n_kv : 0), n_tok), dim3(64), 0, st, q, k, wq, wk, table, 0, row_pos, n_head, n_kv, hd, eps, q_stride,
                       k_stride, 0, rstd_q, rstd_k);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
