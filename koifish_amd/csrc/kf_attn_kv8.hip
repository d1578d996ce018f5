// kf_attn_kv8.hip -- the int8 KV cache (include/kf_abi.h "int8 KV cache"): decode attention for one new token on quantised rows, and the two row kernels of the token
// batches.  gfx950 / wave64.
//
// attn_kv8_kernel is attn_kernel's (kf_attn.hip) launch on the int8 cache: grid = slices x (kv-heads x parts); every workgroup streams its slice of K8 / V8 once (16-byte
// loads = 16 elements per lane, so a key takes hd / 16 lanes and a wave step covers twice the keys of the bf16 kernel), issued before the position is known; the q/k-norm +
// RoPE prologue is load_head / prep_head; the workgroup whose slice holds the position quantises the new K and V rows, writes them with their steps and attends the
// quantised row from LDS.  The score is an exact integer dot on v_dot4c_i32_i8 (4 per lane, key and head, joined over the key's lanes by integer DPP adds) against the
// quantised query head in LDS, then three separate fp32 multiplies and the bf16 rounding; weights and sums are the canonical order's (CanonAcc, canon_shift, fp64), with
// the value step folded into the weight by one fp32 multiply BEFORE the power-of-two scaling.  Slices, publish, arrival counter and the last workgroup's merge are
// attn_kernel's, on the same scratch (hand-off: MI355X "valid forms" row 1 -- agent-scope relaxed atomic stores, every storing wave drains vmcnt, a barrier, ONE lane's
// agent-scope add; the workgroup whose add came last reads with agent-scope relaxed atomic loads behind a barrier and re-zeroes the counter).
// HBM bytes = (pos + 1) * (2 * kv_dim + 8 * n_kv): half the bf16 kernel's.
#include "kf_attn_common.h"
#include "kf_attn_plan.h"

namespace kf {

template <int CTRL>
__device__ __forceinline__ int dpp_int(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
// integer sum over the 2^lg (<= 8) lanes of each aligned lane group: exact, so the tree's shape is free
__device__ __forceinline__ int group_sum_i(int v, int lg) {
    if (lg >= 1) v += dpp_int<0xB1>(v);
    if (lg >= 2) v += dpp_int<0x4E>(v);
    if (lg >= 3) v += dpp_int<0x141>(v);
    return v;
}
template <int GQ>
struct Kv8Acc { /* a lane's 16 elements as two canonical accumulators of 8; l and m live in lo */
    CanonAcc<GQ> lo, hi;
};

// one batch of U key tiles of this lane's key group: k / v tiles (16 codes of this lane), the rows' steps, validity per tile; q8 as 16 codes per head with its step
template <int GQ, int LPK, int U>
__device__ __forceinline__ void kv8_batch(Kv8Acc<GQ>& A, const u32x4 (&q8)[GQ], const float (&sq)[GQ], const u32x4 (&kk)[U], const u32x4 (&vv)[U], const float (&ks)[U],
                                          const float (&vs)[U], const bool (&valid)[U], int lpk_log2, float rden) {
    float f[U][GQ], n[U][GQ], bn[GQ];
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) bn[hq] = -__builtin_inff();
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            int I = __builtin_amdgcn_sdot4((int)q8[hq].x, (int)kk[u].x, 0, false);
            I = __builtin_amdgcn_sdot4((int)q8[hq].y, (int)kk[u].y, I, false);
            I = __builtin_amdgcn_sdot4((int)q8[hq].z, (int)kk[u].z, I, false);
            I = __builtin_amdgcn_sdot4((int)q8[hq].w, (int)kk[u].w, I, false);
            I = group_sum_i(I, lpk_log2);
            const float c = sq[hq] * ks[u];
            const float d = (float)I * c;
            const float s = round_bf16(d * rden);
            kf_exp2_parts(s * KF_LOG2E, f[u][hq], n[u][hq]);
            n[u][hq] = valid[u] ? n[u][hq] : -__builtin_inff();
            bn[hq] = fmaxf(bn[hq], n[u][hq]);
        }
    }
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) { /* the wave's maximum exponent of this batch: across the rows, then across the 16 / LPK key groups of a row */
        bn[hq] = xmax32(xmax16(bn[hq]));
        bn[hq] = fmaxf(bn[hq], dpp_f<0x128>(bn[hq]));
        if (LPK < 8) bn[hq] = fmaxf(bn[hq], dpp_f<0x124>(bn[hq]));
        if (bn[hq] > A.lo.m[hq]) { /* exact rescale of what has been summed so far (wave-uniform branch) */
            if (A.lo.m[hq] > -__builtin_inff()) {
                const int e = canon_shift(A.lo.m[hq] - bn[hq]);
                A.lo.l[hq] = ldexp_d(A.lo.l[hq], e);
#pragma unroll
                for (int i = 0; i < 8; i++) A.lo.o[hq][i] = ldexp_d(A.lo.o[hq][i], e), A.hi.o[hq][i] = ldexp_d(A.hi.o[hq][i], e);
            }
            A.lo.m[hq] = bn[hq];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
        double vd[16];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int b = 0; b < 4; b++) vd[4 * i + b] = (double)((int)(vw[i] << (24 - 8 * b)) >> 24);
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const int e = canon_shift(n[u][hq] - A.lo.m[hq]);
            const float g = f[u][hq] * vs[u]; /* ONE fp32 multiply, before the scaling: free of m */
            const double p = valid[u] ? ldexp_d((double)f[u][hq], e) : 0.0;
            const double pg = valid[u] ? ldexp_d((double)g, e) : 0.0;
            A.lo.l[hq] += p;
#pragma unroll
            for (int i = 0; i < 8; i++) A.lo.o[hq][i] = fma(pg, vd[i], A.lo.o[hq][i]), A.hi.o[hq][i] = fma(pg, vd[8 + i], A.hi.o[hq][i]);
        }
    }
}

template <int GQ, int HD>
__global__ void __launch_bounds__(ATTN_KV8_NW * 64) attn_kv8_kernel(const AttnKv8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int NW = ATTN_KV8_NW, U = ATTN_KV8_U, hd = HD;
    using Slice = AttnSlice<GQ, NW, HD, 16>; /* the shell (kf_attn_common.h): 16 codes of a key per lane */
    constexpr int LPK = Slice::LPK, KPW = Slice::KPW, lpk_log2 = Slice::lpk_log2, tstride = Slice::tstride, NQ = Slice::NQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int PS = hd + 2; /* {O[hd], L, m} as doubles */
    constexpr AttnKv8Lds lds(GQ, HD);
    static_assert(lds.fits(), "LDS");
    double* comb = reinterpret_cast<double*>(smem_raw + lds.comb);
    uint16_t* qb = reinterpret_cast<uint16_t*>(smem_raw + lds.qb);
    uint16_t* knew = reinterpret_cast<uint16_t*>(smem_raw + lds.knew);
    int8_t* q8 = reinterpret_cast<int8_t*>(smem_raw + lds.q8);
    int8_t* k8n = reinterpret_cast<int8_t*>(smem_raw + lds.k8n);
    int8_t* v8n = reinterpret_cast<int8_t*>(smem_raw + lds.v8n);
    float* stp = reinterpret_cast<float*>(smem_raw + lds.stp);
    int* flag = reinterpret_cast<int*>(smem_raw + lds.flag);

    const Slice sl(a.gq_split, a.chunk);
    const int nsp = a.n_splits, h0 = sl.h0(), grp = lane >> lpk_log2, d0 = (lane & (LPK - 1)) * 16, tstart = sl.tstart(wave, grp);

    // ---- the first K/V tiles and their steps before anything else: rows up to the launch bound exist in the cache (zero-filled at allocation: finite); rows past the
    // real position are masked later, and the row AT the position is replaced by the freshly quantised one
    u32x4 kk[U], vv[U];
    float ksr[U], vsr[U];
    auto issue = [&](int tb, int tend) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = tb + u * tstride;
            kk[u] = u32x4{0, 0, 0, 0}, vv[u] = u32x4{0, 0, 0, 0}, ksr[u] = 0.0f, vsr[u] = 0.0f;
            if (t < tend) {
                const size_t off = (size_t)t * a.kv_stride + (size_t)sl.kvh * hd + d0;
                kk[u] = *reinterpret_cast<const u32x4*>(a.k8 + off);
                vv[u] = *reinterpret_cast<const u32x4*>(a.v8 + off);
                ksr[u] = a.ks[(size_t)t * a.n_kv + sl.kvh];
                vsr[u] = a.vs[(size_t)t * a.n_kv + sl.kvh];
            }
        }
    };
    issue(tstart, sl.end(a.pos)); /* a.pos is the launch bound here */
    // ... and the q heads, the raw new key and the new value row this wave will prepare: they do not depend on the position either
    const bool qnorm = a.wq_norm != nullptr;
    HeadRaw qraw[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const int hq = wave + i * NW;
        qraw[i] = load_head(a.q + (size_t)(h0 + (hq < GQ ? hq : 0)) * hd, a.wq_norm, hd);
    }
    const HeadRaw kraw = load_head(a.k_raw + (size_t)sl.kvh * hd, a.wk_norm, hd);
    const HeadRaw vraw = load_head(a.v_raw + (size_t)sl.kvh * hd, nullptr, hd);

    const auto [pos, t1, empty] = sl.at(a.d_pos, a.pos);
    double* const part = a.part; /* [n_head][n_splits][PS] doubles */

    if (!empty) {
        // ---- prologue: the q heads of this group, normed, roped, rounded to bf16 and quantised; the new K and V rows when they lie in this slice
        const float* tab_pos = a.rope_table + (size_t)pos * hd;
#pragma unroll
        for (int i = 0; i < NQ; i++)
            if (wave + i * NW < GQ) {
                const int hq = wave + i * NW;
                prep_head(qraw[i], qnorm, tab_pos, hd, a.eps, qb + hq * hd);
                quant_head_lds(qb + hq * hd, hd, q8 + hq * hd, stp + hq);
            }
        const bool own_new = sl.holds(pos, t1);
        if (own_new && wave == (GQ % NW)) {
            prep_head(kraw, a.wk_norm != nullptr, tab_pos, hd, a.eps, knew);
            quant_head_lds(knew, hd, k8n, stp + GQ);
        }
        if (own_new && wave == ((GQ + 1) % NW)) quant_head(bf2f(vraw.x0), bf2f(vraw.x1), hd, v8n, stp + GQ + 1);
        __syncthreads();
        if (own_new && sl.gpart == 0) { /* every part of the kv-head holds the same row: one writes it */
            int8_t* krow = a.k8 + (size_t)pos * a.kv_stride + (size_t)sl.kvh * hd;
            int8_t* vrow = a.v8 + (size_t)pos * a.kv_stride + (size_t)sl.kvh * hd;
            for (int i = tid; i < hd; i += blockDim.x) krow[i] = k8n[i], vrow[i] = v8n[i];
            if (tid == 0) a.ks[(size_t)pos * a.n_kv + sl.kvh] = stp[GQ], a.vs[(size_t)pos * a.n_kv + sl.kvh] = stp[GQ + 1];
        }
        u32x4 qreg[GQ]; /* this lane's 16 codes of every q head */
        float sq[GQ];
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) qreg[hq] = *reinterpret_cast<const u32x4*>(q8 + hq * hd + d0), sq[hq] = stp[hq];
        Kv8Acc<GQ> A;
        A.lo.init(), A.hi.init();
        const float rden = 1.0f / a.inv_sqrt_hd_den; /* the value canon_score multiplies by */
        for (int tb = tstart; tb - grp - wave * KPW < t1; tb += U * tstride) { /* workgroup-uniform trip count */
            u32x4 ck[U], cv[U];
            float cks[U], cvs[U];
            bool valid[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int t = tb + u * tstride;
                ck[u] = kk[u], cv[u] = vv[u], cks[u] = ksr[u], cvs[u] = vsr[u], valid[u] = t < t1;
                if (valid[u] && t == pos) {
                    ck[u] = *reinterpret_cast<const u32x4*>(k8n + d0), cv[u] = *reinterpret_cast<const u32x4*>(v8n + d0);
                    cks[u] = stp[GQ], cvs[u] = stp[GQ + 1];
                }
            }
            if (tb - grp - wave * KPW + U * tstride < t1) issue(tb + U * tstride, t1);
            kv8_batch<GQ, LPK, U>(A, qreg, sq, ck, cv, cks, cvs, valid, lpk_log2, rden);
        }
        // ---- the wave's key groups summed, the waves through LDS.  hd = 64: four key groups per row of 16 lanes -- lanes i and i ^ 4 are added first (a symmetric
        // exchange: both lanes end with the same bits, and both will store), after which the lane layout is canon_wave_to_lds' two-groups-per-row form (its LPK = 8);
        // that runs once for each half of the lane's 16 elements
        if (LPK < 8) {
#pragma unroll
            for (int hq = 0; hq < GQ; hq++) {
                A.lo.l[hq] += __shfl_xor(A.lo.l[hq], 4, 64);
#pragma unroll
                for (int i = 0; i < 8; i++) A.lo.o[hq][i] += __shfl_xor(A.lo.o[hq][i], 4, 64), A.hi.o[hq][i] += __shfl_xor(A.hi.o[hq][i], 4, 64);
            }
        }
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) A.hi.l[hq] = A.lo.l[hq], A.hi.m[hq] = A.lo.m[hq];
        canon_wave_to_lds<GQ, 8>(A.lo, comb + (size_t)wave * GQ * PS, hd, lane, d0);
        canon_wave_to_lds<GQ, 8>(A.hi, comb + (size_t)wave * GQ * PS, hd, lane, d0 + 8);
        __syncthreads();
        canon_slice_publish<GQ, NW, HD>(comb, part, a.out, h0, nsp, sl.split);
    } else if (nsp > 1) {
        canon_slice_publish_empty<GQ, HD>(part, h0, nsp, sl.split);
    }
    if (nsp == 1) return;
    canon_arrive_and_merge<GQ, NW, HD>(part, a.counters + (int)blockIdx.y * a.cnt_stride, flag, a.out, h0, nsp); /* per (kv-head, part): its slices' workgroups meet here */
}

// ---- kf_kv8_quant_rows: one wave per (row, kv-head), K and V of it; lane j holds elements j and j + hd / 2 as quant_head wants them
__global__ void __launch_bounds__(64) kv8_quant_rows_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, long long ld, int n_kv, int hd, int8_t* __restrict__ k8,
                                                            int8_t* __restrict__ v8, float* __restrict__ ks, float* __restrict__ vs, int pos0, int kv_stride) {
    const int row = blockIdx.x, kvh = blockIdx.y;
    const HeadRaw kr = load_head(k + (size_t)row * ld + (size_t)kvh * hd, nullptr, hd), vr = load_head(v + (size_t)row * ld + (size_t)kvh * hd, nullptr, hd);
    const size_t off = (size_t)(pos0 + row) * kv_stride + (size_t)kvh * hd, so = (size_t)(pos0 + row) * n_kv + kvh;
    quant_head(bf2f(kr.x0), bf2f(kr.x1), hd, k8 + off, ks + so);
    quant_head(bf2f(vr.x0), bf2f(vr.x1), hd, v8 + off, vs + so);
}
// ---- kf_kv8_dequant_rows: one workgroup per row, one element of K and of V per thread and trip
__global__ void __launch_bounds__(256) kv8_dequant_rows_kernel(const int8_t* __restrict__ k8, const int8_t* __restrict__ v8, const float* __restrict__ ks, const float* __restrict__ vs,
                                                               int n_kv, int hd, int kv_stride, uint16_t* __restrict__ kout, uint16_t* __restrict__ vout, long long ld_out) {
    const int row = blockIdx.x, kvd = n_kv * hd;
    for (int i = threadIdx.x; i < kvd; i += blockDim.x) {
        const int kvh = i / hd;
        const size_t src = (size_t)row * kv_stride + i, dst = (size_t)row * ld_out + i;
        kout[dst] = f2bf((float)k8[src] * ks[(size_t)row * n_kv + kvh]);
        vout[dst] = f2bf((float)v8[src] * vs[(size_t)row * n_kv + kvh]);
    }
}

using AttnKv8Kernel = void (*)(AttnKv8Args);
int attn_kv8_launch(hipStream_t st, AttnKv8Args& a, const AttnPlan& p) {
    if (p.status != KF_OK) return p.status;
    if (p.route != ATTN_SLICED_KV8 || p.nw != ATTN_KV8_NW) return KF_INTERNAL_ERR;
    const AttnKv8Kernel k = p.gq == 1   ? (p.hd == 128 ? attn_kv8_kernel<1, 128> : attn_kv8_kernel<1, 64>)
                            : p.gq == 2 ? (p.hd == 128 ? attn_kv8_kernel<2, 128> : attn_kv8_kernel<2, 64>)
                                        : nullptr;
    if (!k) return KF_INTERNAL_ERR; /* a form attn_plan never names */
    a.n_splits = p.n_splits, a.chunk = p.chunk, a.gq_split = p.gq_split, a.cnt_stride = p.cnt_stride;
    a.inv_sqrt_hd_den = sqrtf((float)p.hd);
    void* args[] = {&a};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(k), dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(p.threads), args, (size_t)p.lds, st);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}
int kv8_quant_rows_launch(hipStream_t st, const uint16_t* k, const uint16_t* v, long long ld, int n, int n_kv, int hd, int8_t* k8, int8_t* v8, float* ks, float* vs, int pos0,
                          int kv_stride) {
    hipLaunchKernelGGL(kv8_quant_rows_kernel, dim3(n, n_kv), dim3(64), 0, st, k, v, ld, n_kv, hd, k8, v8, ks, vs, pos0, kv_stride);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}
int kv8_dequant_rows_launch(hipStream_t st, const int8_t* k8, const int8_t* v8, const float* ks, const float* vs, int n, int n_kv, int hd, int kv_stride, uint16_t* kout,
                            uint16_t* vout, long long ld_out) {
    hipLaunchKernelGGL(kv8_dequant_rows_kernel, dim3(n), dim3(256), 0, st, k8, v8, ks, vs, n_kv, hd, kv_stride, kout, vout, ld_out);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
