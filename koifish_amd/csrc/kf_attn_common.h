// kf_attn_common.h -- pieces of the decode attention shared by kf_attn.hip, kf_attn_kv8.hip and the persistent decode engines (kf_engine.hip, kf_xengine*.hip):
// per-head q/k RMSNorm + rotate-half RoPE (ROPE::cuInfer, rope.cu:645-672), the hardware-exp2 softmax exponent, sc1 accessors; the decode slice shell (AttnSlice: grid
// decode, lane geometry and slice ends of the three decode kernels), the canonical order's batch, publish and merge, the int8 cache's row quantiser.
#pragma once
#include <type_traits>

#include "kf_kernels.h"

namespace kf {

// sum over the 2^lg (<= 16) lanes of each aligned lane group, DPP only
__device__ __forceinline__ float group_sum16(float v, int lg) {
    if (lg >= 1) v += dpp_f<0xB1>(v);
    if (lg >= 2) v += dpp_f<0x4E>(v);
    if (lg >= 3) v += dpp_f<0x141>(v);
    if (lg >= 4) v += dpp_f<0x140>(v);
    return v;
}
// One head as loaded (raw bf16 bits, so that the loads can be issued long before their use): lane j holds the pair (j, j + hd/2)
struct HeadRaw {
    uint16_t x0, x1, w0, w1;
};
// Unconditional loads (clamped lane, the head itself standing in for a missing norm weight): a conditional load into a preset
// register makes the compiler wait for it -- and for every K/V load issued before it -- at the join.
__device__ __forceinline__ HeadRaw load_head(const uint16_t* __restrict__ src, const uint16_t* __restrict__ wn, int hd) {
    const int half = hd >> 1;
    int j = threadIdx.x & 63;
    j = j < half ? j : half - 1;
    const uint16_t* w = wn ? wn : src;
    return HeadRaw{src[j], src[j + half], w[j], w[j + half]};
}
// Prepare one head: optional per-head RMSNorm (s rounded to bf16 first, then (a*s)*w, RN store) and rotate-half
// RoPE from the host-built (cos,sin) table.  One wave per head; lane j handles the pair (j, j + hd/2).
// Result: bf16 bits in dst[hd].
// (c, sn) = the table's pair for (position, j), already in registers; rope = false: no rotation
__device__ __forceinline__ void prep_head_cs(const HeadRaw r, bool norm, bool rope, float c, float sn, int hd, float eps, uint16_t* dst, float* rstd_out = nullptr, int lane_in = -1) {
    const int lane = lane_in >= 0 ? lane_in : (int)(threadIdx.x & 63), half = hd >> 1;
    const int j = lane; /* hd <= 128: one trip covers the head */
    const bool act = j < half;
    float x0 = act ? bf2f(r.x0) : 0.f, x1 = act ? bf2f(r.x1) : 0.f; /* lanes past hd/2 hold a clamped copy */
    if (norm) {
        const float w0 = bf2f(r.w0), w1 = bf2f(r.w1);
        const double ss = wave_sum_f64_fast(fma((double)x0, (double)x0, (double)x1 * (double)x1));
        const float s0 = 1.0f / sqrtf((float)ss / (float)hd + eps);
        const float s = round_bf16(s0);
        if (rstd_out && lane == 0) *rstd_out = s0; /* the un-rounded 1/rms, for the training path's backward */
        x0 = round_bf16(x0 * s * w0);
        x1 = round_bf16(x1 * s * w1);
    }
    if (rope) {
        const float a = x0 * c, b = x1 * sn, cc = x0 * sn, d = x1 * c;
        x0 = round_bf16(a - b);
        x1 = round_bf16(cc + d);
    }
    if (act) dst[j] = f2bf(x0), dst[j + half] = f2bf(x1);
}
__device__ __forceinline__ void prep_head(const HeadRaw r, bool norm, const float* __restrict__ tab_pos, int hd, float eps, uint16_t* dst, float* rstd_out = nullptr) {
    const int j = threadIdx.x & 63;
    float c = 1.f, sn = 0.f;
    if (tab_pos && j < (hd >> 1)) c = tab_pos[2 * j], sn = tab_pos[2 * j + 1];
    prep_head_cs(r, norm, tab_pos != nullptr, c, sn, hd, eps, dst, rstd_out);
}

// e^x for x <= 0 through the hardware exp2 (v_exp_f32); exp2(-inf) = 0
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269502162933349609375f); }

constexpr int ATTN_U = 4; /* key tiles kept in flight per wave */

// ------------------------------------------------------------------------------------------------ the decode slice shell
// What attn_kernel, attn_fast_kernel (kf_attn.hip) and attn_kv8_kernel (kf_attn_kv8.hip) share in front of their arithmetic: which slice of which kv-head and which of
// its parts a workgroup is (blockIdx = (slice, kv-head * gq_split + part)), the lane geometry, where a run of tiles ends, what the position makes of the slice.
// EL = the elements of a key one lane holds: 8 (bf16 rows) or 16 (int8 rows).  The q heads' load / prepare loops, the batch loop's two bounds, the issue of the tiles
// and the lane's grp / d0 are NOT here: shared, they changed the compiler's output, so each kernel spells them out.
struct AttnAt { int pos, t1; bool empty; }; /* the position, the slice's end against it, the slice lies wholly behind it */
template <int GQ, int NW, int HD, int EL>
struct AttnSlice {
    static constexpr int hd_log2 = HD == 128 ? 7 : 6; /* head_dim 64 or 128: compile-time, so that the lane-group reductions are straight-line code */
    // LPK lanes per key (EL elements each), KPW keys per wave step, the waves interleaved over the slice; NQ q heads a wave loads and prepares
    static constexpr int LPK = HD / EL, KPW = 64 / LPK, lpk_log2 = hd_log2 - (EL == 16 ? 4 : 3), tstride = NW * KPW, NQ = (GQ + NW - 1) / NW;
    // chunk = keys per slice, fixed by the launch bound so that the K/V stream can start before pos is known; t0 its first key
    const int gq_split, split, kvh, gpart, chunk, t0;
    __device__ __forceinline__ AttnSlice(int gq_split_, int chunk_)
        : gq_split(gq_split_), split(blockIdx.x), kvh((int)blockIdx.y / gq_split), gpart((int)blockIdx.y - kvh * gq_split), chunk(chunk_), t0(split * chunk) {}
    __device__ __forceinline__ int h0() const { return (kvh * gq_split + gpart) * GQ; } /* the first of the GQ heads of THIS workgroup */
    __device__ __forceinline__ int tstart(int wave, int grp) const { return t0 + wave * KPW + grp; } /* the first key a lane walks (then every tstride-th) */
    __device__ __forceinline__ int end(int last) const { /* of the slice's keys among 0 .. last */
        int t = t0 + chunk;
        if (t > last + 1) t = last + 1;
        return t;
    }
    __device__ __forceinline__ AttnAt at(const int* d_pos, int pos_bound) const { /* the position: read from device memory in graph replay, else the launch bound */
        const int pos = d_pos ? *d_pos : pos_bound, len = pos + 1;
        return AttnAt{pos, end(pos), t0 >= len};
    }
    // the new row lies in this slice: the wave behind the q heads' waves prepares it (a second row: the wave behind that), part 0 of the kv-head writes it
    __device__ __forceinline__ bool holds(int pos, int t1) const { return (pos >= t0) && (pos < t1); }
};

// ------------------------------------------------------------------------------------------------ canonical decode attention
// The order kernels and oracle share (oracle/kf_oracle.c section 6, mode CANON), free of launch geometry:
//   score   s = bf16(d * (1 / sqrtf(hd))), d = this key's q.k dot: per lane a chain of 8 fused multiply-adds over its 8 elements, joined over the key's
//           hd / 8 lanes by the balanced tree of group_sum16;
//   weight  p = f * 2^(n - m), (f, n) = kf_exp2_parts(s * log2 e); m = ANY integer >= every n it is compared with: a power of two rescales exactly, so every
//           lane / wave / slice works against a maximum of its own and the partial sums are rescaled when they meet;
//   sums    fp64 (every term p and p * v is exact in fp64: the sums do not depend on their order to far below an fp32 ulp), out = bf16((float)(O / L)).
// The fixed reference exponent (canon_batch_fixed; the persistent engine's canonical forms): m = 0 for every lane, wave and slice, p = f * 2^n, and every partial sum at
// every level is a plain addend -- no maximum is formed or exchanged, nothing is rescaled.  The result is the one above bit for bit while |n| <= KF_CANON_FIX_LIM for
// every valid key: an fp64 addition, fma and division commute with a common power-of-two factor as long as no operand or result leaves the range where fp64 holds it
// exactly as the scaled twin, so the sums against m = 0 are the sums against m = max n times 2^(max n) at every step, and O / L is the same quotient.  The range:
//   f lies in [2^-1/2, 2^1/2] with 24 significant bits (lowest bit >= 2^-24), v is bf16 (lowest bit of the smallest subnormal 2^-133, |v| < 2^128);
//   the definition's own terms: n - m >= -2 LIM, the lowest bit of f * 2^(n - m) * v is >= 2^(-24 - 2 LIM - 133): a multiple of fp64's quantum 2^-1074 -- so exact,
//     and every sum of such terms exact or rounded as its scaled twin -- while 2 LIM <= 917, LIM <= 458.  THIS bounds the limit: beyond it the definition itself (the
//     oracle, the per-layer kernels) would round a tail term in the subnormal range and the two forms could part;
//   the fixed form's terms: lowest bit >= 2^(-157 - LIM) (LIM <= 917), the largest sum < 2^11 keys * 2^(1/2 + LIM) * 2^128 < 2^1024 (LIM <= 884): both far inside.
// LIM = 448 = 7 * 64, the multiple of 64 below 458: scores up to |s| = 448 / log2 e = 310, where an fp32 softmax has long overflowed.  A lane that meets a valid key
// outside the range sets a sticky flag (NaN-safe: !(|n| <= LIM)); what becomes of the flag is the caller's (the engine latches bit 128 of its error word).
constexpr float KF_LOG2E = 1.44269502162933349609375f;
constexpr float KF_CANON_FIX_LIM = 448.0f;
__device__ __forceinline__ float canon_score(const float (&q)[8], u32x4 kw, int lpk_log2, float rden) {
    const uint32_t k4[4] = {kw.x, kw.y, kw.z, kw.w};
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        d = fmaf(q[2 * i], bf_lo(k4[i]), d);
        d = fmaf(q[2 * i + 1], bf_hi(k4[i]), d);
    }
    d = group_sum16(d, lpk_log2);
    return round_bf16(d * rden);
}
// exponent of an exact rescale: d = n - m <= 0 (integer-valued), -inf or NaN (both sides -inf): clamped so that the scaled value underflows to 0
__device__ __forceinline__ int canon_shift(float d) { return (int)fmaxf(d, -1022.0f); }
__device__ __forceinline__ double ldexp_d(double v, int e) { return __builtin_ldexp(v, e); }
// a + b of the two halves of a 32-lane / 16-lane swap, fp64 (the row-swap reduce-scatter of the key-group sums)
__device__ __forceinline__ double swap32_add_d(double a, double b) {
    const unsigned long long ua = __builtin_bit_cast(unsigned long long, a), ub = __builtin_bit_cast(unsigned long long, b);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)ua, (unsigned)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi[0] << 32) | lo[0]) + __builtin_bit_cast(double, ((unsigned long long)hi[1] << 32) | lo[1]);
}
__device__ __forceinline__ double swap16_add_d(double a, double b) {
    const unsigned long long ua = __builtin_bit_cast(unsigned long long, a), ub = __builtin_bit_cast(unsigned long long, b);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)ua, (unsigned)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi[0] << 32) | lo[0]) + __builtin_bit_cast(double, ((unsigned long long)hi[1] << 32) | lo[1]);
}
// One wave's share of a slice: running fp64 sums of its keys against the wave's own reference exponent.
template <int GQ>
struct CanonAcc {
    double o[GQ][8], l[GQ];
    float m[GQ]; /* integer-valued, -inf before the first valid key */
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            m[hq] = -__builtin_inff(), l[hq] = 0.0;
#pragma unroll
            for (int i = 0; i < 8; i++) o[hq][i] = 0.0;
        }
    }
};
// row broadcast (gfx90a+: row_newbcast:K -- every lane of a row of 16 gets lane K's value) and row rotate (row_ror:K: lane i gets lane i + K (mod 16)... of its row)
template <int K>
__device__ __forceinline__ uint32_t row_bcast_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + K, 0xF, 0xF, true);
}
template <int K>
__device__ __forceinline__ float row_bcast_f(float v) { return __uint_as_float(row_bcast_u<K>(__float_as_uint(v))); }
template <int K>
__device__ __forceinline__ double row_bcast_d(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    return __builtin_bit_cast(double, ((unsigned long long)row_bcast_u<K>((uint32_t)(u >> 32)) << 32) | row_bcast_u<K>((uint32_t)u));
}
// the q.k dot of canon_score without the scale and the rounding
__device__ __forceinline__ float canon_dot(const float (&q)[8], u32x4 kw, int lpk_log2) {
    const uint32_t k4[4] = {kw.x, kw.y, kw.z, kw.w};
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        d = fmaf(q[2 * i], bf_lo(k4[i]), d);
        d = fmaf(q[2 * i + 1], bf_hi(k4[i]), d);
    }
    return group_sum16(d, lpk_log2);
}
template <int GQ, int U, int I = 1>
__device__ __forceinline__ void canon_pick_item(const float (&d)[U][GQ], const bool (&valid)[U], int lig, float& mine, bool& vmine) {
    if constexpr (I < U * GQ) {
        mine = lig == I ? d[I / GQ][I % GQ] : mine;
        vmine = lig == I ? valid[I / GQ] : vmine;
        canon_pick_item<GQ, U, I + 1>(d, valid, lig, mine, vmine);
    }
}
// max over the lanes lig, lig + GQ, lig + 2 GQ, ... (U of them) of a row: after the steps lane i holds the maximum over i, i + GQ, ..., i + (U - 1) GQ (mod 16)
template <int GQ, int U, int STEP = 1>
__device__ __forceinline__ float canon_items_max(float v) {
    if constexpr (STEP < U) {
        v = fmaxf(v, dpp_f<0x120 + ((16 - GQ * STEP) & 15)>(v)); /* row_ror:(16 - s): lane i reads lane i + s (mod 16) */
        return canon_items_max<GQ, U, STEP * 2>(v);
    } else {
        return v;
    }
}
template <int GQ, int HQ = 0>
__device__ __forceinline__ void canon_heads_max(float nm, float (&bn)[GQ]) {
    if constexpr (HQ < GQ) {
        bn[HQ] = row_bcast_f<HQ>(nm); /* lane hq of the row: the maximum over the head's items hq, hq + GQ, ... */
        canon_heads_max<GQ, HQ + 1>(nm, bn);
    }
}
template <int GQ, int U, int I = 0>
__device__ __forceinline__ void canon_apply_items(CanonAcc<GQ>& A, double p, const double (&vd)[U][8]) {
    if constexpr (I < U * GQ) {
        constexpr int u = I / GQ, hq = I % GQ;
        const double pi = row_bcast_d<I>(p);
        A.l[hq] += pi;
#pragma unroll
        for (int i = 0; i < 8; i++) A.o[hq][i] = fma(pi, vd[u][i], A.o[hq][i]);
        canon_apply_items<GQ, U, I + 1>(A, p, vd);
    }
}
// (Round 6, measured and removed: two query heads per v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 in the score chain and in the exponential's polynomial -- bit-identical (179
//  canonical tests), half the vector instructions of those two parts, and slower: the single-sequence engine 2304 -> 2103 tokens/s, 32 batched sequences 7770 -> 7410: the operand
//  pairs have to be assembled in even-aligned register pairs per use.)
#ifndef KF_CANON_ITEMS
#define KF_CANON_ITEMS 0 /* scratch/build_variant.py A/B.  1 = the item-per-lane form below: bit for bit the same (194 canonical tests), a quarter fewer vector instructions per key
                            tile on paper -- and SLOWER on the part: 32 sequences 7770 -> 6360 tokens/s, 16: 6240 -> 5710, 8: 4625 -> 4450, the single-sequence engine unchanged (each
                            broadcast is a DPP move with its wait states in front of a dependent fp64 chain; the replicated form keeps sixteen independent lanes busy instead).  Off. */
#endif
// one batch of U key tiles of this lane's key group: k / v tiles (8 elements of this lane), validity per tile; q as 8 floats per head
// KF_CANON_ITEMS (round 6, measured and left off): hd = 128, a key group is a row of 16 lanes -- the U * GQ dots of a group stand in all of its 16 lanes after the tree; the
// score's scale and rounding, the exponential's parts and the exact power-of-two weight p worked out ONCE, item i = u * GQ + hq in lane i of the group, p_i handed to the
// group's lanes by a row broadcast: the same operations on the same values as the per-lane form.
template <int GQ, int LPK, int U = ATTN_U>
__device__ __forceinline__ void canon_batch(CanonAcc<GQ>& A, const float (&qf)[GQ][8], const u32x4 (&kk)[U], const u32x4 (&vv)[U], const bool (&valid)[U], int lpk_log2, float rden) {
    if constexpr (KF_CANON_ITEMS && LPK == 16 && U * GQ <= 16 && (GQ & (GQ - 1)) == 0 && (U & (U - 1)) == 0) {
        constexpr int NI = U * GQ;
        const int lig = (int)(threadIdx.x & 15);
        float d[U][GQ];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int hq = 0; hq < GQ; hq++) d[u][hq] = canon_dot(qf[hq], kk[u], lpk_log2);
        float mine = d[0][0];
        bool vmine = valid[0];
        canon_pick_item<GQ, U>(d, valid, lig, mine, vmine);
        float f, n;
        kf_exp2_parts(round_bf16(mine * rden) * KF_LOG2E, f, n);
        vmine = vmine && lig < NI;
        n = vmine ? n : -__builtin_inff();
        float bn[GQ];
        canon_heads_max<GQ>(canon_items_max<GQ, U>(n), bn);
        float m_mine = A.m[0];
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) { /* the wave's maximum exponent of this batch */
            bn[hq] = xmax32(xmax16(bn[hq]));
            if (bn[hq] > A.m[hq]) { /* exact rescale of what has been summed so far (wave-uniform branch; the first batch has nothing to rescale) */
                if (A.m[hq] > -__builtin_inff()) {
                    const int e = canon_shift(A.m[hq] - bn[hq]);
                    A.l[hq] = ldexp_d(A.l[hq], e);
#pragma unroll
                    for (int i = 0; i < 8; i++) A.o[hq][i] = ldexp_d(A.o[hq][i], e);
                }
                A.m[hq] = bn[hq];
            }
            m_mine = (lig & (GQ - 1)) == hq ? A.m[hq] : m_mine;
        }
        const double p = vmine ? ldexp_d((double)f, canon_shift(n - m_mine)) : 0.0;
        double vd[U][8];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
            for (int i = 0; i < 4; i++) vd[u][2 * i] = (double)bf_lo(vw[i]), vd[u][2 * i + 1] = (double)bf_hi(vw[i]);
        }
        canon_apply_items<GQ, U>(A, p, vd);
        return;
    }
    float f[U][GQ], n[U][GQ], bn[GQ];
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) bn[hq] = -__builtin_inff();
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const float s = canon_score(qf[hq], kk[u], lpk_log2, rden);
            kf_exp2_parts(s * KF_LOG2E, f[u][hq], n[u][hq]);
            n[u][hq] = valid[u] ? n[u][hq] : -__builtin_inff();
            bn[hq] = fmaxf(bn[hq], n[u][hq]);
        }
    }
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) { /* the wave's maximum exponent of this batch */
        bn[hq] = xmax32(xmax16(bn[hq]));
        if (LPK < 16) bn[hq] = fmaxf(bn[hq], dpp_f<0x128>(bn[hq]));
        if (bn[hq] > A.m[hq]) { /* exact rescale of what has been summed so far (wave-uniform branch; the first batch has nothing to rescale) */
            if (A.m[hq] > -__builtin_inff()) {
                const int e = canon_shift(A.m[hq] - bn[hq]);
                A.l[hq] = ldexp_d(A.l[hq], e);
#pragma unroll
                for (int i = 0; i < 8; i++) A.o[hq][i] = ldexp_d(A.o[hq][i], e);
            }
            A.m[hq] = bn[hq];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
        double vd[8];
#pragma unroll
        for (int i = 0; i < 4; i++) vd[2 * i] = (double)bf_lo(vw[i]), vd[2 * i + 1] = (double)bf_hi(vw[i]);
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const double p = valid[u] ? ldexp_d((double)f[u][hq], canon_shift(n[u][hq] - A.m[hq])) : 0.0;
            A.l[hq] += p;
#pragma unroll
            for (int i = 0; i < 8; i++) A.o[hq][i] = fma(p, vd[i], A.o[hq][i]);
        }
    }
}
// ---- the same batch against the fixed reference exponent m = 0 (the rule and its range: the comment block above canon_score): no batch maximum, no cross-lane
// exchange between the exponentials and the P.V chains, no rescale, p = f * 2^n; `oob`: this lane has met a valid key with |n| > KF_CANON_FIX_LIM (sticky)
template <int GQ>
struct CanonAccFixed {
    double o[GQ][8], l[GQ];
    bool oob;
    __device__ __forceinline__ void init() {
        oob = false;
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            l[hq] = 0.0;
#pragma unroll
            for (int i = 0; i < 8; i++) o[hq][i] = 0.0;
        }
    }
};
template <int GQ, int LPK, int U = ATTN_U>
__device__ __forceinline__ void canon_batch_fixed(CanonAccFixed<GQ>& A, const float (&qf)[GQ][8], const u32x4 (&kk)[U], const u32x4 (&vv)[U], const bool (&valid)[U], int lpk_log2, float rden) {
    float f[U][GQ], n[U][GQ];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const float s = canon_score(qf[hq], kk[u], lpk_log2, rden);
            kf_exp2_parts(s * KF_LOG2E, f[u][hq], n[u][hq]);
            A.oob |= valid[u] && !(fabsf(n[u][hq]) <= KF_CANON_FIX_LIM);
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
        double vd[8];
#pragma unroll
        for (int i = 0; i < 4; i++) vd[2 * i] = (double)bf_lo(vw[i]), vd[2 * i + 1] = (double)bf_hi(vw[i]);
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const double p = valid[u] ? ldexp_d((double)f[u][hq], (int)n[u][hq]) : 0.0;
            A.l[hq] += p;
#pragma unroll
            for (int i = 0; i < 8; i++) A.o[hq][i] = fma(p, vd[i], A.o[hq][i]);
        }
    }
}
// sums over the wave's key groups, left in LDS: c[d] for d < hd, c[hd] = l, c[hd + 1] = m (as a double); c = this wave's [hq] row of hd + 2 doubles
// (CanonAccFixed: the same rows without an exponent -- c[hd + 1] is not written)
template <int GQ, int LPK, class Acc>
__device__ __forceinline__ void canon_wave_to_lds(const Acc& A, double* comb_wave /* [GQ][hd + 2] */, int hd, int lane, int d0) {
    const int row = lane >> 4;
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) {
        double s1[4], r2[2];
#pragma unroll
        for (int i = 0; i < 4; i++) s1[i] = swap32_add_d(A.o[hq][i], A.o[hq][i + 4]);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            r2[i] = swap16_add_d(s1[i], s1[i + 2]);
            if (LPK < 16) r2[i] += dpp_d<0x128>(r2[i]); /* two key groups per row: row_ror:8 */
        }
        double lt = xsum16_d(xsum32_d(A.l[hq]));
        if (LPK < 16) lt += dpp_d<0x128>(lt);
        double* c = comb_wave + (size_t)hq * (hd + 2);
        if (LPK == 16 || (lane & 8) == 0) c[d0 + 2 * row] = r2[0], c[d0 + 2 * row + 1] = r2[1];
        if constexpr (std::is_same_v<Acc, CanonAccFixed<GQ>>) {
            if (lane == 0) c[hd] = lt;
        } else {
            if (lane == 0) c[hd] = lt, c[hd + 1] = (double)A.m[hq];
        }
    }
}

// ---- the canonical order's slice bookkeeping behind canon_wave_to_lds, shared by attn_kernel (kf_attn.hip) and attn_kv8_kernel (kf_attn_kv8.hip): ONE body each, so the
// hand-off cannot drift apart between them.  PS = hd + 2 doubles {O[hd], L, m} per (head, slice); h0 = the workgroup's first head; odst = the token's output row.
// the waves' partials in LDS (comb [NW][GQ][PS], behind a barrier) rescaled exactly to the slice's maximum exponent and summed: the output itself when there is one slice,
// else this slice's partial, written with agent-scope relaxed atomic stores
template <int GQ, int NW, int HD>
__device__ __forceinline__ void canon_slice_publish(const double* comb, double* part, uint16_t* odst, int h0, int nsp, int split) {
    constexpr int hd = HD, hd_log2 = HD == 128 ? 7 : 6, PS = hd + 2;
    for (int i = threadIdx.x; i < GQ * hd; i += blockDim.x) {
        const int hq = i >> hd_log2, d = i & (hd - 1);
        float ms = -__builtin_inff();
#pragma unroll
        for (int sl = 0; sl < NW; sl++) ms = fmaxf(ms, (float)comb[((size_t)sl * GQ + hq) * PS + hd + 1]);
        double o = 0.0, L = 0.0;
#pragma unroll
        for (int sl = 0; sl < NW; sl++) {
            const double* c = comb + ((size_t)sl * GQ + hq) * PS;
            const int e = canon_shift((float)c[hd + 1] - ms);
            o += ldexp_d(c[d], e);
            L += ldexp_d(c[hd], e);
        }
        if (nsp == 1) {
            odst[(size_t)(h0 + hq) * hd + d] = f2bf((float)(o / L));
        } else {
            double* dst = part + ((size_t)(h0 + hq) * nsp + split) * PS;
            __hip_atomic_store(dst + d, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) __hip_atomic_store(dst + hd, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_store(dst + hd + 1, (double)ms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// a slice behind the position: a neutral partial (it still arrives)
template <int GQ, int HD>
__device__ __forceinline__ void canon_slice_publish_empty(double* part, int h0, int nsp, int split) {
    constexpr int hd = HD, hd_log2 = HD == 128 ? 7 : 6, PS = hd + 2;
    for (int i = threadIdx.x; i < GQ * hd; i += blockDim.x) {
        const int hq = i >> hd_log2, d = i & (hd - 1);
        double* dst = part + ((size_t)(h0 + hq) * nsp + split) * PS;
        __hip_atomic_store(dst + d, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (d == 0) __hip_atomic_store(dst + hd, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_store(dst + hd + 1, -(double)__builtin_inff(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// arrival, and the merge by the workgroup that arrives last for its (kv-head, part): every storing wave drains vmcnt, the workgroup barriers, ONE lane adds to the counter
// (agent scope); the workgroup whose add returned nsp - 1 reads every partial with agent-scope relaxed atomic loads behind a barrier and re-zeroes the counter.  Every thread
// merges its output elements over the slices: the head is the same for the whole wave (64 | hd), lane sp of the wave fetches (m, L) of slice sp, the maximum exponent and the
// rescaled L are formed in registers; the element's own chain walks the slices in order (fp64: the order does not matter).
template <int GQ, int NW, int HD>
__device__ __forceinline__ void canon_arrive_and_merge(const double* part, int* counter, int* flag, uint16_t* odst, int h0, int nsp) {
    constexpr int hd = HD, hd_log2 = HD == 128 ? 7 : 6, PS = hd + 2;
    const int tid = threadIdx.x, lane = tid & 63;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag[0] = (old == nsp - 1);
    }
    __syncthreads();
    if (!flag[0]) return;
    constexpr int NT = NW * 64;
    constexpr int NV = (GQ * 128 + NT - 1) / NT; /* output elements per thread (hd <= 128) */
#pragma unroll
    for (int e = 0; e < NV; e++) {
        const int i = tid + e * NT;
        const bool in = i < GQ * hd;
        const int hq = in ? (i >> hd_log2) : 0, d = i & (hd - 1);
        const double* p = part + (size_t)(h0 + hq) * nsp * PS;
        const bool mine = in && lane < nsp;
        const float ms = mine ? (float)__hip_atomic_load(p + (size_t)lane * PS + hd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -__builtin_inff();
        const double ls = mine ? __hip_atomic_load(p + (size_t)lane * PS + hd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        const float Mx = wave_max(ms);
        const int sh = canon_shift(ms - Mx);
        const double L = wave_sum_f64_fast(ldexp_d(ls, sh));
        double o = 0.0;
        for (int sp = 0; sp < nsp; sp++) {
            const double v = in ? __hip_atomic_load(p + (size_t)sp * PS + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            o += ldexp_d(v, __builtin_amdgcn_readlane(sh, sp));
        }
        if (in) odst[(size_t)(h0 + hq) * hd + d] = f2bf((float)(o / L));
    }
    if (tid == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ the same slice bookkeeping in fp32 (the engine's default mode)
// Scores on packed bf16 pairs (v_dot2c_f32_bf16), weights p = v_exp_f32(s * log2 e - m) against an INTEGER reference exponent m (the ceiling of the wave's largest
// s * log2 e), fp32 sums.  Integer exponents keep every rescale an exact power of two, so a wave's (O, L, m) meets the other waves' -- and the slices' in the fp64
// merge, which takes them converted -- exactly as the canonical form's do; what differs from it is the approximate exponential and fp32 summation (the decode
// kernel's default arithmetic, held to the tolerance tests).
template <int GQ>
struct FastAcc {
    float o[GQ][8], l[GQ], m[GQ];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            m[hq] = -__builtin_inff(), l[hq] = 0.f;
#pragma unroll
            for (int i = 0; i < 8; i++) o[hq][i] = 0.f;
        }
    }
};
__device__ __forceinline__ int fast_shift(float d) { return (int)fmaxf(d, -200.0f); } /* d = m_a - m_b <= 0, integer-valued, -inf or NaN: clamped so that the scaled value underflows to 0 */
template <int GQ, int LPK, int U>
__device__ __forceinline__ void fast_batch(FastAcc<GQ>& A, const u32x4 (&q)[GQ], const u32x4 (&kk)[U], const u32x4 (&vv)[U], const bool (&valid)[U], int lpk_log2, float rden) {
    float t[U][GQ], bn[GQ];
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) bn[hq] = -__builtin_inff();
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            float d = dot2_bf16(q[hq].x, kk[u].x, 0.f);
            d = dot2_bf16(q[hq].y, kk[u].y, d);
            d = dot2_bf16(q[hq].z, kk[u].z, d);
            d = dot2_bf16(q[hq].w, kk[u].w, d);
            d = group_sum16(d, lpk_log2);
            t[u][hq] = valid[u] ? round_bf16(d * rden) * KF_LOG2E : -__builtin_inff();
            bn[hq] = fmaxf(bn[hq], t[u][hq]);
        }
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) {
        bn[hq] = xmax32(xmax16(bn[hq]));
        if (LPK < 16) bn[hq] = fmaxf(bn[hq], dpp_f<0x128>(bn[hq]));
        bn[hq] = ceilf(bn[hq]);
        if (bn[hq] > A.m[hq]) { /* wave-uniform */
            if (A.m[hq] > -__builtin_inff()) {
                const int e = fast_shift(A.m[hq] - bn[hq]);
                A.l[hq] = __builtin_ldexpf(A.l[hq], e);
#pragma unroll
                for (int i = 0; i < 8; i++) A.o[hq][i] = __builtin_ldexpf(A.o[hq][i], e);
            }
            A.m[hq] = bn[hq];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
        float vf[8];
#pragma unroll
        for (int i = 0; i < 4; i++) vf[2 * i] = bf_lo(vw[i]), vf[2 * i + 1] = bf_hi(vw[i]);
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const float p = valid[u] ? __builtin_amdgcn_exp2f(t[u][hq] - A.m[hq]) : 0.f;
            A.l[hq] += p;
#pragma unroll
            for (int i = 0; i < 8; i++) A.o[hq][i] = fmaf(p, vf[i], A.o[hq][i]);
        }
    }
}
__device__ __forceinline__ float swap32_add_f(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap16_add_f(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// sums over the wave's key groups, left in LDS: c[d] for d < hd, c[hd] = l, c[hd + 1] = m; c = this wave's [hq] row of hd + 2 floats (canon_wave_to_lds in fp32)
template <int GQ, int LPK>
__device__ __forceinline__ void fast_wave_to_lds(const FastAcc<GQ>& A, float* comb_wave /* [GQ][hd + 2] */, int hd, int lane, int d0) {
    const int row = lane >> 4;
#pragma unroll
    for (int hq = 0; hq < GQ; hq++) {
        float s1[4], r2[2];
#pragma unroll
        for (int i = 0; i < 4; i++) s1[i] = swap32_add_f(A.o[hq][i], A.o[hq][i + 4]);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            r2[i] = swap16_add_f(s1[i], s1[i + 2]);
            if (LPK < 16) r2[i] += dpp_f<0x128>(r2[i]); /* two key groups per row: row_ror:8 */
        }
        float lt = xsum16(xsum32(A.l[hq]));
        if (LPK < 16) lt += dpp_f<0x128>(lt);
        float* c = comb_wave + (size_t)hq * (hd + 2);
        if (LPK == 16 || (lane & 8) == 0) *reinterpret_cast<float2*>(c + d0 + 2 * row) = float2{r2[0], r2[1]};
        if (lane == 0) c[hd] = lt, c[hd + 1] = A.m[hq];
    }
}

__device__ __forceinline__ void st_sc1(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the int8 KV cache's row quantiser, shared by attn_kv8_kernel / kv8_quant_rows_kernel (kf_attn_kv8.hip) and attn_prefill_kv8_kernel (kf_attn_prefill_kv8.hip)
// the row quantiser (kf_act_quant_i8's arithmetic) on one head held by one wave as load_head / prep_head deal it: lane j < hd / 2 holds elements j and j + hd / 2
__device__ __forceinline__ void quant_head(float x0, float x1, int hd, int8_t* dst, float* step_out) {
    const int j = threadIdx.x & 63, half = hd >> 1;
    const bool act = j < half;
    const float amax = wave_max(act ? fmaxf(fabsf(x0), fabsf(x1)) : 0.0f);
    const float s = __fdiv_rn(amax, 127.0f);
    float r0 = 0.0f, r1 = 0.0f;
    if (amax != 0.0f) {
        r0 = fminf(fmaxf(roundf(__fdiv_rn(x0, s)), -127.0f), 127.0f);
        r1 = fminf(fmaxf(roundf(__fdiv_rn(x1, s)), -127.0f), 127.0f);
    }
    if (act) dst[j] = (int8_t)(int)r0, dst[j + half] = (int8_t)(int)r1;
    if (j == 0) *step_out = s;
}
// ... on a bf16 head this wave has just written to LDS (prep_head: the lane reads back its own two elements)
__device__ __forceinline__ void quant_head_lds(const uint16_t* src, int hd, int8_t* dst, float* step_out) {
    const int j = threadIdx.x & 63, half = hd >> 1;
    const bool act = j < half; /* the lanes past hd / 2 read nothing: no lane depends on another lane's LDS store */
    quant_head(act ? bf2f(src[j]) : 0.0f, act ? bf2f(src[j + half]) : 0.0f, hd, dst, step_out);
}

}  // namespace kf
