// kf_gemv_w4a8.hip -- kf_linear_w4a8: 4-bit group weights times int8 activations on v_dot4c_i32_i8 (include/kf_abi.h "int8 activations for 4-bit layers"; the launch is
// kf::a8_plan's, kf_a8.h).  The shape is kf_gemv_a8.hip's:
//   * a lane owns one 128-weight group per step: four 16-byte Packed128 blocks of 32 codes (PackedQ.hpp:99-183), streamed with non-temporal 16-byte loads.
//   * the codes become packed int8 operands with a shift and a mask per FOUR weights: (D >> 4c) & 0x0F0F0F0F, c = 0, 1, picks the low (c = 0) or high nibble of every byte
//     of a dword.  A block's dword 3 holds elements 0 .. 7 with element 0 in bits 28 .. 31 (kf_gemv_blocks.h dot_q4_dword), so byte b of dword d holds element
//     8 (3 - d) + 6 - 2b in its high and 8 (3 - d) + 7 - 2b in its low nibble: w4a8_elem.  The activations are staged in LDS ONCE per workgroup in exactly that order.
//   * codes are dotted as they are stored (0 .. 15); qBias * S_g comes off the dotted sum, S_g = the group's sum of q, formed once at staging.
//   * an unpacked group is dotted against every token row of the pass (TT rows); token tiles are grid.y.
//   * order: I_g and S_g are exact int32 whatever lanes form them.  The group's term c = STEP * I_g - ZERO * S_g is three fp32 operations -- the multiply STEP * I_g rounds
//     once (8 + 18 significant bits), ZERO * S_g is exact (8 + 14), the subtract rounds once -- and the row's terms are added in ONE ascending chain over g
//     (A8_ORDER_CHAIN): each step the lanes of a row hand their c round and every lane adds them in lane = group order.  Lanes per row, grid and TT never touch a bit.
//     The file is built with -ffp-contract=off (build.py): the multiply, the subtract and the add below stay three instructions.
#include "kf_a8.h"

namespace kf {

struct W4A8Args {
    const u32x4* w;
    const uint16_t* zerow;
    const uint16_t* stepw;
    const int8_t* q;
    const float* stepx;
    uint16_t* y;
    const uint16_t* bias;
    const uint16_t* residual;
    int M, K, G, nTok, lpr_log2, iters, qBias;
};

template <int TT>
__global__ void __launch_bounds__(A8_THREADS) w4a8_kernel(W4A8Args a) {
    extern __shared__ __align__(16) uint32_t qs[]; /* [TT][G][A8_GDW] */
    const int G = a.G, tok0 = blockIdx.y * TT;
    for (int i = threadIdx.x; i < TT * G * 32; i += A8_THREADS) {
        const int tg = i >> 5, j = i & 31, t = tg / G, g = tg - t * G;
        uint32_t v = 0;
        if (tok0 + t < a.nTok) {
            const uint8_t* qr = reinterpret_cast<const uint8_t*>(a.q) + (size_t)(tok0 + t) * a.K + (size_t)g * A8_GROUP;
#pragma unroll
            for (int b = 0; b < 4; b++) v |= (uint32_t)qr[w4a8_elem(j, b)] << (8 * b);
        }
        qs[tg * A8_GDW + j] = v;
    }
    __syncthreads();
    for (int tg = threadIdx.x; tg < TT * G; tg += A8_THREADS) {
        int s = 0;
        for (int j = 0; j < 32; j++) s = __builtin_amdgcn_sdot4(0x01010101, (int)qs[tg * A8_GDW + j], s, false);
        qs[tg * A8_GDW + 32] = (uint32_t)s;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int LPR = 1 << a.lpr_log2, l = lane & (LPR - 1);
    const long row = ((long)blockIdx.x * (A8_THREADS / 64) + wave) * (64 >> a.lpr_log2) + (lane >> a.lpr_log2);
    const bool rv = row < a.M;
    float acc[TT];
#pragma unroll
    for (int t = 0; t < TT; t++) acc[t] = 0.0f;
    for (int it = 0; it < a.iters; it++) {
        const int g = it * LPR + l;
        int I[TT], S[TT];
#pragma unroll
        for (int t = 0; t < TT; t++) I[t] = 0, S[t] = 0;
        float sw = 0.0f, zw = 0.0f;
        if (rv && g < G) {
            const size_t gi = (size_t)row * G + g;
            sw = bf2f(a.stepw[gi]), zw = bf2f(a.zerow[gi]);
            u32x4 W[W4A8_BLOCKS];
#pragma unroll
            for (int k = 0; k < W4A8_BLOCKS; k++) W[k] = ld_nt(a.w + gi * W4A8_BLOCKS + k);
#pragma unroll
            for (int t = 0; t < TT; t++) {
                const uint32_t* qg = qs + (t * G + g) * A8_GDW;
                const u32x4* qv = reinterpret_cast<const u32x4*>(qg);
                int s = 0;
#pragma unroll
                for (int k = 0; k < W4A8_BLOCKS; k++)
#pragma unroll
                    for (int dp = 0; dp < 2; dp++) { /* dwords 2 dp, 2 dp + 1 of the block: staged dwords 8 k + 4 dp .. + 3 */
                        const u32x4 q0 = qv[k * 2 + dp];
                        const uint32_t D0 = W[k][2 * dp], D1 = W[k][2 * dp + 1];
                        s = __builtin_amdgcn_sdot4((int)(D0 & 0x0F0F0F0Fu), (int)q0[0], s, false);
                        s = __builtin_amdgcn_sdot4((int)((D0 >> 4) & 0x0F0F0F0Fu), (int)q0[1], s, false);
                        s = __builtin_amdgcn_sdot4((int)(D1 & 0x0F0F0F0Fu), (int)q0[2], s, false);
                        s = __builtin_amdgcn_sdot4((int)((D1 >> 4) & 0x0F0F0F0Fu), (int)q0[3], s, false);
                    }
                S[t] = (int)qg[32];
                I[t] = s - a.qBias * S[t];
            }
        }
        const int n = (G - it * LPR) < LPR ? (G - it * LPR) : LPR; /* groups of this step: uniform */
#pragma unroll
        for (int t = 0; t < TT; t++) {
            const float p = sw * (float)I[t]; /* one rounding */
            const float z = zw * (float)S[t]; /* exact: <= 8 + 14 significant bits */
            const float c = p - z;
            for (int j = 0; j < n; j++) acc[t] = acc[t] + __shfl(c, j, LPR);
        }
    }
    if (rv && l == 0) {
#pragma unroll
        for (int t = 0; t < TT; t++) {
            if (tok0 + t >= a.nTok) break;
            a8_store(a.y, a.bias, a.residual, a.stepx[tok0 + t], acc[t], row, (size_t)(tok0 + t) * a.M + row);
        }
    }
}

int w4a8_matvec_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok) {
    W4A8Args a;
    a.w = reinterpret_cast<const u32x4*>(w->data);
    a.zerow = w->gama + w->ne0 + w->ne1;                        /* gama_T(ZERO), GTensor.cpp:456-510 */
    a.stepw = a.zerow + (size_t)w->ne0 * w->ne1 / w->lGroup;    /* gama_T(STEP) */
    a.q = q, a.stepx = step, a.y = y, a.bias = bias, a.residual = residual;
    a.M = w->ne0, a.K = w->ne1, a.G = p.n_groups, a.nTok = nTok, a.lpr_log2 = p.lpr_log2, a.iters = p.iters, a.qBias = p.qbias;
    return p.tok_tile == 1 ? a8_go(w4a8_kernel<1>, p, st, a) : a8_go(w4a8_kernel<A8_TOK_TILE>, p, st, a);
}

}  // namespace kf
