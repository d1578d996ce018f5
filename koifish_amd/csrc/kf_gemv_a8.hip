// kf_gemv_a8.hip -- kf_linear_a8: 1-bit / ternary weights times int8 activations on v_dot4c_i32_i8 (include/kf_abi.h "int8 activations"; the launch is kf::a8_plan's).
//   * a lane owns one 128-weight group per step: one 16-byte Packed128 block of 1-bit codes, two of 2-bit codes (PackedQ.hpp:200-239), streamed with 16-byte loads.
//   * the codes become packed int8 weights with a shift and a mask per FOUR weights -- (D >> s) & 0x01010101 picks bit s of every byte of a dword, (D >> 2k) & 0x03030303
//     every byte's k-th 2-bit code -- and go straight into v_dot4c_i32_i8.  Which four elements that is follows from the blocks' most-significant-first order; the
//     activations are staged in LDS ONCE per workgroup in exactly that order (kf_a8.h a8_elem), so the loop holds no per-weight reversal.
//   * codes are dotted as they are stored; the bias (ternary: code - 1) comes off as qBias * sum(q of the group), a sum formed once at staging.
//   * an unpacked block is dotted against every token row of the pass (TT rows: the XCfg::NB idea); token tiles are grid.y.
//   * order: I_g is an exact int32 whatever lanes form it; the row's fp32 products step_w[g] * I_g are added in ONE ascending chain over g (A8_ORDER_CHAIN): each step the
//     lanes of a row hand their products round and every lane adds them in lane = group order.  Lanes per row, grid and TT never touch a bit.
#include "kf_a8.h"

namespace kf {

struct A8Args {
    const u32x4* w;
    const uint16_t* stepw;
    const int8_t* q;
    const float* stepx;
    uint16_t* y;
    const uint16_t* bias;
    const uint16_t* residual;
    int M, K, G, nTok, lpr_log2, iters, qBias;
};

template <int BITS, int TT>
__global__ void __launch_bounds__(A8_THREADS) a8_kernel(A8Args a) {
    extern __shared__ __align__(16) uint32_t qs[]; /* [TT][G][A8_GDW] */
    const int G = a.G, tok0 = blockIdx.y * TT;
    for (int i = threadIdx.x; i < TT * G * 32; i += A8_THREADS) {
        const int tg = i >> 5, j = i & 31, t = tg / G, g = tg - t * G;
        uint32_t v = 0;
        if (tok0 + t < a.nTok) {
            const uint8_t* qr = reinterpret_cast<const uint8_t*>(a.q) + (size_t)(tok0 + t) * a.K + (size_t)g * A8_GROUP;
#pragma unroll
            for (int b = 0; b < 4; b++) v |= (uint32_t)qr[a8_elem<BITS>(j, b)] << (8 * b);
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
        int I[TT];
#pragma unroll
        for (int t = 0; t < TT; t++) I[t] = 0;
        float sw = 0.0f;
        if (rv && g < G) {
            const size_t gi = (size_t)row * G + g;
            sw = bf2f(a.stepw[gi]);
            constexpr int NB = BITS; /* 16-byte blocks per group */
            u32x4 W[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) W[k] = ld_nt(a.w + gi * NB + k);
#pragma unroll
            for (int t = 0; t < TT; t++) {
                const uint32_t* qg = qs + (t * G + g) * A8_GDW;
                const u32x4* qv = reinterpret_cast<const u32x4*>(qg);
                int s = 0;
#pragma unroll
                for (int k = 0; k < NB; k++)
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const uint32_t D = W[k][d];
                        if (BITS == 1) {
                            const u32x4 q0 = qv[d * 2], q1 = qv[d * 2 + 1];
#pragma unroll
                            for (int b = 0; b < 4; b++) s = __builtin_amdgcn_sdot4((int)((D >> b) & 0x01010101u), (int)q0[b], s, false);
#pragma unroll
                            for (int b = 0; b < 4; b++) s = __builtin_amdgcn_sdot4((int)((D >> (4 + b)) & 0x01010101u), (int)q1[b], s, false);
                        } else {
                            const u32x4 q0 = qv[k * 4 + d];
#pragma unroll
                            for (int c = 0; c < 4; c++) s = __builtin_amdgcn_sdot4((int)((D >> (2 * c)) & 0x03030303u), (int)q0[c], s, false);
                        }
                    }
                I[t] = s - a.qBias * (int)qg[32];
            }
        }
        const int n = (G - it * LPR) < LPR ? (G - it * LPR) : LPR; /* groups of this step: uniform */
#pragma unroll
        for (int t = 0; t < TT; t++) {
            const float p = sw * (float)I[t]; /* exact: <= 8 + 14 significant bits */
            for (int j = 0; j < n; j++) acc[t] = acc[t] + __shfl(p, j, LPR);
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

int a8_matvec_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok) {
    A8Args a;
    a.w = reinterpret_cast<const u32x4*>(w->data);
    a.stepw = w->gama + w->ne0 + w->ne1 + (size_t)w->ne0 * w->ne1 / w->lGroup; /* gama_T(STEP), GTensor.cpp:456-510 */
    a.q = q, a.stepx = step, a.y = y, a.bias = bias, a.residual = residual;
    a.M = w->ne0, a.K = w->ne1, a.G = p.n_groups, a.nTok = nTok, a.lpr_log2 = p.lpr_log2, a.iters = p.iters, a.qBias = p.qbias;
    if (p.bits == 1 && p.tok_tile == 1) return a8_go(a8_kernel<1, 1>, p, st, a);
    if (p.bits == 1) return a8_go(a8_kernel<1, A8_TOK_TILE>, p, st, a);
    if (p.tok_tile == 1) return a8_go(a8_kernel<2, 1>, p, st, a);
    return a8_go(a8_kernel<2, A8_TOK_TILE>, p, st, a);
}

}  // namespace kf
