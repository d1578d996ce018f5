// kf_gemm_w4a8.hip -- kf_linear_w4a8_tiles: 4-bit group weights times int8 activations of a token batch on v_mfma_i32_16x16x64_i8 (include/kf_abi.h "int8 activations
// for 4-bit layers"; the launch is kf::a8_plan's tile route, kf_a8.h).  The arithmetic is kf_linear_w4a8's (kf_gemv_w4a8.hip), bit for bit; the shape is kf_gemm_a8.hip's:
//   * a wave owns 16 output rows -- the A operand -- and NT tiles of 16 tokens -- the B operands; a 128-weight group is TWO MFMA steps of K = 64 into an int32x4 accumulator
//     that starts from zero, so it holds that group's exact sum of code * q and nothing else.  No accumulator runs across a group boundary.
//   * the lane that holds output element (row, token) of the C tile (col = lane & 15 = the token, row = 4 * (lane >> 4) + register) takes qBias * S_g off, computes
//     p = STEP * I_g (one rounding), z = ZERO * S_g (exact), c = p - z and folds c into ITS fp32 chain acc = acc + c, groups ascending (A8_ORDER_CHAIN): one lane, one
//     chain per output element, no split-K, no hand-over between lanes or waves.  Three instructions, never an fma (-ffp-contract=off, build.py).
//   * operands: inside a group any pairing of codes and activations gives the same I_g, so all that matters is that lane quarter h = lane >> 4 of A and of B carry the SAME
//     16 elements in the same order in each step.  Quarter h, step s takes the staged dwords 8h + 4s .. 8h + 4s + 3 of the group (staged order: w4a8_elem, the order the
//     masks (D >> 4c) & 0x0F0F0F0F leave codes in -- kf_gemv_w4a8.hip): that is block h of the group, dwords 2s and 2s + 1, low then high nibbles.  A lane loads the 16
//     bytes of its block per group and makes its eight operand dwords with a shift and a mask each.
//   * activations: staged per chunk of at most A8T_CHUNK groups for every token of the workgroup's tile, 36 dwords per (group, token) -- 32 staged dwords, the sum S_g, pad --
//     so that the 16 tokens of a B read sit on distinct banks.  A thread stages whole groups: eight 16-byte loads, two v_perm_b32 per eight elements.  The loads of chunk
//     c + 1 (activations and the lane's weight blocks) are issued before chunk c is multiplied and land in registers meanwhile.  STEP and ZERO of the workgroup's rows are
//     staged per chunk as fp32.
#include "kf_a8.h"

namespace kf {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct W4A8TArgs {
    const u32x4* w;
    const uint16_t* zerow;
    const uint16_t* stepw;
    const int8_t* q;
    const float* stepx;
    uint16_t* y;
    const uint16_t* bias;
    const uint16_t* residual;
    int M, K, G, nTok, chunk, qBias, q_al;
};

template <int NT>
__global__ void __launch_bounds__(A8T_THREADS) w4a8_tiles_kernel(W4A8TArgs a) {
    constexpr int TT = NT * A8T_TOK_PER_MFMA;
    constexpr int U = (TT * A8T_CHUNK + A8T_THREADS - 1) / A8T_THREADS; /* (group, token) units a thread stages per chunk */
    extern __shared__ __align__(16) uint32_t lds[]; /* qs [chunk][TT][A8_GDW], then sws, zws [A8T_ROW_TILE][chunk] fp32 */
    uint32_t* qs = lds;
    float* sws = reinterpret_cast<float*>(lds + a.chunk * TT * A8_GDW);
    float* zws = sws + A8T_ROW_TILE * a.chunk;
    const int G = a.G, tok0 = blockIdx.y * TT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4, c16 = lane & 15;
    const long wg_row0 = (long)blockIdx.x * A8T_ROW_TILE;
    const long arow = wg_row0 + wave * A8T_ROWS_PER_WAVE + c16; /* the row this lane carries in the A operand */
    const long arow_c = arow < a.M ? arow : a.M - 1;            /* rows past M: a valid row's weights, never stored */
    const u32x4* wl = a.w + (size_t)arow_c * G * W4A8_BLOCKS + h;

    float acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[t][r] = 0.0f;

    // one chunk ahead, in registers: the raw activation bytes of this thread's units and the lane's weight blocks -- in flight while the chunk before is multiplied
    u32x4 pre[U][8];
    u32x4 Wn[A8T_CHUNK];
    auto fetch = [&](int g0) {
        const int gc = (G - g0) < a.chunk ? (G - g0) : a.chunk;
#pragma unroll
        for (int uu = 0; uu < U; uu++) {
            const int u = threadIdx.x + uu * A8T_THREADS, gl = u / TT, t = u - gl * TT;
            if (a.q_al && u < gc * TT && tok0 + t < a.nTok) {
                const u32x4* qr = reinterpret_cast<const u32x4*>(a.q + (size_t)(tok0 + t) * a.K + (size_t)(g0 + gl) * A8_GROUP);
#pragma unroll
                for (int k = 0; k < 8; k++) pre[uu][k] = qr[k];
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) pre[uu][k] = u32x4{0, 0, 0, 0}; /* token rows past nTok multiply zeros */
            }
        }
#pragma unroll
        for (int gl = 0; gl < A8T_CHUNK; gl++) Wn[gl] = gl < gc ? ld_nt(wl + (size_t)(g0 + gl) * W4A8_BLOCKS) : u32x4{0, 0, 0, 0}; /* uniform: a chunk's tail loads nothing */
    };
    fetch(0);

    for (int g0 = 0; g0 < G; g0 += a.chunk) {
        const int gc = (G - g0) < a.chunk ? (G - g0) : a.chunk;
        u32x4 W[A8T_CHUNK];
#pragma unroll
        for (int gl = 0; gl < A8T_CHUNK; gl++) W[gl] = Wn[gl];
        if (g0) __syncthreads(); /* the previous chunk's reads are done */
#pragma unroll
        for (int uu = 0; uu < U; uu++) {
            const int u = threadIdx.x + uu * A8T_THREADS;
            if (u >= gc * TT) continue;
            uint32_t* dst = qs + (size_t)u * A8_GDW; /* u = gl * TT + t */
            uint32_t o[32];
            int s = 0;
            if (a.q_al) {
                uint32_t src[32];
#pragma unroll
                for (int k = 0; k < 8; k++) src[4 * k] = pre[uu][k].x, src[4 * k + 1] = pre[uu][k].y, src[4 * k + 2] = pre[uu][k].z, src[4 * k + 3] = pre[uu][k].w;
#pragma unroll
                for (int k = 0; k < 32; k++) s = __builtin_amdgcn_sdot4(0x01010101, (int)src[k], s, false);
#pragma unroll
                for (int kd = 0; kd < 16; kd++) { /* kd = block * 4 + dword: elements 32 block + 8 (3 - dword) .. + 7 = source dwords lo, hi */
                    const uint32_t lo = src[(kd >> 2) * 8 + (3 - (kd & 3)) * 2], hi = src[(kd >> 2) * 8 + (3 - (kd & 3)) * 2 + 1];
                    o[2 * kd] = __builtin_amdgcn_perm(hi, lo, 0x01030507u);     /* low nibbles: elements 7, 5, 3, 1 */
                    o[2 * kd + 1] = __builtin_amdgcn_perm(hi, lo, 0x00020406u); /* high nibbles: elements 6, 4, 2, 0 */
                }
            } else { /* q rows not 16-byte aligned: the byte gather of kf_gemv_w4a8.hip, in place */
                const int gl = u / TT, t = u - gl * TT;
                const bool live = tok0 + t < a.nTok;
                const uint8_t* qb = reinterpret_cast<const uint8_t*>(a.q) + (live ? (size_t)(tok0 + t) * a.K + (size_t)(g0 + gl) * A8_GROUP : 0);
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    uint32_t v = 0;
                    if (live) {
#pragma unroll
                        for (int b = 0; b < 4; b++) v |= (uint32_t)qb[w4a8_elem(j, b)] << (8 * b);
                    }
                    o[j] = v;
                    s = __builtin_amdgcn_sdot4(0x01010101, (int)v, s, false);
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) reinterpret_cast<u32x4*>(dst)[k] = u32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
            dst[32] = (uint32_t)s; /* S_g of this (token, group) */
        }
        for (int i = threadIdx.x; i < A8T_ROW_TILE * gc; i += A8T_THREADS) {
            const int r = i / gc, gl = i - r * gc;
            const long row = wg_row0 + r < a.M ? wg_row0 + r : a.M - 1;
            const size_t gi = (size_t)row * G + g0 + gl;
            sws[r * a.chunk + gl] = bf2f(a.stepw[gi]);
            zws[r * a.chunk + gl] = bf2f(a.zerow[gi]);
        }
        __syncthreads();
        if (g0 + a.chunk < G) fetch(g0 + a.chunk);

#pragma unroll
        for (int gl = 0; gl < A8T_CHUNK; gl++) {
            if (gl >= gc) break; /* uniform */
            i32x4 A[2];
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int i = 0; i < 4; i++) A[s][i] = (int)((W[gl][2 * s + (i >> 1)] >> (4 * (i & 1))) & 0x0F0F0F0Fu);
            float sw[4], zw[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                sw[r] = sws[(wave * A8T_ROWS_PER_WAVE + 4 * h + r) * a.chunk + gl];
                zw[r] = zws[(wave * A8T_ROWS_PER_WAVE + 4 * h + r) * a.chunk + gl];
            }
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const uint32_t* qg = qs + (size_t)(gl * TT + t * A8T_TOK_PER_MFMA + c16) * A8_GDW;
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(qg + 8 * h), b1 = *reinterpret_cast<const u32x4*>(qg + 8 * h + 4);
                i32x4 I = {0, 0, 0, 0};
                I = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], __builtin_bit_cast(i32x4, b0), I, 0, 0, 0);
                I = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], __builtin_bit_cast(i32x4, b1), I, 0, 0, 0);
                const int S = (int)qg[32];
                const int bias_q = a.qBias * S;
                const float Sf = (float)S;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float p = sw[r] * (float)(I[r] - bias_q); /* one rounding */
                    const float z = zw[r] * Sf;                     /* exact: <= 8 + 14 significant bits */
                    const float c = p - z;
                    acc[t][r] = acc[t][r] + c;
                }
            }
        }
    }

    const long orow0 = wg_row0 + wave * A8T_ROWS_PER_WAVE + 4 * h;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int tok = tok0 + t * A8T_TOK_PER_MFMA + c16;
        if (tok >= a.nTok) continue;
        const float sx = a.stepx[tok];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const long row = orow0 + r;
            if (row >= a.M) break;
            a8_store(a.y, a.bias, a.residual, sx, acc[t][r], row, (size_t)tok * a.M + row);
        }
    }
}

int w4a8_tiles_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok) {
    W4A8TArgs a;
    a.w = reinterpret_cast<const u32x4*>(w->data);
    a.zerow = w->gama + w->ne0 + w->ne1;                     /* gama_T(ZERO), GTensor.cpp:456-510 */
    a.stepw = a.zerow + (size_t)w->ne0 * w->ne1 / w->lGroup; /* gama_T(STEP) */
    a.q = q, a.stepx = step, a.y = y, a.bias = bias, a.residual = residual;
    a.M = w->ne0, a.K = w->ne1, a.G = p.n_groups, a.nTok = nTok, a.chunk = p.chunk, a.qBias = p.qbias;
    a.q_al = ((uintptr_t)q & 15) == 0; /* K is a multiple of 128: every row and group then starts 16-byte aligned */
    if (p.mfma_tok == 1) return a8_go(w4a8_tiles_kernel<1>, p, st, a);
    if (p.mfma_tok == 2) return a8_go(w4a8_tiles_kernel<2>, p, st, a);
    return a8_go(w4a8_tiles_kernel<4>, p, st, a);
}

}  // namespace kf
