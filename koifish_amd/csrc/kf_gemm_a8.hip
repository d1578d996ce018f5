// kf_gemm_a8.hip -- kf_linear_a8_tiles: 1-bit / ternary weights times int8 activations of a token batch on v_mfma_i32_16x16x64_i8 (include/kf_abi.h "int8 activations";
// the launch is kf::a8_plan's tile route, kf_a8.h).  The arithmetic is kf_linear_a8's (kf_gemv_a8.hip), bit for bit:
//   * a wave owns 16 output rows -- the A operand -- and NT tiles of 16 tokens -- the B operands; a 128-weight group is TWO MFMA steps of K = 64 into an int32x4 accumulator
//     that starts from zero, so I_g is that group's exact integer sum and nothing else.  No accumulator runs across a group boundary.
//   * the lane that holds output element (row, token) of the C tile (col = lane & 15 = the token, row = 4 * (lane >> 4) + register) folds I_g into ITS fp32 chain
//     acc = acc + step_w[g] * I_g, groups ascending (A8_ORDER_CHAIN): one lane, one chain per output element, no split-K, no hand-over between lanes or waves.
//   * operands: inside a group any pairing of codes and activations gives the same I_g, so all that matters is that lane quarter h = lane >> 4 of A and of B carry the SAME
//     16 elements in the same order in each step.  Quarter h, step s takes the staged dwords 8h + 4s .. 8h + 4s + 3 of the group (staged order: a8_elem, the order the masks
//     (D >> s) & 0x01010101 and (D >> 2c) & 0x03030303 leave codes in -- kf_gemv_a8.hip): of a 1-bit block that is dword h, bits 4s .. 4s + 3; of a 2-bit group block
//     h >> 1, dword 2 (h & 1) + s, codes 0 .. 3.  A lane loads 4 (1-bit) or 8 (2-bit) bytes of weights per group and makes its eight operand dwords with a shift and a mask each.
//   * codes are multiplied as they are stored; the ternary bias comes off as qBias * sum(q of the group), formed once at staging (exact, as kf_gemv_a8.hip).
//   * activations: staged per chunk of at most A8T_CHUNK groups for every token of the workgroup's tile, 36 dwords per (group, token) -- 32 staged dwords, the sum, pad --
//     so that the 16 tokens of a B read sit on distinct banks.  A thread stages whole groups: eight 16-byte loads, 4 x 4 byte transposes on v_perm_b32.  The loads of
//     chunk c + 1 (activations and the lane's weight dwords) are issued before chunk c is multiplied and land in registers meanwhile.
#include "kf_a8.h"

namespace kf {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct A8TArgs {
    const uint32_t* w;
    const uint16_t* stepw;
    const int8_t* q;
    const float* stepx;
    uint16_t* y;
    const uint16_t* bias;
    const uint16_t* residual;
    int M, K, G, nTok, chunk, qBias, q_al;
};

// o[v] = { byte 3 - v of s0, of s1, of s2, of s3 } (bytes 0 .. 3)
__device__ __forceinline__ void a8t_tr4(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t* o) {
    const uint32_t ah = __builtin_amdgcn_perm(s1, s0, 0x06020703u), bh = __builtin_amdgcn_perm(s3, s2, 0x06020703u); /* {s0.3, s1.3, s0.2, s1.2} */
    const uint32_t al = __builtin_amdgcn_perm(s1, s0, 0x04000501u), bl = __builtin_amdgcn_perm(s3, s2, 0x04000501u); /* {s0.1, s1.1, s0.0, s1.0} */
    o[0] = __builtin_amdgcn_perm(bh, ah, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(bh, ah, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(bl, al, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(bl, al, 0x07060302u);
}

template <int BITS, int NT>
__global__ void __launch_bounds__(A8T_THREADS) a8_tiles_kernel(A8TArgs a) {
    constexpr int TT = NT * A8T_TOK_PER_MFMA;
    constexpr int U = (TT * A8T_CHUNK + A8T_THREADS - 1) / A8T_THREADS; /* (group, token) units a thread stages per chunk */
    constexpr int WDW = BITS;                                           /* weight dwords a lane loads per group */
    extern __shared__ __align__(16) uint32_t lds[]; /* qs [chunk][TT][A8_GDW], then sws [A8T_ROW_TILE][chunk] fp32 */
    uint32_t* qs = lds;
    float* sws = reinterpret_cast<float*>(lds + a.chunk * TT * A8_GDW);
    const int G = a.G, tok0 = blockIdx.y * TT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4, c16 = lane & 15;
    const long wg_row0 = (long)blockIdx.x * A8T_ROW_TILE;
    const long arow = wg_row0 + wave * A8T_ROWS_PER_WAVE + c16; /* the row this lane carries in the A operand */
    const long arow_c = arow < a.M ? arow : a.M - 1;            /* rows past M: a valid row's weights, never stored */
    const uint32_t* wl = a.w + (size_t)arow_c * G * (4 * BITS) + (BITS == 1 ? h : (h >> 1) * 4 + (h & 1) * 2);

    float acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[t][r] = 0.0f;

    // one chunk ahead, in registers: the raw activation bytes of this thread's units and the lane's weight dwords -- in flight while the chunk before is multiplied
    u32x4 pre[U][8];
    uint32_t Wn[A8T_CHUNK][WDW];
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
        for (int gl = 0; gl < A8T_CHUNK; gl++) {
            const int g = g0 + gl < G ? g0 + gl : G - 1;
#pragma unroll
            for (int k = 0; k < WDW; k++) Wn[gl][k] = wl[(size_t)g * (4 * BITS) + k];
        }
    };
    fetch(0);

    for (int g0 = 0; g0 < G; g0 += a.chunk) {
        const int gc = (G - g0) < a.chunk ? (G - g0) : a.chunk;
        uint32_t W[A8T_CHUNK][WDW];
#pragma unroll
        for (int gl = 0; gl < A8T_CHUNK; gl++)
#pragma unroll
            for (int k = 0; k < WDW; k++) W[gl][k] = Wn[gl][k];
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
                if (BITS == 1) {
#pragma unroll
                    for (int d = 0; d < 4; d++)
#pragma unroll
                        for (int v = 0; v < 2; v++) {
                            const uint32_t* c = src + (3 - d) * 8;
                            a8t_tr4(c[7 - v], c[5 - v], c[3 - v], c[1 - v], o + d * 8 + v * 4);
                        }
                } else {
#pragma unroll
                    for (int bd = 0; bd < 8; bd++) { /* bd = block * 4 + dword */
                        const uint32_t* c = src + (bd >> 2) * 16 + (3 - (bd & 3)) * 4;
                        a8t_tr4(c[3], c[2], c[1], c[0], o + bd * 4);
                    }
                }
            } else { /* q rows not 16-byte aligned: the byte gather of kf_gemv_a8.hip, in place */
                const int gl = u / TT, t = u - gl * TT;
                const bool live = tok0 + t < a.nTok;
                const uint8_t* qb = reinterpret_cast<const uint8_t*>(a.q) + (live ? (size_t)(tok0 + t) * a.K + (size_t)(g0 + gl) * A8_GROUP : 0);
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    uint32_t v = 0;
                    if (live) {
#pragma unroll
                        for (int b = 0; b < 4; b++) v |= (uint32_t)qb[a8_elem<BITS>(j, b)] << (8 * b);
                    }
                    o[j] = v;
                    s = __builtin_amdgcn_sdot4(0x01010101, (int)v, s, false);
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) reinterpret_cast<u32x4*>(dst)[k] = u32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
            dst[32] = (uint32_t)(a.qBias * s); /* what comes off every I_g of this (token, group) */
        }
        for (int i = threadIdx.x; i < A8T_ROW_TILE * gc; i += A8T_THREADS) {
            const int r = i / gc, gl = i - r * gc;
            const long row = wg_row0 + r < a.M ? wg_row0 + r : a.M - 1;
            sws[r * a.chunk + gl] = bf2f(a.stepw[(size_t)row * G + g0 + gl]);
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
                for (int i = 0; i < 4; i++) {
                    if constexpr (BITS == 1) A[s][i] = (int)((W[gl][0] >> (4 * s + i)) & 0x01010101u);
                    else A[s][i] = (int)((W[gl][s] >> (2 * i)) & 0x03030303u);
                }
            float sw[4];
#pragma unroll
            for (int r = 0; r < 4; r++) sw[r] = sws[(wave * A8T_ROWS_PER_WAVE + 4 * h + r) * a.chunk + gl];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const uint32_t* qg = qs + (size_t)(gl * TT + t * A8T_TOK_PER_MFMA + c16) * A8_GDW;
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(qg + 8 * h), b1 = *reinterpret_cast<const u32x4*>(qg + 8 * h + 4);
                i32x4 I = {0, 0, 0, 0};
                I = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], __builtin_bit_cast(i32x4, b0), I, 0, 0, 0);
                I = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], __builtin_bit_cast(i32x4, b1), I, 0, 0, 0);
                const int bias_q = a.qBias ? (int)qg[32] : 0; /* uniform: 1-bit storage has no bias */
#pragma unroll
                for (int r = 0; r < 4; r++) acc[t][r] = fmaf(sw[r], (float)(I[r] - bias_q), acc[t][r]); /* the product is exact (<= 8 + 14 significant bits): the bits of acc + sw * I */
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

int a8_tiles_run(hipStream_t st, const A8Plan& p, const kf_weight* w, const int8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok) {
    A8TArgs a;
    a.w = reinterpret_cast<const uint32_t*>(w->data);
    a.stepw = w->gama + w->ne0 + w->ne1 + (size_t)w->ne0 * w->ne1 / w->lGroup; /* gama_T(STEP), GTensor.cpp:456-510 */
    a.q = q, a.stepx = step, a.y = y, a.bias = bias, a.residual = residual;
    a.M = w->ne0, a.K = w->ne1, a.G = p.n_groups, a.nTok = nTok, a.chunk = p.chunk, a.qBias = p.qbias;
    a.q_al = ((uintptr_t)q & 15) == 0; /* K is a multiple of 128: every row and group then starts 16-byte aligned */
    if (p.bits == 1) {
        if (p.mfma_tok == 1) return a8_go(a8_tiles_kernel<1, 1>, p, st, a);
        if (p.mfma_tok == 2) return a8_go(a8_tiles_kernel<1, 2>, p, st, a);
        return a8_go(a8_tiles_kernel<1, 4>, p, st, a);
    }
    if (p.mfma_tok == 1) return a8_go(a8_tiles_kernel<2, 1>, p, st, a);
    if (p.mfma_tok == 2) return a8_go(a8_tiles_kernel<2, 2>, p, st, a);
    return a8_go(a8_tiles_kernel<2, 4>, p, st, a);
}

}  // namespace kf
