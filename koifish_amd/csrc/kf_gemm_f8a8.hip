// kf_gemm_f8a8.hip -- kf_linear_f8a8: per-token e4m3 activation codes times the stored e5m2 bytes of a KF_F8E5M2 weight on v_mfma_f32_16x16x128_f8f6f4 (A format fp8,
// B format bf8), fp32 accumulation (include/kf_abi.h "fp8 activations for f8e5m2 layers"; the launch is kf::f8a8_plan's, kf_f8a8.h).
//   * both operands are K-contiguous bytes as they lie in memory: no unpack, no transpose.  A 128-byte step of a row is one LDS row; lane l of the MFMA holds row l % 16,
//     bytes 32 (l / 16) .. + 31 of it -- the A operand from a code row (a token), the B operand from a weight row -- so byte j of lane group g meets byte j of lane group g:
//     element k of the row sits in slot k % 128 of step k / 128, always.
//   * C tile: lane l holds weight row l % 16 and tokens 4 (l / 16) .. + 3: the 16 lanes of a group store 16 consecutive bf16 of one token's output row.
//   * one fp32 accumulator per output element, fed by the row's steps in ascending order (F8A8_ORDER_CHAIN): one lane, one chain, no split-K, no hand-over.
//   * staging: global_load_lds_dwordx4, eight 128-byte rows per wave instruction, for weight rows and code rows alike; the 16-byte chunk c of tile row r lands at
//     position c ^ ((r >> 1) & 7) (the swizzle is applied to the SOURCE address: the instruction writes lane * 16 bytes), so the 16 rows x one chunk of a ds_read_b128
//     touch all 64 banks once, for both reads of a lane's pair.  F8A8_STAGES buffers: step s + 1 is in flight while step s is multiplied; a counted wait and one
//     barrier per step (kf_gemm3_tile.h's loop).
//   * tails: tile rows past M and tokens past nTok re-read the last valid row (never past the end of either operand) and store nothing.  A half last step (K % 128 ==
//     64): the lanes of chunks 4 .. 7 load nothing and write zeros to their LDS slots instead -- zeros are exact in the MFMA.
#include "kf_a8.h"
#include "kf_f8a8.h"

namespace kf {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f8a8_f32x4 __attribute__((ext_vector_type(4)));

struct F8A8Args {
    const uint8_t* w;
    const uint8_t* q;
    const float* stepx;
    uint16_t* y;
    const uint16_t* bias;
    const uint16_t* residual;
    int M, K, nTok, n_steps, half_tail;
};

// instruction j of a tile (rows 8 j .. 8 j + 7): this lane's source -- row r = 8 j + lane / 8, position p = lane % 8 receives chunk p ^ ((r >> 1) & 7)
__device__ __forceinline__ const uint8_t* f8a8_src(const uint8_t* base, int K, int row0, int nrows, int j, int lane, int* chunk) {
    const int r = j * 8 + (lane >> 3), c = (lane & 7) ^ ((r >> 1) & 7);
    int gr = row0 + r;
    gr = gr < nrows ? gr : nrows - 1;
    *chunk = c;
    return base + (size_t)gr * K + c * 16;
}
// the 32 operand bytes of lane group g from tile row `row`: chunks 2 g and 2 g + 1
__device__ __forceinline__ i32x8 f8a8_frag(const unsigned char* tile, int row, int g) {
    const int f = (row >> 1) & 7;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + row * F8A8_STEP + (((2 * g) ^ f) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(tile + row * F8A8_STEP + (((2 * g + 1) ^ f) << 4));
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

template <int FORM>
__global__ void __launch_bounds__(F8A8_THREADS) f8a8_kernel(F8A8Args a) {
    constexpr F8A8Form C = F8A8_FORMS[FORM];
    constexpr int WT = C.wt, MT = C.mt, NT = C.nt, BT = C.tok_tile;
    constexpr int STAGE = f8a8_stage_bytes(FORM), NIW = F8A8_ROW_TILE / 8, NIQ = BT / 8; /* wave instructions per weight tile and per code tile */
    constexpr int LW = NIW / 4, LQ = (NIQ + 3) / 4;                                       /* ... per wave */
    static_assert(C.wr * C.wt == 4 && C.wr * MT * 16 == F8A8_ROW_TILE && WT * NT * 16 == BT, "four waves cover the tile");
    extern __shared__ __align__(16) unsigned char smem[]; /* F8A8_STAGES x { weight tile [128][128], code tile [BT][128] } */
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid / WT, wn = wid % WT, r16 = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * F8A8_ROW_TILE, tok0 = blockIdx.y * BT;

    const uint8_t *pw[LW], *pq[LQ];
    int cw[LW], cq[LQ];
#pragma unroll
    for (int i = 0; i < LW; i++) pw[i] = f8a8_src(a.w, a.K, row0, a.M, wid * LW + i, lane, &cw[i]);
#pragma unroll
    for (int i = 0; i < LQ; i++) pq[i] = f8a8_src(a.q, a.K, tok0, a.nTok, (wid * LQ + i) % NIQ, lane, &cq[i]);
    auto load = [&](const uint8_t* src, unsigned char* dst, int chunk, bool half) {
        if (half && chunk >= 4) *reinterpret_cast<u32x4*>(dst + lane * 16) = u32x4{0, 0, 0, 0};
        else __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    };
    auto stage = [&](int s, int b) {
        unsigned char* bw = smem + b * STAGE;
        unsigned char* bq = bw + F8A8_ROW_TILE * F8A8_STEP;
        const bool half = a.half_tail && s == a.n_steps - 1;
        const size_t k0 = (size_t)s * F8A8_STEP;
#pragma unroll
        for (int i = 0; i < LW; i++) load(pw[i] + k0, bw + (wid * LW + i) * 1024, cw[i], half);
#pragma unroll
        for (int i = 0; i < LQ; i++)
            if (wid * LQ + i < NIQ) load(pq[i] + k0, bq + (wid * LQ + i) * 1024, cq[i], half); /* uniform per wave: a narrow code tile has fewer instructions than waves */
    };

    f8a8_f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f8a8_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    stage(0, 0);
    for (int s = 0; s < a.n_steps; s++) {
        const int cur = s % F8A8_STAGES;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier(); /* step s has landed for every wave, and every wave is done reading the buffer of step s - 1: the next loads overwrite that one */
        if (s + 1 < a.n_steps) stage(s + 1, (s + 1) % F8A8_STAGES);
        const unsigned char* bw = smem + cur * STAGE;
        const unsigned char* bq = bw + F8A8_ROW_TILE * F8A8_STEP;
        i32x8 qa[NT], wb[MT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) qa[nt] = f8a8_frag(bq, (wn * NT + nt) * 16 + r16, g);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) wb[mt] = f8a8_frag(bw, (wm * MT + mt) * 16 + r16, g);
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
                acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qa[nt], wb[mt], acc[mt][nt], /* A: fp8 */ 0, /* B: bf8 */ 1, 0, 0, 0, 0);
    }

    // C[i][j]: i the A row = token 4 g + r of the tile, j the B row = weight row r16
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int tok = tok0 + (wn * NT + nt) * 16 + 4 * g + r;
            if (tok >= a.nTok) continue;
            const float sx = a.stepx[tok];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const long row = row0 + (wm * MT + mt) * 16 + r16;
                if (row < a.M) a8_store(a.y, a.bias, a.residual, sx, acc[mt][nt][r], row, (size_t)tok * a.M + row);
            }
        }
}

template <int FORM>
static int f8a8_go(hipStream_t st, const F8A8Plan& p, const F8A8Args& a) {
    hipError_t e = hipSuccess;
    if (p.lds > 64 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void*>(f8a8_kernel<FORM>), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
    if (e == hipSuccess) hipLaunchKernelGGL(f8a8_kernel<FORM>, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, a);
    return (e == hipSuccess && hipGetLastError() == hipSuccess) ? KF_OK : KF_HIP_CHECK;
}

int f8a8_run(hipStream_t st, const F8A8Plan& p, const kf_weight* w, const uint8_t* q, const float* step, uint16_t* y, const uint16_t* bias, const uint16_t* residual, int nTok) {
    if (p.status != KF_OK) return p.status;
    F8A8Args a;
    a.w = reinterpret_cast<const uint8_t*>(w->data), a.q = q, a.stepx = step, a.y = y, a.bias = bias, a.residual = residual;
    a.M = w->ne0, a.K = w->ne1, a.nTok = nTok, a.n_steps = p.n_steps, a.half_tail = p.half_tail;
    switch (p.form) {
        case F8A8_TOK16: return f8a8_go<F8A8_TOK16>(st, p, a);
        case F8A8_TOK32: return f8a8_go<F8A8_TOK32>(st, p, a);
        case F8A8_TOK64: return f8a8_go<F8A8_TOK64>(st, p, a);
        case F8A8_WIDE: return f8a8_go<F8A8_WIDE>(st, p, a);
    }
    return KF_INVALID_ARGS; /* not a plan of f8a8_plan */
}

}  // namespace kf
