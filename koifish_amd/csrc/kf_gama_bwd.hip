// kf_gama_bwd.hip -- the gradient of a group-quantised weight's (zero, step) pairs, the reference's "train_target": "gama" branch of SLP::Back (NeuronFuse.cu:538-549 ->
// GamaBack_v0 -> CU_GamaBack_2, kernel/quantizer.cu:66-94), without the weight gradient ever being written.  With w = step (q - qBias) - zero per 128-column group g of row r:
//   dW[r, c]  = sum_i deltaIn[i, r] inp[i, c]                        (the weight-gradient GEMM of kf_linear_backward)
//   g_zero[g] = - sum_{c in g} dW[r, c],      g_step[g] = + sum_{c in g} dW[r, c] (q[r, c] - qBias)
// The reference runs one thread per group over nSample x 128 products of a dequantised copy; here:
//   gama_bwd_kernel  the k-major tiles and k-loop of kf_gemm3.hip (kf_gemm3_tile.h: A = inp [n][IC], B = deltaIn [n][OC], contraction over the token rows) over
//                    [IC tile x OC tile x slab of n].  The epilogue keeps the accumulators in registers: a lane holds, per OC row, 4 consecutive columns of every
//                    16-column block of its wave's IC extent; it multiplies them with the integers q - qBias read straight from the Packed128 stream (never a dequantised
//                    weight), adds its columns, the row's four lanes meet by two row swaps, the waves of a group through LDS in wave order.  Two fp32 numbers per group
//                    leave the workgroup, into the slab's [2][nGroup] partials.  Rows >= OC and columns >= IC store nothing and read nothing.
//   gama_fin_kernel  a thread per gGama element: the slabs in index order, then gGama = bf16(gGama + scale (-/+) S).
// Every sum's order is a function of the shape alone (kf_gama_plan.h): no atomics, every partial of every slab is written before it is read.
#include <string.h>

#include "kf_gama_plan.h"
#include "kf_gemm3_tile.h"

namespace kf {

struct GamaArgs {
    const unsigned char* packed; /* the weight's Packed128 stream, [OC][IC] row-major */
    float* part;                 /* [S][2][nGroup] */
    int fmt, qBias;              /* FMT_Q4 / FMT_Q2 / FMT_Q1 */
    int OC, IC, gpr, nGroup;     /* groups per row */
    int nbx, ntiles, S, nkt;
};

// q - qBias of columns c .. c + 3 (c a multiple of 4) of row r, as floats.  Packed128 (PackedQ.hpp:99-239; kf_gemv_blocks.h): a 16-byte block holds 32 / 64 / 128 elements,
// dword 3 the first ones, element 0 in its top bits
__device__ __forceinline__ f32x4 gama_q4(const GamaArgs& g, int r, int c) {
    const size_t e = (size_t)r * g.IC + c;
    const uint32_t* blk = reinterpret_cast<const uint32_t*>(g.packed);
    int q[4];
    if (g.fmt == FMT_Q4) { /* 32 per block, 8 per dword, element 0 in bits 28..31 */
        const uint32_t D = blk[(e >> 5) * 4 + 3 - ((e & 31) >> 3)];
        const uint32_t v = (D >> (16 - 4 * (int)(e & 7))) & 0xffffu; /* e & 7 is 0 or 4: the upper or the lower half */
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = (int)((v >> (12 - 4 * j)) & 15u);
    } else if (g.fmt == FMT_Q2) { /* 64 per block, 16 per dword, element 0 in bits 30..31 */
        const uint32_t D = blk[(e >> 6) * 4 + 3 - ((e & 63) >> 4)];
        const int k = (int)(e & 15);
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = (int)((D >> (30 - 2 * (k + j))) & 3u);
    } else { /* FMT_Q1: 128 per block, 32 per dword, element 0 in bit 31 */
        const uint32_t D = blk[(e >> 7) * 4 + 3 - ((e & 127) >> 5)];
        const int k = (int)(e & 31);
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = (int)((D >> (31 - (k + j))) & 1u);
    }
    return f32x4{(float)(q[0] - g.qBias), (float)(q[1] - g.qBias), (float)(q[2] - g.qBias), (float)(q[3] - g.qBias)};
}

template <class C>
__global__ void __launch_bounds__(C::NTH, C::WGS_PER_CU * C::NW / 4) gama_bwd_kernel(const GemmArgs a, const GamaArgs g) {
    static_assert(C::BM % GAMA_GROUP == 0 && (16 * C::MT == GAMA_GROUP || 32 * C::MT == GAMA_GROUP), "a tile's IC extent is whole groups: a wave holds a group or half of one");
    constexpr int GPT = C::BM / GAMA_GROUP, WPG = 2 / GPT; /* groups per tile row; waves (along IC) per group */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int slab = blockIdx.x / g.ntiles, tile = g3_remap(blockIdx.x % g.ntiles, g.ntiles);
    const int bx = tile % g.nbx, by = tile / g.nbx;
    const int m0 = bx * C::BM, t0 = by * C::BN; /* IC columns, OC rows */
    const int kt0 = (int)((long long)g.nkt * slab / g.S), kt1 = (int)((long long)g.nkt * (slab + 1) / g.S);
    f32x4 acc[C::MT][C::NT];
#pragma unroll
    for (int i = 0; i < C::MT; i++)
#pragma unroll
        for (int j = 0; j < C::NT; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    g3_mainloop<true, true, G3_BK, C>(a, m0, t0, kt0, kt1, acc, smem_raw, wid, lane); /* ends with a barrier: the stage buffers are free */
    // lane (r16, q4) of wave (wm, wn): columns m0 + wm 16 MT + 16 mt + 4 q4 + j of OC row t0 + wn 16 NT + 16 nt + r16
    const int wm = wid / C::WN, wn = wid % C::WN, r16 = lane & 15, q4 = lane >> 4;
    const int cbase = m0 + wm * (16 * C::MT) + 4 * q4;
    float2* red = reinterpret_cast<float2*>(smem_raw); /* [2 wm][BN] {sum dW, sum dW (q - qBias)} */
#pragma unroll
    for (int nt = 0; nt < C::NT; nt++) {
        const int col = wn * (16 * C::NT) + nt * 16 + r16, r = t0 + col;
        float sz = 0.0f, ss = 0.0f;
        if (r < g.OC && cbase < g.IC) { /* IC is whole groups: a wave's extent lies inside the matrix or outside it */
#pragma unroll
            for (int mt = 0; mt < C::MT; mt++) {
                const f32x4 qi = gama_q4(g, r, cbase + mt * 16), v = acc[mt][nt];
                sz += (v.x + v.y) + (v.z + v.w);
                ss += (v.x * qi.x + v.y * qi.y) + (v.z * qi.z + v.w * qi.w);
            }
        }
        sz += __shfl_xor(sz, 16), ss += __shfl_xor(ss, 16);
        sz += __shfl_xor(sz, 32), ss += __shfl_xor(ss, 32);
        if (q4 == 0) red[wm * C::BN + col] = float2{sz, ss};
    }
    __syncthreads();
    for (int t = tid; t < C::BN * GPT; t += C::NTH) {
        const int col = t % C::BN, gi = t / C::BN, r = t0 + col, c0 = m0 + gi * GAMA_GROUP;
        if (r >= g.OC || c0 >= g.IC) continue;
        float2 s = red[(gi * WPG) * C::BN + col];
        if (WPG == 2) {
            const float2 o = red[(gi * WPG + 1) * C::BN + col];
            s.x += o.x, s.y += o.y;
        }
        const size_t gidx = (size_t)r * g.gpr + c0 / GAMA_GROUP;
        float* ps = g.part + (size_t)slab * 2 * g.nGroup;
        ps[gidx] = s.x, ps[(size_t)g.nGroup + gidx] = s.y;
    }
}

// element i of gGama = [ZERO nGroup][STEP nGroup]: the slabs' partials in index order, the zero gradients negated
__global__ void __launch_bounds__(GAMA_FIN_BLOCK) gama_fin_kernel(const float* __restrict__ part, int S, int nGroup, float scale, uint16_t* __restrict__ gGama) {
    const size_t i = (size_t)blockIdx.x * GAMA_FIN_BLOCK + threadIdx.x, n2 = 2 * (size_t)nGroup;
    if (i >= n2) return;
    float s = 0.0f;
    for (int k = 0; k < S; k++) s += part[(size_t)k * n2 + i];
    const float sg = i < (size_t)nGroup ? -s : s;
    gGama[i] = f2bf(bf2f(gGama[i]) + scale * sg);
}

template <class C>
static int gama_run_c(hipStream_t st, const GamaPlan& p, const GemmArgs& a, const GamaArgs& g) {
    constexpr int SMEM = 2 * C::STAGE;
    static_assert(2 * C::BN * 8 <= SMEM, "the epilogue's exchange fits the stage buffers");
    static int attr_set = 0;
    if (!attr_set && SMEM > 64 * 1024) {
        if (hipFuncSetAttribute((const void*)gama_bwd_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM) != hipSuccess) return KF_HIP_CHECK;
        attr_set = 1;
    }
    hipLaunchKernelGGL((gama_bwd_kernel<C>), dim3(p.gx), dim3(C::NTH), SMEM, st, a, g);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

int gama_backward_launch(hipStream_t st, const GamaPlan& p, const unsigned char* packed, int fmt, int qBias, int OC, int IC, const uint16_t* deltaIn, const uint16_t* inp, int n,
                         uint16_t* gGama, float scale, float* scratch) {
    GemmArgs a; /* the k-major operands as gemm3_km_launch hands them to the k-loop: A = inp [n][IC], B = deltaIn [n][OC] */
    memset(&a, 0, sizeof(a));
    a.w = reinterpret_cast<const unsigned char*>(inp), a.ldr = IC, a.M = IC, a.K = n, a.x = deltaIn, a.ldx = OC, a.n = OC;
    GamaArgs g;
    g.packed = packed, g.part = scratch, g.fmt = fmt, g.qBias = qBias, g.OC = OC, g.IC = IC, g.gpr = IC / GAMA_GROUP, g.nGroup = (int)((long long)OC * IC / GAMA_GROUP);
    g.nbx = p.nbx, g.ntiles = p.nbx * p.nby, g.S = p.S, g.nkt = n / G3_BK;
    const int rc = p.form == G3_BIG ? gama_run_c<G3Big>(st, p, a, g) : gama_run_c<G3Small>(st, p, a, g);
    if (rc != KF_OK) return rc;
    hipLaunchKernelGGL(gama_fin_kernel, dim3((unsigned)p.fin_gx), dim3(GAMA_FIN_BLOCK), 0, st, scratch, p.S, g.nGroup, scale, gGama);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
