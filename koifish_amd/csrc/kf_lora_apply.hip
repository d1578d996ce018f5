// kf_lora_apply.hip -- a trained low-rank pair applied at inference (kf_lora_apply; the reference runs its LORA branch inside SLP::Forw on every forward,
// NeuronFuse.cu:286-302).  The arithmetic per row is kf_lora_forward's (kf_lora.hip):  ax = bf16(s x a^T),  y = bf16(y + s ax b^T)  on top of what the base product left
// in y.  Two forms (which one, and the launch geometry: kf::lora_apply_plan, kf_lora_plan.h):
//   lora_rows_tail_kernel  the tile form, n >= 2: lora_rows_kernel with a row bound.  Rows >= n of a LORA_TM-row tile load as zero and store nothing, neither y nor ax; a
//                          row < n gets the bits kf_lora_forward gives it (an MFMA output row depends on its own input row only).  ax may be NULL.
//   lora_vec_kernel        the vector form, n == 1: up to three adapters (q | k | v, gate | up) that share the input row x, one launch, no grid-wide dependency.  Every
//                          workgroup recomputes the r dot products of length IC (16-byte loads of a and x; a is L2-resident after the first workgroup), leaves them in
//                          LDS as bf16(s sum) and then owns LORA_VEC_ROWS output rows of one adapter.  The order of every sum is fixed (include/kf_abi.h states it):
//                            phase 1  rank j belongs to wave j % 16.  Lane l owns the 8-element chunks l, l + 64, ... of the contraction and adds their products to ONE
//                                     fp32 accumulator, chunks ascending, k ascending inside a chunk (fma; a product of two bf16 is exact in fp32).  The 64 lane sums
//                                     meet in a butterfly: v += shfl_xor(v, m) for m = 32, 16, 8, 4, 2, 1 (both partners add the same two numbers: every lane ends
//                                     with the same bits).
//                            phase 2  lane l of wave 0 owns output row l of the slice: one fp32 chain over j ascending (fma), then bf16(y + s sum).
// No atomics, no scratch memory.
#include "kf_gemm_common.h"
#include "kf_lora_plan.h"

namespace kf {

__device__ __forceinline__ bf16x8 lora_apply_zero_frag() { return __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u}); }

template <int R>
__global__ void __launch_bounds__(64 * LORA_ROW_WAVES) lora_rows_tail_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, const uint16_t* __restrict__ X,
                                                                            uint16_t* __restrict__ Y, uint16_t* __restrict__ Tg, int K, int M, float s, int n) {
    constexpr int JT = R / 16, KS = R >= 32 ? R / 32 : 1, TB = LORA_TM / 16, LDT = R + 8, NTH = 64 * LORA_ROW_WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* red = reinterpret_cast<float*>(smem_raw);                                                 /* [waves][TM][R] */
    uint16_t* ts = reinterpret_cast<uint16_t*>(smem_raw + LORA_ROW_WAVES * LORA_TM * R * 4);         /* [TM][LDT] */
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * LORA_TM;
    bool live[TB]; /* this lane's token row of block tb is one of the n */
#pragma unroll
    for (int tb = 0; tb < TB; tb++) live[tb] = row0 + tb * 16 + l16 < (size_t)n;
    // ---- T = bf16(s X A^T): wave w takes the chunks w, w + 8, ... of K
    f32x4 acc[TB][JT];
#pragma unroll
    for (int tb = 0; tb < TB; tb++)
#pragma unroll
        for (int jt = 0; jt < JT; jt++) acc[tb][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nch = K / LORA_KC;
    for (int ch = wid; ch < nch; ch += LORA_ROW_WAVES) {
#pragma unroll
        for (int kk = 0; kk < LORA_KC / 32; kk++) {
            const int k = ch * LORA_KC + kk * 32 + 8 * q;
            bf16x8 xf[TB], af[JT];
#pragma unroll
            for (int tb = 0; tb < TB; tb++) xf[tb] = live[tb] ? *reinterpret_cast<const bf16x8*>(X + (row0 + tb * 16 + l16) * K + k) : lora_apply_zero_frag();
#pragma unroll
            for (int jt = 0; jt < JT; jt++) af[jt] = *reinterpret_cast<const bf16x8*>(A + (size_t)(jt * 16 + l16) * K + k);
#pragma unroll
            for (int tb = 0; tb < TB; tb++)
#pragma unroll
                for (int jt = 0; jt < JT; jt++) acc[tb][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[tb], af[jt], acc[tb][jt], 0, 0, 0);
        }
    }
    // lane (l16, q): token rows tb 16 + 4 q + reg, rank column jt 16 + l16
#pragma unroll
    for (int tb = 0; tb < TB; tb++)
#pragma unroll
        for (int jt = 0; jt < JT; jt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) red[(wid * LORA_TM + tb * 16 + 4 * q + reg) * R + jt * 16 + l16] = acc[tb][jt][reg];
    __syncthreads();
    for (int i = tid; i < LORA_TM * R; i += NTH) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < LORA_ROW_WAVES; w++) v += red[w * LORA_TM * R + i];
        const uint16_t h = f2bf(s * v);
        const int tok = i / R, j = i % R;
        if (Tg && row0 + tok < (size_t)n) Tg[(row0 + tok) * R + j] = h;
        ts[tok * LDT + j] = h;
    }
    __syncthreads();
    // ---- Y += s T B^T, transposed: B's rows are the MFMA's rows, the tokens its columns.  Rank 16: the upper half of the K step is zero on both sides
    const bool pad = R == 16 && q >= 2;
    bf16x8 tf[TB][KS];
#pragma unroll
    for (int tb = 0; tb < TB; tb++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) tf[tb][ks] = pad ? lora_apply_zero_frag() : *reinterpret_cast<const bf16x8*>(ts + (tb * 16 + l16) * LDT + ks * 32 + 8 * q);
    const int nblk = M / 32;
    for (int blk = wid; blk < nblk; blk += LORA_ROW_WAVES) {
        const int m0 = blk * 32;
        f32x4 d[2][TB];
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
#pragma unroll
            for (int tb = 0; tb < TB; tb++) d[tt][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const size_t m = (size_t)m0 + 8 * (l16 >> 2) + 4 * tt + (l16 & 3); /* MFMA row 4 q + reg of tile tt is column m0 + 8 q + 4 tt + reg */
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const bf16x8 bf = pad ? lora_apply_zero_frag() : *reinterpret_cast<const bf16x8*>(B + m * R + ks * 32 + 8 * q);
#pragma unroll
                for (int tb = 0; tb < TB; tb++) d[tt][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, tf[tb][ks], d[tt][tb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tb = 0; tb < TB; tb++) {
            if (!live[tb]) continue; /* after the MFMAs: they run with every lane */
            u32x4* yp = reinterpret_cast<u32x4*>(Y + (row0 + tb * 16 + l16) * M + m0 + 8 * q);
            const u32x4 old = *yp;
            u32x4 out;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t w2 = old[j];
                const int e0 = 2 * j, e1 = 2 * j + 1;
                const float v0 = bf2f((uint16_t)(w2 & 0xffffu)) + s * d[e0 >> 2][tb][e0 & 3];
                const float v1 = bf2f((uint16_t)(w2 >> 16)) + s * d[e1 >> 2][tb][e1 & 3];
                out[j] = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
            }
            *yp = out;
        }
    }
}

// adapter i's workgroups are [wg_end[i - 1], wg_end[i]) (an unused slot repeats the end before it)
struct LoraVecArgs {
    const uint16_t* a[LORA_APPLY_MAX];
    const uint16_t* b[LORA_APPLY_MAX];
    uint16_t* y[LORA_APPLY_MAX];
    int wg_end[LORA_APPLY_MAX];
    const uint16_t* x;
    int IC;
    float s;
};

template <int R>
__global__ void __launch_bounds__(64 * LORA_VEC_WAVES) lora_vec_kernel(const LoraVecArgs g) {
    constexpr int JW = R / LORA_VEC_WAVES; /* ranks per wave */
    __shared__ __attribute__((aligned(16))) uint16_t ts[R];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wg = (int)blockIdx.x;
    const int i = wg < g.wg_end[0] ? 0 : wg < g.wg_end[1] ? 1 : 2, wg0 = i ? g.wg_end[i - 1] : 0;
    const uint16_t* __restrict__ A = g.a[i];
    const uint16_t* __restrict__ B = g.b[i];
    const uint16_t* __restrict__ X = g.x;
    uint16_t* __restrict__ Y = g.y[i];
    const int IC = g.IC;
    // ---- phase 1: ts[j] = bf16(s x . a[j]), rank j = wid + 16 jj
    float acc[JW];
#pragma unroll
    for (int jj = 0; jj < JW; jj++) acc[jj] = 0.0f;
#pragma unroll 3
    for (int c = lane; c < IC / 8; c += 64) { /* unrolled: the loads of three chunks are in flight together */
        const u32x4 xv = *reinterpret_cast<const u32x4*>(X + 8 * c);
#pragma unroll
        for (int jj = 0; jj < JW; jj++) {
            const u32x4 av = *reinterpret_cast<const u32x4*>(A + (size_t)(wid + LORA_VEC_WAVES * jj) * IC + 8 * c);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                acc[jj] = __builtin_fmaf(__uint_as_float(xv[e] << 16), __uint_as_float(av[e] << 16), acc[jj]);
                acc[jj] = __builtin_fmaf(__uint_as_float(xv[e] & 0xffff0000u), __uint_as_float(av[e] & 0xffff0000u), acc[jj]);
            }
        }
    }
#pragma unroll
    for (int jj = 0; jj < JW; jj++) {
        float v = acc[jj];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) ts[wid + LORA_VEC_WAVES * jj] = f2bf(g.s * v);
    }
    __syncthreads();
    // ---- phase 2: a lane of wave 0 per output row of this workgroup's slice
    if (wid != 0) return;
    const size_t row = (size_t)(wg - wg0) * LORA_VEC_ROWS + lane;
    float v = 0.0f;
#pragma unroll
    for (int j8 = 0; j8 < R / 8; j8++) {
        const u32x4 bv = *reinterpret_cast<const u32x4*>(B + row * R + 8 * j8);
        const u32x4 tv = *reinterpret_cast<const u32x4*>(ts + 8 * j8);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            v = __builtin_fmaf(__uint_as_float(tv[e] << 16), __uint_as_float(bv[e] << 16), v);
            v = __builtin_fmaf(__uint_as_float(tv[e] & 0xffff0000u), __uint_as_float(bv[e] & 0xffff0000u), v);
        }
    }
    Y[row] = f2bf(bf2f(Y[row]) + g.s * v);
}

template <int R>
static int lora_tail_run(hipStream_t st, const LoraApplyPlan& p, const uint16_t* A, const uint16_t* B, const uint16_t* X, uint16_t* Y, uint16_t* T, int K, int M, float s, int n) {
    static int attr_set = 0;
    if (!attr_set && p.lds > 64 * 1024) {
        if (hipFuncSetAttribute((const void*)lora_rows_tail_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds) != hipSuccess) return KF_HIP_CHECK;
        attr_set = 1;
    }
    hipLaunchKernelGGL((lora_rows_tail_kernel<R>), dim3(p.gx), dim3(p.block), p.lds, st, A, B, X, Y, T, K, M, s, n);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

int lora_apply_launch(hipStream_t st, const LoraApplyPlan* p, int n_w, const uint16_t* const* a, const uint16_t* const* b, int r, const int* OC, int IC, const uint16_t* x,
                      uint16_t* const* y, uint16_t* ax, int n, float s) {
    if (p[0].form == LORA_FORM_TILE)
        return r == 16   ? lora_tail_run<16>(st, p[0], a[0], b[0], x, y[0], ax, IC, OC[0], s, n)
               : r == 32 ? lora_tail_run<32>(st, p[0], a[0], b[0], x, y[0], ax, IC, OC[0], s, n)
                         : lora_tail_run<64>(st, p[0], a[0], b[0], x, y[0], ax, IC, OC[0], s, n);
    LoraVecArgs g;
    int end = 0;
    for (int i = 0; i < LORA_APPLY_MAX; i++) {
        const int k = i < n_w ? i : n_w - 1; /* unused slots repeat the last adapter and own no workgroup */
        if (i < n_w) end += p[i].gx;
        g.a[i] = a[k], g.b[i] = b[k], g.y[i] = y[k], g.wg_end[i] = end;
    }
    g.x = x, g.IC = IC, g.s = s;
    if (r == 16) hipLaunchKernelGGL((lora_vec_kernel<16>), dim3(end), dim3(p[0].block), 0, st, g);
    else if (r == 32) hipLaunchKernelGGL((lora_vec_kernel<32>), dim3(end), dim3(p[0].block), 0, st, g);
    else hipLaunchKernelGGL((lora_vec_kernel<64>), dim3(end), dim3(p[0].block), 0, st, g);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
