// kf_lora.hip -- a low-rank pair beside a frozen matrix, the LORA branch of the reference's SLP::Forw / SLP::Back (NeuronFuse.cu:286-302, 343-358, 384-423, 453-468:
// HIERARCH_LorAB::Forw / Back, four cuBLASLt calls with rank-sized operands and the kept buffers Ax and Adelta).  a [r, IC], b [OC, r] bf16 row-major; s (the reference's
// sAB) multiplies BOTH products of each direction:
//   forward    ax [n, r] = bf16(s x a^T)                 y [n, OC] = bf16(y + s ax b^T)
//   backward   adelta [n, r] = bf16(s deltaIn b)         delta [n, IC] = bf16(delta + s adelta a)
//              gB [OC, r] = bf16(gB + s deltaIn^T ax)    gA [r, IC] = bf16(gA + s adelta^T inp)
// Every product runs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; rank 16 is a zero-padded K step.  The kernels (launch geometry: kf_lora_plan.h):
//   lora_rows_kernel  T = bf16(s X A^T) over the long contraction K, then Y += s T B^T over the M output columns, for LORA_TM token rows per workgroup.  The fragments
//                     of X [n, K] and A [r, K] are 16 contiguous bytes per lane in memory; the eight waves' partial tiles meet in LDS in wave order; T goes to memory
//                     and, rounded, to LDS.  The second product is computed transposed (B's rows on the MFMA's row index, taken in the order 0-3, 8-11, ... | 4-7,
//                     12-15, ... of a 32-column block) so that a lane ends up with 8 consecutive columns of one token row: one 16-byte load and store of Y per lane.
//                     Forward: X = x, A = a, B = b.  Backward rows: X = deltaIn, A = bT, B = aT -- the transposed copies lora_tr_kernel writes into the scratch.
//   lora_w_kernel     G [M, r] = U^T V over a slab of the token rows, U [n, M] and V [n, r] both k-major: 64-row k-steps staged in LDS as they lie in memory, the
//                     fragments read with the transposing ds_read_b64_tr_b16 (the idiom of kf_gemm3_tile.h, rows padded by 16 bytes instead of swizzled).  fp32
//                     partials in the gradient's own layout; gB's and gA's workgroups share one launch.
//   lora_fin_kernel   a thread per element of g = [gA | gB]: its slabs in index order, then g = bf16(g + s sum).
// No atomics; nothing read from the scratch that this call has not written.
#include "kf_gemm_common.h"
#include "kf_lora_plan.h"

namespace kf {

typedef __bf16 lora_bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 lora_zero_frag() { return __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u}); }

template <int R>
__global__ void __launch_bounds__(64 * LORA_ROW_WAVES) lora_rows_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, const uint16_t* __restrict__ X,
                                                                       uint16_t* __restrict__ Y, uint16_t* __restrict__ Tg, int K, int M, float s) {
    constexpr int JT = R / 16, KS = R >= 32 ? R / 32 : 1, TB = LORA_TM / 16, LDT = R + 8, NTH = 64 * LORA_ROW_WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* red = reinterpret_cast<float*>(smem_raw);                                                 /* [waves][TM][R] */
    uint16_t* ts = reinterpret_cast<uint16_t*>(smem_raw + LORA_ROW_WAVES * LORA_TM * R * 4);         /* [TM][LDT] */
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * LORA_TM;
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
            for (int tb = 0; tb < TB; tb++) xf[tb] = *reinterpret_cast<const bf16x8*>(X + (row0 + tb * 16 + l16) * K + k);
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
        Tg[(row0 + tok) * R + j] = h;
        ts[tok * LDT + j] = h;
    }
    __syncthreads();
    // ---- Y += s T B^T, transposed: B's rows are the MFMA's rows, the tokens its columns.  Rank 16: the upper half of the K step is zero on both sides
    const bool pad = R == 16 && q >= 2;
    bf16x8 tf[TB][KS];
#pragma unroll
    for (int tb = 0; tb < TB; tb++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) tf[tb][ks] = pad ? lora_zero_frag() : *reinterpret_cast<const bf16x8*>(ts + (tb * 16 + l16) * LDT + ks * 32 + 8 * q);
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
                const bf16x8 bf = pad ? lora_zero_frag() : *reinterpret_cast<const bf16x8*>(B + m * R + ks * 32 + 8 * q);
#pragma unroll
                for (int tb = 0; tb < TB; tb++) d[tt][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, tf[tb][ks], d[tt][tb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tb = 0; tb < TB; tb++) {
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

// aT [IC][r] = a^T, bT [r][OC] = b^T: an element per thread (r (IC + OC) of them, at most 400 K)
__global__ void __launch_bounds__(LORA_FIN_BLOCK) lora_tr_kernel(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b, int r, int OC, int IC, uint16_t* __restrict__ aT,
                                                                 uint16_t* __restrict__ bT) {
    const long long i = (long long)blockIdx.x * LORA_FIN_BLOCK + threadIdx.x, nA = (long long)r * IC, nB = (long long)r * OC;
    if (i < nA) {
        const int ic = (int)(i / r), j = (int)(i % r);
        aT[i] = a[(size_t)j * IC + ic];
    } else if (i < nA + nB) {
        const long long i2 = i - nA;
        const int j = (int)(i2 / OC), oc = (int)(i2 % OC);
        bT[i2] = b[(size_t)oc * r + j];
    }
}

// problem 0: gB (U = deltaIn, V = ax, M = OC, partials [S][M][r]); problem 1: gA (U = inp, V = adelta, M = IC, partials [S][r][M]); workgroups [0, wg0) are problem 0's
struct LoraWArgs {
    const uint16_t* U[2];
    const uint16_t* V[2];
    float* part[2];
    int M[2], S[2], tiles[2];
    int wg0, nkt;
};

// fragment (8 consecutive k of row rowblk16 16 + l16, k = kbase .. kbase + 7) of a [k][rows] LDS image with k-rows of ld bytes: two ds_read_b64_tr_b16, each a
// 4 (k) x 16 (rows) block transposed across 16 lanes -- lane l16 hands in k-row kbase + 4 t + (l16 >> 2), 8-byte piece l16 & 3, and receives row l16's four k
__device__ __forceinline__ bf16x8 lora_frag_km(const unsigned char* tile, int ld, int rowblk16, int kbase, int l16) {
    lora_bf16x4 h[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int k = kbase + 4 * t + (l16 >> 2);
        h[t] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) lora_bf16x4*)(tile + k * ld + (rowblk16 * 16 + 4 * (l16 & 3)) * 2));
    }
    return bf16x8{h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
}

template <int R>
__global__ void __launch_bounds__(256) lora_w_kernel(const LoraWArgs a) {
    constexpr int JT = R / 16, LDU = LORA_BM * 2 + 16, LDV = R * 2 + 16; /* bytes per k-row: 16 more than the data, so that the four k-rows of a transposing read miss each other's banks */
    constexpr int UPR = LORA_BM / 8, VPR = R / 8, NU = LORA_BK * UPR / 256, VCH = LORA_BK * VPR; /* 16-byte pieces per k-row; U pieces per thread; V pieces per step */
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char* Us = smem_raw;
    unsigned char* Vs = smem_raw + LORA_BK * LDU;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int pr = (int)blockIdx.x >= a.wg0 ? 1 : 0, local = (int)blockIdx.x - (pr ? a.wg0 : 0);
    const int M = a.M[pr], S = a.S[pr], tiles = a.tiles[pr];
    const int slab = local / tiles, m0 = (local % tiles) * LORA_BM;
    const int kt0 = (int)((long long)a.nkt * slab / S), kt1 = (int)((long long)a.nkt * (slab + 1) / S);
    const uint16_t* __restrict__ U = a.U[pr];
    const uint16_t* __restrict__ V = a.V[pr];
    u32x4 ur[NU], vr[2];
    auto load = [&](int kt) {
        const size_t t0 = (size_t)kt * LORA_BK;
#pragma unroll
        for (int i = 0; i < NU; i++) {
            const int c = tid + 256 * i;
            ur[i] = *reinterpret_cast<const u32x4*>(U + (t0 + c / UPR) * M + m0 + (c % UPR) * 8);
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int c = tid + 256 * i;
            if (c < VCH) vr[i] = *reinterpret_cast<const u32x4*>(V + (t0 + c / VPR) * R + (c % VPR) * 8);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < NU; i++) {
            const int c = tid + 256 * i;
            *reinterpret_cast<u32x4*>(Us + (c / UPR) * LDU + (c % UPR) * 16) = ur[i];
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int c = tid + 256 * i;
            if (c < VCH) *reinterpret_cast<u32x4*>(Vs + (c / VPR) * LDV + (c % VPR) * 16) = vr[i];
        }
    };
    f32x4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; jt++) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(kt0);
    for (int kt = kt0; kt < kt1; kt++) {
        __syncthreads(); /* every wave is done reading the step before */
        store();
        __syncthreads();
        if (kt + 1 < kt1) load(kt + 1); /* in flight under this step's products */
#pragma unroll
        for (int kk = 0; kk < LORA_BK / 32; kk++) {
            const bf16x8 af = lora_frag_km(Us, LDU, wid, kk * 32 + 8 * q, l16);
#pragma unroll
            for (int jt = 0; jt < JT; jt++) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, lora_frag_km(Vs, LDV, jt, kk * 32 + 8 * q, l16), acc[jt], 0, 0, 0);
        }
    }
    // lane (l16, q): rows m0 + wid 16 + 4 q + reg of G, rank column jt 16 + l16
    float* part = a.part[pr] + (size_t)slab * M * R;
    const int mr = m0 + wid * 16 + 4 * q;
#pragma unroll
    for (int jt = 0; jt < JT; jt++) {
        if (pr == 0) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) part[(size_t)(mr + reg) * R + jt * 16 + l16] = acc[jt][reg];
        } else {
            *reinterpret_cast<f32x4*>(part + (size_t)(jt * 16 + l16) * M + mr) = acc[jt];
        }
    }
}

// element i of g = [gA (r IC) | gB (OC r)]: its gradient's slabs in index order
__global__ void __launch_bounds__(LORA_FIN_BLOCK) lora_fin_kernel(const float* __restrict__ partA, int SA, long long nA, const float* __restrict__ partB, int SB, long long nB,
                                                                  float s, uint16_t* __restrict__ g) {
    const long long i = (long long)blockIdx.x * LORA_FIN_BLOCK + threadIdx.x;
    if (i >= nA + nB) return;
    float v = 0.0f;
    if (i < nA) {
        for (int k = 0; k < SA; k++) v += partA[(size_t)k * nA + i];
    } else {
        for (int k = 0; k < SB; k++) v += partB[(size_t)k * nB + (i - nA)];
    }
    g[i] = f2bf(bf2f(g[i]) + s * v);
}

template <int R>
static int lora_rows_run(hipStream_t st, const LoraPlan& p, const uint16_t* A, const uint16_t* B, const uint16_t* X, uint16_t* Y, uint16_t* T, int K, int M, float s) {
    static int attr_set = 0;
    if (!attr_set && p.rows_lds > 64 * 1024) {
        if (hipFuncSetAttribute((const void*)lora_rows_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, p.rows_lds) != hipSuccess) return KF_HIP_CHECK;
        attr_set = 1;
    }
    hipLaunchKernelGGL((lora_rows_kernel<R>), dim3(p.rows_gx), dim3(p.rows_block), p.rows_lds, st, A, B, X, Y, T, K, M, s);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}
static int lora_rows(hipStream_t st, const LoraPlan& p, int r, const uint16_t* A, const uint16_t* B, const uint16_t* X, uint16_t* Y, uint16_t* T, int K, int M, float s) {
    return r == 16 ? lora_rows_run<16>(st, p, A, B, X, Y, T, K, M, s) : r == 32 ? lora_rows_run<32>(st, p, A, B, X, Y, T, K, M, s) : lora_rows_run<64>(st, p, A, B, X, Y, T, K, M, s);
}

int lora_forward_launch(hipStream_t st, const LoraPlan& p, const uint16_t* a, const uint16_t* b, int r, int OC, int IC, const uint16_t* x, uint16_t* y, uint16_t* ax, int n, float s) {
    (void)n;
    return lora_rows(st, p, r, a, b, x, y, ax, IC, OC, s);
}

int lora_backward_launch(hipStream_t st, const LoraPlan& p, const uint16_t* a, const uint16_t* b, int r, int OC, int IC, const uint16_t* deltaIn, const uint16_t* inp,
                         const uint16_t* ax, uint16_t* delta, uint16_t* g, int n, float s, unsigned char* scratch) {
    uint16_t* adelta = reinterpret_cast<uint16_t*>(scratch + p.off_adelta);
    uint16_t* aT = reinterpret_cast<uint16_t*>(scratch + p.off_aT);
    uint16_t* bT = reinterpret_cast<uint16_t*>(scratch + p.off_bT);
    float* partA = reinterpret_cast<float*>(scratch + p.off_partA);
    float* partB = reinterpret_cast<float*>(scratch + p.off_partB);
    hipLaunchKernelGGL(lora_tr_kernel, dim3((unsigned)p.tr_gx), dim3(LORA_FIN_BLOCK), 0, st, a, b, r, OC, IC, aT, bT);
    if (hipGetLastError() != hipSuccess) return KF_HIP_CHECK;
    const int rc = lora_rows(st, p, r, bT, aT, deltaIn, delta, adelta, OC, IC, s); /* adelta = bf16(s deltaIn b), delta += s adelta a */
    if (rc != KF_OK) return rc;
    LoraWArgs w;
    w.U[0] = deltaIn, w.V[0] = ax, w.part[0] = partB, w.M[0] = OC, w.S[0] = p.SB, w.tiles[0] = p.tilesB;
    w.U[1] = inp, w.V[1] = adelta, w.part[1] = partA, w.M[1] = IC, w.S[1] = p.SA, w.tiles[1] = p.tilesA;
    w.wg0 = p.tilesB * p.SB, w.nkt = n / LORA_BK;
    if (r == 16) hipLaunchKernelGGL((lora_w_kernel<16>), dim3(p.w_gx), dim3(p.w_block), p.w_lds, st, w);
    else if (r == 32) hipLaunchKernelGGL((lora_w_kernel<32>), dim3(p.w_gx), dim3(p.w_block), p.w_lds, st, w);
    else hipLaunchKernelGGL((lora_w_kernel<64>), dim3(p.w_gx), dim3(p.w_block), p.w_lds, st, w);
    if (hipGetLastError() != hipSuccess) return KF_HIP_CHECK;
    hipLaunchKernelGGL(lora_fin_kernel, dim3((unsigned)p.fin_gx), dim3(LORA_FIN_BLOCK), 0, st, partA, p.SA, (long long)r * IC, partB, p.SB, (long long)OC * r, s, g);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
