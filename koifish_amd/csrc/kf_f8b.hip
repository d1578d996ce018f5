// kf_f8b.hip -- layers stored as OCP e4m3 bytes with one fp32 scale per 128 x 128 block (the FP8 releases of the Qwen3 family; include/kf_abi.h "FP8 block-scaled
// layers"), gfx950 / wave64:   W[r][k] = scale[r / 128][k / 128] * e4m3(byte[r][k]).
//
// What the storage gives the hot path: a byte per weight read as it lies; an e4m3 value is a bf16 value, so the unpack (v_cvt_pk_f32_fp8) rounds nothing; an
// e4m3 x bf16 product is exact in fp32; and the scale is constant over a 128-wide k-block of a row, so it multiplies a block's SUM, never a weight.
//
//   f8b_vec_kernel    one token.  Waves own `rows` consecutive output rows for the whole of K; lane l of load i takes the 16 bytes of piece 64 i + l of a row (8 lanes =
//                     one 128-block), several loads in flight; x is staged once per workgroup as fp32 in LDS, panel by panel, laid out so that the four 16-byte reads
//                     of a piece are conflict free ([load][quarter][lane]); a piece is summed unscaled in two fma chains, then acc = fma(scale, piece, acc).  RMSNorm
//                     prologue, residual / SwiGLU epilogues: the rules of kf_device.h.
//   f8b_tile_kernel   token batches: 2 x 2 waves own [32 TM rows of W] x [32 TN tokens].  Per k-block the bytes go global -> registers -> bf16 pairs -> the A operand
//                     registers (no LDS image of W: a lane's 16 consecutive bytes ARE its k-slices of two MFMA steps, the k order inside a block being free as long
//                     as x follows it); x goes global -> LDS as bf16, XOR-swizzled by row, double buffered; four v_mfma_f32_16x16x32_bf16 steps fill a block
//                     accumulator from zero, then acc = fma(scale, blk, acc).  One launch, no scratch, no split over k.
//   f8b_quant_kernel  one workgroup per scale block: amax, scale = 2^e (the power-of-two rule of kf_act_quant_f8), codes by v_cvt_pk_fp8_f32.
//   f8b_dequant_kernel  bf16(scale * value).
#include "kf_f8b_plan.h"
#include "kf_gemm_common.h"

namespace kf {

template <bool HI>
__device__ __forceinline__ f32x2_t e4m3_pair(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI); }
// eight e4m3 bytes (two dwords, ascending k) -> eight bf16 (exact)
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t d0, uint32_t d1) {
    const f32x2_t a = e4m3_pair<false>(d0), b = e4m3_pair<true>(d0), c = e4m3_pair<false>(d1), d = e4m3_pair<true>(d1);
    return __builtin_bit_cast(bf16x8, u32x4{pack_bf16x2(a.x, a.y), pack_bf16x2(b.x, b.y), pack_bf16x2(c.x, c.y), pack_bf16x2(d.x, d.y)});
}

// ------------------------------------------------------------------------------------------------ one token
struct F8bVecJob {
    const unsigned char* w;
    const float* sc;
    uint16_t* y;
    long long y_pos_stride;
    int M;
};
struct F8bVecArgs {
    F8bVecJob job[3];
    int njobs, K, groups;
    const uint16_t *x, *norm_w;
    float eps, inv_dim;
    const uint16_t *residual, *bias;
    float alpha, beta;
    const int* d_pos;
    int pos;
};

// the unscaled sum of one piece (16 weights against 16 x): even k in .x, odd k in .y, one v_pk_fma_f32 per weight pair in ascending k, joined as x + y
__device__ __forceinline__ float piece_dot(u32x4 w, f32x4 x0, f32x4 x1, f32x4 x2, f32x4 x3) {
    f32x2_t c = {0.f, 0.f};
    c = pk_fma(e4m3_pair<false>(w.x), f32x2_t{x0.x, x0.y}, c), c = pk_fma(e4m3_pair<true>(w.x), f32x2_t{x0.z, x0.w}, c);
    c = pk_fma(e4m3_pair<false>(w.y), f32x2_t{x1.x, x1.y}, c), c = pk_fma(e4m3_pair<true>(w.y), f32x2_t{x1.z, x1.w}, c);
    c = pk_fma(e4m3_pair<false>(w.z), f32x2_t{x2.x, x2.y}, c), c = pk_fma(e4m3_pair<true>(w.z), f32x2_t{x2.z, x2.w}, c);
    c = pk_fma(e4m3_pair<false>(w.w), f32x2_t{x3.x, x3.y}, c), c = pk_fma(e4m3_pair<true>(w.w), f32x2_t{x3.z, x3.w}, c);
    return c.x + c.y;
}

template <int R, bool PAIRED>
__global__ void __launch_bounds__(64 * F8B_WAVES) f8b_vec_kernel(const F8bVecArgs a) {
    constexpr int NM = PAIRED ? 2 : 1, NTH = 64 * F8B_WAVES;
    constexpr int U = NM * R >= 4 ? 2 : 4; /* loads of a row in flight */
    __shared__ __attribute__((aligned(16))) float xs[F8B_PANEL];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the rows of this wave: group g of the launch's matrices laid end to end (PAIRED: of gate, and the same rows of up)
    const int g = blockIdx.x * F8B_WAVES + wave;
    const bool live = g < a.groups;
    F8bVecJob J = a.job[0];
    int rem = g;
    if (!PAIRED && a.njobs > 1 && rem >= a.job[0].M / R) {
        rem -= a.job[0].M / R, J = a.job[1];
        if (a.njobs > 2 && rem >= a.job[1].M / R) rem -= a.job[1].M / R, J = a.job[2];
    }
    const int row0 = rem * R, nkb = a.K / F8B_BLOCK;
    const unsigned char* wp[NM];
    const float* sp[NM];
    wp[0] = J.w + (size_t)row0 * a.K, sp[0] = J.sc + (size_t)(row0 / F8B_BLOCK) * nkb;
    if (PAIRED) wp[NM - 1] = a.job[1].w + (size_t)row0 * a.K, sp[NM - 1] = a.job[1].sc + (size_t)(row0 / F8B_BLOCK) * nkb;

    float mul = 1.0f;
    if (a.norm_w) mul = rms_scale((float)block_sumsq_bf16(a.x, a.K, red), a.inv_dim, a.eps);

    float acc[NM][R];
#pragma unroll
    for (int m = 0; m < NM; m++)
#pragma unroll
        for (int r = 0; r < R; r++) acc[m][r] = 0.f;

    for (int k0 = 0; k0 < a.K; k0 += F8B_PANEL) {
        const int pk = a.K - k0 < F8B_PANEL ? a.K - k0 : F8B_PANEL, np = pk >> 4; /* pieces of 16 in this panel */
        __syncthreads(); /* every wave is through with the last panel */
        for (int c = tid; c < (pk >> 3); c += NTH) { /* eight bf16 a chunk = half a piece: quarters j0, j0 + 1 of piece c / 2 */
            u32x4 v = *reinterpret_cast<const u32x4*>(a.x + k0 + 8 * c);
            if (a.norm_w) {
                const u32x4 nw = *reinterpret_cast<const u32x4*>(a.norm_w + k0 + 8 * c);
                v = u32x4{rms_pair(v.x, nw.x, mul), rms_pair(v.y, nw.y, mul), rms_pair(v.z, nw.z, mul), rms_pair(v.w, nw.w, mul)};
            }
            const int P = c >> 1, j0 = (c & 1) * 2;
            u32x4* dst = reinterpret_cast<u32x4*>(xs) + (((P >> 6) * 4 + j0) * 64 + (P & 63));
            dst[0] = widen_bf16x4(v.x, v.y), dst[64] = widen_bf16x4(v.z, v.w);
        }
        __syncthreads();
        if (!live) continue;
        for (int it0 = 0; it0 * 64 < np; it0 += U) {
            u32x4 wv[U][NM][R];
            float s[U][NM];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int P = (it0 + u) * 64 + lane;
                const bool ok = P < np;
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    s[u][m] = ok ? sp[m][(k0 >> 7) + (P >> 3)] : 0.f;
#pragma unroll
                    for (int r = 0; r < R; r++)
                        wv[u][m][r] = ok ? ld_nt(reinterpret_cast<const u32x4*>(wp[m] + (size_t)r * a.K + k0 + 16 * P)) : u32x4{0u, 0u, 0u, 0u};
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if ((it0 + u) * 64 + lane >= np) continue; /* nothing staged there */
                const f32x4* xp = reinterpret_cast<const f32x4*>(xs) + ((it0 + u) * 4 * 64 + lane);
                const f32x4 x0 = xp[0], x1 = xp[64], x2 = xp[128], x3 = xp[192];
#pragma unroll
                for (int m = 0; m < NM; m++)
#pragma unroll
                    for (int r = 0; r < R; r++) acc[m][r] = fmaf(s[u][m], piece_dot(wv[u][m][r], x0, x1, x2, x3), acc[m][r]);
            }
        }
    }
    if (!live) return;
    const int pos = a.d_pos ? *a.d_pos : a.pos;
    uint16_t* y = J.y + (long long)pos * J.y_pos_stride;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const float v = wave_sum(acc[0][r]);
        float v2 = 0.f;
        if (PAIRED) v2 = wave_sum(acc[NM - 1][r]);
        if (lane != r) continue;
        const size_t row = (size_t)row0 + r;
        if (PAIRED) y[row] = swiglu_bf16(round_bf16(v), round_bf16(v2)); /* of the two bf16-rounded projections */
        else y[row] = linear_out_bf16(v, a.alpha, a.beta, y, row, a.bias, row, a.residual, row);
    }
}

template <int R, bool PAIRED>
static int f8b_vec_run(hipStream_t st, const F8bVecPlan& p, const F8bVecArgs& a) {
    hipLaunchKernelGGL((f8b_vec_kernel<R, PAIRED>), dim3(p.grid), dim3(64 * F8B_WAVES), 0, st, a);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

// n_w = 1 .. 3 matrices of one K (paired: gate, up -> SwiGLU into y[0]); every weight has passed f8b_check
int f8b_vec_launch(hipStream_t st, int n_w, const kf_weight* const* w, bool paired, const uint16_t* x, const uint16_t* norm_w, float eps, uint16_t* const* y,
                   const int64_t* y_pos_stride, int pos, const int* d_pos, const uint16_t* bias, float alpha, float beta, const uint16_t* residual) {
    if (n_w < 1 || n_w > 3 || (paired && n_w != 2)) return KF_INVALID_ARGS;
    F8bVecArgs a = {};
    int M[3] = {0, 0, 0};
    for (int i = 0; i < n_w; i++) {
        if (w[i]->ne1 != w[0]->ne1 || (paired && w[i]->ne0 != w[0]->ne0)) return KF_INVALID_ARGS;
        a.job[i] = F8bVecJob{(const unsigned char*)w[i]->data, (const float*)w[i]->qscales, paired ? y[0] : y[i], y_pos_stride ? y_pos_stride[paired ? 0 : i] : 0, w[i]->ne0};
        M[i] = w[i]->ne0;
    }
    const F8bVecPlan p = f8b_vec_plan(M, n_w, w[0]->ne1, paired);
    a.njobs = n_w, a.K = w[0]->ne1, a.groups = p.groups;
    a.x = x, a.norm_w = norm_w, a.eps = eps, a.inv_dim = 1.0f / (float)a.K;
    a.residual = residual, a.bias = bias, a.alpha = alpha, a.beta = beta, a.d_pos = d_pos, a.pos = pos;
    if (paired) return p.rows == 2 ? f8b_vec_run<2, true>(st, p, a) : f8b_vec_run<1, true>(st, p, a);
    return p.rows == 4 ? f8b_vec_run<4, false>(st, p, a) : p.rows == 2 ? f8b_vec_run<2, false>(st, p, a) : f8b_vec_run<1, false>(st, p, a);
}

// ------------------------------------------------------------------------------------------------ token batches
struct F8bTileArgs {
    const unsigned char* w;
    const float* sc;
    const uint16_t* x;
    uint16_t* y;
    const uint16_t *bias, *res;
    float alpha, beta;
    int M, K, n;
};

template <int TM, int TN>
__global__ void __launch_bounds__(256) f8b_tile_kernel(const F8bTileArgs a) {
    constexpr int BM = 32 * TM, BN = 32 * TN, XCH = BN * 16 / 256; /* 16-byte chunks of x per thread and k-block */
    __shared__ __attribute__((aligned(16))) uint16_t xs[2][BN * F8B_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q4 = lane >> 4, wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * BM + wm * TM * 16, tok0 = blockIdx.y * BN, nkb = a.K / F8B_BLOCK;

    u32x4 wraw[TM][2]; /* lane (r16, q4) of fragment i: bytes 64 h + 16 q4 .. + 15 of the k-block of row m0 + 16 i + r16 */
    float scp[TM];
    u32x4 xreg[XCH];
    auto fetch = [&](int kb) { /* k-block kb: global -> registers; a fragment past the last row and a token past the last one read nothing */
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const int mf = m0 + 16 * i;
            const bool in = mf < a.M; /* ne0 % 16 == 0: a fragment is inside or outside as a whole */
            const unsigned char* p = a.w + (size_t)(mf + r16) * a.K + (size_t)kb * F8B_BLOCK + 16 * q4;
#pragma unroll
            for (int h = 0; h < 2; h++) wraw[i][h] = in ? ld_nt(reinterpret_cast<const u32x4*>(p + 64 * h)) : u32x4{0u, 0u, 0u, 0u};
            scp[i] = in ? a.sc[(size_t)(mf >> 7) * nkb + kb] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < XCH; u++) {
            const int id = tid + u * 256, row = id >> 4, c = id & 15, tok = tok0 + row;
            xreg[u] = tok < a.n ? *reinterpret_cast<const u32x4*>(a.x + (size_t)tok * a.K + (size_t)kb * F8B_BLOCK + 8 * c) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto stash = [&](int buf) { /* x registers -> LDS buffer buf: chunk c of row `row` at chunk c ^ (row & 15) */
#pragma unroll
        for (int u = 0; u < XCH; u++) {
            const int id = tid + u * 256, row = id >> 4, c = id & 15;
            *reinterpret_cast<u32x4*>(&xs[buf][row * F8B_BLOCK + 8 * (c ^ (row & 15))]) = xreg[u];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    stash(0);
    __syncthreads();
    for (int kb = 0; kb < nkb; kb++) {
        bf16x8 wf[TM][4]; /* MFMA step s = 2 h + e: this lane's k are 64 h + 16 q4 + 8 e .. + 7 */
        float sc[TM];
#pragma unroll
        for (int i = 0; i < TM; i++) {
            sc[i] = scp[i];
#pragma unroll
            for (int h = 0; h < 2; h++)
                wf[i][2 * h] = e4m3x8_to_bf16(wraw[i][h].x, wraw[i][h].y), wf[i][2 * h + 1] = e4m3x8_to_bf16(wraw[i][h].z, wraw[i][h].w);
        }
        if (kb + 1 < nkb) fetch(kb + 1); /* in flight under the MFMAs */
        const uint16_t* xl = xs[kb & 1];
        f32x4 blk[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++) blk[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int c = 8 * (s >> 1) + 2 * q4 + (s & 1); /* the x chunk that holds this lane's k of step s */
#pragma unroll
            for (int j = 0; j < TN; j++) {
                const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xl + ((wn * TN + j) * 16 + r16) * F8B_BLOCK + 8 * (c ^ r16));
#pragma unroll
                for (int i = 0; i < TM; i++) blk[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i][s], xf, blk[i][j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int e = 0; e < 4; e++) acc[i][j][e] = fmaf(sc[i], blk[i][j][e], acc[i][j][e]);
        if (kb + 1 < nkb) stash((kb + 1) & 1); /* the buffer k-block kb - 1 was read from: every wave passed the barrier that closed it */
        __syncthreads();
    }

    // lane (r16, q4) of tile (i, j): rows m0 + 16 i + 4 q4 .. + 3 of W (four consecutive outputs), token tok0 + 16 (wn TN + j) + r16
    const bool vec_y = (reinterpret_cast<uintptr_t>(a.y) & 7) == 0;
#pragma unroll
    for (int j = 0; j < TN; j++) {
        const int tok = tok0 + (wn * TN + j) * 16 + r16;
        if (tok >= a.n) continue;
        uint16_t* yp = a.y + (size_t)tok * a.M;
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const int o0 = m0 + 16 * i + 4 * q4;
            if (m0 + 16 * i >= a.M) continue;
            uint16_t o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = linear_out_bf16(acc[i][j][e], a.alpha, a.beta, yp, o0 + e, a.bias, o0 + e, a.res, (size_t)tok * a.M + o0 + e);
            if (vec_y) {
                *reinterpret_cast<u32x2*>(yp + o0) = u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) yp[o0 + e] = o[e];
            }
        }
    }
}

template <int TM, int TN>
static int f8b_tile_run(hipStream_t st, const F8bTilePlan& p, const F8bTileArgs& a) {
    hipLaunchKernelGGL((f8b_tile_kernel<TM, TN>), dim3(p.gx, p.gy), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

int f8b_tile_launch(hipStream_t st, const kf_weight* w, const uint16_t* x, int n, uint16_t* y, const uint16_t* bias, float alpha, float beta, const uint16_t* residual) {
    const F8bTilePlan p = f8b_tile_plan(w->ne0, n);
    const F8bTileArgs a = {(const unsigned char*)w->data, (const float*)w->qscales, x, y, bias, residual, alpha, beta, w->ne0, w->ne1, n};
    return p.tm == 4 ? f8b_tile_run<4, 4>(st, p, a) : p.tm == 2 ? f8b_tile_run<2, 2>(st, p, a) : f8b_tile_run<1, 1>(st, p, a);
}

// ------------------------------------------------------------------------------------------------ quantise / dequantise
constexpr float F8B_MAX_FRAC = 0.875f; /* the largest finite e4m3fn, 448, is 0.875 * 2^9 */
constexpr int F8B_MAX_EXP = 9;
__device__ __forceinline__ uint32_t e4m3_pack4(float a, float b, float c, float d) {
    const int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
}
// one workgroup per 128 x 128 block (the last scale row may hold fewer rows); thread t: half (t & 1) of row t / 2, 64 weights
__global__ void __launch_bounds__(256) f8b_quant_kernel(const uint16_t* __restrict__ src, unsigned char* __restrict__ codes, float* __restrict__ scales, int M, int K) {
    __shared__ float mx[4];
    const int tid = threadIdx.x, row = blockIdx.y * F8B_BLOCK + (tid >> 1);
    const size_t off = (size_t)row * K + (size_t)blockIdx.x * F8B_BLOCK + 64 * (tid & 1);
    const bool in = row < M;
    u32x4 v[8];
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        v[c] = in ? *reinterpret_cast<const u32x4*>(src + off + 8 * c) : u32x4{0u, 0u, 0u, 0u};
        const uint32_t d[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
#pragma unroll
        for (int k = 0; k < 4; k++) m = fmaxf(m, fmaxf(fabsf(bf_lo(d[k])), fabsf(bf_hi(d[k]))));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) mx[tid >> 6] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3]));
    int e = 0;
    if (amax != 0.0f) {
        int ex;
        const float fr = frexpf(amax, &ex); /* amax = fr * 2^ex, fr in [0.5, 1) */
        e = ex - (fr <= F8B_MAX_FRAC ? F8B_MAX_EXP : F8B_MAX_EXP - 1);
    }
    if (tid == 0) scales[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = amax != 0.0f ? ldexpf(1.0f, e) : 0.0f;
    if (!in) return;
    auto q = [&](float f) { return amax != 0.0f ? ldexpf(f, -e) : 0.0f; }; /* exact; an all-zero block: codes 0 */
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        uint32_t o[4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const u32x4 t = v[c + h];
            o[2 * h] = e4m3_pack4(q(bf_lo(t.x)), q(bf_hi(t.x)), q(bf_lo(t.y)), q(bf_hi(t.y)));
            o[2 * h + 1] = e4m3_pack4(q(bf_lo(t.z)), q(bf_hi(t.z)), q(bf_lo(t.w)), q(bf_hi(t.w)));
        }
        *reinterpret_cast<u32x4*>(codes + off + 8 * c) = u32x4{o[0], o[1], o[2], o[3]};
    }
}
int f8b_quantize_launch(hipStream_t st, const kf_weight* w, const uint16_t* src) {
    if ((uintptr_t)src & 15) return KF_BLAS_UNALIGN;
    hipLaunchKernelGGL(f8b_quant_kernel, dim3(w->ne1 / F8B_BLOCK, (unsigned)f8b_scale_rows(w->ne0)), dim3(256), 0, st, src, (unsigned char*)const_cast<void*>(w->data),
                       (float*)const_cast<void*>(w->qscales), w->ne0, w->ne1);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

// a thread per 16 bytes: bf16(scale * value), one rounding
__global__ void __launch_bounds__(256) f8b_dequant_kernel(const unsigned char* __restrict__ codes, const float* __restrict__ scales, uint16_t* __restrict__ out, int K, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const size_t row = i / (size_t)(K >> 4);
    const int kc = (int)(i % (size_t)(K >> 4));
    const float s = scales[(row >> 7) * (size_t)(K >> 7) + (kc >> 3)];
    const u32x4 w = *reinterpret_cast<const u32x4*>(codes + 16 * i);
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const f32x2_t lo = e4m3_pair<false>(d[k]), hi = e4m3_pair<true>(d[k]);
        o[2 * k] = pack_bf16x2(s * lo.x, s * lo.y), o[2 * k + 1] = pack_bf16x2(s * hi.x, s * hi.y);
    }
    u32x4* op = reinterpret_cast<u32x4*>(out + 16 * i);
    op[0] = u32x4{o[0], o[1], o[2], o[3]}, op[1] = u32x4{o[4], o[5], o[6], o[7]};
}
int f8b_dequant_launch(hipStream_t st, const kf_weight* w, uint16_t* out) {
    const size_t n16 = (size_t)w->ne0 * w->ne1 / 16;
    hipLaunchKernelGGL(f8b_dequant_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (const unsigned char*)w->data, (const float*)w->qscales, out, w->ne1, n16);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
