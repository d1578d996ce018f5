// kf_attn_prefill_kv8.hip -- causal GQA attention for a batch of prompt tokens on the int8 KV cache (include/kf_abi.h "int8 KV cache", the prompt form): integer scores on
// v_mfma_i32_16x16x64_i8 straight from the cache rows, the decode definition's score / weight arithmetic per element, P.V on v_mfma_f32_16x16x32_bf16.  gfx950 / wave64.
//
// Workgroup = one kv-head x 64 "columns" (token, query head of the group) = 64 / GQ consecutive tokens, 16 columns per wave; the launch is the ATTN_PROMPT_KV8 entry of
// kf::attn_plan.  Prologue: the workgroup's bf16 query heads go to LDS, every wave quantises its 16 of them with the row quantiser (quant_head_lds, the decode kernel's) and
// keeps the codes of its column as the B operand: lane (c = lane & 15, h = lane >> 4) holds q8[column c][64 s + 16 h .. + 15] of step s.
// Key tiles of APK8_KT = 64 keys ANCHORED AT KEY 0 (tile j = keys 64 j .. 64 j + 63 whatever pos0 and n_tok are), staged once in LDS for the four waves: K8 rows as they are
// (16 bytes of row padding), V8 rows converted to bf16 (exact) with 32 bytes of row padding, the two steps of every row.  Per tile and wave:
//   I^T[key][col] = sum_d K8[key][d] Q8[col][d]     four 16-key sub-tiles, each hd / 64 MFMA steps into an int32x4 that starts from zero; A = K8 rows (ds_read_b128): lane
//                                                   (r, h) reads K8[16 u + r][64 s + 16 h ..]; both operands' lane quarter h carries the same 16 elements, and an integer
//                                                   sum does not care about their order.  The lane ends up with keys 16 u + 4 h + {0..3} of ITS column: no cross-lane
//                                                   traffic except the tile's maximum exponent over the column's four lanes.
//   c = sq * KS, d = fp32(I) * c, s = bf16(d * rden), (f, n) = kf_exp2_parts(s * log2 e), g = f * VS, gb = bf16(g)     per element, the definition's order, nothing fused
//   m = max(m, the tile's largest n over keys <= the column's position); when it moves O and L are multiplied by 2^(m_old - m_new): exact
//   O^T[d][col] += sum_key V^T[d][key] (gb 2^(n - m))[key][col]    the weights of sub-tiles (2 w, 2 w + 1), packed to bf16 (exact), ARE the B operand of step w: slot
//                                                   (h, j) <-> key 32 w + 16 (j >> 2) + 4 h + (j & 3); A = V^T fragments read from the row-major bf16 V tile with two
//                                                   transposing ds_read_b64_tr_b16 (4 keys x 16 d per 16 lanes), as kf_attn_prefill.hip reads its V tile.
//   L += f 2^(n - m)  in the lane, fp32; the column's four lanes are added at the end, (l0 + l1) + (l2 + l3).
// out = bf16(O / L), a correctly rounded fp32 division.  A key's place (tile, sub-tile, lane quarter, register) is a function of the key's index alone, a column's m after
// tile j is the largest n among its keys in tiles 0 .. j, and keys past the column's position contribute +0 / -0 and never move m: a row's output bits depend on its
// position, its q row and the cache, not on pos0, n_tok, its neighbours or the grid.  No scratch, no hand-off between workgroups.
#include "kf_attn_common.h"
#include "kf_attn_plan.h"

namespace kf {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 k8_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 k8_bf16x4 __attribute__((ext_vector_type(4)));

// four int8 codes of a dword -> four bf16 (exact: |code| <= 128 has 8 significant bits), as two packed pairs
__device__ __forceinline__ u32x2 codes_to_bf16(uint32_t w) {
    const float c0 = (float)((int)(w << 24) >> 24), c1 = (float)((int)(w << 16) >> 24), c2 = (float)((int)(w << 8) >> 24), c3 = (float)((int)w >> 24);
    return u32x2{(__float_as_uint(c0) >> 16) | (__float_as_uint(c1) & 0xffff0000u), (__float_as_uint(c2) >> 16) | (__float_as_uint(c3) & 0xffff0000u)};
}

template <int HD, int GQ>
__global__ void __launch_bounds__(256) attn_prefill_kv8_kernel(const AttnPrefillKv8Args a) {
    constexpr int KT = APK8_KT, COLS = APK8_COLS;
    constexpr int KSB = HD + APK8_KPAD;   /* K8 row, bytes */
    constexpr int VSE = HD + APK8_VPAD;   /* bf16 V row, elements */
    constexpr int NS = HD / 64;           /* integer MFMA steps over d */
    constexpr int NDB = HD / 16;          /* 16-row blocks of O^T */
    constexpr int TQ = COLS / GQ;         /* tokens per workgroup */
    constexpr int CPR = HD / 16;          /* 16-byte chunks per cache row */
    constexpr int CPT = KT * CPR / 256;   /* chunks per thread and tile */
    static_assert(KT == 64 && COLS == 64 && KT * CPR % 256 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr AttnTileKv8Lds lds(HD);
    static_assert(lds.fits(), "LDS");
    int8_t* kt8 = reinterpret_cast<int8_t*>(smem_raw + lds.kt8);          // [KT][KSB]
    uint16_t* vt = reinterpret_cast<uint16_t*>(smem_raw + lds.vt);        // [KT][VSE] bf16 bits
    float* kst = reinterpret_cast<float*>(smem_raw + lds.kst);            // [KT] K steps, [KT] V steps behind them
    float* vst = reinterpret_cast<float*>(smem_raw + lds.vst);
    int8_t* q8 = reinterpret_cast<int8_t*>(smem_raw + lds.q8);            // [COLS][HD] query codes
    float* sqs = reinterpret_cast<float*>(smem_raw + lds.sqs);            // [COLS] query steps
    uint16_t* qb = reinterpret_cast<uint16_t*>(smem_raw + lds.qb);        // prologue only: [COLS][HD] bf16 query heads, in the V tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h = lane >> 4;
    const int kvh = blockIdx.y, blk = (int)gridDim.x - 1 - (int)blockIdx.x; /* the blocks with the most keys first */
    const int tok0 = blk * TQ;
    const int ci = wave * 16 + c, tq = ci / GQ, hq = ci - tq * GQ;
    const bool col_ok = tok0 + tq < a.n_tok;
    const int tok = col_ok ? tok0 + tq : a.n_tok - 1;
    const int pos_q = a.pos0 + tok; /* the last key this column attends to */
    const int last_tok = tok0 + TQ - 1 < a.n_tok - 1 ? tok0 + TQ - 1 : a.n_tok - 1;
    const int kmax = a.pos0 + last_tok; /* the last key any column of the workgroup needs: nothing past it is read */
    const int ntile = kmax / KT + 1;
    const int wave_last = tok0 + (wave * 16 + 15) / GQ < a.n_tok - 1 ? tok0 + (wave * 16 + 15) / GQ : a.n_tok - 1;
    const int ntile_w = (a.pos0 + wave_last) / KT + 1; /* tiles this wave multiplies */

    // ---- prologue: the wave's 16 query heads to LDS, quantised there, the lane's codes to registers
    for (int i = lane; i < 16 * (HD / 8); i += 64) {
        const int j = i / (HD / 8), dc = i - j * (HD / 8), cj = wave * 16 + j, tj0 = tok0 + cj / GQ, tj = tj0 < a.n_tok ? tj0 : a.n_tok - 1;
        *reinterpret_cast<u32x4*>(qb + cj * HD + dc * 8) =
            *reinterpret_cast<const u32x4*>(a.q + (size_t)tj * a.q_stride + (size_t)(kvh * GQ + cj % GQ) * HD + dc * 8);
    }
    __syncthreads();
    for (int j = 0; j < 16; j++) quant_head_lds(qb + (wave * 16 + j) * HD, HD, q8 + (wave * 16 + j) * HD, sqs + wave * 16 + j);
    __syncthreads();
    i32x4 qreg[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) qreg[s] = *reinterpret_cast<const i32x4*>(q8 + ci * HD + 64 * s + 16 * h);
    const float sq = sqs[ci];

    // ---- tiles travel global -> registers -> LDS; tile t + 1 is loaded while tile t is multiplied
    u32x4 kr[CPT], vr[CPT];
    float sr = 0.0f;
    auto tload = [&](int t) {
#pragma unroll
        for (int i = 0; i < CPT; i++) {
            const int ch = tid + 256 * i, key = ch / CPR, dc = ch - key * CPR;
            int kk = t * KT + key;
            if (kk > kmax) kk = kmax; /* rows past the last needed key are masked below; never read past it */
            const size_t off = (size_t)kk * a.kv_stride + (size_t)kvh * HD + dc * 16;
            kr[i] = *reinterpret_cast<const u32x4*>(a.k8 + off);
            vr[i] = *reinterpret_cast<const u32x4*>(a.v8 + off);
        }
        if (tid < 2 * KT) {
            int kk = t * KT + (tid & (KT - 1));
            if (kk > kmax) kk = kmax;
            sr = (tid < KT ? a.ks : a.vs)[(size_t)kk * a.n_kv + kvh];
        }
    };
    auto tstore = [&]() {
#pragma unroll
        for (int i = 0; i < CPT; i++) {
            const int ch = tid + 256 * i, key = ch / CPR, dc = ch - key * CPR;
            *reinterpret_cast<u32x4*>(kt8 + key * KSB + dc * 16) = kr[i];
            const u32x2 b0 = codes_to_bf16(vr[i].x), b1 = codes_to_bf16(vr[i].y), b2 = codes_to_bf16(vr[i].z), b3 = codes_to_bf16(vr[i].w);
            const u32x4 lo = u32x4{b0.x, b0.y, b1.x, b1.y}, hi = u32x4{b2.x, b2.y, b3.x, b3.y};
            *reinterpret_cast<u32x4*>(vt + key * VSE + dc * 16) = lo;
            *reinterpret_cast<u32x4*>(vt + key * VSE + dc * 16 + 8) = hi;
        }
        if (tid < 2 * KT) kst[tid] = sr; /* vst = kst + KT */
    };

    f32x4 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; db++) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -__builtin_inff(), l = 0.f;

    tload(0);
    tstore();
    __syncthreads();
    for (int t = 0; t < ntile; t++) {
        const bool more = t + 1 < ntile;
        if (more) tload(t + 1);
        if (t < ntile_w) {
            // ---- the integer scores of the four sub-tiles
            i32x4 I[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                I[u] = i32x4{0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    const i32x4 A = *reinterpret_cast<const i32x4*>(kt8 + (16 * u + c) * KSB + 64 * s + 16 * h);
                    I[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, qreg[s], I[u], 0, 0, 0);
                }
            }
            // ---- score, exp2 parts, the tile's maximum exponent of this column
            float f[4][4], n[4][4], g[4][4];
            float mt = -__builtin_inff();
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const f32x4 ksv = *reinterpret_cast<const f32x4*>(kst + 16 * u + 4 * h), vsv = *reinterpret_cast<const f32x4*>(vst + 16 * u + 4 * h);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int key = t * KT + 16 * u + 4 * h + r;
                    const float cc = sq * ksv[r];
                    const float d = (float)I[u][r] * cc;
                    const float s = round_bf16(d * a.rden);
                    kf_exp2_parts(s * KF_LOG2E, f[u][r], n[u][r]);
                    g[u][r] = round_bf16(f[u][r] * vsv[r]); /* ONE fp32 multiply before the scaling, then the bf16 operand */
                    n[u][r] = key <= pos_q ? n[u][r] : -__builtin_inff(); /* a select: whatever a row past the position holds (NaN included) goes no further */
                    mt = fmaxf(mt, n[u][r]);
                }
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            if (mt > m) { /* exact rescale by a power of two; the first tile holds key 0 of every column, so m is finite from there on */
                const float sc = m == -__builtin_inff() ? 0.0f : __builtin_amdgcn_ldexpf(1.0f, (int)(m - mt));
                l *= sc;
#pragma unroll
                for (int db = 0; db < NDB; db++) o[db] *= sc;
                m = mt;
            }
            // ---- weights: p = f 2^(n - m) into L, gb 2^(n - m) as the bf16 B operand
            uint32_t pw[4][2];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                float gs[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const bool valid = n[u][r] != -__builtin_inff();
                    const int e = valid ? (int)(n[u][r] - m) : 0;
                    l += valid ? __builtin_amdgcn_ldexpf(f[u][r], e) : 0.0f;
                    gs[r] = valid ? __builtin_amdgcn_ldexpf(g[u][r], e) : 0.0f;
                }
                pw[u][0] = pack_bf16x2(gs[0], gs[1]), pw[u][1] = pack_bf16x2(gs[2], gs[3]);
            }
            // ---- O^T += V^T . P^T, two steps of 32 keys
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const u32x4 B = u32x4{pw[2 * w][0], pw[2 * w][1], pw[2 * w + 1][0], pw[2 * w + 1][1]};
#pragma unroll
                for (int db = 0; db < NDB; db++) {
                    // lane l16 of a 16-lane group addresses key-row (l16 >> 2) of its 4, d-piece 4 (l16 & 3) of the block's 16 d; it receives the 4 keys of d = l16
                    const uint16_t* vp = vt + (32 * w + 4 * h + (c >> 2)) * VSE + 16 * db + 4 * (c & 3);
                    const k8_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) k8_bf16x4*)(vp));
                    const k8_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) k8_bf16x4*)(vp + 16 * VSE));
                    const k8_bf16x8 A = k8_bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(k8_bf16x8, B), o[db], 0, 0, 0);
                }
            }
        }
        __syncthreads(); /* every wave is done with the tile */
        if (more) {
            tstore();
            __syncthreads();
        }
    }
    // ---- out[col][d] = O^T[d][col] / L; lane (c, h) holds d = 16 db + 4 h + {0..3}
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (!col_ok) return;
    uint16_t* orow = a.out + (size_t)tok * a.q_stride + (size_t)(kvh * GQ + hq) * HD + 4 * h;
#pragma unroll
    for (int db = 0; db < NDB; db++) {
        const uint32_t w0 = pack_bf16x2(__fdiv_rn(o[db][0], l), __fdiv_rn(o[db][1], l)), w1 = pack_bf16x2(__fdiv_rn(o[db][2], l), __fdiv_rn(o[db][3], l));
        *reinterpret_cast<u32x2*>(orow + 16 * db) = u32x2{w0, w1};
    }
}

using ApKv8Kernel = void (*)(AttnPrefillKv8Args);
int attn_prefill_kv8_launch(hipStream_t st, AttnPrefillKv8Args& a, const AttnPlan& p) {
    if (p.status != KF_OK) return p.status;
    if (p.route != ATTN_TILE_KV8 || p.kt != APK8_KT || p.threads != 256) return KF_INTERNAL_ERR;
    static constexpr ApKv8Kernel forms[2][4] = {
        {attn_prefill_kv8_kernel<64, 1>, attn_prefill_kv8_kernel<64, 2>, attn_prefill_kv8_kernel<64, 4>, attn_prefill_kv8_kernel<64, 8>},
        {attn_prefill_kv8_kernel<128, 1>, attn_prefill_kv8_kernel<128, 2>, attn_prefill_kv8_kernel<128, 4>, attn_prefill_kv8_kernel<128, 8>}};
    if ((p.hd != 64 && p.hd != 128) || p.gq < 1 || p.gq > 8 || (p.gq & (p.gq - 1))) return KF_INTERNAL_ERR; /* a form attn_plan never names */
    a.rden = 1.0f / sqrtf((float)p.hd);
    void* args[] = {&a};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(forms[p.hd == 128][__builtin_ctz(p.gq)]), dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(p.threads), args, (size_t)p.lds, st);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
