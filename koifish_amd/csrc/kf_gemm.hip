// kf_gemm.hip -- fused PackedQ unpack + MFMA GEMM for a batch of tokens (prefill, SLP::Forw with nToken > 1), gfx950 / wave64.
//
// Reference: SLP::Forw (NeuronFuse.cu:305-381) -> GTensor::GetDataX dequantises the WHOLE weight to bf16 in gBUFF->tmpTernary
// (quantizer.cu:249-392), then cuBLASLt multiplies (gemm.cu:93-214); Fish::Chat feeds the prompt one token at a time through it
// (GoPT.cpp:1139-1146).  Here y[n, M] = x[n, K] . W[M, K]^T reads the packed stream once per 128-token tile, dequantises 8 weights
// per lane in registers with the reference's bf16-stepwise arithmetic (T.cu:274) straight into an MFMA A-fragment, and contracts on
// v_mfma_f32_32x32x16_bf16 against x fragments staged through LDS.
//
// Fragment mapping (cdna_hip_programming.md section 3): for the 32x32x16 bf16 MFMA lane l (r = l & 31, h = l >> 5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r], j = 0..7; D has col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h.
// A = weights (rows = output features), B = x^T (cols = tokens).  The contraction index may be visited in any order as long as A and B
// agree, so the two lane halves do not take k and k+8 of one 16-wide step: over a staged tile of 128 k, half h owns whole 16-byte
// packed blocks (4-bit: blocks 2p + h; 2-bit: block h; 1-bit: the 8-byte half h of the block; bf16 / f8: the same element ranges) and
// walks them 8 elements per MFMA step.  Every lane therefore issues plain 16-byte (8-byte for 1-bit) loads of the packed stream and
// never exchanges data with another lane; the x fragment of a step is read from LDS at the matching element offset.
//
// Workgroup = 4 waves = RBW row blocks of 32 output rows x KS halves of the staged k tile (KS = 1: 128 rows; KS = 2: 64 rows, each k
// half on its own wave, partial sums combined through LDS in a fixed order).  Grid = (row tiles, 128-token tiles).
// fp32 accumulation inside the MFMA, one bf16 round-to-nearest store; the epilogue is linear_out_bf16 (kf_device.h: alpha, beta*y, bias, store,
// residual add + store), called by gemm_epilogue and by the direct kernel's reduce tail.  Differs from the token-serial mat-vec only in fp32 summation order.
// Every storage format has its own WTile body (load, frag(sl, a, ks)) over one of two element ranges, koff_unit / koff_half; a common load shell for the five
// unit formats was tried and is not here: DESIGN.md section 4.0.
#include <stdlib.h>
#include <string.h>

#include "kf_gemm_common.h"

namespace kf {

// ---- the weights one lane needs for one staged tile: NS = 8 / KS MFMA steps
// step sl of wave-half ks: elements [koff, koff + 8) of the 128-wide tile
template <int FMT, int KS>
struct WTile;
// the two element ranges, stated once.  Unit formats (32 weights per unit: 4-bit, the row forms, bf16, f8): pair P = ks * NP + p (NP = 2 / KS), lane half h owns
// elements (2P + h) * 32 .. + 32.  2-bit / 1-bit (blocks of 64 / 128): lane half h owns 64 elements, global step s = ks * NS + sl covers its elements 8s .. 8s + 7
template <int KS>
__device__ __forceinline__ int koff_unit(int sl, int h, int ks) { return (2 * (ks * (2 / KS) + (sl >> 2)) + h) * 32 + 8 * (sl & 3); }
template <int KS>
__device__ __forceinline__ int koff_half(int sl, int h, int ks) { return 64 * h + 8 * (ks * (8 / KS) + sl); }

template <int KS>
struct WTile<FMT_Q4, KS> {
    static constexpr int NP = 2 / KS;
    u32x4 b[NP];
    uint16_t st[NP], ze[NP]; /* raw bf16 bits: converted at use, so that nothing waits on the loads right behind their issue */
    bool in[NP];
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int ks) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            // a row's last staged tile may be half empty (K a multiple of 64 only): blocks past the row end are read from the last valid
            // block (no branch around the load) and given step = zero = 0, which unpacks to weights of 0
            int bi = it * 4 + 2 * (ks * NP + p) + h;
            const bool in_row = bi < a.nBlk;
            if (!in_row) bi = a.nBlk - 1;
            const uint32_t bidx = (uint32_t)row * (uint32_t)a.nBlk + (uint32_t)bi;
            b[p] = ld_nt(reinterpret_cast<const u32x4*>(a.w) + bidx);
            const uint32_t gi = bidx >> a.gshift;
            st[p] = a.step[gi], ze[p] = a.zero[gi], in[p] = in_row;
        }
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_unit<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs& a, int) const {
        const int p = sl >> 2, c = sl & 3;
        const uint32_t D = c == 0 ? b[p].w : (c == 1 ? b[p].z : (c == 2 ? b[p].y : b[p].x));
        const float s = in[p] ? bf2f(st[p]) : 0.f, z = in[p] ? bf2f(ze[p]) : 0.f;
        return frag_q4(D, s, s * 0.0625f, -a.qBias * s, z);
    }
};
// 4-bit row codebook: the same block ranges as the Packed128 form; the row's 16-entry table rides along (two 16-byte loads through the cache)
template <int KS>
struct WTile<FMT_Q4R, KS> {
    static constexpr int NP = 2 / KS;
    u32x4 b[NP];
    u32x4 ta, tb;
    bool in[NP];
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int ks) {
        const u32x4* lt = reinterpret_cast<const u32x4*>(a.zero) + 2 * (size_t)row; /* a.zero carries the table base */
        ta = lt[0], tb = lt[1];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            int bi = it * 4 + 2 * (ks * NP + p) + h;
            const bool in_row = bi < a.nBlk;
            if (!in_row) bi = a.nBlk - 1;
            b[p] = ld_nt(reinterpret_cast<const u32x4*>(a.w) + (uint32_t)row * (uint32_t)a.nBlk + (uint32_t)bi);
            in[p] = in_row;
        }
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_unit<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs&, int) const {
        const int p = sl >> 2, c = sl & 3;
        const uint32_t D = c == 0 ? b[p].x : (c == 1 ? b[p].y : (c == 2 ? b[p].z : b[p].w)); /* stream order: dword 0 holds elements 0..7 */
        const u32x4 o = frag_q4r(D, ta, tb);
        const uint32_t keep = in[p] ? 0xffffffffu : 0u;
        return u32x4{o.x & keep, o.y & keep, o.z & keep, o.w & keep};
    }
};
// 3- / 2-bit row forms (kf_set_row_unpack): the units of 32 weights take the place of the 4-bit row codebook's blocks -- the same element ranges per lane, the same
// fragments as frag_q4r forms from the nibble stream of the same ids -- in 12 / 8 bytes each; the row's 8 / 4 entries (row RTN: its (zero, step)) ride along
template <int FMT, int KS>
struct WTileRowQ {
    static constexpr int NP = 2 / KS, BITS = FMT == FMT_Q3R ? 3 : 2, UB = rowq_unit_bytes(FMT);
    u32x4 b[NP];
    u32x4 ta;
    bool in[NP];
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int ks) {
        if constexpr (FMT == FMT_Q3R) ta = reinterpret_cast<const u32x4*>(a.zero)[row]; /* a.zero carries the table base */
        else if constexpr (FMT == FMT_Q2R) {
            const u32x2 v = reinterpret_cast<const u32x2*>(a.zero)[row];
            ta = u32x4{v.x, v.y, 0u, 0u};
        } else ta = u32x4{reinterpret_cast<const uint32_t*>(a.zero)[row], 0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < NP; p++) {
            int bi = it * 4 + 2 * (ks * NP + p) + h;
            const bool in_row = bi < a.nBlk;
            if (!in_row) bi = a.nBlk - 1;
            b[p] = ld_unit<UB>(a.w + ((size_t)row * (size_t)a.nBlk + (size_t)bi) * UB);
            in[p] = in_row;
        }
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_unit<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs&, int) const {
        const int p = sl >> 2, c = sl & 3;
        const RowTab t = FMT == FMT_Q2N ? row_tab_rtn(ta.x) : row_tab<(1 << BITS)>(ta);
        const u32x4 o = row_pairs8<BITS>(row_unit_ids8<BITS>(b[p], c), t);
        const uint32_t keep = in[p] ? 0xffffffffu : 0u;
        return u32x4{o.x & keep, o.y & keep, o.z & keep, o.w & keep};
    }
};
template <int KS>
struct WTile<FMT_Q3R, KS> : WTileRowQ<FMT_Q3R, KS> {};
template <int KS>
struct WTile<FMT_Q2R, KS> : WTileRowQ<FMT_Q2R, KS> {};
template <int KS>
struct WTile<FMT_Q2N, KS> : WTileRowQ<FMT_Q2N, KS> {};
template <int KS>
struct WTile<FMT_BF16, KS> {
    static constexpr int NP = 2 / KS;
    u32x4 b[NP][4];
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int ks) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            int e = it * GM_KT + (2 * (ks * NP + p) + h) * 32; /* first of this lane's 32 elements; past the row end: zeros (address clamped) */
            const uint32_t keep = e < a.K ? 0xffffffffu : 0u;
            if (e >= a.K) e = a.K - 32;
            const u32x4* src = reinterpret_cast<const u32x4*>(a.w + ((size_t)row * a.K + (size_t)e) * 2);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const u32x4 v = ld_nt(src + c);
                b[p][c] = u32x4{v.x & keep, v.y & keep, v.z & keep, v.w & keep};
            }
        }
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_unit<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs&, int) const { return b[sl >> 2][sl & 3]; }
};
template <int KS>
struct WTile<FMT_F8, KS> {
    static constexpr int NP = 2 / KS;
    u32x4 b[NP][2];
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int ks) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            int e = it * GM_KT + (2 * (ks * NP + p) + h) * 32;
            const uint32_t keep = e < a.K ? 0xffffffffu : 0u;
            if (e >= a.K) e = a.K - 32;
            const u32x4* src = reinterpret_cast<const u32x4*>(a.w + (size_t)row * a.K + (size_t)e);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const u32x4 v = ld_nt(src + c);
                b[p][c] = u32x4{v.x & keep, v.y & keep, v.z & keep, v.w & keep};
            }
        }
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_unit<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs&, int) const {
        const int p = sl >> 2, c = sl & 3;
        const u32x4 v = b[p][c >> 1];
        return (c & 1) ? frag_f8(v.z, v.w) : frag_f8(v.x, v.y);
    }
};
// 2-bit: the staged tile is two 64-element blocks, lane half h owns block h
template <int KS>
struct WTile<FMT_Q2, KS> {
    u32x4 b;
    uint16_t st, ze;
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int) {
        const uint32_t bidx = (uint32_t)row * (uint32_t)a.nBlk + (uint32_t)(it * 2 + h);
        b = ld_nt(reinterpret_cast<const u32x4*>(a.w) + bidx);
        const uint32_t gi = bidx >> a.gshift;
        st = a.step[gi], ze = a.zero[gi];
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_half<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs& a, int ks) const {
        const uint32_t dw[4] = {b.w, b.z, b.y, b.x}; /* dword3 holds elements 0..15 */
        uint32_t D = dw[sl >> 1];
        if (KS == 2) D = ks ? dw[2 + (sl >> 1)] : D;
        const uint32_t v = (sl & 1) ? (D & 0xffffu) : (D >> 16);
        const float s = bf2f(st);
        return frag_q2(v, s, -a.qBias * s, bf2f(ze));
    }
};
// 1-bit: the staged tile is one 128-element block, lane half h owns its 8-byte half (elements 64h .. 64h+63)
template <int KS>
struct WTile<FMT_Q1, KS> {
    u32x2 b; /* b.y: first 32 elements of the half, b.x: next 32 */
    uint16_t st, ze;
    __device__ __forceinline__ void load(const GemmArgs& a, int row, int it, int h, int) {
        const uint32_t bidx = (uint32_t)row * (uint32_t)a.nBlk + (uint32_t)it;
        b = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(a.w) + (size_t)bidx * 2 + (1 - h));
        const uint32_t gi = bidx >> a.gshift;
        st = a.step[gi], ze = a.zero[gi];
    }
    static __device__ __forceinline__ int koff(int sl, int h, int ks) { return koff_half<KS>(sl, h, ks); }
    __device__ __forceinline__ u32x4 frag(int sl, const GemmArgs& a, int ks) const {
        const uint32_t D = (KS == 2) ? (ks ? b.x : b.y) : ((sl >> 2) ? b.x : b.y);
        const uint32_t byte = (D >> (24 - 8 * (sl & 3))) & 0xffu;
        const float s = bf2f(st), z = bf2f(ze), nb = -a.qBias * s; /* dequant(0), dequant(1): loop-invariant, hoisted by the compiler */
        const uint32_t r = pack_bf16x2(fmaf(0.0f, s, nb), fmaf(1.0f, s, nb));
        const uint32_t ww = pack_bf16x2(bf_lo(r) - z, bf_hi(r) - z);
        return frag_q1(byte, ww & 0xffffu, ww >> 16);
    }
};

template <int FMT, int KS>
__global__ void __launch_bounds__(256) gemm_kernel(const GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint16_t* xs = reinterpret_cast<uint16_t*>(smem_raw); /* 2 x [GM_TOK][GM_XS] bf16; reused as the k-half combine buffer at the end */
    constexpr int RBW = 4 / KS, NS = 8 / KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int rb = wave % RBW, ks = wave / RBW;
    const int row_base = (blockIdx.x * RBW + rb) * 32;
    int row = row_base + r;
    if (row >= a.M) row = a.M - 1; /* rows past the end recompute the last row; their results are not stored */
    const int tok0 = blockIdx.y * GM_TOK;
    const int nit = (a.K + GM_KT - 1) / GM_KT;

    f32x16 acc[4];
#pragma unroll
    for (int tb = 0; tb < 4; tb++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[tb][i] = 0.f;

    // x staging: 16 threads cover one token row of 256 B, 16 rows per pass, 8 passes
    const int trow = tid >> 4, seg = tid & 15;
    u32x4 xr[8];
    auto xload = [&](int it) {
#pragma unroll
        for (int p = 0; p < 8; p++) {
            int tok = tok0 + p * 16 + trow;
            if (tok >= a.n) tok = a.n - 1; /* rows past the batch repeat the last token: loaded unconditionally, never stored */
            int col = it * GM_KT + seg * 8;
            if (col >= a.K) col = a.K - 8; /* half-empty last tile: the weights there are 0, any finite x will do */
            xr[p] = *reinterpret_cast<const u32x4*>(a.x + (size_t)tok * a.ldx + col);
        }
    };
    auto xstore = [&](int buf) {
        uint16_t* dst = xs + (size_t)buf * GM_TOK * GM_XS;
#pragma unroll
        for (int p = 0; p < 8; p++) *reinterpret_cast<u32x4*>(dst + (p * 16 + trow) * GM_XS + seg * 8) = xr[p];
    };

    // Two tiles in flight: while tile `it` is multiplied out of LDS, tile it+1 waits in registers (loaded during the previous iteration,
    // written to the other LDS buffer at the end of this one) and tile it+2's loads are issued -- a load has a whole iteration of
    // arithmetic plus a barrier to land before anything waits for it (one tile ahead left ~2 us of latency exposed per iteration).
    WTile<FMT, KS> wc, w1, w2;
    u32x4 xr2[8];
    auto xload2 = [&](int it) {
#pragma unroll
        for (int p = 0; p < 8; p++) {
            int tok = tok0 + p * 16 + trow;
            if (tok >= a.n) tok = a.n - 1;
            int col = it * GM_KT + seg * 8;
            if (col >= a.K) col = a.K - 8;
            xr2[p] = *reinterpret_cast<const u32x4*>(a.x + (size_t)tok * a.ldx + col);
        }
    };
    wc.load(a, row, 0, h, ks);
    xload(0);
    xstore(0);
    // every load below is unconditional (past the last tile the last one is simply fetched again): with branches around them hipcc
    // cannot count the loads in flight and falls back to s_waitcnt vmcnt(0), which waits for the NEWEST tile as well
    {
        const int i1 = nit > 1 ? 1 : 0;
        w1.load(a, row, i1, h, ks);
        xload(i1);
    }
    __syncthreads();
    for (int it = 0; it < nit; it++) {
        const bool more = it + 1 < nit, more2 = true;
        {
            const int i2 = it + 2 < nit ? it + 2 : nit - 1;
            w2.load(a, row, i2, h, ks);
            xload2(i2);
        }
        const uint16_t* xb = xs + (size_t)(it & 1) * GM_TOK * GM_XS;
        // x fragments of step sl+1 are read from LDS while the weights of step sl are unpacked and multiplied (read just before
        // each MFMA, every ds_read_b128 round trip sat in front of its MFMA)
        u32x4 Bc[4], Bn[4];
        {
            const int ko = WTile<FMT, KS>::koff(0, h, ks);
#pragma unroll
            for (int tb = 0; tb < 4; tb++) Bc[tb] = *reinterpret_cast<const u32x4*>(xb + (tb * 32 + r) * GM_XS + ko);
        }
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            if (sl + 1 < NS) {
                const int ko = WTile<FMT, KS>::koff(sl + 1, h, ks);
#pragma unroll
                for (int tb = 0; tb < 4; tb++) Bn[tb] = *reinterpret_cast<const u32x4*>(xb + (tb * 32 + r) * GM_XS + ko);
            }
            __builtin_amdgcn_sched_barrier(0); /* keep the reads up here: left alone, the scheduler sinks each one next to its MFMA */
            const bf16x8 A = __builtin_bit_cast(bf16x8, wc.frag(sl, a, ks));
#pragma unroll
            for (int tb = 0; tb < 4; tb++) acc[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(bf16x8, Bc[tb]), acc[tb], 0, 0, 0);
#pragma unroll
            for (int tb = 0; tb < 4; tb++) Bc[tb] = Bn[tb];
        }
        if (more) {
            xstore((it + 1) & 1);
            wc = w1;
        }
        if (more2) {
            w1 = w2;
#pragma unroll
            for (int p = 0; p < 8; p++) xr[p] = xr2[p];
        }
        __syncthreads();
    }

    if (KS == 2) { /* the k-halves of a row block: upper half hands its sums over, fixed order (lower + upper) */
        float* red = reinterpret_cast<float*>(smem_raw);
        if (ks == 1) {
#pragma unroll
            for (int tb = 0; tb < 4; tb++)
#pragma unroll
                for (int i = 0; i < 16; i++) red[((rb * 4 + tb) * 16 + i) * 64 + lane] = acc[tb][i];
        }
        __syncthreads();
        if (ks == 1) return;
#pragma unroll
        for (int tb = 0; tb < 4; tb++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[tb][i] = acc[tb][i] + red[((rb * 4 + tb) * 16 + i) * 64 + lane];
    }

    gemm_epilogue<4>(acc, a, tok0, row_base, r, h);
}

// ---- small token counts: every wave is independent.  Workgroup = one block of 32 output rows x TB*32 tokens; its NW waves split k in
// groups of UPG consecutive 64-element units (for 2-bit / 1-bit: halves of a 128-element unit): wave w takes groups w, w + NW, ...,
// reads its x fragments straight from global memory (x is n*K*2 bytes: L2-resident) and meets the others once, at the end, where
// wave 0 adds the sums in wave order.  All loads of a group are issued before any of its arithmetic and the next group's loads before
// the current group's arithmetic: the prompt-sized GEMMs of a 0.6B model are latency-bound (a 1024 x 1024 4-bit matrix is 0.5 MB,
// far fewer waves than SIMDs), so the k loop is kept as short as the register file allows (K = 1024: one group per wave, no loop).
// PAIRED: the workgroup multiplies the same x fragments against TWO matrices (gate, up) and stores silu(gate) * up: the bf16 stores of
// gate and up and the SwiGLU expression are the ones of the separate launches (kf_linear x 2 + kf_swiglu), so the result is bit-identical.
// Otherwise a launch may carry up to three matrices that share x (Q, K, V): blockIdx.x walks their 32-row blocks one job after the other.
template <int FMT, int TB, int UPG, int NW, bool PAIRED>
__global__ void __launch_bounds__(NW * 64) gemm_direct_kernel(const GemmArgs a0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* red = reinterpret_cast<float*>(smem_raw); /* [PAIRED ? 2 : 1][NW][TB][16][64] */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    GemmArgs a = a0;
    int rb = blockIdx.x;
    if (!PAIRED && a0.njobs > 1 && rb >= a0.rb_end[0]) { /* workgroup-uniform: the fields below stay scalar */
        const bool j2 = a0.njobs > 2 && rb >= a0.rb_end[1];
        rb -= j2 ? a0.rb_end[1] : a0.rb_end[0];
        a.w = j2 ? a0.xw[1] : a0.xw[0];
        a.zero = j2 ? a0.xzero[1] : a0.xzero[0];
        a.step = j2 ? a0.xstep[1] : a0.xstep[0];
        a.qBias = j2 ? a0.xqBias[1] : a0.xqBias[0];
        a.M = j2 ? a0.xM[1] : a0.xM[0];
        a.y = j2 ? a0.xy[1] : a0.xy[0];
        a.ldy = j2 ? a0.xldy[1] : a0.xldy[0];
    }
    GemmArgs b = a0; /* PAIRED: the second matrix */
    if (PAIRED) b.w = a0.xw[0], b.zero = a0.xzero[0], b.step = a0.xstep[0], b.qBias = a0.xqBias[0];
    const int row_base = rb * 32;
    int row = row_base + r;
    if (row >= a.M) row = a.M - 1;
    const int tok0 = blockIdx.y * (TB * 32);
    const int nunit = a.K / 64;

    f32x16 acc[TB], acc2[PAIRED ? TB : 1];
#pragma unroll
    for (int tb = 0; tb < TB; tb++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
            acc[tb][i] = 0.f;
            if (PAIRED) acc2[tb][i] = 0.f;
        }

    // x rows of this lane's tokens (rows past n read row n-1: their results are not stored)
    const uint16_t* xrow[TB];
#pragma unroll
    for (int tb = 0; tb < TB; tb++) {
        int tok = tok0 + tb * 32 + r;
        if (tok >= a.n) tok = a.n - 1;
        xrow[tb] = a.x + (size_t)tok * a.ldx;
    }
    struct Group {
        WTile<FMT, 2> w[UPG];
        WTile<FMT, 2> w2[PAIRED ? UPG : 1];
        u32x4 x[UPG][4][TB];
    };
    auto gload = [&](int u0, Group& g) { /* units u0 .. u0+UPG-1; units past the end repeat the last one and are skipped in the arithmetic */
#pragma unroll
        for (int j = 0; j < UPG; j++) {
            int u = u0 + j;
            if (u >= nunit) u = nunit - 1;
            const int it = u >> 1, ks = u & 1;
            g.w[j].load(a, row, it, h, ks);
            if (PAIRED) g.w2[j].load(b, row, it, h, ks);
#pragma unroll
            for (int sl = 0; sl < 4; sl++) {
                const int ko = it * GM_KT + WTile<FMT, 2>::koff(sl, h, ks);
#pragma unroll
                for (int tb = 0; tb < TB; tb++) g.x[j][sl][tb] = *reinterpret_cast<const u32x4*>(xrow[tb] + ko);
            }
        }
    };
    Group gc, gn;
    int u0 = wave * UPG;
    if (u0 < nunit) gload(u0, gc);
    for (; u0 < nunit; u0 += NW * UPG) {
        const bool more = u0 + NW * UPG < nunit;
        if (more) gload(u0 + NW * UPG, gn);
#pragma unroll
        for (int j = 0; j < UPG; j++) {
            if (u0 + j < nunit) {
#pragma unroll
                for (int sl = 0; sl < 4; sl++) {
                    const bf16x8 A = __builtin_bit_cast(bf16x8, gc.w[j].frag(sl, a, (u0 + j) & 1));
#pragma unroll
                    for (int tb = 0; tb < TB; tb++)
                        acc[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(bf16x8, gc.x[j][sl][tb]), acc[tb], 0, 0, 0);
                    if (PAIRED) {
                        const bf16x8 A2 = __builtin_bit_cast(bf16x8, gc.w2[j].frag(sl, b, (u0 + j) & 1));
#pragma unroll
                        for (int tb = 0; tb < TB; tb++)
                            acc2[tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A2, __builtin_bit_cast(bf16x8, gc.x[j][sl][tb]), acc2[tb], 0, 0, 0);
                    }
                }
            }
        }
        if (more) gc = gn;
    }
    // fixed-order sum over the k-slices, ((w0 + w1) + w2) + ..., and the epilogue, spread over the waves: every wave leaves its 16 sums per token block in LDS and
    // wave w adds and stores accumulator registers 16 w / NW .. (two adjacent output rows per lane with 8 waves) -- the same additions in the same order as one wave
    // doing all of it, at an eighth of the serial work behind the barrier (measured on the 0.6B shapes at 128 tokens: reduce 0.65 us + epilogue 1.3-1.7 us by wave 0)
    constexpr int RPW = 16 / NW; /* registers per wave */
    static_assert(NW == 8 || NW == 4, "registers per wave: pairs of adjacent rows");
#pragma unroll
    for (int tb = 0; tb < TB; tb++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
            red[((wave * TB + tb) * 16 + i) * 64 + lane] = acc[tb][i];
            if (PAIRED) red[(((NW + wave) * TB + tb) * 16 + i) * 64 + lane] = acc2[tb][i];
        }
    __syncthreads();
#pragma unroll
    for (int tb = 0; tb < TB; tb++) {
        const int tok = tok0 + tb * 32 + r;
#pragma unroll
        for (int q = 0; q < RPW; q += 2) {
            const int i0 = wave * RPW + q; /* registers i0, i0 + 1: rows rg, rg + 1 */
            float v[2] = {0.f, 0.f}, v2[2] = {0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NW; w++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float p = red[((w * TB + tb) * 16 + i0 + j) * 64 + lane];
                    v[j] = w == 0 ? p : v[j] + p;
                    if (PAIRED) {
                        const float p2 = red[(((NW + w) * TB + tb) * 16 + i0 + j) * 64 + lane];
                        v2[j] = w == 0 ? p2 : v2[j] + p2;
                    }
                }
            const int rg = row_base + 8 * (i0 >> 2) + 4 * h + (i0 & 3);
            if (tok >= a.n || rg >= a.M) continue;
            uint16_t o[2] = {0, 0};
            uint16_t* yp = a.y + (size_t)tok * a.ldy + rg;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (rg + j >= a.M) continue;
                if (!PAIRED) {
                    o[j] = linear_out_bf16(v[j], a.alpha, a.beta, yp, j, a.bias, rg + j, a.residual, (size_t)tok * a.ldr + rg + j);
                } else { /* act = silu(gate) * up on the bf16-rounded gate / up (Relu::Forw SWIG, Activation.cu:85-93; the expression of kf_swiglu) */
                    const float g = round_bf16(v[j]), u = round_bf16(v2[j]);
                    o[j] = swiglu_bf16(g, u);
                }
            }
            if (((a.ldy & 1) == 0) && ((reinterpret_cast<uintptr_t>(a.y) & 3) == 0) && rg + 1 < a.M) {
                *reinterpret_cast<uint32_t*>(yp) = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
            } else {
                yp[0] = o[0];
                if (rg + 1 < a.M) yp[1] = o[1];
            }
        }
    }
}

template <int FMT>
static void gm_launch(const GemmKern& k, const GemmArgs& a, hipStream_t st) {
    const dim3 grid(k.gx, k.gy), block(k.block);
    if (k.fam == GK_PAIRED) /* paired SwiGLU */
        hipLaunchKernelGGL((gemm_direct_kernel<FMT, 1, GD_UPG, GD_NW, true>), grid, block, k.lds, st, a);
    else if (k.fam == GK_DIRECT && k.form == 64) /* 64-token tiles: every weight block is unpacked for two token blocks */
        hipLaunchKernelGGL((gemm_direct_kernel<FMT, 2, GD_UPG, GD_NW, false>), grid, block, k.lds, st, a);
    else if (k.fam == GK_DIRECT)
        hipLaunchKernelGGL((gemm_direct_kernel<FMT, 1, GD_UPG, GD_NW, false>), grid, block, k.lds, st, a);
    else if (k.form == 2)
        hipLaunchKernelGGL((gemm_kernel<FMT, 2>), grid, block, k.lds, st, a);
    else
        hipLaunchKernelGGL((gemm_kernel<FMT, 1>), grid, block, k.lds, st, a);
}
// the executor of every family: kf_gemm3.hip, kf_gemm2.hip, or this file's direct / paired / staged kernels
static int gemm_run(hipStream_t st, const GemmKern& k, const GemmArgs& a, void* ws) {
    if (k.fam == GK_G3) return gemm3_run(st, k, a, ws);
    if (k.fam == GK_G2) return gemm2_run(st, k, a);
    switch (k.fmt) {
        case FMT_BF16: gm_launch<FMT_BF16>(k, a, st); break;
        case FMT_F8: gm_launch<FMT_F8>(k, a, st); break;
        case FMT_Q4: gm_launch<FMT_Q4>(k, a, st); break;
        case FMT_Q2: gm_launch<FMT_Q2>(k, a, st); break;
        case FMT_Q4R: gm_launch<FMT_Q4R>(k, a, st); break;
        case FMT_Q3R: gm_launch<FMT_Q3R>(k, a, st); break;
        case FMT_Q2R: gm_launch<FMT_Q2R>(k, a, st); break;
        case FMT_Q2N: gm_launch<FMT_Q2N>(k, a, st); break;
        default: gm_launch<FMT_Q1>(k, a, st); break;
    }
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

GmWeight gm_operand(const kf_weight* w, const GemmKern& k) {
    GmWeight g = gm_bf16(w->data, w->ne0, w->ne1);
    g.qBias = (float)w->qBias;
    if (k.fmt == FMT_Q4R || fmt_rowq(k.fmt)) {
        g.zero = w->gama + w->ne0 + w->ne1; /* the rows' tables */
    } else if (k.fmt >= FMT_Q4) {
        g.zero = w->gama + w->ne0 + w->ne1;
        g.step = g.zero + (size_t)g.M * g.K / w->lGroup;
    }
    return g;
}
static void gm_base(GemmArgs& a, const GemmKern& k, const GmWeight& g, const uint16_t* x, long long ldx, int n, uint16_t* y, long long ldy) {
    memset(&a, 0, sizeof(a));
    a.w = g.w, a.zero = g.zero, a.step = g.step, a.qBias = g.qBias;
    a.M = g.M, a.K = g.K, a.nBlk = g.K / (fmt_rowq(k.fmt) ? 32 : GM_EPB[k.fmt]), a.gshift = k.gshift;
    a.x = x, a.ldx = ldx, a.n = n, a.y = y, a.ldy = ldy, a.alpha = 1.0f, a.njobs = 1;
    a.rb_end[0] = a.rb_end[1] = a.rb_end[2] = (g.M + 31) / 32;
}

int gemm_multi_launch(hipStream_t st, const GemmKern& k, int n_w, const GmWeight* g, const uint16_t* x, long long ldx, int n, uint16_t* const* y) {
    GemmArgs a;
    gm_base(a, k, g[0], x, ldx, n, y[0], g[0].M);
    if (k.fam == GK_PAIRED) {
        a.xw[0] = g[1].w, a.xzero[0] = g[1].zero, a.xstep[0] = g[1].step, a.xqBias[0] = g[1].qBias;
        return gemm_run(st, k, a, nullptr);
    }
    a.njobs = n_w;
    int end = 0;
    for (int i = 0; i < 3; i++) {
        if (i < n_w) end += (g[i].M + 31) / 32;
        a.rb_end[i] = end;
        if (i >= 1 && i < n_w)
            a.xw[i - 1] = g[i].w, a.xzero[i - 1] = g[i].zero, a.xstep[i - 1] = g[i].step, a.xqBias[i - 1] = g[i].qBias, a.xM[i - 1] = g[i].M, a.xy[i - 1] = y[i],
                     a.xldy[i - 1] = g[i].M;
    }
    return gemm_run(st, k, a, nullptr);
}

int gemm_launch(hipStream_t st, const GemmKern& k, const GmWeight& g, const uint16_t* x, long long ldx, int n, uint16_t* y, long long ldy, const uint16_t* bias, float alpha,
                float beta, const uint16_t* residual, long long ldr, void* ws) {
    GemmArgs a;
    gm_base(a, k, g, x, ldx, n, y, ldy);
    a.bias = bias, a.residual = residual, a.ldr = ldr, a.alpha = alpha, a.beta = beta;
    return gemm_run(st, k, a, ws);
}

}  // namespace kf
