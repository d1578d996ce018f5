// kf_gemm3_tile.h -- the global_load_lds operand tiles and the two-buffer k-loop of kf_gemm3.hip, shared with the kernels that put another epilogue on the same
// accumulator tiles (kf_head_score.hip: the LM head with the log-softmax in its epilogue).  Device code only.
#pragma once
#include <type_traits>

#include "kf_gemm_common.h"

namespace kf {

// G3Cfg (kf_gemm_plan.h): the workgroup tiles -- 256 x 256 (Big), 128 x 128 (Small), 64 x 128 (Mid), 64 x 64 (Tiny), 192 x 256 (Wide)

// one operand tile (256 rows x 2 BK bytes) = BK / 2 wave instructions of 1 KiB; wave `wid` issues BK / 16 of them.  BK = 64: 8 rows per instruction, chunk c of row r
// at position c ^ ((r >> 1) & 7); BK = 32: 16 rows per instruction (64-byte rows), chunk c at position c ^ ((r >> 2) & 3) -- either way a fragment read
// (16 rows x one 16-byte chunk) touches all 64 banks once.
template <int BK, int NI>
__device__ __forceinline__ const uint16_t* g3_src(const uint16_t* __restrict__ src, long long ld, int row0, int nrows, int i, int wid, int lane) {
    constexpr int CPR = BK / 8, RPI = 64 / CPR; /* chunks per row, rows per instruction */
    const int j = wid * NI + i;
    const int r = j * RPI + lane / CPR, p = lane % CPR, c = BK == 64 ? p ^ ((r >> 1) & 7) : p ^ ((r >> 2) & 3);
    int gr = row0 + r;
    gr = gr < nrows ? gr : nrows - 1; /* rows past the end re-read the last row: their outputs are not stored */
    return src + (size_t)gr * ld + c * 8; /* + k0 per step */
}
template <int BK>
__device__ __forceinline__ bf16x8 g3_frag(const unsigned char* tile, int row, int c) {
    const int p = BK == 64 ? c ^ ((row >> 1) & 7) : c ^ ((row >> 2) & 3);
    return *reinterpret_cast<const bf16x8*>(tile + row * (2 * BK) + (p << 4));
}

// the same tile from a K-MAJOR operand (src[k][row], `row` contiguous: an activation or a weight as it lies in memory when the contraction runs over its ROWS --
// both GEMMs of SLP::Back): the LDS image is [BK k][ROWS rows] (512- or 256-byte k-rows), one wave instruction = two or four k-rows; its 32-byte blocks are XOR-swizzled by k & 3 and
// its 128-byte quarters by bit 3 of k, so that the transposing fragment read below (per 32 lanes: k-rows k .. k+3 and k+8 .. k+11, 32 bytes of each) touches all 64
// banks once (without the second term the two 16-lane halves meet in the same 32 banks: SQ_LDS_BANK_CONFLICT = 50 % of the LDS cycles, measured).
// ROWS = the tile's rows (256 or 128): a k-row of the image is 2 ROWS bytes = CPK chunks of 16 bytes, one wave instruction covers 64 / CPK k-rows, wave `wid` issues
// instructions NI wid .. NI wid + NI - 1 of the ROWS / 8
template <int BK, int ROWS, int NI>
__device__ __forceinline__ const uint16_t* g3_src_km(const uint16_t* __restrict__ src, long long ld, int row0, int nrows, int i, int wid, int lane) {
    constexpr int CPK = ROWS / 8, KPI = 64 / CPK;
    const int j = wid * NI + i;
    const int kr = j * KPI + lane / CPK, p = lane % CPK, c = p ^ ((kr & 3) << 1) ^ (((kr >> 3) & 1) << 3);
    int col = row0 + c * 8;
    col = col + 8 <= nrows ? col : (nrows - 8 > 0 ? nrows - 8 : 0); /* chunks past the end re-read the last whole chunk: their outputs are not stored (rows % 8 == 0) */
    return src + (size_t)kr * ld + col; /* + k0 * ld per step */
}
// fragment (8 consecutive k of row `row`, k = kbase .. kbase + 7) of a k-major tile: two ds_read_b64_tr_b16, each a 4 (k) x 16 (rows) block transposed across 16 lanes
// (lane i of the 16 receives D[(i >> 2) + 4 j][i & 3], scratch/dbg/ds_read_tr_probe.hip): lane l16 reads k-row kbase + (l16 >> 2), 8-byte piece l16 & 3 of the 16-row block
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
template <int ROWS>
__device__ __forceinline__ bf16x8 g3_frag_km(const unsigned char* tile, int rowblk16, int kbase, int l16) {
    bf16x4 h[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int k = kbase + 4 * t + (l16 >> 2);
        const int byte_in_row = (rowblk16 * 16 + 4 * (l16 & 3)) * 2, c = byte_in_row >> 4, p = c ^ ((k & 3) << 1) ^ (((k >> 3) & 1) << 3);
        h[t] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(tile + k * (2 * ROWS) + p * 16 + (byte_in_row & 8)));
    }
    return bf16x8{h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
}

// k-steps kt0 .. kt1 - 1 (of BK) of the output tile at (m0, t0) accumulated into acc (the caller zeroes it).  NST = 128 KiB / stage LDS buffers: the loads of step
// kt + NST - 1 are issued while step kt is multiplied and drained with a COUNTED s_waitcnt vmcnt + one raw s_barrier per step (a __syncthreads() would drain the loads
// in flight): BK = 64 -> 2 buffers; BK = 32 -> 4 buffers, three steps in flight (measured slower, see g3_run_c).  Also measured and dropped: the barrier moved into
// the middle of the step's MFMA stream (the last 16 MFMAs of a step held back behind it, the first fragments of the next step read under them): 979 TFLOP/s against
// 1000 on the forward shapes at 246 VGPRs, and the k-major forms spill; four waves of 128 x 128 outputs each (256 accumulator AGPRs, a third less LDS traffic per MFMA,
// the vendor library's shape): the compiler fills all 512 registers and still spills inside the loop, 228 TFLOP/s -- that form needs a hand-scheduled loop.
template <bool AKM, bool BKM, int BK, class C>
__device__ __forceinline__ void g3_mainloop(const GemmArgs& a, int m0, int t0, int kt0, int kt1, f32x4 (&acc)[C::MT][C::NT], unsigned char* smem_raw, int wid, int lane) {
    static_assert(BK == G3_BK, "two k-halves of 32 per step");
    constexpr int NST = 2, LPW = C::NIA + C::NIB; /* loads per wave and step */
    const int wm = wid / C::WN, wn = wid % C::WN;
    const uint16_t* const W = reinterpret_cast<const uint16_t*>(a.w);
    auto bufA = [&](int b) { return smem_raw + (size_t)b * C::STAGE; };
    auto bufB = [&](int b) { return smem_raw + (size_t)b * C::STAGE + C::BM * BK * 2; };
    // AKM: W is [K][M] with row stride a.ldr (re-used field: the residual is not served by the k-major forms); BKM: x is [K][n] with row stride a.ldx.
    // Per-lane source pointers are set up once; a step adds a uniform offset (a 64-bit multiply per load and step was a tenth of the loop's issue slots).
    const uint16_t *pa[C::NIA], *pb[C::NIB];
#pragma unroll
    for (int i = 0; i < C::NIA; i++) pa[i] = AKM ? g3_src_km<BK, C::BM, C::NIA>(W, a.ldr, m0, a.M, i, wid, lane) : g3_src<BK, C::NIA>(W, a.K, m0, a.M, i, wid, lane);
#pragma unroll
    for (int i = 0; i < C::NIB; i++) pb[i] = BKM ? g3_src_km<BK, C::BN, C::NIB>(a.x, a.ldx, t0, a.n, i, wid, lane) : g3_src<BK, C::NIB>(a.x, a.ldx, t0, a.n, i, wid, lane);
    const long long stepA = AKM ? (long long)BK * a.ldr : BK, stepB = BKM ? (long long)BK * a.ldx : BK;
    auto stage = [&](int kt, int b) {
        const long long oa = stepA * kt, ob = stepB * kt;
#pragma unroll
        for (int i = 0; i < C::NIA; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[i] + oa),
                                             (__attribute__((address_space(3))) void*)(bufA(b) + (wid * C::NIA + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < C::NIB; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb[i] + ob),
                                             (__attribute__((address_space(3))) void*)(bufB(b) + (wid * C::NIB + i) * 1024), 16, 0, 0);
    };
#pragma unroll
    for (int st = 0; st < NST - 1; st++)
        if (kt0 + st < kt1) stage(kt0 + st, st);
    const int r16 = lane & 15, q4 = lane >> 4;
    // the steps are unrolled by the NST buffers so that every LDS address of a step is base + an immediate
    auto step = [&](int kt, auto cur_c) {
        constexpr int cur = decltype(cur_c)::value;
        const int left = kt1 - 1 - kt; /* steps issued after kt that may stay in flight */
        if (NST >= 4 && left >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPW) : "memory");
        else if (NST >= 3 && left >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier(); /* step kt has landed for every wave, and every wave is done reading the buffer of step kt - 1: the next loads overwrite that one */
        if (kt + NST - 1 < kt1) stage(kt + NST - 1, (cur + NST - 1) % NST);
#pragma unroll
        for (int kk = 0; kk < BK / 32; kk++) {
            bf16x8 af[C::MT], bfr[C::NT];
#pragma unroll
            for (int nt = 0; nt < C::NT; nt++) {
                if constexpr (BKM) bfr[nt] = g3_frag_km<C::BN>(bufB(cur), wn * C::NT + nt, kk * 32 + 8 * q4, r16);
                else bfr[nt] = g3_frag<BK>(bufB(cur), wn * (16 * C::NT) + nt * 16 + r16, kk * 4 + q4);
            }
#pragma unroll
            for (int mt = 0; mt < C::MT; mt++) {
                if constexpr (AKM) af[mt] = g3_frag_km<C::BM>(bufA(cur), wm * C::MT + mt, kk * 32 + 8 * q4, r16);
                else af[mt] = g3_frag<BK>(bufA(cur), wm * (16 * C::MT) + mt * 16 + r16, kk * 4 + q4);
            }
#pragma unroll
            for (int mt = 0; mt < C::MT; mt++)
#pragma unroll
                for (int nt = 0; nt < C::NT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bfr[nt], acc[mt][nt], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    for (int kt = kt0; kt < kt1; kt += NST) {
        step(kt, std::integral_constant<int, 0>{});
        if (kt + 1 < kt1) step(kt + 1, std::integral_constant<int, 1>{});
    }
    __builtin_amdgcn_s_barrier(); /* a following segment's first loads must not overtake the last reads */
}

// bijective XCD remap: the blocks with equal blockIdx % 8 (one XCD under round-robin placement) get consecutive logical indices
__device__ __forceinline__ int g3_remap(int orig, int nwg) {
    const int q = nwg / 8, rr = nwg % 8, xcd = orig % 8;
    return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
}

}  // namespace kf
