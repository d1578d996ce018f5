// kf_muon.hip -- the Muon update of a hidden matrix W [ne0 = out][ne1 = in] (ne0 >= ne1), PIPE_Muon::CU_core (Optimizer.cu:498-583) restated for gfx950:
//   muon_momentum_kernel  CU_muon_mG (Optimizer.cu:93-109):  mG <- sr(mG + (1 - mu)(g - mG)),  X <- sr(g + mu (mG' - g)),  sum X^2
//   muon_prescale_kernel  X <- bf16(X + (alpha - 1) X),  alpha = 1 / (sqrt(sum X^2) + eps) formed on the device (the reference reads the sum back to the host: D2e)
//   n_iter x [ A = bf16(X^T X);  B = bf16(b A + bf16(c A A));  X' = bf16(a X + bf16(X B)) ]     the Newton-Schulz iteration, cublasGemmEx / cublasAxpyEx at Optimizer.cu:541-559
//   muon_apply_kernel     CU_muon_update (Optimizer.cu:111-131):  p <- sr((1 - lr wd) p + (-lr) X),  g <- 0,  sum p'^2 (wnorm^2)
// The reference's column-major X (m = ne1, n = ne0) is W^T: its A = X X^T is W^T W, [ne1, ne1].  isTrans is forced off there (Pipe.cpp:27); no transposed branch here.
//
// A, A A and B are SYMMETRIC: ns_gram_kernel computes only the tiles (i, j >= i) of them -- nt (nt + 1) / 2 workgroups, closed-form triangular index, no atomics -- and
// stores every finished element twice, at (r, c) and at (c, r); of a diagonal tile only the elements on and above the diagonal are stored (and mirrored), so both
// matrices are symmetric bit for bit whatever order the MFMA sums in.  X^T X contracts over the ROWS of X: both operands k-major (g3_src_km / g3_frag_km of
// kf_gemm3_tile.h, 128 x 128 tiles); A A = A A^T reads the symmetric A k-contiguous on 64 x 64 tiles (ne1 = 1600: 325 of them).  X B is a plain NT product on the
// 128 x 128 tile mainloop with the axpy in its epilogue, written to the other X buffer (ping-pong: no copy back).  Every axpy is fp32 multiply, fp32 add, one bf16 store.
//
// Sums of squares are deterministic: each workgroup of an elementwise kernel leaves one fp64 partial (its threads' sums joined in a fixed tree), and a one-workgroup
// follow-up adds the partials in workgroup order.  Products of bf16 values are exact in fp64.
#include "kf_gemm3_tile.h"

namespace kf {

constexpr int MUON_T = 512, MUON_EPT = 8, MUON_PER_WG = MUON_T * MUON_EPT; /* TASKA_1p1 (packedN.cuh:612-643): 512 threads x 8 bf16, as adamw_kernel */

// the workgroup's fp64 sum in a fixed order: butterfly inside each wave, then the 8 waves in wave order (block_sum_f64, kf_device.h)
__device__ __forceinline__ void muon_block_sum(double ss, double* __restrict__ partials) { block_sum_f64<MUON_T>(ss, partials + blockIdx.x); }
// partials[0 .. np) added in workgroup order: thread t adds its contiguous run in order, thread 0 adds the 256 runs in order (runs_sum_f64, kf_device.h)
__global__ void __launch_bounds__(256) muon_sum_kernel(const double* __restrict__ partials, int np, double* __restrict__ out) {
    const double tot = runs_sum_f64(partials, np);
    if (threadIdx.x == 0) *out = tot;
}

__global__ void __launch_bounds__(MUON_T) muon_momentum_kernel(uint16_t* __restrict__ mG, const uint16_t* __restrict__ grads, uint16_t* __restrict__ X, size_t n, float one_minus_mu,
                                                               float mu, unsigned int seed, double* __restrict__ partials) {
    const size_t idx = ((size_t)blockIdx.x * MUON_T + threadIdx.x) * MUON_EPT;
    double ss = 0.0;
    if (idx < n) {
        const unsigned int thr = squirrel5(threadIdx.x + 198491317u * (blockIdx.x * MUON_T), seed) & 0xFFFFu;
        const u32x4 M = *reinterpret_cast<const u32x4*>(mG + idx), G = *reinterpret_cast<const u32x4*>(grads + idx);
        const uint32_t mw[4] = {M.x, M.y, M.z, M.w}, gw[4] = {G.x, G.y, G.z, G.w};
        uint32_t mo[4], xo[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint16_t m2[2], x2[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float m = h ? bf_hi(mw[i]) : bf_lo(mw[i]), g = h ? bf_hi(gw[i]) : bf_lo(gw[i]);
                m2[h] = stochastic_bf16(m + one_minus_mu * (g - m), thr);  /* PackedN::Lerp(mG, grads, 1 - mui) */
                x2[h] = stochastic_bf16(g + mu * (bf2f(m2[h]) - g), thr);  /* PackedN::Lerp(grads, mui) on the value just rounded */
                const double xd = (double)bf2f(x2[h]);
                ss = fma(xd, xd, ss);
            }
            mo[i] = (uint32_t)m2[0] | ((uint32_t)m2[1] << 16), xo[i] = (uint32_t)x2[0] | ((uint32_t)x2[1] << 16);
        }
        *reinterpret_cast<u32x4*>(mG + idx) = u32x4{mo[0], mo[1], mo[2], mo[3]};
        *reinterpret_cast<u32x4*>(X + idx) = u32x4{xo[0], xo[1], xo[2], xo[3]};
    }
    if (partials) muon_block_sum(ss, partials);
}

__global__ void __launch_bounds__(MUON_T) muon_apply_kernel(uint16_t* __restrict__ params, uint16_t* __restrict__ grads, const uint16_t* __restrict__ X, size_t n, float s1, float s2,
                                                            unsigned int seed, double* __restrict__ partials) {
    const size_t idx = ((size_t)blockIdx.x * MUON_T + threadIdx.x) * MUON_EPT;
    double ss = 0.0;
    if (idx < n) {
        const unsigned int thr = squirrel5(threadIdx.x + 198491317u * (blockIdx.x * MUON_T), seed) & 0xFFFFu;
        const u32x4 P = *reinterpret_cast<const u32x4*>(params + idx), S = *reinterpret_cast<const u32x4*>(X + idx);
        const uint32_t pw[4] = {P.x, P.y, P.z, P.w}, xw[4] = {S.x, S.y, S.z, S.w};
        uint32_t po[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint16_t p2[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float p = h ? bf_hi(pw[i]) : bf_lo(pw[i]), x = h ? bf_hi(xw[i]) : bf_lo(xw[i]);
                p2[h] = stochastic_bf16(s1 * p + s2 * x, thr); /* PackedN::Add2(1 - lr wd, params, -lr, X) */
                const double pd = (double)bf2f(p2[h]);
                ss = fma(pd, pd, ss);
            }
            po[i] = (uint32_t)p2[0] | ((uint32_t)p2[1] << 16);
        }
        *reinterpret_cast<u32x4*>(params + idx) = u32x4{po[0], po[1], po[2], po[3]};
        *reinterpret_cast<u32x4*>(grads + idx) = u32x4{0, 0, 0, 0};
    }
    if (partials) muon_block_sum(ss, partials);
}

// sum X^2 of a matrix handed to kf_newton_schulz without its sum: the momentum kernel's geometry and order
__global__ void __launch_bounds__(MUON_T) muon_sumsq_kernel(const uint16_t* __restrict__ X, size_t n, double* __restrict__ partials) {
    const size_t idx = ((size_t)blockIdx.x * MUON_T + threadIdx.x) * MUON_EPT;
    double ss = 0.0;
    if (idx < n) {
        const u32x4 S = *reinterpret_cast<const u32x4*>(X + idx);
        const uint32_t xw[4] = {S.x, S.y, S.z, S.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double lo = (double)bf_lo(xw[i]), hi = (double)bf_hi(xw[i]);
            ss = fma(lo, lo, ss), ss = fma(hi, hi, ss);
        }
    }
    muon_block_sum(ss, partials);
}

// v <- bf16(v + s v): cublasAxpyEx(s, X, X) with fp32 compute
__device__ __forceinline__ float muon_scale(float v, float s) { return round_bf16(v + s * v); }

// pre-scale (Optimizer.cu:522-531): alpha in fp64 from the device's sum, narrowed to float, THEN the 1 is taken off in float; post != 0 (only when no iteration follows): the post-scale too
__global__ void __launch_bounds__(256) muon_prescale_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, size_t n, const double* __restrict__ sumsq, float eps, float post) {
    const size_t idx = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (idx >= n) return;
    const float am1 = (float)(1.0 / (sqrt(*sumsq) + (double)eps)) - 1.0f;
    const u32x4 S = *reinterpret_cast<const u32x4*>(src + idx);
    const uint32_t xw[4] = {S.x, S.y, S.z, S.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float lo = muon_scale(bf_lo(xw[i]), am1), hi = muon_scale(bf_hi(xw[i]), am1);
        if (post != 0.0f) lo = muon_scale(lo, post), hi = muon_scale(hi, post);
        o[i] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
    }
    *reinterpret_cast<u32x4*>(dst + idx) = u32x4{o[0], o[1], o[2], o[3]};
}

// ---------------------------------------------------------------- the symmetric product
struct NsGram {
    const uint16_t* P; /* KM: X [K = ne0][dim] (contraction over its rows); else the symmetric A [dim][dim] */
    int dim, K;
    uint16_t* out;      /* [dim][dim] */
    const uint16_t* A0; /* NULL: out = bf16(acc) (A = X^T X); else out = bf16(b A0 + bf16(c acc)) (B = b A + c A A: the GEMM's bf16 store, then the axpy's) */
    float b, c;
};
// first linear index of row i of the upper triangle of an nt x nt tile grid
__device__ __forceinline__ int ns_tri_off(int i, int nt) { return i * nt - ((i * (i - 1)) >> 1); }

template <bool KM, class C>
__global__ void __launch_bounds__(C::NTH, C::WGS_PER_CU * C::NW / 4) ns_gram_kernel(const NsGram g) {
    static_assert(C::BM == C::BN, "square tiles: the mirror of tile (i, j) is tile (j, i)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nt = (g.dim + C::BM - 1) / C::BM, ntri = (nt * (nt + 1)) >> 1;
    // workgroup -> tile (i, j >= i): row i holds nt - i tiles; i from the root of off(i) = t, two integer steps against the fp32 square root's rounding
    const int t = g3_remap(blockIdx.x, ntri);
    const float s = 2.0f * nt + 1.0f;
    int i = (int)((s - sqrtf(s * s - 8.0f * (float)t)) * 0.5f);
    i = i < 0 ? 0 : (i > nt - 1 ? nt - 1 : i);
    while (i > 0 && ns_tri_off(i, nt) > t) i--;
    while (i < nt - 1 && ns_tri_off(i + 1, nt) <= t) i++;
    const int j = i + (t - ns_tri_off(i, nt));
    const int m0 = i * C::BM, t0 = j * C::BN;
    GemmArgs a = {};
    a.w = reinterpret_cast<const unsigned char*>(g.P), a.x = g.P, a.M = g.dim, a.n = g.dim, a.K = KM ? g.K : g.dim, a.ldr = g.dim, a.ldx = g.dim;
    f32x4 acc[C::MT][C::NT];
#pragma unroll
    for (int p = 0; p < C::MT; p++)
#pragma unroll
        for (int q = 0; q < C::NT; q++) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    g3_mainloop<KM, KM, G3_BK, C>(a, m0, t0, 0, a.K / G3_BK, acc, smem_raw, wid, lane);
    // lane holds rows r .. r + 3 of column col of a 16 x 16 block: out[col][r .. r + 3] is one 8-byte store (the mirror), out[r + q][col] four 2-byte stores
    const int wm = wid / C::WN, wn = wid % C::WN, r16 = lane & 15, q4 = lane >> 4;
    const bool diag = i == j;
#pragma unroll
    for (int mt = 0; mt < C::MT; mt++)
#pragma unroll
        for (int nn = 0; nn < C::NT; nn++) {
            const int col = t0 + wn * (16 * C::NT) + nn * 16 + r16, r = m0 + wm * (16 * C::MT) + mt * 16 + 4 * q4;
            if (col >= g.dim || r >= g.dim) continue; /* dim is a multiple of 64: r < dim covers r + 3 */
            if (diag && r > col) continue;            /* below the diagonal: the mirror of the element above it is what gets stored */
            const float vv[4] = {acc[mt][nn].x, acc[mt][nn].y, acc[mt][nn].z, acc[mt][nn].w};
            uint16_t* const lowp = g.out + (size_t)col * g.dim + r;
            float a0[4] = {0.f, 0.f, 0.f, 0.f};
            if (g.A0) {
                const u32x2 w4 = *reinterpret_cast<const u32x2*>(g.A0 + (size_t)col * g.dim + r); /* A0 is symmetric: A0[r + q][col] = A0[col][r + q] */
                a0[0] = bf_lo(w4.x), a0[1] = bf_hi(w4.x), a0[2] = bf_lo(w4.y), a0[3] = bf_hi(w4.y);
            }
            uint16_t o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = g.A0 ? f2bf(g.b * a0[q] + round_bf16(g.c * vv[q])) : f2bf(vv[q]);
            if (!diag || r + 3 <= col) {
                *reinterpret_cast<u32x2*>(lowp) = u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
#pragma unroll
                for (int q = 0; q < 4; q++) g.out[(size_t)(r + q) * g.dim + col] = o[q];
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (r + q <= col) lowp[q] = o[q], g.out[(size_t)(r + q) * g.dim + col] = o[q];
            }
        }
}

// X' [ne0, ne1] = bf16(a X + bf16(X B)), B symmetric [ne1, ne1]: the NT product y[row][m] = sum_k X[row][k] B[m][k]; post != 0: X' <- bf16(X' + post X') after the last iteration
struct NsXB {
    const uint16_t *X, *B;
    uint16_t* out;
    int ne0, ne1;
    float a, post;
};
template <class C>
__global__ void __launch_bounds__(C::NTH, C::WGS_PER_CU * C::NW / 4) ns_xb_kernel(const NsXB g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nbx = (g.ne1 + C::BM - 1) / C::BM, nby = (g.ne0 + C::BN - 1) / C::BN;
    const int wg = g3_remap(blockIdx.x, nbx * nby);
    const int m0 = (wg % nbx) * C::BM, t0 = (wg / nbx) * C::BN;
    GemmArgs a = {};
    a.w = reinterpret_cast<const unsigned char*>(g.B), a.M = g.ne1, a.K = g.ne1, a.x = g.X, a.ldx = g.ne1, a.n = g.ne0;
    f32x4 acc[C::MT][C::NT];
#pragma unroll
    for (int p = 0; p < C::MT; p++)
#pragma unroll
        for (int q = 0; q < C::NT; q++) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    g3_mainloop<false, false, G3_BK, C>(a, m0, t0, 0, a.K / G3_BK, acc, smem_raw, wid, lane);
    const int wm = wid / C::WN, wn = wid % C::WN, r16 = lane & 15, q4 = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < C::MT; mt++)
#pragma unroll
        for (int nn = 0; nn < C::NT; nn++) {
            const int row = t0 + wn * (16 * C::NT) + nn * 16 + r16, m = m0 + wm * (16 * C::MT) + mt * 16 + 4 * q4;
            if (row >= g.ne0 || m >= g.ne1) continue;
            const u32x2 w4 = *reinterpret_cast<const u32x2*>(g.X + (size_t)row * g.ne1 + m);
            const float x0[4] = {bf_lo(w4.x), bf_hi(w4.x), bf_lo(w4.y), bf_hi(w4.y)}, vv[4] = {acc[mt][nn].x, acc[mt][nn].y, acc[mt][nn].z, acc[mt][nn].w};
            uint16_t o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float v = round_bf16(g.a * x0[q] + round_bf16(vv[q]));
                if (g.post != 0.0f) v = muon_scale(v, g.post);
                o[q] = f2bf(v);
            }
            *reinterpret_cast<u32x2*>(g.out + (size_t)row * g.ne1 + m) = u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
        }
}

// ---------------------------------------------------------------- host side
static inline int muon_ok() { return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK; }
static inline unsigned muon_blocks(size_t n) { return (unsigned)((n + MUON_PER_WG - 1) / MUON_PER_WG); }

MuonLayout muon_layout(int ne0, int ne1) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    MuonLayout L;
    const size_t n = (size_t)ne0 * ne1, sq = up((size_t)ne1 * ne1 * 2), xs = up(n * 2);
    L.A = 0, L.B = sq, L.X0 = 2 * sq, L.X1 = L.X0 + xs, L.part = L.X1 + xs, L.dbl = L.part + up((size_t)muon_blocks(n) * sizeof(double)), L.bytes = L.dbl + 256;
    return L;
}

int muon_momentum_launch(hipStream_t st, uint16_t* mG, const uint16_t* grads, uint16_t* X, size_t n, float mui, unsigned int seed, double* partials, double* d_sumsq) {
    const unsigned nb = muon_blocks(n);
    hipLaunchKernelGGL(muon_momentum_kernel, dim3(nb), dim3(MUON_T), 0, st, mG, grads, X, n, 1.0f - mui, mui, seed, d_sumsq ? partials : nullptr);
    if (d_sumsq) hipLaunchKernelGGL(muon_sum_kernel, dim3(1), dim3(256), 0, st, partials, (int)nb, d_sumsq);
    return muon_ok();
}
int muon_apply_launch(hipStream_t st, uint16_t* params, uint16_t* grads, const uint16_t* X, size_t n, float lr, float wd, unsigned int seed, double* partials, double* d_wnormsq) {
    const unsigned nb = muon_blocks(n);
    hipLaunchKernelGGL(muon_apply_kernel, dim3(nb), dim3(MUON_T), 0, st, params, grads, X, n, 1.0f - lr * wd, -lr, seed, d_wnormsq ? partials : nullptr);
    if (d_wnormsq) hipLaunchKernelGGL(muon_sum_kernel, dim3(1), dim3(256), 0, st, partials, (int)nb, d_wnormsq);
    return muon_ok();
}

// X [ne0, ne1] in place.  The pre-scale writes to whichever of the two buffers leaves the LAST iteration's output in X itself.
int newton_schulz_launch(hipStream_t st, uint16_t* X, int ne0, int ne1, const double* d_sumsq, float eps, int n_iter, float a, float b, float c, void* scratch) {
    const MuonLayout L = muon_layout(ne0, ne1);
    char* const sc = reinterpret_cast<char*>(scratch);
    uint16_t *const A = reinterpret_cast<uint16_t*>(sc + L.A), *const Bm = reinterpret_cast<uint16_t*>(sc + L.B), *const X1 = reinterpret_cast<uint16_t*>(sc + L.X1);
    const size_t n = (size_t)ne0 * ne1;
    if (!d_sumsq) {
        double *const part = reinterpret_cast<double*>(sc + L.part), *const dbl = reinterpret_cast<double*>(sc + L.dbl);
        const unsigned nb = muon_blocks(n);
        hipLaunchKernelGGL(muon_sumsq_kernel, dim3(nb), dim3(MUON_T), 0, st, X, n, part);
        hipLaunchKernelGGL(muon_sum_kernel, dim3(1), dim3(256), 0, st, part, (int)nb, dbl);
        d_sumsq = dbl;
    }
    // post-scale (Optimizer.cu:567-570): beta = sqrt(max(1, m / n)) - 1 with m = ne1, n = ne0.  Every Muon tensor has ne0 >= ne1, so beta is 0 and the branch is
    // never taken on this path; it is kept (folded into the last store of X) so that the arithmetic stays the reference's if the routing rule ever widens.
    const float m_over_n = (float)ne1 * 1.0f / (float)ne0, beta = sqrtf(m_over_n > 1.0f ? m_over_n : 1.0f) - 1.0f;
    uint16_t* cur = (n_iter & 1) ? X1 : X;
    hipLaunchKernelGGL(muon_prescale_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, X, cur, n, d_sumsq, eps, n_iter == 0 ? beta : 0.0f);
    const int nt128 = (ne1 + 127) / 128, nt64 = ne1 / 64;
    for (int it = 0; it < n_iter; it++) {
        uint16_t* const nxt = cur == X ? X1 : X;
        NsGram g1 = {cur, ne1, ne0, A, nullptr, 0.0f, 0.0f};
        hipLaunchKernelGGL((ns_gram_kernel<true, G3Small>), dim3(nt128 * (nt128 + 1) / 2), dim3(G3Small::NTH), 2 * G3Small::STAGE, st, g1);
        NsGram g2 = {A, ne1, ne1, Bm, A, b, c};
        hipLaunchKernelGGL((ns_gram_kernel<false, G3Tiny>), dim3(nt64 * (nt64 + 1) / 2), dim3(G3Tiny::NTH), 2 * G3Tiny::STAGE, st, g2);
        NsXB x = {cur, Bm, nxt, ne0, ne1, a, it == n_iter - 1 ? beta : 0.0f};
        hipLaunchKernelGGL((ns_xb_kernel<G3Small>), dim3(nt128 * ((ne0 + 127) / 128)), dim3(G3Small::NTH), 2 * G3Small::STAGE, st, x);
        cur = nxt;
    }
    return muon_ok();
}

}  // namespace kf
