// kf_evo.hip -- the evolve step of "Evolutionary Optimization of Experts": Fuyou::Exploitation (Optimizer.cu:439-484) over one follower matrix x (bf16 master, in place)
// and the head's matrix (bf16, read only), CU_mix_ / CU_PSO_2D / CU_crossover_ (operator.cuh:326-390) restated for gfx950 -- and the ensemble mean of per-row losses
// (Fish::ForwardOnRLS, gLLM.cpp:722-787: tmpLoss[i] / curB).
//
// The reference keeps one curandState per ROW and walks the row serially; PSO and crossover are two launches.  XORWOW streams cannot be restated outside curand, so the
// draw here is this project's own, counter-based: ONE SquirrelNoise5 hash per element, keyed on the flat row-major index and the launch's seed,
//     h = squirrel5(i, seed);  b0 .. b3 = the four bytes of h, low to high;  r = float(b0 + b1 + b2) * (1.0f / 765.0f)
// r (the mean of three uniform bytes: support [0, 1], mean 0.5, standard deviation 0.1673) stands where the reference has clip((N(0,1) + 3) / 6, 0, 1] (1/6); b3 decides
// the crossover.  Every element is independent of the launch geometry: the pass is fully parallel, PSO + crossover are ONE pass, and tests/evo_restate.py states the same
// bits in numpy.  r == 0 leaves the element as it is (the reference's `continue`).  The multiply and the add of every update are separate fp32 operations
// (-ffp-contract=off); stores are round-to-nearest-even, the reference's (T) cast -- not the optimiser's stochastic store.
//
// Memory-bound: 2 B read + 2 B written of x, 2 B read of head per element.  16-byte loads and stores (8 bf16 per lane per trip), 256-thread workgroups, a grid of at
// most 8 workgroups per CU striding over the tensor; x by a plain load (it is written back), head non-temporally (read once).
#include "kf_device.h"
#include "kf_kernels.h"

namespace kf {

constexpr int EVO_T = 256, EVO_EPT = 8, EVO_WG_PER_CU = 8;

template <int ALGO>
__device__ __forceinline__ uint32_t evo_one(uint32_t xb, uint32_t gb, uint32_t i, uint32_t seed, float alpha, float beta, float social, uint32_t thr) {
    const float xf = __uint_as_float(xb << 16), gf = __uint_as_float(gb << 16);
    if (ALGO == KF_EVO_MIX) {
        const float a = alpha * xf, b = beta * gf;
        return f2bf(a + b);
    }
    const uint32_t h = squirrel5(i, seed);
    const uint32_t s3 = (h & 255u) + ((h >> 8) & 255u) + ((h >> 16) & 255u);
    const float r = (float)s3 * (1.0f / 765.0f);
    const float t = social * r, d = gf - xf;
    const float td = t * d;
    const uint32_t pso = f2bf(xf + td);
    uint32_t out = s3 != 0 ? pso : xb; /* a select, not a branch: r == 0 is one element in 2^24 */
    if (ALGO == KF_EVO_PSO_GA && (h >> 24) < thr) out = gb; /* CU_crossover_ runs over the PSO result: the head's 16 bits verbatim */
    return out;
}

template <int ALGO>
__global__ void __launch_bounds__(EVO_T) evolve_kernel(uint16_t* __restrict__ x, const uint16_t* __restrict__ head, uint32_t n8, float alpha, float beta, float social,
                                                       uint32_t thr, uint32_t seed) {
    const uint32_t stride = gridDim.x * EVO_T;
    for (uint32_t v = blockIdx.x * EVO_T + threadIdx.x; v < n8; v += stride) { /* n8 < 2^29 (the entry bounds n below 2^32) and the stride is a few 2^19: v + stride does not wrap */
        const u32x4 X = *reinterpret_cast<const u32x4*>(x + (size_t)v * EVO_EPT);
        const u32x4 G = ld_nt(reinterpret_cast<const u32x4*>(head + (size_t)v * EVO_EPT));
        const uint32_t xw[4] = {X.x, X.y, X.z, X.w}, gw[4] = {G.x, G.y, G.z, G.w};
        uint32_t o[4];
        const uint32_t i0 = v * EVO_EPT;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t lo = evo_one<ALGO>(xw[k] & 0xFFFFu, gw[k] & 0xFFFFu, i0 + 2 * k, seed, alpha, beta, social, thr);
            const uint32_t hi = evo_one<ALGO>(xw[k] >> 16, gw[k] >> 16, i0 + 2 * k + 1, seed, alpha, beta, social, thr);
            o[k] = lo | (hi << 16);
        }
        *reinterpret_cast<u32x4*>(x + (size_t)v * EVO_EPT) = u32x4{o[0], o[1], o[2], o[3]};
    }
}

// workgroups of one launch over n8 16-byte vectors: enough to cover them, at most EVO_WG_PER_CU per CU of the current device (asked once per device)
static int evo_grid(uint32_t n8, unsigned* grid) {
    static int cu_of[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return KF_HIP_CHECK;
    if (cu_of[dev] == 0) {
        int n_cu = 0;
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu < 1) return KF_HIP_CHECK;
        cu_of[dev] = n_cu;
    }
    const unsigned need = (n8 + EVO_T - 1) / EVO_T, cap = (unsigned)cu_of[dev] * EVO_WG_PER_CU;
    *grid = need < cap ? need : cap;
    return KF_OK;
}

int evolve_launch(hipStream_t st, uint16_t* x, const uint16_t* head, size_t n, int algorithm, float alpha, float beta, float social, unsigned int thr, unsigned int seed) {
    if (n < 8 || n % 8 || n >= ((size_t)1 << 32)) return KF_INVALID_ARGS;
    const uint32_t n8 = (uint32_t)(n / 8);
    unsigned grid = 0;
    const int rc = evo_grid(n8, &grid);
    if (rc != KF_OK) return rc;
    switch (algorithm) {
        case KF_EVO_PSO: hipLaunchKernelGGL(evolve_kernel<KF_EVO_PSO>, dim3(grid), dim3(EVO_T), 0, st, x, head, n8, alpha, beta, social, thr, seed); break;
        case KF_EVO_PSO_GA: hipLaunchKernelGGL(evolve_kernel<KF_EVO_PSO_GA>, dim3(grid), dim3(EVO_T), 0, st, x, head, n8, alpha, beta, social, thr, seed); break;
        case KF_EVO_MIX: hipLaunchKernelGGL(evolve_kernel<KF_EVO_MIX>, dim3(grid), dim3(EVO_T), 0, st, x, head, n8, alpha, beta, social, thr, seed); break;
        default: return KF_INVALID_ARGS;
    }
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

// The ensemble mean, one branch at a time (the trainer has ONE losses buffer, which the next branch's forward overwrites): index 0 starts the sum, every later index adds
// to it, the last index divides -- fp32, in index order, `/` correctly rounded: ((l0 + l1) + l2) / count.
__global__ void __launch_bounds__(256) loss_mean_kernel(float* __restrict__ acc, const float* __restrict__ losses, uint32_t n, int first, int last, float count) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = losses[i];
    if (!first) s = acc[i] + s;
    if (last) s = s / count;
    acc[i] = s;
}
int loss_mean_launch(hipStream_t st, float* acc, const float* losses, size_t n, int index, int count) {
    if (n == 0 || n >= ((size_t)1 << 31) || count < 1 || index < 0 || index >= count) return KF_INVALID_ARGS;
    hipLaunchKernelGGL(loss_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc, losses, (uint32_t)n, index == 0, index == count - 1, (float)count);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
