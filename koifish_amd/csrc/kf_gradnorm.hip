// kf_gradnorm.hip -- the gradient norms of a training step: the sum of squares of EVERY gradient tensor in one launch, the clip factors left on the device for
// kf_adamw_scaled.  The reference takes them one tensor at a time (GTensor::Length, huTensor.cu:665-704: a memset, an atomicAdd kernel and a blocking read-back per
// tensor; Optimizer.cu:756-774 forms grad_scale on the host); here the host reads nothing and the order of every sum is fixed:
//   gn_sumsq_kernel  one workgroup per 4096-element chunk of the table (kf_gradnorm_plan.h); muon_sumsq_kernel's arithmetic: each bf16 widened to fp64,
//                    ss = fma(x, x, ss) over the thread's 8 elements in element order, then muon_block_sum's order -- butterfly inside each wave, the 8 waves in
//                    wave order -- one fp64 partial per chunk.  Elements at or past n are not loaded.
//   gn_tensor_kernel one workgroup per tensor: its chunk partials in muon_sum_kernel's order (256 contiguous runs, each added in order, then the runs in order);
//                    sumsq[i], gnorm[i] = (float)sqrt(sumsq[i]) (the root in fp64, narrowed once)
//   gn_total_kernel  one workgroup: the per-tensor sums in tensor order -> sumsq[n_tensors], gnorm[n_tensors]; then the scales (fp32 division)
// No atomics.  Products of bf16 values are exact in fp64; only the additions round.
// Each kernel first compares the stamp in the table's sentinel row with the host's (kf_gradnorm_plan.h): on a mismatch the first two do nothing and the last one
// reports NaN norms and unit scales.
#include "kf_gradnorm_plan.h"

namespace kf {

__global__ void __launch_bounds__(GN_T) gn_sumsq_kernel(const GradNormEntry* __restrict__ tab, int n_tensors, unsigned long long stamp, double* __restrict__ partials) {
    if ((unsigned long long)tab[n_tensors].n != stamp) return; /* uniform */
    const int wg = blockIdx.x; /* uniform: the search runs on scalar registers */
    const int ti = gradnorm_find(tab, n_tensors, wg);
    const uint16_t* const g = tab[ti].g;
    const long long n = tab[ti].n, idx = ((long long)(wg - tab[ti].wg0) * GN_T + threadIdx.x) * GN_EPT;
    double ss = 0.0;
    if (idx < n) { /* n is a multiple of 8: the 8 elements of a thread are inside or outside together */
        const u32x4 S = *reinterpret_cast<const u32x4*>(g + idx);
        const uint32_t xw[4] = {S.x, S.y, S.z, S.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double lo = (double)bf_lo(xw[i]), hi = (double)bf_hi(xw[i]);
            ss = fma(lo, lo, ss), ss = fma(hi, hi, ss);
        }
    }
    block_sum_f64<GN_T>(ss, partials + wg); /* the one body muon_block_sum uses */
}

__global__ void __launch_bounds__(256) gn_tensor_kernel(const GradNormEntry* __restrict__ tab, int n_tensors, unsigned long long stamp, const double* __restrict__ partials,
                                                        double* __restrict__ sumsq, float* __restrict__ gnorm) {
    if ((unsigned long long)tab[n_tensors].n != stamp) return;
    const int ti = blockIdx.x, p0 = tab[ti].wg0, np = tab[ti + 1].wg0 - p0;
    const double tot = runs_sum_f64(partials + p0, np); /* the one body muon_sum_kernel uses */
    if (threadIdx.x == 0) sumsq[ti] = tot, gnorm[ti] = (float)sqrt(tot);
}

// A NaN norm compares false (scale 1.0f), +inf gives c / inf = 0.0f: no special case; kf_adamw's own non-finite guard does the rest
__global__ void __launch_bounds__(256) gn_total_kernel(const GradNormEntry* __restrict__ tab, int n_tensors, unsigned long long stamp, int mode, float c,
                                                       double* __restrict__ sumsq, float* __restrict__ gnorm, float* __restrict__ scale) {
    __shared__ float gtot;
    if ((unsigned long long)tab[n_tensors].n != stamp) { /* not the table that was planned: nothing of it was followed */
        for (int i = threadIdx.x; i <= n_tensors; i += 256) {
            sumsq[i] = __builtin_nan(""), gnorm[i] = __builtin_nanf("");
            if (i < n_tensors) scale[i] = 1.0f;
        }
        return;
    }
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < n_tensors; i++) tot += sumsq[i];
        const float gn = (float)sqrt(tot);
        sumsq[n_tensors] = tot, gnorm[n_tensors] = gn, gtot = gn;
    }
    __syncthreads();
    const float sg = gtot > c ? c / gtot : 1.0f;
    for (int i = threadIdx.x; i < n_tensors; i += 256) {
        float s = 1.0f;
        if (!tab[i].no_clip) {
            if (mode == KF_CLIP_TENSOR) {
                const float gn = gnorm[i];
                s = gn > c ? c / gn : 1.0f;
            } else if (mode == KF_CLIP_GLOBAL) {
                s = sg;
            }
        }
        scale[i] = s;
    }
}

int grad_norms_launch(hipStream_t st, const void* scratch, const GradNormPlan& p, int mode, float gclip, double* d_sumsq, float* d_gnorm, float* d_scale) {
    const GradNormEntry* const tab = reinterpret_cast<const GradNormEntry*>(reinterpret_cast<const char*>(scratch) + p.off_table);
    double* const part = reinterpret_cast<double*>(const_cast<char*>(reinterpret_cast<const char*>(scratch)) + p.off_part);
    hipLaunchKernelGGL(gn_sumsq_kernel, dim3((unsigned)p.total_wg), dim3(GN_T), 0, st, tab, p.n_tensors, p.stamp, part);
    hipLaunchKernelGGL(gn_tensor_kernel, dim3((unsigned)p.n_tensors), dim3(256), 0, st, tab, p.n_tensors, p.stamp, part, d_sumsq, d_gnorm);
    hipLaunchKernelGGL(gn_total_kernel, dim3(1), dim3(256), 0, st, tab, p.n_tensors, p.stamp, mode, gclip, d_sumsq, d_gnorm, d_scale);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
