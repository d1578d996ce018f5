// kf_gradnorm_plan.h -- how kf_grad_norms (the sums of squares of EVERY gradient tensor of a step in one launch, include/kf_abi.h "gradient norms") is laid out:
// kf::gradnorm_plan, one pure host function, makes the table the kernels read -- which workgroups a tensor owns -- and the scratch layout; kf_grad_norms_plan
// writes what it returns to the device once, the launcher (kf_gradnorm.hip) carries it out and decides nothing.
// Tensor i of n[i] elements is cut into chunks of GN_CHUNK = 4096 elements (512 threads x 8 bf16: the geometry of muon_sumsq_kernel and adamw_kernel); it owns the
// workgroups [wg0[i], wg0[i + 1]), one chunk each, wg0[0] = 0, wg0[i + 1] = wg0[i] + ceil(n[i] / 4096).  A workgroup finds its tensor by gradnorm_find: the
// largest i with wg0[i] <= wg, a binary search the kernel runs with the same body.  The bits depend on n alone: the chunk is the unit of the summation order.
#pragma once
#include "kf_kernels.h"

namespace kf {

constexpr int GN_T = 512, GN_EPT = 8, GN_CHUNK = GN_T * GN_EPT; /* = MUON_PER_WG (kf_muon.hip) */
constexpr int GN_MAX_TENSORS = 1 << 12; /* gn_total_kernel adds the per-tensor sums serially on one thread (the fixed tensor order): measured at 580 tensors, microseconds at 4096 */

// one row of the device table; row n_tensors is the sentinel: g = NULL, wg0 = the grid, n = the plan's stamp.  Every kernel compares the stamp it finds there with
// the one the host remembers before it follows a pointer of the table: a scratch that was freed and handed out again since it was planned (same address, other
// contents) makes the launch a no-op that reports NaN norms, not a walk through garbage pointers.
struct GradNormEntry {
    const uint16_t* g;
    long long n;
    int wg0;
    int no_clip; /* != 0: the tensor's scale is 1.0f in every mode (it still counts in the total) */
};
struct GradNormPlan {
    int status;     /* KF_OK, or the refusal */
    int bad;        /* the first tensor that caused it, or -1 */
    int n_tensors;
    int total_wg;   /* the first launch's grid */
    size_t off_table, off_part; /* byte offsets into the scratch, each a multiple of 256: GradNormEntry [n_tensors + 1]; double [total_wg] */
    size_t bytes;
    unsigned long long stamp;   /* set by kf_grad_norms_plan (unique per call); 0 from gradnorm_plan */
};
constexpr unsigned long long GN_STAMP0 = 0x4B46474E00000000ull; /* "KFGN" << 32, + a per-process counter */

inline GradNormPlan gradnorm_plan(int n_tensors, const long long* n) {
    GradNormPlan p = {};
    p.bad = -1;
    if (n_tensors < 1 || n_tensors > GN_MAX_TENSORS || !n) {
        p.status = KF_INVALID_ARGS;
        return p;
    }
    long long wg = 0;
    for (int i = 0; i < n_tensors; i++) {
        if (n[i] < 8 || (n[i] & 7) || n[i] > (1LL << 40)) {
            p.status = KF_INVALID_ARGS, p.bad = i;
            return p;
        }
        wg += (n[i] + GN_CHUNK - 1) / GN_CHUNK;
        if (wg > 0x7FFFFFFFLL) {
            p.status = KF_INVALID_ARGS, p.bad = i;
            return p;
        }
    }
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    p.n_tensors = n_tensors, p.total_wg = (int)wg;
    p.off_table = 0, p.off_part = up(sizeof(GradNormEntry) * ((size_t)n_tensors + 1)), p.bytes = p.off_part + up(sizeof(double) * (size_t)wg);
    return p;
}
// wg0 of every tensor and the sentinel: out[0 .. n_tensors]
inline void gradnorm_wg0(int n_tensors, const long long* n, int* out) {
    int wg = 0;
    for (int i = 0; i < n_tensors; i++) out[i] = wg, wg += (int)((n[i] + GN_CHUNK - 1) / GN_CHUNK);
    out[n_tensors] = wg;
}
// the tensor that owns workgroup wg < tab[n_tensors].wg0: the largest i with tab[i].wg0 <= wg (every tensor owns at least one workgroup: wg0 is strictly increasing)
__host__ __device__ inline int gradnorm_find(const GradNormEntry* tab, int n_tensors, int wg) {
    int lo = 0, hi = n_tensors; /* tab[lo].wg0 <= wg < tab[hi].wg0 */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].wg0 <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- the launcher (kf_gradnorm.hip): carries out a plan that kf_grad_norms_plan has written to `scratch`; KF_OK or KF_HIP_CHECK
int grad_norms_launch(hipStream_t st, const void* scratch, const GradNormPlan& p, int mode, float gclip, double* d_sumsq, float* d_gnorm, float* d_scale);

}  // namespace kf
