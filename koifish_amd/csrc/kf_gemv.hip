// kf_gemv.hip -- the one-token mat-vec launcher: a GemvLaunch becomes a problem, kf::gemv_plan (kf_gemv_plan.h) decides, this file carries the plan out with the
// v_dot2c_f32_bf16 instantiations of gemv_kernel (kf_gemv_kernel.h) or, in the canonical order, with kf_gemv_canon.hip's; and the arg-max pick behind the LM head.
#include "kf_gemv_kernel.h"

namespace kf {

Knobs g_knobs;

// Final pick over the per-workgroup partial maxima, then the decode-state update for graph replay.
__global__ void __launch_bounds__(256) argmax_finish_kernel(const float* val, const int* idx, int n, int32_t* d_argmax, int32_t* d_state,
                                                            int32_t* d_tokens_out) {
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    // all of a thread's partials are requested before the first compare (n <= KF_MAX_ARGMAX_PARTIALS = 16 per thread): one memory latency instead of 16
    constexpr int PER = KF_MAX_ARGMAX_PARTIALS / 256;
    float v[PER];
    int ix[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = threadIdx.x + k * 256;
        const int ic = i < n ? i : 0;
        v[k] = val[ic], ix[k] = idx[ic];
        if (i >= n) v[k] = -__builtin_inff(), ix[k] = 0x7fffffff;
    }
#pragma unroll
    for (int k = 0; k < PER; k++)
        if (v[k] > bv || (v[k] == bv && ix[k] < bi)) bv = v[k], bi = ix[k];
    for (int i = threadIdx.x + PER * 256; i < n; i += blockDim.x) { /* never taken: n <= KF_MAX_ARGMAX_PARTIALS */
        const float w = val[i];
        const int jx = idx[i];
        if (w > bv || (w == bv && jx < bi)) bv = w, bi = jx;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        float ov = __shfl_xor(bv, m, 64);
        int oi = __shfl_xor(bi, m, 64);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    __shared__ float sv[4];
    __shared__ int si[4];
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) bv = sv[w], bi = si[w];
        if (d_argmax) *d_argmax = bi;
        if (d_state) {
            const int p = d_state[1];
            if (d_tokens_out) d_tokens_out[p] = bi;
            d_state[0] = bi;
            d_state[1] = p + 1;
        }
    }
}

void argmax_finish_launch(hipStream_t st, const float* val, const int* idx, int n, int32_t* d_argmax, int32_t* d_state, int32_t* d_tokens_out) {
    hipLaunchKernelGGL(argmax_finish_kernel, dim3(1), dim3(256), 0, st, val, idx, n, d_argmax, d_state, d_tokens_out);
}

int gemv_dispatch_dot2(const GemvPlan& p, const GemvArgs& a, hipStream_t st) { return gemv_dispatch<false>(p, a, st); }

GemvProblem gemv_problem(const GemvLaunch& L) {
    GemvProblem P = {};
    P.mode = L.mode, P.n_w = L.n;
    for (int j = 0; j < L.n; j++) P.w[j] = mat_of(L.w[j]);
    P.sparse = L.args.row_map != nullptr, P.n_hot = L.n_hot;
    P.norm = L.args.norm_w != nullptr, P.canon = L.canon != 0;
    P.q4_perm = g_knobs.q4_perm != 0, P.q2_tab = g_knobs.q2_tab != 0, P.q1_tab = g_knobs.q1_tab != 0, P.xf2 = g_knobs.gemv_xf2 != 0;
    return P;
}

int gemv_launch(hipStream_t st, GemvLaunch& L, const GemvPlan& p) {
    if (p.status) return p.status;
    GemvArgs& a = L.args;
    a.njobs = p.njobs, a.K = p.K, a.nBlk = p.nBlk, a.lpr_log2 = p.lpr_log2, a.iters = p.iters, a.lGroup = p.lgroup, a.gshift = p.gshift;
    a.spw = p.spw, a.total_slots = p.total_slots, a.stream_ok = p.stream_ok;
    a.inv_dim = 1.0f / (float)p.K;
    for (int j = 0; j < 3; j++) {
        GemvJob& jb = a.job[j];
        jb.slot0 = p.slot0[j];
        if (j >= L.n) continue;
        const kf_weight* w = L.w[j];
        jb.w = w->data, jb.M = p.M[j], jb.qBias = w->qBias;
        jb.zero = jb.step = nullptr;
        if (p.fmt >= FMT_Q4) jb.zero = w->gama + w->ne0 + w->ne1; /* gama_T(ZERO), GTensor.cpp:456-510; FMT_Q4R: the row codebooks, 16 entries per row */
        if (p.fmt >= FMT_Q4 && p.fmt != FMT_Q4R) jb.step = jb.zero + (size_t)w->ne0 * w->ne1 / w->lGroup;
    }
    L.blocks = p.grid;
    return p.canon ? gemv_dispatch_canon(p, a, st) : gemv_dispatch_dot2(p, a, st);
}

}  // namespace kf
