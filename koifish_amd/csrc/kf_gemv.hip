// kf_gemv.hip -- the one-token mat-vec launcher: a GemvLaunch becomes a problem, kf::gemv_plan (kf_gemv_plan.h) decides, this file carries the plan out with the
// v_dot2c_f32_bf16 instantiations of gemv_kernel (kf_gemv_kernel.h) or, in the canonical order, with kf_gemv_canon.hip's; and the arg-max pick behind the LM head.
#include "kf_gemv_kernel.h"
#include "kf_rowq.h"

namespace kf {

Knobs g_knobs;

// Final pick over the per-workgroup partial maxima, then the decode-state update for graph replay.
__global__ void __launch_bounds__(256) argmax_finish_kernel(const float* val, const int* idx, int n, int32_t* d_argmax, int32_t* d_state,
                                                            int32_t* d_tokens_out) {
    float bv = FIRST_MAX_NONE_V;
    int bi = FIRST_MAX_NONE_I;
    // all of a thread's partials are requested before the first compare (n <= KF_MAX_ARGMAX_PARTIALS = 16 per thread): one memory latency instead of 16
    constexpr int PER = KF_MAX_ARGMAX_PARTIALS / 256;
    float v[PER];
    int ix[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = threadIdx.x + k * 256;
        const int ic = i < n ? i : 0;
        v[k] = val[ic], ix[k] = idx[ic];
        if (i >= n) v[k] = FIRST_MAX_NONE_V, ix[k] = FIRST_MAX_NONE_I;
    }
#pragma unroll
    for (int k = 0; k < PER; k++) first_max(bv, bi, v[k], ix[k]);
    for (int i = threadIdx.x + PER * 256; i < n; i += blockDim.x) first_max(bv, bi, val[i], idx[i]); /* never taken: n <= KF_MAX_ARGMAX_PARTIALS */
    block_first_max_256(bv, bi);
    if (threadIdx.x == 0) {
        if (d_argmax) *d_argmax = bi;
        if (d_state) advance_decode_state(d_state, d_tokens_out, bi);
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
    // the 3- / 2-bit row forms behind kf_set_row_unpack: planned as 4-bit row codebooks of their shape (plain and paired launches; the arg-max and sparse forms refuse
    // them as they are)
    if (L.row_unpack && L.mode != GEMV_ARGMAX && !L.args.row_map) (void)rowq_standins(L.n, L.w, P.w, false);
    P.sparse = L.args.row_map != nullptr, P.n_hot = L.n_hot;
    P.norm = L.args.norm_w != nullptr, P.canon = L.canon != 0;
    P.q4_perm = g_knobs.q4_perm != 0, P.q2_tab = g_knobs.q2_tab != 0, P.q1_tab = g_knobs.q1_tab != 0, P.xf2 = g_knobs.gemv_xf2 != 0;
    return P;
}

int gemv_launch(hipStream_t st, GemvLaunch& L, const GemvPlan& p) {
    if (p.status) return p.status;
    GemvPlan q = p;
    if (L.row_unpack && p.fmt == FMT_Q4R && rowq_fmt(L.w[0]) >= 0) q.fmt = rowq_fmt(L.w[0]); /* the stand-in's plan, the weight's own unpack */
    GemvArgs& a = L.args;
    a.njobs = p.njobs, a.K = p.K, a.nBlk = p.nBlk, a.lpr_log2 = p.lpr_log2, a.iters = p.iters, a.lGroup = p.lgroup, a.gshift = p.gshift;
    a.spw = p.spw, a.total_slots = p.total_slots, a.stream_ok = p.stream_ok;
    a.inv_dim = 1.0f / (float)p.K;
    gemv_fill_jobs(a.job, p.slot0, p.M, L.w, L.n, q.fmt);
    L.blocks = p.grid;
    return p.canon ? gemv_dispatch_canon(q, a, st) : gemv_dispatch_dot2(q, a, st);
}

}  // namespace kf
