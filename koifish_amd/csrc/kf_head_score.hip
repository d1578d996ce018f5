// kf_head_score.hip -- the LM head with the log-softmax in its epilogue: per row the log-probability of a target id, the row's log-sum-exp and its greedy id, without
// the [rows x vocabulary] logit matrix ever being written (Qwen3: 2047 x 151 936 bf16 = 622 MB per prompt).  What Fish_ppl / Fish::Eval_ppl of the reference compute
// token by token as log(P_softmax(target, logits, nVocab)); here (logit[target] - m) - log(sum exp(logit - m)) with m the row maximum, which is the same number without
// P_softmax's underflow to log(0) = -inf for an unlikely token.
//   head_score_kernel   the tiles and k-loop of kf_gemm3.hip (kf_gemm3_tile.h: global_load_lds operands, two LDS buffers, v_mfma_f32_16x16x32_bf16) over
//                       [vocabulary tile x row block]; the epilogue rounds every accumulator to bf16 -- the logit kf_linear / kf_lm_head would store -- and folds the
//                       tile's columns into ONE partial per row: {max, sum exp(v - max), first index of the max, the target's logit if it lies in the tile}.  A lane
//                       holds one row's 4 MT logits of the wave's vocabulary half; the row's four lanes meet by two row swaps, the two vocabulary halves through LDS.
//                       Columns >= V are left out of max, sum and index; rows >= n store nothing.  Workgroup order: the row blocks of one vocabulary tile back to back
//                       on one XCD (after the XCD remap), so a tile of W is fetched once into that L2 and the (small) activations are what is re-read.
//   score_merge_kernel  a wave per row: lane l folds the partials of tiles l, l + 64, ... in ascending order, then a fixed butterfly over the lanes.  The order is a
//                       function of the shape alone, never of timing; ties of the maximum go to the lower index at every merge, across tiles too.
//   score_rows_kernel   the panel route's fold of one materialised panel of bf16 logits (kf_linear's output) into the same numbers: a workgroup per row.
// exp / log are the fixed kf_expf / kf_logf (as kf_fused_classifier).  Partials are written with ordinary vector stores.
#include <string.h>

#include "kf_gemm3_tile.h"
#include "kf_score_plan.h"

namespace kf {

struct ScoreState {
    float m, s; /* running maximum; sum of exp(v - m) */
    int i;      /* first index of the maximum */
    float t;    /* the target's logit (0 until met) */
};
__device__ __forceinline__ ScoreState score_empty() { return ScoreState{-__builtin_inff(), 0.0f, 0x7fffffff, 0.0f}; }
// commutative in its fp32 results: either argument order gives the same bits (the butterfly below relies on it)
__device__ __forceinline__ ScoreState score_merge(const ScoreState& a, const ScoreState& b) {
    ScoreState o;
    o.m = a.m > b.m ? a.m : b.m;
    const float ea = a.m == o.m ? 1.0f : kf_expf(a.m - o.m), eb = b.m == o.m ? 1.0f : kf_expf(b.m - o.m); /* kf_expf(0) = 1 exactly */
    o.s = a.s * ea + b.s * eb;
    o.i = a.m > b.m ? a.i : (b.m > a.m ? b.i : (a.i < b.i ? a.i : b.i));
    o.t = a.t + b.t; /* at most one side has met the target */
    return o;
}
__device__ __forceinline__ ScoreState score_xor(const ScoreState& a, int off) {
    ScoreState o;
    o.m = __shfl_xor(a.m, off), o.s = __shfl_xor(a.s, off), o.i = __shfl_xor(a.i, off), o.t = __shfl_xor(a.t, off);
    return o;
}
__device__ __forceinline__ f32x4 score_pack(const ScoreState& a) { return f32x4{a.m, a.s, __int_as_float(a.i), a.t}; }
__device__ __forceinline__ ScoreState score_unpack(const f32x4& v) { return ScoreState{v.x, v.y, __float_as_int(v.z), v.w}; }
// a row's three outputs from its merged state; tgt < 0: not scored (logprob 0); tgt >= V can only come from ids the host never saw: NaN, nothing is read for it
__device__ __forceinline__ void score_finish(const ScoreState& st, float tlogit, int tgt, int V, int row, float* logprob, float* lse, int32_t* top1) {
    const float lg = kf_logf(st.s);
    logprob[row] = tgt < 0 ? 0.0f : (tgt < V ? (tlogit - st.m) - lg : __builtin_nanf(""));
    if (lse) lse[row] = st.m + lg;
    if (top1) top1[row] = st.i;
}

struct ScoreArgs {
    const int32_t* targets;
    f32x4* part; /* [n][n_vt] */
    int n_vt, n_rb;
};

template <class C>
__global__ void __launch_bounds__(C::NTH, C::WGS_PER_CU * C::NW / 4) head_score_kernel(const GemmArgs a, const ScoreArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wg = g3_remap(blockIdx.x, s.n_vt * s.n_rb);
    const int bx = wg / s.n_rb, by = wg % s.n_rb; /* row blocks fast: the workgroups an XCD runs back to back share their tile of W */
    const int m0 = bx * C::BM, t0 = by * C::BN;
    f32x4 acc[C::MT][C::NT];
#pragma unroll
    for (int i = 0; i < C::MT; i++)
#pragma unroll
        for (int j = 0; j < C::NT; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    g3_mainloop<false, false, G3_BK, C>(a, m0, t0, 0, a.K / G3_BK, acc, smem_raw, wid, lane); /* ends with a barrier: the stage buffers are free */
    // lane (r16, q4) of wave (wm, wn): vocabulary rows m0 + wm 16 MT + 16 mt + 4 q4 + j of row (token) t0 + wn 16 NT + 16 nt + r16
    const int wm = wid / C::WN, wn = wid % C::WN, r16 = lane & 15, q4 = lane >> 4;
    const int vbase = m0 + wm * (16 * C::MT) + 4 * q4;
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw); /* [2 wm][BN] */
#pragma unroll
    for (int nt = 0; nt < C::NT; nt++) {
        const int col = wn * (16 * C::NT) + nt * 16 + r16, tok = t0 + col;
        const int tgt = tok < a.n ? s.targets[tok] : -1;
        ScoreState st = score_empty();
#pragma unroll
        for (int mt = 0; mt < C::MT; mt++)
#pragma unroll
            for (int j = 0; j < 4; j++) { /* ascending vocabulary index: > keeps the first maximum */
                const int v = vbase + mt * 16 + j;
                const float x = round_bf16(acc[mt][nt][j]);
                acc[mt][nt][j] = x;
                if (v < a.M && x > st.m) st.m = x, st.i = v;
                if (v == tgt) st.t = x;
            }
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) { /* the row's four lanes: maximum and its first index */
            const float om = __shfl_xor(st.m, off);
            const int oi = __shfl_xor(st.i, off);
            if (om > st.m || (om == st.m && oi < st.i)) st.m = om, st.i = oi;
            st.t += __shfl_xor(st.t, off);
        }
#pragma unroll
        for (int mt = 0; mt < C::MT; mt++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (vbase + mt * 16 + j < a.M) st.s += kf_expf(acc[mt][nt][j] - st.m);
        st.s += __shfl_xor(st.s, 16);
        st.s += __shfl_xor(st.s, 32);
        if (q4 == 0) red[wm * C::BN + col] = score_pack(st);
    }
    __syncthreads();
    if (tid < C::BN && t0 + tid < a.n) {
        const ScoreState st = score_merge(score_unpack(red[tid]), score_unpack(red[C::BN + tid]));
        s.part[(size_t)(t0 + tid) * s.n_vt + bx] = score_pack(st);
    }
}

__global__ void __launch_bounds__(64 * SCORE_MERGE_ROWS) score_merge_kernel(const f32x4* __restrict__ part, int n_vt, int bm, int V, int n, const int32_t* __restrict__ targets,
                                                                             float* logprob, float* lse, int32_t* top1) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * SCORE_MERGE_ROWS + (threadIdx.x >> 6);
    if (row >= n) return;
    const f32x4* pr = part + (size_t)row * n_vt;
    ScoreState st = score_empty();
    for (int vt = lane; vt < n_vt; vt += 64) st = score_merge(st, score_unpack(pr[vt]));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) st = score_merge(st, score_xor(st, off));
    if (lane == 0) {
        const int tgt = targets[row];
        const float tl = tgt >= 0 && tgt < V ? pr[tgt / bm].w : 0.0f;
        score_finish(st, tl, tgt, V, row, logprob, lse, top1);
    }
}

__global__ void __launch_bounds__(256) score_rows_kernel(const uint16_t* __restrict__ logits, long long ldl, int V, const int32_t* __restrict__ targets, float* logprob, float* lse,
                                                         int32_t* top1) {
    __shared__ f32x4 red[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, row = blockIdx.x;
    const uint16_t* lr = logits + (size_t)row * ldl;
    ScoreState st = score_empty();
    for (int v = tid; v < V; v += 256) { /* ascending per thread: > keeps the first maximum */
        const float x = bf2f(lr[v]);
        if (x > st.m) st.s = st.s * kf_expf(st.m - x) + 1.0f, st.m = x, st.i = v;
        else st.s += kf_expf(x - st.m);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) st = score_merge(st, score_xor(st, off));
    if (lane == 0) red[wid] = score_pack(st);
    __syncthreads();
    if (tid == 0) {
        st = score_unpack(red[0]);
        for (int w = 1; w < 4; w++) st = score_merge(st, score_unpack(red[w]));
        const int tgt = targets[row];
        const float tl = tgt >= 0 && tgt < V ? bf2f(lr[tgt]) : 0.0f;
        score_finish(st, tl, tgt, V, row, logprob, lse, top1);
    }
}

template <class C>
static int score_fused_c(hipStream_t st, const ScorePlan& p, const GemmArgs& a, const ScoreArgs& s) {
    constexpr int SMEM = 2 * C::STAGE;
    static_assert(2 * C::BN * 16 <= SMEM && C::BN <= C::NTH, "the epilogue's exchange fits the stage buffers, one thread per row of the tile");
    static int attr_set = 0;
    if (!attr_set && SMEM > 64 * 1024) {
        if (hipFuncSetAttribute((const void*)head_score_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM) != hipSuccess) return KF_HIP_CHECK;
        attr_set = 1;
    }
    hipLaunchKernelGGL((head_score_kernel<C>), dim3(p.gx), dim3(C::NTH), SMEM, st, a, s);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}
int score_fused_launch(hipStream_t st, const ScorePlan& p, const uint16_t* W, int V, int K, const uint16_t* x, long long ldx, int n, const int32_t* targets, float* logprob,
                       float* lse, int32_t* top1, void* scratch) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.w = reinterpret_cast<const unsigned char*>(W), a.M = V, a.K = K, a.x = x, a.ldx = ldx, a.n = n;
    ScoreArgs s;
    s.targets = targets, s.part = reinterpret_cast<f32x4*>(scratch), s.n_vt = p.n_vt, s.n_rb = p.n_rb;
    const int rc = p.form == G3_BIG ? score_fused_c<G3Big>(st, p, a, s) : score_fused_c<G3Small>(st, p, a, s);
    if (rc != KF_OK) return rc;
    hipLaunchKernelGGL(score_merge_kernel, dim3((unsigned)cdiv(n, SCORE_MERGE_ROWS)), dim3(64 * SCORE_MERGE_ROWS), 0, st, s.part, p.n_vt, G3_FORMS[p.form].bm, V, n, targets, logprob, lse,
                       top1);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}
int score_rows_launch(hipStream_t st, const uint16_t* logits, long long ldl, int V, int n, const int32_t* targets, float* logprob, float* lse, int32_t* top1) {
    hipLaunchKernelGGL(score_rows_kernel, dim3(n), dim3(256), 0, st, logits, ldl, V, targets, logprob, lse, top1);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
