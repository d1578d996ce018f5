// kf_attn_seqs.hip -- decode attention for n_seq INDEPENDENT sequences in one launch (include/kf_abi.h kf_attn_block_seqs): sequence s brings one new token at its own
// position pos[s] of its own cache rows row0[s] .. row0[s] + pos[s].  gfx950 / wave64.
//
// The work: grid = (slices of the LONGEST sequence, sequence x kv-head x part).  y's leading index walks the sequences in the order the entry dealt them (a.order: the
// longest key walks first, so the short ones fill the tail of the launch); every workgroup reads ITS sequence's position and row origin from the device tables, cuts the
// sequence's keys by attn_slices -- the one rule, at the sequence's own position: the cut kf_attn_block would make there -- and leaves at once when its x lies past that
// count or the sequence is parked (pos < 0).  So a short sequence costs the workgroups of its own slices and nothing else, a one-slice sequence writes its output row
// without a hand-off, and a sequence's arrival counters wait for its own slice count.
// Data: a workgroup streams its slice of K and V once, 16 bytes per lane and row, ATTN_U tiles in flight, for the (at most ATTN_CANON_GQ_WG) query heads of its part: the
// heads share every K / V tile in registers.  Nothing is loaded before the position is read: the tables are device memory (parked sequences, positions the host only
// bounds), and a row past a sequence's position may belong to its neighbour's region.  The q heads and the new key are normed + roped into LDS by one wave each
// (load_head / prep_head); the slice that holds the position takes the new key from LDS and the new value row from v_raw, and part 0 of the kv-head writes both rows to
// the cache.
// Arithmetic: the canonical order only (kf_attn_common.h: canon_batch, canon_wave_to_lds, canon_slice_publish, canon_arrive_and_merge -- the bodies attn_kernel runs), which
// does not depend on launch geometry: every output row and every cache row written carries the bits of kf_attn_block on that sequence alone.
// Scratch: one decode scratch per sequence (counters, then [n_head][n_splits][hd + 2] doubles), s * attn_decode_scratch_bytes apart; counters return to zero.
#include "kf_attn_common.h"
#include "kf_attn_plan.h"

namespace kf {

template <int GQ, int HD>
__global__ void __launch_bounds__(ATTN_SEQS_NW * 64) attn_seqs_kernel(const AttnSeqsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int NW = ATTN_SEQS_NW, hd = HD, PS = hd + 2;
    using Slice = AttnSlice<GQ, NW, HD, 8>;
    constexpr int LPK = Slice::LPK, KPW = Slice::KPW, lpk_log2 = Slice::lpk_log2, tstride = Slice::tstride, NQ = Slice::NQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr AttnCanonLds lds(GQ, NW, HD);
    static_assert(lds.fits(), "LDS");
    double* comb = reinterpret_cast<double*>(smem_raw + lds.comb);
    uint16_t* qb = reinterpret_cast<uint16_t*>(smem_raw + lds.qb);
    uint16_t* knew = reinterpret_cast<uint16_t*>(smem_raw + lds.knew);
    int* flag = reinterpret_cast<int*>(smem_raw + lds.flag);

    // ---- which sequence, which (kv-head, part), which of ITS slices: all workgroup-uniform (scalar) work
    const int per_seq = a.n_kv * a.gq_split, si = (int)blockIdx.y / per_seq, y = (int)blockIdx.y - si * per_seq;
    const unsigned long long ow = (si >> 3) == 0 ? a.order[0] : (si >> 3) == 1 ? a.order[1] : (si >> 3) == 2 ? a.order[2] : a.order[3];
    const int s = (int)((ow >> ((si & 7) * 8)) & 0xff);
    const int pos = a.pos[s];
    if (pos < 0) return; /* parked: nothing read, nothing written */
    const AttnSlices cut = attn_slices(pos, a.n_kv, GQ * a.gq_split);
    const int nsp = cut.n_splits;
    if ((int)blockIdx.x >= nsp) return;
    if (nsp > (int)gridDim.x) return; /* the host's mirror broke its promise (h_pos < d_pos): the grid is short of this sequence's slices, so NONE of its workgroups runs --
                                         its row and cache rows stay untouched and its counters at zero, instead of partials that no workgroup would ever merge */
    const Slice sl(a.gq_split, cut.chunk, y);
    const size_t base = (size_t)a.row0[s] * a.kv_stride + (size_t)sl.kvh * hd;
    uint16_t* const kc = a.kcache + base; /* this kv-head's column of the sequence's rows */
    uint16_t* const vc = a.vcache + base;
    const uint16_t* const qsrc = a.q + (size_t)s * a.q_stride;
    const uint16_t* const vsrc = a.v_raw + (size_t)s * a.v_stride + (size_t)sl.kvh * hd;
    uint16_t* const odst = a.out + (size_t)s * a.out_stride;
    const int h0 = sl.h0(), grp = lane >> lpk_log2, d0 = (lane & (LPK - 1)) * 8, tstart = sl.tstart(wave, grp);
    const int t1 = sl.end(pos);
    const bool empty = sl.t0 > pos;

    u32x4 kk[ATTN_U], vv[ATTN_U];
    auto issue = [&](int tb) {
#pragma unroll
        for (int u = 0; u < ATTN_U; u++) {
            const int t = tb + u * tstride;
            kk[u] = u32x4{0, 0, 0, 0}, vv[u] = u32x4{0, 0, 0, 0};
            if (t < t1) {
                const size_t off = (size_t)t * a.kv_stride + d0;
                kk[u] = *reinterpret_cast<const u32x4*>(kc + off);
                vv[u] = *reinterpret_cast<const u32x4*>(vc + off);
            }
        }
    };
    issue(tstart);
    HeadRaw qraw[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const int hq = wave + i * NW;
        qraw[i] = load_head(qsrc + (size_t)(h0 + (hq < GQ ? hq : 0)) * hd, a.wq_norm, hd);
    }
    const HeadRaw kraw = load_head(a.k_raw + (size_t)s * a.k_stride + (size_t)sl.kvh * hd, a.wk_norm, hd);
    const u32x4 vnew = *reinterpret_cast<const u32x4*>(vsrc + d0); /* this lane's 8 dims of the new value row */

    const size_t seq_scratch = (size_t)s * attn_decode_scratch_bytes(a.n_head, HD);
    double* const part = a.part + seq_scratch / sizeof(double);

    if (!empty) {
        // ---- prologue: the q heads of this part and, in the slice that holds the position, the new key
        const float* tab_pos = a.rope_table + (size_t)pos * hd;
#pragma unroll
        for (int i = 0; i < NQ; i++)
            if (wave + i * NW < GQ) prep_head(qraw[i], a.wq_norm != nullptr, tab_pos, hd, a.eps, qb + (wave + i * NW) * hd);
        const bool own_new = sl.holds(pos, t1);
        if (own_new && wave == (GQ % NW)) prep_head(kraw, a.wk_norm != nullptr, tab_pos, hd, a.eps, knew);
        __syncthreads();
        if (own_new && sl.gpart == 0) { /* every part of the kv-head holds the same rows: one writes them */
            const size_t rowoff = (size_t)pos * a.kv_stride;
            for (int i = tid; i < hd; i += blockDim.x) kc[rowoff + i] = knew[i], vc[rowoff + i] = vsrc[i];
        }
        float qf[GQ][8];
#pragma unroll
        for (int hq = 0; hq < GQ; hq++) {
            const u32x4 qv = *reinterpret_cast<const u32x4*>(qb + hq * hd + d0);
            const uint32_t q4[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int i = 0; i < 4; i++) qf[hq][2 * i] = bf_lo(q4[i]), qf[hq][2 * i + 1] = bf_hi(q4[i]);
        }
        CanonAcc<GQ> A;
        A.init();
        const float rden = 1.0f / a.inv_sqrt_hd_den;
        for (int tb = tstart; tb - grp - wave * KPW < t1; tb += ATTN_U * tstride) { /* workgroup-uniform trip count */
            u32x4 ck[ATTN_U], cv[ATTN_U];
            bool valid[ATTN_U];
#pragma unroll
            for (int u = 0; u < ATTN_U; u++) {
                const int t = tb + u * tstride;
                ck[u] = kk[u], cv[u] = vv[u], valid[u] = t < t1;
                if (valid[u] && t == pos) ck[u] = *reinterpret_cast<const u32x4*>(knew + d0), cv[u] = vnew;
            }
            if (tb - grp - wave * KPW + ATTN_U * tstride < t1) issue(tb + ATTN_U * tstride);
            canon_batch<GQ, LPK>(A, qf, ck, cv, valid, lpk_log2, rden);
        }
        canon_wave_to_lds<GQ, LPK>(A, comb + (size_t)wave * GQ * PS, hd, lane, d0);
        __syncthreads();
        canon_slice_publish<GQ, NW, HD>(comb, part, odst, h0, nsp, sl.split);
    } else if (nsp > 1) { /* a slice behind the position: a neutral partial, but it still arrives */
        canon_slice_publish_empty<GQ, HD>(part, h0, nsp, sl.split);
    }
    if (nsp == 1) return;
    canon_arrive_and_merge<GQ, NW, HD>(part, a.counters + seq_scratch / sizeof(int) + y * a.cnt_stride, flag, odst, h0, nsp); /* per (sequence, kv-head, part) */
}

using AttnSeqsKernel = void (*)(AttnSeqsArgs);
int attn_seqs_launch(hipStream_t st, AttnSeqsArgs& a, const AttnPlan& p) {
    if (p.status != KF_OK) return p.status;
    if (p.route != ATTN_SLICED_SEQS || p.nw != ATTN_SEQS_NW) return KF_INTERNAL_ERR;
    const AttnSeqsKernel k = p.gq == 1   ? (p.hd == 128 ? attn_seqs_kernel<1, 128> : attn_seqs_kernel<1, 64>)
                             : p.gq == 2 ? (p.hd == 128 ? attn_seqs_kernel<2, 128> : attn_seqs_kernel<2, 64>)
                                         : nullptr;
    if (!k) return KF_INTERNAL_ERR; /* a form attn_plan never names */
    if (p.grid[0] == 0) return KF_OK; /* the plan's empty grid: every sequence parked */
    a.gq_split = p.gq_split, a.cnt_stride = p.cnt_stride;
    a.inv_sqrt_hd_den = sqrtf((float)p.hd);
    void* args[] = {&a};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(k), dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(p.threads), args, (size_t)p.lds, st);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

// ---- the slots' bookkeeping between two steps of a batched decode (kf_seqs_advance): one thread per sequence.  A live sequence (pos >= 0) takes the id picked for it,
// appends it to its ids and moves on one position; it parks (pos = -1) on `eos` or with its max_new-th id.  A parked sequence is left alone.
__global__ void __launch_bounds__(64) seqs_advance_kernel(const int* __restrict__ top1, int* __restrict__ tok, int* __restrict__ pos, int* __restrict__ count, int* __restrict__ ids,
                                                          int ids_stride, int max_new, int eos, int n_seq) {
    const int s = threadIdx.x;
    if (s >= n_seq) return;
    const int p = pos[s];
    if (p < 0) return;
    const int id = top1[s], c = count[s];
    if (c < ids_stride) ids[(size_t)s * ids_stride + c] = id;
    count[s] = c + 1, tok[s] = id;
    pos[s] = (id == eos || c + 1 >= max_new) ? -1 : p + 1;
}
int seqs_advance_launch(hipStream_t st, const int* top1, int* tok, int* pos, int* count, int* ids, int ids_stride, int max_new, int eos, int n_seq) {
    hipLaunchKernelGGL(seqs_advance_kernel, dim3(1), dim3(64), 0, st, top1, tok, pos, count, ids, ids_stride, max_new, eos, n_seq);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
