// kf_qknorm_rope_bwd.hip -- the backward of the per-head q/k RMSNorm + rotate-half RoPE (kf_qknorm_rope_train) in ONE pass over the attention backward's dq | dk | dv.
//
// Replaces, per layer of the Qwen3 backward, two in-place kf_rope_backward launches, three strided-to-dense copies, two zero fills and two kf_norm_backward launches
// (the backward branches of ROPE::cuFlow, kernel/rope.cu, and of LayerNormal::cuFlow, T.cu:605-646: CU_rms_back_llmc over n_tok * n_head rows of head_dim).  Per head row
// (row r = token t, head h; position t % seq_len; (c_j, s_j) = rope_table[pos][j]; half = head_dim / 2):
//   g_j = d_j c_j + d_{j+half} s_j;   g_{j+half} = d_{j+half} c_j - d_j s_j             the transpose of the rotation, as kf_rope_backward -- kept in fp32
//   B = sum_i (w_i g_i) raw_i;   dnn = B / head_dim * rstd;   norm_i = raw_i rstd
//   d_raw_i = bf16(((w_i g_i) - norm_i dnn) rstd);   dw_i += sum_rows norm_i g_i         kf_norm_backward's RMS branch on a zero-filled dinp
// One bf16 rounding fewer than the two-launch route (g never goes through bf16).  The gradients arrive as column blocks of fused rows (one ld_d), the raw q / k with a
// row stride each; d_raw and the copy of dv leave dense.
//
// HBM-bound: 2 reads + 1 write per q / k element, 1 + 1 per v element.  A head row belongs to head_dim / 16 lanes: lane l of the row holds columns [8 l, 8 l + 8) and
// their rotation partners [half + 8 l, half + 8 l + 8) -- two 16-byte loads per operand, the pair (j, j + half) in one lane, the row sum B inside the row's 4 or 8 lanes
// (DPP).  A workgroup takes 4 x 64 / LPR consecutive head rows per round (rows [(i G + w) nslot, ...) for workgroup w of G in round i); q rows, k rows and the v copy
// are blockIdx.y = 0, 1, 2 of one launch.
// No atomics: the weight-gradient column sums are fp64, over a lane's rows in round order, over the workgroup's lanes in (wave, row slot) order through LDS, then over
// the G workgroups by kf_norm_backward's reduce launch (8 contiguous chunks in index order, the chunk sums in order; bf16(fp32 sum + old gradient)).  Every partial the
// reduce reads is written by this launch first: the result does not depend on what the scratch held.
#include "kf_kernels.h"

namespace kf {

constexpr int QKB_MAX_GROUPS = 1024;

// rows per workgroup round: 4 waves x 64 / (hd / 16) rows
static int qkb_nslot(int hd) { return 4 * (64 / (hd / 16)); }
int qknorm_rope_backward_groups(long long rows, int hd) {
    const long long g = (rows + qkb_nslot(hd) - 1) / qkb_nslot(hd);
    return (int)(g < 1 ? 1 : (g > QKB_MAX_GROUPS ? QKB_MAX_GROUPS : g));
}

struct QkbArgs {
    const uint16_t *d[3];       /* dq, dk, dv: rows of stride ld_d */
    const uint16_t *raw[2];     /* pre-norm q, k */
    const uint16_t *w[2];
    const float *rstd[2];
    uint16_t *out[3];           /* dense dq_raw, dk_raw, dv_out */
    double *part[2];            /* [G][hd] column partials */
    long long ld_d, ld_raw[2];
    const float *table;
    const int *pos;             /* POS form: [n_tok] the rows' positions, in place of t % seq_len */
    int n_tok, seq_len, nh[2], G[2], Gv;
};

template <int HD, bool POS = false>
__global__ void __launch_bounds__(256) qknorm_rope_backward_kernel(QkbArgs a) {
    constexpr int LPR = HD / 16, RPW = 64 / LPR, NSLOT = 4 * RPW, HALF = HD / 2;
    const int tid = threadIdx.x, which = blockIdx.y;
    if (which == 2) { /* the dense copy of dv: n_tok rows of nh[1] * HD */
        if ((int)blockIdx.x >= a.Gv) return;
        const long long vpr = (long long)a.nh[1] * (HD / 8), total = (long long)a.n_tok * vpr;
        for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)a.Gv * 256) {
            const long long t = i / vpr, v = i - t * vpr;
            *reinterpret_cast<u32x4*>(a.out[2] + (size_t)i * 8) = *reinterpret_cast<const u32x4*>(a.d[2] + (size_t)t * a.ld_d + (size_t)v * 8);
        }
        return;
    }
    const int G = a.G[which];
    if ((int)blockIdx.x >= G) return; /* workgroup-uniform */
    __shared__ double red[4][16][72]; /* [wave][k][lane]: a wave stores 64 consecutive doubles per k, no bank conflict; 8 doubles of padding spread the readers' k over the banks */
    const int lane = tid & 63, wave = tid >> 6, ll = lane & (LPR - 1), slot = wave * RPW + lane / LPR;
    const int nh = a.nh[which];
    const long long rows = (long long)a.n_tok * nh;
    const uint16_t *dsrc = a.d[which], *raw = a.raw[which];
    const float* rstd = a.rstd[which];
    uint16_t* out = a.out[which];
    const long long ld_raw = a.ld_raw[which];
    float wf[16];
    {
        const u32x4 w0 = *reinterpret_cast<const u32x4*>(a.w[which] + ll * 8), w1 = *reinterpret_cast<const u32x4*>(a.w[which] + HALF + ll * 8);
        const uint32_t q0[4] = {w0.x, w0.y, w0.z, w0.w}, q1[4] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int k = 0; k < 4; k++) wf[2 * k] = bf_lo(q0[k]), wf[2 * k + 1] = bf_hi(q0[k]), wf[8 + 2 * k] = bf_lo(q1[k]), wf[8 + 2 * k + 1] = bf_hi(q1[k]);
    }
    double dw[16];
#pragma unroll
    for (int k = 0; k < 16; k++) dw[k] = 0.0;
    for (long long i = 0;; i++) {
        const long long r0 = (i * G + blockIdx.x) * NSLOT; /* the first row of this round: workgroup-uniform exit */
        if (r0 >= rows) break;
        const bool ok = r0 + slot < rows;
        const long long r = ok ? r0 + slot : r0;
        const long long t = r / nh;
        const int h = (int)(r - t * nh);
        const size_t od = (size_t)t * a.ld_d + (size_t)h * HD + ll * 8, orw = (size_t)t * ld_raw + (size_t)h * HD + ll * 8;
        const u32x4 d0 = *reinterpret_cast<const u32x4*>(dsrc + od), d1 = *reinterpret_cast<const u32x4*>(dsrc + od + HALF);
        const u32x4 x0 = *reinterpret_cast<const u32x4*>(raw + orw), x1 = *reinterpret_cast<const u32x4*>(raw + orw + HALF);
        const float* cs = a.table + ((size_t)(POS ? a.pos[t] : (int)(t % a.seq_len)) * HALF + ll * 8) * 2;
        f32x4 tb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) tb[k] = *reinterpret_cast<const f32x4*>(cs + 4 * k); /* (c, s) of columns 2k, 2k + 1 */
        const float rs = rstd[r];
        const uint32_t dq0[4] = {d0.x, d0.y, d0.z, d0.w}, dq1[4] = {d1.x, d1.y, d1.z, d1.w}, xq0[4] = {x0.x, x0.y, x0.z, x0.w}, xq1[4] = {x1.x, x1.y, x1.z, x1.w};
        float g[16], x[16];
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const float lo = e ? bf_hi(dq0[k]) : bf_lo(dq0[k]), hi = e ? bf_hi(dq1[k]) : bf_lo(dq1[k]);
                const float c = e ? tb[k].z : tb[k].x, s = e ? tb[k].w : tb[k].y;
                const float p0 = lo * c, p1 = hi * s, p2 = hi * c, p3 = lo * s;
                g[2 * k + e] = p0 + p1;
                g[8 + 2 * k + e] = p2 - p3;
                x[2 * k + e] = e ? bf_hi(xq0[k]) : bf_lo(xq0[k]);
                x[8 + 2 * k + e] = e ? bf_hi(xq1[k]) : bf_lo(xq1[k]);
            }
        }
        double sb = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const float dn = wf[k] * g[k];
            sb += (double)(dn * x[k]);
        }
        sb += dpp_d<0xB1>(sb);
        sb += dpp_d<0x4E>(sb);
        if (LPR == 8) sb += dpp_d<0x141>(sb);
        const float dnn = (float)sb / (float)HD * rs;
        uint32_t o0[4], o1[4];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float res[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int c = 2 * k + e;
                const float norm = x[c] * rs;
                if (ok) dw[c] += (double)(norm * g[c]);
                float dval = wf[c] * g[c];
                dval -= norm * dnn;
                dval *= rs;
                res[e] = dval;
            }
            if (k < 4) o0[k] = pack_bf16x2(res[0], res[1]);
            else o1[k - 4] = pack_bf16x2(res[0], res[1]);
        }
        if (ok) {
            uint16_t* po = out + (size_t)r * HD + ll * 8;
            *reinterpret_cast<u32x4*>(po) = u32x4{o0[0], o0[1], o0[2], o0[3]};
            *reinterpret_cast<u32x4*>(po + HALF) = u32x4{o1[0], o1[1], o1[2], o1[3]};
        }
    }
    // column partials: every lane to LDS, then thread c < HD sums the lanes that hold column c in (wave, row slot) order
#pragma unroll
    for (int k = 0; k < 16; k++) red[wave][k][lane] = dw[k];
    __syncthreads();
    if (tid < HD) {
        const int hi = tid >= HALF, cc = tid - hi * HALF, l0 = cc >> 3, k = hi * 8 + (cc & 7);
        double tw = 0.0;
        for (int w2 = 0; w2 < 4; w2++)
            for (int rr = 0; rr < RPW; rr++) tw += red[w2][k][rr * LPR + l0];
        a.part[which][(size_t)blockIdx.x * HD + tid] = tw;
    }
}

size_t qknorm_rope_backward_scratch_bytes(int n_tok, int n_head, int n_kv, int hd) {
    if (n_tok < 1 || n_head < 1 || n_kv < 1 || n_head % n_kv || (hd != 64 && hd != 128)) return 0;
    return sizeof(double) * (size_t)hd * ((size_t)qknorm_rope_backward_groups((long long)n_tok * n_head, hd) + (size_t)qknorm_rope_backward_groups((long long)n_tok * n_kv, hd));
}

int qknorm_rope_backward_launch(hipStream_t st, const uint16_t* dq, const uint16_t* dk, const uint16_t* dv, long long ld_d, const uint16_t* q_raw, long long ld_qraw,
                                const uint16_t* k_raw, long long ld_kraw, const uint16_t* wq, const uint16_t* wk, const float* rstd_q, const float* rstd_k, const float* table,
                                int n_tok, int seq_len, int n_head, int n_kv, int hd, uint16_t* dq_raw, uint16_t* dk_raw, uint16_t* dv_out, uint16_t* dwq, uint16_t* dwk,
                                double* scratch, const int* pos) { /* pos != NULL: the POS form, seq_len is not read */
    if (qknorm_rope_backward_scratch_bytes(n_tok, n_head, n_kv, hd) == 0 || (!pos && (seq_len < 1 || n_tok % seq_len))) return KF_INVALID_ARGS;
    QkbArgs a;
    a.d[0] = dq, a.d[1] = dk, a.d[2] = dv, a.raw[0] = q_raw, a.raw[1] = k_raw, a.w[0] = wq, a.w[1] = wk, a.rstd[0] = rstd_q, a.rstd[1] = rstd_k;
    a.out[0] = dq_raw, a.out[1] = dk_raw, a.out[2] = dv_out;
    a.ld_d = ld_d, a.ld_raw[0] = ld_qraw, a.ld_raw[1] = ld_kraw, a.table = table, a.pos = pos, a.n_tok = n_tok, a.seq_len = pos ? 1 : seq_len, a.nh[0] = n_head, a.nh[1] = n_kv;
    a.G[0] = qknorm_rope_backward_groups((long long)n_tok * n_head, hd), a.G[1] = qknorm_rope_backward_groups((long long)n_tok * n_kv, hd);
    a.part[0] = scratch, a.part[1] = scratch + (size_t)a.G[0] * hd;
    const long long vvec = (long long)n_tok * n_kv * (hd / 8);
    a.Gv = dv ? (int)((vvec + 255) / 256 > QKB_MAX_GROUPS ? QKB_MAX_GROUPS : (vvec + 255) / 256) : 0;
    const int gx = a.G[0] > a.Gv ? a.G[0] : a.Gv; /* G[1] <= G[0]: n_kv <= n_head */
    const auto kern = pos ? (hd == 64 ? qknorm_rope_backward_kernel<64, true> : qknorm_rope_backward_kernel<128, true>)
                          : (hd == 64 ? qknorm_rope_backward_kernel<64, false> : qknorm_rope_backward_kernel<128, false>);
    hipLaunchKernelGGL(kern, dim3(gx, dv ? 3 : 2), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return KF_HIP_CHECK;
    int rc = norm_backward_reduce_launch(st, dwq, a.part[0], a.G[0], hd);
    if (rc == KF_OK) rc = norm_backward_reduce_launch(st, dwk, a.part[1], a.G[1], hd);
    return rc;
}

}  // namespace kf
