// kf_distill.hip -- distilling classifier: cross entropy against hard labels + temperature-scaled KL(teacher || student) against a teacher's logits, per token row,
// and the gradient of their weighted sum written over the student's logits.  The contract and the order of operations are stated in include/kf_abi.h
// (kf_distill_classifier) and restated in numpy by tests/distill_restate.py; this file follows them line by line.  There is nothing to port: the reference's
// src/Fuzi/Distillation.hpp is a stub and src/Device/CUDA/Distill.cu a forward-only attention-relation loss that is not built here.
//
// One workgroup of 1024 threads per row, rows in reverse order, 16-byte loads of both rows -- kf_loss.hip's decomposition, so that the student's temperature-1
// statistics (m_z, S1), p and the CE term are fused_classifier_kernel's to the bit.  A row pair at the Qwen3 vocabulary is 608 KB and does not fit LDS: three sweeps.
//   sweep 1   z: the running (max, sum) of kf_loss.hip;  u: the running max.       Block max of both, the rescale, block sum -> m_z, S1, m_u
//   sweep 2   (KD only) with both maxima known, per thread in sweep 1's visiting order:  st += exp((z - m_z) it),  eu = exp((u - m_u) it),  ut += eu,
//             A = fma(eu, ((u - m_u) - (z - m_z)) it, A);  three block sums -> S_t, U_t, A.  The z and u sums run through the SAME chain and trees: u == z
//             gives U_t == S_t bit for bit and A == 0
//   sweep 3   (write_dlogits) every element once, ascending as kf_loss.hip: the gradient over the logit
// Six kf_expf per element with KD (1 + 2 + 3), two without; sweeps 2 and 3 re-read rows that sweep 1 left in L2 / MALL.
#include "kf_kernels.h"

namespace kf {
namespace {

template <bool IS_MAX>
__device__ __forceinline__ float half_wave_butterfly(float v) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = IS_MAX ? fmaxf(v, o) : v + o;
    }
    return v;
}
// kf_loss.hip's block_reduce_1024: 32 groups of 32 threads, the butterfly inside each, the 32 results through LDS, the butterfly again
template <bool IS_MAX>
__device__ __forceinline__ float block_reduce_1024(float v, float* sh) {
    const int grp = threadIdx.x >> 5, l32 = threadIdx.x & 31;
    __syncthreads(); /* sh may still be read by the previous reduction */
    v = half_wave_butterfly<IS_MAX>(v);
    if (l32 == 0) sh[grp] = v;
    __syncthreads();
    return half_wave_butterfly<IS_MAX>(sh[l32]);
}

// thread tid's elements in kf_loss.hip's order: the 8-element vectors i = ceil(V/8) + tid - 1024, i - 1024, ... >= 0, highest first, the elements of a vector
// ascending, the ragged last vector bounds-checked.  f(z, u); u = 0 without a teacher row
template <bool KD, class F>
__device__ __forceinline__ void visit_desc(const uint16_t* __restrict__ row, const uint16_t* __restrict__ urow, int V, int tid, F&& f) {
    int i = (V + 7) / 8 + tid - 1024;
    while (i >= 0 && (i + 1) * 8 > V) {
        for (int k = 0; k < 8 && i * 8 + k < V; k++) f(bf2f(row[i * 8 + k]), KD ? bf2f(urow[i * 8 + k]) : 0.0f);
        i -= 1024;
    }
    for (; i >= 0; i -= 1024) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(row + (size_t)i * 8);
        const u32x4 r = KD ? *reinterpret_cast<const u32x4*>(urow + (size_t)i * 8) : u32x4{0u, 0u, 0u, 0u};
        const uint32_t w[4] = {q.x, q.y, q.z, q.w}, x[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; k++) f(bf_lo(w[k]), bf_lo(x[k])), f(bf_hi(w[k]), bf_hi(x[k]));
    }
}

template <bool KD>
__global__ void __launch_bounds__(1024) distill_classifier_kernel(uint16_t* __restrict__ logits, const uint16_t* __restrict__ teacher, long tld, float* __restrict__ losses,
                                                                  float* __restrict__ kd, float dloss, const int* __restrict__ targets, int V, int P,
                                                                  const int* __restrict__ mask, float a, float b, float tau, int write_dlogits) {
    __shared__ float sh[32];
    const long idx = (long)gridDim.x - ((long)blockIdx.x + 1); /* reverse order, as kf_loss.hip */
    if (mask && (mask[idx] & 0x10000)) return;
    const bool ce = a != 0.0f;
    const int ix = ce ? targets[idx] : -1; /* ce_weight == 0: the targets are not read, no element is the target */
    uint16_t* const row = logits + idx * (long)P;
    const uint16_t* const urow = KD ? teacher + idx * tld : nullptr;
    const int tid = threadIdx.x;
    const float it = 1.0f / tau;

    // sweep 1
    float tmax = -__builtin_inff(), tsum = 0.0f, umax = -__builtin_inff();
    visit_desc<KD>(row, urow, V, tid, [&](float v, float u) {
        if (v > tmax) {
            if (tmax != -__builtin_inff()) tsum *= kf_expf(tmax - v);
            tmax = v;
        }
        tsum += kf_expf(v - tmax);
        if (KD) umax = fmaxf(umax, u);
    });
    const float bmax = block_reduce_1024<true>(tmax, sh);
    tsum *= kf_expf(tmax - bmax); /* a thread without elements: 0 * exp(-inf) = 0 */
    const float bsum = block_reduce_1024<false>(tsum, sh);
    const float scale = 1.0f / bsum;

    // sweep 2
    float mu = 0.0f, rst = 0.0f, rut = 0.0f, kl = 0.0f;
    if (KD) {
        mu = block_reduce_1024<true>(umax, sh);
        float st = 0.0f, ut = 0.0f, at = 0.0f;
        visit_desc<true>(row, urow, V, tid, [&](float v, float u) {
            const float dz = v - bmax, du = u - mu;
            st += kf_expf(dz * it);
            const float eu = kf_expf(du * it);
            ut += eu;
            at = fmaf(eu, (du - dz) * it, at);
        });
        const float St = block_reduce_1024<false>(st, sh);
        const float Ut = block_reduce_1024<false>(ut, sh);
        const float At = block_reduce_1024<false>(at, sh);
        kl = (At / Ut - kf_logf(Ut)) + kf_logf(St);
        rst = 1.0f / St, rut = 1.0f / Ut;
    }

    if (tid == 0) {
        float c = 0.0f;
        if (ce) c = a * -kf_logf(kf_expf(bf2f(row[ix]) - bmax) * scale);
        if (KD) {
            const float w = (b * tau) * tau;
            c = ce ? fmaf(w, kl, c) : w * kl;
            if (kd) kd[idx] = kl;
        }
        losses[idx] += c;
    }
    if (!write_dlogits) return;
    __syncthreads(); /* the target logit is read before anyone overwrites the row */

    // sweep 3
    const float bt = b * tau;
    auto grad = [&](float v, float u, int e) {
        const float dz = v - bmax;
        float t = ce ? a * (kf_expf(dz) * scale - (e == ix ? 1.0f : 0.0f)) : 0.0f;
        if (KD) t = fmaf(bt, kf_expf(dz * it) * rst - kf_expf((u - mu) * it) * rut, t);
        return t * dloss;
    };
    const int nvec = V / 8;
    for (int v8 = tid; v8 < nvec; v8 += 1024) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(row + (size_t)v8 * 8);
        const u32x4 r = KD ? *reinterpret_cast<const u32x4*>(urow + (size_t)v8 * 8) : u32x4{0u, 0u, 0u, 0u};
        const uint32_t w[4] = {q.x, q.y, q.z, q.w}, x[4] = {r.x, r.y, r.z, r.w};
        uint32_t g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = pack_bf16x2(grad(bf_lo(w[k]), bf_lo(x[k]), v8 * 8 + 2 * k), grad(bf_hi(w[k]), bf_hi(x[k]), v8 * 8 + 2 * k + 1));
        *reinterpret_cast<u32x4*>(row + (size_t)v8 * 8) = u32x4{g[0], g[1], g[2], g[3]};
    }
    for (int e = nvec * 8 + tid; e < V; e += 1024) row[e] = f2bf(grad(bf2f(row[e]), KD ? bf2f(urow[e]) : 0.0f, e));
}

}  // namespace

int distill_classifier_launch(hipStream_t st, uint16_t* logits, const uint16_t* teacher, long teacher_ld, float* losses, float* kd, float dloss, const int* targets,
                              long rows, int V, int P, const int* mask, float ce_weight, float kd_weight, float temperature, int write_dlogits) {
    if (rows < 1 || rows > 0x7fffffffL || V < 1 || P < V || (P % 8) != 0) return KF_INVALID_ARGS;
    if (kd_weight != 0.0f) {
        if (!teacher || teacher_ld < V || (teacher_ld % 8) != 0) return KF_INVALID_ARGS;
        hipLaunchKernelGGL(distill_classifier_kernel<true>, dim3((unsigned)rows), dim3(1024), 0, st, logits, teacher, teacher_ld, losses, kd, dloss, targets, V, P, mask,
                           ce_weight, kd_weight, temperature, write_dlogits);
    } else {
        hipLaunchKernelGGL(distill_classifier_kernel<false>, dim3((unsigned)rows), dim3(1024), 0, st, logits, (const uint16_t*)nullptr, 0L, losses, (float*)nullptr, dloss,
                           targets, V, P, mask, ce_weight, kd_weight, temperature, write_dlogits);
    }
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
