// kf_head_screen.hip -- the int8 screen copy of a bf16 [vocab, dim] LM head (kf_engine_set_head_screen): what the decode engine streams instead of the head itself on the
// steps of a multi-step launch whose logits nobody can observe (kf_engine.hip, eng_head_main).  Built once, on the device, from the exact bf16 values.
//
// Layout of the caller's buffer: [q8: vocab x dim bytes, biased (q + 128), rounded up to 256 B] [vocab x {float scale, float E}].
//   scale_r = absmax_r / 127 (fp32), q = rint(w / scale) in [-127, 127], w^_i = scale * q_i.
//   E_r bounds |approx_r - exact_r| / ||x||_2 for ANY activation vector x, where approx_r is the engine's fp32 evaluation of scale_r * sum((u_i - 128) x_i) and exact_r the
//   fp32 value the exact head chain leaves in front of its bf16 store:
//     |sum (w_i - w^_i) x_i|            <= ||w_r - w^_r||_2 ||x||_2                      (Cauchy-Schwarz; the norm is taken in fp64 from the exact bf16 values)
//     |approx_r - sum w^_i x_i|         <= gamma * scale_r * sum (|u_i| + 128) |x_i|    <= gamma * scale_r * 383 sqrt(dim) ||x||_2
//     |exact_r  - sum w_i x_i|          <= gamma * sum |w_i x_i|                        <= gamma * ||w_r||_2 ||x||_2
//   gamma = 2^-16 >= gamma_128 = 128 u / (1 - 128 u), u = 2^-24: no product of either evaluation passes through more than 128 fp32 roundings (the screen: two chains of
//   <= 16 fmas per lane, their join, the bias term, a 6-level tree, the scale; the exact chain: <= 32 products per lane -- at most three roundings each in the v_dot2c form -- a join and the
//   same tree).  E_r = (err2_r (1 + 2^-20) + gamma (scale_r 383 sqrt(dim) + ||w_r||_2)) rounded UP to fp32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_device.h"
#include "kf_kernels.h"

namespace kf {

size_t head_screen_bytes(int vocab, int dim) {
    if (vocab < 1 || dim < 16 || (dim % 16) != 0) return 0;
    return (((size_t)vocab * dim + 255) & ~(size_t)255) + (((size_t)vocab * 8 + 255) & ~(size_t)255);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// one wave per row
__global__ void __launch_bounds__(256) head_screen_build_kernel(const uint16_t* __restrict__ w, int vocab, int dim, uint8_t* __restrict__ q8, float2* __restrict__ rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= vocab) return;
    const uint16_t* wr = w + (size_t)row * dim;
    float amax = 0.f;
    for (int i = lane; i < dim; i += 64) amax = fmaxf(amax, fabsf(bf2f(wr[i])));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
    const float scale = amax / 127.0f;
    const bool ok = scale > 0.f && scale < __builtin_inff(); /* an all-zero row (or one with a non-finite value) keeps q = 0: its bound is then ||w_r|| itself */
    double e2 = 0.0, w2 = 0.0;
    for (int i = lane; i < dim; i += 64) {
        const float v = bf2f(wr[i]);
        float q = ok ? rintf(v / scale) : 0.f;
        q = fminf(fmaxf(q, -127.f), 127.f);
        q8[(size_t)row * dim + i] = (uint8_t)((int)q + 128);
        const double d = (double)v - (double)scale * (double)q; /* scale * q is exact in fp64 (24 + 8 bits) */
        e2 = fma(d, d, e2), w2 = fma((double)v, (double)v, w2);
    }
    e2 = wave_sum_d(e2), w2 = wave_sum_d(w2);
    if (lane == 0) {
        const double gamma = 1.0 / 65536.0;
        const double E = sqrt(e2) * (1.0 + 1.0 / 1048576.0) + gamma * ((double)scale * 383.0 * sqrt((double)dim) + sqrt(w2) * (1.0 + 1.0 / 1048576.0));
        float Ef = __double2float_ru(E);
        if (!(Ef == Ef)) Ef = __builtin_inff(); /* a NaN in the row: an infinite bound keeps the row a candidate on every step */
        rows[row] = float2{ok ? scale : 0.f, Ef};
    }
}

int head_screen_build(const uint16_t* head, int vocab, int dim, void* buf, size_t bytes, hipStream_t st) {
    if (!head || !buf || ((uintptr_t)buf & 255) != 0 || head_screen_bytes(vocab, dim) == 0 || bytes < head_screen_bytes(vocab, dim)) return KF_INVALID_ARGS;
    uint8_t* q8 = reinterpret_cast<uint8_t*>(buf);
    float2* rows = reinterpret_cast<float2*>(q8 + (((size_t)vocab * dim + 255) & ~(size_t)255));
    hipLaunchKernelGGL(head_screen_build_kernel, dim3((vocab + 3) / 4), dim3(256), 0, st, head, vocab, dim, q8, rows);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
