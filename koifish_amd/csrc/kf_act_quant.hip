// kf_act_quant.hip -- kf_act_quant_i8: the per-token symmetric int8 activation quantiser in front of the integer mat-vec (huTensor::Quant4A -> CU_X2A8_, T.cu:24-102,
// with the ABSOLUTE row maximum: include/kf_abi.h "int8 activations").  One workgroup per row; an optional RMSNorm prologue norms the row and rounds it to bf16 exactly
// as kf_rmsnorm stores it (rmsnorm_kernel, kf_ops.hip) before it is quantised, so q | k | v and gate | up share one launch for norm + quantise.
#include "kf_a8.h"

namespace kf {

__global__ void __launch_bounds__(256) act_quant_kernel(const uint16_t* __restrict__ x, long long ldx, const uint16_t* __restrict__ norm_w, float eps, float inv_dim, int dim,
                                                        int8_t* __restrict__ q, float* __restrict__ step) {
    __shared__ double red[16];
    __shared__ float mx[4];
    const uint16_t* xr = x + (size_t)blockIdx.x * ldx;
    int8_t* qr = q + (size_t)blockIdx.x * dim;
    float mul = 1.0f;
    if (norm_w) {
        const double ss = block_sumsq_bf16(xr, dim, red);
        mul = rms_scale((float)ss, inv_dim, eps);
    }
    auto value = [&](int i) { return norm_w ? round_bf16((bf2f(xr[i]) * mul) * bf2f(norm_w[i])) : bf2f(xr[i]); };
    float m = 0.0f;
    for (int i = threadIdx.x; i < dim; i += blockDim.x) m = fmaxf(m, fabsf(value(i)));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3]));
    const float s = __fdiv_rn(amax, 127.0f); /* IEEE division: a multiply by a reciprocal changes bits and is not the definition */
    for (int i = threadIdx.x; i < dim; i += blockDim.x) {
        float r = 0.0f;
        if (amax != 0.0f) r = fminf(fmaxf(roundf(__fdiv_rn(value(i), s)), -127.0f), 127.0f); /* std::round: halves away from zero (T.cu:60) */
        qr[i] = (int8_t)(int)r;
    }
    if (threadIdx.x == 0) step[blockIdx.x] = s;
}

int act_quant_launch(hipStream_t st, const uint16_t* x, long long ldx, const uint16_t* norm_w, float eps, int rows, int dim, int8_t* q, float* step) {
    hipLaunchKernelGGL(act_quant_kernel, dim3(rows), dim3(256), 0, st, x, ldx, norm_w, eps, 1.0f / (float)dim, dim, q, step);
    return hipGetLastError() == hipSuccess ? KF_OK : KF_HIP_CHECK;
}

}  // namespace kf
