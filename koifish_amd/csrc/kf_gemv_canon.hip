// kf_gemv_canon.hip -- the mat-vec kernels of kf_gemv_kernel.h in the CANONICAL summation order (oracle/kf_oracle.c section 4c): every pair of products is two
// v_fma_f32 (low element first) instead of one v_dot2c_f32_bf16, so that the host reproduces every output bit with fmaf.  A translation unit of its own, so that the
// two instantiation sets compile side by side.
#include "kf_gemv_kernel.h"

namespace kf {

int gemv_dispatch_canon(const GemvPlan& p, const GemvArgs& a, hipStream_t st) { return gemv_dispatch<true>(p, a, st); }

}  // namespace kf
