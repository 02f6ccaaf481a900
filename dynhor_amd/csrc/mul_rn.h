// A product that nothing can contract into an fma: HIP's __fmul_rn is a plain operator that hipcc fuses with a following add (also
// under `#pragma clang fp contract(off)` once inlined), so kernels whose fp32 operations must round one by one -- to agree bit for bit
// with a tensor expression of the same operations (march.hip, trace.hip) -- multiply through this one-instruction asm.
#pragma once
#include <hip/hip_runtime.h>

namespace dh {

__device__ __forceinline__ float mul_rn(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// the same for doubles (image_metrics.hip: an fp64 formula that a numpy restatement repeats bit for bit)
__device__ __forceinline__ double mul_rn(double a, double b) {
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

}  // namespace dh
