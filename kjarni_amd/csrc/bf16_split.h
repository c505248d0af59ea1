// An f32 number as three bf16 pieces, exactly (gemm_split.hip's comment has the arithmetic): shared by the kernels that stage f32
// operands for the bf16 matrix cores (gemm_split.hip, fp8_gemm.hip).  Translation units that use it are compiled with
// -fno-slp-vectorize (the Makefile says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_utils.h"

namespace kjarni {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t sp_pack(float a, float b)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2v{a, b}, bf16x2));  // v_cvt_pk_bf16_f32, round to nearest even
}
__device__ __forceinline__ void sp_split(const f32x4 x, u32x2& p1, u32x2& p2, u32x2& p3)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float x0 = x[2 * i], x1 = x[2 * i + 1];
        const uint32_t a = sp_pack(x0, x1);
        const float r0 = x0 - __builtin_bit_cast(float, a << 16), r1 = x1 - __builtin_bit_cast(float, a & 0xffff0000u);
        const uint32_t b = sp_pack(r0, r1);
        const float s0 = r0 - __builtin_bit_cast(float, b << 16), s1 = r1 - __builtin_bit_cast(float, b & 0xffff0000u);
        p1[i] = a;
        p2[i] = b;
        p3[i] = sp_pack(s0, s1);
    }
}

}  // namespace kjarni
