// FP8 (OCP e4m3fn) codes to values on gfx950, shared by every kernel that reads the codes from HBM (fp8_kernels.hip, fp8_gemm.hip,
// moe_fp8_kernels.hip): the 16-byte piece as 16 floats for the weight-streaming kernels, and eight codes as eight bf16 operands
// for the matrix-core tile loaders.  Both conversions are exact: the hardware decodes, nothing is rounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_split.h"

namespace kjarni {

__device__ __forceinline__ u32x4 load_nt16(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }

// The 16 codes of a piece as floats (code 4 d + e of the piece in w[4 d + e]): v_cvt_pk_f32_fp8, two codes per instruction.
__device__ __forceinline__ void decode16(u32x4 p, float (&w)[16])
{
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)p[d], false);
        const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)p[d], true);
        w[4 * d] = lo[0];
        w[4 * d + 1] = lo[1];
        w[4 * d + 2] = hi[0];
        w[4 * d + 3] = hi[1];
    }
}

// Eight codes (two dwords, code j in byte j) as eight bf16 in the same order: v_cvt_scalef32_pk_bf16_fp8 with scale 1.0, one
// instruction per pair of codes (v_cvt_pk_f32_fp8 and a byte permute to keep the high halves is the same result in twice as many).
// Every e4m3fn value is a bf16 number, so the conversion has nothing to round; the scale operand stays 1.0 -- a matrix's real scale
// is applied in f32 by the kernel.
__device__ __forceinline__ u32x4 fp8x8_to_bf16x8(u32x2 c)
{
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        o[2 * d] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[d], 1.0f, false));     // codes 4d, 4d + 1
        o[2 * d + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[d], 1.0f, true));  // codes 4d + 2, 4d + 3
    }
    return o;
}

}  // namespace kjarni
