// FP8 (OCP e4m3fn) V offload table: a chunk row is 8 token rows x 128 bytes = 1 KiB, with one f32
// power-of-two scale per token row in a separate HBM tensor.  v'[d] = bf16(scale * f32(e4m3(byte[d]))): the product of an
// e4m3 number and a power of two in [2^-100, 2^100] is a bf16 number, so the conversion below is exact whichever way the
// hardware rounds.
#pragma once
#include "skv_common.h"

// eight e4m3 bytes (two words) of ONE token row -> the 16-byte unit of 8 bf16 the bf16 table would have held there
__device__ __forceinline__ u32x4 skv_e4m3x8_dequant(u32x2 w, float scale) {
    u32x4 r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], scale, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], scale, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], scale, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], scale, true));
    return r;
}
