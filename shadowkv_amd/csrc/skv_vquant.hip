// Quantisation pass of the FP8 V offload table: bf16 token rows of 128 values -> 128 OCP e4m3fn
// bytes + one f32 power-of-two scale per token row.
//     amax  = max |v[d]|
//     scale = the smallest power of two with amax / scale <= 448, clamped to [2^-100, 2^100]; amax == 0: 1
//     byte  = e4m3fn(RNE(clamp(f32(v[d]) / scale, -448, 448)))
// 448 = 1.75 * 2^8, so with amax = 1.f * 2^e the exponent of the scale is e - 8 for 1.f <= 1.75 and e - 7 above: integer
// arithmetic on the bits of amax, no log / division.  v / scale is a multiplication by 2^-k: exact (a product below the f32
// normals is far below half the smallest e4m3 subnormal, 2^-10, and becomes 0 either way).
// Mapping: 16 lanes per token row (16 B = 8 values per lane, the amax a 16-lane reduction), 16 token rows per workgroup,
// one launch for every (batch, head, token).  The input is read through element strides (V arrives as a transposed view of
// the fused QKV output); the output rows of a (batch, head) are contiguous: 128 bytes and one scale per token.
#include "../../include/shadowkv_hip.h"
#include "skv_common.h"

#define VQ_D 128
#define VQ_ROWS_PER_WG 16

__global__ __launch_bounds__(256) void skv_quantize_v_rows_kernel(const bf16_t* __restrict__ v, long long stride_b,
                                                                  long long stride_h, long long stride_t, int heads,
                                                                  int tokens, uint8_t* __restrict__ table,
                                                                  long long table_block_stride, float* __restrict__ scale,
                                                                  long long scale_block_stride) {
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int sub = threadIdx.x & 15;
    const long long t = (long long)blockIdx.x * VQ_ROWS_PER_WG + (threadIdx.x >> 4);
    const long long tc = t < tokens ? t : tokens - 1;            // rows past the end: a duplicate, never stored
    const u32x4 w = *reinterpret_cast<const u32x4*>(v + b * stride_b + h * stride_h + tc * stride_t + 8 * sub);
    // |x| of a finite bf16 orders like its 15 low bits
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) am = max(am, max(w[j] & 0x7fffu, (w[j] >> 16) & 0x7fffu));
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, m, 16));
    // am = bf16 bits of amax: exponent field am >> 7, seven mantissa bits (1.75 = 1.1100000b)
    int k = (int)(am >> 7) - 127 - ((am & 0x7fu) <= 0x60u ? 8 : 7);
    k = min(max(k, -100), 100);
    if (am == 0) k = 0;
    const float sc = __uint_as_float((uint32_t)(127 + k) << 23), inv = __uint_as_float((uint32_t)(127 - k) << 23);
    float x[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[2 * j] = fminf(fmaxf(bf_lo(w[j]) * inv, -448.f), 448.f);
        x[2 * j + 1] = fminf(fmaxf(bf_hi(w[j]) * inv, -448.f), 448.f);
    }
    u32x2 o;
#pragma unroll
    for (int j = 0; j < 2; ++j) {                                // v_cvt_pk_fp8_f32: two f32 -> two OCP e4m3fn bytes, RNE
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j], x[4 * j + 1], 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j + 2], x[4 * j + 3], p, true);
        o[j] = (uint32_t)p;
    }
    if (t < tokens) {
        *reinterpret_cast<u32x2*>(table + (long long)bh * table_block_stride + t * VQ_D + 8 * sub) = o;
        if (sub == 0) scale[(long long)bh * scale_block_stride + t] = sc;
    }
}

// every check is made on the host before the launch (bad pointers / strides: SKV_ERR_ARG, other shapes: SKV_ERR_UNSUPPORTED)
int skv_launch_quantize_v_rows(const void* v, long long stride_b, long long stride_h, long long stride_t, int batch_size,
                               int heads, int tokens, int head_dim, void* table, long long table_block_stride, float* scale,
                               long long scale_block_stride, hipStream_t st) {
    if (!v || !table || !scale || batch_size < 1 || heads < 1 || tokens < 1) return SKV_ERR_ARG;
    if (head_dim != VQ_D) return SKV_ERR_UNSUPPORTED;
    if ((stride_b % 8) || (stride_h % 8) || (stride_t % 8) || stride_t < VQ_D || ((uintptr_t)v % 16)) return SKV_ERR_ARG;
    if ((table_block_stride % 8) || table_block_stride < (long long)tokens * VQ_D || ((uintptr_t)table % 8)) return SKV_ERR_ARG;
    if (scale_block_stride < tokens || ((uintptr_t)scale % 4)) return SKV_ERR_ARG;
    if ((long long)batch_size * heads > 65535) return SKV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(skv_quantize_v_rows_kernel, dim3((tokens + VQ_ROWS_PER_WG - 1) / VQ_ROWS_PER_WG, batch_size * heads),
                       dim3(256), 0, st, (const bf16_t*)v, stride_b, stride_h, stride_t, heads, tokens,
                       (uint8_t*)table, table_block_stride, scale, scale_block_stride);
    return SKV_OK;
}
