// Weight-only FP8 sibling of skv_rows_gemm.hip: the dense projections of a decode step with 2..32 token rows, the weights as OCP
// e4m3fn bytes with one f32 scale per output row,
//     Y[m][n] = scale[n] * sum_k e4m3(W8[n][k]) * X[m][k] (+ bias[n]),   W8 [N][K] bytes row-major, X [M][K], Y [M][N] bf16, M <= 32
// and the gate/up variant (W8 = [gate; up], 2I rows): Y[m][i] = bf16(silu(t_g)) * t_u, each row with its own scale.
// Contract per output: f32 accumulation, the split-K partials summed in wave order, then ONE f32 multiply
// by scale[n]; t then takes exactly the epilogue of skv_linear_rows_bf16.  Activations stay bf16: e4m3 -> bf16 is exact, the
// multiply is v_mfma_f32_16x16x32_bf16.
//
// Tile shapes, the (SILU_PAIR, MT, RT, NWV) family, the reduction, the epilogue and the host's branch tree are skv_rows_frame.h,
// shared with skv_rows_gemm.hip; this file keeps the weight operand's stream.
// A 16-byte load now holds 16 weights, so a k-step is 64 elements and feeds TWO MFMAs:
//     A operand (weights): lane (a = lane & 15, g = lane >> 4) loads 16 B = W8[row a][64 s + 16 g .. +16]  (nontemporal);
//                          bytes 0..7 -> 8 bf16 for the first MFMA, bytes 8..15 for the second (4 + 4 v_cvt_scalef32_pk_bf16_fp8,
//                          scale 1.0: two bytes -> one packed bf16 pair, straight into the operand registers)
//     B operand (tokens) : lane (a, g) reads the 32 bytes X[token min(a, M-1)][64 s + 16 g .. +16] as two 16-byte vectors, the
//                          first for the first MFMA, the second for the second (the k order inside an MFMA is free as long as
//                          both operands agree: lane group g owns k = 16 g .. 16 g + 15 of the step, split 8 | 8)
//     D                  : lane holds D[rows 4 g .. 4 g + 3][token a]
// Per 16 B of weights: 8 conversions and 2 * MT MFMAs.
#include "../../include/shadowkv_hip.h"
#include "skv_rows_frame.h"

#ifndef RG8_WAVES
#define RG8_WAVES 8
#endif
#ifndef RG8_U
#define RG8_U 8
#endif
// RG8_WAVES: waves per 16-row tile (K split);  RG8_U: k-steps (16-B weight loads) in flight per wave of the first generation

// eight e4m3 bytes (two words) -> the 8 bf16 of one MFMA operand, element order = byte order.  gfx950 decodes OCP e4m3fn.
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t w0, uint32_t w1) {
    u32x4 r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
    return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 w, const u32x4& x, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}

// PAIRX (M <= 8): token columns 8..15 of the MFMA are never stored, so their lanes (a >= 8) load the SECOND 16-byte vector of
// token a - 8 (same k-step) and hand it over with one DPP row rotate: one token-operand load serves both MFMAs of a k-step.
// MT = 2 (17 <= M <= 32): two token tiles per weight load, as in skv_rows_gemm_kernel.
template <bool SILU_PAIR, bool PAIRX, int MT, int U>
__global__ __launch_bounds__(RG8_WAVES * 64) void skv_rows_gemm_fp8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                                           const bf16_t* __restrict__ X,
                                                                           const bf16_t* __restrict__ bias, bf16_t* __restrict__ Y,
                                                                           int N, int K, int M, int I /* SILU_PAIR: rows of one half */) {
    static_assert(!(PAIRX && MT > 1), "the paired token operand serves one tile of <= 8 tokens");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = skv_rows_a(lane), g = skv_rows_g(lane);
    const uint8_t* wp = W + skv_rows_weight_row<SILU_PAIR>(blockIdx.x, a, N, I) * K + 16 * g;
    const bf16_t* xp[MT];                                               // batches (PAIRX: lanes a >= 8 at the second vector)
    const bf16_t* xs[MT];                                               // single steps: every lane both vectors of its token
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        xs[t] = X + (size_t)skv_rows_token(t, PAIRX ? (a & 7) : a, M) * K + 16 * g;
        xp[t] = xs[t] + (PAIRX ? (a >> 3) * 8 : 0);
    }
    int s0, s1;
    skv_rows_k_slice<RG8_WAVES>(K / 64, wave, s0, s1);
    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        acc0[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int s = s0;
    for (; s + U <= s1; s += U) {
        u32x4 wv[U], xv[MT][U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wv[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (size_t)(s + u) * 64));
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                xv[t][u][0] = *reinterpret_cast<const u32x4*>(xp[t] + (size_t)(s + u) * 64);
                if (!PAIRX) xv[t][u][1] = *reinterpret_cast<const u32x4*>(xp[t] + (size_t)(s + u) * 64 + 8);
            }
        }
        // every load of the batch is issued before the first conversion: the fence of skv_rows_gemm2_kernel keeps the compiler from
        // sinking a load to its use, the scheduling barrier keeps the machine scheduler from weaving loads into the conversions
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (PAIRX) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    xv[0][u][1][j] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xv[0][u][0][j], 0x128 /*row_ror:8*/, 0xf, 0xf, false);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bf16x8 w0 = e4m3x8_to_bf16(wv[u][0], wv[u][1]), w1 = e4m3x8_to_bf16(wv[u][2], wv[u][3]);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                acc0[t] = mfma_bf16(w0, xv[t][u][0], acc0[t]);
                acc1[t] = mfma_bf16(w1, xv[t][u][1], acc1[t]);
            }
        }
    }
    for (; s < s1; ++s) {
        const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (size_t)s * 64));
        u32x4 xv[MT][2];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            xv[t][0] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64);
            xv[t][1] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64 + 8);
        }
        const bf16x8 w0 = e4m3x8_to_bf16(wv[0], wv[1]), w1 = e4m3x8_to_bf16(wv[2], wv[3]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            acc0[t] = mfma_bf16(w0, xv[t][0], acc0[t]);
            acc1[t] = mfma_bf16(w1, xv[t][1], acc1[t]);
        }
    }
    f32x4 acc[1][MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0][t][r] = acc0[t][r] + acc1[t][r];
    skv_rows_epilogue<SILU_PAIR, true, true, RG8_WAVES>(acc, tid, a, g, scale, bias, Y, N, M, I);
}

// Second generation (skv_rows_gemm2_kernel): a wave walks RT tiles of 16 weight rows over its K slice, so one token-operand load
// (32 bytes here) per k-step serves 2 * RT (x MT) MFMAs.  U k-steps in flight: RT * U weight loads of 1 KB per wave.
template <bool SILU_PAIR, int MT, int RT, int NWV, int U>
__global__ __launch_bounds__(NWV * 64) void skv_rows_gemm2_fp8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                                      const bf16_t* __restrict__ X, const bf16_t* __restrict__ bias,
                                                                      bf16_t* __restrict__ Y, int N, int K, int M,
                                                                      int I /* SILU_PAIR: rows of one half */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = skv_rows_a(lane), g = skv_rows_g(lane);
    const uint8_t* wp[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) wp[r] = W + skv_rows_weight_row<SILU_PAIR>(blockIdx.x * RT + r, a, N, I) * K + 16 * g;
    const bf16_t* xs[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xs[t] = X + (size_t)skv_rows_token(t, a, M) * K + 16 * g;
    int s0, s1;
    skv_rows_k_slice<NWV>(K / 64, wave, s0, s1);
    f32x4 acc[RT][MT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[r][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int s = s0;
    for (; s + U <= s1; s += U) {
        u32x4 wv[RT][U], xv[MT][U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                wv[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)(s + u) * 64));
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                xv[t][u][0] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)(s + u) * 64);
                xv[t][u][1] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)(s + u) * 64 + 8);
            }
        }
        // every load of the batch is issued before the first conversion (fence + scheduling barrier, as in the first generation)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const bf16x8 w = e4m3x8_to_bf16(wv[r][u][2 * h], wv[r][u][2 * h + 1]);
#pragma unroll
                    for (int t = 0; t < MT; ++t) acc[r][t] = mfma_bf16(w, xv[t][u][h], acc[r][t]);
                }
    }
    for (; s < s1; ++s) {
        u32x4 xv[MT][2];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            xv[t][0] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64);
            xv[t][1] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64 + 8);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)s * 64));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bf16x8 w = e4m3x8_to_bf16(wv[2 * h], wv[2 * h + 1]);
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[r][t] = mfma_bf16(w, xv[t][h], acc[r][t]);
            }
        }
    }
    skv_rows_epilogue<SILU_PAIR, true, false, NWV>(acc, tid, a, g, scale, bias, Y, N, M, I);
}

// k-steps in flight per wave (weight loads of 16 B per lane; every k-step adds 2 * MT token loads): 8 with the paired token
// operand, 4 in the other first-generation shapes (two workgroups fit a CU's registers; 8 steps leave room for one), 4 in the
// second generation, 2 in its 4x4 shape (16 loads per step pair).  Like the thresholds of skv_rows_pick for this format:
// chosen from the register counts, not timed.
struct RowsFp8 {
    const uint8_t* W;
    const float* scale;
    const bf16_t *X, *bias;
    bf16_t* Y;
    int M, N, K;
    hipStream_t st;
    template <bool SILU_PAIR, bool PAIRX, int MT>
    void gen1(int grid, int I) const {
        hipLaunchKernelGGL((skv_rows_gemm_fp8_kernel<SILU_PAIR, PAIRX, MT, PAIRX ? RG8_U : 4>), dim3(grid), dim3(RG8_WAVES * 64), 0, st,
                           W, scale, X, bias, Y, N, K, M, I);
    }
    template <bool SILU_PAIR, int MT, int RT, int NWV>
    void gen2(int grid, int I) const {
        hipLaunchKernelGGL((skv_rows_gemm2_fp8_kernel<SILU_PAIR, MT, RT, NWV, RT == 4 ? 2 : 4>), dim3(grid), dim3(NWV * 64), 0, st,
                           W, scale, X, bias, Y, N, K, M, I);
    }
};

extern "C" int skv_linear_rows_fp8(const void* W8, const void* scale, const void* X, const void* bias, void* Y, int M, int N, int K,
                                   int fuse_silu_mul, skv_stream_t stream) {
    // every argument check on the host, before any HIP call
    if (!W8 || !scale || !X || !Y || M < 1 || N < 1) return SKV_ERR_ARG;
    if (fuse_silu_mul && (N % 2 || bias)) return SKV_ERR_ARG;
    if (M > 32 || K % 64 || K < 64) return SKV_ERR_UNSUPPORTED;
    const RowsFp8 l{(const uint8_t*)W8, (const float*)scale, (const bf16_t*)X, (const bf16_t*)bias, (bf16_t*)Y, M, N, K, (hipStream_t)stream};
    return skv_rows_dispatch(l, M, N, K, fuse_silu_mul != 0);
}
