// Weight-only MXFP4 sibling of skv_rows_gemm_fp8.hip: the dense projections of a decode step with 2..32 token rows, the weights as
// OCP MX e2m1 nibbles with one e8m0 scale byte per 32 consecutive elements of a row (the format of skv_gemv_mxfp4.hip),
//     Y[m][n] = sum_k 2^(scale[n][k / 32] - 127) * e2m1(nibble[n][k]) * X[m][k] (+ bias[n]),
//     W4 [N][K / 2] bytes row-major, element 2i in the low nibble of byte i;  scale [N][K / 32] bytes;  X [M][K], Y [M][N] bf16, M <= 32
// and the gate/up variant (W4 = [gate; up], 2I rows): Y[m][i] = bf16(silu(t_g)) * t_u.
// Contract per output: the block scale is applied to the WEIGHT - 2^s * e2m1 has two significant bits and
// is a normal bf16 number for scale bytes 27..227, so the converted operand is exact - f32 accumulation (MFMA, the kernel's
// accumulators, the split-K partials in wave order), NO multiply after the reduction; t then takes exactly the epilogue of
// skv_linear_rows_bf16.  Activations stay bf16, the multiply is v_mfma_f32_16x16x32_bf16.
//
// Tile shapes, the (SILU_PAIR, MT, RT, NWV) family, the reduction, the epilogue and the host's branch tree are skv_rows_frame.h,
// shared with skv_rows_gemm.hip and skv_rows_gemm_fp8.hip; this file keeps the weight operand's stream.
// A 16-byte load holds 32 weights = exactly one MX block, so a k-step is 128 elements and feeds FOUR MFMAs:
//     A operand (weights): lane (a = lane & 15, g = lane >> 4) loads 16 B = W4[row a][64 s + 16 g .. +16]  (nontemporal) and ONE
//                          scale byte scale[row a][4 s + g] (a byte load: one shift to the f32 2^s; taking byte g of the row's
//                          aligned dword compiled to a per-lane shift + mask more per k-step and 1-2 more VGPRs per instance);
//                          dword j of the load -> the 8 bf16 of MFMA j (4 v_cvt_scalef32_pk_bf16_fp4, byte_sel 0..3: one byte =
//                          two nibbles -> one packed bf16 pair, low nibble first, straight into the operand registers)
//     B operand (tokens) : lane (a, g) reads the 64 bytes X[token min(a, M-1)][128 s + 32 g .. +32] as four 16-byte vectors, vector
//                          j for MFMA j (the k order inside an MFMA is free as long as both operands agree: lane group g owns
//                          k = 32 g .. 32 g + 31 of the step, split 8 | 8 | 8 | 8)
//     D                  : lane holds D[rows 4 g .. 4 g + 3][token a]
// Per 16 B of weights: 16 conversions and 4 * MT MFMAs, and 64 B of x per token tile (bf16 weights: 16 B, FP8: 32 B).
#include "../../include/shadowkv_hip.h"
#include "skv_rows_frame.h"

#ifndef RG4_WAVES
#define RG4_WAVES 8
#endif
// RG4_WAVES: waves per 16-row tile of the first generation (K split)

// the f32 2^(byte - 127) of an e8m0 scale byte (bytes 1..254; the contract is 27..227)
__device__ __forceinline__ float rows_e8m0_f32(uint32_t byte) { return __uint_as_float(byte << 23); }
// one word = eight e2m1 nibbles -> the 8 bf16 of one MFMA operand, each times `scale`; element order = nibble order
__device__ __forceinline__ bf16x8 e2m1x8_to_bf16(uint32_t w, float scale) {
    u32x4 r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
    return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 w, const u32x4& x, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}

// PAIRX (M <= 8): token columns 8..15 of the MFMA are never stored, so their lanes (a >= 8) load vectors 2, 3 of token a - 8
// (same k-step) and hand them over with DPP row rotates: two token-operand loads per k-step instead of four.
// MT = 2 (17 <= M <= 32): two token tiles per weight load, as in skv_rows_gemm_kernel.
// Two accumulators per token tile: MFMAs 0, 2 of a k-step go to the first, 1, 3 to the second.
template <bool SILU_PAIR, bool PAIRX, int MT, int U>
__global__ __launch_bounds__(RG4_WAVES * 64) void skv_rows_gemm_mxfp4_kernel(const uint8_t* __restrict__ W, const uint8_t* __restrict__ scale,
                                                                             const bf16_t* __restrict__ X,
                                                                             const bf16_t* __restrict__ bias, bf16_t* __restrict__ Y,
                                                                             int N, int K, int M, int I /* SILU_PAIR: rows of one half */) {
    static_assert(!(PAIRX && MT > 1), "the paired token operand serves one tile of <= 8 tokens");
    constexpr int XL = PAIRX ? 2 : 4;                                   // 16-byte token vectors a lane loads per k-step and tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = skv_rows_a(lane), g = skv_rows_g(lane);
    const size_t row = skv_rows_weight_row<SILU_PAIR>(blockIdx.x, a, N, I);
    const uint8_t* wp = W + row * (K / 2) + 16 * g;                     // a k-step is 64 bytes of a row's nibbles
    const uint8_t* sp = scale + row * (K / 32) + g;                     // and 4 scale bytes, one per lane group
    const bf16_t* xp[MT];                                               // batches (PAIRX: lanes a >= 8 at vectors 2, 3)
    const bf16_t* xs[MT];                                               // single steps: every lane all four vectors of its token
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        xs[t] = X + (size_t)skv_rows_token(t, PAIRX ? (a & 7) : a, M) * K + 32 * g;
        xp[t] = xs[t] + (PAIRX ? (a >> 3) * 16 : 0);
    }
    int s0, s1;
    skv_rows_k_slice<RG4_WAVES>(K / 128, wave, s0, s1);
    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        acc0[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int s = s0;
    for (; s + U <= s1; s += U) {
        u32x4 wv[U], xv[MT][U][4];
        uint32_t sv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wv[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (size_t)(s + u) * 64));
            sv[u] = sp[(size_t)(s + u) * 4];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int j = 0; j < XL; ++j) xv[t][u][j] = *reinterpret_cast<const u32x4*>(xp[t] + (size_t)(s + u) * 128 + 8 * j);
        }
        // every load of the batch is issued before the first conversion: the fence keeps the compiler from sinking a load to its
        // use, the scheduling barrier keeps the machine scheduler from weaving loads into the conversions
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (PAIRX) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        xv[0][u][2 + h][j] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xv[0][u][h][j], 0x128 /*row_ror:8*/, 0xf, 0xf, false);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float sc = rows_e8m0_f32(sv[u]);
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
                const bf16x8 w0 = e2m1x8_to_bf16(wv[u][j], sc), w1 = e2m1x8_to_bf16(wv[u][j + 1], sc);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    acc0[t] = mfma_bf16(w0, xv[t][u][j], acc0[t]);
                    acc1[t] = mfma_bf16(w1, xv[t][u][j + 1], acc1[t]);
                }
            }
        }
    }
    for (; s < s1; ++s) {
        const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (size_t)s * 64));
        const float sc = rows_e8m0_f32(sp[(size_t)s * 4]);
        u32x4 xv[MT][4];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[t][j] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 128 + 8 * j);
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const bf16x8 w0 = e2m1x8_to_bf16(wv[j], sc), w1 = e2m1x8_to_bf16(wv[j + 1], sc);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                acc0[t] = mfma_bf16(w0, xv[t][j], acc0[t]);
                acc1[t] = mfma_bf16(w1, xv[t][j + 1], acc1[t]);
            }
        }
    }
    f32x4 acc[1][MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0][t][r] = acc0[t][r] + acc1[t][r];
    skv_rows_epilogue<SILU_PAIR, false, true, RG4_WAVES>(acc, tid, a, g, nullptr, bias, Y, N, M, I);
}

// Second generation (skv_rows_gemm2_kernel): a wave walks RT tiles of 16 weight rows over its K slice, so one token-operand load
// (64 bytes here) per k-step serves 4 * RT (x MT) MFMAs.  U k-steps in flight: RT * U weight loads of 1 KB per wave.
template <bool SILU_PAIR, int MT, int RT, int NWV, int U>
__global__ __launch_bounds__(NWV * 64) void skv_rows_gemm2_mxfp4_kernel(const uint8_t* __restrict__ W, const uint8_t* __restrict__ scale,
                                                                        const bf16_t* __restrict__ X, const bf16_t* __restrict__ bias,
                                                                        bf16_t* __restrict__ Y, int N, int K, int M,
                                                                        int I /* SILU_PAIR: rows of one half */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = skv_rows_a(lane), g = skv_rows_g(lane);
    const uint8_t *wp[RT], *sp[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const size_t row = skv_rows_weight_row<SILU_PAIR>(blockIdx.x * RT + r, a, N, I);
        wp[r] = W + row * (K / 2) + 16 * g;
        sp[r] = scale + row * (K / 32) + g;
    }
    const bf16_t* xs[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xs[t] = X + (size_t)skv_rows_token(t, a, M) * K + 32 * g;
    int s0, s1;
    skv_rows_k_slice<NWV>(K / 128, wave, s0, s1);
    f32x4 acc[RT][MT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[r][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int s = s0;
    for (; s + U <= s1; s += U) {
        u32x4 wv[RT][U], xv[MT][U][4];
        uint32_t sv[RT][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                wv[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)(s + u) * 64));
                sv[r][u] = sp[r][(size_t)(s + u) * 4];
            }
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[t][u][j] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)(s + u) * 128 + 8 * j);
        }
        // every load of the batch is issued before the first conversion (fence + scheduling barrier, as in the first generation)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const bf16x8 w = e2m1x8_to_bf16(wv[r][u][j], rows_e8m0_f32(sv[r][u]));
#pragma unroll
                    for (int t = 0; t < MT; ++t) acc[r][t] = mfma_bf16(w, xv[t][u][j], acc[r][t]);
                }
    }
    for (; s < s1; ++s) {
        u32x4 xv[MT][4];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[t][j] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 128 + 8 * j);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)s * 64));
            const float sc = rows_e8m0_f32(sp[r][(size_t)s * 4]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x8 w = e2m1x8_to_bf16(wv[j], sc);
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[r][t] = mfma_bf16(w, xv[t][j], acc[r][t]);
            }
        }
    }
    skv_rows_epilogue<SILU_PAIR, false, false, NWV>(acc, tid, a, g, nullptr, bias, Y, N, M, I);
}

// k-steps in flight per wave.  A k-step holds 4 (weights) + 1 (scale) VGPRs per row tile and 16 * MT of x (8 with the paired
// token operand), against FP8's 4 + 8 * MT: 4 steps in the first generation's one-tile shapes (the same 4 KB of weights per wave
// as FP8's; at K = 4096 a wave's slice is 4 k-steps, so more would never form a batch), 2 with two token tiles and in every
// second-generation shape.  Chosen from the register counts, not timed.
struct RowsMxfp4 {
    const uint8_t *W, *scale;
    const bf16_t *X, *bias;
    bf16_t* Y;
    int M, N, K;
    hipStream_t st;
    template <bool SILU_PAIR, bool PAIRX, int MT>
    void gen1(int grid, int I) const {
        hipLaunchKernelGGL((skv_rows_gemm_mxfp4_kernel<SILU_PAIR, PAIRX, MT, MT == 1 ? 4 : 2>), dim3(grid), dim3(RG4_WAVES * 64), 0, st,
                           W, scale, X, bias, Y, N, K, M, I);
    }
    template <bool SILU_PAIR, int MT, int RT, int NWV>
    void gen2(int grid, int I) const {
        hipLaunchKernelGGL((skv_rows_gemm2_mxfp4_kernel<SILU_PAIR, MT, RT, NWV, 2>), dim3(grid), dim3(NWV * 64), 0, st,
                           W, scale, X, bias, Y, N, K, M, I);
    }
};

extern "C" int skv_linear_rows_mxfp4(const void* W4, const void* scale_e8m0, const void* X, const void* bias, void* Y, int M, int N,
                                     int K, int fuse_silu_mul, skv_stream_t stream) {
    // every argument check on the host, before any HIP call
    if (!W4 || !scale_e8m0 || !X || !Y || M < 1 || N < 1) return SKV_ERR_ARG;
    if (fuse_silu_mul && (N % 2 || bias)) return SKV_ERR_ARG;
    if (M > 32 || K % 128 || K < 128) return SKV_ERR_UNSUPPORTED;
    const RowsMxfp4 l{(const uint8_t*)W4, (const uint8_t*)scale_e8m0, (const bf16_t*)X, (const bf16_t*)bias, (bf16_t*)Y, M, N, K,
                      (hipStream_t)stream};
    return skv_rows_dispatch(l, M, N, K, fuse_silu_mul != 0);
}
